"""The pool extension (include/smst.h group 3) on the GPU, at the presets: 16 single-stream objects in a StretchPool, one-second calls,
against same-seed unattached twins (exact comparisons), and a 4-channel geometry so that the kVocoderN state rows are moved too."""
import numpy as np
import pytest

from conftest import package
from pool_cases import Pair, one_submission

SR = 48000
PRESETS = {
    "default": (lambda o: o.presetDefault(2, SR), dict(preset="default", sample_rate=SR)),
    "cheaper": (lambda o: o.presetCheaper(2, SR), dict(preset="cheaper", sample_rate=SR)),  # split computation: a block is in flight between calls
}


def _table(o):
    f = (np.arange(256) + 0.5)/512
    o.setFreqMapTable((f*1.2 + 0.01*np.sin(60*f)).astype(np.float32))


SETUPS = [None, lambda o: o.setTransposeSemitones(4, 0.2), _table, lambda o: o.setFormantSemitones(2, True)]
RATIOS = [3.0, 1.0, 1.5, 2.5, 0.75, 1.25, 2.2, 1.0]  # output / input; several beyond 2x (seeded random time factors)


def _pairs(lib, configure, n, first_seed):
    return [Pair(lib, first_seed + s, configure, SETUPS[s % len(SETUPS)], sr=SR) for s in range(n)]


def _counts(s, r):
    n_out = SR + 480*((s + r) % 5)  # about one second of output per call, ragged
    return max(1, int(n_out/RATIOS[s % len(RATIOS)])), n_out


@pytest.mark.gpu
@pytest.mark.parametrize("preset", sorted(PRESETS))
def test_pooled_equals_standalone(hip, preset):
    pkg = package()
    pairs = _pairs(hip, PRESETS[preset][0], 16, 300)
    pairs[5].silent = (2, 3)
    pool = pkg.StretchPool(lib=hip)
    for p in pairs:
        pool.add(p.obj)
    for r in range(6):
        on = [(s, p) for s, p in enumerate(pairs) if not (r == 2 and s == 1) and not (r == 4 and s in (7, 8))]  # some sit a round out
        for s, p in on:
            n_in, n_out = _counts(s, r)
            p.begin(n_in, 0 if (r == 3 and s == 2) else n_out, r)
        calls = pool.engine_calls()
        pool.run()
        assert pool.engine_calls() == calls + 1  # one geometry: one engine call
        for s, p in on:
            p.end()
    for p in pairs:
        p.check("pooled " + preset)
    pool.close()
    for p in pairs:
        p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("preset", sorted(PRESETS))
def test_attach_detach_regrowth_and_pool_destruction_mid_stream(hip, preset):
    pkg = package()
    pairs = _pairs(hip, PRESETS[preset][0], 16, 400)
    pool = pkg.StretchPool(lib=hip)
    attached = 0
    for r in range(8):
        if r < 6:  # 3, 6, 9, 12, 15, 16 members: the group regrows at 5 and at 9 (4 -> 8 -> 16 slots)
            for p in pairs[attached:min(16, attached + 3)]:
                pool.add(p.obj)
            attached = min(16, attached + 3)
        if r == 6:
            pool.remove(pairs[2].obj)
            pool.remove(pairs[9].obj)
            pool.add(pairs[2].obj)
            assert pool.members() == 15
        if r == 7:
            pool.close()  # the members finish unattached
        for s, p in enumerate(pairs):
            n_in, n_out = _counts(s, r)
            p.begin(n_in//3, n_out//3 + 7*(r % 2), r)  # a third of a second: blocks are in flight when the slots move
        if r < 7:
            pool.run()
        for p in pairs:
            p.end()
    for p in pairs:
        p.check("mid-stream " + preset)
        p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("preset", sorted(PRESETS))
def test_one_submission(hip, preset):
    configure, batch_kwargs = PRESETS[preset]
    one_submission(hip, configure, batch_kwargs, SR, int(SR*1.5), sr=SR)


@pytest.mark.gpu
def test_four_channels_pooled_and_moved(hip):
    """3-8 channels take kVocoderN: its carried rows ([S][C][M] with C = 4) move between engines like the stereo ones."""
    pkg = package()
    pairs = _pairs(hip, lambda o: o.configure(4, 4096, 1024), 6, 500)
    pool = pkg.StretchPool(lib=hip)
    for r in range(6):
        if r < 3:  # 2, 4, 6 members: one regrowth
            for p in pairs[2*r:2*r + 2]:
                pool.add(p.obj)
        if r == 4:
            pool.remove(pairs[0].obj)
        for s, p in enumerate(pairs):
            n_in, n_out = _counts(s, r)
            p.begin(n_in//2, n_out//2, r)
        before = hip.smst_debug_launch_count(b"vocoder_n")
        pool.run()
        assert hip.smst_debug_launch_count(b"vocoder_n") > before
        for p in pairs:
            p.end()
    for p in pairs:
        p.check("four channels")
    pool.close()
    for p in pairs:
        p.close()
    if hip.smst_device_count() > 1:  # a handle on another device is refused
        far = pkg.SignalsmithStretch(seed=1, device=1, lib=hip)
        pool = pkg.StretchPool(lib=hip)
        assert hip.smst_pool_attach(pool.h, far.h) == -1 and b"another device" in hip.smst_last_error()
        pool.close()
        far.close()
