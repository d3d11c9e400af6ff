"""Shared drivers of tests/test_clone_state_emu.py (CPU stand-in) and tests/test_clone_state_gpu.py: the carried state of a stream through
smst_clone -- a split handle with a block in flight and two frequency-map table rows in use, unattached (Batch::copyStateFrom) and as a
pool member (Batch::moveStreamFrom) -- and through the debug setters and getters of a batch.  Small geometry throughout (block 512,
interval 128, stereo); every comparison is EXACT."""
import numpy as np
import pytest

from conftest import package, synth_input

SR = 48000
RATIO = 2.6  # beyond 2x: the random engine draws, inside the block in flight too
WARM = (150, 187, 224, 261)  # input samples of the calls before the clone: short, so a block is in flight between them
AFTER = (261, 150, 224, 187)  # ... and of the calls the original and the clone continue with


def _table(points, slope):
    f = (np.arange(points) + 0.5)/(2*points)
    return (f*slope + 0.02*np.sin(40*f)).astype(np.float32)


def _split_handle(lib, seed):
    o = package().SignalsmithStretch(seed=seed, lib=lib)
    o.configure(2, 512, 128, True)
    o.setFreqMapTable(_table(64, 1.25))
    o.setFormantSemitones(2, True)
    return o


def _call(o, x, n_out):
    """process() in the form that every handle takes: a pool member's request runs with wait()"""
    o.processAsync(x, n_out)
    return o.wait().copy()


def _same(a, b, what):
    assert a.shape == b.shape and np.isfinite(a).all(), what
    assert np.array_equal(a, b), "%s: %d samples differ, worst %g" % (what, int((a != b).sum()), float(np.abs(a - b).max()))


def case_split_clone(lib, pooled):
    """The original (`a`, a pool member when `pooled`), a same-seed twin that never meets a pool and is never cloned, and -- pooled only -- a
    second unattached twin `u` whose clone is what the member's clone is compared with."""
    pkg = package()
    seed = 21
    x = synth_input(seed, 2, 4000, SR) + 0.4*synth_input(2, 2, 4000, SR)
    other = np.ascontiguousarray(synth_input(7, 2, 600, SR))
    handles = [_split_handle(lib, seed) for _ in range(3 if pooled else 2)]
    a, twin = handles[0], handles[1]
    pool = None
    if pooled:
        pool = pkg.StretchPool(lib=lib)
        pool.add(a)
    pos = 0

    def step(n_in, what):
        nonlocal pos
        chunk = np.ascontiguousarray(x[:, pos:pos + n_in])
        pos += n_in
        ys = [_call(o, chunk, int(n_in*RATIO)) for o in live]
        for y in ys[1:]:
            _same(ys[0], y, what)
        return ys[0]

    live = list(handles)
    for k, n_in in enumerate(WARM):
        step(n_in, "before the clone, call %d" % k)
    for o in live:  # mid-interval: the block in flight keeps the row its steps have read, the new table takes another
        o.setFreqMapTable(_table(160, 1.1))
    clones = [a.clone()] + ([handles[2].clone()] if pooled else [])
    if pooled:
        assert lib.smst_pool_detach(clones[0].h) != 0 and b"not attached" in lib.smst_last_error()  # a member's clone is unattached
    live = handles + clones
    loud = 0.0
    for k, n_in in enumerate(AFTER):
        loud = max(loud, float(np.abs(step(n_in, "after the clone, call %d" % k)).max()))
        steps = [lib.smst_block_steps(o.h) for o in live]
        assert steps == [steps[0]]*len(live) and steps[0] > 0, steps
    assert loud > 1e-3, "silence only"
    flushed = [o.flush(300).copy() for o in live]
    for y in flushed[1:]:
        _same(flushed[0], y, "flush")
    # the clone goes its own way without disturbing the original
    for k in range(2):
        _call(clones[0], other[:, 300*k:300*(k + 1)], 500)
    live = [a, twin]
    step(200, "the original after its clone went its own way")
    if pool is not None:
        pool.close()
    for o in handles + clones:
        o.close()


def case_debug_round_trip(lib, half_state):
    """debug_set_state(debug_state()) and debug_set_carry(debug_carry()) change nothing, in fp16 storage either: the stored values are
    representable, and the energy (stored as its square root) squares and un-squares exactly."""
    pkg = package()
    S, Cn, n = 3, 2, 1500
    x = np.stack([synth_input(s, Cn, 3*n, SR) for s in range(S)])
    batches = [pkg.StretchBatch(S, Cn, block=512, interval=128, split=False, lib=lib, seed=5, half_state=half_state) for _ in range(2)]
    b, twin = batches
    for o in batches:
        for k in range(2):
            o.process(x[:, :, k*n:(k + 1)*n], int(n*1.3))

    def snapshot():
        planes = [b.debug_state(s, w).tobytes() for s in range(S) for w in range(4)]
        carries = [part.tobytes() for s in range(S) for part in b.debug_carry(s)]
        return planes + carries

    before = snapshot()
    assert any(np.frombuffer(p, np.float32).any() for p in before)
    for which in range(4):
        b.debug_set_state(1, which, b.debug_state(1, which))
        assert snapshot() == before, which
    b.debug_set_carry(1, *b.debug_carry(1))
    assert snapshot() == before
    y, want = (o.process(x[:, :, 2*n:3*n], int(n*1.3)) for o in batches)
    _same(np.asarray(y), np.asarray(want), "the call after the round trip")
    assert float(np.abs(np.asarray(want)).max()) > 1e-3
    for o in batches:
        o.close()


def case_debug_ranges(lib):
    """An out-of-range stream or selector raises, in the getters as in the setters."""
    pkg = package()
    S, Cn = 3, 2
    b = pkg.StretchBatch(S, Cn, block=512, interval=128, split=False, lib=lib)
    plane, energy = b.debug_state(0, 0), b.debug_state(0, 3)
    sums, products = b.debug_carry(0)
    for stream in (-1, S):
        with pytest.raises(pkg.StretchError):
            b.debug_state(stream, 0)
        with pytest.raises(pkg.StretchError):
            b.debug_set_state(stream, 0, plane)
        with pytest.raises(pkg.StretchError):
            b.debug_carry(stream)
        with pytest.raises(pkg.StretchError):
            b.debug_set_carry(stream, sums, products)
    for which in (-1, 4):
        with pytest.raises(pkg.StretchError):
            b.debug_state(0, which)
        with pytest.raises(pkg.StretchError):
            b.debug_set_state(0, which, plane)
    b.debug_set_state(S - 1, 3, energy)  # the last valid ones pass
    assert b.debug_state(S - 1, 3).shape == energy.shape
    b.close()
