"""Shared drivers of tests/test_pool_emu.py (CPU stand-in, small geometries) and tests/test_pool_gpu.py (presets at 48 kHz): single-stream
objects in a StretchPool against same-seed unattached twins.  Every comparison is EXACT: the thing compared with is the unpooled handle,
which is the behaviour the parity suite pins to the reference."""
import ctypes as C

import numpy as np

from conftest import package, synth_input

LAUNCH_NAMES = ("vocoder_aligned", "vocoder_staged", "vocoder_gather", "vocoder_n", "vocoder_one", "vocoder_across", "chain_unfused",
                "analyse_teams", "analyse_fast", "analyse_generic", "synth_teams", "synth_fast", "synth_generic")  # include/smst.h, smst_debug_launch_count
_fp = C.POINTER(C.c_float)


def launch_counts(lib):
    pkg = package()
    return np.array([pkg.launch_count(n, lib=lib) for n in LAUNCH_NAMES], np.int64)


class Pair:
    """A member candidate and its twin: same seed, same configuration, same calls.  `obj` meets a pool, `twin` never does."""

    def __init__(self, lib, seed, configure, setup=None, sr=48000):
        pkg = package()
        self.lib, self.sr, self.seed = lib, sr, seed
        self.obj = pkg.SignalsmithStretch(seed=seed, lib=lib)
        self.twin = pkg.SignalsmithStretch(seed=seed, lib=lib)
        for o in (self.obj, self.twin):
            configure(o)
            if setup:
                setup(o)
        self.pos = 0
        self.got, self.want = [], []
        self.silent = ()

    def signal(self, n, round_index):
        x = synth_input(self.seed, self.obj.channels, self.pos + n, self.sr)[:, self.pos:self.pos + n]
        if round_index in self.silent:
            x = np.zeros_like(x)
        self.pos += n
        return np.ascontiguousarray(x, np.float32)

    def begin(self, n_in, n_out, round_index=-1):
        x = self.signal(n_in, round_index)
        self.obj.processAsync(x, n_out)
        self.want.append(self.twin.process(x, n_out).copy())

    def end(self):
        self.got.append(self.obj.wait().copy())

    def both(self, f):
        return f(self.obj), f(self.twin)

    def check(self, what=""):
        assert len(self.got) == len(self.want) and self.got
        for k, (a, b) in enumerate(zip(self.got, self.want)):
            assert a.shape == b.shape
            if a.size:
                assert np.isfinite(b).all()
            assert np.array_equal(a, b), "%s seed %d call %d: %d samples differ, worst %g" % (
                what, self.seed, k, int((a != b).sum()), float(np.abs(a - b).max()))
        assert any(np.abs(b).max() > 1e-4 for b in self.want if b.size), "%s seed %d: the twin produced silence only" % (what, self.seed)

    def close(self):
        self.obj.close()
        self.twin.close()


def raw_begin(lib, stretch, x, n_out):
    """smst_process_begin with buffers the CALLER keeps (two requests of one object can then be alive at once) -> (rc, keepalive, out)"""
    a = np.ascontiguousarray(np.asarray(x, np.float32).reshape(stretch.channels, -1))
    out = np.zeros((stretch.channels, max(n_out, 1)), np.float32)
    pi, po = stretch._planes(a), stretch._planes(out)
    rc = lib.smst_process_begin(stretch.h, pi, a.shape[1], po, n_out)
    return rc, (a, pi, po), out[:, :n_out]


def one_submission(lib, make_pair_configure, batch_kwargs, n_in, n_out, sr=48000):
    """Issue test 4: a run of 8 members whose group holds exactly 8 slots launches what ONE smst_batch_process of an 8-stream batch with
    the same counts launches, and strictly less than 8 single-handle calls do."""
    pkg = package()
    N = 8
    pairs = [Pair(lib, 40 + s, make_pair_configure, sr=sr) for s in range(N)]
    pool = pkg.StretchPool(lib=lib)
    for p in pairs:
        pool.add(p.obj)
    xs = [p.signal(n_in, -1) for p in pairs]
    calls0 = pool.engine_calls()
    for p, x in zip(pairs, xs):
        p.obj.processAsync(x, n_out)
    before = launch_counts(lib)
    pool.run()
    pooled = launch_counts(lib) - before
    assert pool.engine_calls() == calls0 + 1
    got = [p.obj.wait().copy() for p in pairs]

    batch = pkg.StretchBatch(N, pairs[0].obj.channels, lib=lib, seed=40, **batch_kwargs)
    before = launch_counts(lib)
    yb = batch.process(np.stack(xs), n_out)
    one_batch = launch_counts(lib) - before
    batch.close()

    before = launch_counts(lib)
    want = [p.twin.process(x, n_out).copy() for p, x in zip(pairs, xs)]
    singles = launch_counts(lib) - before

    assert pooled.sum() > 0
    assert np.array_equal(pooled, one_batch), dict(zip(LAUNCH_NAMES, zip(pooled.tolist(), one_batch.tolist())))
    assert pooled.sum() < singles.sum(), (pooled.tolist(), singles.tolist())
    for s in range(N):
        assert np.array_equal(got[s], want[s]), s
        assert np.array_equal(got[s], yb[s][:, :n_out]), s  # (stream s of a batch seeded 40 is the instance of seed 40 + s)
    pool.close()
    for p in pairs:
        p.close()
