"""The pool extension (include/smst.h group 3) on the CPU stand-in: single-stream objects attached to a StretchPool, driven through
smst_process_begin / smst_process_end, against same-seed unattached twins driven through smst_process.  Exact comparisons throughout."""
import ctypes as C

import numpy as np

from conftest import package
from pool_cases import Pair, one_submission, raw_begin

STEREO = lambda o: o.configure(2, 512, 128)                 # noqa: E731
MONO_SPLIT = lambda o: o.configure(1, 1024, 256, True)      # noqa: E731
STEREO_SPLIT = lambda o: o.configure(2, 512, 128, True)     # noqa: E731


def _table(o):
    f = (np.arange(64) + 0.5)/128
    o.setFreqMapTable((f*1.25 + 0.02*np.sin(40*f)).astype(np.float32))


def test_pooled_equals_standalone(emu):
    pkg = package()
    pairs = [
        Pair(emu, 11, STEREO),                                             # stretched beyond 2x: seeded random time factors
        Pair(emu, 12, STEREO, lambda o: o.setTransposeSemitones(4, 0.2)),   # transposed with a tonality limit
        Pair(emu, 13, STEREO, _table),                                     # a frequency-map table of its own
        Pair(emu, 14, MONO_SPLIT),                                         # exact silence for part of its input
        Pair(emu, 15, MONO_SPLIT, lambda o: o.setFormantSemitones(2, True)),  # beyond 2x in the split geometry (a block in flight draws when it runs)
    ]
    pairs[3].silent = (2, 3)
    pool = pkg.StretchPool(lib=emu)
    for p in pairs:
        pool.add(p.obj)
    assert pool.members() == 5
    # (nIn, nOut) per round and member; None: the member sits the round out
    rounds = [
        [(300, 900), (700, 700), (640, 800), (1500, 1500), (400, 1000)],
        [(250, 800), (333, 400), (512, 512), (900, 1100), (350, 900)],
        [(310, 950), None, (200, 300), (2500, 2500), (512, 1290)],
        [(128, 400), (1000, 900), (200, 0), (2600, 2600), (300, 777)],
        [(290, 870), (450, 500), (640, 640), None, None],
        [(300, 901), (700, 640), (100, 131), (1200, 1500), (400, 1001)],
    ]
    for r, counts in enumerate(rounds):
        on = [(p, c) for p, c in zip(pairs, counts) if c is not None]
        for p, (n_in, n_out) in on:
            p.begin(n_in, n_out, r)
        assert pool.pending() == len(on)
        groups = len({p.obj.blockSamples() for p, _ in on})
        calls = pool.engine_calls()
        pool.run()
        assert pool.engine_calls() == calls + groups, (r, calls, pool.engine_calls(), groups)
        assert pool.pending() == 0
        for p, _ in on:
            p.end()
        assert pool.engine_calls() == calls + groups  # wait() after a run finds nothing pending
    for p in pairs:
        p.check("pooled")
        assert p.obj.lib.smst_block_steps(p.obj.h) == p.twin.lib.smst_block_steps(p.twin.h)
    pool.close()
    for p in pairs:
        p.close()


def test_attach_detach_regrowth_and_pool_destruction_mid_stream(emu):
    pkg = package()
    setups = [None, lambda o: o.setTransposeSemitones(-3, 0.3), None, _table, lambda o: o.setFormantSemitones(3), None,
              lambda o: o.setTransposeFactor(1.2), None, None]
    pairs = [Pair(emu, 100 + s, STEREO_SPLIT, setups[s]) for s in range(9)]
    pool = pkg.StretchPool(lib=emu)
    ratios = [3.0, 1.0, 2.6, 1.3, 1.1, 0.8, 1.5, 3.2, 1.0]  # several beyond 2x
    for r in range(12):
        if r < 9:
            before = pool.allocation_events()
            pool.add(pairs[r].obj)  # one more member between two rounds; the 5th and the 9th make the group regrow (4 -> 8 -> 16 slots)
            assert pool.allocation_events() > before
        if r == 9:
            pool.remove(pairs[1].obj)
            pool.remove(pairs[3].obj)
            assert pool.members() == 7
        if r == 10:
            pool.add(pairs[1].obj)  # takes a freed slot
            assert pool.members() == 8
        if r == 11:
            pool.close()  # destroyed in the middle of the stream: the members finish unattached
        for s, p in enumerate(pairs):
            n_in = 150 + 37*((s + r) % 4)  # short calls: blocks are in flight when the slots move
            p.begin(n_in, int(n_in*ratios[s]) + (r % 3), r)
        if r < 11:
            pool.run()
        for p in pairs:
            p.end()
    for p in pairs:
        p.check("mid-stream")
        p.close()


def test_program_order(emu):
    pkg = package()
    pool = pkg.StretchPool(lib=emu)
    by = Pair(emu, 70, STEREO_SPLIT)  # a bystander with requests of its own
    a = Pair(emu, 71, STEREO_SPLIT)
    b = Pair(emu, 72, STEREO_SPLIT)
    c = Pair(emu, 73, STEREO_SPLIT)
    d = Pair(emu, 74, STEREO_SPLIT)
    for p in (by, a, b, c, d):
        pool.add(p.obj)
    # a setter between begin and end: the request runs with the OLD value, as the twin's synchronous call did
    by.begin(300, 400)
    a.begin(300, 450)
    a.both(lambda o: o.setTransposeSemitones(5, 0.25))
    assert pool.pending() == 0  # the setter ran the pool
    a.end()
    by.end()
    a.begin(280, 420)
    a.end()
    # a second begin without an end
    x0, x1 = b.signal(200, -1), b.signal(260, -1)
    rc0, keep0, out0 = raw_begin(emu, b.obj, x0, 300)
    assert rc0 == 0 and pool.pending() == 1
    rc1, keep1, out1 = raw_begin(emu, b.obj, x1, 700)
    assert rc1 == 0 and pool.pending() == 1  # the first one ran
    assert emu.smst_process_end(b.obj.h) == 0
    b.got += [out0.copy(), out1.copy()]
    b.want += [b.twin.process(x0, 300).copy(), b.twin.process(x1, 700).copy()]
    # flush and reset with a request pending
    c.begin(400, 500)
    f_obj, f_twin = c.both(lambda o: o.flush(200, 1.0).copy())
    assert pool.pending() == 0
    c.end()
    c.got.append(f_obj)
    c.want.append(f_twin)
    c.begin(300, 380)
    c.both(lambda o: o.reset())
    c.end()
    for _ in range(2):
        c.begin(350, 900)
        c.end()
    # seek / outputSeek / exact on a member
    x = d.signal(1200, -1)
    d.both(lambda o: o.seek(x[:, :600], 0.8))
    d.begin(300, 400)
    d.end()
    d.both(lambda o: o.outputSeek(x[:, :o.outputSeekLength(1.0)]))
    d.begin(300, 300)
    d.end()
    e_obj, e_twin = d.both(lambda o: o.exact(x, 1500))
    assert e_obj[1] and e_twin[1]
    d.got.append(e_obj[0].copy())
    d.want.append(e_twin[0].copy())
    # configure moves a member to another geometry's group
    by.begin(256, 256)
    a.begin(256, 300)
    a.both(lambda o: o.configure(1, 1024, 256))
    assert pool.pending() == 0
    a.end()
    by.end()
    assert a.obj.blockSamples() == 1024
    calls = pool.engine_calls()
    for r in range(3):
        by.begin(300, 333)
        a.begin(700, 1800)
        pool.run()
        a.end()
        by.end()
    assert pool.engine_calls() == calls + 6  # two groups now
    # a clone of a member is unattached and independent
    k_obj, k_twin = a.both(lambda o: o.clone())
    assert emu.smst_pool_detach(k_obj.h) != 0 and b"not attached" in emu.smst_last_error()
    x = a.signal(600, -1)
    assert np.array_equal(k_obj.process(x, 700), k_twin.process(x, 700))
    a.obj.processAsync(x, 700)
    a.got.append(a.obj.wait().copy())
    a.want.append(a.twin.process(x, 700).copy())
    k_obj.close()
    k_twin.close()
    # destroying a member with a request pending runs the pool first
    z = pkg.SignalsmithStretch(seed=75, lib=emu)
    z.configure(2, 512, 128, True)
    pool.add(z)
    by.begin(300, 300)
    z.processAsync(x, 640)
    assert pool.pending() == 2 and pool.members() == 6
    z.close()
    assert pool.pending() == 0 and pool.members() == 5
    by.end()
    for p in (by, a, b, c, d):
        p.check("program order")
    pool.close()
    for p in (by, a, b, c, d):
        p.close()


def test_one_submission(emu):
    one_submission(emu, STEREO, dict(block=512, interval=128, split=False), 1024, 1536)


def test_errors_and_unattached_fallback(emu):
    pkg = package()
    pool = pkg.StretchPool(lib=emu)
    h = pkg.SignalsmithStretch(seed=5, lib=emu)
    # not attached: begin IS process, end reports its status
    x = np.ascontiguousarray(np.random.default_rng(1).uniform(-0.3, 0.3, (2, 600)), np.float32)
    h.channels = 2
    rc, keep, out = raw_begin(emu, h, x, 600)
    assert rc == -1 and b"unconfigured" in emu.smst_last_error()
    assert emu.smst_process_end(h.h) == -1 and b"unconfigured" in emu.smst_last_error()
    h.configure(2, 512, 128)
    twin = h.clone()
    rc, keep, out = raw_begin(emu, h, x, 700)
    assert rc == 0 and emu.smst_process_end(h.h) == 0
    assert np.array_equal(out, twin.process(x, 700)) and np.abs(out).max() > 1e-3
    h.processAsync(x, 500)
    assert np.array_equal(h.wait(), twin.process(x, 500))
    assert emu.smst_pool_detach(h.h) == -1 and b"not attached" in emu.smst_last_error()
    # attaching twice
    pool.add(h)
    assert emu.smst_pool_attach(pool.h, h.h) == -1 and b"already attached" in emu.smst_last_error()
    other = pkg.StretchPool(lib=emu)
    assert emu.smst_pool_attach(other.h, h.h) == -1 and b"already attached" in emu.smst_last_error()
    other.close()
    # begin on an unconfigured member
    u = pkg.SignalsmithStretch(seed=6, lib=emu)
    pool.add(u)
    u.channels = 2
    rc, keep, out = raw_begin(emu, u, x, 100)
    assert rc == -1 and b"unconfigured" in emu.smst_last_error()
    assert pool.pending() == 0 and pool.members() == 2
    u.configure(2, 512, 128)  # configured while attached: it takes a slot
    rc, keep, out = raw_begin(emu, u, x, 640)
    assert rc == 0 and pool.pending() == 1
    assert emu.smst_process_end(u.h) == 0 and np.abs(out).max() > 1e-3
    # null buffers with a non-zero count
    planes = (C.POINTER(C.c_float)*2)()
    assert emu.smst_process_begin(h.h, None, 10, keep[2], 10) == -1 and b"null buffers" in emu.smst_last_error()
    assert emu.smst_process_begin(h.h, keep[1], 10, planes, 10) == -1 and b"null buffers" in emu.smst_last_error()
    assert emu.smst_process_begin(h.h, keep[1], -1, keep[2], 10) == -1 and b"negative" in emu.smst_last_error()
    assert pool.pending() == 0
    assert emu.smst_process_begin(h.h, None, 0, None, 0) == 0 and emu.smst_process_end(h.h) == 0  # nothing in, nothing out: no buffers needed
    twin.process(x[:, :0], 0)
    h.processAsync(x, 600)
    assert np.array_equal(h.wait(), twin.process(x, 600))
    # a handle on another device (needs a second device: the stand-in has one)
    if emu.smst_device_count() > 1:
        far = pkg.SignalsmithStretch(seed=7, device=1, lib=emu)
        assert emu.smst_pool_attach(pool.h, far.h) == -1 and b"another device" in emu.smst_last_error()
        far.close()
    p2 = C.c_void_p()
    assert emu.smst_pool_create(C.byref(p2), 99) == -1 and b"out of range" in emu.smst_last_error()
    pool.close()
    for o in (h, u, twin):
        o.close()


def test_no_steady_state_allocation(emu):
    pkg = package()
    pool = pkg.StretchPool(lib=emu)
    pairs = [Pair(emu, 200 + s, STEREO if s < 3 else MONO_SPLIT) for s in range(5)]
    for p in pairs:
        pool.add(p.obj)

    def run():
        for s, p in enumerate(pairs):
            p.begin(600 + 10*s, 900 + 7*s)
        pool.run()
        for p in pairs:
            p.end()
    run()
    run()
    before = pool.allocation_events()
    assert before > 0
    for _ in range(10):
        run()
    assert pool.allocation_events() == before, (before, pool.allocation_events())
    for p in pairs:
        p.check("steady state")
    pool.close()
    for p in pairs:
        p.close()
