"""Cross-stream ordering of the engine on the CPU stand-in's stream model (tests/emu/hip/hip_runtime.h).

Every process() call runs over four HIP streams (`st`, `stChain`, `stSynth`, `stGate`) joined by events.  The stand-in's default
schedule runs every operation when it is enqueued, so a missing join cannot show there.  Here each scenario runs again under the
`lazy` schedule (nothing runs before a host-blocking call needs it, and then only what the HIP contract says that call waits for) and
under seeded `random` schedules (all queued work in a random order that keeps each stream's order and the event edges).  The kernels
are deterministic, so outputs and carried state must be bit-identical to the eager run: any difference is a missing edge.

The first tests prove that the model itself has teeth, independently of the engine: each rule it relies on, switched off, changes
what a test observes."""
import ctypes as C

import numpy as np
import pytest

import parity_cases as pc
from conftest import package, synth_input

SCHEDULES = ("lazy", "random:1", "random:2", "random:3")
I_ALIGNED = 480                                  # block 1920 / interval 480: the line-aligned producers' geometry (kVocoderCont)
ALIGNED = dict(block=1920, interval=I_ALIGNED)


@pytest.fixture(scope="module")
def model(emu):
    """The stand-in library with the stream model's test hooks bound; every test leaves the eager schedule and all rules on."""
    hooks = {
        "smst_emu_set_schedule": (C.c_int, [C.c_char_p]),
        "smst_emu_set_rule": (C.c_int, [C.c_char_p, C.c_int]),
        "smst_emu_stream_create": (C.c_void_p, []),
        "smst_emu_stream_destroy": (None, [C.c_void_p]),
        "smst_emu_stream_synchronize": (C.c_int, [C.c_void_p]),
        "smst_emu_device_synchronize": (C.c_int, []),
        "smst_emu_event_create": (C.c_void_p, []),
        "smst_emu_event_destroy": (None, [C.c_void_p]),
        "smst_emu_event_record": (C.c_int, [C.c_void_p, C.c_void_p]),
        "smst_emu_stream_wait_event": (C.c_int, [C.c_void_p, C.c_void_p]),
        "smst_emu_memcpy_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
        "smst_emu_host_malloc": (C.c_void_p, [C.c_size_t]),
        "smst_emu_host_free": (None, [C.c_void_p]),
        "smst_emu_register_device": (None, [C.c_void_p, C.c_size_t]),
        "smst_emu_unregister_device": (None, [C.c_void_p]),
        "smst_emu_enqueue_tick": (None, [C.c_void_p, C.c_void_p]),
        "smst_emu_queued": (C.c_longlong, []),
        "smst_emu_pageable_async_copies": (C.c_longlong, []),
    }
    for name, (res, args) in hooks.items():
        f = getattr(emu, name)
        f.restype, f.argtypes = res, args
    return emu


@pytest.fixture
def hooks(model):
    yield model
    model.smst_emu_set_schedule(None)
    for rule in ("waits", "bind_at_wait", "pinned_at_execution"):
        model.smst_emu_set_rule(rule.encode(), 1)


def _schedule(lib, spec):
    assert lib.smst_emu_set_schedule(spec.encode() if spec else None) == 0, spec


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


# ---- the model's self-test ---------------------------------------------------------------------------------------------------------

def _producer_consumer(lib, wait, rerecord=False):
    """Stream A copies `fresh` over the device buffer D, stream B copies D into `seen`; B waits for A's copy if `wait`.  With
    `rerecord`, A then copies `later` over D and re-records the event after the wait was enqueued.  Returns what B saw."""
    A, B = lib.smst_emu_stream_create(), lib.smst_emu_stream_create()
    e = lib.smst_emu_event_create()
    stale, fresh, later = (np.full(64, v, np.float32) for v in (1, 2, 3))
    D, seen = stale.copy(), np.zeros(64, np.float32)
    lib.smst_emu_register_device(_ptr(D), D.nbytes)
    try:
        lib.smst_emu_memcpy_async(_ptr(D), _ptr(fresh), D.nbytes, A)
        lib.smst_emu_event_record(e, A)
        if wait:
            lib.smst_emu_stream_wait_event(B, e)
        if rerecord:
            lib.smst_emu_memcpy_async(_ptr(D), _ptr(later), D.nbytes, A)
            lib.smst_emu_event_record(e, A)
        lib.smst_emu_memcpy_async(_ptr(seen), _ptr(D), D.nbytes, B)
        lib.smst_emu_stream_synchronize(B)
        out = float(seen[0])
        lib.smst_emu_device_synchronize()
    finally:
        lib.smst_emu_unregister_device(_ptr(D))
        lib.smst_emu_event_destroy(e)
        lib.smst_emu_stream_destroy(A)
        lib.smst_emu_stream_destroy(B)
    return out


def test_model_consumer_without_wait_reads_stale(hooks):
    _schedule(hooks, "lazy")
    assert _producer_consumer(hooks, wait=False) == 1.0
    _schedule(hooks, "eager")  # the rule this leg relies on is the deferred schedule: eagerly, the same program reads fresh data
    assert _producer_consumer(hooks, wait=False) == 2.0


def test_model_consumer_with_wait_reads_fresh(hooks):
    _schedule(hooks, "lazy")
    assert _producer_consumer(hooks, wait=True) == 2.0
    hooks.smst_emu_set_rule(b"waits", 0)
    assert _producer_consumer(hooks, wait=True) == 1.0


def test_model_rerecorded_event_does_not_retarget_a_wait(hooks):
    _schedule(hooks, "lazy")
    assert _producer_consumer(hooks, wait=True, rerecord=True) == 2.0  # bound to the record that existed when B waited
    hooks.smst_emu_set_rule(b"bind_at_wait", 0)
    assert _producer_consumer(hooks, wait=True, rerecord=True) == 3.0


def test_model_wait_on_never_recorded_event_does_not_block(hooks):
    _schedule(hooks, "lazy")
    A, B = hooks.smst_emu_stream_create(), hooks.smst_emu_stream_create()
    e = hooks.smst_emu_event_create()
    a_ran, b_ran = np.zeros(1, np.int32), np.zeros(1, np.int32)
    hooks.smst_emu_enqueue_tick(A, _ptr(a_ran))
    hooks.smst_emu_stream_wait_event(B, e)
    hooks.smst_emu_enqueue_tick(B, _ptr(b_ran))
    hooks.smst_emu_stream_synchronize(B)
    assert b_ran[0] > 0 and a_ran[0] == 0  # B ran; nothing of A's was needed
    hooks.smst_emu_device_synchronize()
    assert a_ran[0] > 0 and hooks.smst_emu_queued() == 0
    hooks.smst_emu_event_destroy(e)
    hooks.smst_emu_stream_destroy(A)
    hooks.smst_emu_stream_destroy(B)


def test_model_pinned_source_is_read_when_the_copy_runs(hooks):
    def run():
        A = hooks.smst_emu_stream_create()
        p = hooks.smst_emu_host_malloc(256)
        pinned = np.ctypeslib.as_array((C.c_float*64).from_address(p))
        pinned[:] = 1
        D = np.zeros(64, np.float32)
        hooks.smst_emu_register_device(_ptr(D), D.nbytes)
        hooks.smst_emu_memcpy_async(_ptr(D), C.c_void_p(p), D.nbytes, A)
        pinned[:] = 2  # the host rewrites the staging after the enqueue
        hooks.smst_emu_stream_synchronize(A)
        hooks.smst_emu_unregister_device(_ptr(D))
        hooks.smst_emu_stream_destroy(A)
        del pinned
        hooks.smst_emu_host_free(C.c_void_p(p))
        return float(D[0])
    _schedule(hooks, "lazy")
    assert run() == 2.0
    hooks.smst_emu_set_rule(b"pinned_at_execution", 0)
    assert run() == 1.0
    # a pageable source is staged at enqueue (the documented choice of the model)
    A = hooks.smst_emu_stream_create()
    src, D = np.ones(64, np.float32), np.zeros(64, np.float32)
    hooks.smst_emu_register_device(_ptr(D), D.nbytes)
    hooks.smst_emu_memcpy_async(_ptr(D), _ptr(src), D.nbytes, A)
    src[:] = 2
    hooks.smst_emu_stream_synchronize(A)
    hooks.smst_emu_unregister_device(_ptr(D))
    hooks.smst_emu_stream_destroy(A)
    assert D[0] == 1.0


def _tick_order(lib, spec, streams=4, per_stream=6):
    _schedule(lib, spec)
    ss = [lib.smst_emu_stream_create() for _ in range(streams)]
    slots = np.zeros((streams, per_stream), np.int32)
    for k in range(per_stream):
        for i, s in enumerate(ss):
            lib.smst_emu_enqueue_tick(s, C.c_void_p(slots.ctypes.data + 4*(i*per_stream + k)))
    lib.smst_emu_device_synchronize()
    for s in ss:
        lib.smst_emu_stream_destroy(s)
    assert (np.diff(slots, axis=1) > 0).all(), slots  # each stream's FIFO order holds in every schedule
    return np.argsort(slots.ravel()).tolist()


def test_model_random_seeds_order_independent_work_differently(hooks):
    a, b, a2 = _tick_order(hooks, "random:1"), _tick_order(hooks, "random:2"), _tick_order(hooks, "random:1")
    assert a != b and a == a2


def test_model_random_keeps_event_edges(hooks):
    """Under every seed, work behind a wait runs after the work the event recorded, never before it."""
    for seed in range(8):
        _schedule(hooks, "random:%d" % seed)
        A, B = hooks.smst_emu_stream_create(), hooks.smst_emu_stream_create()
        e = hooks.smst_emu_event_create()
        t = np.zeros(4, np.int32)
        hooks.smst_emu_enqueue_tick(A, _ptr(t[0:]))
        hooks.smst_emu_event_record(e, A)
        hooks.smst_emu_enqueue_tick(A, C.c_void_p(t.ctypes.data + 4))
        hooks.smst_emu_stream_wait_event(B, e)
        hooks.smst_emu_enqueue_tick(B, C.c_void_p(t.ctypes.data + 8))
        hooks.smst_emu_stream_synchronize(B)
        assert t[2] > t[0] > 0, (seed, t)
        hooks.smst_emu_device_synchronize()
        assert hooks.smst_emu_queued() == 0
        hooks.smst_emu_event_destroy(e)
        hooks.smst_emu_stream_destroy(A)
        hooks.smst_emu_stream_destroy(B)


# ---- the engine under the deferred schedules ---------------------------------------------------------------------------------------

def _same(a, b, where="result"):
    """Bit-identity of two nested results (dicts / lists / arrays / scalars); NaNs must sit in the same places."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (p, q) in enumerate(zip(a, b)):
            _same(p, q, "%s[%d]" % (where, i))
    elif a is None or isinstance(a, (int, float, bool, str)):
        assert a == b, (where, a, b)
    else:
        p, q = np.asarray(a), np.asarray(b)
        assert p.shape == q.shape, (where, p.shape, q.shape)
        if not np.array_equal(p, q, equal_nan=True):
            bad = np.argwhere(~((p == q) | (np.isnan(p) & np.isnan(q)))) if p.dtype.kind in "fc" else np.argwhere(p != q)
            raise AssertionError("%s differs in %d places, first %s: max |diff| %g" % (where, len(bad), bad[:3].tolist(),
                                 float(np.nanmax(np.abs(p.astype(np.complex128) - q.astype(np.complex128))))))


def _check_schedules(lib, scenario, schedules=SCHEDULES):
    """Run `scenario(lib)` eagerly and under every deferred schedule: everything it returns must be bit-identical."""
    _schedule(lib, "eager")
    want = scenario(lib)
    failures = []
    for spec in schedules:
        _schedule(lib, spec)
        try:
            got = scenario(lib)
            lib.smst_emu_device_synchronize()
            _same(want, got)
        except AssertionError as e:
            failures.append("%s: %s" % (spec, e))
        finally:
            _schedule(lib, None)
    assert not failures, "\n".join(failures)
    return want


def _state(b, streams=None):
    return [[b.debug_state(s, w) for w in (0, 1, 2, 3)] for s in (range(b.streams) if streams is None else streams)]


def _inputs(S, C, n, sr=48000):
    return np.stack([synth_input(s, C, n, sr) + 0.3*synth_input(s + 4, C, n, sr) for s in range(S)])


def _calls(b, x, calls):
    """process() calls of (out, in) samples per stream, through the host-memory path; returns the outputs and the final state."""
    outs, pos = [], 0
    for nout, nin in calls:
        nout, nin = np.asarray(nout, np.int32), np.asarray(nin, np.int32)
        outs.append(np.array(b.process(np.ascontiguousarray(x[:, :, pos:pos + int(nin.max())]), nout, in_samples=nin), copy=True))
        pos += int(nin.max())
    return outs


def _multi_tile(lib, setup=None, S=3, Cn=2, I=128, calls=None):
    pkg = package()
    calls = calls or [([150*I + 17, 100*I + 5, 40*I], [100*I, 100*I, 50*I]), ([70*I, 130*I + 3, 66*I], [70*I, 90*I, 66*I]), ([20*I]*3, [20*I]*3)]
    x = _inputs(S, Cn, sum(max(c[1]) for c in calls))
    b = pkg.StretchBatch(S, Cn, block=4*I, interval=I, lib=lib)
    if setup:
        setup(b)
    r = dict(out=_calls(b, x, calls), state=_state(b))
    b.close()
    return r


def test_multi_tile_plain(hooks):
    _check_schedules(hooks, _multi_tile)


def test_multi_tile_mapped(hooks):
    _check_schedules(hooks, lambda lib: _multi_tile(lib, setup=lambda b: b.setTransposeSemitones(5, 8000/48000)))


def test_multi_tile_formants_estimated_base(hooks):
    def setup(b):
        b.setTransposeSemitones(-3, 0)
        b.setFormantFactor(1.2, True)
        b.setFormantBase(0)  # estimated per hop
    _check_schedules(hooks, lambda lib: _multi_tile(lib, setup=setup))


@pytest.mark.parametrize("how", ["sub_streams", "workspace"])
def test_sub_batches(hooks, monkeypatch, how):
    if how == "sub_streams":
        monkeypatch.setenv("SMST_SUB_STREAMS", "2")
    else:
        monkeypatch.setenv("SMST_WORKSPACE_GIB", "0.009")  # 2 streams per sub-batch at this geometry (as case_sub_batches)
    I = 128
    calls = [([90*I]*5, [70*I]*5), ([66*I + 3, 80*I, 10*I, 70*I, 1], [50*I]*5)]
    _check_schedules(hooks, lambda lib: _multi_tile(lib, S=5, calls=calls, setup=lambda b: b.setTransposeSemitones(2, 0, stream=3)))


# Tile patterns of SMST_CONTINUOUS=1 that reach the end-of-segment joins: parity_cases.CONTINUOUS_PATTERNS (N C C, N C C N, N N N C C),
# each proved by the launch counters of its last call.
PATTERNS = pc.CONTINUOUS_PATTERNS


def _continuous(lib, calls, expect=None, Cn=1, more=None):
    pkg = package()
    S = len(calls[0][0])
    x = _inputs(S, Cn, sum(max(c[1]) for c in calls) + (sum(max(c[1]) for c in more) if more else 0))
    b = pkg.StretchBatch(S, Cn, lib=lib, **ALIGNED)
    outs = []
    for i, call in enumerate(calls):
        before = [pkg.launch_count(k, lib) for k in ("vocoder_continuous",) + pc.TILED_FORMS]
        pos = sum(max(c[1]) for c in calls[:i])
        outs += _calls(b, x[:, :, pos:], [call])
        grew = [pkg.launch_count(k, lib) - v for k, v in zip(("vocoder_continuous",) + pc.TILED_FORMS, before)]
        if expect and i == len(calls) - 1:
            assert (grew[0], sum(grew[1:])) == expect, ("continuous / tile-by-tile launches", grew, expect)
    if more:  # calls after the pattern: they start from the state its last tiles handed over
        outs += _calls(b, x[:, :, sum(max(c[1]) for c in calls):], more)
    r = dict(out=outs, state=_state(b))
    b.close()
    return r


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_continuous_tile_patterns(hooks, monkeypatch, pattern):
    monkeypatch.setenv("SMST_CONTINUOUS", "1")
    calls, expect = PATTERNS[pattern]
    S = len(calls[0][0])
    more = [([40*I_ALIGNED]*S, [40*I_ALIGNED]*S)]
    cont = _check_schedules(hooks, lambda lib: _continuous(lib, calls, expect, more=more))
    monkeypatch.delenv("SMST_CONTINUOUS")
    _same(cont, _continuous(hooks, calls, more=more), "continuous vs tile by tile")  # (and the cross-check itself holds)


def test_continuous_stereo_two_calls(hooks, monkeypatch):
    monkeypatch.setenv("SMST_CONTINUOUS", "1")
    I = I_ALIGNED
    _check_schedules(hooks, lambda lib: _continuous(lib, [([200*I, 150*I + 7], [200*I, 100*I])], Cn=2, more=[([130*I, 129*I + 1], [130*I, 90*I])]))


def _split_session(lib):
    """Split computation: blocks in flight across calls (runPendingBlocks), flush() mid-interval, seek() and outputSeek()."""
    pkg = package()
    S, Cn, I = 3, 2, 128
    x = _inputs(S, Cn, 60000)
    b = pkg.StretchBatch(S, Cn, block=512, interval=I, split=True, lib=lib)
    b.setTransposeSemitones(3, 0, stream=1)
    r = {}
    r["a"] = _calls(b, x, [([5*I + 40, 3*I + 100, 7*I], [5*I, 3*I, 7*I]), ([2*I + 60, 90, 4*I + 3], [2*I, 100, 4*I]), ([31, 45, 2*I], [31, 45, 2*I])])
    b.setFormantFactor(1.3, True, stream=2)  # a setter between a block's steps (the block keeps what it saw)
    r["b"] = _calls(b, x[:, :, 3000:], [([70, 3*I, 200], [70, 3*I, 200])])
    r["flush"] = b.flush([I + 50, 77, 3*I])
    r["state_flush"] = _state(b)
    b.seek(np.ascontiguousarray(x[:, :, 9000:9000 + b.seekLength()]), [1.0, 0.8, 1.25])
    r["c"] = _calls(b, x[:, :, 12000:], [([6*I + 5]*3, [6*I]*3), ([20*I]*3, [15*I]*3)])
    b.outputSeek(np.ascontiguousarray(x[:, :, 20000:26000]))
    r["d"] = _calls(b, x[:, :, 26000:], [([9*I]*3, [9*I]*3)])
    r["state"] = _state(b)
    b.close()
    return r


def test_split_pending_flush_seek(hooks):
    _check_schedules(hooks, _split_session)


def _setters_between_calls(lib):
    pkg = package()
    S, Cn, I = 3, 2, 128
    x = _inputs(S, Cn, 110*I)
    b = pkg.StretchBatch(S, Cn, block=512, interval=I, lib=lib)
    r = []
    r += _calls(b, x, [([70*I]*3, [70*I]*3)])
    table = np.array([(i + 0.5)/160*1.2 for i in range(80)], np.float32)
    b.setFreqMapTable(table, stream=0)         # a table upload while the kernels of the call before may still run
    r += _calls(b, x[:, :, 20*I:], [([66*I]*3, [60*I]*3)])
    b.setFreqMapTable(table[:40]*1.1, stream=2)
    b.setTransposeSemitones(-4, 0.2, stream=1)
    r += _calls(b, x[:, :, 30*I:], [([65*I]*3, [65*I]*3)])
    b.setFormantFactor(0.8, True)
    b.setFormantBase(180/48000, stream=0)
    r += _calls(b, x[:, :, 10*I:], [([64*I + 9]*3, [70*I]*3)])
    b.setFreqMapTable(None)
    r += _calls(b, x[:, :, 40*I:], [([30*I]*3, [30*I]*3)])
    r.append(_state(b))
    b.close()
    return r


def test_setters_between_calls(hooks):
    _check_schedules(hooks, _setters_between_calls)


def _clone_and_debug(lib, monkeypatch):
    pkg = package()
    Cn, I = 2, 128
    x = _inputs(1, Cn, 40000)[0]
    a = pkg.SignalsmithStretch(seed=3, lib=lib)
    a.configure(Cn, 512, I, False)
    a.setTransposeSemitones(3, 8000/48000)
    a.setFormantFactor(1.1, True)
    r = [a.process(x[:, :6000], 7500)]
    b = a.clone()
    r += [a.process(x[:, 6000:9000], 3600), b.process(x[:, 6000:9000], 3000), a.flush(300), b.flush(200)]
    a.close()
    b.close()
    monkeypatch.setenv("SMST_NO_FEED_FUSION", "1")  # (debug_formants needs the separate producers)
    batch = pkg.StretchBatch(2, Cn, block=512, interval=I, lib=lib)
    batch.setTransposeSemitones(4, 0)
    batch.setFormantFactor(1.2, True, stream=1)
    xx = _inputs(2, Cn, 20000)
    for k, n in enumerate((70*I, 33, 90, 2*I + 5, 64*I)):  # carried-only calls (no hop fires) between calls that fire hops
        r.append(np.array(batch.process(np.ascontiguousarray(xx[:, :, 1000*k:1000*k + n]), n), copy=True))
        r.append([batch.debug_map(0), batch.debug_formants(1), batch.debug_carry(0)])
    r.append(_state(batch))
    batch.close()
    monkeypatch.delenv("SMST_NO_FEED_FUSION")
    return r


def test_clone_debug_getters_carried_only(hooks, monkeypatch):
    _check_schedules(hooks, lambda lib: _clone_and_debug(lib, monkeypatch))


def _realtime(lib, quantum=128, quanta=40):
    pkg = package()
    Cn = 2
    x = _inputs(1, Cn, quantum*(quanta + 40))[0]
    o = pkg.SignalsmithStretch(lib=lib)
    o.configure(Cn, 512, 128, False)
    live = [o.process(x[:, q*quantum:(q + 1)*quantum], quantum) for q in range(quanta)]
    o.reset()
    buf_len = o.inputLatency() + o.outputLatency()
    play = []
    for q in range(quanta):  # buffered playback: every quantum re-seeks, then asks for output without new input
        end = int(round((q + 1)*quantum*0.8)) + o.inputLatency()
        buf = np.zeros((Cn, buf_len), np.float32)
        lo = max(0, end - buf_len)
        buf[:, buf_len - (end - lo):] = x[:, lo:end]
        o.seek(buf, 0.8)
        play.append(o.process(x[:, :0], quantum))
    o.close()
    return [live, play]


def test_realtime_quanta(hooks):
    _check_schedules(hooks, _realtime)


def _device_memory(lib, continuous):
    """SMST_MEM_DEVICE with the caller's own producer and consumer streams: the producer uploads each call's input, the batch waits
    for it (smst_batch_wait_for_stream), and the consumer, ordered after the batch by smst_batch_signal_stream, copies the output
    out.  The output is read on the consumer only, never after smst_batch_synchronize."""
    pkg = package()
    S, Cn, I = 2, 2, (I_ALIGNED if continuous else 128)
    x = _inputs(S, Cn, 400*I + 70)  # (130 + 70 + 200) I + 70: the longest input of each call below -- one sample less and the last upload reads past `x`
    b = pkg.StretchBatch(S, Cn, lib=lib, **(ALIGNED if continuous else dict(block=512, interval=128)))
    prod, cons = lib.smst_emu_stream_create(), lib.smst_emu_stream_create()
    keep, results, pos = [], [], 0
    for nout, nin in ([150*I, 130*I], [100*I, 130*I]), ([70*I + 9, 64*I], [70*I, 64*I]), ([30, 70], [30, 70]), ([200*I, 66*I], [200*I, 66*I]):
        n, m = max(nin), max(nout)
        dx = np.zeros((S, Cn, n), np.float32)                    # "device" buffers: a fresh pair per call, alive to the end
        dy = np.full((S, Cn, m), np.nan, np.float32)
        for a in (dx, dy):
            lib.smst_emu_register_device(_ptr(a), a.nbytes)
        host_x = np.ascontiguousarray(x[:, :, pos:pos + n])
        pos += n
        lib.smst_emu_memcpy_async(_ptr(dx), _ptr(host_x), dx.nbytes, prod)
        assert lib.smst_batch_wait_for_stream(b.h, prod) == 0
        pin, pout = np.asarray(nin, np.int32), np.asarray(nout, np.int32)
        assert lib.smst_batch_process(b.h, _ptr(dx), Cn*n, n, pin.ctypes.data_as(C.POINTER(C.c_int)), _ptr(dy), Cn*m, m,
                                      pout.ctypes.data_as(C.POINTER(C.c_int)), pkg.MEM_DEVICE) == 0
        assert lib.smst_batch_signal_stream(b.h, cons) == 0
        y = np.zeros_like(dy)
        lib.smst_emu_memcpy_async(_ptr(y), _ptr(dy), dy.nbytes, cons)
        lib.smst_emu_stream_synchronize(cons)
        results.append(y)
        keep += [dx, dy, host_x]
    lib.smst_emu_device_synchronize()
    for a in keep:
        lib.smst_emu_unregister_device(_ptr(a))
    lib.smst_emu_stream_destroy(prod)
    lib.smst_emu_stream_destroy(cons)
    results.append(_state(b))
    b.close()
    return results


@pytest.mark.parametrize("continuous", [False, True])
def test_device_memory_caller_streams(hooks, monkeypatch, continuous):
    if continuous:
        monkeypatch.setenv("SMST_CONTINUOUS", "1")
    _check_schedules(hooks, lambda lib: _device_memory(lib, continuous))


# ---- the whole-call stages: seek, flush, outputSeek, the resets under them, exact() ---------------------------------------------------------

class _DeviceCalls:
    """whole_call_cases' calls through the C ABI on SMST_MEM_DEVICE buffers with the caller's own producer and consumer streams, as
    _device_memory: an input goes up from pinned memory on the producer, the batch waits for it; an output is read on the consumer, ordered
    after the batch by smst_batch_signal_stream, never after smst_batch_synchronize.  Every buffer is a fresh one and lives to close()."""

    def __init__(self, lib, batch):
        self.lib, self.b, self.pkg = lib, batch, package()
        self.prod, self.cons = lib.smst_emu_stream_create(), lib.smst_emu_stream_create()
        self.device, self.pinned = [], []

    def _ints(self, v):
        a = np.ascontiguousarray(v, np.int32)
        return a, a.ctypes.data_as(C.POINTER(C.c_int))

    def _new(self, shape, dtype, fill):
        d = np.full(shape, fill, dtype)
        self.lib.smst_emu_register_device(_ptr(d), d.nbytes)
        self.device.append(d)
        return d

    def _up(self, x):
        p = self.lib.smst_emu_host_malloc(x.nbytes)
        self.pinned.append(p)
        C.memmove(p, x.ctypes.data, x.nbytes)
        d = self._new(x.shape, x.dtype, 0)
        self.lib.smst_emu_memcpy_async(_ptr(d), C.c_void_p(p), d.nbytes, self.prod)
        assert self.lib.smst_batch_wait_for_stream(self.b.h, self.prod) == 0
        return d

    def _ok(self, rc):
        assert rc == 0, self.lib.smst_last_error()

    def seek(self, x, counts, rates):
        d, (_, n), r = self._up(x), self._ints(counts), np.ascontiguousarray(rates, np.float64)
        self._ok(self.lib.smst_batch_seek(self.b.h, _ptr(d), x.shape[1]*x.shape[2], x.shape[2], n, r.ctypes.data_as(C.POINTER(C.c_double)), self.pkg.MEM_DEVICE))

    def process(self, x, nin, nout):
        d, (_, pin), (_, pout), m = self._up(x), self._ints(nin), self._ints(nout), max(max(nout), 1)
        y = self._new((x.shape[0], x.shape[1], m), np.float32, np.nan)
        self._ok(self.lib.smst_batch_process(self.b.h, _ptr(d), x.shape[1]*x.shape[2], x.shape[2], pin, _ptr(y), x.shape[1]*m, m, pout, self.pkg.MEM_DEVICE))
        return y

    def flush(self, counts, rates):
        (_, n), r, m = self._ints(counts), np.ascontiguousarray(rates, np.float32), max(max(counts), 1)
        y = self._new((self.b.streams, self.b.channels, m), np.float32, np.nan)
        self._ok(self.lib.smst_batch_flush(self.b.h, _ptr(y), self.b.channels*m, m, n, r.ctypes.data_as(C.POINTER(C.c_float)), self.pkg.MEM_DEVICE))
        return y

    def output_seek(self, x, lengths):
        d, (_, n) = self._up(x), self._ints(lengths)
        self._ok(self.lib.smst_batch_output_seek(self.b.h, _ptr(d), x.shape[1]*x.shape[2], x.shape[2], n, self.pkg.MEM_DEVICE))

    def exact(self, x, nin, nout, frames):
        d, (_, pin), (_, pout), m = self._up(x), self._ints(nin), self._ints(nout), max(nout)
        status, Cn = np.full(self.b.streams, 1, np.int32), self.b.channels
        if frames:
            n, y = x.shape[1], self._new((x.shape[0], m, Cn), np.int16, 0x5A5A)
            self._ok(self.lib.smst_batch_exact_pcm(self.b.h, _ptr(d), n*Cn, Cn, pin, _ptr(y), m*Cn, Cn, pout, status.ctypes.data_as(C.POINTER(C.c_int)),
                                                   self.pkg.PCM_S16, self.pkg.MEM_DEVICE))
        else:
            n, y = x.shape[2], self._new((x.shape[0], Cn, m), np.float32, np.nan)
            self._ok(self.lib.smst_batch_exact(self.b.h, _ptr(d), Cn*n, n, pin, _ptr(y), Cn*m, m, pout, status.ctypes.data_as(C.POINTER(C.c_int)), self.pkg.MEM_DEVICE))
        return y, status == 0

    def host(self, d):
        y = np.zeros_like(d)
        assert self.lib.smst_batch_signal_stream(self.b.h, self.cons) == 0
        self.lib.smst_emu_memcpy_async(_ptr(y), _ptr(d), d.nbytes, self.cons)
        self.lib.smst_emu_stream_synchronize(self.cons)
        return y

    def close(self):
        self.lib.smst_emu_device_synchronize()
        for d in self.device:
            self.lib.smst_emu_unregister_device(_ptr(d))
        for p in self.pinned:
            self.lib.smst_emu_host_free(C.c_void_p(p))
        self.lib.smst_emu_stream_destroy(self.prod)
        self.lib.smst_emu_stream_destroy(self.cons)


def _whole_call(lib, split, rounds=1):
    """-> (the digests of whole_call_cases.SEQUENCE on device memory, async copies from pageable memory it made)"""
    import whole_call_cases as wc
    b = wc.new_batch(lib, split)
    calls = _DeviceCalls(lib, b)
    before = lib.smst_emu_pageable_async_copies()
    digests = wc.run_sequence(b, calls, rounds=rounds)
    pageable = lib.smst_emu_pageable_async_copies() - before
    calls.close()
    b.close()
    return digests, pageable


@pytest.mark.parametrize("name", ["plain", "split"])
def test_whole_call_stages(hooks, name):
    """Bit-identical under every schedule -- the stages' tables are pinned, so a set rewritten before its upload ran would show -- and equal
    to what the parent commit gave on host memory."""
    import json
    import whole_call_cases as wc
    digests, _ = _check_schedules(hooks, lambda lib: _whole_call(lib, wc.SCENARIOS[name]))
    assert digests == json.load(open(wc.GOLDEN["emu"]))["scenarios"][name]


@pytest.mark.parametrize("name", ["plain", "split"])
def test_no_pageable_async_copy_on_the_calling_paths(hooks, name):
    """csrc/smst_engine.h: "nothing pageable is handed to an async copy" -- over the whole-call sequence on device memory, setters between
    the calls included, and a second round of it (every set has been used before), the stand-in counts no such copy."""
    import whole_call_cases as wc
    _schedule(hooks, "eager")
    assert _whole_call(hooks, wc.SCENARIOS[name], rounds=2)[1] == 0


# ---- the _pcm calls' per-call table: every combination of its sections, on device memory -------------------------------------------------

class _DevicePcmCalls(_DeviceCalls):
    """pcm_tables_cases' frame calls through the C ABI on SMST_MEM_DEVICE buffers; frames are [S, n, C] (packed int24: [S, n, C, 3] bytes)"""

    def _format(self, a):
        return self.pkg.PCM_S24 if a.dtype == np.uint8 else {"int16": self.pkg.PCM_S16, "float32": self.pkg.PCM_F32}[a.dtype.name]

    def _out(self, like, m):
        return self._new((like.shape[0], m) + like.shape[2:], like.dtype, 0x5A if like.dtype == np.uint8 else 0x5A5A if like.dtype == np.int16 else np.nan)

    def process(self, x, nin, nout):
        d, (_, pin), (_, pout), m, Cn = self._up(x), self._ints(nin), self._ints(nout), max(max(nout), 1), self.b.channels
        y = self._out(x, m)
        self._ok(self.lib.smst_batch_process_pcm(self.b.h, _ptr(d), x.shape[1]*Cn, Cn, pin, _ptr(y), m*Cn, Cn, pout, self._format(x), self.pkg.MEM_DEVICE))
        return y

    def flush(self, counts, rates, fmt):
        (_, n), r, m, Cn = self._ints(counts), np.ascontiguousarray(rates, np.float32), max(max(counts), 1), self.b.channels
        like = {"s16": np.zeros((self.b.streams, 0, Cn), np.int16), "s24": np.zeros((self.b.streams, 0, Cn, 3), np.uint8), "f32": np.zeros((self.b.streams, 0, Cn), np.float32)}[fmt]
        y = self._out(like, m)
        self._ok(self.lib.smst_batch_flush_pcm(self.b.h, _ptr(y), m*Cn, Cn, n, r.ctypes.data_as(C.POINTER(C.c_float)), self._format(y), self.pkg.MEM_DEVICE))
        return y

    def exact(self, x, nin, nout):
        d, (_, pin), (_, pout), m, Cn = self._up(x), self._ints(nin), self._ints(nout), max(nout), self.b.channels
        status, y = np.full(self.b.streams, 1, np.int32), self._out(x, m)
        self._ok(self.lib.smst_batch_exact_pcm(self.b.h, _ptr(d), x.shape[1]*Cn, Cn, pin, _ptr(y), m*Cn, Cn, pout, status.ctypes.data_as(C.POINTER(C.c_int)),
                                               self._format(x), self.pkg.MEM_DEVICE))
        return y, status == 0


@pytest.mark.parametrize("spec", ("eager",) + SCHEDULES)
def test_pcm_tables_stages(hooks, spec):
    """pcm_tables_cases' sequence on device memory under each schedule: equal to what the parent commit gave on host memory -- the table sets
    are pinned and rotate, so one rewritten before its upload ran would show -- and no async copy from pageable memory."""
    import json
    import pcm_tables_cases as pt
    _schedule(hooks, spec)
    b = pt.new_batch(hooks)
    calls = _DevicePcmCalls(hooks, b)
    before = hooks.smst_emu_pageable_async_copies()
    digests = pt.run_sequence(b, calls)
    pageable = hooks.smst_emu_pageable_async_copies() - before
    calls.close()
    b.close()
    want = json.load(open(pt.GOLDEN["emu"]))["memory"]["host"]
    assert [k for k in sorted(want) if digests.get(k) != want[k]] == [] and sorted(digests) == sorted(want)
    assert pageable == 0
