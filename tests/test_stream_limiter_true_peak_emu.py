"""The stream limiter's true-peak flag (include/smst.h, "Stream limiter") on the CPU stand-in: the numpy mirror against the known answers and
its own prefixes, the hook against the mirror bit for bit, cut invariance, NaN and inf, processFrames and flushFrames end to end, the opt-in,
the steady state, the getters and refusals, the clearing rules, the deferred schedules and the overshoot figures
(tests/stream_limiter_true_peak_cases.py has the mirror and the checks).  On a library without the flag's entry points every test but the
mirror's own fails at its first call."""
import ctypes as C

import numpy as np
import pytest

import dither_cases as dc
import level_cases as lc
import limiter_cases as lm
import pcm_cases as pc
import pcm_format_cases as fc
import stream_limiter_true_peak_cases as st
from conftest import package
from test_pcm_emu import hooks  # noqa: F401  (the fixture: the stream model's hooks bound, the eager schedule restored afterwards)
from test_stream_order_emu import _same

FORMATS = [(fc.S16, False), (fc.S16, True), (fc.S24, False), (fc.S24, True), (fc.F32, False)]


def test_mirror_known_answers_and_prefixes():
    st.check_mirror()


def test_overshoot_figures():
    """printed, not asserted (include/smst.h and EXPERIMENTS.md quote them): the worst true peak over the ceiling without and with the flag"""
    for H in (72, 36, 8, 1):
        print("H %4d: sample-peak detector %.3g over the ceiling, true-peak detector %.3g" % (H, st.overshoot(H, False), st.overshoot(H, True)))


def test_known_answers_through_the_hook(emu):
    st.check_known_answers(emu)


@pytest.mark.parametrize("lookahead", [1, 2, 3, 72])
@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_hook_against_mirror(emu, channels, lookahead):
    st.check_hook(emu, channels, lookahead, variants=(channels % 5, (channels + 2) % 5))


@pytest.mark.parametrize("channels", [1, 2])
def test_hook_against_mirror_longest_lookahead(emu, channels):
    st.check_hook(emu, channels, lm.MAX_H, variants=st.LONGEST_VARIANTS)


def test_cut_invariance(emu):
    st.check_cut_invariance(emu)


def test_nan_and_inf(emu):
    st.check_nan_inf(emu)


def test_two_runs_of_the_hook_are_bit_identical(emu):
    st.check_reproducible(emu)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_process_and_flush(emu, fmt, dithered):
    st.check_session(emu, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_process_and_flush_short_lookahead(emu, fmt, dithered):
    st.check_session(emu, fmt, dithered, H=3)


def test_two_sessions_are_identical(emu):
    st.check_two_runs(emu)


def test_behind_a_stream_output_resample(emu):
    st.check_behind_out_resample(emu)


def test_opt_in(emu):
    st.check_opt_in(emu)


def test_steady_state(emu):
    st.check_steady_state(emu)


def test_getters_and_refusals(emu):
    st.check_refusals(emu)


@pytest.mark.parametrize("action", ["flag_again", "flag_one", "flag_off", "setter", "lookahead", "reset", "level"])
def test_clearing(emu, action):
    st.check_clearing(emu, action)


# ---- stream order: two device-memory process calls in flight under the deferred schedules ------------------------------------------------

def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _ordered_stream_limiter(lib):
    """test_stream_limiter_emu._ordered_stream_limiter with a flagged stream beside a limited one without the flag: two
    smst_batch_process_pcm calls in SMST_MEM_DEVICE, issued back to back, with the caller's own producer and consumer streams.  The second
    call's feed passes write the lines the first call's conversion reads, and both calls share the rows -- stream order alone must keep them
    apart.  The outputs are read on the consumer only, behind both calls."""
    pkg = package()
    S, Cn, fmt = 3, 2, fc.S16
    frames, _ = dc.session_inputs(fmt)
    b = pkg.StretchBatch(S, Cn, lib=lib, seed=4, **pc.GEOMETRY)
    st.set_session(b, lc.ceiling(fmt, True))
    b.setPcmDither(dc.TPDF, 8)
    prod, cons = lib.smst_emu_stream_create(), lib.smst_emu_stream_create()
    keep, results = [], []
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    pos = 0
    for nout, nin in (([700, 300, 130], [640, 300, 128]), ([128, 515, 0], [128, 500, 0])):
        n = max(nin)
        host = np.ascontiguousarray(frames[:, pos:pos + n])
        pos += n
        dev = np.zeros_like(host)
        out = np.full((S, max(nout), Cn), 0x5A5A, host.dtype)
        y = np.zeros_like(out)
        for a in (dev, out):
            lib.smst_emu_register_device(_ptr(a), a.nbytes)
        lib.smst_emu_memcpy_async(_ptr(dev), _ptr(host), dev.nbytes, prod)
        assert lib.smst_batch_wait_for_stream(b.h, prod) == 0
        rc = lib.smst_batch_process_pcm(b.h, _ptr(dev), Cn*n, Cn, ip(ints(nin)), _ptr(out), Cn*out.shape[1], Cn, ip(ints(nout)), fmt, pkg.MEM_DEVICE)
        assert rc == 0, lib.smst_last_error()
        assert lib.smst_batch_signal_stream(b.h, cons) == 0
        lib.smst_emu_memcpy_async(_ptr(y), _ptr(out), out.nbytes, cons)
        results.append(y)
        keep.extend([dev, out, host])
    lib.smst_emu_stream_synchronize(cons)
    results.extend(b.take_pcm_stream_limiter())
    results.extend(b.take_pcm_peaks())
    results.append(b.takePcmOvers()[0])
    for a in keep[0::3] + keep[1::3]:
        lib.smst_emu_unregister_device(_ptr(a))
    lib.smst_emu_stream_destroy(prod)
    lib.smst_emu_stream_destroy(cons)
    b.close()
    return results


def test_device_memory_stream_limiter_under_deferred_schedules(hooks):  # noqa: F811
    assert hooks.smst_emu_set_schedule(b"eager") == 0
    want = _ordered_stream_limiter(hooks)
    assert want[0].any() and want[1].any() and want[2][0] < 1 and want[2][1] == 1 and want[3][0] > 0 and want[3][1] == 0
    failures = []
    for spec in ("lazy", "random:1", "random:2", "random:3"):
        assert hooks.smst_emu_set_schedule(spec.encode()) == 0
        try:
            got = _ordered_stream_limiter(hooks)
            hooks.smst_emu_device_synchronize()
            _same(want, got)
        except AssertionError as e:
            failures.append("%s: %s" % (spec, e))
        finally:
            hooks.smst_emu_set_schedule(None)
    assert not failures, "\n".join(failures)
