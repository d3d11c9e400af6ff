"""The stream meter of the frame output (include/smst.h, "Stream meter") on the CPU stand-in: cut invariance and the equality with the clip
meters bit for bit, readings mid-programme, the true-peak edge, the capacity, NaN and inf, a second rate, the float64 numpy mirrors,
processFrames and flushFrames end to end, the opt-in, the steady state, the refusals, the clearing rules, two runs and the deferred
schedules (tests/stream_meter_cases.py has the checks).  On a library without the stream meter's entry points every test fails at its
first call."""
import ctypes as C

import numpy as np
import pytest

import pcm_cases as pc
import pcm_format_cases as fc
import stream_meter_cases as sm
from conftest import package
from test_pcm_emu import hooks  # noqa: F401  (the fixture: the stream model's hooks bound, the eager schedule restored afterwards)
from test_stream_order_emu import _same


@pytest.mark.parametrize("form", sm.FORMS)
@pytest.mark.parametrize("kind", sm.CUTS)
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_cut_invariance_and_clip_equivalence(emu, channels, kind, form):
    sm.check_cut(emu, sm.FS, channels, kind, forms=(form,))


@pytest.mark.parametrize("form", sm.FORMS)
@pytest.mark.parametrize("kind", sm.CUTS)
def test_cut_invariance_and_clip_equivalence_stable_rate(emu, kind, form):
    sm.check_cut(emu, sm.FS_STABLE, 2, kind, forms=(form,))


@pytest.mark.parametrize("form", sm.FORMS)
def test_cut_invariance_16_channels(emu, form):
    sm.check_cut(emu, sm.FS, 16, "ragged", forms=(form,))


def test_the_stable_programme_discriminates(emu):
    sm.check_discriminates(emu)


def test_weights_and_an_unmetered_stream(emu):
    sm.check_weights_and_unmetered(emu)


@pytest.mark.parametrize("form", sm.FORMS)
@pytest.mark.parametrize("fs", [sm.FS, sm.FS_STABLE])
def test_mid_programme_readings(emu, fs, form):
    sm.check_mid_readings(emu, fs, 2, form)


@pytest.mark.parametrize("form", sm.FORMS)
def test_true_peak_edge(emu, form):
    sm.check_true_peak_edge(emu, form)


@pytest.mark.parametrize("form", sm.FORMS)
def test_capacity(emu, form):
    sm.check_capacity(emu, form)


@pytest.mark.parametrize("form", sm.FORMS)
@pytest.mark.parametrize("fs", [sm.FS, sm.FS_STABLE])
def test_nan_and_inf(emu, fs, form):
    sm.check_nan_inf(emu, fs, form)


@pytest.mark.parametrize("form", sm.FORMS)
def test_second_rate(emu, form):
    sm.check_second_rate(emu, form)


def test_against_the_numpy_mirrors(emu):
    sm.check_against_mirrors(emu)


def test_two_runs_of_the_hook_are_bit_identical(emu):
    sm.check_reproducible(emu)


def test_hook_refusals(emu):
    sm.check_hook_refusals(emu)


@pytest.mark.parametrize("fs", [sm.E2E_FS, sm.E2E_FS_STABLE])
def test_process_and_flush(emu, fs):
    sm.check_e2e(emu, fs)


@pytest.mark.parametrize("fmt,dithered", sm.FORMATS)
def test_the_meter_changes_no_output_byte(emu, fmt, dithered):
    sm.check_e2e_bytes(emu, fmt, dithered)


def test_opt_in(emu):
    sm.check_opt_in(emu)


def test_steady_state(emu):
    sm.check_steady_state(emu)


def test_refusals_and_getters(emu):
    sm.check_refusals(emu)


@pytest.mark.parametrize("action", ["setter", "setter_one", "reset", "level"])
def test_clearing(emu, action):
    sm.check_clearing(emu, action)


# ---- stream order: device-memory process calls in flight under the deferred schedules ----------------------------------------------------

def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _ordered_stream_meter(lib):
    """Three smst_batch_process_pcm calls in SMST_MEM_DEVICE, issued back to back, with the caller's own producer and consumer streams
    (test_stream_limiter_emu._ordered_stream_limiter): every call's update reads and writes the ONE set of carried state, and the calls share
    the output image -- stream order alone must keep them apart.  The setter's clear is issued behind the first call: it, too, is ordered by
    the batch's stream.  The meter is read behind all of them."""
    pkg = package()
    S, Cn, fmt = 3, 2, fc.S16
    frames = sm.e2e_inputs(fmt)
    b = pkg.StretchBatch(S, Cn, lib=lib, seed=4, **pc.GEOMETRY)
    b.set_pcm_stream_meter(True, sm.E2E_FS_STABLE, 8)
    prod, cons = lib.smst_emu_stream_create(), lib.smst_emu_stream_create()
    keep, results = [], []
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    pos = 0
    for k, (nout, nin) in enumerate((([700, 300, 130], [640, 300, 128]), ([128, 515, 0], [128, 500, 0]), ([640, 640, 7], [512, 512, 6]))):
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
        if k == 0:
            b.set_pcm_stream_meter(True, sm.E2E_FS_STABLE, 8, stream=1)          # (stream 1 begins again behind the first call)
        assert lib.smst_batch_signal_stream(b.h, cons) == 0
        lib.smst_emu_memcpy_async(_ptr(y), _ptr(out), out.nbytes, cons)
        results.append(y)
        keep.extend([dev, out, host])
    lib.smst_emu_stream_synchronize(cons)
    take = b.take_pcm_stream_meter()
    results.extend(take[k] for k in sorted(take))
    assert [b.pcm_stream_meter_frames(s)[1] for s in range(S)] == [1468, 1155, 137]
    for a in keep[0::3] + keep[1::3]:
        lib.smst_emu_unregister_device(_ptr(a))
    lib.smst_emu_stream_destroy(prod)
    lib.smst_emu_stream_destroy(cons)
    b.close()
    return results


def test_device_memory_stream_meter_under_deferred_schedules(hooks):  # noqa: F811
    assert hooks.smst_emu_set_schedule(b"eager") == 0
    want = _ordered_stream_meter(hooks)
    assert want[0].any() and want[1].any() and (want[-1] > 0).all()              # (the last sorted key: true_peaks)
    failures = []
    for spec in ("lazy", "random:1", "random:2", "random:3"):
        assert hooks.smst_emu_set_schedule(spec.encode()) == 0
        try:
            got = _ordered_stream_meter(hooks)
            hooks.smst_emu_device_synchronize()
            _same(want, got)
        except AssertionError as e:
            failures.append("%s: %s" % (spec, e))
        finally:
            hooks.smst_emu_set_schedule(None)
    assert not failures, "\n".join(failures)
