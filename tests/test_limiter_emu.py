"""The limiter flag of the frame output (include/smst.h, "Limiter") on the CPU stand-in: the numpy mirror against the known answers, the
library's window against the formula, the two passes against the mirror bit for bit, NaN and inf, whole clips through exactFrames, the
clip-free ceilings, the opt-in, the steady state, the refusals and the command-line tool (tests/limiter_cases.py has the mirror and the
checks).  On a library without the limiter's entry points every test but the mirror's own fails at its first call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dither_cases as dc
import level_cases as lc
import limiter_cases as lm
import pcm_cases as pc
import pcm_format_cases as fc
import true_peak_cases as tp
from conftest import ROOT, package
from test_pcm_emu import hooks  # noqa: F401  (the fixture: the stream model's hooks bound, the eager schedule restored afterwards)
from test_stream_order_emu import _same


def test_mirror_known_answers():
    lm.check_mirror()


def test_clip_free_ceilings_of_the_mirror():
    lm.check_ceiling_table()


def test_limited_output_meets_its_ceiling():
    """the sample peak is bounded (asserted in the sweep); the true peak is a measured property, printed here: include/smst.h and EXPERIMENTS.md quote it"""
    for lookahead in (72, 36, 8, 1):
        print("H = %d: the worst true peak of the limited output exceeds its ceiling by %.3e" % (lookahead, lm.overshoot(lookahead)))


def test_window_against_formula(emu):
    lm.check_window(emu)


@pytest.mark.parametrize("lookahead", [1, 2, 72])
@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_passes_against_mirror(emu, channels, lookahead):
    lm.check_hook(emu, channels, lookahead)


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_passes_against_mirror_longest_lookahead(emu, channels):
    lm.check_hook(emu, channels, lm.MAX_H)


def test_mixed_batch(emu):
    lm.check_mixed(emu)


def test_nan_and_inf(emu):
    lm.check_nan_inf(emu)


def test_two_runs_are_bit_identical(emu):
    lm.check_reproducible(emu)
    lm.check_two_runs(emu)


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, False), (fc.S16, True), (fc.S24, False), (fc.S24, True), (fc.F32, False)])
def test_whole_clips(emu, fmt, dithered):
    lm.check_clips(emu, fmt, dithered)


def test_opt_in(emu):
    lm.check_opt_in(emu)


def test_steady_state(emu):
    lm.check_steady_state(emu)


def test_refusals(emu):
    lm.check_refusals(emu)


def test_flag_is_refused_in_streaming_calls(emu):
    lm.check_refused_in_streaming_calls(emu)


# ---- stream order: the device-memory exact call with the limiter's passes under the deferred schedules -------------------------------------

def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _ordered_limiter(lib):
    """Two exact calls in SMST_MEM_DEVICE with the levels and flags of limiter_cases.CLIP_LEVELS and the caller's own producer and consumer
    streams (test_true_peak_emu._ordered_true_peak): the two passes must find their place behind the engine's last emitting kernel, the
    loudness and the true-peak passes and in front of the limited kClipOut by stream order alone.  The output is read on the consumer only."""
    pkg = package()
    nin, nout = lm.CLIPS["inputs"], lm.CLIPS["outputs"]
    S, Cn, fmt = len(nin), 2, fc.S16
    planar = tp.clip_frames(fc.F32)[1]
    b = pkg.StretchBatch(S, Cn, lib=lib, seed=4, **pc.GEOMETRY)
    lm.set_clip_levels(b, lc.ceiling(fmt, True))
    b.setPcmDither(dc.TPDF, 8)
    prod, cons = lib.smst_emu_stream_create(), lib.smst_emu_stream_create()
    keep, results = [], []
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    for call in range(2):
        x = planar if call == 0 else np.ascontiguousarray(planar[::-1]*np.float32(0.5))
        n_in, n_out = (nin, nout) if call == 0 else (nin[::-1], nout[::-1])
        host = fc.encode_frames(pc.frames_of(x), fmt)
        dev = np.zeros_like(host)
        out = np.full((S, max(nout), Cn), 0x5A5A, host.dtype)
        for a in (dev, out):
            lib.smst_emu_register_device(_ptr(a), a.nbytes)
        lib.smst_emu_memcpy_async(_ptr(dev), _ptr(host), dev.nbytes, prod)
        assert lib.smst_batch_wait_for_stream(b.h, prod) == 0
        status = np.full(S, 99, np.int32)
        rc = lib.smst_batch_exact_pcm(b.h, _ptr(dev), Cn*dev.shape[1], Cn, ip(ints(n_in)), _ptr(out), Cn*out.shape[1], Cn, ip(ints(n_out)), ip(status), fmt, pkg.MEM_DEVICE)
        assert rc == 0, lib.smst_last_error()
        assert lib.smst_batch_signal_stream(b.h, cons) == 0
        y = np.zeros_like(out)
        lib.smst_emu_memcpy_async(_ptr(y), _ptr(out), out.nbytes, cons)
        lib.smst_emu_stream_synchronize(cons)
        results.extend([y, status])
        keep.extend([dev, out, host])
    results.extend(b.take_pcm_limiter())
    results.extend(b.take_pcm_peaks())
    results.append(b.takePcmOvers()[0])
    for a in keep[0::3] + keep[1::3]:
        lib.smst_emu_unregister_device(_ptr(a))
    lib.smst_emu_stream_destroy(prod)
    lib.smst_emu_stream_destroy(cons)
    b.close()
    return results


def test_device_memory_limiter_under_deferred_schedules(hooks):  # noqa: F811
    assert hooks.smst_emu_set_schedule(b"eager") == 0
    want = _ordered_limiter(hooks)
    assert want[0].any() and (want[4] < 1).any() and (want[5] > 0).any() and (want[7] > 1).any()  # (limited, at a gain its ceiling alone would not allow)
    failures = []
    for spec in ("lazy", "random:1", "random:2", "random:3"):
        assert hooks.smst_emu_set_schedule(spec.encode()) == 0
        try:
            got = _ordered_limiter(hooks)
            hooks.smst_emu_device_synchronize()
            _same(want, got)
        except AssertionError as e:
            failures.append("%s: %s" % (spec, e))
        finally:
            hooks.smst_emu_set_schedule(None)
    assert not failures, "\n".join(failures)


def test_cli_limit_emulated(emu, tmp_path):
    exe = str(tmp_path/"stretch_cli_emu")
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "tools", "stretch_cli.cpp"), "-o", exe, "-L" + emu_dir,
                    "-l:libsmst_emu.so", "-Wl,-rpath," + emu_dir], check=True)
    lm.check_cli(exe, tmp_path, emu)
