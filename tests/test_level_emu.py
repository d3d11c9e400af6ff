"""Per-stream gain, peak meters and clip-safe whole-clip gains of the frame output, on the CPU stand-in (tests/level_cases.py has the mirror
and the checks; every comparison with it is exact).  On a library without the level entry points every test but the ceiling sweep fails at
its first call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dither_cases as dc
import exact_cases as xc
import level_cases as lc
import pcm_cases as pc
import pcm_format_cases as fc
from conftest import ROOT, package
from test_pcm_emu import hooks  # noqa: F401  (the fixture: the stream model's hooks bound, the eager schedule restored afterwards)
from test_stream_order_emu import _same


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("fmt", lc.ALL_FORMATS)
def test_converter_against_mirror(emu, fmt, channels):
    lc.check_converter(emu, fmt, channels, (0, 1, 5) if fmt == fc.S24 else (0, fc.ELEM_BYTES[fmt]))


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", [fc.S16, fc.S24, fc.F32])
def test_clip_pair_against_mirror(emu, fmt, channels):
    lc.check_clip_pair(emu, fmt, channels)


@pytest.mark.parametrize("fmt,dithered", sorted(lc.CEILINGS))
def test_ceiling_table(emu, fmt, dithered):
    lc.check_ceiling_table(fmt, dithered)
    lc.check_ceiling_on_device(emu, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, False), (fc.S16, True), (fc.S24, True), (fc.F32, False)])
def test_session_equals_mirror_of_planar(emu, fmt, dithered):
    lc.check_session(emu, fmt, dithered)


def test_session_cut_into_other_calls(emu):
    lc.check_recut(emu, fc.S16)


def test_whole_clip_mode_is_refused_in_streaming_calls(emu):
    lc.check_whole_clip_mode_refused_in_streaming_calls(emu)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_whole_clips(emu, fmt, wide):
    lc.check_clips(emu, fmt, wide=wide)


@pytest.mark.parametrize("dithered", [False, True])
def test_opt_in(emu, dithered):
    lc.check_opt_in(emu, dithered)


def test_steady_state(emu):
    lc.check_steady_state(emu)


def test_refusals(emu):
    lc.check_refusals(emu)


# ---- stream order: the device-memory exact call with a whole-clip gain under the deferred schedules --------------------------------

def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _ordered_protect(lib):
    """Two exact calls in SMST_MEM_DEVICE with PROTECT / NORMALISE / FIXED over the streams and the caller's own producer and consumer
    streams (test_exact_emu._ordered_session): the memset of the clip peaks, kClipPeak and the levelled kClipOut must find their places
    behind the engine's last emitting kernel by stream order alone.  The output is read on the consumer only."""
    pkg = package()
    nin, nout = xc.CLIPS["inputs"], xc.CLIPS["outputs"]
    S, Cn, fmt = len(nin), 2, fc.S16
    planar = xc.clip_inputs(Cn, nin, loud=0)
    b = pkg.StretchBatch(S, Cn, lib=lib, seed=4, **xc.GEOMETRY)
    for s in range(S):
        b.set_pcm_level((lc.PROTECT, lc.NORMALISE, lc.FIXED)[s % 3], 0.75, lc.ceiling(fmt, True), stream=s)
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
    peaks, gains = b.take_pcm_peaks()
    results.extend([peaks, gains, b.takePcmOvers()[0]])
    for a in keep[0::3] + keep[1::3]:
        lib.smst_emu_unregister_device(_ptr(a))
    lib.smst_emu_stream_destroy(prod)
    lib.smst_emu_stream_destroy(cons)
    b.close()
    return results


def test_device_memory_protect_under_deferred_schedules(hooks):  # noqa: F811
    assert hooks.smst_emu_set_schedule(b"eager") == 0
    want = _ordered_protect(hooks)
    assert want[0].any() and (want[-3] > 0).sum() >= 4 and (want[-2] != 1).sum() >= 4 and not want[-1].any()    # (levelled clips, nothing clamped)
    failures = []
    for spec in ("lazy", "random:1", "random:2", "random:3"):
        assert hooks.smst_emu_set_schedule(spec.encode()) == 0
        try:
            got = _ordered_protect(hooks)
            hooks.smst_emu_device_synchronize()
            _same(want, got)
        except AssertionError as e:
            failures.append("%s: %s" % (spec, e))
        finally:
            hooks.smst_emu_set_schedule(None)
    assert not failures, "\n".join(failures)


def test_cli_level_emulated(emu, tmp_path):
    exe = str(tmp_path/"stretch_cli_emu")
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "tools", "stretch_cli.cpp"), "-o", exe, "-L" + emu_dir,
                    "-l:libsmst_emu.so", "-Wl,-rpath," + emu_dir], check=True)
    lc.check_cli(exe, tmp_path, emu)
