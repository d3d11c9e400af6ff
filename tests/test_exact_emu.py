"""Whole clips of ragged lengths and rates in one call (smst_batch_exact / smst_batch_exact_pcm, include/smst.h) on the CPU stand-in: the two
copy kernels against a numpy mirror, the batch call against S single-stream handles and the compiled reference, masks, frames, refusals,
allocations, and the order of the copy kernels against the engine's streams on the deferred-stream model.  Every comparison is exact (the
reference leg has parity_cases' caps)."""
import ctypes as C

import numpy as np
import pytest

import exact_cases as xc
import pcm_cases as pc
import pcm_format_cases as pf
from conftest import package
from test_pcm_emu import hooks  # noqa: F401  (the fixture: the stream model's hooks bound, the eager schedule restored afterwards)
from test_stream_order_emu import SCHEDULES, _same

FORMATS = (xc.PLANAR,) + xc.FRAME_FORMATS


# ---- 1. the copy kernels --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", FORMATS)
def test_clip_kernels_against_mirror(emu, fmt, channels):
    sweep = channels == 2                                # every alignment of the caller's buffer with every alignment of the image
    xc.check_clip_kernels(emu, fmt, channels, xc.sub_alignments(fmt) if sweep else (0, 4 if fmt == xc.PLANAR else pf.ELEM_BYTES[fmt]),
                          image_offsets=xc.IMAGE_ALIGNMENTS if sweep else (1,))


@pytest.mark.parametrize("fmt", xc.FRAME_FORMATS)
def test_clip_kernels_with_wide_frames(emu, fmt):
    xc.check_clip_kernels(emu, fmt, 2, (0, pf.ELEM_BYTES[fmt]), wide_frames=True)


def test_clip_copy_rejects_bad_arguments(emu):
    a, b = np.zeros(64, np.int16), np.zeros(64, np.float32)
    segs = np.zeros((1, 2, 4), np.int32)
    segs[0, 0] = (0, 0, 4, 0)
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int))
    call = lambda fmt, fs, t=segs: emu.smst_debug_clip_copy(0, 0, fmt, 1, 2, ip(t), C.c_void_p(a.ctypes.data), 8, fs, C.c_void_p(b.ctypes.data), 16, 8, None, None)
    assert call(pf.S16, 2) == 0
    assert call(3, 2) == -1 and b"format" in emu.smst_last_error()
    assert call(pf.S16, 1) == -1 and b"frame stride" in emu.smst_last_error()
    bad = segs.copy()
    bad[0, 1] = (0, -1, 4, 0)
    assert call(pf.S16, 2, bad) == -1 and b"negative" in emu.smst_last_error()


# ---- 2. the batch call against single handles and the reference -----------------------------------------------------------------------

def _device_exact(lib, batch, x, nout, nin, frames=False):
    """the device-memory call on the stand-in, where a numpy array is device memory: eager schedule, synchronised before the read"""
    S = batch.streams
    fmt = batch._describe_frames(x, "input")[4] if frames else None
    out = batch._new_frames(max(max(nout), 1), fmt, None) if frames else np.zeros((S, batch.channels, max(max(nout), 1)), np.float32)
    d_in = batch._describe_frames(x, "input") if frames else batch._describe(x, "input")
    d_out = batch._describe_frames(out, "output") if frames else batch._describe(out, "output")
    nin, nout = np.ascontiguousarray(nin, np.int32), np.ascontiguousarray(nout, np.int32)
    status = np.full(S, 1, np.int32)
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int))
    if frames:
        rc = lib.smst_batch_exact_pcm(batch.h, d_in[0], d_in[1], d_in[2], ip(nin), d_out[0], d_out[1], d_out[2], ip(nout), ip(status), fmt, 1)
    else:
        rc = lib.smst_batch_exact(batch.h, d_in[0], d_in[1], d_in[2], ip(nin), d_out[0], d_out[1], d_out[2], ip(nout), ip(status), 1)
    assert rc == 0, lib.smst_last_error()
    batch.synchronize()
    return out, status == 0


def _run(emu, memory):
    return xc.host_exact if memory == "host" else (lambda b, x, nout, nin, frames=False: _device_exact(emu, b, x, nout, nin, frames))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("memory", ["host", "device"])
def test_exact_equals_single_handles(emu, memory, split):
    xc.check_equals_single_handles(emu, 2, xc.CLIPS, split, run=_run(emu, memory))


def test_exact_equals_single_handles_three_channels(emu):
    xc.check_equals_single_handles(emu, 3, xc.CLIPS_UNITY, False)


@pytest.mark.parametrize("split", [False, True])
def test_exact_against_the_reference(emu, ref, split):
    if getattr(ref, "is_port", False):
        pytest.skip("the plain port does not restate exact()")
    xc.check_against_reference(emu, ref, split)


# ---- 3. masks -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", [False, True])
def test_short_and_left_out_streams_keep_their_state(emu, split):
    xc.check_masks(emu, split)


# ---- 4. frames ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("fmt", xc.FRAME_FORMATS)
def test_exact_frames_equal_planar(emu, fmt, memory):
    run = _run(emu, memory)
    xc.check_frames_equal_planar(emu, fmt, run_frames=lambda b, x, nout, nin: run(b, x, nout, nin, frames=True))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------

def test_exact_refusals(emu):
    xc.check_refusals(emu)


# ---- 6. steady state and accounting ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("frames", [False, True])
def test_exact_does_not_allocate_in_steady_state(emu, frames, memory):
    run = _run(emu, memory)
    xc.check_steady_state(emu, lambda b, x, nout, nin: run(b, x, nout, nin, frames=frames), frames=frames)


def test_exact_runs_one_main_process(emu):
    xc.check_one_main_process(emu, _run(emu, "device"))


# ---- 7. stream order: the device-memory call under the deferred schedules -------------------------------------------------------------

def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _ordered_session(lib, fmt):
    """Two exact calls in SMST_MEM_DEVICE with the caller's own producer and consumer streams: the producer uploads the clips, the batch
    waits for it (smst_batch_wait_for_stream), the consumer -- ordered behind the batch by smst_batch_signal_stream -- copies the output
    out.  The output is read on the consumer only, never after smst_batch_synchronize."""
    pkg = package()
    nin, nout = xc.CLIPS["inputs"], xc.CLIPS["outputs"]
    S, Cn = len(nin), 2
    planar = xc.clip_inputs(Cn, nin)
    b = pkg.StretchBatch(S, Cn, lib=lib, seed=4, **xc.GEOMETRY)
    prod, cons = lib.smst_emu_stream_create(), lib.smst_emu_stream_create()
    keep, results = [], []
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    for call in range(2):
        x = planar if call == 0 else np.ascontiguousarray(planar[::-1]*np.float32(0.5))
        n_in, n_out = (nin, nout) if call == 0 else (nin[::-1], nout[::-1])
        host = x if fmt == xc.PLANAR else pf.encode_frames(pc.frames_of(x), fmt)
        dev = np.zeros_like(host)
        out = np.full((S, Cn, max(nout)) if fmt == xc.PLANAR else (S, max(nout), Cn), 777.0 if fmt == xc.PLANAR else 0x5A5A, host.dtype)
        for a in (dev, out):
            lib.smst_emu_register_device(_ptr(a), a.nbytes)
        lib.smst_emu_memcpy_async(_ptr(dev), _ptr(host), dev.nbytes, prod)
        assert lib.smst_batch_wait_for_stream(b.h, prod) == 0
        status = np.full(S, 99, np.int32)
        if fmt == xc.PLANAR:
            rc = lib.smst_batch_exact(b.h, _ptr(dev), Cn*dev.shape[2], dev.shape[2], ip(ints(n_in)), _ptr(out), Cn*out.shape[2], out.shape[2], ip(ints(n_out)), ip(status), pkg.MEM_DEVICE)
        else:
            rc = lib.smst_batch_exact_pcm(b.h, _ptr(dev), Cn*dev.shape[1], Cn, ip(ints(n_in)), _ptr(out), Cn*out.shape[1], Cn, ip(ints(n_out)), ip(status), fmt, pkg.MEM_DEVICE)
        assert rc == 0, lib.smst_last_error()
        assert lib.smst_batch_signal_stream(b.h, cons) == 0
        y = np.zeros_like(out)
        lib.smst_emu_memcpy_async(_ptr(y), _ptr(out), out.nbytes, cons)
        lib.smst_emu_stream_synchronize(cons)
        results.extend([y, status])
        keep.extend([dev, out, host])
    lib.smst_emu_device_synchronize()
    for a in keep[0::3] + keep[1::3]:
        lib.smst_emu_unregister_device(_ptr(a))
    lib.smst_emu_stream_destroy(prod)
    lib.smst_emu_stream_destroy(cons)
    results.append([[b.debug_state(s, w) for w in (0, 1, 2, 3)] for s in range(S)])
    b.close()
    return results


@pytest.mark.parametrize("fmt", [xc.PLANAR, pf.S16])
def test_device_memory_exact_under_deferred_schedules(hooks, fmt):  # noqa: F811
    assert hooks.smst_emu_set_schedule(b"eager") == 0
    want = _ordered_session(hooks, fmt)
    # the eager device-memory run is the host-memory call, with the caller's sentinel behind every stream's count
    nin, nout = xc.CLIPS["inputs"], xc.CLIPS["outputs"]
    planar = xc.clip_inputs(2, nin)
    b = package().StretchBatch(len(nin), 2, lib=hooks, seed=4, **xc.GEOMETRY)
    host, ok = xc.host_exact(b, planar if fmt == xc.PLANAR else pf.encode_frames(pc.frames_of(planar), fmt), nout, nin, frames=fmt != xc.PLANAR)
    b.close()
    assert want[1].tolist() == [0 if k else xc.ERR_SHORT for k in ok]
    for s, n in enumerate(nout):
        if fmt == xc.PLANAR:
            assert np.array_equal(want[0][s, :, :n], host[s, :, :n]) and (want[0][s, :, n:] == 777.0).all()
        else:
            assert np.array_equal(want[0][s, :n], host[s, :n]) and (want[0][s, n:] == 0x5A5A).all()
    failures = []
    for spec in SCHEDULES:
        assert hooks.smst_emu_set_schedule(spec.encode()) == 0
        try:
            got = _ordered_session(hooks, fmt)
            hooks.smst_emu_device_synchronize()
            _same(want, got)
        except AssertionError as e:
            failures.append("%s: %s" % (spec, e))
        finally:
            hooks.smst_emu_set_schedule(None)
    assert not failures, "\n".join(failures)
