"""Interleaved PCM through the batch API (smst_batch_*_pcm, include/smst.h) on the CPU stand-in: the two conversion kernels against a
float64 mirror of the stated rule, the frame calls against the planar calls on the same samples, the staging's allocations, and the
ordering of the two kernels against the engine's streams on the deferred-stream model.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import pcm_cases as pc
from conftest import package
from test_stream_order_emu import SCHEDULES, _same


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8, 16])
def test_converter_against_mirror(emu, channels):
    pc.check_converter(emu, channels)


def test_converter_special_values(emu):
    pc.check_special_values(emu)


def test_converter_all_int16_codes_round_trip(emu):
    pc.check_all_codes(emu)


def test_converter_rejects_bad_arguments(emu):
    a, b = np.zeros(64, np.int16), np.zeros(64, np.float32)
    n = np.array([4], np.int32)
    call = lambda fmt, fs, src=a: emu.smst_debug_pcm_convert(0, 0, fmt, 1, 2, n.ctypes.data_as(C.POINTER(C.c_int)), C.c_void_p(src.ctypes.data if src is not None else None), 8, fs, C.c_void_p(b.ctypes.data), 16, 8)
    assert call(pc.S16, 2) == 0
    assert call(3, 2) == -1 and b"format" in emu.smst_last_error()
    assert call(pc.S16, 1) == -1 and b"frame stride" in emu.smst_last_error()
    assert call(pc.S16, 2, None) == -1


@pytest.mark.parametrize("fmt", [pc.F32, pc.S16])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_session_equals_planar(emu, channels, fmt):
    pc.check_session(emu, channels, fmt)


def test_frame_calls_reject_bad_arguments(emu):
    pkg = package()
    b = pkg.StretchBatch(2, 2, lib=emu, **pc.GEOMETRY)
    x = np.zeros((2, 64, 2), np.int16)
    n = np.array([64, 64], np.int32)
    ip = n.ctypes.data_as(C.POINTER(C.c_int))
    px, null = C.c_void_p(x.ctypes.data), C.c_void_p(None)
    assert emu.smst_batch_process_pcm(b.h, px, 128, 2, ip, px, 128, 2, ip, 7, pkg.MEM_HOST) == -1 and b"format" in emu.smst_last_error()
    assert emu.smst_batch_process_pcm(b.h, px, 128, 1, ip, px, 128, 2, ip, pc.S16, pkg.MEM_HOST) == -1 and b"frame stride" in emu.smst_last_error()
    assert emu.smst_batch_process_pcm(b.h, null, 128, 2, ip, px, 128, 2, ip, pc.S16, pkg.MEM_HOST) == -1 and b"null buffer" in emu.smst_last_error()
    assert emu.smst_batch_seek_pcm(b.h, null, 128, 2, ip, None, pc.S16, pkg.MEM_HOST) == -1
    assert emu.smst_batch_flush_pcm(b.h, null, 128, 2, ip, None, pc.S16, pkg.MEM_HOST) == -1
    assert emu.smst_batch_output_seek_pcm(b.h, px, 128, 1, ip, pc.F32, pkg.MEM_HOST) == -1
    b.close()


def test_strided_frames_in_host_memory(emu):
    """frameStride > C in host memory (gathered frame by frame): the same result as dense frames, the gaps of the output untouched"""
    pkg = package()
    S, Cn, n = 3, 2, 700
    frames, _ = pc.inputs(S, Cn, n, pc.S16)
    wide_in = np.zeros((S, n, Cn + 1), np.int16)
    wide_in[:, :, :Cn] = frames
    wide_out = np.full((S, n, Cn + 1), 0x5A5A, np.int16)
    b1, b2 = (pkg.StretchBatch(S, Cn, lib=emu, **pc.GEOMETRY) for _ in range(2))
    dense = b1.processFrames(frames, [n, 300, 0])
    b2.processFrames(wide_in[:, :, :Cn], [n, 300, 0], out=wide_out[:, :, :Cn])
    assert np.array_equal(wide_out[0, :, :Cn], dense[0]) and np.array_equal(wide_out[1, :300, :Cn], dense[1, :300])
    assert (wide_out[:, :, Cn] == 0x5A5A).all() and (wide_out[1, 300:] == 0x5A5A).all() and (wide_out[2] == 0x5A5A).all()
    b1.close()
    b2.close()


def test_silence_passes_the_codes_through(emu):
    """Input below the noise floor for longer than the silence threshold (2 blocks) is passed through (kPassThrough): the int16 codes come
    back as they went in, and nothing is written behind a stream's count."""
    pkg = package()
    S, Cn, n = 3, 2, 3*512
    b = pkg.StretchBatch(S, Cn, lib=emu, **pc.GEOMETRY)
    x = np.zeros((S, n, Cn), np.int16)
    b.processFrames(x, n)                                       # the silence counter passes 2 blocks
    out = np.full((S, 300, Cn), 0x5A5A, np.int16)
    b.processFrames(x[:, :300], [300, 100, 0], out=out)
    assert (out[0] == 0).all() and (out[1, :100] == 0).all() and (out[1, 100:] == 0x5A5A).all() and (out[2] == 0x5A5A).all()
    b.close()


@pytest.mark.parametrize("fmt", [pc.F32, pc.S16])
def test_output_seek_equals_planar(emu, fmt):
    pkg = package()
    S, Cn = 3, 2
    frames, planar = pc.inputs(S, Cn, 3000, fmt)
    lengths = [1500, 900, 600]
    a, b = (pkg.StretchBatch(S, Cn, lib=emu, **pc.GEOMETRY) for _ in range(2))
    a.outputSeek(np.ascontiguousarray(planar[:, :, :1500]), lengths)
    b.outputSeekFrames(np.ascontiguousarray(frames[:, :1500]), lengths)
    want = a.process(np.ascontiguousarray(planar[:, :, 1500:2500]), [1100, 1000, 0])
    got = b.processFrames(np.ascontiguousarray(frames[:, 1500:2500]), [1100, 1000, 0])
    assert np.array_equal(got, pc.expect_frames(want, fmt)) and np.any(got != 0)
    a.close()
    b.close()


@pytest.mark.parametrize("fmt", [pc.F32, pc.S16])
def test_frame_calls_do_not_allocate_in_steady_state(emu, fmt):
    pkg = package()
    S, Cn, n = 3, 2, 1400
    frames, _ = pc.inputs(S, Cn, 5*n, fmt)
    b = pkg.StretchBatch(S, Cn, lib=emu, **pc.GEOMETRY)
    out = np.zeros((S, n + 100, Cn), pc.DTYPES[fmt])
    for k in range(2):  # (both sets of count tables have been used after two calls)
        b.processFrames(frames[:, k*n:(k + 1)*n], n + 100, out=out)
    before = b.allocation_events()
    for k in range(2, 5):
        b.processFrames(frames[:, k*n:(k + 1)*n], n + 100, out=out)
    assert b.allocation_events() == before


# ---- stream order: the device-memory frame calls under the deferred schedules -----------------------------------------------------

@pytest.fixture
def hooks(emu):
    sigs = {
        "smst_emu_set_schedule": (C.c_int, [C.c_char_p]),
        "smst_emu_stream_create": (C.c_void_p, []),
        "smst_emu_stream_destroy": (None, [C.c_void_p]),
        "smst_emu_stream_synchronize": (C.c_int, [C.c_void_p]),
        "smst_emu_device_synchronize": (C.c_int, []),
        "smst_emu_memcpy_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
        "smst_emu_register_device": (None, [C.c_void_p, C.c_size_t]),
        "smst_emu_unregister_device": (None, [C.c_void_p]),
    }
    for name, (res, args) in sigs.items():
        f = getattr(emu, name)
        f.restype, f.argtypes = res, args
    yield emu
    emu.smst_emu_set_schedule(None)  # back to the eager schedule


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _device_session(lib, fmt):
    """pc.SESSION in SMST_MEM_DEVICE with the caller's own producer and consumer streams: the producer uploads each call's frames, the
    batch waits for it, and the consumer -- ordered after the batch by smst_batch_signal_stream -- copies the frames out.  The output is
    read on the consumer only, never after smst_batch_synchronize."""
    pkg = package()
    S, Cn, dt = 3, 2, pc.DTYPES[fmt]
    frames, _ = pc.session_inputs(Cn, fmt)
    b = pkg.StretchBatch(S, Cn, lib=lib, **pc.GEOMETRY)
    prod, cons = lib.smst_emu_stream_create(), lib.smst_emu_stream_create()
    keep, results = [], []
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))

    def upload(host):
        dev = np.zeros_like(host)
        lib.smst_emu_register_device(_ptr(dev), dev.nbytes)
        lib.smst_emu_memcpy_async(_ptr(dev), _ptr(host), dev.nbytes, prod)
        assert lib.smst_batch_wait_for_stream(b.h, prod) == 0
        keep.extend([dev, host])
        return dev

    def download(dev):
        assert lib.smst_batch_signal_stream(b.h, cons) == 0
        y = np.zeros_like(dev)
        lib.smst_emu_memcpy_async(_ptr(y), _ptr(dev), dev.nbytes, cons)
        lib.smst_emu_stream_synchronize(cons)
        results.append(y)

    def output(n):
        dev = np.full((S, max(max(n), 1), Cn), 0x5A5A if fmt == pc.S16 else 777.0, dt)
        lib.smst_emu_register_device(_ptr(dev), dev.nbytes)
        keep.append(dev)
        return dev

    pos = max(pc.SESSION["seek"])
    dx = upload(np.ascontiguousarray(frames[:, :pos]))
    rates = np.asarray(pc.SESSION["rates"], np.float64)
    assert lib.smst_batch_seek_pcm(b.h, _ptr(dx), pos*Cn, Cn, ip(ints(pc.SESSION["seek"])), rates.ctypes.data_as(C.POINTER(C.c_double)), fmt, pkg.MEM_DEVICE) == 0
    for nout, nin in pc.SESSION["calls"]:
        n = max(nin)
        dx, dy = upload(np.ascontiguousarray(frames[:, pos:pos + n])), output(nout)
        pos += n
        assert lib.smst_batch_process_pcm(b.h, _ptr(dx), n*Cn, Cn, ip(ints(nin)), _ptr(dy), dy.shape[1]*Cn, Cn, ip(ints(nout)), fmt, pkg.MEM_DEVICE) == 0
        download(dy)
    dy = output(pc.SESSION["flush"])
    assert lib.smst_batch_flush_pcm(b.h, _ptr(dy), dy.shape[1]*Cn, Cn, ip(ints(pc.SESSION["flush"])), None, fmt, pkg.MEM_DEVICE) == 0
    download(dy)
    lib.smst_emu_device_synchronize()
    for a in keep:
        lib.smst_emu_unregister_device(_ptr(a))
    lib.smst_emu_stream_destroy(prod)
    lib.smst_emu_stream_destroy(cons)
    results.append([[b.debug_state(s, w) for w in (0, 1, 2, 3)] for s in range(S)])
    b.close()
    return results


@pytest.mark.parametrize("fmt", [pc.F32, pc.S16])
def test_device_memory_frames_under_deferred_schedules(hooks, fmt):
    assert hooks.smst_emu_set_schedule(b"eager") == 0
    want = _device_session(hooks, fmt)
    # the eager device-memory run is the host-memory session, with the caller's sentinel behind every stream's count
    host = pc.frame_session(hooks, 2, pc.session_inputs(2, fmt)[0], fmt)
    counts = [c[0] for c in pc.SESSION["calls"]] + [pc.SESSION["flush"]]
    for w, h, n in zip(want, host, counts):
        for s in range(3):
            assert np.array_equal(w[s, :max(n[s], 0)], h[s, :max(n[s], 0)])
            assert (w[s, max(n[s], 0):] == (0x5A5A if fmt == pc.S16 else 777.0)).all()
    failures = []
    for spec in SCHEDULES:
        assert hooks.smst_emu_set_schedule(spec.encode()) == 0
        try:
            got = _device_session(hooks, fmt)
            hooks.smst_emu_device_synchronize()
            _same(want, got)
        except AssertionError as e:
            failures.append("%s: %s" % (spec, e))
        finally:
            hooks.smst_emu_set_schedule(None)
    assert not failures, "\n".join(failures)
