"""Shared cases of the interleaved-PCM tests (test_pcm_emu.py on the CPU stand-in, test_pcm_gpu.py on the device).

Every comparison is exact: the conversion rule is deterministic (include/smst.h), and the planar float path is the reference for
the frame path -- the same engine on the same samples."""
import ctypes as C

import numpy as np

from conftest import package, synth_input

TILE = 512                      # frames one workgroup of kPcmIn / kPcmOut moves (kPcmTileFrames, csrc/smst_device.h)
S16, F32 = 1, 2
DTYPES = {S16: np.int16, F32: np.float32}
COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, TILE - 1, TILE, TILE + 1)
GEOMETRY = dict(block=512, interval=128)


def mirror_s16(x):
    """float -> int16 as include/smst.h states it, in float64: sign(v)*floor(|v| + 0.5) of v = x*32768 (ties away from zero), clamped
    to [-32768, 32767]; NaN -> 0."""
    x = np.asarray(x, np.float32)
    v = x.astype(np.float64)*32768.0
    with np.errstate(invalid="ignore"):
        q = np.sign(v)*np.floor(np.abs(v) + 0.5)
        q = np.clip(q, -32768.0, 32767.0)
    return np.where(np.isnan(v), 0.0, q).astype(np.int16)


def decode_s16(codes):
    return np.asarray(codes, np.int16).astype(np.float32)/np.float32(32768)


def aligned(n, dtype, offset=0):
    """n elements of dtype whose first one lies `offset` elements behind a 16-byte boundary"""
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n + offset + 16//item + 1, dtype)
    skip = (-raw.ctypes.data % 16)//item
    a = raw[skip + offset:skip + offset + n]
    assert a.ctypes.data % 16 == (offset*item) % 16
    return a


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def convert(lib, direction, fmt, counts, channels, src, src_ss, src_inner, dst, dst_ss, dst_inner):
    counts = np.ascontiguousarray(counts, np.int32)
    rc = lib.smst_debug_pcm_convert(0, direction, fmt, len(counts), channels, _ip(counts), C.c_void_p(src.ctypes.data), src_ss, src_inner,
                                    C.c_void_p(dst.ctypes.data), dst_ss, dst_inner)
    assert rc == 0, (lib.smst_last_error() or b"").decode()


def special_values():
    """(float32 values, what each must become): the ties, the value floorf(x + 0.5f) gets wrong, full scale, signed zero, NaN, the largest float"""
    q = [k + 0.5 for k in range(4)] + [float(np.float32(0.49999997)), 1.0, 1.5]
    vals = [s*np.float32(v)/np.float32(32768) for v in q for s in (1, -1)]
    vals += [s*np.float32(v) for v in (1.0, 1.5, 0.0, np.finfo(np.float32).max) for s in (1, -1)] + [np.float32(np.nan)]
    vals = np.array(vals, np.float32)
    anchors = {0: 1, 1: -1, 2: 2, 3: -2, 4: 3, 5: -3, 6: 4, 7: -4, 8: 0, 9: 0, 10: 1, 11: -1, 12: 2, 13: -2,
               14: 32767, 15: -32768, 16: 32767, 17: -32768, 18: 0, 19: 0, 20: 32767, 21: -32768, 22: 0}
    return vals, anchors


def _rng(*key):
    return np.random.Generator(np.random.PCG64(abs(hash(key)) % (2**32)))


def _pcm_values(fmt, n, rng):
    if fmt == S16:
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return rng.uniform(-1.5, 1.5, n).astype(np.float32)


def _planar_values(fmt, n, rng):
    x = rng.uniform(-1.1, 1.1, n).astype(np.float32)
    ties = (rng.integers(-40000, 40000, n).astype(np.float32) + np.float32(0.5))/np.float32(32768)
    x = np.where(rng.random(n) < 0.25, ties, x).astype(np.float32)
    vals, _ = special_values()
    x[:min(n, len(vals))] = vals[:min(n, len(vals))]
    return x


def check_converter(lib, channels, counts=COUNTS):
    """Both kernels, both formats, base pointer 0 / 1 element behind a 16-byte boundary, a stream stride that is a multiple of 16 bytes
    and one that is not, frameStride = C and C + 1: the converted samples, and every destination element the call does not own, untouched."""
    S, Cn, most = len(counts), channels, max(counts)
    for fmt in (S16, F32):
        dt = DTYPES[fmt]
        for offset in (0, 1):
            for fs in (Cn, Cn + 1):
                for odd_stride in (False, True):
                    pss = (most*fs + 7)//8*8 + (3 if odd_stride else 0)       # PCM side: elements between two streams
                    pcs, planar_ss = most + 3, Cn*(most + 3) + 5               # planar side: deliberately odd pitches
                    pcm_len, planar_len = (S - 1)*pss + (most - 1)*fs + Cn, (S - 1)*planar_ss + (Cn - 1)*pcs + most
                    rng = _rng(Cn, fmt, offset, fs, odd_stride)
                    where = dict(C=Cn, fmt=fmt, offset=offset, frame_stride=fs, stream_stride=pss)
                    # PCM -> planar
                    src = aligned(pcm_len, dt, offset)
                    src[:] = _pcm_values(fmt, pcm_len, rng)
                    dst = aligned(planar_len, np.float32, offset)
                    dst[:] = 777.0
                    want = dst.copy()
                    for s, n in enumerate(counts):
                        for c in range(Cn):
                            col = src[s*pss + c:s*pss + c + (n - 1)*fs + 1:fs] if n else src[:0]
                            want[s*planar_ss + c*pcs:s*planar_ss + c*pcs + n] = decode_s16(col) if fmt == S16 else col
                    convert(lib, 0, fmt, counts, Cn, src, pss, fs, dst, planar_ss, pcs)
                    assert np.array_equal(dst.view(np.uint32), want.view(np.uint32)), ("PCM -> planar", where)
                    # planar -> PCM
                    src = aligned(planar_len, np.float32, offset)
                    src[:] = _planar_values(fmt, planar_len, rng)
                    dst = aligned(pcm_len, dt, offset)
                    dst[:] = 0x5A5A if fmt == S16 else 777.0
                    want = dst.copy()
                    for s, n in enumerate(counts):
                        for c in range(Cn):
                            row = src[s*planar_ss + c*pcs:s*planar_ss + c*pcs + n]
                            if n:
                                want[s*pss + c:s*pss + c + (n - 1)*fs + 1:fs] = mirror_s16(row) if fmt == S16 else row
                    convert(lib, 1, fmt, counts, Cn, src, planar_ss, pcs, dst, pss, fs)
                    bits = np.uint16 if fmt == S16 else np.uint32
                    assert np.array_equal(dst.view(bits), want.view(bits)), ("planar -> PCM", where)


def check_special_values(lib):
    vals, anchors = special_values()
    n = len(vals)
    for Cn in (1, 2):
        for offset in (0, 1):
            frames = (n + Cn - 1)//Cn
            in_frame_order = np.zeros(frames*Cn, np.float32)
            in_frame_order[:n] = vals
            src = aligned(Cn*frames, np.float32)
            src[:] = in_frame_order.reshape(frames, Cn).T.reshape(-1)  # planar [C][frames]
            dst = aligned(frames*Cn, np.int16, offset)
            dst[:] = 0x5A5A
            convert(lib, 1, S16, [frames], Cn, src, Cn*frames, frames, dst, frames*Cn, Cn)
            got = dst[:n]
            assert np.array_equal(got, mirror_s16(vals)), (Cn, offset, got.tolist())
            for i, q in anchors.items():
                assert got[i] == q, (Cn, offset, i, float(vals[i]), int(got[i]), q)


def check_all_codes(lib):
    """int16 -> float -> int16 is the identity on all 65,536 codes, and the float is code/32768 exactly"""
    codes = aligned(65536, np.int16, 1)
    codes[:] = np.arange(-32768, 32768).astype(np.int16)
    planar = aligned(65536, np.float32)
    convert(lib, 0, S16, [32768], 2, codes, 65536, 2, planar, 65536, 32768)
    assert np.array_equal(planar.reshape(2, 32768).T.reshape(-1), np.arange(-32768, 32768, dtype=np.float64)/32768.0)
    back = aligned(65536, np.int16, 1)
    convert(lib, 1, S16, [32768], 2, planar, 65536, 32768, back, 65536, 2)
    assert np.array_equal(back, codes)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def frames_of(planar):
    """[S, C, n] -> [S, n, C], contiguous"""
    return np.ascontiguousarray(np.transpose(np.asarray(planar), (0, 2, 1)))


def inputs(S, Cn, n, fmt):
    """-> (frames [S, n, C] of the format, the planar float32 [S, C, n] they decode to)"""
    x = np.stack([synth_input(s, Cn, n, 48000) + 0.3*synth_input(s + 4, Cn, n, 48000) for s in range(S)]).astype(np.float32)
    if fmt == S16:
        codes = mirror_s16(x)
        return frames_of(codes), decode_s16(codes)
    return frames_of(x), x


def expect_frames(planar_out, fmt):
    f = frames_of(planar_out)
    return mirror_s16(f) if fmt == S16 else f


# (out, in) per stream and call.  The last three calls are there for the silence gate, which reads the call's input on a stream of its own:
# 1100 and then 300 silent frames -- the second of them is passed through and clears the streams' state --, then sound again.  A gate that
# read the input image before the conversion had filled it would see the previous call's samples and decide differently each time.
SESSION = dict(seek=[640, 640, 0], rates=[1.0, 0.8, 1.25],
               calls=[([700, 300, 0], [600, 300, 0]), ([129, 0, 515], [128, 5, 500]), ([1000, 64, 200], [900, 64, 210]),
                      ([1100]*3, [1100]*3), ([300]*3, [300]*3), ([600, 610, 77], [600, 600, 80])],
               silent=(3, 4), flush=[200, -1, 150])


def session_length():
    return max(SESSION["seek"]) + sum(max(nin) for _, nin in SESSION["calls"])


def session_inputs(Cn, fmt):
    """inputs() for the session, silent where SESSION says so"""
    frames, planar = inputs(3, Cn, session_length(), fmt)
    pos = max(SESSION["seek"])
    for k, (_, nin) in enumerate(SESSION["calls"]):
        if k in SESSION["silent"]:
            frames[:, pos:pos + max(nin)] = 0
            planar[:, :, pos:pos + max(nin)] = 0
        pos += max(nin)
    return frames, planar


def planar_session(lib, Cn, x, **kw):
    """seek, three process calls of unequal ragged sizes (with zeros), a flush with one negative count: the planar float API"""
    pkg = package()
    b = pkg.StretchBatch(3, Cn, lib=lib, **GEOMETRY, **kw)
    outs, pos = [], max(SESSION["seek"])
    b.seek(np.ascontiguousarray(x[:, :, :pos]), SESSION["rates"], in_samples=SESSION["seek"])
    for nout, nin in SESSION["calls"]:
        outs.append(np.array(b.process(np.ascontiguousarray(x[:, :, pos:pos + max(nin)]), nout, in_samples=nin), copy=True))
        pos += max(nin)
    outs.append(np.array(b.flush(SESSION["flush"]), copy=True))
    b.close()
    return outs


def frame_session(lib, Cn, frames, fmt, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """the same session through the frame methods; to_memory / to_host move a numpy array into the memory under test and back"""
    pkg = package()
    b = pkg.StretchBatch(3, Cn, lib=lib, **GEOMETRY)
    outs, pos = [], max(SESSION["seek"])
    b.seekFrames(to_memory(np.ascontiguousarray(frames[:, :pos])), SESSION["rates"], in_samples=SESSION["seek"])
    for nout, nin in SESSION["calls"]:
        outs.append(to_host(b.processFrames(to_memory(np.ascontiguousarray(frames[:, pos:pos + max(nin)])), nout, in_samples=nin)))
        pos += max(nin)
    like = to_memory(np.zeros((1,), np.float32))
    outs.append(to_host(b.flushFrames(SESSION["flush"], like=like, dtype=DTYPES[fmt])))
    b.close()
    return outs


def check_session(lib, Cn, fmt, **memory):
    frames, planar = session_inputs(Cn, fmt)
    want = planar_session(lib, Cn, planar)
    got = frame_session(lib, Cn, frames, fmt, **memory)
    assert len(want) == len(got)
    for k, (w, g) in enumerate(zip(want, got)):
        e = expect_frames(w, fmt)
        assert g.dtype == e.dtype and g.shape == e.shape, (k, g.dtype, g.shape, e.shape)
        assert np.array_equal(g.view(np.uint16 if fmt == S16 else np.uint32), e.view(np.uint16 if fmt == S16 else np.uint32)), ("call", k, "C", Cn, "format", fmt)
    assert any(np.any(g != 0) for g in got)  # (the session makes sound)
