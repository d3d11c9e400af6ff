"""Shared cases of the packed int24 / int32 / float16 frame formats and of the overs counters (test_pcm_formats_emu.py on the CPU
stand-in, test_pcm_formats_gpu.py on the device), next to pcm_cases.py for int16 / float32.

Every comparison is exact -- bit patterns, any float16 NaN equal to any other --: the rule of include/smst.h is deterministic, and its
reference here is a float64 numpy mirror written from that text.  For sessions the reference is the planar float API on the same samples."""
import ctypes as C

import numpy as np

import pcm_cases as pc
from conftest import package

S16, F32, S24, S32, F16 = 1, 2, 4, 5, 6
NEW_FORMATS = (S24, S32, F16)
ELEM_BYTES = {S16: 2, F32: 4, S24: 3, S32: 4, F16: 2}
DTYPES = {S16: np.int16, F32: np.float32, S32: np.int32, F16: np.float16}       # (packed int24 has none: codes travel as int32 here)
FULL_SCALE = {S16: 2.0**15, S24: 2.0**23, S32: 2.0**31}
COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 47, 48, 49, 63, 64, 65, 511, 512, 513)
FLT_MAX = np.finfo(np.float32).max


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def mirror(x, fmt):
    """float32 -> (values of the format, clamped mask, NaN mask) as include/smst.h states it.
    Integer formats, in float64: q = sign(v)*floor(|v| + 0.5) of v = x*scale (ties away from zero; exact: x has 24 significant bits),
    clamped to [-scale, scale - 1], NaN -> 0; clamped = the clamp changed q.  float16: round to nearest even, subnormals kept, overflow
    to +-inf, NaN stays NaN -- numpy's own float32 -> float16; clamped = a finite value became +-inf.  float32: itself."""
    x = np.asarray(x, np.float32)
    nan = np.isnan(x)
    if fmt == F32:
        return x, np.zeros(x.shape, bool), nan
    if fmt == F16:
        with np.errstate(over="ignore"):
            h = x.astype(np.float16)
        return h, np.isfinite(x) & np.isinf(h), nan
    scale = FULL_SCALE[fmt]
    v = x.astype(np.float64)*scale
    with np.errstate(invalid="ignore"):
        q = np.sign(v)*np.floor(np.abs(v) + 0.5)
        c = np.clip(q, -scale, scale - 1)
    codes = np.where(nan, 0.0, c).astype(np.int64)
    return codes.astype(np.int16 if fmt == S16 else np.int32), ~nan & (q != c), nan


def decode(values, fmt):
    """values of the format -> float32 as include/smst.h states it (int32: numpy converts to float32 round-to-nearest-even)"""
    if fmt == F32:
        return np.asarray(values, np.float32)
    if fmt == F16:
        return np.asarray(values, np.float16).astype(np.float32)
    if fmt == S32:
        return np.asarray(values, np.int32).astype(np.float32)*np.float32(2.0**-31)
    return np.asarray(values).astype(np.float32)/np.float32(FULL_SCALE[fmt])


def to_rows(values, fmt):
    """values [n] of the format -> uint8 [n, element bytes]: the bytes in memory (int24: little-endian, the low three of the code)"""
    if fmt == S24:
        c = np.asarray(values, np.int32).reshape(-1)
        return np.stack([c & 255, (c >> 8) & 255, (c >> 16) & 255], -1).astype(np.uint8)
    return np.ascontiguousarray(values, DTYPES[fmt]).reshape(-1).view(np.uint8).reshape(-1, ELEM_BYTES[fmt])


def from_rows(rows, fmt):
    if fmt == S24:
        b = np.asarray(rows).astype(np.int32)
        v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
        return np.where(v & 0x800000, v - (1 << 24), v).astype(np.int32)
    return np.ascontiguousarray(rows).reshape(-1).view(DTYPES[fmt])


def same_values(a, b, fmt):
    """bit patterns equal; for float16 (a, b float16) and decoded float16 (float32) any NaN equals any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = {2: np.uint16, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]
    eq = a.view(bits) == b.view(bits)
    if fmt == F16 and a.dtype.kind == "f":
        eq |= np.isnan(a) & np.isnan(b)
    return bool(eq.all())


def byte_buffer(nbytes, offset):
    """nbytes of uint8 whose first one lies `offset` bytes behind a 16-byte boundary"""
    raw = np.zeros(nbytes + 32, np.uint8)
    skip = -raw.ctypes.data % 16
    a = raw[skip + offset:skip + offset + nbytes]
    assert a.ctypes.data % 16 == offset % 16
    return a


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def convert(lib, direction, fmt, counts, channels, src, src_ss, src_inner, dst, dst_ss, dst_inner, counted=False):
    counts = np.ascontiguousarray(counts, np.int32)
    if counted:
        f = lib.smst_debug_pcm_convert_counted
        f.restype, f.argtypes = C.c_int, [C.c_int]*4 + [C.POINTER(C.c_int), C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong, C.c_longlong,
                                                     C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        clamped, nans = np.full(len(counts), -1, np.int64), np.full(len(counts), -1, np.int64)
        rc = f(0, fmt, len(counts), channels, _ip(counts), C.c_void_p(src.ctypes.data), src_ss, src_inner, C.c_void_p(dst.ctypes.data), dst_ss, dst_inner, _lp(clamped), _lp(nans))
        assert rc == 0, (lib.smst_last_error() or b"").decode()
        return clamped, nans
    rc = lib.smst_debug_pcm_convert(0, direction, fmt, len(counts), channels, _ip(counts), C.c_void_p(src.ctypes.data), src_ss, src_inner,
                                    C.c_void_p(dst.ctypes.data), dst_ss, dst_inner)
    assert rc == 0, (fmt, (lib.smst_last_error() or b"").decode())


# ---- values --------------------------------------------------------------------------------------------------------------------------

def special_values(fmt):
    """(float32 values, {index: the code / float16 bit pattern it must become})"""
    f = np.float32
    if fmt == F16:
        table = [(65504.0, 0x7BFF), (65519.99, 0x7BFF), (65520.0, 0x7C00), (-65520.0, 0xFC00), (2.0**-24, 0x0001), (2.0**-25, 0x0000), (6e-8, 0x0001),
                 (-2.0**-24, 0x8001), (1.0 + 2.0**-11, 0x3C00), (1.0 + 3*2.0**-11, 0x3C02), (1.0, 0x3C00), (-1.0, 0xBC00), (1.5, 0x3E00), (-1.5, 0xBE00),
                 (0.0, 0x0000), (-0.0, 0x8000), (FLT_MAX, 0x7C00), (-FLT_MAX, 0xFC00), (np.inf, 0x7C00), (-np.inf, 0xFC00), (2.0**-14 - 2.0**-25, 0x0400),
                 (np.nan, None)]
        return np.array([v for v, _ in table], f), {i: a for i, (_, a) in enumerate(table) if a is not None}
    scale = f(FULL_SCALE[fmt])
    hi, lo = int(FULL_SCALE[fmt]) - 1, -int(FULL_SCALE[fmt])
    table = []
    for k in range(4):                                  # ties at +-(k + 0.5)/scale: away from zero
        table += [(f(k + 0.5)/scale, k + 1), (-f(k + 0.5)/scale, -(k + 1))]
    table += [(f(0.49999997)/scale, 0), (-f(0.49999997)/scale, 0), (f(1.0)/scale, 1), (-f(1.0)/scale, -1), (f(1.5)/scale, 2), (-f(1.5)/scale, -2)]
    table += [(1.0, hi), (-1.0, lo), (1.5, hi), (-1.5, lo), (0.0, 0), (-0.0, 0), (FLT_MAX, hi), (-FLT_MAX, lo), (np.inf, hi), (-np.inf, lo), (np.nan, 0)]
    if fmt == S32:
        table += [(np.nextafter(f(1.0), f(0.0)), 2147483520), (np.nextafter(f(-1.0), f(0.0)), -2147483520)]
        assert hi == 2147483647
    return np.array([v for v, _ in table], f), dict(enumerate(a for _, a in table))


def _pcm_values(fmt, n, rng):
    if fmt == S24:
        return rng.integers(-2**23, 2**23, n).astype(np.int32)
    if fmt == S32:
        return rng.integers(-2**31, 2**31, n).astype(np.int32)
    return rng.integers(0, 65536, n).astype(np.uint16).view(np.float16)  # every kind of half, NaN and inf among them


def _planar_values(fmt, n, rng):
    if fmt == F16:  # magnitudes from below the smallest subnormal to beyond the largest half
        x = (rng.uniform(-1.0, 1.0, n)*2.0**rng.integers(-28, 19, n)).astype(np.float32)
    else:
        x = rng.uniform(-1.1, 1.1, n).astype(np.float32)
        ties = (rng.integers(-40000, 40000, n).astype(np.float32) + np.float32(0.5))/np.float32(FULL_SCALE[fmt])
        x = np.where(rng.random(n) < 0.25, ties, x).astype(np.float32)
    vals, _ = special_values(fmt)
    x[:min(n, len(vals))] = vals[:min(n, len(vals))]
    return x


# ---- converter against mirror --------------------------------------------------------------------------------------------------------

def check_converter(lib, fmt, channels, byte_offsets, counts=COUNTS):
    """Both kernels of one format: the base pointer at every given byte offset behind a 16-byte boundary, a stream stride that is a multiple
    of 16 bytes and one that is not, frameStride = C and C + 1: the converted samples, and every destination byte the call does not own,
    untouched (sentinel fill).  The planar side's pitches are deliberately odd."""
    S, Cn, most, esz = len(counts), channels, max(counts), ELEM_BYTES[fmt]
    for offset in byte_offsets:
        for fs in (Cn, Cn + 1):
            for odd_stride in (False, True):
                pss = (most*fs + 15)//16*16 + (3 if odd_stride else 0)     # PCM side: elements between two streams
                assert (pss*esz % 16 != 0) == odd_stride
                pcs, planar_ss = most + 3, Cn*(most + 3) + 5
                pcm_len, planar_len = (S - 1)*pss + (most - 1)*fs + Cn, (S - 1)*planar_ss + (Cn - 1)*pcs + most
                rng = pc._rng(Cn, fmt, offset, fs, odd_stride)
                where = dict(C=Cn, fmt=fmt, byte_offset=offset, frame_stride=fs, stream_stride=pss)
                index = lambda s, c, n: np.arange(n)*fs + s*pss + c           # the elements of channel c of stream s
                # PCM -> planar
                src = byte_buffer(pcm_len*esz, offset)
                values = _pcm_values(fmt, pcm_len, rng)
                src.reshape(-1, esz)[:] = to_rows(values, fmt)
                dst = pc.aligned(planar_len, np.float32, 1)
                dst[:] = 777.0
                want = dst.copy()
                for s, n in enumerate(counts):
                    for c in range(Cn):
                        want[s*planar_ss + c*pcs:s*planar_ss + c*pcs + n] = decode(values[index(s, c, n)], fmt)
                convert(lib, 0, fmt, counts, Cn, src, pss, fs, dst, planar_ss, pcs)
                assert same_values(dst, want, fmt), ("PCM -> planar", where)
                # planar -> PCM
                src = pc.aligned(planar_len, np.float32, 1)
                src[:] = _planar_values(fmt, planar_len, rng)
                dst = byte_buffer(pcm_len*esz, offset)
                dst[:] = 0x5A
                want = dst.copy()
                rows = want.reshape(-1, esz)
                for s, n in enumerate(counts):
                    for c in range(Cn):
                        rows[index(s, c, n)] = to_rows(mirror(src[s*planar_ss + c*pcs:s*planar_ss + c*pcs + n], fmt)[0], fmt)
                convert(lib, 1, fmt, counts, Cn, src, planar_ss, pcs, dst, pss, fs)
                if fmt == F16:
                    assert same_values(from_rows(dst.reshape(-1, esz), fmt), from_rows(rows, fmt), fmt), ("planar -> PCM", where)
                else:
                    assert np.array_equal(dst, want), ("planar -> PCM", where)


def encode_run(lib, fmt, x, Cn=1, offset=0, counted=False):
    """x (float32, frame order) through kPcmOut as one dense stream of C channels -> the values of the format (and the counts)"""
    n, esz = len(x), ELEM_BYTES[fmt]
    assert n % Cn == 0
    frames = n//Cn
    src = pc.aligned(n, np.float32)
    src[:] = np.asarray(x, np.float32).reshape(frames, Cn).T.reshape(-1)    # planar [C][frames]
    dst = byte_buffer(n*esz, offset)
    dst[:] = 0x5A
    got = convert(lib, 1, fmt, [frames], Cn, src, n, frames, dst, n, Cn, counted=counted)
    values = from_rows(dst.reshape(-1, esz), fmt)
    return (values, got) if counted else values


def decode_run(lib, fmt, values, Cn=1, offset=0):
    """values of the format (frame order) through kPcmIn as one dense stream of C channels -> float32, frame order"""
    n, esz = len(values), ELEM_BYTES[fmt]
    assert n % Cn == 0
    frames = n//Cn
    src = byte_buffer(n*esz, offset)
    src.reshape(-1, esz)[:] = to_rows(values, fmt)
    dst = pc.aligned(n, np.float32)
    dst[:] = 777.0
    convert(lib, 0, fmt, [frames], Cn, src, n, Cn, dst, n, frames)
    return dst.reshape(Cn, frames).T.reshape(-1).copy()


def check_special_values(lib, fmt):
    vals, anchors = special_values(fmt)
    pad = np.zeros(-len(vals) % 2, np.float32)
    for Cn in (1, 2):
        for offset in (0, ELEM_BYTES[fmt]):
            got = encode_run(lib, fmt, np.concatenate([vals, pad]), Cn, offset)[:len(vals)]
            assert same_values(got, mirror(vals, fmt)[0], fmt), (fmt, Cn, offset, got.tolist())
            codes = got.view(np.uint16) if fmt == F16 else got
            for i, q in anchors.items():
                assert int(codes[i]) == q, (fmt, Cn, offset, i, float(vals[i]), int(codes[i]), q)
            if fmt == F16:
                assert np.isnan(got[-1])


def check_s24_codes(lib, codes):
    """int24 -> float -> int24 is the identity on the codes, and the float is code/8388608 exactly (one call per direction)"""
    codes = np.asarray(codes, np.int32)
    Cn = 2 if len(codes) % 2 == 0 else 1
    planar = decode_run(lib, S24, codes, Cn, offset=1)
    assert np.array_equal(planar, codes.astype(np.float64)/8388608.0)
    assert np.array_equal(encode_run(lib, S24, planar, Cn, offset=5), codes)


def check_f16_patterns(lib):
    """all 65,536 halves widen as numpy widens them; back is the identity on every pattern that is no NaN (and NaN stays NaN)"""
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    planar = decode_run(lib, F16, halves, 2, offset=2)
    assert same_values(planar, halves.astype(np.float32), F16)
    back = encode_run(lib, F16, planar, 2, offset=2)
    nan = np.isnan(halves)
    assert np.array_equal(back.view(np.uint16)[~nan], halves.view(np.uint16)[~nan]) and np.isnan(back[nan]).all() and nan.sum() == 2046


def check_s32_codes(lib):
    rng = pc._rng(9002)
    edge = [-2**31, -2**31 + 1, -1, 0, 1, 2**24, 2**24 + 1, 2**31 - 1 - 127, 2**31 - 1]
    codes = np.concatenate([np.array(edge, np.int64), rng.integers(-2**31, 2**31, 2**20)]).astype(np.int32)
    planar = decode_run(lib, S32, codes, 1, offset=4)
    want = codes.astype(np.float32)*np.float32(2.0**-31)
    assert np.array_equal(planar.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(encode_run(lib, S32, planar, 1, offset=4), mirror(want, S32)[0])
    assert planar[len(edge) - 1] == 1.0 and planar[0] == -1.0   # (INT32_MAX rounds up to 2^31: it comes back clamped)


# ---- overs ---------------------------------------------------------------------------------------------------------------------------

def check_overs_converter(lib, fmt, Cn=2):
    """kPcmOut's counts for planar inputs with a known number of values beyond full scale and of NaNs per stream -- one stream has none,
    one has no frames --, dense and strided, against the mirror's masks"""
    counts = [0, 513, 700, 1201]
    beyond = {S16: [1.5, -3.0, 1.0, np.inf], S24: [1.5, -3.0, 1.0, -np.inf], S32: [1.5, -3.0, 1.0, np.inf], F16: [70000.0, -1e6, 65520.0, FLT_MAX], F32: []}[fmt]
    planted = {0: (0, 0), 1: (0, 0), 2: (37, 5), 3: (301, 64)}                   # stream -> (values beyond full scale, NaNs)
    S, most = len(counts), max(counts)
    esz = ELEM_BYTES[fmt]
    for fs in (Cn, Cn + 1):
        rng = pc._rng(9001, fmt, fs)
        planar = rng.uniform(-0.9, 0.9, (S, Cn, most)).astype(np.float32)
        want_c, want_n = np.zeros(S, np.int64), np.zeros(S, np.int64)
        for s, n in enumerate(counts):
            k, m = planted[s]
            spots = rng.permutation(n*Cn)[:k + m]
            row = planar[s, :, :n].reshape(-1).copy()
            if beyond:
                row[spots[:k]] = np.resize(np.array(beyond, np.float32), k)
            row[spots[k:]] = np.nan
            planar[s, :, :n] = row.reshape(Cn, n)
            _, cm, nm = mirror(planar[s, :, :n], fmt)
            want_c[s], want_n[s] = cm.sum(), nm.sum()
            assert (want_c[s], want_n[s]) == ((k if beyond else 0), m)
        src = pc.aligned(planar.size, np.float32)
        src[:] = planar.reshape(-1)
        pss = most*fs + 3
        dst = byte_buffer(S*pss*esz, 1 if fmt == S24 else 0)
        clamped, nans = convert(lib, 1, fmt, counts, Cn, src, Cn*most, most, dst, pss, fs, counted=True)
        assert np.array_equal(clamped, want_c) and np.array_equal(nans, want_n), (fmt, fs, clamped.tolist(), want_c.tolist(), nans.tolist(), want_n.tolist())
        rows = dst[:((S - 1)*pss + (most - 1)*fs + Cn)*esz].reshape(-1, esz)     # (and the conversion itself is the plain call's)
        for s, n in enumerate(counts):
            for c in range(Cn):
                got = from_rows(rows[np.arange(n)*fs + s*pss + c], fmt)
                assert same_values(got, np.ascontiguousarray(mirror(planar[s, c, :n], fmt)[0]), fmt)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def encode_frames(x, fmt):
    """float32 [S, n, C] -> the frames the Python layer takes for the format (packed int24: uint8 [S, n, C, 3])"""
    v = mirror(x, fmt)[0]
    return to_rows(v, S24).reshape(v.shape + (3,)) if fmt == S24 else np.ascontiguousarray(v)


def decode_frames(frames, fmt):
    return decode(from_rows(frames, S24), fmt) if fmt == S24 else decode(frames, fmt)


def frame_dtype(fmt):
    return "s24" if fmt == S24 else DTYPES[fmt]


def session_inputs(Cn, fmt, gains=None):
    """-> (frames of the format for pc.SESSION, the planar float32 [S, C, n] they decode to); gains: a factor per stream"""
    x, _ = pc.session_inputs(Cn, pc.F32)
    if gains is not None:
        x = x*np.asarray(gains, np.float32)[:, None, None]
    frames = encode_frames(x, fmt)
    return frames, np.ascontiguousarray(np.transpose(decode_frames(frames, fmt), (0, 2, 1)))


def frame_session(lib, Cn, frames, fmt, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True), batch=None):
    """pc.SESSION through the frame methods (pc.frame_session for any format)"""
    b = batch or package().StretchBatch(3, Cn, lib=lib, **pc.GEOMETRY)
    outs, pos = [], max(pc.SESSION["seek"])
    b.seekFrames(to_memory(np.ascontiguousarray(frames[:, :pos])), pc.SESSION["rates"], in_samples=pc.SESSION["seek"])
    for nout, nin in pc.SESSION["calls"]:
        outs.append(to_host(b.processFrames(to_memory(np.ascontiguousarray(frames[:, pos:pos + max(nin)])), nout, in_samples=nin)))
        pos += max(nin)
    outs.append(to_host(b.flushFrames(pc.SESSION["flush"], like=to_memory(np.zeros((1,), np.float32)), dtype=frame_dtype(fmt))))
    if batch is None:
        b.close()
    return outs


def session_counts():
    """the output frames per stream of every call of frame_session (a negative flush count writes nothing)"""
    return [nout for nout, _ in pc.SESSION["calls"]] + [[max(n, 0) for n in pc.SESSION["flush"]]]


def check_session(lib, Cn, fmt, **memory):
    frames, planar = session_inputs(Cn, fmt)
    want = pc.planar_session(lib, Cn, planar)
    got = frame_session(lib, Cn, frames, fmt, **memory)
    assert len(want) == len(got)
    for k, (w, g) in enumerate(zip(want, got)):
        e = encode_frames(pc.frames_of(w), fmt)
        assert g.dtype == e.dtype and g.shape == e.shape, (k, g.dtype, g.shape, e.dtype, e.shape)
        assert same_values(g, e, fmt), ("call", k, "C", Cn, "format", fmt)
    assert any(np.any(g != 0) for g in got)  # (the session makes sound)


def check_session_overs(lib, fmt, factor=4.0):
    """pc.SESSION with stream 0 scaled by `factor` and stream 1 by 0.25: takePcmOvers() is the number of elements the mirror clamps in the
    planar session's output of the same calls -- some for the loud stream, none for the quiet one --, a second take is zero, and neither
    the takes nor a further call allocate."""
    Cn = 2
    frames, planar = session_inputs(Cn, fmt, gains=[factor, 0.25, 1.0])
    want = pc.planar_session(lib, Cn, planar)
    expect = np.zeros(3, np.int64)
    for w, counts in zip(want, session_counts()):
        for s, n in enumerate(counts):
            _, cm, nm = mirror(w[s, :, :n], fmt)
            expect[s] += cm.sum()
            assert not nm.any()
    b = package().StretchBatch(3, Cn, lib=lib, **pc.GEOMETRY)
    assert b.takePcmOvers()[0].tolist() == [0, 0, 0]
    got = frame_session(lib, Cn, frames, fmt, batch=b)
    for w, g in zip(want, got):
        assert same_values(g, encode_frames(pc.frames_of(w), fmt), fmt)
    before = b.allocation_events()
    clamped, nans = b.takePcmOvers()
    assert clamped.dtype == np.int64 and nans.dtype == np.int64
    assert clamped.tolist() == expect.tolist() and nans.tolist() == [0, 0, 0], (clamped.tolist(), expect.tolist(), nans.tolist())
    assert clamped[0] > 0 and clamped[1] == 0, clamped.tolist()
    again = b.takePcmOvers()
    assert again[0].tolist() == [0, 0, 0] and again[1].tolist() == [0, 0, 0]
    b.processFrames(np.ascontiguousarray(frames[:, :600]), [600, 300, 0])       # (sizes the session has used)
    b.takePcmOvers()
    assert b.allocation_events() == before
    b.close()
