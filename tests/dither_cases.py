"""Shared cases of the TPDF dither of the int16 / int24 output (test_dither_emu.py on the CPU stand-in, test_dither_gpu.py on the device),
next to pcm_cases.py and pcm_format_cases.py.

The numpy mirror below restates the "Dither" section of include/smst.h: 32-bit wrapping integer arithmetic for the noise, ONE float32
addition t = v*scale + d, rounding half away from zero.  Every comparison with it is exact -- bytes and counters."""
import ctypes as C
import struct
import subprocess

import numpy as np

import pcm_cases as pc
import pcm_format_cases as fc
from conftest import package, synth_input

NONE, TPDF, HP = 0, 1, 2
MODES = (TPDF, HP)
DITHERED_FORMATS = (fc.S16, fc.S24)
FIRST_FRAMES = (0, 1, 2**32 - 3)            # (hi32(n) changes inside a run that begins at the last one)
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def mix(x):
    """uint64 arrays that hold 32-bit words (every product stays below 2^64)"""
    x = np.asarray(x, np.uint64) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x*np.uint64(0x7feb352d)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x*np.uint64(0x846ca68b)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def stream_hash(seed):
    d = int(seed) & M64
    return int(mix(int(mix((d & M32) ^ 0x736d7374)) ^ (d >> 32)))


def key(seed, c):
    return int(mix((stream_hash(seed) + 0x9E3779B9*(c + 1)) & M32))


def frame_indices(first, count):
    """first, first + 1, ... modulo 2^64, uint64"""
    return np.uint64(int(first) & M64) + np.arange(count, dtype=np.uint64)


def word(seed, c, n, j):
    n = np.atleast_1d(np.asarray(n, np.uint64))
    lo, hi = n & np.uint64(M32), n >> np.uint64(32)
    step = (np.uint64(0x85EBCA6B)*((np.uint64(2)*hi + np.uint64(j + 1)) & np.uint64(M32))) & np.uint64(M32)
    return mix(mix(np.uint64(key(seed, c)) ^ lo) + step)


def unit(seed, c, n, j):
    return (word(seed, c, n, j) >> np.uint64(8)).astype(np.float32)*np.float32(2.0**-24) - np.float32(0.5)


def dither(mode, seed, c, n):
    """d of frames n (uint64 array) of channel c, float32"""
    n = np.atleast_1d(np.asarray(n, np.uint64))
    if mode == NONE:
        return np.zeros(len(n), np.float32)
    if mode == TPDF:
        return unit(seed, c, n, 0) + unit(seed, c, n, 1)
    return unit(seed, c, n, 0) - unit(seed, c, n - np.uint64(1), 0)


def mirror(x, fmt, mode=NONE, seed=0, first=0):
    """x float32 [C, n], one stream's planar samples whose first frame has the index `first` -> (codes [n, C], clamped mask, NaN mask).
    Mode NONE, and the formats that are not dithered: pcm_format_cases.mirror."""
    x = np.asarray(x, np.float32)
    if mode == NONE or fmt not in DITHERED_FORMATS:
        return tuple(np.ascontiguousarray(np.asarray(a).T) for a in fc.mirror(x, fmt))
    scale = np.float32(fc.FULL_SCALE[fmt])
    n = frame_indices(first, x.shape[1])
    d = np.stack([dither(mode, seed, c, n) for c in range(x.shape[0])])
    with np.errstate(over="ignore", invalid="ignore"):
        t = (x*scale + d).astype(np.float32)               # (float32 throughout: the product is exact, the sum is the one rounding)
        assert t.dtype == np.float32 and (x*scale).dtype == np.float32
        v = t.astype(np.float64)
        q = np.sign(v)*np.floor(np.abs(v) + 0.5)
        c = np.clip(q, -float(scale), float(scale) - 1)
    nan = np.isnan(x)
    codes = np.where(nan, 0.0, c).astype(np.int64).astype(np.int16 if fmt == fc.S16 else np.int32)
    return np.ascontiguousarray(codes.T), np.ascontiguousarray((~nan & (q != c)).T), np.ascontiguousarray(nan.T)


def mirror_frames(planar, counts, fmt, modes, seeds, firsts):
    """[S, C, n] float32 -> the frames the Python layer returns ([S, n, C], packed int24 [S, n, C, 3]); stream s dithered as (modes[s],
    seeds[s]) from frame index firsts[s], its first counts[s] frames -- the rest is zeros, as in a fresh output array"""
    S, Cn, most = planar.shape
    out = np.zeros((S, most, Cn), np.int16 if fmt == fc.S16 else np.int32)
    for s in range(S):
        k = max(counts[s], 0)
        out[s, :k] = mirror(planar[s, :, :k], fmt, modes[s], seeds[s], firsts[s])[0]
    return fc.to_rows(out, fc.S24).reshape(out.shape + (3,)) if fmt == fc.S24 else out


def check_known_answers():
    """the known answers of include/smst.h"""
    assert int(mix(1)) == 0x688990c0 and int(mix(0xffffffff)) == 0x6768824a
    assert [key(0, 0), key(0, 1), key(-7, 1), key(2**40 + 5, 15)] == [0xd56e12bd, 0x56302af1, 0xdbfc9700, 0xdbe9456e]
    n = np.arange(3, dtype=np.uint64)
    assert word(0, 0, n, 0).tolist() == [0x8ea83340, 0xd3f7b664, 0xa82e2bc5]
    assert word(0, 0, n, 1).tolist() == [0x73eac46c, 0xdfcaa731, 0x2ea8393e]
    scaled = lambda d: (d.astype(np.float64)*2.0**24).tolist()
    assert scaled(dither(TPDF, 0, 0, n)) == [168695, 11780701, -2697628]
    assert scaled(dither(HP, 0, 0, n)) == [-7219755, 4542339, -2869643]
    n = np.array([0, 2**32 - 1, 2**32, 2**64 - 1], np.uint64)
    assert scaled(dither(TPDF, -7, 1, n)) == [7581456, 5086807, 515381, 7516847]
    assert scaled(dither(HP, -7, 1, n)) == [1786397, -1939039, -6678722, -988138]
    x = np.full((1, 16), np.float32(0.3)/np.float32(32768), np.float32)
    assert mirror(x, fc.S16, TPDF)[0][:, 0].tolist() == [0, 1, 0, 0, 1, 0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]
    assert mirror(x, fc.S16, HP)[0][:, 0].tolist() == [0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1]
    for mode in MODES:                                                       # both sums are exact: multiples of 2^-24 inside (-1, 1)
        d = dither(mode, 12345, 3, frame_indices(2**32 - 100, 4096)).astype(np.float64)
        assert np.array_equal(d*2.0**24, np.round(d*2.0**24)) and np.abs(d).max() < 1.0


# ---- the converter hook --------------------------------------------------------------------------------------------------------------

def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def _signed64(v):
    v = int(v) & M64
    return v - 2**64 if v >= 2**63 else v


def convert(lib, fmt, counts, channels, src, src_ss, src_cs, dst, dst_ss, dst_fs, modes, seeds, firsts):
    """smst_debug_pcm_convert_dithered -> (clamped, nans)"""
    counts = np.ascontiguousarray(counts, np.int32)
    modes = np.ascontiguousarray(modes, np.int32)
    seeds = np.array([_signed64(v) for v in seeds], np.int64)
    firsts = np.array([_signed64(v) for v in firsts], np.int64)
    clamped, nans = np.full(len(counts), -1, np.int64), np.full(len(counts), -1, np.int64)
    rc = lib.smst_debug_pcm_convert_dithered(0, fmt, len(counts), channels, _ip(counts), C.c_void_p(src.ctypes.data), src_ss, src_cs,
                                             C.c_void_p(dst.ctypes.data), dst_ss, dst_fs, _ip(modes), _lp(seeds), _lp(firsts), _lp(clamped), _lp(nans))
    assert rc == 0, (lib.smst_last_error() or b"").decode()
    return clamped, nans


def encode_run(lib, fmt, x, mode, seed, first=0, offset=0):
    """x float32 [C, n] through the dithered kernel as one dense stream -> (codes [n, C], clamped, nans)"""
    Cn, n = x.shape
    esz = fc.ELEM_BYTES[fmt]
    src = pc.aligned(x.size, np.float32)
    src[:] = x.reshape(-1)
    dst = fc.byte_buffer(x.size*esz, offset)
    dst[:] = 0x5A
    clamped, nans = convert(lib, fmt, [n], Cn, src, x.size, n, dst, x.size, Cn, [mode], [seed], [first])
    return fc.from_rows(dst.reshape(-1, esz), fmt).reshape(n, Cn), int(clamped[0]), int(nans[0])


def _planar_values(fmt, n, rng):
    """what pcm_format_cases feeds the converter, plus values that clamp only because of the dither -- 0.4 LSB inside the value at which the
    undithered rule begins to clamp, either side (largest code + 0.5, smallest - 0.5), and 0.4 LSB inside the largest and smallest code;
    float32 has them to within its ulp, 0.5 LSB at the top of int24 -- and NaN, +-inf"""
    x = fc._planar_values(fmt, n, rng)
    scale = np.float32(fc.FULL_SCALE[fmt])
    lsb = lambda v: np.float32(np.float64(v)/np.float64(scale))
    edge = np.array([lsb(float(scale) - 0.9), lsb(-float(scale) - 0.1), lsb(float(scale) - 1.4), lsb(-float(scale) + 0.4), np.nan, np.inf, -np.inf], np.float32)
    spots = rng.random(n) < 0.06
    x[spots] = edge[rng.integers(0, len(edge), int(spots.sum()))]
    return x


def check_converter(lib, fmt, channels, byte_offsets, counts=fc.COUNTS):
    """The dithered kernel against the mirror: one stream per count -- 0 ... 513, across the 512-frame tile --, modes NONE, TPDF, HP and
    first frames 0, 1, 2^32 - 3 dealt over the streams and turned from one layout to the next so that every count meets every mode; the
    base pointer at every given byte offset behind a 16-byte boundary, frameStride = C and C + 1, a stream stride that is a multiple of 16
    bytes and one that is not.  Codes, the counters, every destination byte the call does not own (sentinel fill); the NONE streams'
    bytes are pcm_format_cases.mirror's."""
    S, Cn, most, esz = len(counts), channels, max(counts), fc.ELEM_BYTES[fmt]
    turn = 0
    only_dither = 0
    for offset in byte_offsets:
        for fs in (Cn, Cn + 1):
            odd_stride = turn % 2 == 1
            pss = (most*fs + 15)//16*16 + (3 if odd_stride else 0)
            pcs, planar_ss = most + 3, Cn*(most + 3) + 5
            pcm_len, planar_len = (S - 1)*pss + (most - 1)*fs + Cn, (S - 1)*planar_ss + (Cn - 1)*pcs + most
            rng = pc._rng(9003, Cn, fmt, offset, fs)
            modes = [(s + turn) % 3 for s in range(S)]
            firsts = [FIRST_FRAMES[(s//3 + turn) % 3] for s in range(S)]
            seeds = [(-7, 0, 12345, 2**40 + 5)[(s + turn) % 4] + s for s in range(S)]
            where = dict(C=Cn, fmt=fmt, byte_offset=offset, frame_stride=fs, stream_stride=pss, turn=turn)
            src = pc.aligned(planar_len, np.float32, 1)
            src[:] = _planar_values(fmt, planar_len, rng)
            dst = fc.byte_buffer(pcm_len*esz, offset)
            dst[:] = 0x5A
            want = dst.copy()
            rows = want.reshape(-1, esz)
            want_c, want_n = np.zeros(S, np.int64), np.zeros(S, np.int64)
            for s, n in enumerate(counts):
                x = np.stack([src[s*planar_ss + c*pcs:s*planar_ss + c*pcs + n] for c in range(Cn)])
                codes, cm, nm = mirror(x, fmt, modes[s], seeds[s], firsts[s])
                plain = fc.mirror(x, fmt)
                if modes[s] == NONE:
                    assert np.array_equal(codes, plain[0].T)
                only_dither += int((cm & ~plain[1].T).sum())
                want_c[s], want_n[s] = cm.sum(), nm.sum()
                for c in range(Cn):
                    rows[np.arange(n)*fs + s*pss + c] = fc.to_rows(codes[:, c], fmt)
            clamped, nans = convert(lib, fmt, counts, Cn, src, planar_ss, pcs, dst, pss, fs, modes, seeds, firsts)
            assert np.array_equal(dst, want), where
            assert np.array_equal(clamped, want_c) and np.array_equal(nans, want_n), (where, clamped.tolist(), want_c.tolist(), nans.tolist(), want_n.tolist())
            assert want_n.sum() > 0 and want_c.sum() > 0
            turn += 1
    assert turn >= 3 and only_dither > 0            # (every count met every mode; some element was clamped by its dither alone)


def check_statistics(lib, mode, seed):
    """N = 65536 stereo frames of x = 0.3 + 3.7 sin(0.01 n) LSB into int16 through the hook: the codes are the mirror's, and the error
    e = code - x has |mean| <= 5*0.5/sqrt(N) and |variance - 1/4| <= 0.0062 (five standard errors: rectangular rounding error + triangular
    dither, fourth moment 2.6 sigma^4); the dither's lag-1 autocorrelation is 0 (TPDF) or -1/2 (HP) and its two channels are uncorrelated,
    each to 0.02."""
    N = 65536
    lsb = (0.3 + 3.7*np.sin(0.01*np.arange(N))).astype(np.float32)
    x = np.stack([lsb, lsb])/np.float32(32768)
    codes, clamped, nans = encode_run(lib, fc.S16, x, mode, seed)
    assert np.array_equal(codes, mirror(x, fc.S16, mode, seed)[0]) and (clamped, nans) == (0, 0)
    n = frame_indices(0, N)
    d = np.stack([dither(mode, seed, c, n) for c in range(2)]).astype(np.float64)
    for c in range(2):
        e = codes[:, c].astype(np.float64) - lsb.astype(np.float64)
        assert abs(e.mean()) <= 0.0098, (mode, seed, c, e.mean())
        assert abs(e.var() - 0.25) <= 0.0062, (mode, seed, c, e.var())
        r1 = np.corrcoef(d[c, 1:], d[c, :-1])[0, 1]
        assert abs(r1 - (-0.5 if mode == HP else 0.0)) <= 0.02, (mode, seed, c, r1)
    r = np.corrcoef(d[0], d[1])[0, 1]
    assert abs(r) <= 0.02, (mode, seed, r)


def check_constant_below_one_lsb(lib):
    """what dither buys: the constant 0.3 LSB is digital silence undithered, and its dithered codes average 0.30 +- 0.01"""
    x = np.full((1, 65536), np.float32(0.3)/np.float32(32768), np.float32)
    assert not fc.encode_run(lib, fc.S16, x.reshape(-1)).any()
    for mode in MODES:
        codes, _, _ = encode_run(lib, fc.S16, x, mode, 0)
        assert np.array_equal(codes, mirror(x, fc.S16, mode, 0)[0])
        assert abs(codes.mean() - 0.30) <= 0.01, (mode, codes.mean())
    assert mirror(x[:, :16], fc.S16, TPDF)[0][:, 0].tolist() == [0, 1, 0, 0, 1, 0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]


# ---- sessions ------------------------------------------------------------------------------------------------------------------------

# a seek, two process calls of ragged counts (one count 0), a flush with one negative count: (out, in) per stream
SESSION = dict(seek=pc.SESSION["seek"], rates=pc.SESSION["rates"], calls=pc.SESSION["calls"][:2], flush=pc.SESSION["flush"])
# the same input and output cut into other calls: the first call in two
RECUT = dict(SESSION, calls=[([300, 100, 0], [250, 100, 0]), ([400, 200, 0], [350, 200, 0])] + pc.SESSION["calls"][1:2])
SESSION_MODES, SESSION_SEED = (TPDF, HP, TPDF), 5                            # per stream; stream s has seed 5 + s
_planar_cache = {}


def _session_length(session):
    return max(session["seek"]) + sum(max(nin) for _, nin in session["calls"])


def session_inputs(fmt, Cn=2):
    """-> (frames of the format, the planar float32 [S, C, n] they decode to)"""
    frames, planar = fc.session_inputs(Cn, fmt)
    n = _session_length(SESSION)
    return np.ascontiguousarray(frames[:, :n]), np.ascontiguousarray(planar[:, :, :n])


def planar_session(lib, planar, session, Cn=2):
    """the session through the planar float API -> the outputs of its process calls and of its flush ([S, C, n] each)"""
    b = package().StretchBatch(3, Cn, lib=lib, **pc.GEOMETRY)
    outs, pos = [], max(session["seek"])
    b.seek(np.ascontiguousarray(planar[:, :, :pos]), session["rates"], in_samples=session["seek"])
    for nout, nin in session["calls"]:
        outs.append(np.array(b.process(np.ascontiguousarray(planar[:, :, pos:pos + max(nin)]), nout, in_samples=nin), copy=True))
        pos += max(nin)
    outs.append(np.array(b.flush(session["flush"]), copy=True))
    b.close()
    return outs


def planar_reference(lib, fmt, session_name):
    """planar_session of the format's decoded inputs, computed once per library, format and session and left unchanged"""
    k = (id(lib), fmt, session_name)
    if k not in _planar_cache:
        _planar_cache[k] = planar_session(lib, session_inputs(fmt)[1], dict(session=SESSION, recut=RECUT)[session_name])
    return _planar_cache[k]


def frame_session(batch, frames, fmt, session, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True), between=None):
    """the session through the frame methods -> the outputs; between(k): called behind process call k"""
    outs, pos = [], max(session["seek"])
    batch.seekFrames(to_memory(np.ascontiguousarray(frames[:, :pos])), session["rates"], in_samples=session["seek"])
    for k, (nout, nin) in enumerate(session["calls"]):
        outs.append(to_host(batch.processFrames(to_memory(np.ascontiguousarray(frames[:, pos:pos + max(nin)])), nout, in_samples=nin)))
        pos += max(nin)
        if between:
            between(k)
    outs.append(to_host(batch.flushFrames(session["flush"], like=to_memory(np.zeros((1,), np.float32)), dtype=fc.frame_dtype(fmt))))
    return outs


def session_counts(session):
    return [nout for nout, _ in session["calls"]] + [[max(n, 0) for n in session["flush"]]]


def set_session_dither(batch):
    for s, mode in enumerate(SESSION_MODES):
        batch.setPcmDither(mode, SESSION_SEED + s, stream=s)


def check_session(lib, fmt, session_name="session", **memory):
    """The frame session with dither on = the mirror of the planar session's output, n running across the calls and on into the flush;
    pcmDither() reports the counters the rule predicts; the overs are the mirror's."""
    session = dict(session=SESSION, recut=RECUT)[session_name]
    frames, _ = session_inputs(fmt)
    want = planar_reference(lib, fmt, session_name)
    b = package().StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    set_session_dither(b)
    assert [b.pcmDither(s) for s in range(3)] == [(SESSION_MODES[s], SESSION_SEED + s, 0) for s in range(3)]
    got = frame_session(b, frames, fmt, session, **memory)
    seeds = [SESSION_SEED + s for s in range(3)]
    firsts, clamped = [0, 0, 0], np.zeros(3, np.int64)
    for k, (w, g, counts) in enumerate(zip(want, got, session_counts(session))):
        e = mirror_frames(w, counts, fmt, SESSION_MODES, seeds, firsts)
        assert g.dtype == e.dtype and g.shape == e.shape, (k, g.dtype, g.shape, e.dtype, e.shape)
        assert np.array_equal(g, e), ("call", k, "format", fmt, session_name)
        for s in range(3):
            clamped[s] += mirror(w[s, :, :counts[s]], fmt, SESSION_MODES[s], seeds[s], firsts[s])[1].sum()
        firsts = [f + n for f, n in zip(firsts, counts)]
    assert [b.pcmDither(s)[2] for s in range(3)] == firsts and firsts[0] > 0
    assert b.takePcmOvers()[0].tolist() == clamped.tolist()
    b.reset()
    assert [b.pcmDither(s) for s in range(3)] == [(SESSION_MODES[s], seeds[s], firsts[s]) for s in range(3)]    # (reset() leaves the counters alone)
    b.close()
    assert any(np.any(g != 0) for g in got)
    plain = [fc.encode_frames(pc.frames_of(w), fmt) for w in want]
    assert not all(np.array_equal(g, p) for g, p in zip(got, plain))         # (dither did change codes)
    return got


def check_recut(lib, fmt):
    """The same input and output cut into other calls: the frames are the mirror of THAT planar session with n running across its calls --
    and, the engine's own output being the same however the session is cut, the same bytes as the first cut's."""
    a, b = check_session(lib, fmt, "session"), check_session(lib, fmt, "recut")
    join = lambda outs, counts, s: np.concatenate([o[s, :n[s]] for o, n in zip(outs, counts)])
    for s in range(3):
        pa = np.concatenate([w[s, :, :n[s]] for w, n in zip(planar_reference(lib, fmt, "session"), session_counts(SESSION))], axis=1)
        pb = np.concatenate([w[s, :, :n[s]] for w, n in zip(planar_reference(lib, fmt, "recut"), session_counts(RECUT))], axis=1)
        assert pa.shape == pb.shape
        same = np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
        assert np.array_equal(join(a, session_counts(SESSION), s), join(b, session_counts(RECUT), s)) == same, s
    # the dither itself does not know the cut: one planar signal, converted in one run and in three
    x = planar_reference(lib, fmt, "session")[0][0][:, :700]
    whole = encode_run(lib, fmt, x, HP, 9)[0]
    parts = [encode_run(lib, fmt, np.ascontiguousarray(x[:, lo:hi]), HP, 9, first=lo)[0] for lo, hi in ((0, 1), (1, 514), (514, 700))]
    assert np.array_equal(whole, np.concatenate(parts))


def check_restart(lib, fmt=fc.S16):
    """setPcmDither in the middle of a session restarts the stream's n at 0 (and only that stream's)"""
    frames, _ = session_inputs(fmt)
    want = planar_reference(lib, fmt, "session")
    b = package().StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    set_session_dither(b)
    got = frame_session(b, frames, fmt, SESSION, between=lambda k: b.setPcmDither(TPDF, 77, stream=1) if k == 0 else None)
    counts = session_counts(SESSION)
    assert counts[0][1] > 0 and counts[1][0] > 0
    modes, seeds, firsts = list(SESSION_MODES), [SESSION_SEED + s for s in range(3)], [0, 0, 0]
    for k, (w, g, n) in enumerate(zip(want, got, counts)):
        assert np.array_equal(g, mirror_frames(w, n, fmt, modes, seeds, firsts)), k
        firsts = [f + m for f, m in zip(firsts, n)]
        if k == 0:
            modes[1], seeds[1], firsts[1] = TPDF, 77, 0
    assert [b.pcmDither(s) for s in range(3)] == [(modes[s], seeds[s], firsts[s]) for s in range(3)]
    b.close()


def check_other_formats_unchanged(lib, fmt, **memory):
    """S32, F16, F32 with dither on: today's session bit for bit -- and the counters of the streams still run"""
    frames, _ = session_inputs(fmt)
    pkg = package()
    plain, dithered = (pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY) for _ in range(2))
    set_session_dither(dithered)
    before = pkg.launch_count("pcm_out_dithered", lib)
    a = frame_session(plain, frames, fmt, SESSION, **memory)
    b = frame_session(dithered, frames, fmt, SESSION, **memory)
    assert pkg.launch_count("pcm_out_dithered", lib) == before
    for k, (p, q) in enumerate(zip(a, b)):
        assert p.dtype == q.dtype and fc.same_values(p, q, fmt), (fmt, k)
    assert any(np.any(p != 0) for p in a)
    totals = [sum(n[s] for n in session_counts(SESSION)) for s in range(3)]
    assert [dithered.pcmDither(s)[2] for s in range(3)] == totals and [plain.pcmDither(s) for s in range(3)] == [(NONE, 0, 0)]*3
    plain.close()
    dithered.close()


def check_steady_state_and_launches(lib, to_memory=lambda a: a):
    """a repeated dithered call allocates nothing; it counts as pcm_out_dithered and not as pcm_out, an undithered batch's the reverse;
    a batch whose only dithering stream is switched off again is an undithered one"""
    pkg = package()
    frames = np.ascontiguousarray(session_inputs(fc.S16)[0][:, :600])
    count = lambda: (pkg.launch_count("pcm_out", lib), pkg.launch_count("pcm_out_dithered", lib))
    b, plain = (pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY) for _ in range(2))
    b.setPcmDither(HP, 3, stream=1)
    x = to_memory(frames)
    b.processFrames(x, [600, 300, 0])
    b.processFrames(x, [600, 300, 0])
    events, c0 = b.allocation_events(), count()
    b.processFrames(x, [600, 300, 0])
    b.synchronize()
    assert b.allocation_events() == events and b.pcmDither(1)[2] == 900 and b.pcmDither(0)[2] == 0
    c1 = count()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, 1)
    plain.processFrames(x, [600, 300, 0])
    plain.synchronize()
    c2 = count()
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (1, 0)
    b.setPcmDither(NONE, stream=1)
    b.processFrames(x, [600, 300, 0])
    b.synchronize()
    c3 = count()
    assert (c3[0] - c2[0], c3[1] - c2[1]) == (1, 0)
    b.close()
    plain.close()


# ---- whole clips ---------------------------------------------------------------------------------------------------------------------

CLIPS = dict(inputs=[3000, 4000, 200, 6250, 5000], outputs=[7500, 5000, 300, -1, 4000], short=2, left_out=3)   # three clips, one too short, one left out
CLIP_MODES, CLIP_SEED = (TPDF, HP, TPDF, HP, HP), 21


def check_clips(lib, fmt, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True), wide=False):
    """exactFrames with dither = the mirror of exact's planar output with n from 0 per clip; the short clip is zero codes with ok False, the
    left-out clip's buffer is untouched, the counters stand, clip_out_dithered is counted; a second call obeys the same rule (and gives
    the same bytes where the engine gives the same samples).  wide: `out` is the [S, n, C] view into frames of C + 1 channels -- the
    kernel's element-by-element store in device memory, the frame-by-frame copy behind it in host memory -- and the pad element of every
    frame stays as it was"""
    import exact_cases as ec
    pkg = package()
    nin, nout, short, left = CLIPS["inputs"], CLIPS["outputs"], CLIPS["short"], CLIPS["left_out"]
    S, Cn, most = len(nin), 2, max(nout)
    frames = fc.encode_frames(pc.frames_of(ec.clip_inputs(Cn, nin, loud=0)), fmt)
    planar = np.ascontiguousarray(np.transpose(fc.decode_frames(frames, fmt), (0, 2, 1)))
    p, f = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(2))
    for s in range(S):
        f.setPcmDither(CLIP_MODES[s], CLIP_SEED + s, stream=s)
    seeds = [CLIP_SEED + s for s in range(S)]
    results = []
    for call in range(2):
        want, ok_p = p.exact(planar, nout, in_samples=nin)
        want = np.array(want, copy=True)
        out = np.full(frames.shape[:1] + (most,) + frames.shape[2:], 0x5A, frames.dtype)
        before = (pkg.launch_count("clip_out", lib), pkg.launch_count("clip_out_dithered", lib))
        store = to_memory(np.full(out.shape[:2] + (Cn + 1,) + out.shape[3:], 0x5A, out.dtype) if wide else out)
        dev_out = store[:, :, :Cn] if wide else store
        got, ok_f = f.exactFrames(to_memory(frames), nout, in_samples=nin, out=dev_out)
        got = to_host(got)
        assert got.shape == out.shape and (to_host(store)[:, :, Cn:] == 0x5A).all()
        after = (pkg.launch_count("clip_out", lib), pkg.launch_count("clip_out_dithered", lib))
        assert (after[0] - before[0], after[1] - before[1]) == (0, 1)
        assert ok_p.tolist() == ok_f.tolist() == [s not in (short, left) for s in range(S)]
        expect = out.copy()
        clamped = np.zeros(S, np.int64)
        for s in range(S):
            if s == left:
                continue
            mode = NONE if s == short else CLIP_MODES[s]
            codes, cm, _ = mirror(want[s, :, :nout[s]], fmt, mode, seeds[s], 0)
            expect[s, :nout[s]] = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
            clamped[s] = cm.sum()
        assert np.array_equal(got, expect), (fmt, call)
        assert not got[short, :nout[short]].any() and (got[left] == 0x5A).all() and got[0].any()
        assert f.takePcmOvers()[0].tolist() == clamped.tolist() and clamped[0] > 0 and clamped[short] == 0
        assert [f.pcmDither(s) for s in range(S)] == [(CLIP_MODES[s], seeds[s], 0) for s in range(S)]
        results.append((want, got))
    (w0, g0), (w1, g1) = results
    assert np.array_equal(g0, g1) == np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
    p.close()
    f.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def check_refusals(lib):
    pkg = package()
    b = pkg.StretchBatch(2, 2, lib=lib, **pc.GEOMETRY)
    for mode in (-1, 3, 7):
        assert lib.smst_batch_set_pcm_dither(b.h, -1, mode, 0) == -1 and b"mode" in lib.smst_last_error()
    for stream in (-2, 2, 100):
        assert lib.smst_batch_set_pcm_dither(b.h, stream, TPDF, 0) == -1 and b"stream" in lib.smst_last_error()
    for stream in (-1, 2):
        assert lib.smst_batch_pcm_dither(b.h, stream, None, None, None) == -1 and b"stream" in lib.smst_last_error()
    assert lib.smst_batch_set_pcm_dither(None, 0, TPDF, 0) == -1 and lib.smst_batch_pcm_dither(None, 0, None, None, None) == -1
    assert [b.pcmDither(s) for s in range(2)] == [(NONE, 0, 0)]*2                # (a refused call changes nothing)
    with pytest_raises(pkg.StretchError):
        b.setPcmDither(5)
    b.setPcmDither(pkg.DITHER_TPDF_HP, seed=-7)
    assert [b.pcmDither(s) for s in range(2)] == [(HP, -7, 0), (HP, -6, 0)] and lib.smst_batch_pcm_dither(b.h, 1, None, None, None) == 0
    assert (pkg.DITHER_NONE, pkg.DITHER_TPDF, pkg.DITHER_TPDF_HP) == (NONE, TPDF, HP)
    # the hook refuses an unknown mode as well
    src, dst = pc.aligned(8, np.float32), fc.byte_buffer(16, 0)
    counts, modes, zeros = np.array([4], np.int32), np.array([3], np.int32), np.zeros(1, np.int64)
    rc = lib.smst_debug_pcm_convert_dithered(0, fc.S16, 1, 2, _ip(counts), C.c_void_p(src.ctypes.data), 8, 4, C.c_void_p(dst.ctypes.data), 8, 2,
                                             _ip(modes), _lp(zeros), _lp(zeros), None, None)
    assert rc == -1 and b"mode" in lib.smst_last_error()
    b.close()


def pytest_raises(exc):
    import pytest
    return pytest.raises(exc)


# ---- the command-line tool -----------------------------------------------------------------------------------------------------------

def data_chunk(path):
    raw = open(path, "rb").read()
    pos, fmt = 12, None
    while pos + 8 <= len(raw):
        tag, size = raw[pos:pos + 4], struct.unpack("<I", raw[pos + 4:pos + 8])[0]
        if tag == b"fmt ":
            fmt = struct.unpack("<HHIIHH", raw[pos + 8:pos + 24])
        if tag == b"data":
            return fmt, raw[pos + 8:pos + 8 + size]
        pos += 8 + size + (size & 1)
    raise ValueError("no data chunk")


def check_cli(cli, tmp_path):
    """A two-file run: each data chunk is the mirror of the --out-format=f32 samples with seed + file index and n from 0 (the flush goes on
    counting); no --dither = --dither=none = the default file; --dither with f32 is refused."""
    from test_cli import write_wav16
    sr = 48000
    srcs = [str(tmp_path/("in%d.wav" % k)) for k in range(2)]
    write_wav16(srcs[0], 1.2*synth_input(1, 2, 6001, sr), sr)
    write_wav16(srcs[1], 0.5*synth_input(3, 2, 5000, sr), sr)

    def run(name, flags, expect_ok=True):
        outs = [str(tmp_path/("%s%d.wav" % (name, k))) for k in range(2)]
        res = subprocess.run([cli, "--time=1.1", "--semitones=2"] + flags + [srcs[0], outs[0], srcs[1], outs[1]], capture_output=True, text=True)
        assert (res.returncode == 0) == expect_ok, (flags, res.returncode, res.stderr)
        return outs, res
    f32, _ = run("f32", ["--out-format=f32"])
    floats = []
    for path in f32:
        fmt, data = data_chunk(path)
        assert fmt[:2] == (3, 2) and fmt[5] == 32
        floats.append(np.frombuffer(data, "<f4").reshape(-1, 2))
    assert len(floats[0]) == round(6001*1.1) and np.abs(floats[0]).max() > 0.5
    for name, flags, fmt, mode, seed in (("tpdf", ["--dither=tpdf", "--dither-seed=5", "--out-format=s16"], fc.S16, TPDF, 5),
                                         ("hp", ["--dither=tpdf-hp", "--out-format", "s24"], fc.S24, HP, 0)):
        outs, _ = run(name, flags)
        for k, path in enumerate(outs):
            head, data = data_chunk(path)
            assert head == (1, 2, sr, sr*2*fc.ELEM_BYTES[fmt], 2*fc.ELEM_BYTES[fmt], 8*fc.ELEM_BYTES[fmt])
            codes = mirror(np.ascontiguousarray(floats[k].T), fmt, mode, seed + k, 0)[0]
            assert np.array_equal(np.frombuffer(data, np.uint8), fc.to_rows(codes.reshape(-1), fmt).reshape(-1)), (name, k)
            assert not np.array_equal(codes, fc.mirror(floats[k], fmt)[0])
    default, _ = run("default", [])
    none, _ = run("none", ["--dither=none"])
    s16, _ = run("s16", ["--out-format=s16", "--dither-seed=9"])
    for k in range(2):
        raw = open(default[k], "rb").read()
        assert raw == open(none[k], "rb").read() == open(s16[k], "rb").read()
        head, data = data_chunk(default[k])
        assert head == (1, 2, sr, sr*4, 4, 16) and np.array_equal(np.frombuffer(data, "<i2"), fc.mirror(floats[k].reshape(-1), fc.S16)[0])
    _, res = run("bad", ["--dither=tpdf", "--out-format=f32"], expect_ok=False)
    assert "dither" in res.stderr
    run("bad2", ["--dither=blue"], expect_ok=False)
