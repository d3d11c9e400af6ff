"""Shared cases of the per-stream gain, the peak meters and the whole-clip gains of the frame output (test_level_emu.py on the CPU stand-in,
test_level_gpu.py on the device), next to dither_cases.py.

The numpy mirror below restates the "Level" section of include/smst.h: w = float32(v)*float32(g) -- one float32 multiply --, then
dither_cases.mirror on w; g of a whole-clip mode from float32(ceiling)/float32(peak) -- one float32 division --; the peak as the largest bit
pattern of |v|, NaN skipped.  Every comparison with it is exact -- bytes, counters, peaks and gains.  The inputs keep every product that
is not 0 above 2^-126: the denormal mode is not part of the contract."""
import re
import subprocess

import numpy as np

import dither_cases as dc
import pcm_cases as pc
import pcm_format_cases as fc
from conftest import package, synth_input

FIXED, PROTECT, NORMALISE = 0, 1, 2
ALL_FORMATS = (fc.S16, fc.F32, fc.S24, fc.S32, fc.F16)
GAINS = (0.5, 1.0, -1.75)
CLIP_PEAK_TILE = 2048                      # frames of a row one workgroup of kClipPeak reads (kClipTileFloats)
# the clip-free ceilings of include/smst.h as ceiling*scale: (format, dithered) -> (the largest that never clamps, the next one up, which does)
CEILINGS = {(fc.S16, False): (32767.0, 32768.0), (fc.S16, True): (32766.0, 32767.0),
            (fc.S24, False): (8388606.0, 8388607.0), (fc.S24, True): (8388605.0, 8388606.0),
            (fc.S32, False): (2.0**31 - 256, 2.0**31 - 128)}


def ceiling(fmt, dithered, which=0):
    """the tabulated ceiling as the float32 a caller passes; the float formats have none: 1.0"""
    if (fmt, dithered) not in CEILINGS:
        return np.float32(1.0)
    c = np.float32(CEILINGS[(fmt, dithered)][which]/fc.FULL_SCALE[fmt])
    assert float(c)*fc.FULL_SCALE[fmt] == CEILINGS[(fmt, dithered)][which]       # (exact: 24 bits at the most)
    return c


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def levelled(x, g):
    """w = v*g, one float32 multiply"""
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.asarray(x, np.float32)*np.float32(g)
    assert w.dtype == np.float32
    return w


def peak_of(x):
    """the largest |v| as the bit patterns order it, NaN skipped, 0 for nothing: float32"""
    bits = np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7fffffff)
    bits = np.where(bits > 0x7f800000, 0, bits).astype(np.uint32)
    return np.array([bits.max() if bits.size else 0], np.uint32).view(np.float32)[0]


def gain_of(mode, gain, ceil, peak):
    gain, ceil, peak = np.float32(gain), np.float32(ceil), np.float32(peak)
    if mode == FIXED or peak == 0 or not np.isfinite(peak):
        return gain
    with np.errstate(over="ignore"):
        q = ceil/peak
    assert q.dtype == np.float32
    return q if mode == NORMALISE or not gain <= q else gain


def mirror(x, fmt, g=1.0, mode=dc.NONE, seed=0, first=0):
    """x float32 [C, n] of one stream -> (codes [n, C], clamped mask, NaN mask) of the levelled conversion"""
    return dc.mirror(levelled(x, g), fmt, mode, seed, first)


def same_bytes(got, want, fmt):
    """two byte buffers of the format's elements: equal, any NaN of a float format equal to any other (the multiply may touch its payload)"""
    if fmt in (fc.F16, fc.F32):
        esz = fc.ELEM_BYTES[fmt]
        a, b = (fc.from_rows(v.reshape(-1, esz), fmt) for v in (got, want))
        return bool(((a.view(np.uint16 if esz == 2 else np.uint32) == b.view(np.uint16 if esz == 2 else np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return np.array_equal(got, want)


def _values(fmt, n, rng):
    """what the dither / format cases feed the converter -- ties, +-0, beyond full scale, NaN, +-inf --, plus values that clamp only after a
    gain of -1.75 (0.6, -0.58) and values that a gain of 0.5 stops from clamping (1.9, -1.99)"""
    x = dc._planar_values(fmt, n, rng) if fmt in dc.DITHERED_FORMATS else fc._planar_values(fc.S16 if fmt == fc.F32 else fmt, n, rng)
    extra = np.array([0.6, -0.58, 1.9, -1.99, np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32)
    spots = rng.random(n) < 0.05
    x[spots] = extra[rng.integers(0, len(extra), int(spots.sum()))]
    return x


# ---- 1. the converter ----------------------------------------------------------------------------------------------------------------

def check_converter(lib, fmt, channels, byte_offsets, counts=fc.COUNTS):
    """The levelled kPcmOut against the mirror: one stream per count -- 0 ... 513, across the 512-frame tile --, the gains 0.5, 1.0, -1.75
    and (int16 / int24) the dither modes dealt over the streams and turned from one layout to the next; the base pointer at every given
    byte offset, frameStride = C and C + 1, a stream stride that is a multiple of 16 bytes and one that is not.  Codes, every destination
    byte the call does not own (sentinel fill), the clamped / NaN counters, the peaks (NaN skipped, inf reported)."""
    pkg = package()
    S, Cn, most, esz = len(counts), channels, max(counts), fc.ELEM_BYTES[fmt]
    turn = 0
    seen = dict(only_gain=0, freed_by_gain=0, inf_peak=0, finite_peak=0)
    before = pkg.launch_count("pcm_out_levelled", lib)
    for offset in byte_offsets:
        for fs in (Cn, Cn + 1):
            pss = (most*fs + 15)//16*16 + (3 if turn % 2 else 0)
            pcs, planar_ss = most + 3, Cn*(most + 3) + 5
            pcm_len, planar_len = (S - 1)*pss + (most - 1)*fs + Cn, (S - 1)*planar_ss + (Cn - 1)*pcs + most
            rng = pc._rng(9101, Cn, fmt, offset, fs)
            gains = [GAINS[(s + turn) % 3] for s in range(S)]
            modes = [(s//3 + turn) % 3 if fmt in dc.DITHERED_FORMATS else dc.NONE for s in range(S)]
            firsts = [dc.FIRST_FRAMES[(s//2 + turn) % 3] for s in range(S)]
            seeds = [(-7, 0, 12345, 2**40 + 5)[(s + turn) % 4] + s for s in range(S)]
            where = dict(C=Cn, fmt=fmt, byte_offset=offset, frame_stride=fs, stream_stride=pss, turn=turn)
            src = pc.aligned(planar_len, np.float32, 1)
            src[:] = _values(fmt, planar_len, rng)
            dst = fc.byte_buffer(pcm_len*esz, offset)
            dst[:] = 0x5A
            want = dst.copy()
            rows = want.reshape(-1, esz)
            want_c, want_n, want_p = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.float32)
            for s, n in enumerate(counts):
                x = np.stack([src[s*planar_ss + c*pcs:s*planar_ss + c*pcs + n] for c in range(Cn)])
                codes, cm, nm = mirror(x, fmt, gains[s], modes[s], seeds[s], firsts[s])
                plain = dc.mirror(x, fmt, modes[s], seeds[s], firsts[s])
                if gains[s] == 1.0:
                    assert fc.same_values(codes, plain[0], fmt)
                seen["only_gain"] += int((cm & ~plain[1]).sum())
                seen["freed_by_gain"] += int((plain[1] & ~cm).sum())
                want_c[s], want_n[s], want_p[s] = cm.sum(), nm.sum(), peak_of(x)
                for c in range(Cn):
                    rows[np.arange(n)*fs + s*pss + c] = fc.to_rows(codes[:, c], fmt)
            clamped, nans, peaks = pkg.debug_pcm_convert_levelled(fmt, counts, Cn, src, planar_ss, pcs, dst, pss, fs, modes,
                                                                  [dc._signed64(v) for v in seeds], [dc._signed64(v) for v in firsts], gains, lib=lib)
            assert same_bytes(dst, want, fmt), where
            assert np.array_equal(clamped, want_c) and np.array_equal(nans, want_n), (where, clamped.tolist(), want_c.tolist(), nans.tolist(), want_n.tolist())
            assert np.array_equal(peaks.view(np.uint32), want_p.view(np.uint32)), (where, peaks.tolist(), want_p.tolist())
            assert want_p[0] == 0 and want_n.sum() > 0
            seen["inf_peak"] += int(np.isinf(want_p).sum())
            seen["finite_peak"] += int((np.isfinite(want_p) & (want_p > 0)).sum())
            turn += 1
    assert turn >= 3 and pkg.launch_count("pcm_out_levelled", lib) == before + turn
    assert seen["inf_peak"] > 0 and seen["finite_peak"] > 0, seen
    if fmt != fc.F32:                                    # (float32 clamps nothing)
        assert seen["only_gain"] > 0 and seen["freed_by_gain"] > 0, seen


# ---- 2. the clip pair: kClipPeak and the levelled kClipOut ---------------------------------------------------------------------------

# per table: (frames of segment 0, of segment 1) of the streams 0 ... 5; stream 6 moves nothing (table 0) or a run of zeros (table 1)
CLIP_TABLES = ([(1, 511), (512, 513), (0, 7), (513, 1), (64, CLIP_PEAK_TILE + 1), (9, 0)],
               [(511, 1), (7, 512), (CLIP_PEAK_TILE, 65), (0, 513), (2*CLIP_PEAK_TILE + 4, 3), (512, 0)])
CLIP_OFFSETS = (0, 1, 3, 4, 5, 511, 513)
#              FIXED  PROTECT that bites  PROTECT that does not  NORMALISE  all-zero clip  a clip with an inf  nothing / zeros
CLIP_LEVELS = (FIXED, PROTECT, PROTECT, NORMALISE, PROTECT, NORMALISE, NORMALISE)
CLIP_GAINS = (-1.75, 2.0, 0.5, 3.0, 0.6, 0.8, 0.7)
CLIP_DITHER = (dc.NONE, dc.TPDF, dc.HP, dc.TPDF, dc.HP, dc.NONE, dc.TPDF)
CLIP_PEAKS = (1.3, 1.3, 1.25, 0.37)                                # of the streams 0 ... 3, planted in the clip's last segment


def check_clip_pair(lib, fmt, channels):
    """kClipPeak + the levelled kClipOut through smst_debug_clip_copy_levelled against the mirror: seven streams -- FIXED, a PROTECT that
    lowers its gain and one that does not, NORMALISE, an all-zero clip and one that holds an inf (both: g = gain), and one that moves
    nothing or a run of zeros (not levelled, metered or reported) -- with segments of 0, 1, 511, 512, 513 frames and more than one tile of
    the peak pass, at offsets around them, frameStride C and C + 1.  The clip's peak lies in its second segment where it has one; the
    image around the segments holds 7.0, which a peak pass that read outside them would report.  Peaks, applied gains, codes, counters,
    every destination byte the call does not own."""
    pkg = package()
    S, Cn, esz = 7, channels, fc.ELEM_BYTES[fmt]
    dithered = fmt in dc.DITHERED_FORMATS
    ceil = ceiling(fmt, dithered)
    before = [pkg.launch_count(k, lib) for k in ("clip_peak", "clip_out_levelled")]
    for table_no, pairs in enumerate(CLIP_TABLES):
        fs = Cn + table_no
        segs = np.zeros((S, 2, 4), np.int32)
        for s, (n0, n1) in enumerate(pairs):
            a0, b0 = CLIP_OFFSETS[(s + 2*table_no) % 7], CLIP_OFFSETS[(3*s + 1 + table_no) % 7]
            segs[s, 0] = (a0, b0, n0, 0)
            segs[s, 1] = (a0 + n0 + 5, b0 + n0, n1, 0)                           # (the destination is one clip; the source has a gap)
        if table_no == 1:
            segs[6, 0] = (0, 3, 70, 1)
        image_end = int((segs[:, :, 0] + segs[:, :, 2]).max())
        out_end = int((segs[:, :, 1] + segs[:, :, 2]).max())
        ics, iss = image_end + 3, Cn*(image_end + 3) + 5
        css = out_end*fs + 3
        image_len, out_len = (S - 1)*iss + (Cn - 1)*ics + image_end, (S - 1)*css + (out_end - 1)*fs + Cn
        rng = pc._rng(9102, fmt, Cn, table_no)
        src = pc.aligned(image_len, np.float32, (Cn + table_no) % 4)
        src[:] = 7.0
        clips = []
        for s in range(S):
            n0, n1 = int(segs[s, 0, 2]), int(segs[s, 1, 2])
            x = rng.uniform(-0.3, 0.3, (Cn, n0 + n1)).astype(np.float32)
            x[rng.random(x.shape) < 0.02] = np.nan
            if s == 4 or segs[s, 0, 3]:
                x[:] = 0.0
            elif s == 5:
                x[Cn - 1, 3] = -np.inf
            elif x.size:
                x[(s + 1) % Cn, n0 + n1 - 1 - (s % max(min(n1, 3), 1))] = np.float32(CLIP_PEAKS[s])*(-1 if s % 2 else 1)
            clips.append(x)
            if not segs[s, 0, 3]:
                for c in range(Cn):
                    src[s*iss + c*ics + segs[s, 0, 0] + np.arange(n0)] = x[c, :n0]
                    src[s*iss + c*ics + segs[s, 1, 0] + np.arange(n1)] = x[c, n0:]
        dst = fc.byte_buffer(out_len*esz, esz*table_no)
        dst[:] = 0x5A
        want = dst.copy()
        rows = want.reshape(-1, esz)
        want_p, want_g = np.zeros(S, np.float32), np.ones(S, np.float32)
        want_c, want_n = np.zeros(S, np.int64), np.zeros(S, np.int64)
        for s, x in enumerate(clips):
            zeros = bool(segs[s, 0, 3])
            if x.size and not zeros:
                want_p[s] = peak_of(x)
                want_g[s] = gain_of(CLIP_LEVELS[s], CLIP_GAINS[s], ceil, want_p[s])
            codes, cm, nm = mirror(x, fmt, want_g[s], dc.NONE if zeros else CLIP_DITHER[s], 30 + s, int(segs[s, 0, 1]))
            want_c[s], want_n[s] = cm.sum(), nm.sum()
            for c in range(Cn):
                rows[(int(segs[s, 0, 1]) + np.arange(x.shape[1]))*fs + s*css + c] = fc.to_rows(codes[:, c], fmt)
        clamped, nans, peaks, applied = pkg.debug_clip_copy_levelled(fmt, segs, Cn, src, iss, ics, dst, css, fs, CLIP_LEVELS, CLIP_GAINS, [ceil]*S, CLIP_DITHER,
                                                                     [30 + s for s in range(S)], lib=lib)
        where = dict(fmt=fmt, C=Cn, table=table_no)
        assert np.array_equal(peaks.view(np.uint32), want_p.view(np.uint32)), (where, peaks.tolist(), want_p.tolist())
        assert np.array_equal(applied.view(np.uint32), want_g.view(np.uint32)), (where, applied.tolist(), want_g.tolist())
        assert same_bytes(dst, want, fmt), where
        assert np.array_equal(clamped, want_c) and np.array_equal(nans, want_n), (where, clamped.tolist(), want_c.tolist(), nans.tolist(), want_n.tolist())
        # the cases are what their names say
        assert want_g[0] == np.float32(-1.75) and want_g[1] < 2.0 and want_g[2] == 0.5 and want_g[3] != 3.0 and want_g[4] == np.float32(0.6), want_g.tolist()
        assert want_p[4] == 0 and np.isinf(want_p[5]) and want_g[5] == np.float32(0.8) and want_p[6] == 0 and want_g[6] == 1.0
        assert [float(p) for p in want_p[:4]] == [float(np.float32(p)) for p in CLIP_PEAKS]
        if fmt != fc.F32:
            assert want_c[1] == 0 and want_c[3] == 0 and want_c[0] > 0 and want_n.sum() > 0, (where, want_c.tolist())
    after = [pkg.launch_count(k, lib) for k in ("clip_peak", "clip_out_levelled")]
    assert [a - b for a, b in zip(after, before)] == [len(CLIP_TABLES)]*2


# ---- 3. the ceiling table ------------------------------------------------------------------------------------------------------------

_sweeps = {}


def ceiling_sweep(fmt, dithered, which, n=1 << 20):
    """n sampled peaks p (both signs; log-uniform over 2^-16 ... 2^3, and the neighbourhood of the ceiling itself) normalised to the
    tabulated ceiling (which = 0) or the next one up (1) through the mirror -> (clamped elements, the p whose |t| came out largest)"""
    k = (fmt, dithered, which)
    if k not in _sweeps:
        rng = pc._rng(9103, fmt, dithered)
        c = ceiling(fmt, dithered, which)
        p = (2.0**rng.uniform(-16, 3, n)).astype(np.float32)
        p[::4] = (np.float64(c)*rng.uniform(0.5, 2.0, len(p[::4]))).astype(np.float32)
        p[::2] *= np.float32(-1)
        g = (c/np.abs(p)).astype(np.float32)
        w = levelled(p, g)
        clamped = 0
        for mode in ((dc.TPDF, dc.HP) if dithered else (dc.NONE,)):
            clamped += int(dc.mirror(w.reshape(1, -1), fmt, mode, 11, 0)[1].sum())
        _sweeps[k] = (clamped, float(p[np.argmax(np.abs(w))]))
    return _sweeps[k]


def check_ceiling_table(fmt, dithered):
    """on the CPU: no sampled peak clamps at the tabulated ceiling, some does at the next one up"""
    assert ceiling_sweep(fmt, dithered, 0)[0] == 0, (fmt, dithered, ceiling_sweep(fmt, dithered, 0))
    assert ceiling_sweep(fmt, dithered, 1)[0] > 0, (fmt, dithered)


def check_ceiling_on_device(lib, fmt, dithered):
    """one clip per format whose peak element realises the worst case of the sweep -- the peak whose normalised value came out largest --,
    normalised to the tabulated ceiling by the kernels themselves: nothing is clamped, and the codes are the mirror's"""
    pkg = package()
    worst = np.float32(ceiling_sweep(fmt, dithered, 0)[1])
    Cn, n = 2, 1200
    rng = pc._rng(9104, fmt, dithered)
    x = (rng.uniform(-1, 1, (Cn, n))*abs(float(worst))*0.999).astype(np.float32)
    x[1, 700] = worst
    x[0, 5] = -worst
    src = pc.aligned(x.size, np.float32)
    src[:] = x.reshape(-1)
    esz = fc.ELEM_BYTES[fmt]
    dst = fc.byte_buffer(x.size*esz, 0)
    segs = np.array([[[0, 0, 513, 0], [513, 513, n - 513, 0]]], np.int32)
    mode = dc.TPDF if dithered else dc.NONE
    c = ceiling(fmt, dithered)
    clamped, nans, peaks, applied = pkg.debug_clip_copy_levelled(fmt, segs, Cn, src, x.size, n, dst, x.size, Cn, [NORMALISE], [1.0], [c], [mode], [11], lib=lib)
    g = gain_of(NORMALISE, 1.0, c, abs(worst))
    assert peaks[0] == abs(worst) and applied[0] == g
    codes, cm, _ = mirror(x, fmt, g, mode, 11, 0)
    assert not cm.any() and clamped[0] == 0 and nans[0] == 0, (fmt, dithered, int(clamped[0]))
    assert np.array_equal(dst, fc.to_rows(codes.reshape(-1), fmt).reshape(-1))
    top = np.abs(codes.astype(np.int64)).max()
    assert top >= CEILINGS[(fmt, dithered)][0]*(1 if fmt != fc.S32 else 0.999999) - 2, (fmt, dithered, int(top))   # (the clip does reach the ceiling)


# ---- 4. sessions ---------------------------------------------------------------------------------------------------------------------

SESSION_GAINS = (0.5, -4.0, 1.0)                                             # per stream


def set_session_levels(batch):
    for s, g in enumerate(SESSION_GAINS):
        batch.set_pcm_level(FIXED, g, stream=s)


def check_session(lib, fmt, dithered, session_name="session", **memory):
    """The frame session with FIXED gains per stream = the mirror of the planar session's output; take_pcm_peaks() is the largest |v| of that
    output (before the gain) and the gains set, a second take gives zero peaks and the same gains; the overs are the mirror's."""
    session = dict(session=dc.SESSION, recut=dc.RECUT)[session_name]
    frames, _ = dc.session_inputs(fmt)
    want = dc.planar_reference(lib, fmt, session_name)
    b = package().StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    set_session_levels(b)
    assert [b.pcm_level(s) for s in range(3)] == [(FIXED, g, 1.0) for g in SESSION_GAINS]
    modes = dc.SESSION_MODES if dithered else (dc.NONE,)*3
    if dithered:
        dc.set_session_dither(b)
    peaks0, gains0 = b.take_pcm_peaks()
    assert peaks0.tolist() == [0, 0, 0] and gains0.tolist() == [1, 1, 1]
    got = dc.frame_session(b, frames, fmt, session, **memory)
    seeds = [dc.SESSION_SEED + s for s in range(3)]
    firsts, clamped, peak_bits = [0, 0, 0], np.zeros(3, np.int64), np.zeros(3, np.uint32)
    for k, (w, g, counts) in enumerate(zip(want, got, dc.session_counts(session))):
        e = np.zeros(g.shape[:3], fc.from_rows(g.reshape(-1, 3)[:1], fmt).dtype if fmt == fc.S24 else g.dtype)
        for s in range(3):
            n = counts[s]
            codes, cm, nm = mirror(w[s, :, :n], fmt, SESSION_GAINS[s], modes[s], seeds[s], firsts[s])
            e[s, :n] = codes
            clamped[s] += cm.sum()
            assert not nm.any()
            peak_bits[s] = max(peak_bits[s], peak_of(w[s, :, :n]).view(np.uint32))
        e = fc.to_rows(e, fc.S24).reshape(e.shape + (3,)) if fmt == fc.S24 else e
        assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g, e), ("call", k, "format", fmt, session_name)
        firsts = [f + n for f, n in zip(firsts, counts)]
    peaks, gains = b.take_pcm_peaks()
    assert peaks.dtype == np.float32 and np.array_equal(peaks.view(np.uint32), peak_bits) and (peaks > 0).all(), (peaks.tolist(), peak_bits.view(np.float32).tolist())
    assert gains.tolist() == [float(np.float32(g)) for g in SESSION_GAINS]
    again = b.take_pcm_peaks()
    assert again[0].tolist() == [0, 0, 0] and again[1].tolist() == gains.tolist()
    assert b.takePcmOvers()[0].tolist() == clamped.tolist()
    if fmt != fc.F32:
        assert clamped[1] > 0                                                # (the stream at -4 does clamp)
    b.close()
    return got


def check_recut(lib, fmt):
    """the same input and output cut into other calls: the same bytes where the engine gives the same samples (dither_cases.check_recut)"""
    a, b = check_session(lib, fmt, True, "session"), check_session(lib, fmt, True, "recut")
    join = lambda outs, counts, s: np.concatenate([o[s, :n[s]] for o, n in zip(outs, counts)])
    for s in range(3):
        pa = np.concatenate([w[s, :, :n[s]] for w, n in zip(dc.planar_reference(lib, fmt, "session"), dc.session_counts(dc.SESSION))], axis=1)
        pb = np.concatenate([w[s, :, :n[s]] for w, n in zip(dc.planar_reference(lib, fmt, "recut"), dc.session_counts(dc.RECUT))], axis=1)
        same = np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
        assert np.array_equal(join(a, dc.session_counts(dc.SESSION), s), join(b, dc.session_counts(dc.RECUT), s)) == same, s


def check_whole_clip_mode_refused_in_streaming_calls(lib, **memory):
    """A stream in PROTECT makes processFrames and flushFrames fail (SMST_ERR_INVALID with a message) and touches no stream's state: the
    session, interrupted by refused calls between its calls, goes on to the bytes of an uninterrupted one."""
    pkg = package()
    fmt = fc.S16
    frames, _ = dc.session_inputs(fmt)
    to_memory = memory.get("to_memory", lambda a: a)
    plain, b = (pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY) for _ in range(2))
    for batch in (plain, b):
        set_session_levels(batch)
    want = dc.frame_session(plain, frames, fmt, dc.SESSION, **memory)

    def refused(k):
        b.set_pcm_level(PROTECT, 1.0, 0.9, stream=0)
        x = to_memory(np.ascontiguousarray(frames[:, :600]))
        for call in (lambda: b.processFrames(x, [600, 300, 0]), lambda: b.flushFrames([100, -1, 50], like=to_memory(np.zeros((1,), np.float32))),
                     lambda: b.flushFrames([100, 100, 100], like=to_memory(np.zeros((1,), np.float32)))):
            with dc.pytest_raises(pkg.StretchError) as e:
                call()
            assert "whole-clip" in str(e.value) and "error -1" in str(e.value), str(e.value)
        b.set_pcm_level(NORMALISE, 1.0, 0.9, stream=1)
        b.set_pcm_level(FIXED, SESSION_GAINS[0], stream=0)
        b.flushFrames([-1, -1, -1], like=to_memory(np.zeros((1,), np.float32)))    # (stream 1 takes no part: not refused -- and nothing is flushed)
        b.set_pcm_level(FIXED, SESSION_GAINS[1], stream=1)
    before = b.allocation_events()
    got = dc.frame_session(b, frames, fmt, dc.SESSION, between=lambda k: refused(k) if k == 0 else None, **memory)
    assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:])) and np.array_equal(got[0], want[0])
    assert b.allocation_events() >= before
    plain.close()
    b.close()


# ---- 5. whole clips ------------------------------------------------------------------------------------------------------------------

CLIP_STREAM_LEVELS = ((PROTECT, 1.0), (NORMALISE, 1.0), (NORMALISE, 1.0), (PROTECT, 2.0), (FIXED, 0.5))    # (mode, gain) per stream of dc.CLIPS


def check_clips(lib, fmt, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True), wide=False):
    """exactFrames with PROTECT, NORMALISE and FIXED mixed over the streams and TPDF on = the mirror of exact's planar output at the mirror's
    gain; peaks and gains exact; at the tabulated ceiling nothing is clamped where the same clips unlevelled are; the short clip is zero
    codes, the left-out clip's buffer untouched, and neither has a peak or a gain.  Two calls: the gains stand until the next conversion."""
    import exact_cases as ec
    pkg = package()
    nin, nout, short, left = dc.CLIPS["inputs"], dc.CLIPS["outputs"], dc.CLIPS["short"], dc.CLIPS["left_out"]
    S, Cn, most = len(nin), 2, max(nout)
    frames = fc.encode_frames(pc.frames_of(ec.clip_inputs(Cn, nin, loud=0)), fmt)
    planar = np.ascontiguousarray(np.transpose(fc.decode_frames(frames, fmt), (0, 2, 1)))
    p, f, u = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(3))
    ceil = ceiling(fmt, True)
    for s in range(S):
        for batch in (f, u):
            batch.setPcmDither(dc.CLIP_MODES[s], dc.CLIP_SEED + s, stream=s)
        f.set_pcm_level(CLIP_STREAM_LEVELS[s][0], CLIP_STREAM_LEVELS[s][1], ceil, stream=s)
    seeds = [dc.CLIP_SEED + s for s in range(S)]
    counters = ("clip_out", "clip_out_dithered", "clip_out_levelled", "clip_peak")
    for call in range(2):
        want, ok_p = p.exact(planar, nout, in_samples=nin)
        want = np.array(want, copy=True)
        u.exactFrames(to_memory(frames), nout, in_samples=nin)
        unlevelled = u.takePcmOvers()[0]
        out = np.full(frames.shape[:1] + (most,) + frames.shape[2:], 0x5A, frames.dtype)
        before = [pkg.launch_count(k, lib) for k in counters]
        store = to_memory(np.full(out.shape[:2] + (Cn + 1,) + out.shape[3:], 0x5A, out.dtype) if wide else out)
        dev_out = store[:, :, :Cn] if wide else store
        got, ok_f = f.exactFrames(to_memory(frames), nout, in_samples=nin, out=dev_out)
        got = to_host(got)
        assert got.shape == out.shape and (to_host(store)[:, :, Cn:] == 0x5A).all()
        assert [pkg.launch_count(k, lib) - n for k, n in zip(counters, before)] == [0, 0, 1, 1]
        assert ok_p.tolist() == ok_f.tolist() == [s not in (short, left) for s in range(S)]
        expect = out.copy()
        want_p, want_g = np.zeros(S, np.float32), np.ones(S, np.float32) if call == 0 else want_g
        for s in range(S):
            if s == left:
                continue
            x = want[s, :, :nout[s]]
            if s != short:
                want_p[s] = peak_of(x)
                want_g[s] = gain_of(CLIP_STREAM_LEVELS[s][0], CLIP_STREAM_LEVELS[s][1], ceil, want_p[s])
            codes, cm, _ = mirror(x, fmt, want_g[s] if s != short else 1.0, dc.NONE if s == short else dc.CLIP_MODES[s], seeds[s], 0)
            assert not cm.any(), (fmt, call, s)
            expect[s, :nout[s]] = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
        assert np.array_equal(got, expect), (fmt, call)
        assert not got[short, :nout[short]].any() and (got[left] == 0x5A).all() and got[0].any()
        assert f.takePcmOvers()[0].tolist() == [0]*S and unlevelled[0] > 0, unlevelled.tolist()
        peaks, gains = f.take_pcm_peaks()
        assert np.array_equal(peaks.view(np.uint32), want_p.view(np.uint32)), (peaks.tolist(), want_p.tolist())
        assert np.array_equal(gains.view(np.uint32), want_g.view(np.uint32)), (gains.tolist(), want_g.tolist())
        assert want_p[0] > 1.0 and want_g[0] < 1.0 and want_g[1] != 1.0 and want_g[4] == 0.5 and want_p[short] == 0 and want_g[short] == 1.0 and want_g[left] == 1.0
    for batch in (p, f, u):
        batch.close()


# ---- 6. opt-in -----------------------------------------------------------------------------------------------------------------------

LEVEL_COUNTERS = ("pcm_out_levelled", "clip_out_levelled", "clip_peak")


def check_opt_in(lib, dithered, **memory):
    """A batch that never sets a level: today's bytes (the mirror of the planar calls' output), today's launch counters, none of the new
    ones.  After set_pcm_level(FIXED, 1.0) on every stream: the same bytes from the levelled kernels.  kClipPeak runs only when a stream
    that takes part in an exact call has a whole-clip mode."""
    import exact_cases as ec
    pkg = package()
    fmt = fc.S16
    to_memory, to_host = memory.get("to_memory", lambda a: a), memory.get("to_host", lambda a: np.array(a, copy=True))
    count = lambda names: [pkg.launch_count(k, lib) for k in names]
    old = ("pcm_out_dithered", "clip_out_dithered") if dithered else ("pcm_out", "clip_out")
    frames, _ = dc.session_inputs(fmt)
    want = dc.planar_reference(lib, fmt, "session")
    modes, seeds = (dc.SESSION_MODES if dithered else (dc.NONE,)*3), [dc.SESSION_SEED + s for s in range(3)]
    nin, nout = dc.CLIPS["inputs"][:3], dc.CLIPS["outputs"][:3]
    clips = fc.encode_frames(pc.frames_of(ec.clip_inputs(2, nin)), fmt)

    def run(batch):
        if dithered:
            dc.set_session_dither(batch)
        outs = dc.frame_session(batch, frames, fmt, dc.SESSION, **memory)
        batch.reset()
        clip, ok = batch.exactFrames(to_memory(clips), nout, in_samples=nin)
        return outs + [to_host(clip)]
    plain, unity = (pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY) for _ in range(2))
    c0 = count(old + LEVEL_COUNTERS)
    a = run(plain)
    c1 = count(old + LEVEL_COUNTERS)
    assert c1[0] > c0[0] and c1[1] == c0[1] + 1 and c1[2:] == c0[2:], (c0, c1)
    firsts = [0, 0, 0]
    for w, g, counts in zip(want, a, dc.session_counts(dc.SESSION)):
        assert np.array_equal(g, dc.mirror_frames(w, counts, fmt, modes, seeds, firsts))
        firsts = [f + n for f, n in zip(firsts, counts)]
    unity.set_pcm_level(FIXED, 1.0, stream=-1)
    b = run(unity)
    c2 = count(old + LEVEL_COUNTERS)
    assert c2[:2] == c1[:2] and c2[2] - c1[2] == c1[0] - c0[0] and c2[3] == c1[3] + 1 and c2[4] == c1[4], (c1, c2)
    assert len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b)) and a[-1].any()
    # the peak pass: a whole-clip mode on a stream that is left out does not start it, one on a stream that runs does
    for stream, left_out, ran in ((1, [7500, -1, 300], 0), (1, nout, 1)):
        unity.set_pcm_level(PROTECT, 1.0, 0.9, stream=stream)
        before = count(("clip_peak",))[0]
        unity.exactFrames(to_memory(clips), left_out, in_samples=nin)
        unity.synchronize()
        assert count(("clip_peak",))[0] - before == ran, (stream, left_out)
    plain.close()
    unity.close()


# ---- 7. steady state -----------------------------------------------------------------------------------------------------------------

def check_steady_state(lib, to_memory=lambda a: a):
    """the second levelled processFrames / exactFrames of the same shapes allocates nothing, and neither do the takes"""
    import exact_cases as ec
    pkg = package()
    frames = np.ascontiguousarray(dc.session_inputs(fc.S16)[0][:, :600])
    nin, nout = dc.CLIPS["inputs"][:3], dc.CLIPS["outputs"][:3]
    clips = to_memory(fc.encode_frames(pc.frames_of(ec.clip_inputs(2, nin)), fc.S16))
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_level(FIXED, 0.5, stream=-1)
    b.setPcmDither(dc.TPDF, 3, stream=1)
    x = to_memory(frames)
    for _ in range(2):
        b.processFrames(x, [600, 300, 0])
    events = b.allocation_events()
    b.processFrames(x, [600, 300, 0])
    b.take_pcm_peaks()
    assert b.allocation_events() == events
    b.set_pcm_level(PROTECT, 1.0, 0.9, stream=0)
    b.set_pcm_level(NORMALISE, 1.0, 0.9, stream=1)
    for _ in range(2):
        b.exactFrames(clips, nout, in_samples=nin)
    events = b.allocation_events()
    b.exactFrames(clips, nout, in_samples=nin)
    peaks, gains = b.take_pcm_peaks()
    b.takePcmOvers()
    assert b.allocation_events() == events and peaks[0] > 0 and gains[1] == np.float32(0.9)/peaks[1] and gains[2] == 1.0   # (stream 2: too short, and no frame of it was ever converted)
    b.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------

def check_refusals(lib):
    pkg = package()
    b = pkg.StretchBatch(2, 2, lib=lib, **pc.GEOMETRY)
    inf, nan = float("inf"), float("nan")
    bad = [((-1, 3, 1.0, 1.0), b"mode"), ((-1, -1, 1.0, 1.0), b"mode"), ((2, FIXED, 1.0, 1.0), b"stream"), ((-2, FIXED, 1.0, 1.0), b"stream"),
           ((0, FIXED, inf, 1.0), b"gain"), ((0, FIXED, nan, 1.0), b"gain"), ((0, NORMALISE, -inf, 1.0), b"gain"),
           ((0, PROTECT, 0.0, 1.0), b"gain"), ((0, PROTECT, -1.0, 1.0), b"gain"),
           ((0, PROTECT, 1.0, 0.0), b"ceiling"), ((0, PROTECT, 1.0, inf), b"ceiling"), ((0, NORMALISE, 1.0, nan), b"ceiling"), ((0, NORMALISE, 1.0, -0.5), b"ceiling")]
    for args, word in bad:
        assert lib.smst_batch_set_pcm_level(b.h, *args) == -1 and word in lib.smst_last_error(), (args, lib.smst_last_error())
    assert lib.smst_batch_set_pcm_level(None, 0, FIXED, 1.0, 1.0) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_level(None, 0, None, None, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_take_pcm_peaks(None, None, None) == -1 and b"null" in lib.smst_last_error()
    for stream in (-1, 2):
        assert lib.smst_batch_pcm_level(b.h, stream, None, None, None) == -1 and b"stream" in lib.smst_last_error()
    assert [b.pcm_level(s) for s in range(2)] == [(FIXED, 1.0, 1.0)]*2           # (a refused call changes nothing)
    with dc.pytest_raises(pkg.StretchError):
        b.set_pcm_level(5)
    # what is allowed: a fixed gain of 0 or below, a ceiling that FIXED ignores, every pointer of the getter null
    b.set_pcm_level(FIXED, -2.0, -1.0)
    b.set_pcm_level(NORMALISE, 0.0, 0.25, stream=1)
    assert [b.pcm_level(s) for s in range(2)] == [(FIXED, -2.0, -1.0), (NORMALISE, 0.0, 0.25)] and lib.smst_batch_pcm_level(b.h, 1, None, None, None) == 0
    assert lib.smst_batch_take_pcm_peaks(b.h, None, None) == 0
    assert (pkg.LEVEL_FIXED, pkg.LEVEL_PROTECT, pkg.LEVEL_NORMALISE) == (FIXED, PROTECT, NORMALISE)
    b.close()


# ---- 10. the command-line tool -------------------------------------------------------------------------------------------------------

def level_lines(stdout):
    """the "level:" lines of a run -> [(file, peak, gain, overs)], the two floats as float32"""
    found = re.findall(r"^level: (\S+) peak=(\S+) gain=(\S+) overs=(-?\d+)$", stdout, re.M)
    return [(name, np.float32(peak), np.float32(gain), int(overs)) for name, peak, gain, overs in found]


def check_cli(cli, tmp_path, lib):
    """--exact renders what exactFrames renders; --protect / --normalize print the clip's peak and a gain of ceiling/peak, write the mirror of
    the --exact floats at that gain and clamp nothing where the same run at 0 dB does; --gain works in the default flow too; --protect
    with --normalize is refused.  (A run without the new flags: test_cli.py and the dither tests pin it.)"""
    from test_cli import write_wav16
    pkg = package()
    sr, lengths = 48000, (6001, 7000)
    srcs = [str(tmp_path/("in%d.wav" % k)) for k in range(2)]
    write_wav16(srcs[0], 1.2*synth_input(1, 2, lengths[0], sr), sr)
    write_wav16(srcs[1], 0.5*synth_input(3, 2, lengths[1], sr), sr)

    def run(name, flags, expect=0):
        outs = [str(tmp_path/("%s%d.wav" % (name, k))) for k in range(2)]
        res = subprocess.run([cli, "--time=1.1", "--semitones=2"] + flags + [srcs[0], outs[0], srcs[1], outs[1]], capture_output=True, text=True)
        assert res.returncode == expect, (flags, res.returncode, res.stderr)
        return outs, res

    def floats_of(paths):
        got = []
        for path in paths:
            head, data = dc.data_chunk(path)
            assert head[:2] == (3, 2) and head[5] == 32
            got.append(np.frombuffer(data, "<f4").reshape(-1, 2))
        return got
    outs, res = run("xf32", ["--exact", "--out-format=f32"])
    assert not level_lines(res.stdout)
    floats = floats_of(outs)
    nout = [round(n*1.1) for n in lengths]
    assert [len(f) for f in floats] == nout
    # ... which is what the library's exact() makes of the files' samples
    x = np.zeros((2, 2, max(lengths)), np.float32)
    for k, path in enumerate(srcs):
        x[k, :, :lengths[k]] = np.frombuffer(dc.data_chunk(path)[1], "<i2").reshape(-1, 2).T.astype(np.float32)/np.float32(32768)
    b = pkg.StretchBatch(2, 2, preset="default", sample_rate=sr, seed=0, lib=lib)
    b.setTransposeSemitones(2, 8000/sr)
    b.setFormantBase(100/sr)
    want, ok = b.exact(x, nout, in_samples=list(lengths))
    b.close()
    assert ok.all() and all(np.array_equal(floats[k], want[k, :, :nout[k]].T) for k in range(2))
    peaks = [peak_of(f) for f in floats]
    up = 10**(6/20)
    assert peaks[0]*up > 1.0 > peaks[1]*up, peaks                             # (at +6 dB file 0 clips, file 1 does not)
    # a fixed gain of +6 dB: the overs it costs
    outs, res = run("fixed", ["--exact", "--gain=6", "--out-format=s16", "--dither=tpdf"])
    lines = level_lines(res.stdout)
    assert [(l[0], l[1]) for l in lines] == [(outs[k], peaks[k]) for k in range(2)] and lines[0][3] > 0 and lines[1][3] == 0, lines
    assert lines[0][2] == lines[1][2] and abs(float(lines[0][2]) - up) <= 1e-6*up
    for k in range(2):
        codes, cm, _ = mirror(np.ascontiguousarray(floats[k].T), fc.S16, lines[k][2], dc.TPDF, k, 0)
        assert np.array_equal(np.frombuffer(dc.data_chunk(outs[k])[1], "<i2"), codes.reshape(-1)) and lines[k][3] == int(cm.sum())
    for name, flags, fmt, mode, level, db in (("prot", ["--protect=-0.5", "--gain=6", "--out-format=s16", "--dither=tpdf"], fc.S16, dc.TPDF, PROTECT, -0.5),
                                              ("norm", ["--normalize=-1", "--out-format=s24"], fc.S24, dc.NONE, NORMALISE, -1.0)):
        outs, res = run(name, flags)
        lines = level_lines(res.stdout)
        assert len(lines) == 2, res.stdout
        for k, (path, peak, gain, overs) in enumerate(lines):
            assert path == outs[k] and peak == peaks[k] and overs == 0, (name, lines)
            bites = level == NORMALISE or peaks[k]*up > 10**(db/20)
            expect = 10**(db/20)/float(peaks[k]) if bites else up
            assert abs(float(gain) - expect) <= 1e-6*expect, (name, k, float(gain), expect)
            head, data = dc.data_chunk(path)
            esz = fc.ELEM_BYTES[fmt]
            assert head == (1, 2, sr, sr*2*esz, 2*esz, 8*esz)
            codes, cm, _ = mirror(np.ascontiguousarray(floats[k].T), fmt, gain, mode, k, 0)
            assert np.array_equal(np.frombuffer(data, np.uint8), fc.to_rows(codes.reshape(-1), fmt).reshape(-1)) and not cm.any(), (name, k)
        assert lines[0][2] < up and (abs(float(lines[1][2]) - up) <= 1e-6*up) == (level == PROTECT)
    _, res = run("both", ["--protect=-1", "--normalize=-1"], expect=2)
    assert "exclude" in res.stderr
    # the default flow: --gain sends its two stages through the frame calls
    default = floats_of(run("f32", ["--out-format=f32"])[0])
    outs, res = run("gain", ["--gain=-6"])
    lines = level_lines(res.stdout)
    g = np.float32(10**(-6/20))
    assert len(lines) == 2 and abs(float(lines[0][2]) - float(g)) <= 1e-6*float(g) and lines[0][2] == lines[1][2]
    for k, (path, peak, gain, overs) in enumerate(lines):
        head, data = dc.data_chunk(path)
        assert head == (1, 2, sr, sr*4, 4, 16) and peak == peak_of(default[k])
        codes, cm, _ = mirror(np.ascontiguousarray(default[k].T), fc.S16, gain)
        assert np.array_equal(np.frombuffer(data, "<i2"), codes.reshape(-1)) and overs == int(cm.sum()), (k, overs)
