"""Shared cases of the true-peak flag of the frame output (include/smst.h, "True peak"): test_true_peak_emu.py runs them on the CPU stand-in,
test_true_peak_gpu.py on the device, next to level_cases.py and loudness_cases.py.

The numpy mirror below restates the definition: per phase p = 1, 2, 3 the sum over the 12 taps in float64, accumulated from 0.0 in the order
j = 0 ... 11 over the clip padded with 5 zeros in front and 6 behind, each result rounded once to float32, and the maximum of the bit
patterns of |v| over those and the samples themselves, NaN skipped.  Every product of two float32 values is exact in float64 and the
additions come in the device's order, so every comparison of a true peak is one of BIT PATTERNS -- there is no tolerance to choose.  The
mirror takes the library's own tap table (smst_debug_true_peak_taps), which is compared with the formula on its own: the host's libm and
numpy may differ in the last bit of a double, hence 1 float32 ulp there."""
import math
import re
import subprocess

import numpy as np

import dither_cases as dc
import exact_cases as xc
import level_cases as lc
import loudness_cases as ld
import pcm_cases as pc
import pcm_format_cases as fc
from conftest import package, synth_input

T = 1024                                             # frames one workgroup of the pass measures (kTruePeakTile, SMST_TRUE_PEAK_TILE)
TAPS, LEAD, TRAIL = 12, 5, 6
FIXED, PROTECT, NORMALISE, LOUDNESS = lc.FIXED, lc.PROTECT, lc.NORMALISE, ld.LOUDNESS
compared = dict(peaks=0)                             # true peaks compared bit for bit with the mirror so far (printed by the tests; EXPERIMENTS.md)


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def formula_taps():
    """c[p - 1][j] = float32(h/sum h), h = sinc(t)*0.5*(1 + cos(pi*t/6)), t = j - 5 - p/4: float32 [3, 12]"""
    c = np.zeros((3, TAPS), np.float32)
    for p in (1, 2, 3):
        t = np.arange(TAPS, dtype=np.float64) - LEAD - p/4
        h = np.sin(np.pi*t)/(np.pi*t)*0.5*(1 + np.cos(np.pi*t/6))
        c[p - 1] = (h/h.sum()).astype(np.float32)
    return c


def phases(x, taps):
    """x [C, N] float32 of one clip -> y [3, C, N] float64: y_p(n) = sum_j double(c[p][j])*double(x(n + j - 5)), from 0.0, in the order of j"""
    x = np.asarray(x, np.float32)
    Cn, N = x.shape
    pad = np.zeros((Cn, N + LEAD + TRAIL), np.float64)
    pad[:, LEAD:LEAD + N] = x
    y = np.zeros((3, Cn, N), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(3):
            for j in range(TAPS):
                y[p] = y[p] + float(taps[p, j])*pad[:, j:j + N]
    return y


def _bits(v):
    """float32 values -> the bit patterns of |v| as the meter orders them: NaN gives 0"""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0x7fffffff)
    return np.where(b > 0x7f800000, 0, b).astype(np.uint32)


def true_peak(x, taps, where=False):
    """the true peak of one clip x [C, N]: float32.  where: -> (the peak, (phase 0 ... 3, channel, frame) of its first occurrence)"""
    x = np.asarray(x, np.float32)
    if x.shape[1] == 0:
        return (np.float32(0), None) if where else np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        y32 = phases(x, taps).astype(np.float32)
    bits = np.concatenate([_bits(x)[None], _bits(y32)])
    most = bits.max()
    peak = np.array([most], np.uint32).view(np.float32)[0]
    if not where:
        return peak
    return peak, tuple(int(i) for i in np.argwhere(bits == most)[0])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def faded_tone(f, n=4000):
    """a Hann-faded tone of frequency f (cycles per sample) whose samples straddle its crests: the samples lie half a step beside them"""
    t = np.arange(n) + 0.5
    return (np.sin(2*np.pi*f*t)*0.5*(1 - np.cos(2*np.pi*t/n))).astype(np.float32)[None, :]


def check_mirror():
    """the formula's known answers of include/smst.h and the properties the definition states"""
    c = formula_taps()
    known2 = "-9.85122286e-04 1.03496173e-02 -3.36731486e-02 8.00664872e-02 -1.80965975e-01 6.25208139e-01".split()
    known1 = ("-1.63094362e-03 1.03549864e-02 -3.00933104e-02 6.91253021e-02 -1.61381096e-01 8.96035254e-01 2.88544923e-01 -1.03407115e-01 4.62428667e-02 "
              "-1.85171217e-02 4.89363540e-03 -1.67361679e-04").split()
    assert ["%.8e" % v for v in c[1]] == known2 + known2[::-1], c[1]
    assert ["%.8e" % v for v in c[0]] == known1, c[0]
    assert np.array_equal(c[2], c[0][::-1])
    assert np.abs(c.astype(np.float64).sum(axis=1) - 1).max() <= 1e-7
    impulse = np.array([[1.0]], np.float32)
    assert true_peak(impulse, c) == np.float32(1.0)
    assert "%.8f" % _inter(impulse, c) == "0.89603525"
    assert "%.7f" % true_peak(np.array([[1.0, 1.0]], np.float32), c) == "1.2504163"
    for f, db in ((0.25, -0.041), (0.125, -0.006)):
        x = faded_tone(f)
        tp = float(true_peak(x, c))
        assert abs(20*math.log10(tp)) <= 0.05 and abs(20*math.log10(tp) - db) < 1e-3, (f, tp)
    assert "%.5f" % true_peak(faded_tone(0.25), c) == "0.99528" and "%.5f" % lc.peak_of(faded_tone(0.25)) == "0.70711"
    assert "%.5f" % true_peak(faded_tone(0.125), c) == "0.99930" and "%.5f" % true_peak(faded_tone(0.375), c) == "0.97687"


def _inter(x, taps):
    """the inter-sample part alone: the largest of the three phases"""
    return np.array([_bits(phases(x, taps).astype(np.float32)).max()], np.uint32).view(np.float32)[0]


# ---- 1. the taps and the pass against the mirror ------------------------------------------------------------------------------------------

_taps = {}


def library_taps(lib):
    key = id(lib)
    if key not in _taps:
        _taps[key] = package().debug_true_peak_taps(lib)
    return _taps[key]


def check_taps(lib):
    """the library's table against the formula, within 1 float32 ulp; every phase sums to 1 within 1e-7; phase 3 mirrors phase 1"""
    got, want = library_taps(lib), formula_taps()
    assert got.shape == (3, TAPS) and got.dtype == np.float32
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1 and np.array_equal(np.signbit(got), np.signbit(want)), (got.tolist(), want.tolist())
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1).max() <= 1e-7
    assert package().TRUE_PEAK_TILE == T


LENGTHS = (1, 2, 5, 6, 7, 11, 12, 13, T - 1, T, T + 1, T + 5, T + 6, T + 7, 2*T + 3)
JOINS = (0, 1, 5, 6, 7, T - 6, T - 5, T, T + 5, T + 6, 10**9)              # where segment 1 begins in the clip (beyond its length: segment 1 empty)
SRC_OFFSETS = (1, 3, 0, 5, 511, 513, 4, 7)
# (length, join): every length, every join on a clip it cuts, and the joins around a tile's edge on clips that end around the next halo
PAIRS = tuple((n, JOINS[i % len(JOINS)]) for i, n in enumerate(LENGTHS)) + tuple((2*T + 3, j) for j in JOINS) + tuple((T + 7, j) for j in JOINS[5:])
assert len(PAIRS) == 32


def _noise(rng, Cn, n, stream):
    """noise, scaled differently per stream and channel"""
    return (rng.uniform(-1, 1, (Cn, n))*(0.1 + 0.2*stream)*(1 + 0.1*np.arange(Cn))[:, None]).astype(np.float32)


def run_hook(lib, clips, joins, offsets, base_offset=1, flags=None, zeros=()):
    """the hook on the clips' image (loudness_cases.build_image: rows at odd float offsets, a gap between the two segments, 7.0 around them)
    -> (true peaks, sample peaks); zeros: the streams whose segment 0 is marked as a run of zeros"""
    pkg = package()
    image, segs, iss, ics = ld.build_image(clips, joins, offsets, base_offset)
    for s in zeros:
        segs[s, 0, 3] = 1
    before = pkg.launch_count("clip_true_peak", lib)
    tp, sp = pkg.debug_clip_true_peak(segs, clips[0].shape[0], image, iss, ics, flags, lib=lib)
    assert pkg.launch_count("clip_true_peak", lib) == before + 1
    return tp, sp, segs


def compare_hook(lib, clips, joins, offsets, base_offset=1):
    """both outputs of the hook equal the mirror's as bit patterns, for every stream"""
    taps = library_taps(lib)
    tp, sp, segs = run_hook(lib, clips, joins, offsets, base_offset)
    for s, x in enumerate(clips):
        where = dict(stream=s, C=x.shape[0], n=x.shape[1], join=int(segs[s, 0, 2]), offset=offsets[s])
        want = true_peak(x, taps)
        assert same_bits(tp[s], want), (where, float(tp[s]), float(want))
        assert same_bits(sp[s], lc.peak_of(x)) and tp[s] >= sp[s], (where, float(sp[s]))
        compared["peaks"] += 1
    return tp, sp


def check_hook(lib, channels):
    """the pass through smst_debug_clip_true_peak against the mirror, four calls of eight streams: the lengths and joins of PAIRS, rows at
    offsets that are no multiples of 4 floats, the image itself one float behind a 16-byte boundary"""
    rng = pc._rng(9301, channels)
    inter = 0
    for g in range(0, len(PAIRS), 8):
        group = PAIRS[g:g + 8]
        clips = [_noise(rng, channels, n, s) for s, (n, _) in enumerate(group)]
        tp, sp = compare_hook(lib, clips, [j for _, j in group], SRC_OFFSETS)
        inter += int((tp > sp).sum())
    assert inter >= 16, inter                          # (noise: the largest value of most clips lies between the samples)
    print("true peaks bit-identical to the mirror so far: %d" % compared["peaks"])


def _planted(rng, n, kind, at):
    """[2, n]: noise at 1e-3 and, in channel 1, a figure whose largest value lies BETWEEN samples: `pair` -- two equal samples at at - 1 and
    at, the crest half way between them (1.25 of the samples) --; `back` / `front` -- six samples of alternating sign that decay away from
    `at` backwards / forwards, the crest a quarter step beyond `at` on the side where the figure ends (1.09 of the largest sample)"""
    x = (rng.uniform(-1, 1, (2, n))*1e-3).astype(np.float32)
    if kind == "pair":
        x[1, at - 1:at + 1] = 0.8
    else:
        for k in range(6):
            i = at - k if kind == "back" else at + k
            if 0 <= i < n:
                x[1, i] = 0.9*(-0.8)**k
    return x


def check_planted(lib):
    """Clips whose largest value is an inter-sample one that needs a halo: (a) between the last frame of tile 0 and the first of tile 1, from
    either side; (b) between the last frame of segment 0 and the first of segment 1; (c) between frame N - 1 and the zeros behind the clip;
    (d) between frame 0 and frame 1, the 5 zeros in front.  Silence elsewhere but for noise at 1e-3: a kernel that drops a halo is off by
    8 % and more.  In the same call: a stream with the flag off, one whose segment is a run of zeros, one of count 0 -- each reports 0."""
    taps = library_taps(lib)
    rng = pc._rng(9302)
    n = T + 300
    cases = [("pair", T, 10**9, (2, 1, T - 1)),          # (a): y_2(T - 1) needs x(T), tile 0's halo behind
             ("back", T, 10**9, (1, 1, T)),              # (a): y_1(T) needs x(T - 5 ... T - 1), tile 1's halo in front
             ("pair", 700, 700, (2, 1, 699)),            # (b)
             ("back", n - 1, 333, (1, 1, n - 1)),        # (c)
             ("pair", 1, T + 5, (2, 1, 0))]              # (d)
    clips = [_planted(rng, n, kind, at) for kind, at, _, _ in cases]
    for x, (kind, at, _, spot) in zip(clips, cases):
        peak, where = true_peak(x, taps, where=True)
        assert where == spot and peak > 1.08*lc.peak_of(x), (kind, at, where, float(peak))
    clips += [_noise(rng, 2, n, 1), _noise(rng, 2, n, 2), np.zeros((2, 0), np.float32)]
    joins = [j for _, _, j, _ in cases] + [5, 10**9, 0]
    flags = [1]*5 + [0, 1, 1]
    tp, sp, _ = run_hook(lib, clips, joins, SRC_OFFSETS, flags=flags, zeros=(6,))
    for s in range(5):
        assert same_bits(tp[s], true_peak(clips[s], taps)) and same_bits(sp[s], lc.peak_of(clips[s])), (s, float(tp[s]))
        compared["peaks"] += 1
    assert tp[5] == 0 and same_bits(sp[5], lc.peak_of(clips[5])) and sp[5] > 0      # the flag off: not measured (kClipPeak still reads it)
    assert tp[6] == 0 and sp[6] == 0 and tp[7] == 0 and sp[7] == 0                    # a run of zeros; nothing


def check_nan_inf(lib):
    """one NaN in a clip -- inside a tile, and three frames behind a tile's edge, where it reaches the tile in front through the halo --: the
    windows that hold it are skipped and the rest is metered as the mirror says; +inf gives inf; +inf and -inf within 12 frames of each
    other: IEEE on both sides (inf - inf is a NaN, skipped)"""
    taps = library_taps(lib)
    rng = pc._rng(9303)
    n = T + 50
    clips = [_noise(rng, 2, n, s) for s in range(5)]
    clips[0][1, 500] = np.nan
    clips[1][0, T + 2] = np.nan
    loud = np.float32(50.0)                                # a loud sample beside stream 1's NaN: every window that weighs it heavily holds the NaN
    clips[1][0, T + 1] = loud
    clips[2][0, 77] = np.inf
    clips[3][1, 100], clips[3][1, 107] = np.inf, -np.inf
    clips[4][0, T - 1], clips[4][0, T + 3] = -np.inf, np.inf
    tp, sp = compare_hook(lib, clips, (333, T, 5, 101, T + 1), SRC_OFFSETS)
    assert np.isfinite(tp[:2]).all() and (tp[:2] > 0).all() and tp[1] >= loud and np.isinf(tp[2:]).all(), tp.tolist()
    # (the mirror's inter-sample part of stream 3 between the two infinities is a NaN: the case is there)
    assert np.isnan(phases(clips[3], taps)[:, 1, 101:107]).any()


def check_reproducible(lib):
    """two runs of the hook give the same bits"""
    rng = pc._rng(9304)
    clips = [_noise(rng, 3, n, s) for s, n in enumerate((2*T + 3, T + 7, 13))]
    runs = [run_hook(lib, clips, (T - 5, 7, 6), SRC_OFFSETS)[:2] for _ in range(2)]
    for a, b in zip(*runs):
        assert same_bits(a, b)
    assert runs[0][0].min() > 0


# ---- 2. whole clips through smst_batch_exact_pcm ---------------------------------------------------------------------------------------

#  five clips of ragged lengths and rates, three tiles and a few frames at the most
CLIPS = dict(inputs=[1500, 2000, 2400, 2800, 1800], outputs=[3*T + 3, 2500, 3000, 2100, 2700])
CLIP_LEVELS = ((NORMALISE, 1.0), (PROTECT, 8.0), (LOUDNESS, 1.0), (FIXED, 0.5), (NORMALISE, 1.0))     # (mode, gain); PROTECT at +18 dB: the ceiling bites
CLIP_TARGET, CLIP_FS = 6.0, 6000.0                                                                     # LOUDNESS at +6 LUFS: the ceiling bites; h = 600, two blocks
CLIP_FLAGS = (1, 1, 1, 1, 0)
CLIP_SEED = 41


def set_clip_levels(batch, ceil, flags=CLIP_FLAGS):
    for s, (mode, gain) in enumerate(CLIP_LEVELS):
        if mode == LOUDNESS:
            batch.set_pcm_loudness(CLIP_TARGET, ceil, CLIP_FS, stream=s)
        else:
            batch.set_pcm_level(mode, gain, ceil, stream=s)
        batch.set_pcm_true_peak(bool(flags[s]), stream=s)
        assert batch.pcm_true_peak(s) == bool(flags[s])


def crest_tone(n, stream, channels=2):
    """[C, n]: a tone at a quarter of the sample rate whose samples straddle its crests -- its sample peak is 0.71 of its true peak in every
    period.  (A tone of any other frequency puts a sample near a crest sooner or later, and the synthetic clips of the other tests are such
    tones: their true peak is their sample peak.)"""
    t = np.arange(n)
    return np.stack([(1 - 0.1*c)*np.sin(2*np.pi*0.25*t + np.pi/4 + 0.05*stream) for c in range(channels)]).astype(np.float32)


def clip_frames(fmt):
    nin = CLIPS["inputs"]
    x = np.float32(0.4)*xc.clip_inputs(2, nin, loud=0)
    for s, n in enumerate(nin):
        x[s, :, :n] += np.float32(0.6)*crest_tone(n, s)
    frames = fc.encode_frames(pc.frames_of(x), fmt)
    return frames, np.ascontiguousarray(np.transpose(fc.decode_frames(frames, fmt), (0, 2, 1)))


def check_clips(lib, fmt, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """exactFrames of CLIPS with NORMALISE, PROTECT (biting), LOUDNESS (biting), FIXED and NORMALISE over the streams, the flag on all but the
    last: the true peaks are the mirror's of smst_batch_exact's planar output, bit for bit; the gains are clipGain restated with the true
    peak; the bytes are level_cases.mirror at that gain; the unflagged stream's bytes and gain are those of a twin batch without any flag;
    nothing is clamped at the clip-free ceiling; take_pcm_peaks still reports the sample peak.  Two calls."""
    pkg = package()
    taps = library_taps(lib)
    nin, nout = CLIPS["inputs"], CLIPS["outputs"]
    S, Cn, most = len(nin), 2, max(nout)
    dithered = fmt in dc.DITHERED_FORMATS
    frames, planar = clip_frames(fmt)
    p, f, u = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(3))
    xc.check_lengths(p, dict(inputs=nin, outputs=nout, short=None))
    ceil = lc.ceiling(fmt, dithered)
    modes = [dc.CLIP_MODES[s] if dithered else dc.NONE for s in range(S)]
    for b in (f, u):
        if dithered:
            for s in range(S):
                b.setPcmDither(modes[s], CLIP_SEED + s, stream=s)
    set_clip_levels(f, ceil)
    set_clip_levels(u, ceil, (0,)*S)
    assert f.take_pcm_true_peaks().tolist() == [0.0]*S                      # (nothing has measured yet)
    counters = ("clip_true_peak", "clip_peak", "clip_loudness", "clip_out_levelled")
    for call in range(2):
        want, ok_p = p.exact(planar, nout, in_samples=nin)
        want = np.array(want, copy=True)
        plain, _ = u.exactFrames(to_memory(frames), nout, in_samples=nin)
        plain = to_host(plain)
        _, plain_gains = u.take_pcm_peaks()
        assert u.take_pcm_true_peaks().tolist() == [0.0]*S
        out = np.full(frames.shape[:1] + (most,) + frames.shape[2:], 0x5A, frames.dtype)
        before = [pkg.launch_count(k, lib) for k in counters]
        got, ok_f = f.exactFrames(to_memory(frames), nout, in_samples=nin, out=to_memory(out))
        got = to_host(got)
        assert [pkg.launch_count(k, lib) - n for k, n in zip(counters, before)] == [1, 1, 1, 1]
        assert ok_p.all() and ok_f.all()
        tps = f.take_pcm_true_peaks()
        assert same_bits(tps, f.take_pcm_true_peaks())                      # (a take resets nothing)
        peaks, gains = f.take_pcm_peaks()
        overs = f.takePcmOvers()[0]
        expect = out.copy()
        lowered = 0
        for s in range(S):
            where = dict(fmt=fmt, call=call, stream=s)
            x = want[s, :, :nout[s]]
            mode, gain = CLIP_LEVELS[s]
            sample = lc.peak_of(x)
            tp = true_peak(x, taps)
            assert same_bits(peaks[s], sample), where
            assert same_bits(tps[s], tp if CLIP_FLAGS[s] else 0.0), (where, float(tps[s]), float(tp))
            compared["peaks"] += 1
            peak = tp if CLIP_FLAGS[s] else sample
            if mode == LOUDNESS:
                m = ld.mirror(x, CLIP_FS, None, CLIP_TARGET)
                q = lc.gain_of(PROTECT, np.float32(np.inf), ceil, peak)
                assert m["defined"] and float(m["gain"]) > 1.5*float(q), (where, m["lufs"], float(q))    # (the ceiling decides, by a wide margin)
                g = q
            else:
                g = lc.gain_of(mode, gain, ceil, peak)
            assert same_bits(gains[s], g), (where, float(gains[s]), float(g))
            if mode == PROTECT:
                assert g < gain
            if CLIP_FLAGS[s] and mode != FIXED:
                assert tp >= sample and g <= lc.gain_of(NORMALISE, 1.0, ceil, sample), where
                lowered += int(g < lc.gain_of(NORMALISE, 1.0, ceil, sample))                              # (the flag lowered the gain)
            codes, cm, _ = lc.mirror(x, fmt, g, modes[s], CLIP_SEED + s, 0)
            assert overs[s] == int(cm.sum()) and (mode == FIXED or overs[s] == 0), (where, int(overs[s]))
            expect[s, :nout[s]] = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
        assert lc.same_bytes(got.reshape(-1).view(np.uint8), expect.reshape(-1).view(np.uint8), fmt), (fmt, call)
        assert lowered >= 2, lowered                                           # (the clips' crests lie between their samples: the flag matters)
        last = S - 1
        assert np.array_equal(got[last, :nout[last]], plain[last, :nout[last]]) and same_bits(gains[last], plain_gains[last]), (fmt, call)
        assert not np.array_equal(got[0, :nout[0]], plain[0, :nout[0]]), (fmt, call)
    for b in (p, f, u):
        b.close()


def run_clips(lib, fmt=fc.S16):
    """the bytes, the true peaks, the peaks and the gains of one flagged call on a fresh batch"""
    pkg = package()
    frames, _ = clip_frames(fmt)
    b = pkg.StretchBatch(len(CLIPS["inputs"]), 2, lib=lib, seed=3, **pc.GEOMETRY)
    set_clip_levels(b, lc.ceiling(fmt, False))
    out, ok = b.exactFrames(frames, CLIPS["outputs"], in_samples=CLIPS["inputs"])
    res = [np.array(out, copy=True), ok, b.take_pcm_true_peaks()] + list(b.take_pcm_peaks())
    b.close()
    return res


def check_two_runs(lib):
    a, b = run_clips(lib), run_clips(lib)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert a[0].any() and (a[2] > 0).sum() == 4


# ---- 3. opt-in, steady state, refusals -------------------------------------------------------------------------------------------------

OPT_IN_COUNTERS = lc.LEVEL_COUNTERS + ("clip_loudness", "clip_out", "clip_out_dithered", "clip_in")


def check_opt_in(lib, **memory):
    """a levelled batch with the flag off on every stream: the whole-clip cases of level_cases.py -- bytes, peaks and gains against their
    mirror -- launch the pass zero times; a batch whose flags were turned on and off again gives the bytes, gains and launch counters of one
    that never had them; a flagged stream that a call leaves out does not start the pass"""
    pkg = package()
    to_memory, to_host = memory.get("to_memory", lambda a: a), memory.get("to_host", lambda a: np.array(a, copy=True))
    before = pkg.launch_count("clip_true_peak", lib)
    assert before >= 0, "the library has no clip_true_peak counter"
    lc.check_clips(lib, fc.S16, **memory)
    assert pkg.launch_count("clip_true_peak", lib) == before
    nin, nout = CLIPS["inputs"], CLIPS["outputs"]
    frames, _ = clip_frames(fc.S16)
    ceil = lc.ceiling(fc.S16, False)
    never, again = (pkg.StretchBatch(len(nin), 2, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(2))
    set_clip_levels(never, ceil, (0,)*5)
    assert lib.smst_batch_set_pcm_true_peak(again.h, -1, 1) == 0 and all(again.pcm_true_peak(s) for s in range(5))
    set_clip_levels(again, ceil, (0,)*5)                                       # (the level setters leave the flag; the last line of each stream clears it)
    results = []
    for b in (never, again):
        c0 = [pkg.launch_count(k, lib) for k in OPT_IN_COUNTERS + ("clip_true_peak",)]
        out, ok = b.exactFrames(to_memory(frames), nout, in_samples=nin)
        out = to_host(out)
        results.append((out, b.take_pcm_peaks()[1], [pkg.launch_count(k, lib) - n for k, n in zip(OPT_IN_COUNTERS + ("clip_true_peak",), c0)]))
        assert b.take_pcm_true_peaks().tolist() == [0.0]*5
    assert np.array_equal(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1]) and results[0][0].any()
    assert results[0][2] == results[1][2] and results[0][2][-1] == 0 and results[0][2][1:4] == [1, 1, 1], results
    again.set_pcm_true_peak(True, stream=1)
    for counts, ran in (([nout[0], -1, nout[2], -1, -1], 0), (nout, 1)):
        c0 = pkg.launch_count("clip_true_peak", lib)
        again.exactFrames(to_memory(frames), counts, in_samples=nin)
        again.synchronize()
        assert pkg.launch_count("clip_true_peak", lib) - c0 == ran, counts
    tps = again.take_pcm_true_peaks()
    assert tps[1] > 0 and not tps[[0, 2, 3, 4]].any()
    never.close()
    again.close()


def check_steady_state(lib, to_memory=lambda a: a):
    """the first flagged call grows the workspace by the true-peak words, a second call of the same shapes allocates nothing, nor do the takes"""
    pkg = package()
    nin, nout = CLIPS["inputs"][:3], CLIPS["outputs"][:3]
    clips = to_memory(np.ascontiguousarray(clip_frames(fc.S16)[0][:3]))
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_level(NORMALISE, 1.0, 0.9)
    for _ in range(2):
        b.exactFrames(clips, nout, in_samples=nin)
    b.synchronize()
    plain = b.workspaceBytes()
    b.set_pcm_true_peak(True)
    for _ in range(2):
        b.exactFrames(clips, nout, in_samples=nin)
    b.synchronize()
    events, grown = b.allocation_events(), b.workspaceBytes()
    assert grown == plain + 3*4, (plain, grown)
    b.exactFrames(clips, nout, in_samples=nin)
    tps = b.take_pcm_true_peaks()
    b.take_pcm_peaks()
    assert b.allocation_events() == events and b.workspaceBytes() == grown and (tps > 0).all()
    b.close()


def check_refusals(lib):
    pkg = package()
    b = pkg.StretchBatch(2, 3, lib=lib, **pc.GEOMETRY)
    for stream in (2, -2):
        assert lib.smst_batch_set_pcm_true_peak(b.h, stream, 1) == -1 and b"stream" in lib.smst_last_error()
    for stream in (2, -1):
        assert lib.smst_batch_pcm_true_peak(b.h, stream, None) == -1 and b"stream" in lib.smst_last_error()
    assert [b.pcm_true_peak(s) for s in range(2)] == [False, False]             # (a refused call changes nothing)
    assert lib.smst_batch_set_pcm_true_peak(None, 0, 1) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_true_peak(None, 0, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_take_pcm_true_peaks(None, None) == -1 and b"null" in lib.smst_last_error()
    # what is allowed: null pointers in the getter and the take; the flag beside every mode, untouched by the level setters
    assert lib.smst_batch_pcm_true_peak(b.h, 0, None) == 0 and lib.smst_batch_take_pcm_true_peaks(b.h, None) == 0
    b.set_pcm_true_peak(True, stream=1)
    b.set_pcm_level(PROTECT, 1.0, 0.9)
    b.set_pcm_loudness(-23.0, 1.0, 8000.0, stream=1)
    assert [b.pcm_true_peak(s) for s in range(2)] == [False, True] and b.pcm_level(1)[0] == LOUDNESS and b.pcm_level(0)[0] == PROTECT
    b.set_pcm_true_peak(False)
    assert [b.pcm_true_peak(s) for s in range(2)] == [False, False] and b.pcm_level(1)[0] == LOUDNESS
    b.close()


def check_refused_in_streaming_calls(lib, **memory):
    """a flagged stream that takes part makes processFrames and flushFrames fail before anything runs, whatever its mode; one that a flush
    leaves out by a negative count does not"""
    pkg = package()
    frames, _ = dc.session_inputs(fc.S16)
    to_memory = memory.get("to_memory", lambda a: a)
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_true_peak(True, stream=1)                                          # (the stream is in LEVEL_FIXED)
    x = to_memory(np.ascontiguousarray(frames[:, :600]))
    like = to_memory(np.zeros((1,), np.float32))
    for call in (lambda: b.processFrames(x, [600, 300, 0]), lambda: b.flushFrames([100, 50, -1], like=like)):
        with dc.pytest_raises(pkg.StretchError) as e:
            call()
        assert "true-peak" in str(e.value) and "error -1" in str(e.value), str(e.value)
    b.flushFrames([100, -1, 100], like=like)                                     # (stream 1 takes no part: not refused)
    b.set_pcm_true_peak(False, stream=1)
    b.processFrames(x, [600, 300, 0])
    b.close()


# ---- 4. the command-line tool ----------------------------------------------------------------------------------------------------------

def true_peak_lines(stdout):
    """the "level:" lines of a --true-peak run -> [(file, peak, gain, overs, dBTP)]"""
    found = re.findall(r"^level: (\S+) peak=(\S+) gain=(\S+) overs=(-?\d+) true-peak=(\S+)$", stdout, re.M)
    return [(name, np.float32(peak), np.float32(gain), int(overs), float(db)) for name, peak, gain, overs, db in found]


def check_cli(cli, tmp_path, lib):
    """--exact --true-peak --normalize=-1: the printed true peak is the mirror's of the --exact floats in dBTP, to the printed digits; the gain
    is ceiling/true peak; the file is level_cases.mirror of those floats at the printed gain, and its own mirror-measured true peak lies
    within one step of the format of -1 dBTP (every sample moves by half a step at the most, a phase's taps sum to 1.86 in magnitude at
    the most, and the fp32 gain adds 1e-7 relative: 0.93 steps).  Alone the flag only meters; without --exact it is refused; without it
    the lines are the ones level_cases.py parses."""
    from test_cli import write_wav16
    taps = library_taps(lib)
    sr, lengths = 8000, (2500, 2790)
    srcs = [str(tmp_path/("in%d.wav" % k)) for k in range(2)]
    write_wav16(srcs[0], 0.5*synth_input(1, 2, lengths[0], sr) + 0.4*crest_tone(lengths[0], 0), sr)
    write_wav16(srcs[1], 0.1*synth_input(2, 2, lengths[1], sr) + 0.25*crest_tone(lengths[1], 1), sr)

    def run(name, flags, expect=0):
        outs = [str(tmp_path/("%s%d.wav" % (name, k))) for k in range(2)]
        res = subprocess.run([cli, "--time=1.1"] + flags + [srcs[0], outs[0], srcs[1], outs[1]], capture_output=True, text=True)
        assert res.returncode == expect, (flags, res.returncode, res.stderr)
        return outs, res
    outs, _ = run("xf32", ["--exact", "--out-format=f32"])
    floats = []
    for path in outs:
        head, data = dc.data_chunk(path)
        assert head[:3] == (3, 2, sr)
        floats.append(np.ascontiguousarray(np.frombuffer(data, "<f4").reshape(-1, 2).T))
    assert max(f.shape[1] for f in floats) <= 3*T + 8
    tps = [true_peak(f, taps) for f in floats]
    ceil = 10**(-1/20)
    outs, res = run("norm", ["--exact", "--true-peak", "--normalize=-1", "--out-format=s16"])
    lines = true_peak_lines(res.stdout)
    assert len(lines) == 2 and not lc.level_lines(res.stdout), res.stdout
    for k, (path, peak, gain, overs, db) in enumerate(lines):
        assert path == outs[k] and peak == lc.peak_of(floats[k]) and overs == 0 and tps[k] > peak, (k, lines[k])
        assert abs(db - 20*math.log10(float(tps[k]))) <= 5.1e-5, (k, db, float(tps[k]))
        q = ceil/float(tps[k])
        assert abs(float(gain) - q) <= 1e-6*q, (k, float(gain), q)
        head, data = dc.data_chunk(path)
        assert head == (1, 2, sr, sr*4, 4, 16)
        codes, cm, _ = lc.mirror(floats[k], fc.S16, gain, dc.NONE, k, 0)
        assert np.array_equal(np.frombuffer(data, "<i2"), codes.reshape(-1)) and not cm.any(), k
        written = np.ascontiguousarray(codes.T).astype(np.float32)/np.float32(32768)
        assert abs(float(true_peak(written, taps)) - ceil) <= 1/32768, (k, float(true_peak(written, taps)), ceil)
    # alone: metered only
    outs, res = run("meter", ["--exact", "--true-peak", "--out-format=s16"])
    lines = true_peak_lines(res.stdout)
    assert [(l[2], "%.4f" % l[4]) for l in lines] == [(1.0, "%.4f" % (20*math.log10(float(t)))) for t in tps], lines
    # without the flag: the lines of today
    _, res = run("plain", ["--normalize=-1", "--out-format=s16"])
    assert len(lc.level_lines(res.stdout)) == 2 and not true_peak_lines(res.stdout) and "true-peak" not in res.stdout
    flagged = true_peak_lines(run("again", ["--true-peak", "--normalize=-1"])[1].stdout)                 # (--normalize implies --exact)
    assert all(a[2] > b[2] for a, b in zip(lc.level_lines(res.stdout), flagged)) and len(flagged) == 2    # (a dBTP ceiling: the lower gain)
    _, res = run("bad", ["--true-peak"], expect=2)
    assert "--exact" in res.stderr
