"""Shared cases of the stream limiter's true-peak flag (include/smst.h, "Stream limiter", "True-peak detector"):
test_stream_limiter_true_peak_emu.py runs them on the CPU stand-in, test_stream_limiter_true_peak_gpu.py on the device, next to
stream_limiter_cases.py.

The definition is the clip limiter's WITH its true-peak flag, applied to the clip [D frames of +0.0, every frame emitted so far], D = 2H + 6:
the mirror below is three lines over limiter_cases' need_of, gain_curve and limited.  As there, every comparison of r, frames, integer codes
and meters is one of BIT PATTERNS -- no tolerance appears anywhere; a NaN of the float32 output equals any other NaN."""
import numpy as np

import dither_cases as dc
import level_cases as lc
import limiter_cases as lm
import pcm_cases as pc
import pcm_format_cases as fc
import stream_limiter_cases as sl
import true_peak_cases as tp
from conftest import package

T = lm.T
ON, TRUE_PEAK = 1, 2                                 # the bits of the hook's flags
FLAGGED = ON | TRUE_PEAK
DELAY = 6                                            # SMST_STREAM_LIMITER_TRUE_PEAK_DELAY
COUNTERS = ("pcm_limit_feed", "pcm_limit_feed_true_peak", "pcm_limit_gain", "pcm_out_limited")
OLD_COUNTERS = sl.OLD_COUNTERS
compared = dict(frames=0)                            # frames of r compared bit for bit with the mirror so far (printed by the tests; EXPERIMENTS.md)
same_bits, meters_of, drive = sl.same_bits, sl.meters_of, sl.drive


def delay_of(H, flags=FLAGGED):
    return 0 if not flags & ON else 2*H + (DELAY if flags & TRUE_PEAK else 0)


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def mirror(v, g, ceil, H, win, taps):
    """v [C, T] float32, the frames emitted so far -> (r [T], u [C, T]): the first T frames of the clip [2H + 6 zeros, v], limited with the
    true-peak phases in the detector"""
    x = np.concatenate([np.zeros((v.shape[0], 2*H + DELAY), np.float32), np.asarray(v, np.float32)], axis=1)
    r = lm.gain_curve(lm.need_of(x, abs(np.float32(g)), ceil, True, taps), H, win)[:v.shape[1]]
    return r, lm.limited(x[:, :v.shape[1]], g, r)


def mirror_of(flags, v, g, ceil, H, win, taps):
    """the mirror of a stream of the hook: flagged, limited without the flag (stream_limiter_cases.mirror) or without the setting"""
    if flags & ON:
        return mirror(v, g, ceil, H, win, taps) if flags & TRUE_PEAK else sl.mirror(v, g, ceil, H, win)
    return np.ones(v.shape[1], np.float32), lc.levelled(v, g)


KNOWN_1 = "3f7bba48 3f6ee91e 3f5dd23c 3f510112 3f4cbb59 3f510112 3f5dd23c 3f6ee91e 3f7bba48"
KNOWN_2 = "3f732ed6 3f598c83 3f4cbb59 3f598c83 3f732ed6"


def known_inputs():
    a = np.zeros((1, 24), np.float32)
    a[0, 6:8] = 1
    b = np.zeros((1, 12), np.float32)
    b[0, 0:2] = 1
    return a, b


def assert_known(first, second):
    """first, second: (r, frames of the one channel, min gain, limited frames) of the two known answers of include/smst.h"""
    r, u, low, count = first
    assert lm.hexes(r) == " ".join(["3f800000"]*12 + [KNOWN_1] + ["3f800000"]*3), lm.hexes(r)
    assert lm.hexes(u[16:18]) == "3f4cbb59 3f510112" and not np.delete(u, [16, 17]).view(np.uint32).any(), lm.hexes(u)
    assert lm.hexes(low) == "3f4cbb59" and int(count) == 9
    r, u, low, count = second
    assert lm.hexes(r) == " ".join(["3f800000"]*6 + [KNOWN_2] + ["3f800000"]), lm.hexes(r)
    assert lm.hexes(u) == " ".join(["80000000"]*8 + ["bf4cbb59", "bf598c83"] + ["80000000"]*2), lm.hexes(u)
    assert int(count) == 5


PREFIX_H = (1, 2, 3, 8, 72)


def prefix_lengths(H):
    return sorted(set([1, 5, 6, 7, 11, 12, 13, 2*H + 5, 2*H + 6, 2*H + 7, 300, 699]))


def check_mirror():
    """the two known answers of include/smst.h; the need of the inter-sample crest; prefix invariance: every prefix of a stream gives the
    bits of the longer clip, so the result does not depend on the cuts"""
    taps = tp.formula_taps()
    a, b = known_inputs()
    r, u = mirror(a, 1.0, 1.0, 2, lm.formula_window(2), taps)
    first = (r, u[0]) + meters_of(r)
    r, u = mirror(b, -1.0, 1.0, 1, lm.formula_window(1), taps)
    assert_known(first, (r, u[0]) + meters_of(r))
    assert lm.hexes(np.float32(1)/tp.true_peak(np.ones((1, 2), np.float32), taps)) == "3f4cbb59"
    rng = pc._rng(9601)
    for H in PREFIX_H:
        x, g = drive(lm._signal(rng, "noise", 2, 699, 0, H))
        win = lm.formula_window(H)
        whole = mirror(x, g, 0.5, H, win, taps)
        assert (whole[0] < 1).any()
        for n in prefix_lengths(H):
            part = mirror(x[:, :n], g, 0.5, H, win, taps)
            assert same_bits(part[0], whole[0][:n]) and same_bits(part[1], whole[1][:, :n]), (H, n)


# ---- the hook ------------------------------------------------------------------------------------------------------------------------

def run_hook(lib, clips, cuts, H, gains, ceilings, flags):
    """stream_limiter_cases.run_hook with flags of two bits -> (r [S, most], frames [S, most, C], min gain [S], limited frames [S]).  Per call
    in which a stream with the setting has frames the gain pass and the conversion are launched once, and each feed kernel once where a
    stream of its kind has frames"""
    pkg = package()
    S, Cn = len(clips), clips[0].shape[0]
    most = max(max(x.shape[1] for x in clips), 1)
    image = np.zeros((S, Cn, most), np.float32)
    for s, x in enumerate(clips):
        assert sum(max(c, 0) for c in cuts[s]) == x.shape[1] and len(cuts[s]) == len(cuts[0])
        image[s, :, :x.shape[1]] = x
    counts = np.ascontiguousarray(np.asarray(cuts, np.int32).T)
    calls = range(counts.shape[0])
    plain = sum(int(any(flags[s] & FLAGGED == ON and counts[k, s] > 0 for s in range(S))) for k in calls)
    late = sum(int(any(flags[s] & FLAGGED == FLAGGED and counts[k, s] > 0 for s in range(S))) for k in calls)
    either = sum(int(any(flags[s] & ON and counts[k, s] > 0 for s in range(S))) for k in calls)
    before = [pkg.launch_count(k, lib) for k in COUNTERS]
    assert min(before) >= 0, "the library has no counter of the true-peak feed kernel"
    out = pkg.debug_pcm_stream_limit(counts, Cn, image, Cn*most, most, gains, ceilings, flags, H, most, lib=lib)
    assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS, before)] == [plain, late, either, either]
    return out


def compare_hook(lib, clips, cuts, H, gains, ceilings, flags):
    """r, the float32 frames and both meters equal the mirror's as bit patterns, for every stream: a flagged stream against the mirror above,
    a limited one without the flag against stream_limiter_cases' -- today's bits, 2H late --, one without the setting against the levelled
    form, not delayed"""
    win, taps = lm.library_window(lib, H), tp.library_taps(lib)
    r, frames, low, count = run_hook(lib, clips, cuts, H, gains, ceilings, flags)
    mirrors = []
    for s, x in enumerate(clips):
        n = x.shape[1]
        where = dict(stream=s, C=x.shape[0], n=n, H=H, cuts=list(cuts[s]), flags=flags[s], gain=float(gains[s]), ceiling=float(ceilings[s]))
        mr, mu = mirror_of(flags[s], x, gains[s], ceilings[s], H, win, taps)
        bad = np.flatnonzero(r[s, :n].view(np.uint32) != mr.view(np.uint32))
        assert not len(bad), (where, bad[:8].tolist(), lm.hexes(r[s, bad[:4]]), lm.hexes(mr[bad[:4]]))
        assert same_bits(frames[s, :n], mu.T), (where, np.argwhere(frames[s, :n].view(np.uint32) != np.ascontiguousarray(mu.T).view(np.uint32))[:4].tolist())
        assert (r[s, n:] == 1).all() and not frames[s, n:].any(), where
        ml, mc = meters_of(mr)
        assert same_bits(low[s], ml) and int(count[s]) == mc, (where, float(low[s]), float(ml), int(count[s]), mc)
        compared["frames"] += n
        mirrors.append((mr, mu))
    return mirrors


def cut_counts(H):
    """0, a stream that takes no part, 1, the counts around the 5 and 6 frames the taps reach and around their 11 and 12, around the delay
    (2H + 6), the need line (4H), a tile with the taps' reach on either side, and beyond two tiles"""
    return [0, -1, 1, 5, 6, 7, 11, 12, 2*H + 5, 2*H + 6, 2*H + 7, 4*H, 4*H + 1, T - 7, T - 6, T, T + 5, T + 6, 2*T + 3]


SETTINGS = ("flag", "flag_negative", "plain", "off", "inf")
STREAM_KINDS = ("spikes", "am", "noise", "noise", "am")
# At H = 1024 the curve of the AM tone is nearly flat -- hold is the window's one loudest crest, which a sample often sits on --, and the
# flag changes 0.39 to 0.48 of its frames on the mirror (1 and 2 channels; 0.53 to 0.998 at H = 1, 2, 3 and 72), so check_flag_matters' "at
# least half" cannot be stated for it there.  The one variant run at that lookahead is the one that gives the flag to the two noise streams
# (1.000 of the frames); the AM tones then run without the flag and with a ceiling of +inf, the spikes with the setting off
LONGEST_VARIANTS = (3,)


def check_flag_matters(kind, x, g, H, win, taps):
    """on the mirror: the true-peak curve differs in bit pattern from the sample-peak curve 6 frames later in at least half of the frames of
    an AM tone or of noise and in at least one frame of the spikes: a library that ignores the flag cannot pass"""
    with_flag = mirror(x, g, 0.5, H, win, taps)[0]
    without = sl.mirror(np.concatenate([np.zeros((x.shape[0], DELAY), np.float32), x], axis=1), g, 0.5, H, win)[0][:x.shape[1]]
    share = float((with_flag.view(np.uint32) != without.view(np.uint32)).mean())
    assert share >= 0.5 if kind != "spikes" else share > 0, (kind, H, share)
    return share


def check_hook(lib, channels, H, variants=(0, 2)):
    """five streams in one sequence of calls, each with the counts of cut_counts(H) in an order of its own: limiter_cases' three signal kinds,
    then noise and an AM tone again, each driven 12 dB over a ceiling of 0.5.  The settings -- the flag, the flag with a negative gain, the
    setting without the flag, the setting off, the flag with a ceiling of +inf -- move round the streams from one variant to the next"""
    counts = cut_counts(H)
    n = sum(max(c, 0) for c in counts)
    taps = tp.library_taps(lib)
    win = lm.library_window(lib, H)
    for variant in variants:
        rng = pc._rng(9602, channels, H, variant)
        clips, cuts, gains, ceilings, flags, settings = [], [], [], [], [], []
        for s in range(5):
            x, g = drive(lm._signal(rng, STREAM_KINDS[s], channels, n, s, H))
            setting = SETTINGS[(s + variant) % 5]
            clips.append(x)
            cuts.append(counts[4*s:] + counts[:4*s])
            gains.append(-g if setting == "flag_negative" else g)
            ceilings.append(np.float32(np.inf) if setting == "inf" else np.float32(0.5))
            flags.append({"off": 0, "plain": ON}.get(setting, FLAGGED))
            settings.append(setting)
            if setting in ("flag", "flag_negative"):
                print("H %d, %d channels, %s: the flag changes %.3f of the frames" % (H, channels, STREAM_KINDS[s], check_flag_matters(STREAM_KINDS[s], x, gains[s], H, win, taps)))
        mirrors = compare_hook(lib, clips, cuts, H, gains, ceilings, flags)
        for s, (mr, mu) in enumerate(mirrors):
            setting, D = settings[s], delay_of(H, flags[s])
            assert (mr < 1).any() == (setting in ("flag", "flag_negative", "plain")), (s, setting)
            if setting == "inf":                                                 # (a delay only)
                assert same_bits(mu[:, D:], lc.levelled(clips[s][:, :n - D], gains[s])) and not mu[:, :D].any()
            if setting in ("flag", "flag_negative", "plain"):
                assert float(lc.peak_of(mu)) <= 0.5*(1 + 2.0**-22), (s, float(lc.peak_of(mu)))
    print("frames of r bit-identical to the mirror so far: %d" % compared["frames"])


def check_known_answers(lib):
    """the two known answers through the hook, cut as include/smst.h cuts them"""
    a, b = known_inputs()
    r, frames, low, count = run_hook(lib, [a], [[5, 1, 7, 11]], 2, [1.0], [1.0], [FLAGGED])
    first = (r[0], frames[0, :, 0], low[0], count[0])
    r, frames, low, count = run_hook(lib, [b], [[3, 9]], 1, [-1.0], [1.0], [FLAGGED])
    assert_known(first, (r[0], frames[0, :, 0], low[0], count[0]))


def check_cut_invariance(lib, H=lm.DEFAULT_H, channels=2, n=2*T + 300):
    """one flagged stream as one call, as 128-frame quanta and as drawn cuts: r, the frames and the meters are identical (and the mirror's)"""
    rng = pc._rng(9603)
    x, g = drive(lm._signal(rng, "noise", channels, n, 0, H))
    quanta = [128]*(n//128) + [n % 128]
    drawn = [3, 0]                                                               # (a call without frames among them)
    while sum(drawn) < n:
        drawn.append(min(int(rng.integers(0, 4*H + 40)), n - sum(drawn)))
    results = []
    for cuts in ([n], quanta, drawn):
        compare_hook(lib, [x], [cuts], H, [g], [np.float32(0.5)], [FLAGGED])
        results.append(run_hook(lib, [x], [cuts], H, [g], [np.float32(0.5)], [FLAGGED]))
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (results[0][0] < 1).any() and len(drawn) > 8 and 0 in drawn


def check_nan_inf(lib):
    """stream_limiter_cases.check_nan_inf's contract with the flag: a NaN is skipped by the detector -- the sample's word and every phase
    sum that it enters --, an inf gives need 1 where it is the largest word, the NaN stays a NaN in the float32 output and the inf an inf;
    planted around the cuts, where the line carries them"""
    rng = pc._rng(9604)
    H = 8
    cuts = [[300, 1, 2*H, 4*H + 1, T + 50 - 300 - 1 - 2*H - 4*H - 1]]*3
    clips, gains = [], []
    for s in range(3):
        x, g = drive(lm._signal(rng, "noise", 2, T + 50, s, H))
        clips.append(x)
        gains.append(g if s != 1 else -g)
    clips[0][0, 299], clips[0][1, 300] = np.nan, np.inf                          # (the last frame of a call, the only frame of the next one)
    clips[1][0, 301 + 2*H - 1], clips[1][1, 10] = -np.inf, np.nan
    clips[2][:, 500] = np.nan                                                    # (every channel: the sample's word is 0)
    clips[2][0, 0] = np.inf
    m = compare_hook(lib, clips, cuts, H, gains, [np.float32(0.5)]*3, [FLAGGED]*3)
    taps = tp.library_taps(lib)
    D = delay_of(H)
    for s, spots in ((0, (300,)), (1, (301 + 2*H - 1,)), (2, (0,))):
        x = np.concatenate([np.zeros((2, D), np.float32), clips[s]], axis=1)
        need = lm.need_of(x, abs(gains[s]), 0.5, True, taps)
        for at in spots:
            assert need[D + at] == 1, (s, at)                                    # (the inf is the frame's largest word: w is not finite)
        assert (m[s][0] < 1).any()
    u = m[0][1]
    assert np.isnan(u[0, D + 299]) and np.isinf(u[1, D + 300]) and np.isfinite(u[1, D + 299])


def check_reproducible(lib):
    rng = pc._rng(9605)
    H = lm.DEFAULT_H
    clips = [drive(lm._signal(rng, k, 3, 2*T + 3, s, H))[0] for s, k in enumerate(lm.KINDS)]
    cuts = [[T + 1, 0, T + 2], [128, 2*T - 125, 0], [1, 1, 2*T + 1]]
    runs = [run_hook(lib, clips, cuts, H, [2.0, -2.0, 2.0], [0.5]*3, [FLAGGED, FLAGGED, ON]) for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (runs[0][0] < 1).any(axis=1).all()


# ---- end to end: processFrames and flushFrames ----------------------------------------------------------------------------------------------

GAINS = sl.GAINS                                                                 # 8, 0.5, -4
KINDS = (FLAGGED, 0, ON)                                                         # per stream: flagged, without the setting, limited without the flag


def session_of(H):
    """dither_cases.SESSION with its flush asked for 2H + 6 frames more"""
    return dict(dc.SESSION, flush=[n + 2*H + DELAY if n >= 0 else n for n in dc.SESSION["flush"]])


def set_session(batch, ceil, H=None, kinds=KINDS):
    if H is not None:
        batch.set_pcm_limiter_lookahead(H)
    for s, g in enumerate(GAINS):
        batch.set_pcm_level(lc.FIXED, g, stream=s)
        batch.set_pcm_stream_limiter(bool(kinds[s] & ON), ceil, stream=s)
        if kinds[s] & TRUE_PEAK:
            batch.set_pcm_stream_limiter_true_peak(True, stream=s)


_twins = {}


def twin_session(lib, fmt, H):
    """what a twin batch of the same seed, geometry and calls writes as float32 frames without any level: per call [S, n, C]; computed once
    per library, format and lookahead and left unchanged"""
    key = (id(lib), fmt, H)
    if key not in _twins:
        t = package().StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
        _twins[key] = dc.frame_session(t, pc.frames_of(dc.session_inputs(fmt)[1]), fc.F32, session_of(H))
        t.close()
    return _twins[key]


def run_session(lib, fmt, dithered, H=lm.DEFAULT_H, kinds=KINDS, **memory):
    """the limited session on a fresh batch -> (the calls' frames, the batch)"""
    b = package().StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    set_session(b, lc.ceiling(fmt, dithered), H if H != lm.DEFAULT_H else None, kinds)
    if dithered:
        dc.set_session_dither(b)
    return dc.frame_session(b, dc.session_inputs(fmt)[0], fmt, session_of(H), **memory), b


def check_session(lib, fmt, dithered, H=lm.DEFAULT_H, **memory):
    """processFrames twice and flushFrames, asked for 2H + 6 frames more, with the gains 8, 0.5 and -4: the first stream flagged, the second
    without the setting, the third limited without the flag.  The bytes are the format's rule and the dither of the running counter on the
    mirror's u of the twin's float32 frames; the peaks are those of the frames written; the overs are the mirror's; the limiter's meters
    accumulate over the three calls and a second take gives 1 and 0.  The flagged total is the twin's, frame for frame, 2H + 6 frames late"""
    pkg = package()
    session, win, taps = session_of(H), lm.library_window(lib, H), tp.library_taps(lib)
    ceil = lc.ceiling(fmt, dithered)
    twin = twin_session(lib, fmt, H)
    counts = dc.session_counts(session)
    before = [pkg.launch_count(k, lib) for k in COUNTERS + OLD_COUNTERS]
    got, b = run_session(lib, fmt, dithered, H, **memory)
    ran = [sum(int(any(KINDS[s] & FLAGGED == kind and n[s] > 0 for s in range(3))) for n in counts) for kind in (ON, FLAGGED)]
    assert ran == [2, 3]                                                         # (a call in which only the flagged stream has frames is among them)
    assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS + OLD_COUNTERS, before)] == ran + [3, 3, 0, 0, 0]
    assert b.pcm_stream_limiter_latency() == 2*H and [b.pcm_stream_limiter_latency_of(s) for s in range(3)] == [2*H + DELAY, 0, 2*H]
    assert [b.pcm_stream_limiter_true_peak(s) for s in range(3)] == [True, False, False]
    modes = dc.SESSION_MODES if dithered else (dc.NONE,)*3
    clamped = np.zeros(3, np.int64)
    low, count = b.take_pcm_stream_limiter()
    peaks, gains = b.take_pcm_peaks()
    for s in range(3):
        where = dict(fmt=fmt, dithered=dithered, stream=s)
        v = np.concatenate([np.ascontiguousarray(t[s, :n[s]].T) for t, n in zip(twin, counts)], axis=1)     # [C, total]
        total, D = v.shape[1], delay_of(H, KINDS[s])
        r, u = mirror_of(KINDS[s], v, GAINS[s], ceil, H, win, taps)
        written = np.concatenate([np.zeros((2, D), np.float32), v], axis=1)[:, :total]
        ml, mc = meters_of(r)
        assert same_bits(low[s], ml) and int(count[s]) == mc and (mc > 0) == bool(KINDS[s]), (where, float(low[s]), float(ml), int(count[s]), mc)
        assert same_bits(u[:, D:], lm.limited(v[:, :total - D], GAINS[s], r[D:])), where                 # (the twin's frames, D late)
        compared["frames"] += total
        assert same_bits(peaks[s], lc.peak_of(written)) and gains[s] == np.float32(GAINS[s]), (where, float(peaks[s]))
        first = 0
        for k, n in enumerate(counts):
            codes, cm, _ = dc.mirror(u[:, first:first + n[s]], fmt, modes[s], dc.SESSION_SEED + s, first)
            want = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
            assert lc.same_bytes(np.ascontiguousarray(got[k][s, :n[s]]).reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8), fmt), (where, "call", k)
            clamped[s] += cm.sum()
            first += n[s]
        if dithered:
            assert b.pcmDither(s)[2] == total, where
        if KINDS[s]:
            assert clamped[s] == 0, where                                        # (the clip-free ceiling)
    assert b.takePcmOvers()[0].tolist() == clamped.tolist()
    again = b.take_pcm_stream_limiter()
    assert again[0].tolist() == [1.0]*3 and again[1].tolist() == [0]*3
    b.close()
    return got


def check_two_runs(lib, **memory):
    a, b = (run_session(lib, fc.S16, True, **memory) for _ in range(2))
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)
    for x, y in zip(a[1].take_pcm_stream_limiter(), b[1].take_pcm_stream_limiter()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and x.any()
    a[1].close()
    b[1].close()


# ---- behind a stream output resample ------------------------------------------------------------------------------------------------------

OUT_RATIO = (147, 160)                                                           # 48 kHz rendered, 44.1 kHz delivered
METER_FS = 2570.0                                                                # what the meter is told: h = 257, so that the short session has blocks


def check_behind_out_resample(lib, H=lm.DEFAULT_H, **memory):
    """three batches of the same seed, geometry, calls and stream output resample, float32 frames, the stream meter on: one without any
    level, whose frames are the delivered ones v; one with the stream limiter as it is today; one with the flag on the first two streams.
    The limiter sees the delivered frames: the flagged streams' frames are the mirror of v, 2H + 6 late behind the resample's Dl, the third
    stream's and the unflagged batch's today's; the meter measures v in all three, so the readings are those of the session without the flag"""
    pkg = package()
    taps, win = tp.library_taps(lib), lm.library_window(lib, H)
    g, ceil = np.float32(6.0), np.float32(0.5)
    frames = pc.frames_of(dc.session_inputs(fc.F32)[1])
    kinds = (FLAGGED, FLAGGED, ON)
    outs, takes, meters = [], [], []
    for which in ("delivered", "plain", "flag"):
        b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
        b.set_pcm_stream_out_resample(*OUT_RATIO)
        b.set_pcm_stream_meter(True, METER_FS, 64)
        Dl = b.stream_out_resample_latency(0)
        if which != "delivered":
            b.set_pcm_level(lc.FIXED, g)
            b.set_pcm_stream_limiter(True, ceil)
        if which == "flag":
            for s in range(3):
                b.set_pcm_stream_limiter_true_peak(bool(kinds[s] & TRUE_PEAK), stream=s)
            assert [b.stream_out_resample_latency(s) + b.pcm_stream_limiter_latency_of(s) for s in range(3)] == [Dl + 2*H + DELAY]*2 + [Dl + 2*H] and Dl > 0
        session = dict(dc.SESSION, flush=[n + Dl + 2*H + DELAY if n >= 0 else n for n in dc.SESSION["flush"]])
        outs.append(dc.frame_session(b, frames, fc.F32, session, **memory))
        meters.append(b.take_pcm_stream_meter())
        takes.append(b.take_pcm_stream_limiter())
        b.close()
    counts = dc.session_counts(session)
    for s in range(3):
        v, plain, flag = (np.concatenate([np.ascontiguousarray(t[s, :n[s]].T) for t, n in zip(out, counts)], axis=1) for out in outs)
        assert not v[:, :Dl].any() and v[:, Dl:].any(), s                       # (the delivered frames come Dl late)
        r, u = sl.mirror(v, g, ceil, H, win)
        assert same_bits(plain, u) and meters_of(r)[1] > 0, s
        assert same_bits(takes[1][0][s], meters_of(r)[0]) and int(takes[1][1][s]) == meters_of(r)[1], s
        r, u = mirror_of(kinds[s], v, g, ceil, H, win, taps)
        assert same_bits(flag, u) and not u[:, :Dl + delay_of(H, kinds[s])].any(), s
        assert same_bits(takes[2][0][s], meters_of(r)[0]) and int(takes[2][1][s]) == meters_of(r)[1], s
        assert (kinds[s] & TRUE_PEAK) == 0 or not same_bits(flag[:, DELAY:], plain[:, :-DELAY]), s   # (the flag is not a delay alone)
        compared["frames"] += v.shape[1]
    for key in meters[0]:
        for other in meters[1:]:
            assert np.array_equal(meters[0][key].view(np.uint8), other[key].view(np.uint8)), key
    assert (meters[0]["blocks"] > 0).any() and (meters[0]["true_peaks"] > 0).all()  # (the longest stream has 400-ms blocks)


# ---- opt-in, steady state, getters, refusals, clearing -----------------------------------------------------------------------------------------

def check_opt_in(lib, **memory):
    """a batch that never sets the flag, and one that sets it and clears it again, run stream_limiter_cases' session with today's counters
    -- the new one does not move -- and today's bytes; workspaceBytes is today's up to the first call with the flag on, which adds the
    flag's lines; a call with a flagged stream counts the new kernel"""
    pkg = package()
    H = lm.DEFAULT_H
    ceil = lc.ceiling(fc.S16, True)
    runs = []
    for toggled in (False, True):
        b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
        sl.set_session(b, ceil)
        dc.set_session_dither(b)
        size = b.workspaceBytes()
        if toggled:
            b.set_pcm_stream_limiter_true_peak(False)                                # (off: nothing is allocated)
            assert b.workspaceBytes() == size
            b.set_pcm_stream_limiter_true_peak(True, stream=0)
            assert b.workspaceBytes() == size + 2*3*2*(2*H + 11)*4, (size, b.workspaceBytes())
            b.set_pcm_stream_limiter_true_peak(False, stream=0)
        before = [pkg.launch_count(k, lib) for k in COUNTERS + OLD_COUNTERS]
        assert min(before) >= 0, "the library has no counter of the true-peak feed kernel"
        runs.append(dc.frame_session(b, dc.session_inputs(fc.S16)[0], fc.S16, sl.session_of(H), **memory))
        assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS + OLD_COUNTERS, before)] == [3, 0, 3, 3, 0, 0, 0]
        assert [b.pcm_stream_limiter_latency_of(s) for s in range(3)] == [2*H, 0, 2*H]
        b.close()
    for x, y in zip(*runs):
        assert np.array_equal(x, y) and x.any()
    # the flag alone, on a batch without the setting: inert -- the unlevelled kernels, no delay
    plain, b = (pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY) for _ in range(2))
    b.set_pcm_stream_limiter_true_peak(True)
    before = [pkg.launch_count(k, lib) for k in COUNTERS]
    x, y = (dc.frame_session(t, dc.session_inputs(fc.S16)[0], fc.S16, dc.SESSION, **memory) for t in (plain, b))
    assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS, before)] == [0]*4
    assert [b.pcm_stream_limiter_latency_of(s) for s in range(3)] == [0]*3 and all(b.pcm_stream_limiter_true_peak(s) for s in range(3))
    for p, q in zip(x, y):
        assert np.array_equal(p, q) and p.any()
    plain.close()
    b.close()


def check_steady_state(lib, to_memory=lambda a: a):
    """the setter allocates the flag's lines outside any call; the first limited call grows the rows once; a second call of the same shapes
    leaves allocation_events and workspaceBytes where they are, as do the takes"""
    pkg = package()
    S, Cn, H = 3, 2, 8
    frames, _ = dc.session_inputs(fc.S16)
    x = to_memory(np.ascontiguousarray(frames[:, :640]))
    b = pkg.StretchBatch(S, Cn, lib=lib, **pc.GEOMETRY)
    b.set_pcm_level(lc.FIXED, 4.0)
    for _ in range(2):
        b.processFrames(x, [600, 300, 128])
    b.synchronize()
    b.set_pcm_limiter_lookahead(H)
    b.set_pcm_stream_limiter(True, 0.5)
    lines = b.workspaceBytes()
    b.set_pcm_stream_limiter_true_peak(True, stream=0)
    flagged = b.workspaceBytes()
    assert flagged == lines + 2*S*Cn*(2*H + 11)*4, (lines, flagged)
    b.set_pcm_stream_limiter_true_peak(True, stream=2)
    assert b.workspaceBytes() == flagged
    b.processFrames(x, [600, 300, 128])
    b.synchronize()
    events, grown = b.allocation_events(), b.workspaceBytes()
    assert grown >= flagged + S*(4*H + 2*600)*4, (flagged, grown)
    for _ in range(3):
        b.processFrames(x, [600, 300, 128])
        low, count = b.take_pcm_stream_limiter()
        b.take_pcm_peaks()
    b.flushFrames([100, 100, 100], like=to_memory(np.zeros((1,), np.float32)))
    assert b.allocation_events() == events and b.workspaceBytes() == grown and (count > 0).all() and (low < 1).all()
    # another lookahead: the lines are made again for it, outside any call
    b.set_pcm_limiter_lookahead(3)
    assert [b.pcm_stream_limiter_latency_of(s) for s in range(3)] == [12, 6, 12]
    b.processFrames(x, [600, 300, 128])
    b.synchronize()
    events = b.allocation_events()
    b.processFrames(x, [600, 300, 128])
    assert b.allocation_events() == events
    b.close()


def check_refusals(lib, **memory):
    pkg = package()
    to_memory = memory.get("to_memory", lambda a: a)
    assert pkg.STREAM_LIMITER_TRUE_PEAK_DELAY == DELAY
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    H = lm.DEFAULT_H
    state = lambda: ([(b.pcm_stream_limiter_true_peak(s), b.pcm_stream_limiter_latency_of(s)) for s in range(3)], b.workspaceBytes(), b.allocation_events())
    start = state()
    assert start[0] == [(False, 0)]*3
    for stream in (3, -2):
        assert lib.smst_batch_set_pcm_stream_limiter_true_peak(b.h, stream, 1) == -1 and b"stream" in lib.smst_last_error()
    for stream in (3, -1):
        assert lib.smst_batch_pcm_stream_limiter_true_peak(b.h, stream, None) == -1 and b"stream" in lib.smst_last_error()
        assert lib.smst_batch_pcm_stream_limiter_latency_of(b.h, stream, None) == -1 and b"stream" in lib.smst_last_error()
    assert state() == start                                                      # (a refused call changes nothing)
    assert lib.smst_batch_set_pcm_stream_limiter_true_peak(None, 0, 1) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_stream_limiter_true_peak(None, 0, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_stream_limiter_latency_of(None, 0, None) == -1 and b"null" in lib.smst_last_error()
    # what is allowed: null pointers in the getters; the flag before the setting, and beside it
    assert lib.smst_batch_pcm_stream_limiter_true_peak(b.h, 0, None) == 0 and lib.smst_batch_pcm_stream_limiter_latency_of(b.h, 0, None) == 0
    b.set_pcm_stream_limiter_true_peak(True, stream=1)
    assert [b.pcm_stream_limiter_latency_of(s) for s in range(3)] == [0, 0, 0]   # (inert while the setting is off)
    b.set_pcm_stream_limiter(True, 0.5)
    assert [b.pcm_stream_limiter_latency_of(s) for s in range(3)] == [2*H, 2*H + DELAY, 2*H] and b.pcm_stream_limiter_latency() == 2*H
    assert [b.pcm_stream_limiter(s) for s in range(3)] == [(True, 0.5)]*3 and [b.pcm_stream_limiter_true_peak(s) for s in range(3)] == [False, True, False]
    b.set_pcm_limiter_lookahead(5)
    assert [b.pcm_stream_limiter_latency_of(s) for s in range(3)] == [10, 16, 10] and b.pcm_stream_limiter_latency() == 10
    # the whole-clip true-peak flag is another setting, and stays refused in the streaming calls; exactFrames keeps refusing the setting
    frames, _ = dc.session_inputs(fc.S16)
    assert not b.pcm_true_peak(1)
    clip, n = to_memory(np.ascontiguousarray(frames)), frames.shape[1]
    with dc.pytest_raises(pkg.StretchError) as e:
        b.exactFrames(clip, [n + 100]*3)
    assert "smst_batch_set_pcm_limiter" in str(e.value) and "error -1" in str(e.value), str(e.value)
    b.set_pcm_stream_limiter(False, 1.0)
    assert [b.pcm_stream_limiter_latency_of(s) for s in range(3)] == [0, 0, 0] and b.pcm_stream_limiter_true_peak(1)
    out, ok = b.exactFrames(clip, [n + 100]*3)
    assert ok.all()
    b.close()


def check_clearing(lib, action, **memory):
    """call A, the action, call B, on a flagged batch and on a twin without any level: the new setter (on again, or off: the stream goes on
    2H late, from a cleared line), the limiter's setter, set_pcm_limiter_lookahead and reset clear the line -- B comes out as the first call
    of a stream does --, set_pcm_level does not: need of the frames whose taps were complete in A was formed with the old gain, need of the
    others is formed in B with the new one, and every frame B writes takes the new one"""
    pkg = package()
    to_memory, to_host = memory.get("to_memory", lambda a: a), memory.get("to_host", lambda a: np.array(a, copy=True))
    H, g, ceil = 8, np.float32(6.0), np.float32(0.25)
    _, planar = dc.session_inputs(fc.F32)
    frames = pc.frames_of(planar)
    b, t = (pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY) for _ in range(2))
    b.set_pcm_limiter_lookahead(H)
    b.set_pcm_level(lc.FIXED, g)
    b.set_pcm_stream_limiter(True, ceil)
    b.set_pcm_stream_limiter_true_peak(True)
    calls = [to_memory(np.ascontiguousarray(frames[:, k*600:(k + 1)*600])) for k in range(2)]
    nout = [[600, 300, 20], [500, 640, 2*H - 3]]
    a_b, a_t = to_host(b.processFrames(calls[0], nout[0])), to_host(t.processFrames(calls[0], nout[0]))
    H2, g2 = H, g
    flags2 = [FLAGGED]*3
    if action == "flag_again":
        b.set_pcm_stream_limiter_true_peak(True)
    elif action == "flag_one":
        b.set_pcm_stream_limiter_true_peak(True, stream=1)                       # (the other streams keep their lines)
    elif action == "flag_off":
        b.set_pcm_stream_limiter_true_peak(False, stream=1)
        flags2[1] = ON
    elif action == "setter":
        b.set_pcm_stream_limiter(True, ceil)
    elif action == "lookahead":
        H2 = 5
        b.set_pcm_limiter_lookahead(H2)
    elif action == "reset":
        b.reset()
        t.reset()
    elif action == "level":
        g2 = np.float32(-3.0)
        b.set_pcm_level(lc.FIXED, g2)
    else:
        raise ValueError(action)
    b_b, b_t = to_host(b.processFrames(calls[1], nout[1])), to_host(t.processFrames(calls[1], nout[1]))
    win, win2, taps = lm.library_window(lib, H), lm.library_window(lib, H2), tp.library_taps(lib)
    D = delay_of(H)
    for s in range(3):
        where = dict(action=action, stream=s)
        va, vb = np.ascontiguousarray(a_t[s, :nout[0][s]].T), np.ascontiguousarray(b_t[s, :nout[1][s]].T)
        na, nb = va.shape[1], vb.shape[1]
        assert same_bits(a_b[s, :na], mirror(va, g, ceil, H, win, taps)[1].T), where
        cleared = action in ("flag_again", "setter", "lookahead", "reset") or (action in ("flag_one", "flag_off") and s == 1)
        if cleared:
            u = mirror_of(flags2[s], vb, g2, ceil, H2, win2, taps)[1]
        else:
            x = np.concatenate([np.zeros((2, D), np.float32), va, vb], axis=1)
            # need of the clip's frames 0 ... 2H + na - 1 was formed in A (from frames that reach 6 further), the rest in B
            need = np.concatenate([lm.need_of(x, abs(g), ceil, True, taps)[:2*H + na], lm.need_of(x, abs(g2), ceil, True, taps)[2*H + na:2*H + na + nb]])
            r = lm.gain_curve(need, H, win)[na:na + nb]
            u = lm.limited(x[:, na:na + nb], g2, r)
            assert (r < 1).any() or s == 2, where                                # (the third stream's few frames stay under the ceiling)
        assert same_bits(b_b[s, :nb], u.T), where
    b.close()
    t.close()


# ---- overshoot: what the flag buys (CPU only; printed, not asserted, as limiter_cases.overshoot's figures are) ---------------------------------

def overshoot(H, flag, n=6*T, seed=9407):
    """the worst true peak of the streaming mirror's float32 output over its ceiling, as a ratio minus 1, for limiter_cases.overshoot's
    signals: white noise, AM tones and sparse spikes driven 12 dB over a ceiling of 0.5"""
    rng = pc._rng(seed, H)
    taps, win = tp.formula_taps(), lm.formula_window(H)
    worst = 0.0
    for s, kind in enumerate(lm.KINDS*2):
        x, g = drive(lm._signal(rng, kind, 2, n, 2*s, H))
        u = (mirror(x, g, 0.5, H, win, taps) if flag else sl.mirror(x, g, 0.5, H, win))[1]
        assert float(lc.peak_of(u)) <= 0.5*(1 + 2.0**-22), (H, kind, float(lc.peak_of(u)))
        worst = max(worst, float(tp.true_peak(u, taps))/0.5 - 1)
    return worst
