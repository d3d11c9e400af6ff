"""Shared cases of the stream limiter of the frame output (include/smst.h, "Stream limiter"): test_stream_limiter_emu.py runs them on the
CPU stand-in, test_stream_limiter_gpu.py on the device, next to limiter_cases.py.

The definition is the clip limiter's, applied to the clip [2H frames of +0.0, every frame emitted so far]: the mirror below is three lines
over limiter_cases' need_of, gain_curve and limited.  As there, every comparison of r, frames and meters is one of BIT PATTERNS -- no
tolerance appears anywhere; a NaN of the float32 output equals any other NaN (the multiplies may touch its payload)."""
import numpy as np

import dither_cases as dc
import level_cases as lc
import limiter_cases as lm
import pcm_cases as pc
import pcm_format_cases as fc
from conftest import package

T = lm.T
ON = 1
COUNTERS = ("pcm_limit_feed", "pcm_limit_gain", "pcm_out_limited")
OLD_COUNTERS = ("pcm_out_levelled", "pcm_out", "pcm_out_dithered")
compared = dict(frames=0)                            # frames of r compared bit for bit with the mirror so far (printed by the tests; EXPERIMENTS.md)


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def mirror(v, g, ceil, H, win):
    """v [C, T] float32, the frames emitted so far -> (r [T], u [C, T]): the first T frames of the limited clip [2H zeros, v]"""
    x = np.concatenate([np.zeros((v.shape[0], 2*H), np.float32), np.asarray(v, np.float32)], axis=1)
    r = lm.gain_curve(lm.need_of(x, abs(np.float32(g)), ceil), H, win)[:v.shape[1]]
    return r, lm.limited(x[:, :v.shape[1]], g, r)


def meters_of(r):
    return (np.float32(r.min()) if len(r) else np.float32(1)), int((r < 1).sum())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def check_mirror():
    """the two known answers of include/smst.h"""
    win = lm.formula_window(2)
    v = np.zeros((1, 17), np.float32)
    v[0, 6] = 1
    r, u = mirror(v, 1.0, 0.5, 2, win)
    curve = "3f755556 3f555556 3f2aaaab 3f0aaaab 3f000000 3f0aaaab 3f2aaaab 3f555556 3f755556"
    assert lm.hexes(r) == " ".join(["3f800000"]*6 + [curve] + ["3f800000"]*2)
    assert lm.hexes(u[0]) == " ".join(["00000000"]*10 + ["3f000000"] + ["00000000"]*6)
    assert lm.hexes(meters_of(r)[0]) == "3f000000" and meters_of(r)[1] == 9
    v = np.zeros((1, 9), np.float32)
    v[0, 0] = 1
    r, u = mirror(v, -1.0, 0.5, 2, win)
    assert lm.hexes(r) == curve and lm.hexes(u[0]) == " ".join(["80000000"]*4 + ["bf000000"] + ["80000000"]*4) and meters_of(r)[1] == 9


# ---- the hook ------------------------------------------------------------------------------------------------------------------------

def run_hook(lib, clips, cuts, H, gains, ceilings, flags):
    """clips: per stream [C, n] float32, every frame of the stream in order; cuts: per stream the counts of its calls (as many for every
    stream) -> (r [S, most], frames [S, most, C], min gain [S], limited frames [S]); the three counters move by one per call in which a
    stream with the setting has frames"""
    pkg = package()
    S, Cn = len(clips), clips[0].shape[0]
    most = max(max(x.shape[1] for x in clips), 1)
    image = np.zeros((S, Cn, most), np.float32)
    for s, x in enumerate(clips):
        assert sum(max(c, 0) for c in cuts[s]) == x.shape[1] and len(cuts[s]) == len(cuts[0])
        image[s, :, :x.shape[1]] = x
    counts = np.ascontiguousarray(np.asarray(cuts, np.int32).T)
    ran = sum(int(any(flags[s] & ON and counts[k, s] > 0 for s in range(S))) for k in range(counts.shape[0]))
    before = [pkg.launch_count(k, lib) for k in COUNTERS]
    out = pkg.debug_pcm_stream_limit(counts, Cn, image, Cn*most, most, gains, ceilings, flags, H, most, lib=lib)
    assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS, before)] == [ran]*3
    return out


def compare_hook(lib, clips, cuts, H, gains, ceilings, flags):
    """r, the float32 frames and both meters equal the mirror's as bit patterns, for every stream; a stream without the setting is not
    delayed, has the levelled form's frames and reports r 1, 1 and 0"""
    win = lm.library_window(lib, H)
    r, frames, low, count = run_hook(lib, clips, cuts, H, gains, ceilings, flags)
    mirrors = []
    for s, x in enumerate(clips):
        n = x.shape[1]
        where = dict(stream=s, C=x.shape[0], n=n, H=H, cuts=list(cuts[s]), flags=flags[s], gain=float(gains[s]), ceiling=float(ceilings[s]))
        if flags[s] & ON:
            mr, mu = mirror(x, gains[s], ceilings[s], H, win)
        else:
            mr, mu = np.ones(n, np.float32), lc.levelled(x, gains[s])
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
    """0, a stream that takes no part, 1, the counts around the frame line (2H) and the need line (4H), around a tile and beyond two"""
    return [0, -1, 1, 2*H - 1, 2*H, 2*H + 1, 4*H, 4*H + 1, T - 1, T, T + 1, 2*T + 3]


def drive(x, over_db=12.0, ceil=0.5):
    """the signal at peak 1 and the gain that drives it over_db over the ceiling"""
    x = x*np.float32(1.0/float(lc.peak_of(x)))
    return np.ascontiguousarray(x, np.float32), np.float32(ceil*10**(over_db/20))


SETTINGS = ("on", "off", "negative", "inf")


def check_hook(lib, channels, H, variants=(0, 1)):
    """four streams in one sequence of calls, each with the counts of cut_counts(H) in an order of its own and one of limiter_cases' signals
    driven 12 dB over a ceiling of 0.5; one stream with the setting off, one with a negative gain, one with a ceiling of +inf (r is 1
    throughout, the output only late).  The settings move round the streams from one variant to the next, so that every signal is limited"""
    counts = cut_counts(H)
    n = sum(max(c, 0) for c in counts)
    for variant in variants:
        rng = pc._rng(9501, channels, H, variant)
        clips, cuts, gains, ceilings, flags = [], [], [], [], []
        for s in range(4):
            x, g = drive(lm._signal(rng, lm.KINDS[s % 3], channels, n, s, H))
            setting = SETTINGS[(s + variant) % 4]
            clips.append(x)
            cuts.append(counts[3*s:] + counts[:3*s])
            gains.append(-g if setting == "negative" else g)
            ceilings.append(np.float32(np.inf) if setting == "inf" else np.float32(0.5))
            flags.append(0 if setting == "off" else ON)
        mirrors = compare_hook(lib, clips, cuts, H, gains, ceilings, flags)
        for s, (mr, mu) in enumerate(mirrors):
            setting = SETTINGS[(s + variant) % 4]
            assert (mr < 1).any() == (setting in ("on", "negative")), (s, setting)
            if setting == "inf":                                                 # (a delay only)
                assert same_bits(mu[:, 2*H:], lc.levelled(clips[s][:, :n - 2*H], gains[s])) and not mu[:, :2*H].any()
            if setting in ("on", "negative"):
                assert float(lc.peak_of(mu)) <= 0.5*(1 + 2.0**-22), (s, float(lc.peak_of(mu)))
    print("frames of r bit-identical to the mirror so far: %d" % compared["frames"])


def check_known_answers(lib):
    """the two known answers through the hook, cut as include/smst.h cuts them"""
    v = np.zeros((1, 17), np.float32)
    v[0, 6] = 1
    r, frames, low, count = run_hook(lib, [v], [[5, 1, 7, 4]], 2, [1.0], [0.5], [ON])
    assert lm.hexes(r[0, 6:15]) == "3f755556 3f555556 3f2aaaab 3f0aaaab 3f000000 3f0aaaab 3f2aaaab 3f555556 3f755556" and (np.delete(r[0], range(6, 15)) == 1).all()
    assert lm.hexes(frames[0, 10]) == "3f000000" and not np.delete(frames[0, :, 0], 10).view(np.uint32).any()
    assert lm.hexes(low) == "3f000000" and count.tolist() == [9]
    v = np.zeros((1, 9), np.float32)
    v[0, 0] = 1
    r, frames, low, count = run_hook(lib, [v], [[3, 6]], 2, [-1.0], [0.5], [ON])
    assert lm.hexes(r[0]) == "3f755556 3f555556 3f2aaaab 3f0aaaab 3f000000 3f0aaaab 3f2aaaab 3f555556 3f755556"
    assert lm.hexes(frames[0, :, 0]) == " ".join(["80000000"]*4 + ["bf000000"] + ["80000000"]*4) and count.tolist() == [9]


def check_cut_invariance(lib, H=lm.DEFAULT_H, channels=2, n=2*T + 300):
    """one stream as one call, as 128-frame quanta and as drawn cuts: r, the frames and the meters are identical (and the mirror's)"""
    rng = pc._rng(9502)
    x, g = drive(lm._signal(rng, "noise", channels, n, 0, H))
    quanta = [128]*(n//128) + [n % 128]
    drawn = [3, 0]                                                               # (a call without frames among them)
    while sum(drawn) < n:
        drawn.append(min(int(rng.integers(0, 4*H + 40)), n - sum(drawn)))
    results = []
    for cuts in ([n], quanta, drawn):
        compare_hook(lib, [x], [cuts], H, [g], [np.float32(0.5)], [ON])
        results.append(run_hook(lib, [x], [cuts], H, [g], [np.float32(0.5)], [ON]))
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (results[0][0] < 1).any() and len(drawn) > 8 and 0 in drawn


def check_nan_inf(lib):
    """limiter_cases.check_nan_inf's contract on the carried form: a NaN is skipped by the detector and an inf gives need 1 -- r around
    them is what the other frames ask for --, the NaN stays a NaN in the float32 output and the inf an inf (the conversion's own rule then
    codes the one as 0 and clamps the other, and counts both); planted around the cuts, where the line carries them"""
    rng = pc._rng(9503)
    H = 8
    cuts = [[300, 1, 2*H, 4*H + 1, T + 50 - 300 - 1 - 2*H - 4*H - 1]]*3
    clips, gains = [], []
    for s in range(3):
        x, g = drive(lm._signal(rng, "noise", 2, T + 50, s, H))
        clips.append(x)
        gains.append(g if s != 1 else -g)
    clips[0][0, 299], clips[0][1, 300] = np.nan, np.inf                          # (the last frame of a call, the only frame of the next one)
    clips[1][0, 301 + 2*H - 1], clips[1][1, 10] = -np.inf, np.nan
    clips[2][:, 500] = np.nan                                                    # (every channel: m = 0, need 1)
    clips[2][0, 0] = np.inf
    m = compare_hook(lib, clips, cuts, H, gains, [np.float32(0.5)]*3, [ON]*3)
    win = lm.library_window(lib, H)
    for s, spots in ((0, (300,)), (1, (301 + 2*H - 1,)), (2, (500, 0))):
        x = np.concatenate([np.zeros((2, 2*H), np.float32), clips[s]], axis=1)
        need = lm.need_of(x, abs(gains[s]), 0.5)
        for at in spots:
            assert need[2*H + at] == 1, (s, at)
        assert (m[s][0] < 1).any() and (lm.gain_curve(need, H, win)[:T + 50].view(np.uint32) == m[s][0].view(np.uint32)).all()
    u = m[0][1]
    assert np.isnan(u[0, 2*H + 299]) and np.isinf(u[1, 2*H + 300]) and np.isfinite(u[1, 2*H + 299])


def check_reproducible(lib):
    rng = pc._rng(9504)
    H = lm.DEFAULT_H
    clips = [drive(lm._signal(rng, k, 3, 2*T + 3, s, H))[0] for s, k in enumerate(lm.KINDS)]
    cuts = [[T + 1, 0, T + 2], [128, 2*T - 125, 0], [1, 1, 2*T + 1]]
    runs = [run_hook(lib, clips, cuts, H, [2.0, -2.0, 2.0], [0.5]*3, [ON]*3) for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (runs[0][0] < 1).any(axis=1).all()


# ---- end to end: processFrames and flushFrames ----------------------------------------------------------------------------------------------

GAINS = (8.0, 0.5, -4.0)                                                         # per stream; the setting is off on the second
LIMITED = (True, False, True)


def session_of(H):
    """dither_cases.SESSION with its flush asked for 2H frames more"""
    return dict(dc.SESSION, flush=[n + 2*H if n >= 0 else n for n in dc.SESSION["flush"]])


def set_session(batch, ceil, H=None):
    if H is not None:
        batch.set_pcm_limiter_lookahead(H)
    for s, g in enumerate(GAINS):
        batch.set_pcm_level(lc.FIXED, g, stream=s)
        batch.set_pcm_stream_limiter(LIMITED[s], ceil, stream=s)


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


def run_session(lib, fmt, dithered, H=lm.DEFAULT_H, **memory):
    """the limited session on a fresh batch -> (the calls' frames, the batch)"""
    b = package().StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    set_session(b, lc.ceiling(fmt, dithered), H if H != lm.DEFAULT_H else None)
    if dithered:
        dc.set_session_dither(b)
    return dc.frame_session(b, dc.session_inputs(fmt)[0], fmt, session_of(H), **memory), b


def check_session(lib, fmt, dithered, H=lm.DEFAULT_H, **memory):
    """processFrames twice and flushFrames, asked for 2H frames more, with the gains 8, 0.5 and -4 and the setting off on the second stream:
    the bytes are the format's rule and the dither of the running counter on the mirror's u of the twin's float32 frames; the peaks are those
    of the frames written; the overs are the mirror's (none on a limited stream at the clip-free ceiling); the limiter's meters accumulate
    over the three calls and a second take gives 1 and 0.  The flush of count + 2H delivers the whole tail: the limited total is the twin's,
    frame for frame, 2H frames late"""
    pkg = package()
    session, win = session_of(H), lm.library_window(lib, H)
    ceil = lc.ceiling(fmt, dithered)
    twin = twin_session(lib, fmt, H)
    counts = dc.session_counts(session)
    before = [pkg.launch_count(k, lib) for k in COUNTERS + OLD_COUNTERS]
    got, b = run_session(lib, fmt, dithered, H, **memory)
    assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS + OLD_COUNTERS, before)] == [3, 3, 3, 0, 0, 0]
    assert b.pcm_stream_limiter_latency() == 2*H and [b.pcm_stream_limiter(s)[0] for s in range(3)] == list(LIMITED)
    modes = dc.SESSION_MODES if dithered else (dc.NONE,)*3
    clamped = np.zeros(3, np.int64)
    low, count = b.take_pcm_stream_limiter()
    peaks, gains = b.take_pcm_peaks()
    for s in range(3):
        where = dict(fmt=fmt, dithered=dithered, stream=s)
        v = np.concatenate([np.ascontiguousarray(t[s, :n[s]].T) for t, n in zip(twin, counts)], axis=1)     # [C, total]
        total = v.shape[1]
        if LIMITED[s]:
            r, u = mirror(v, GAINS[s], ceil, H, win)
            written = np.concatenate([np.zeros((2, 2*H), np.float32), v], axis=1)[:, :total]
            ml, mc = meters_of(r)
            assert mc > 0 and same_bits(low[s], ml) and int(count[s]) == mc, (where, float(low[s]), float(ml), int(count[s]), mc)
            assert same_bits(u[:, 2*H:], lm.limited(v[:, :total - 2*H], GAINS[s], r[2*H:])), where   # (the twin's frames, 2H late)
            compared["frames"] += total
        else:
            u, written = lc.levelled(v, GAINS[s]), v
            assert low[s] == 1 and count[s] == 0, where
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
        if LIMITED[s]:
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


# ---- opt-in, steady state, refusals, clearing ------------------------------------------------------------------------------------------------

def check_opt_in(lib, **memory):
    """a batch that never calls the setter: level_cases' and dither_cases' sessions give the bytes their own mirrors ask for and move none
    of the three new counters; with the setting on, a call in which no limited stream has frames launches the levelled kernel as before"""
    pkg = package()
    before = [pkg.launch_count(k, lib) for k in COUNTERS + OLD_COUNTERS]
    assert min(before) >= 0, "the library has no stream limiter counters"
    lc.check_session(lib, fc.S16, True, **memory)
    dc.check_session(lib, fc.S16, **memory)
    pc.check_session(lib, 2, pc.F32, **memory)
    moved = [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS + OLD_COUNTERS, before)]
    assert moved[:3] == [0, 0, 0] and min(moved[3:]) > 0, moved
    to_memory, to_host = memory.get("to_memory", lambda a: a), memory.get("to_host", lambda a: np.array(a, copy=True))
    frames, _ = dc.session_inputs(fc.S16)
    plain, b = (pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY) for _ in range(2))
    for batch in (plain, b):
        lc.set_session_levels(batch)
    b.set_pcm_stream_limiter(True, 0.9, stream=0)
    for batch in (plain, b):
        batch.processFrames(to_memory(np.ascontiguousarray(frames[:, :640])), [640]*3)  # (past the engine's leading zeros)
    x = to_memory(np.ascontiguousarray(frames[:, 640:1240]))
    before = [pkg.launch_count(k, lib) for k in COUNTERS + OLD_COUNTERS]
    got = to_host(b.processFrames(x, [0, 300, 200], in_samples=[600, 300, 200]))
    assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS + OLD_COUNTERS, before)] == [0, 0, 0, 1, 0, 0]
    want = to_host(plain.processFrames(x, [0, 300, 200], in_samples=[600, 300, 200]))
    assert np.array_equal(got[1, :300], want[1, :300]) and np.array_equal(got[2, :200], want[2, :200]) and got[1, :300].any()
    plain.close()
    b.close()


def check_steady_state(lib, to_memory=lambda a: a):
    """the setter allocates the lines (and the window) outside any call; the first limited call grows the rows once; a second call of the
    same shapes leaves allocation_events and workspaceBytes where they are, as do the takes"""
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
    plain = b.workspaceBytes()
    b.set_pcm_stream_limiter(True, 0.5)
    lines = b.workspaceBytes()
    assert lines == plain + (2*lm.MAX_H + 1)*4 + (2*(S*4*H + S*Cn*2*H) + 2*S)*4, (plain, lines)
    b.set_pcm_stream_limiter(True, 0.25, stream=1)
    assert b.workspaceBytes() == lines
    b.processFrames(x, [600, 300, 128])
    b.synchronize()
    events, grown = b.allocation_events(), b.workspaceBytes()
    assert grown >= lines + S*(4*H + 2*600)*4, (lines, grown)
    for _ in range(3):
        b.processFrames(x, [600, 300, 128])
        low, count = b.take_pcm_stream_limiter()
        b.take_pcm_peaks()
    b.flushFrames([100, 100, 100], like=to_memory(np.zeros((1,), np.float32)))
    assert b.allocation_events() == events and b.workspaceBytes() == grown and (count > 0).all() and (low < 1).all()
    b.close()


def check_refusals(lib, **memory):
    pkg = package()
    to_memory = memory.get("to_memory", lambda a: a)
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    state = lambda: ([b.pcm_stream_limiter(s) for s in range(3)], b.workspaceBytes(), b.allocation_events())
    start = state()
    assert start[0] == [(False, 1.0)]*3
    for stream in (3, -2):
        assert lib.smst_batch_set_pcm_stream_limiter(b.h, stream, 1, 1.0) == -1 and b"stream" in lib.smst_last_error()
    for stream in (3, -1):
        assert lib.smst_batch_pcm_stream_limiter(b.h, stream, None, None) == -1 and b"stream" in lib.smst_last_error()
    for ceil in (float("nan"), 0.0, -1.0, float("-inf")):
        assert lib.smst_batch_set_pcm_stream_limiter(b.h, 0, 1, ceil) == -1 and b"ceiling" in lib.smst_last_error()
    assert state() == start                                                      # (a refused call changes nothing)
    assert lib.smst_batch_set_pcm_stream_limiter(None, 0, 1, 1.0) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_stream_limiter(None, 0, None, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_stream_limiter_latency(None, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_take_pcm_stream_limiter(None, None, None) == -1 and b"null" in lib.smst_last_error()
    # what is allowed: null pointers in the getters and the take, a ceiling of +inf, the setting beside the level setters
    assert lib.smst_batch_pcm_stream_limiter(b.h, 0, None, None) == 0 and lib.smst_batch_pcm_stream_limiter_latency(b.h, None) == 0
    assert lib.smst_batch_take_pcm_stream_limiter(b.h, None, None) == 0
    assert b.pcm_stream_limiter_latency() == 2*lm.DEFAULT_H
    b.set_pcm_stream_limiter(True, float("inf"), stream=1)
    b.set_pcm_level(lc.FIXED, 2.0, 0.75, stream=1)
    assert [b.pcm_stream_limiter(s) for s in range(3)] == [(False, 1.0), (True, float("inf")), (False, 1.0)]
    assert b.pcm_level(1) == (lc.FIXED, 2.0, 0.75) and not b.pcm_limiter(1)      # (the level's own ceiling; the clip limiter's flag is another setting)
    b.set_pcm_limiter_lookahead(5)
    assert b.pcm_stream_limiter_latency() == 10
    # a whole-clip mode is still refused in the streaming calls, with the setting on as well
    frames, _ = dc.session_inputs(fc.S16)
    x = to_memory(np.ascontiguousarray(frames[:, :600]))
    like = to_memory(np.zeros((1,), np.float32))
    b.set_pcm_level(lc.PROTECT, 1.0, 0.9, stream=1)
    for call in (lambda: b.processFrames(x, [600, 300, 0]), lambda: b.flushFrames([100, 50, -1], like=like)):
        with dc.pytest_raises(pkg.StretchError) as e:
            call()
        assert "whole-clip" in str(e.value) and "error -1" in str(e.value), str(e.value)
    # exactFrames refuses a participating limited stream and names the whole-clip form; it accepts one that a negative count leaves out
    b.set_pcm_level(lc.FIXED, 2.0, stream=1)
    clip, n = to_memory(np.ascontiguousarray(frames)), frames.shape[1]
    with dc.pytest_raises(pkg.StretchError) as e:
        b.exactFrames(clip, [n + 100]*3)
    assert "smst_batch_set_pcm_limiter" in str(e.value) and "error -1" in str(e.value), str(e.value)
    out, ok = b.exactFrames(clip, [n + 100, -1, n + 100])
    assert ok.tolist() == [True, False, True]
    b.set_pcm_stream_limiter(False, 1.0)
    out, ok = b.exactFrames(clip, [n + 100]*3)
    assert ok.all()
    b.close()


def check_clearing(lib, action, **memory):
    """call A, the action, call B, on a limited batch (mono stream 0 of two, float32 frames) and on a twin without any level: the setter for
    the stream, set_pcm_limiter_lookahead and reset clear the line -- B comes out as the first call of a stream does --, set_pcm_level does
    not: need of A's frames was formed with the old gain, need of B's is formed with the new one, and every frame B writes takes the new one"""
    pkg = package()
    to_memory, to_host = memory.get("to_memory", lambda a: a), memory.get("to_host", lambda a: np.array(a, copy=True))
    H, g, ceil = 8, np.float32(6.0), np.float32(0.25)
    _, planar = dc.session_inputs(fc.F32)
    frames = pc.frames_of(planar)
    b, t = (pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY) for _ in range(2))
    b.set_pcm_limiter_lookahead(H)
    b.set_pcm_level(lc.FIXED, g)
    b.set_pcm_stream_limiter(True, ceil)
    calls = [to_memory(np.ascontiguousarray(frames[:, k*600:(k + 1)*600])) for k in range(2)]
    nout = [[600, 300, 20], [500, 640, 2*H - 3]]
    a_b, a_t = to_host(b.processFrames(calls[0], nout[0])), to_host(t.processFrames(calls[0], nout[0]))
    H2, g2 = H, g
    if action == "setter":
        b.set_pcm_stream_limiter(True, ceil)
    elif action == "setter_one":
        b.set_pcm_stream_limiter(True, ceil, stream=1)                           # (the other streams keep their lines)
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
    win, win2 = lm.library_window(lib, H), lm.library_window(lib, H2)
    for s in range(3):
        where = dict(action=action, stream=s)
        va, vb = np.ascontiguousarray(a_t[s, :nout[0][s]].T), np.ascontiguousarray(b_t[s, :nout[1][s]].T)
        assert same_bits(a_b[s, :nout[0][s]], mirror(va, g, ceil, H, win)[1].T), where
        cleared = action in ("setter", "lookahead", "reset") or (action == "setter_one" and s == 1)
        if cleared:
            u = mirror(vb, g2, ceil, H2, win2)[1]
        else:
            x = np.concatenate([np.zeros((2, 2*H), np.float32), va, vb], axis=1)
            need = np.concatenate([lm.need_of(x[:, :2*H + va.shape[1]], abs(g), ceil), lm.need_of(vb, abs(g2), ceil)])
            r = lm.gain_curve(need, H, win)[va.shape[1]:va.shape[1] + vb.shape[1]]
            u = lm.limited(x[:, va.shape[1]:va.shape[1] + vb.shape[1]], g2, r)
            assert (r < 1).any() or s == 2, where                                # (the third stream's few frames stay under the ceiling)
        assert same_bits(b_b[s, :nout[1][s]], u.T), where
    b.close()
    t.close()
