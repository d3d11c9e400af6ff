"""Shared cases of the limiter flag of the frame output (include/smst.h, "Limiter"): test_limiter_emu.py runs them on the CPU stand-in,
test_limiter_gpu.py on the device, next to true_peak_cases.py.

The numpy mirror below restates the definition step by step: the detector's bit patterns (with the true-peak flag, true_peak_cases.phases),
one float32 multiply and one float32 division for need, a sliding minimum for hold, the float64 sum over the window accumulated from 0.0 in
the order k = -H ... H, one rounding to float32, the idle rule and the minimum with need.  Every product of two float32 values is exact in
float64 and the additions come in the device's order, so every comparison of need, r and the meters is one of BIT PATTERNS -- there is no
tolerance to choose.  The mirror takes the library's own window (smst_debug_limiter_window), which is compared with the formula on its
own: the host's libm and numpy may differ in the last bit of a double, hence 1 float32 ulp there."""
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
import true_peak_cases as tp
from conftest import package, synth_input

T = 1024                                             # frames one workgroup of either pass takes (kLimitTile, SMST_LIMITER_TILE)
MAX_H, DEFAULT_H = 1024, 72
FIXED, PROTECT, NORMALISE, LOUDNESS = lc.FIXED, lc.PROTECT, lc.NORMALISE, ld.LOUDNESS
TRUE_PEAK, LIMITER = 1, 2                            # the bits of a stream's flags
ONE = 0x3f800000
compared = dict(frames=0)                            # frames of r compared bit for bit with the mirror so far (printed by the tests; EXPERIMENTS.md)


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def formula_window(H):
    """win[k + H] = float32(h_k/sum h), h_k = 0.5*(1 + cos(pi*k/(H + 1))), k = -H ... H"""
    k = np.arange(-H, H + 1, dtype=np.float64)
    h = 0.5*(1 + np.cos(np.pi*k/(H + 1)))
    return (h/h.sum()).astype(np.float32)


def detector(x, true_peak, taps):
    """x [C, N] float32 -> m(n) as float32 [N]: the largest bit pattern over the channels (and, flagged, the three phases), NaN skipped"""
    x = np.asarray(x, np.float32)
    bits = tp._bits(x)
    if true_peak and x.shape[1]:
        with np.errstate(invalid="ignore", over="ignore"):
            y32 = tp.phases(x, taps).astype(np.float32)
        bits = np.concatenate([bits[None], tp._bits(y32)]).max(axis=0)
    return np.ascontiguousarray(bits.max(axis=0) if bits.shape[0] else np.zeros(x.shape[1], np.uint32), np.uint32).view(np.float32)


def need_of(x, g, ceil, true_peak=False, taps=None):
    """need(n), float32 [N]: ceil/w where w = m*g is finite and above ceil, else 1"""
    m = detector(x, true_peak, taps)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = m*np.float32(g)
        assert w.dtype == np.float32
        on = np.isfinite(w) & (w > np.float32(ceil))
        q = np.float32(ceil)/np.where(on, w, np.float32(1))
    assert q.dtype == np.float32
    return np.where(on, q, np.float32(1)).astype(np.float32)


def _sliding_min(a, width):
    return np.lib.stride_tricks.sliding_window_view(a, width).min(axis=1)


def gain_curve(need, H, win):
    """need float32 [N] -> r float32 [N] (steps 4 to 6 of the definition)"""
    need = np.asarray(need, np.float32)
    N = len(need)
    if N == 0:
        return need.copy()
    padded = np.ones(N + 4*H, np.float32)
    padded[2*H:2*H + N] = need
    hold = _sliding_min(padded, 2*H + 1)                 # hold(i), i = -H ... N + H - 1
    assert len(hold) == N + 2*H
    idle = _sliding_min(hold, 2*H + 1) == 1
    h64 = hold.astype(np.float64)
    y = np.zeros(N, np.float64)
    for k in range(2*H + 1):
        y = y + float(win[k])*h64[k:k + N]
    return np.where(idle, np.float32(1), np.minimum(y.astype(np.float32), need)).astype(np.float32)


def mirror(x, g, ceil, H, win, true_peak=False, taps=None):
    """one limited clip x [C, N] -> (need, r, the lowest r, the frames with r < 1)"""
    need = need_of(x, g, ceil, true_peak, taps)
    r = gain_curve(need, H, win)
    return need, r, (r.min() if len(r) else np.float32(1)), int((r < 1).sum())


def limited(x, g, r):
    """u = (v*g)*r: two float32 multiplies"""
    with np.errstate(over="ignore", invalid="ignore"):
        u = lc.levelled(x, g)*np.asarray(r, np.float32)[None, :]
    assert u.dtype == np.float32
    return u


def hexes(v):
    return " ".join("%08x" % b for b in np.ascontiguousarray(v, np.float32).view(np.uint32))


def check_mirror():
    """the known answers of include/smst.h and the properties the definition states"""
    assert hexes(formula_window(1)) == "3e800000 3f000000 3e800000"
    assert hexes(formula_window(2)) == "3daaaaab 3e800000 3eaaaaab 3e800000 3daaaaab"
    w72 = formula_window(72)
    assert hexes(w72[[0, 1, 72]]) == "36d4ca98 37d4b160 3c607038"
    for H in (1, 2, 8, 72, 1024):
        assert abs(formula_window(H).astype(np.float64).sum() - 1) <= 1e-7, H
    x = np.zeros((1, 13), np.float32)
    x[0, 6] = 1
    need, r, low, count = mirror(x, 1.0, 0.5, 2, formula_window(2))
    assert hexes(r) == "3f800000 3f800000 3f755556 3f555556 3f2aaaab 3f0aaaab 3f000000 3f0aaaab 3f2aaaab 3f555556 3f755556 3f800000 3f800000"
    assert low == np.float32(0.5) and count == 9
    x = np.zeros((1, 5), np.float32)
    x[0, 0] = 1
    assert hexes(mirror(x, 1.0, 0.5, 2, formula_window(2))[1]) == "3f000000 3f0aaaab 3f2aaaab 3f555556 3f755556"
    x = np.zeros((1, 12), np.float32)
    x[0, 5:7] = 1
    need, r, _, _ = mirror(x, 1.0, 1.0, 1, formula_window(1), True, tp.formula_taps())
    assert hexes(need[5:6]) == "3f4cbb59" and hexes(r[3:8]) == "3f732ed6 3f598c83 3f4cbb59 3f598c83 3f732ed6"
    assert (np.delete(r, range(3, 8)) == 1).all() and (np.delete(need, 5) == 1).all()
    # r <= need everywhere; r == 1 exactly where idle; a clip under its ceiling gives r identically 1
    rng = pc._rng(9401)
    for H in (1, 2, 8, 72):
        x = _signal(rng, "lone", 2, 3*T, 0, H)
        x[1, 2*T + 100] = -3.0
        need, r, _, _ = mirror(x, 1.5, 0.5, H, formula_window(H))
        active = np.flatnonzero(need < 1)
        far = np.abs(np.arange(3*T)[:, None] - active[None, :]).min(axis=1) > 2*H
        assert (r <= need).all() and (r[far] == 1).all() and (r[~far] < 1).all() and far.any() and len(active), H
        assert (mirror(x, 1.5, 100.0, H, formula_window(H))[1] == 1).all()


# ---- signals ---------------------------------------------------------------------------------------------------------------------------

def _signal(rng, kind, Cn, n, stream, H):
    """[C, n] float32.  spikes: a bed at 1e-3 with spikes within 2H of the clip's two ends and of the tiles' edges; lone: the bed with one
    spike at frame 5 (a long clip keeps idle tiles); am: an amplitude-modulated tone; noise"""
    t = np.arange(n)
    scale = (1 + 0.1*np.arange(Cn))[:, None]
    if kind in ("spikes", "lone"):
        x = rng.uniform(-1, 1, (Cn, n))*1e-3
        spots = [H, n - 1 - H, T - H, T + 1, T + 2*H - 1, 0, n - 1] if kind == "spikes" else [min(5, n - 1)]
        for i, at in enumerate(spots):
            if 0 <= at < n:
                x[(i + stream) % Cn, at] = (2.0 + 0.37*i)*(-1)**i
    elif kind == "am":
        x = (0.5 + 0.5*np.sin(2*np.pi*t/97.0 + stream))[None, :]*np.sin(2*np.pi*0.0731*t[None, :] + 0.4*np.arange(Cn)[:, None])*scale
    else:
        x = rng.uniform(-1, 1, (Cn, n))*scale
    return np.ascontiguousarray(x, np.float32)


KINDS = ("spikes", "am", "noise")


def lengths(H):
    if H == MAX_H:
        return (1, 2049, T + 2*H + 1)
    return tuple(dict.fromkeys((1, 2, H, 2*H, 2*H + 1, 4*H + 1, T - 1, T, T + 1, T + 2*H, 2*T + 3)))


def joins(H):
    """where segment 1 begins in the clip (beyond its length: segment 1 empty)"""
    return (0, 1, 2*H, T - 2*H if T > 2*H else 3, T, 10**9)


# ---- 1. the window and the passes against the mirror ------------------------------------------------------------------------------------

_windows = {}


def library_window(lib, H):
    key = (id(lib), H)
    if key not in _windows:
        _windows[key] = package().debug_limiter_window(H, lib)
    return _windows[key]


def check_window(lib):
    """the library's window against the formula, within 1 float32 ulp, for H = 1, 2, 72, 1024; it sums to 1 within 1e-7"""
    pkg = package()
    for H in (1, 2, DEFAULT_H, MAX_H):
        got, want = library_window(lib, H), formula_window(H)
        assert got.shape == (2*H + 1,) and got.dtype == np.float32
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1 and (got > 0).all(), (H, int(ulps.max()))
        assert abs(got.astype(np.float64).sum() - 1) <= 1e-7, H
    assert (pkg.LIMITER_TILE, pkg.LIMITER_MAX_LOOKAHEAD, pkg.LIMITER_DEFAULT_LOOKAHEAD) == (T, MAX_H, DEFAULT_H)
    for H in (0, MAX_H + 1):
        assert lib.smst_debug_limiter_window(H, np.zeros(4, np.float32).ctypes.data_as(pkg._fp)) == -1


def run_hook(lib, clips, cuts, H, gains, ceilings, flags, base_offset=1, zeros=()):
    """the hook on the clips' image (loudness_cases.build_image) -> (need, r, lowest r, limited frames)"""
    pkg = package()
    offsets = [tp.SRC_OFFSETS[s % len(tp.SRC_OFFSETS)] for s in range(len(clips))]
    image, segs, iss, ics = ld.build_image(clips, cuts, offsets, base_offset)
    for s in zeros:
        segs[s, 0, 3] = 1
    most = max(max(x.shape[1] for x in clips), 1)
    before = [pkg.launch_count(k, lib) for k in ("clip_limit_need", "clip_limit_gain")]
    out = pkg.debug_clip_limit(segs, clips[0].shape[0], image, iss, ics, gains, ceilings, flags, H, most, lib=lib)
    ran = int(any((f & LIMITER) and x.shape[1] and s not in zeros for s, (f, x) in enumerate(zip(flags, clips))))
    assert [pkg.launch_count(k, lib) - n for k, n in zip(("clip_limit_need", "clip_limit_gain"), before)] == [ran, ran]
    return out


def compare_hook(lib, clips, cuts, H, gains, ceilings, flags, zeros=()):
    """need, r and both meters equal the mirror's as bit patterns, for every stream; a stream that is not limited reports 1, 1, 1 and 0"""
    taps, win = tp.library_taps(lib), library_window(lib, H)
    need, r, low, count = run_hook(lib, clips, cuts, H, gains, ceilings, flags, zeros=zeros)
    mirrors = []
    for s, x in enumerate(clips):
        n = x.shape[1]
        where = dict(stream=s, C=x.shape[0], n=n, H=H, cut=cuts[s], flags=flags[s])
        if (flags[s] & LIMITER) and s not in zeros:
            m = mirror(x, gains[s], ceilings[s], H, win, bool(flags[s] & TRUE_PEAK), taps)
        else:
            m = (np.ones(n, np.float32), np.ones(n, np.float32), np.float32(1), 0)
        assert tp.same_bits(need[s, :n], m[0]), (where, np.flatnonzero(need[s, :n].view(np.uint32) != m[0].view(np.uint32))[:8].tolist())
        bad = np.flatnonzero(r[s, :n].view(np.uint32) != m[1].view(np.uint32))
        assert not len(bad), (where, bad[:8].tolist(), hexes(r[s, bad[:4]]), hexes(m[1][bad[:4]]))
        assert (need[s, n:] == 1).all() and (r[s, n:] == 1).all(), where
        assert tp.same_bits(low[s], m[2]) and int(count[s]) == m[3], (where, float(low[s]), float(m[2]), int(count[s]), m[3])
        compared["frames"] += n
        mirrors.append(m)
    return mirrors


def check_hook(lib, channels, H):
    """the two passes through smst_debug_clip_limit against the mirror: every length of lengths(H) with the true-peak flag off and on, the
    three signals in turn, the joins in turn, and every join on the longest clip; rows at offsets that are no multiples of 4 floats"""
    rng = pc._rng(9402, channels, H)
    ns, js = lengths(H), joins(H)
    ceil = np.float32(0.5)
    cases = [(n, js[i % len(js)], KINDS[i % 3], LIMITER | (TRUE_PEAK if (i + f) % 2 else 0)) for f in range(2) for i, n in enumerate(ns)]
    cases += [(ns[-1], j, KINDS[(i + 1) % 3], LIMITER | (TRUE_PEAK if i % 2 else 0)) for i, j in enumerate(js)]
    if H != MAX_H:
        cases.append((3*T - 7, T + 1, "lone", LIMITER))                # (two idle tiles)
    active = idle = 0
    for g0 in range(0, len(cases), 8):
        group = cases[g0:g0 + 8]
        clips = [_signal(rng, kind, channels, n, s, H) for s, (n, _, kind, _) in enumerate(group)]
        gains = [np.float32(1.0 + 0.25*s) for s in range(len(group))]
        mirrors = compare_hook(lib, clips, [j for _, j, _, _ in group], H, gains, [ceil]*len(group), [f for _, _, _, f in group])
        for m in mirrors:
            active += int((m[1] < 1).any())
            idle += int((m[1] == 1).sum() >= T and (m[1] < 1).any())
    assert active >= len(ns) and (idle >= 1 or H == MAX_H), (active, idle)
    print("frames of r bit-identical to the mirror so far: %d" % compared["frames"])


def check_mixed(lib):
    """one call with limited streams, unflagged ones, a zero-length one and one whose segment is a run of zeros (a stream too short for its
    rate): the latter three report need 1, r 1, 1 and 0; a clip under its ceiling is limited to r identically 1"""
    rng = pc._rng(9403)
    H = 8
    clips = [_signal(rng, "noise", 2, T + 40, 0, H), _signal(rng, "noise", 2, T + 40, 1, H), np.zeros((2, 0), np.float32), _signal(rng, "am", 2, 700, 3, H),
             _signal(rng, "lone", 2, 2*T + 3, 4, H), _signal(rng, "noise", 2, 300, 5, H)]
    flags = [LIMITER, TRUE_PEAK, LIMITER, LIMITER | TRUE_PEAK, LIMITER, LIMITER]
    gains = [1.5, 1.5, 1.5, 1.5, 1.5, 0.25]
    m = compare_hook(lib, clips, [T, 5, 0, 333, 10**9, 7], H, gains, [0.5]*6, flags, zeros=(3,))
    assert (m[0][1] < 1).any() and (m[4][1] < 1).any() and (m[5][1] == 1).all() and m[5][3] == 0


def check_nan_inf(lib):
    """a NaN and an inf planted: need is 1 there -- the NaN is skipped, w of the inf is not finite -- and the rest is as the mirror says, with
    the true-peak flag (whose windows spread both over 12 frames) and without"""
    rng = pc._rng(9404)
    H = 8
    clips = [_signal(rng, "noise", 1, T + 50, s, H) for s in range(4)]
    for s in (0, 1):
        clips[s][0, 500] = np.nan
        clips[s][0, T + 2] = np.inf
    clips[2][0, 100], clips[2][0, 107] = np.inf, -np.inf
    clips[3][0, T - 1] = -np.inf
    flags = [LIMITER, LIMITER | TRUE_PEAK, LIMITER | TRUE_PEAK, LIMITER]
    m = compare_hook(lib, clips, [333, T, 5, T + 1], H, [1.5]*4, [0.5]*4, flags)
    for s in range(4):
        assert (m[s][1] < 1).any()
    assert m[0][0][500] == 1 and m[0][0][T + 2] == 1 and m[3][0][T - 1] == 1 and m[0][0][499] < 1
    assert (m[1][0][T - 4:T + 8] == 1).all() and m[1][0][500] == 1               # (the 12 frames whose taps weigh the inf; the NaN's own frame)


def check_reproducible(lib):
    """two runs of the hook give the same bits"""
    rng = pc._rng(9405)
    H = DEFAULT_H
    clips = [_signal(rng, k, 3, n, s, H) for s, (k, n) in enumerate((("noise", 2*T + 3), ("am", T + 7), ("lone", 3*T)))]
    runs = [run_hook(lib, clips, (T - 5, 7, 6), H, [1.5]*3, [0.5]*3, [LIMITER | TRUE_PEAK, LIMITER, LIMITER]) for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (runs[0][1] < 1).any(axis=1).all()


# ---- 2. whole clips through smst_batch_exact_pcm ---------------------------------------------------------------------------------------

CLIPS = tp.CLIPS
#  (mode, gain, flags): PROTECT at +18 dB and LOUDNESS at +6 LUFS -- the ceiling would bite --, limited; NORMALISE with the flag (inert); PROTECT and FIXED without
CLIP_LEVELS = ((PROTECT, 8.0, LIMITER), (LOUDNESS, 1.0, LIMITER | TRUE_PEAK), (NORMALISE, 1.0, LIMITER), (PROTECT, 8.0, 0), (FIXED, 0.5, 0))
CLIP_TARGET, CLIP_FS, CLIP_SEED = tp.CLIP_TARGET, tp.CLIP_FS, 43


def set_clip_levels(batch, ceil, limiter=True, levels=CLIP_LEVELS):
    for s, (mode, gain, flags) in enumerate(levels):
        if mode == LOUDNESS:
            batch.set_pcm_loudness(CLIP_TARGET, ceil, CLIP_FS, stream=s)
        else:
            batch.set_pcm_level(mode, gain, ceil, stream=s)
        batch.set_pcm_true_peak(bool(flags & TRUE_PEAK), stream=s)
        batch.set_pcm_limiter(bool(flags & LIMITER) and limiter, stream=s)
        assert batch.pcm_limiter(s) == (bool(flags & LIMITER) and limiter)


def is_limited(mode, flags):
    return bool(flags & LIMITER) and mode in (PROTECT, LOUDNESS)


LIMIT_COUNTERS = ("clip_limit_need", "clip_limit_gain", "clip_out_limited")


def check_clips(lib, fmt, dithered=None, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """exactFrames of CLIPS with CLIP_LEVELS: the bytes are the mirror applied to smst_batch_exact's planar output of the same batch; the
    gains of the limited streams are g, not min(g, q) -- the LOUDNESS clip reaches its target, which the same clip without the flag does
    not --; take_pcm_limiter is the mirror's; nothing is clamped at the clip-free ceiling; the streams that are not limited have the
    bytes and gains of a twin batch without any limiter flag.  Two calls."""
    pkg = package()
    taps, win = tp.library_taps(lib), library_window(lib, DEFAULT_H)
    nin, nout = CLIPS["inputs"], CLIPS["outputs"]
    S, Cn, most = len(nin), 2, max(nout)
    dithered = fmt in dc.DITHERED_FORMATS if dithered is None else dithered
    frames, planar = tp.clip_frames(fmt)
    p, f, u = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(3))
    ceil = lc.ceiling(fmt, dithered)
    modes = [dc.CLIP_MODES[s] if dithered else dc.NONE for s in range(S)]
    for b in (f, u):
        if dithered:
            for s in range(S):
                b.setPcmDither(modes[s], CLIP_SEED + s, stream=s)
    set_clip_levels(f, ceil)
    set_clip_levels(u, ceil, limiter=False)
    assert f.pcm_limiter_lookahead() == DEFAULT_H
    low0, count0 = f.take_pcm_limiter()
    assert low0.tolist() == [1.0]*S and count0.tolist() == [0]*S               # (nothing has limited yet)
    for call in range(2):
        want, ok_p = p.exact(planar, nout, in_samples=nin)
        want = np.array(want, copy=True)
        plain, _ = u.exactFrames(to_memory(frames), nout, in_samples=nin)
        plain = to_host(plain)
        _, plain_gains = u.take_pcm_peaks()
        assert u.take_pcm_limiter()[1].tolist() == [0]*S
        out = np.full(frames.shape[:1] + (most,) + frames.shape[2:], 0x5A, frames.dtype)
        before = [pkg.launch_count(k, lib) for k in LIMIT_COUNTERS + ("clip_out_levelled",)]
        got, ok_f = f.exactFrames(to_memory(frames), nout, in_samples=nin, out=to_memory(out))
        got = to_host(got)
        assert [pkg.launch_count(k, lib) - n for k, n in zip(LIMIT_COUNTERS + ("clip_out_levelled",), before)] == [1, 1, 1, 0]
        assert ok_p.all() and ok_f.all()
        low, count = f.take_pcm_limiter()
        again = f.take_pcm_limiter()
        assert tp.same_bits(low, again[0]) and np.array_equal(count, again[1])  # (a take resets nothing)
        peaks, gains = f.take_pcm_peaks()
        overs = f.takePcmOvers()[0]
        expect = out.copy()
        for s in range(S):
            where = dict(fmt=fmt, call=call, stream=s)
            x = want[s, :, :nout[s]]
            mode, gain, flags = CLIP_LEVELS[s]
            sample = lc.peak_of(x)
            assert tp.same_bits(peaks[s], sample), where
            peak = tp.true_peak(x, taps) if flags & TRUE_PEAK else sample
            if is_limited(mode, flags):
                if mode == LOUDNESS:
                    m = ld.mirror(x, CLIP_FS, None, CLIP_TARGET)
                    assert m["defined"] and ld.ulps32(gains[s], m["gain"]) <= 1, (where, float(gains[s]), float(m["gain"]))
                    g = gains[s]                                                  # (gL itself: the applied gain reaches the target ...)
                else:
                    g = np.float32(gain)
                    assert tp.same_bits(gains[s], g), (where, float(gains[s]))
                q = lc.gain_of(PROTECT, np.float32(np.inf), ceil, peak)
                assert tp.same_bits(plain_gains[s], q) and float(g) > 1.5*float(q), (where, float(g), float(q), float(plain_gains[s]))   # (... which the clip without the flag misses)
                need, r, lowest, n_limited = mirror(x, g, ceil, DEFAULT_H, win, bool(flags & TRUE_PEAK), taps)
                assert n_limited > 0 and tp.same_bits(low[s], lowest) and int(count[s]) == n_limited, (where, float(low[s]), float(lowest), int(count[s]), n_limited)
                compared["frames"] += len(r)
                codes, cm, _ = dc.mirror(limited(x, g, r), fmt, modes[s], CLIP_SEED + s, 0)
                assert overs[s] == 0 and not cm.any(), (where, int(overs[s]))
                assert not np.array_equal(got[s, :nout[s]], plain[s, :nout[s]]), where
            else:
                g = lc.gain_of(mode, gain, ceil, peak)
                assert tp.same_bits(gains[s], g) and tp.same_bits(gains[s], plain_gains[s]), (where, float(gains[s]), float(g))
                assert low[s] == 1 and count[s] == 0, where
                codes, cm, _ = lc.mirror(x, fmt, g, modes[s], CLIP_SEED + s, 0)
                assert overs[s] == int(cm.sum()), where
                assert np.array_equal(got[s, :nout[s]], plain[s, :nout[s]]), where
            expect[s, :nout[s]] = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
        assert lc.same_bytes(got.reshape(-1).view(np.uint8), expect.reshape(-1).view(np.uint8), fmt), (fmt, call)
    for b in (p, f, u):
        b.close()


def run_clips(lib, fmt=fc.S16):
    """the bytes, the limiter's meters, the peaks and the gains of one limited call on a fresh batch"""
    pkg = package()
    frames, _ = tp.clip_frames(fmt)
    b = pkg.StretchBatch(len(CLIPS["inputs"]), 2, lib=lib, seed=3, **pc.GEOMETRY)
    set_clip_levels(b, lc.ceiling(fmt, False))
    out, ok = b.exactFrames(frames, CLIPS["outputs"], in_samples=CLIPS["inputs"])
    res = [np.array(out, copy=True), ok] + list(b.take_pcm_limiter()) + list(b.take_pcm_peaks())
    b.close()
    return res


def check_two_runs(lib):
    a, b = run_clips(lib), run_clips(lib)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert a[0].any() and (a[3] > 0).sum() == 2


# ---- 3. opt-in, steady state, refusals -------------------------------------------------------------------------------------------------

def check_opt_in(lib, **memory):
    """a levelled batch that never sets the flag: the whole-clip cases of level_cases.py and true_peak_cases.py launch none of the three new
    kernels; a flagged stream in NORMALISE or FIXED launches neither pass and the batch writes the bytes of one without flags; a limited
    clip under its ceiling runs the passes and has the limiter-off bytes"""
    pkg = package()
    to_memory, to_host = memory.get("to_memory", lambda a: a), memory.get("to_host", lambda a: np.array(a, copy=True))
    before = [pkg.launch_count(k, lib) for k in LIMIT_COUNTERS]
    assert min(before) >= 0, "the library has no limiter counters"
    lc.check_clips(lib, fc.S16, **memory)
    tp.check_clips(lib, fc.S16, **memory)
    assert [pkg.launch_count(k, lib) for k in LIMIT_COUNTERS] == before
    nin, nout = CLIPS["inputs"], CLIPS["outputs"]
    frames, _ = tp.clip_frames(fc.S16)
    ceil = lc.ceiling(fc.S16, False)
    inert = ((NORMALISE, 1.0, LIMITER), (FIXED, 0.5, LIMITER | TRUE_PEAK), (NORMALISE, 1.0, LIMITER | TRUE_PEAK), (FIXED, 2.0, LIMITER), (PROTECT, 8.0, 0))
    under = ((PROTECT, 0.01, LIMITER), (PROTECT, 0.02, LIMITER | TRUE_PEAK), (LOUDNESS, 1.0, LIMITER), (PROTECT, 0.5, 0), (FIXED, 0.5, 0))
    counters = LIMIT_COUNTERS + ("clip_out_levelled", "clip_peak", "clip_true_peak", "clip_loudness")
    for levels, ran in ((inert, 0), (under, 1)):
        results = []
        for limiter in (False, True):
            b = pkg.StretchBatch(len(nin), 2, lib=lib, seed=3, **pc.GEOMETRY)
            target = -40.0 if levels is under else CLIP_TARGET
            for s, (mode, gain, flags) in enumerate(levels):
                if mode == LOUDNESS:
                    b.set_pcm_loudness(target, ceil, CLIP_FS, stream=s)
                else:
                    b.set_pcm_level(mode, gain, ceil, stream=s)
                b.set_pcm_true_peak(bool(flags & TRUE_PEAK), stream=s)
                b.set_pcm_limiter(bool(flags & LIMITER) and limiter, stream=s)
            c0 = [pkg.launch_count(k, lib) for k in counters]
            out, ok = b.exactFrames(to_memory(frames), nout, in_samples=nin)
            out = to_host(out)
            results.append((out, b.take_pcm_peaks()[1], [pkg.launch_count(k, lib) - n for k, n in zip(counters, c0)], b.take_pcm_limiter()))
            b.close()
        (out0, g0, n0, _), (out1, g1, n1, (low, count)) = results
        assert np.array_equal(out0, out1) and tp.same_bits(g0, g1) and out0.any(), levels
        assert n0[:4] == [0, 0, 0, 1] and n1[:4] == [ran, ran, ran, 1 - ran] and n0[4:] == n1[4:], (n0, n1)
        assert low.tolist() == [1.0]*5 and count.tolist() == [0]*5


def check_steady_state(lib, to_memory=lambda a: a):
    """the first limited call grows the workspace once, a second call of the same shapes allocates nothing, nor do the takes; setting the
    flag puts the window on the device outside any call"""
    pkg = package()
    nin, nout = CLIPS["inputs"][:3], CLIPS["outputs"][:3]
    clips = to_memory(np.ascontiguousarray(tp.clip_frames(fc.S16)[0][:3]))
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_level(PROTECT, 8.0, 0.9)
    for _ in range(2):
        b.exactFrames(clips, nout, in_samples=nin)
    b.synchronize()
    plain = b.workspaceBytes()
    b.set_pcm_limiter(True)
    b.set_pcm_limiter_lookahead(8)
    assert b.pcm_limiter_lookahead() == 8
    window = b.workspaceBytes()
    assert window == plain + (2*MAX_H + 1)*4, (plain, window)
    b.exactFrames(clips, nout, in_samples=nin)
    b.synchronize()
    events, grown = b.allocation_events(), b.workspaceBytes()
    assert grown >= window + (2*3 + 2*3*max(nout))*4, (window, grown)
    for _ in range(2):
        b.exactFrames(clips, nout, in_samples=nin)
        low, count = b.take_pcm_limiter()
        b.take_pcm_peaks()
    assert b.allocation_events() == events and b.workspaceBytes() == grown and (count > 0).all() and (low < 1).all()
    b.close()


def check_refusals(lib):
    pkg = package()
    b = pkg.StretchBatch(2, 3, lib=lib, **pc.GEOMETRY)
    for stream in (2, -2):
        assert lib.smst_batch_set_pcm_limiter(b.h, stream, 1) == -1 and b"stream" in lib.smst_last_error()
    for stream in (2, -1):
        assert lib.smst_batch_pcm_limiter(b.h, stream, None) == -1 and b"stream" in lib.smst_last_error()
    assert [b.pcm_limiter(s) for s in range(2)] == [False, False]               # (a refused call changes nothing)
    for frames in (0, MAX_H + 1, -5):
        assert lib.smst_batch_set_pcm_limiter_lookahead(b.h, frames) == -1 and b"lookahead" in lib.smst_last_error()
    assert b.pcm_limiter_lookahead() == DEFAULT_H
    assert lib.smst_batch_set_pcm_limiter(None, 0, 1) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_limiter(None, 0, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_set_pcm_limiter_lookahead(None, 8) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_limiter_lookahead(None, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_take_pcm_limiter(None, None, None) == -1 and b"null" in lib.smst_last_error()
    # what is allowed: null pointers in the getters and the take; both ends of the lookahead; the flag beside every mode, untouched by the level setters
    assert lib.smst_batch_pcm_limiter(b.h, 0, None) == 0 and lib.smst_batch_pcm_limiter_lookahead(b.h, None) == 0 and lib.smst_batch_take_pcm_limiter(b.h, None, None) == 0
    for frames in (1, MAX_H):
        b.set_pcm_limiter_lookahead(frames)
        assert b.pcm_limiter_lookahead() == frames
    b.set_pcm_limiter(True, stream=1)
    b.set_pcm_level(PROTECT, 1.0, 0.9)
    b.set_pcm_loudness(-23.0, 1.0, 8000.0, stream=1)
    assert [b.pcm_limiter(s) for s in range(2)] == [False, True] and b.pcm_level(1)[0] == LOUDNESS and not b.pcm_true_peak(1)
    b.set_pcm_limiter(False)
    assert [b.pcm_limiter(s) for s in range(2)] == [False, False] and b.pcm_level(1)[0] == LOUDNESS
    b.close()


def check_refused_in_streaming_calls(lib, **memory):
    """a flagged stream that takes part makes processFrames and flushFrames fail before anything runs, whatever its mode; one that a flush
    leaves out by a negative count does not"""
    pkg = package()
    frames, _ = dc.session_inputs(fc.S16)
    to_memory = memory.get("to_memory", lambda a: a)
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_limiter(True, stream=1)                                            # (the stream is in LEVEL_FIXED)
    x = to_memory(np.ascontiguousarray(frames[:, :600]))
    like = to_memory(np.zeros((1,), np.float32))
    for call in (lambda: b.processFrames(x, [600, 300, 0]), lambda: b.flushFrames([100, 50, -1], like=like)):
        with dc.pytest_raises(pkg.StretchError) as e:
            call()
        assert "limiter" in str(e.value) and "error -1" in str(e.value), str(e.value)
    b.flushFrames([100, -1, 100], like=like)                                     # (stream 1 takes no part: not refused)
    b.set_pcm_limiter(False, stream=1)
    b.processFrames(x, [600, 300, 0])
    b.close()


# ---- 4. the clip-free ceilings and the true peak of the limited output (CPU only: properties of the mirror) ----------------------------------

def ceiling_sweep(fmt, dithered, which, n=1 << 18):
    """level_cases.ceiling_sweep on the limiter's arithmetic: n sampled values w = |v*g| above the tabulated ceiling (which = 0) or the next
    one up (1), each as the loudest frame of its neighbourhood -- r = need = ceiling/w, the largest r the definition allows -> clamped elements"""
    rng = pc._rng(9406, fmt, dithered)
    c = lc.ceiling(fmt, dithered, which)
    w = (np.float64(c)*2.0**rng.uniform(0, 12, n)).astype(np.float32)
    w[::4] = (np.float64(c)*(1 + rng.uniform(0, 1e-5, len(w[::4])))).astype(np.float32)
    w = w[w > c]
    w[::2] *= np.float32(-1)
    need = (c/np.abs(w)).astype(np.float32)
    u = w*need
    clamped = 0
    for mode in ((dc.TPDF, dc.HP) if dithered else (dc.NONE,)):
        clamped += int(dc.mirror(u.reshape(1, -1), fmt, mode, 11, 0)[1].sum())
    return clamped


def check_ceiling_table():
    """per format and dither mode: nothing clamps at level_cases.CEILINGS' ceiling -- the limiter's table is today's --, something does one up"""
    for (fmt, dithered) in lc.CEILINGS:
        assert ceiling_sweep(fmt, dithered, 0) == 0, (fmt, dithered)
        assert ceiling_sweep(fmt, dithered, 1) > 0, (fmt, dithered)


def overshoot(H, n=6*T, seed=9407):
    """the worst true peak of the limiter mirror's float32 output over its ceiling, as a ratio minus 1: white noise, AM tones and sparse
    spikes driven 12 dB over a ceiling of 0.5, true-peak flag on"""
    rng = pc._rng(seed, H)
    taps, win = tp.formula_taps(), formula_window(H)
    worst = 0.0
    for s, kind in enumerate(KINDS*2):
        x = _signal(rng, kind, 2, n, 2*s, H)
        x *= np.float32(1.0/float(lc.peak_of(x)))
        g, ceil = np.float32(0.5*10**(12/20)), np.float32(0.5)
        _, r, _, _ = mirror(x, g, ceil, H, win, True, taps)
        u = limited(x, g, r)
        # the SAMPLE peak is bounded: fl(w*fl(ceil/w)) carries two roundings of 2^-24 relative each, and r <= need
        assert float(lc.peak_of(u)) <= float(ceil)*(1 + 2.0**-22), (H, kind, float(lc.peak_of(u)))
        worst = max(worst, float(tp.true_peak(u, taps))/float(ceil) - 1)
    return worst


# ---- 5. the command-line tool ----------------------------------------------------------------------------------------------------------

def limit_lines(stdout):
    """the "level:" lines of a --limit run -> [(file, lufs or None, peak, gain, overs, limit dB, limited frames)]"""
    found = re.findall(r"^level: (\S+) (?:loudness=(\S+) )?peak=(\S+) gain=(\S+) overs=(-?\d+)(?: true-peak=\S+)? limit=(\S+) limited=(\d+)$", stdout, re.M)
    return [(name, float(lufs) if lufs else None, np.float32(peak), np.float32(gain), int(overs), float(db), int(count)) for name, lufs, peak, gain, overs, db, count in found]


def check_cli(cli, tmp_path, lib):
    """--protect with --gain and --limit, --loudness with --protect and --limit: the printed gain is the unclamped one, the printed meters are
    the mirror's of the --exact floats at the lookahead the tool derives from the file rate, and the file's bytes are the mirror's; --limit
    is refused with --normalize and without a ceiling's mode; without it the lines are the ones of today"""
    from test_cli import write_wav16
    sr, lens = 8000, (3100, 4400)                                                  # (at 1.1x both clips hold a 400-ms block)
    H = int(round(1.5e-3*sr))
    win = library_window(lib, H)
    srcs = [str(tmp_path/("in%d.wav" % k)) for k in range(2)]
    write_wav16(srcs[0], 0.5*synth_input(1, 2, lens[0], sr) + 0.4*tp.crest_tone(lens[0], 0), sr)
    write_wav16(srcs[1], 0.1*synth_input(2, 2, lens[1], sr) + 0.25*tp.crest_tone(lens[1], 1), sr)

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
    ceil = np.float32(10**(-6/20))

    def verify(lines, outs, gains):
        for k, (path, _, peak, gain, overs, db, count) in enumerate(lines):
            assert path == outs[k] and peak == lc.peak_of(floats[k]) and overs == 0 and tp.same_bits(gain, gains[k]), (k, lines[k], float(gains[k]))
            assert float(gain)*float(peak) > float(ceil), (k, lines[k])                                   # (the ceiling would have lowered this gain)
            need, r, low, n = mirror(floats[k], gain, ceil, H, win)
            assert n > 0 and count == n and abs(db - 20*math.log10(float(low))) <= 5.1e-5, (k, lines[k], float(low), n)
            head, data = dc.data_chunk(path)
            assert head == (1, 2, sr, sr*4, 4, 16)
            codes, cm, _ = dc.mirror(limited(floats[k], gain, r), fc.S16, dc.NONE, k, 0)
            assert np.array_equal(np.frombuffer(data, "<i2"), codes.reshape(-1)) and not cm.any(), k
            assert np.abs(codes.astype(np.int64)).max() <= int(round(float(ceil)*32768)), k
    outs, res = run("prot", ["--gain=12", "--protect=-6", "--limit", "--out-format=s16"])
    lines = limit_lines(res.stdout)
    assert len(lines) == 2 and not lc.level_lines(res.stdout), res.stdout
    verify(lines, outs, [np.float32(10**(12/20))]*2)
    outs, res = run("loud", ["--loudness=-3", "--protect=-6", "--limit", "--out-format=s16"])
    lines = limit_lines(res.stdout)
    assert len(lines) == 2 and all(l[1] is not None for l in lines), res.stdout
    gains = []
    for k, l in enumerate(lines):
        m = ld.mirror(floats[k], float(sr), None, -3.0)
        assert m["defined"] and abs(l[1] - m["lufs"]) <= 1e-3 and ld.ulps32(l[3], m["gain"]) <= 1, (k, l, m["lufs"], float(m["gain"]))
        gains.append(l[3])
    verify(lines, outs, gains)
    plain = ld.loudness_lines(run("plain", ["--loudness=-3", "--protect=-6", "--out-format=s16"])[1].stdout)
    assert len(plain) == 2 and all(a[3] < b[3] for a, b in zip(plain, lines)), (plain, lines)                 # (without --limit the files miss -3 LUFS)
    _, res = run("look", ["--gain=12", "--protect=-6", "--limit", "--limit-lookahead=0.25"])
    assert [l[6] for l in limit_lines(res.stdout)] == [mirror(f, np.float32(10**(12/20)), ceil, 2, library_window(lib, 2))[3] for f in floats]
    for flags, word in ((["--limit"], "--protect"), (["--limit", "--normalize=-1"], "--normalize"), (["--limit", "--gain=3"], "--protect")):
        _, res = run("bad", flags, expect=2)
        assert word in res.stderr, (flags, res.stderr)
    _, res = run("far", ["--protect=-6", "--limit", "--limit-lookahead=500"], expect=1)
    assert "lookahead" in res.stderr
