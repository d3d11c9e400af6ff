"""Shared cases of the loudness-range meter of the frame output (include/smst.h, "Loudness range"): test_loudness_range_emu.py runs them on
the CPU stand-in, test_loudness_range_gpu.py on the device, next to loudness_cases.py, whose mirror pieces they reuse.

The mirror below restates the definition in float64: the K-weighted channels (loudness_cases.k_weight), the 100-ms sub-block sums, the
block powers, the 3-s short-term powers with their 30 sums added from 0.0 in ascending order, the two gates with the mean's sum in block
order, and the nearest-rank selection.  The device sums the filter's output in another order, so a power is compared relatively, within
loudness_cases.TOL = 1e-9; an order statistic moves by at most as much as its inputs, so the same bound holds for lo and hi once the counts
agree, and the counts are exact: every case builder keeps every short-term power and every block power GATE_CLEARANCE away from its gates.
The selection itself is checked bit for bit (check_selection): from the powers the device returned, a host that gates in block order,
sorts and takes the nearest ranks must get the device's lo, hi, n and maxima exactly.  Gains are within 1 fp32 ulp."""
import hashlib
import math
import re
import subprocess

import numpy as np

import dither_cases as dc
import exact_cases as xc
import level_cases as lc
import limiter_cases as lm
import loudness_cases as ld
import pcm_cases as pc
import pcm_format_cases as fc
from conftest import package, synth_input
from loudness_cases import GATE_CLEARANCE, JOINS, SRC_OFFSETS, TOL, WEIGHTS, build_image, close, hop, k_weight  # noqa: F401

TILE = 256                                           # short-term powers the stage's workgroup takes at a time (kLoudRangeThreads, SMST_LOUDNESS_RANGE_TILE):
#                                                      the one capacity the selection has -- it has no small-n path, and reads the values where they lie
WINDOW = 30                                          # sub-blocks of a short-term power
ABS_GATE = ld.ABS_GATE
FIXED, PROTECT, NORMALISE, LOUDNESS = lc.FIXED, lc.PROTECT, lc.NORMALISE, ld.LOUDNESS
COUNTER = "clip_loudness_range"
compared = dict(powers=0)                            # short-term powers, maxima and order statistics compared with the mirror so far (EXPERIMENTS.md)


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def ranks(n):
    """(kLo, kHi): the nearest ranks of the 10th and the 95th percentile among n values"""
    return ((n - 1)*10 + 50)//100, ((n - 1)*95 + 50)//100


def lufs_of(power):
    return -0.691 + 10*math.log10(power) if power > 0 else -math.inf


def power_of(lufs):
    return 10**((lufs + 0.691)/10)


def _largest(v):
    v = np.asarray(v, np.float64)
    v = v[~np.isnan(v)]
    return float(v.max()) if v.size else 0.0


def gate_and_select(st):
    """the gates in block order and the nearest ranks, float64 -> dict: first (the count past the absolute gate), rel, n, lo, hi, lra"""
    st = np.asarray(st, np.float64)
    with np.errstate(invalid="ignore"):
        first = st > ABS_GATE
        rel = 0.01*(float(np.cumsum(st[first])[-1])/int(first.sum())) if first.any() else 0.0     # (cumsum: one sum in block order)
        both = first & (st > rel)
    v = np.sort(st[both])
    n = len(v)
    lo, hi = (float(v[ranks(n)[0]]), float(v[ranks(n)[1]])) if n else (0.0, 0.0)
    with np.errstate(divide="ignore"):
        lra = 10*math.log10(hi/lo) if n and lo > 0 and math.isfinite(hi) else 0.0
    return dict(first=int(first.sum()), rel=rel, n=n, lo=lo, hi=hi, lra=lra)


def mirror(x, fs, weights=None, y=None):
    """x [C, N] of one clip (y: its K-weighted channels, where the caller has them) -> dict: z, st, M, ST, ns, and gate_and_select(st)'s"""
    x = np.asarray(x, np.float64)
    Cn, N = x.shape
    w = np.ones(Cn) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    h = hop(fs)
    n_sub = N//h if N >= 4*h else 0
    nb, ns = (n_sub - 3 if n_sub else 0), (n_sub - (WINDOW - 1) if n_sub >= WINDOW else 0)
    y = k_weight(x, fs) if y is None else y
    with np.errstate(invalid="ignore", over="ignore"):
        sub = (y[:, :n_sub*h]**2).reshape(Cn, n_sub, h).sum(axis=2)
        z = np.array([sum(w[c]*float(sub[c, i:i + 4].sum()) for c in range(Cn))/(4*h) for i in range(nb)], np.float64)
        q = np.zeros((Cn, ns))
        for j in range(WINDOW):                                                                   # (from 0.0, in ascending j)
            q = q + sub[:, j:j + ns]
        st = np.zeros(ns)
        for c in range(Cn):                                                                       # (in channel order)
            st = st + w[c]*q[c]
        st = st/(WINDOW*h)
    m = dict(z=z, st=st, M=_largest(z), ST=_largest(st), ns=ns)
    m.update(gate_and_select(st))
    return m


def gates_clear(m):
    """no short-term power within GATE_CLEARANCE (relative) of either LRA gate, no block power within it of an integrated gate"""
    st = m["st"][np.isfinite(m["st"])]
    for gate in (ABS_GATE, m["rel"]):
        if gate > 0 and st.size and np.min(np.abs(st/gate - 1)) < GATE_CLEARANCE:
            return False
    z = m["z"]
    with np.errstate(invalid="ignore"):
        first = z > ABS_GATE
    rel = 0.1*z[first].mean() if first.any() else 0.0
    return ld.gates_clear(dict(z=z, rel=rel))


def cap_gain(cap_lufs, top):
    """float32(sqrt(P/top)) where the cap is finite and the maximum finite and above 0, else +inf"""
    if not (math.isfinite(cap_lufs) and top > 0 and math.isfinite(top)):
        return np.float32(np.inf)
    with np.errstate(over="ignore"):
        return np.float32(math.sqrt(power_of(cap_lufs)/top))


def _sine_parts(levels, fs, seconds=20):
    n = seconds*fs
    t = np.arange(n*len(levels))
    return np.sin(2*np.pi*1000*t/fs)*np.repeat([10**(db/20) for db in levels], n)


def _k_weight_scalar(x, fs):
    """loudness_cases.k_weight of ONE row, the same operations in the same order on Python floats (a numpy loop over a single row spends its
    time on call overhead: this is several times quicker, and check_mirror holds it against k_weight bit for bit)"""
    out = [float(v) for v in x]
    sb, sa, hb, ha = ld.k_coefficients(fs)
    for b, a in ((sb, sa), (hb, ha)):
        b0, b1, b2, a1, a2 = b[0], b[1], b[2], a[1], a[2]
        x1 = x2 = y1 = y2 = 0.0
        for i, x0 in enumerate(out):
            y0 = b0*x0 + b1*x1 + b2*x2 - a1*y1 - a2*y2
            out[i] = y0
            x2, x1, y2, y1 = x1, x0, y1, y0
    return np.array(out, np.float64)


KNOWN = (((-20, -30), 10.0, 371, 371), ((-20, -15), 5.0, 371, 371), ((-40, -20), 20.0, 371, 371), ((-50, -35, -20, -35, -50), 15.0, 627, 971))


def check_mirror(fs=8000):
    """the known answers of include/smst.h's definition (Tech 3342's conformance signals: a stereo 1-kHz sine in parts of 20 s) within 1e-6 LU
    and with exact counts, the maxima of the first, and the nearest-rank formulas"""
    assert [ranks(n) for n in (1, 2, 10, 11, 21)] == [(0, 0), (0, 1), (1, 9), (1, 10), (2, 19)]
    for n in (1, 2, 10, 11, 21, 371, 627):
        assert ranks(n) == (int(math.floor(0.10*(n - 1) + 0.5)), int(math.floor(0.95*(n - 1) + 0.5))), n
    probe = _sine_parts((-20, -30), fs, 1)[:3000]
    assert np.array_equal(_k_weight_scalar(probe, fs), k_weight(probe[None, :], fs)[0])
    for k, (levels, lra, n, ns) in enumerate(KNOWN):
        x = _sine_parts(levels, fs)
        y = _k_weight_scalar(x, fs)
        m = mirror(np.stack([x, x]), fs, None, np.stack([y, y]))
        assert abs(m["lra"] - lra) < 1e-6 and (m["n"], m["ns"]) == (n, ns), (levels, m["lra"], m["n"], m["ns"])
        assert gates_clear(m), levels
        if k == 0:
            assert abs(lufs_of(m["M"]) + 19.9804) < 5e-5 and abs(lufs_of(m["ST"]) + 19.9804) < 5e-5, (lufs_of(m["M"]), lufs_of(m["ST"]))
    quiet = mirror(np.zeros((2, 40*hop(fs))), fs)
    assert (quiet["n"], quiet["ns"], quiet["lra"], quiet["M"], quiet["ST"]) == (0, 11, 0.0, 0.0, 0.0)


# ---- 1. the hook against the mirror ------------------------------------------------------------------------------------------------------

def run_hook(lib, clips, fs, weights, joins, offsets, target=-23.0, caps=None, base_offset=1):
    """-> (the hook's results, the image's parts)"""
    pkg = package()
    Cn = clips[0].shape[0]
    image, segs, iss, ics = build_image(clips, joins, offsets, base_offset)
    most = max(max(x.shape[1]//hop(fs) for x in clips), 1)
    before = [pkg.launch_count(k, lib) for k in (COUNTER, "clip_loudness")]
    assert before[0] >= 0, "the library has no %s counter" % COUNTER
    res = pkg.debug_clip_loudness_range(segs, Cn, image, iss, ics, fs, weights, target, caps, most, lib=lib)
    assert [pkg.launch_count(k, lib) - n for k, n in zip((COUNTER, "clip_loudness"), before)] == [1, 1]
    return res, (image, segs, iss, ics)


def compare_hook(lib, clips, fs, weights, joins, offsets, mirrors=None, **kw):
    """the hook on the clips' image against the mirror of every clip -> (the mirrors, the hook's results)"""
    mirrors = [mirror(x, fs, weights) for x in clips] if mirrors is None else mirrors
    assert all(gates_clear(m) for m in mirrors), "a power lies on a gate: change the input"
    (M, ST, lo, hi, ns, n, gains, powers), _ = run_hook(lib, clips, fs, weights, joins, offsets, **kw)
    for s, m in enumerate(mirrors):
        where = dict(stream=s, fs=fs, C=clips[s].shape[0], frames=clips[s].shape[1])
        assert (int(ns[s]), int(n[s])) == (m["ns"], m["n"]), (where, int(ns[s]), int(n[s]), m["ns"], m["n"])
        assert close(powers[s, :m["ns"]], m["st"]) and np.isnan(powers[s, m["ns"]:]).all(), where
        for name, got, want in (("M", M[s], m["M"]), ("ST", ST[s], m["ST"]), ("lo", lo[s], m["lo"]), ("hi", hi[s], m["hi"])):
            assert close(got, want), (where, name, float(got), want)
        compared["powers"] += m["ns"] + 4
    return mirrors, (M, ST, lo, hi, ns, n, gains, powers)


def hook_lengths(fs):
    """4h - 1 (nothing), 4h, 30h - 1 (no short-term power), 30h (one), 31h - 1, 31h (two), and n = TILE and TILE + 1: the stage's one capacity
    and one more (the selection has no small-n path; every n goes through the same passes)"""
    h = hop(fs)
    return (4*h - 1, 4*h, WINDOW*h - 1, WINDOW*h, (WINDOW + 1)*h - 1, (WINDOW + 1)*h, (TILE + WINDOW - 1)*h + 17, (TILE + WINDOW)*h)


_hook_reference = {}


def hook_reference(fs):
    """the 16-channel clips of hook_lengths(fs) and their K-weighted channels, computed once: a case of C channels takes the first C"""
    if fs not in _hook_reference:
        rng = pc._rng(9301, int(fs))
        clips = [ld._clip(rng, 16, n, s) for s, n in enumerate(hook_lengths(fs))]
        ys = [None]*len(clips)
        for group in (range(6), range(6, 8)):                                       # (the short clips side by side, then the two long ones)
            most = max(clips[s].shape[1] for s in group)
            rows = np.zeros((len(group)*16, most))
            for k, s in enumerate(group):
                rows[16*k:16*k + 16, :clips[s].shape[1]] = clips[s]
            y = k_weight(rows, fs)
            for k, s in enumerate(group):
                ys[s] = y[16*k:16*k + 16, :clips[s].shape[1]]
        _hook_reference[fs] = (clips, ys)
    return _hook_reference[fs]


def check_hook(lib, fs, channels):
    """the four passes and the range stage through smst_debug_clip_loudness_range against the mirror: eight streams of hook_lengths, the
    joins, odd row offsets and weights of loudness_cases.check_hook"""
    clips, ys = hook_reference(fs)
    clips = [np.ascontiguousarray(x[:channels]) for x in clips]
    mirrors = [mirror(x, fs, WEIGHTS[channels], y[:channels]) for x, y in zip(clips, ys)]
    compare_hook(lib, clips, fs, WEIGHTS[channels], JOINS, SRC_OFFSETS, mirrors)
    assert [m["ns"] for m in mirrors] == [0, 0, 0, 1, 1, 2, TILE, TILE + 1] and [m["n"] for m in mirrors] == [m["ns"] for m in mirrors]
    assert [len(m["z"]) for m in mirrors[:4]] == [0, 1, WINDOW - 4, WINDOW - 3] and mirrors[1]["M"] > 0 and mirrors[0]["M"] == 0
    print("largest |p/p_mirror - 1| so far: %.3g over %d powers" % (ld.worst_seen["power"], compared["powers"]))


LOWEST_FS = 2560                                     # h = the chunk of the loudness passes: the lowest rate the setters accept


def check_hook_lowest_rate(lib, channels=2):
    """fs = 2560, where h equals the chunk.  The K-weighting shelf's centre (1682 Hz) lies above this rate's Nyquist frequency: its biquad is
    unstable (a2 = 3.9), a sequential filter overflows within 1000 samples and the chunked one at once (A^256 is not finite), so no power
    of the two can be compared -- every one is inf or NaN, in either.  What is defined is checked: the counts ns of hook_lengths, n = 0
    (a NaN passes no gate, and +inf does not pass a relative gate of +inf), lo = hi = 0, and two runs with the same bits"""
    rng = pc._rng(9301, LOWEST_FS)
    clips = [ld._clip(rng, channels, n, s) for s, n in enumerate(hook_lengths(LOWEST_FS))]
    runs = [run_hook(lib, clips, LOWEST_FS, WEIGHTS[channels], JOINS, SRC_OFFSETS)[0] for _ in range(2)]
    M, ST, lo, hi, ns, n, gains, powers = runs[0]
    assert ns.tolist() == [0, 0, 0, 1, 1, 2, TILE, TILE + 1] and not n.any() and not lo.any() and not hi.any(), (ns.tolist(), n.tolist())
    assert not np.isfinite(powers[7, :TILE + 1]).any() and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*runs))


# ---- 2. the selection, bit for bit -------------------------------------------------------------------------------------------------------

def selection_clips(fs=5120, Cn=2):
    """-> clips whose gated values hold exact duplicates (the samples repeat with period h = two chunks: every sub-block is filtered from
    the same state once the transient is gone), ascend (a slow fade in) and descend (a slow fade out)"""
    h = hop(fs)
    n = 80*h
    rng = pc._rng(9302, int(fs))
    period = rng.uniform(-0.4, 0.4, (Cn, h)).astype(np.float32)
    noise = rng.uniform(-0.4, 0.4, (Cn, n)).astype(np.float32)
    ramp = np.linspace(0.05, 1.0, n).astype(np.float32)
    return [np.tile(period, (1, n//h)), noise*ramp[None, :], noise*ramp[None, ::-1]]


def _bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def check_selection(lib, fs=5120):
    """from the hook's own short-term powers, a host that gates in float64 in block order, sorts and takes the nearest ranks gets lo, hi, both
    counts and ST bit for bit; M is the largest block power of smst_debug_clip_loudness on the same image"""
    pkg = package()
    clips = selection_clips(fs)
    (M, ST, lo, hi, ns, n, gains, powers), (image, segs, iss, ics) = run_hook(lib, clips, fs, (1.0, 1.41), (1003, 0, 257), SRC_OFFSETS)
    _, _, _, _, z = pkg.debug_clip_loudness(segs, 2, image, iss, ics, fs, (1.0, 1.41), -23.0, powers.shape[1] + WINDOW, lib=lib)
    shapes = []
    for s in range(len(clips)):
        st = powers[s, :ns[s]]
        want = gate_and_select(st)
        assert int(ns[s]) == clips[s].shape[1]//hop(fs) - (WINDOW - 1) and not np.isnan(st).any()
        assert int(n[s]) == want["n"] and want["n"] > 20, (s, int(n[s]), want["n"])
        assert _bits(lo[s]) == _bits(want["lo"]) and _bits(hi[s]) == _bits(want["hi"]), (s, float(lo[s]), want["lo"], float(hi[s]), want["hi"])
        assert _bits(ST[s]) == _bits(_largest(st)) and _bits(M[s]) == _bits(_largest(z[s])), (s, float(ST[s]), float(M[s]))
        with np.errstate(invalid="ignore"):
            gated = st[(st > ABS_GATE) & (st > want["rel"])]
        shapes.append((len(np.unique(gated)) < len(gated), bool((np.diff(gated) > 0).all()), bool((np.diff(gated) < 0).all())))
        compared["powers"] += 4
    assert shapes == [(True, False, False), (False, True, False), (False, False, True)], shapes


# ---- 3. content --------------------------------------------------------------------------------------------------------------------------

def content_clips(fs, Cn=2):
    """-> loud then -40 dB; a stretch at 1e-4; silence; a NaN in the middle; a clip shorter than 3 s"""
    h = hop(fs)
    rng = pc._rng(9303, int(fs))
    loud = lambda n: (rng.uniform(-0.3, 0.3, (Cn, n))).astype(np.float32)
    a = loud(100*h)
    a[:, 40*h:] *= np.float32(0.01)
    b = loud(100*h)
    b[:, 30*h:70*h] = rng.uniform(-1e-4, 1e-4, (Cn, 40*h)).astype(np.float32)
    c = np.zeros((Cn, 60*h), np.float32)
    d = loud(60*h)
    d[0, 45*h + 17] = np.nan
    e = loud(10*h)
    return [a, b, c, d, e]


def check_content(lib, fs=8000):
    """what the gates and the maxima are for: the relative gate drops the short-term powers of the quiet part (0 < n < ns), the absolute gate
    those of the stretch at 1e-4; silence has n = 0, LRA 0 and maxima of 0 (-inf LUFS); a NaN leaves the powers in front of it and the
    maxima skip it; a clip shorter than 3 s has no short-term power, and its momentary maximum is reported all the same"""
    clips = content_clips(fs)
    mirrors, (M, ST, lo, hi, ns, n, gains, powers) = compare_hook(lib, clips, fs, None, (1003, 0, 5, 257, 2), SRC_OFFSETS)
    a, b, c, d, e = mirrors
    assert a["first"] == a["ns"] and 0 < a["n"] < a["ns"] and a["lra"] > 1
    assert 0 < b["first"] < b["ns"] and 0 < b["n"] <= b["first"]
    assert (c["ns"], c["n"], c["lra"]) == (31, 0, 0.0) and M[2] == ST[2] == lo[2] == hi[2] == 0.0 and lufs_of(float(M[2])) == -math.inf
    assert 0 < d["n"] < d["ns"] and np.isnan(d["st"][-1]) and np.isnan(d["z"][-1]) and math.isfinite(d["M"]) and d["M"] > 0 and d["ST"] > 0
    assert (e["ns"], e["n"]) == (0, 0) and e["M"] > 0 and ST[4] == 0.0 and M[4] > 0


# ---- 4. caps -----------------------------------------------------------------------------------------------------------------------------

def check_caps(lib, fs=8000):
    """gL' = min(gL, gm, gs) of the mirror within an ulp: a stream where the momentary cap decides, one where the short-term cap does, one where
    neither does -- the bits of gL from smst_debug_clip_loudness --, a stream below the absolute gate (no loudness: gL = 1, and the cap still
    acts), silence (nothing to cap) and a call without caps"""
    pkg = package()
    h = hop(fs)
    rng = pc._rng(9304, int(fs))
    clips = [(rng.uniform(-0.3, 0.3, (2, 40*h))*np.linspace(0.3, 1.0, 40*h)[None, :]).astype(np.float32) for _ in range(3)]
    clips.append(rng.uniform(-1e-4, 1e-4, (2, 40*h)).astype(np.float32))
    clips.append(np.zeros((2, 40*h), np.float32))
    target = -23.0
    mirrors = [mirror(x, fs) for x in clips]
    loud = [ld.mirror(x, fs, None, target) for x in clips]
    assert all(m["defined"] for m in loud[:3]) and not loud[3]["defined"] and loud[3]["gain"] == 1.0 and mirrors[3]["M"] > 0
    db = lambda g: 20*math.log10(float(g))
    caps = np.full((5, 2), np.inf)
    caps[0] = (lufs_of(mirrors[0]["M"]) + db(loud[0]["gain"]) - 6, lufs_of(mirrors[0]["ST"]) + db(loud[0]["gain"]) - 2)
    caps[1] = (lufs_of(mirrors[1]["M"]) + db(loud[1]["gain"]) - 1, lufs_of(mirrors[1]["ST"]) + db(loud[1]["gain"]) - 3)
    caps[2] = (lufs_of(mirrors[2]["M"]) + db(loud[2]["gain"]) + 20, lufs_of(mirrors[2]["ST"]) + db(loud[2]["gain"]) + 3)
    caps[3] = (lufs_of(mirrors[3]["M"]) - 6, np.inf)
    caps[4] = (-40.0, -40.0)
    joins = (1003, 0, 5, 257, 2)
    _, (M, ST, lo, hi, ns, n, gains, powers) = compare_hook(lib, clips, fs, None, joins, SRC_OFFSETS, mirrors, target=target, caps=caps)
    image, segs, iss, ics = build_image(clips, joins, SRC_OFFSETS)
    plain = pkg.debug_clip_loudness(segs, 2, image, iss, ics, fs, None, target, 0, lib=lib)[3]
    decides = []
    for s in range(5):
        gm, gs = cap_gain(caps[s, 0], mirrors[s]["M"]), cap_gain(caps[s, 1], mirrors[s]["ST"])
        want = min(loud[s]["gain"], gm, gs)
        assert gains.dtype == np.float32 and ld.ulps32(gains[s], want) <= 1, (s, float(gains[s]), float(want))
        decides.append("m" if gm < min(loud[s]["gain"], gs) else "s" if gs < min(loud[s]["gain"], gm) else "-")
        if decides[-1] == "-":
            assert gains[s].view(np.uint32) == plain[s].view(np.uint32), (s, float(gains[s]), float(plain[s]))
        else:
            assert gains[s] < plain[s], s
    assert decides == ["m", "s", "-", "m", "-"] and gains[4] == 1.0, decides
    _, (_, _, _, _, _, _, uncapped, _) = compare_hook(lib, clips, fs, None, joins, SRC_OFFSETS, mirrors, target=target)
    assert np.array_equal(uncapped.view(np.uint32), plain.view(np.uint32))


def check_reproducible(lib, fs=5120):
    """two runs of the hook give the same bits"""
    clips = selection_clips(fs)
    caps = np.array([[-30.0, np.inf], [np.inf, -30.0], [np.inf, np.inf]])
    runs = [run_hook(lib, clips, fs, (1.0, 1.41), (1003, 0, 257), SRC_OFFSETS, caps=caps)[0] for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert runs[0][5].min() > 0


# ---- 5. whole clips through smst_batch_exact_pcm -----------------------------------------------------------------------------------------

CLIP_FS = 4000.0                                     # h = 400: a low rate (its shelf is still stable), so that clips of 12000 frames have short-term powers
CLIP_H = 400
CLIPS = dict(inputs=[6000, 7500, 200, 9000, 10500, 9800, 7500, 6000], outputs=[13500, 12300, 300, 12000, 13100, 12800, 11700, 12000], short=2, left=7)
#  per stream: (mode, gain, target, meter flag, (momentary cap, short-term cap), limiter)
INF = float("inf")
CLIP_STREAMS = ((FIXED, 0.5, None, True, (INF, INF), False),         # metered, at the flag's rate
                (NORMALISE, 1.0, None, True, (INF, INF), False),     # metered
                (LOUDNESS, 1.0, -20.0, True, (INF, INF), False),     # too short
                (LOUDNESS, 1.0, -20.0, True, (INF, INF), False),     # metered, at the mode's rate
                (LOUDNESS, 1.0, -16.0, False, (INF, -30.0), False),  # capped: the cap implies the meter, and decides
                (LOUDNESS, 1.0, 6.0, False, (2.0, 40.0), True),      # capped and limited: the momentary cap decides, the limiter holds the ceiling
                (PROTECT, 8.0, None, False, (INF, INF), False),      # unflagged
                (LOUDNESS, 1.0, -20.0, True, (-30.0, INF), False))   # left out
CLIP_SEED = 47


def clip_frames(fmt):
    frames = fc.encode_frames(pc.frames_of(xc.clip_inputs(2, CLIPS["inputs"], loud=0)), fmt)
    return frames, np.ascontiguousarray(np.transpose(fc.decode_frames(frames, fmt), (0, 2, 1)))


def set_clip_streams(batch, ceil, flags=True):
    for s, (mode, gain, target, meter, caps, limiter) in enumerate(CLIP_STREAMS):
        if mode == LOUDNESS:
            batch.set_pcm_loudness(target, ceil, CLIP_FS, stream=s)
        else:
            batch.set_pcm_level(mode, gain, ceil, stream=s)
        batch.set_pcm_limiter(limiter, stream=s)
        if flags:
            batch.set_pcm_loudness_range(meter, CLIP_FS, stream=s)
            batch.set_pcm_loudness_caps(*caps, stream=s)
            assert batch.pcm_loudness_range(s) == (meter, CLIP_FS if meter else 0.0) and batch.pcm_loudness_caps(s) == caps


_clip_mirrors = {}


def clip_mirrors(x, weights, target):
    """(mirror, loudness_cases.mirror) of one rendered clip, computed once per content: the calls, the memory kinds and most formats render
    the same floats"""
    key = (hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest(), x.shape, tuple(weights), target)
    if key not in _clip_mirrors:
        _clip_mirrors[key] = (mirror(x, CLIP_FS, weights), ld.mirror(x, CLIP_FS, weights, target))
    return _clip_mirrors[key]


def check_clips(lib, fmt, dithered, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True), calls=2):
    """exactFrames of CLIPS with CLIP_STREAMS, `calls` times: the range meters and -- for every measured stream, FIXED and NORMALISE included -- the
    integrated loudness are the mirrors' of smst_batch_exact's planar output; a metered stream outside the loudness mode has the gain of a
    twin batch without any flag, a capped one min(gL, gm, gs) within an ulp, limited by ceiling/peak unless the limiter holds the ceiling;
    the bytes are the level mirror -- the limiter's for the limited stream, whose need follows from the capped gain -- at the gain the device
    reported; the unflagged, the short and the left-out stream have the bytes of the twin batch"""
    pkg = package()
    win = lm.library_window(lib, lm.DEFAULT_H)
    nin, nout, short, left = CLIPS["inputs"], CLIPS["outputs"], CLIPS["short"], CLIPS["left"]
    S, Cn, most = len(nin), 2, max(nout)
    frames, planar = clip_frames(fmt)
    p, f, u = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(3))
    ceil = lc.ceiling(fmt, dithered)
    modes = [dc.CLIP_MODES[s % len(dc.CLIP_MODES)] if dithered else dc.NONE for s in range(S)]
    weights = (1.0, 1.41)
    for b in (f, u):
        b.set_pcm_loudness_weights(weights)
        for s in range(S):
            if dithered:
                b.setPcmDither(modes[s], CLIP_SEED + s, stream=s)
    set_clip_streams(f, ceil)
    set_clip_streams(u, ceil, flags=False)
    assert f.take_pcm_loudness_range()[5].tolist() == [0]*S                      # (nothing has metered yet)
    n_out = [(-1 if s == left else n) for s, n in enumerate(nout)]
    counters = (COUNTER, "clip_loudness", "clip_out_limited")
    for call in range(calls):
        want, ok_p = p.exact(planar, n_out, in_samples=nin)
        want = np.array(want, copy=True)
        fill = lambda: np.full(frames.shape[:1] + (most,) + frames.shape[2:], 0x5A, frames.dtype)
        plain, _ = u.exactFrames(to_memory(frames), n_out, in_samples=nin, out=to_memory(fill()))
        plain = to_host(plain)
        _, plain_gains = u.take_pcm_peaks()
        plain_lufs = u.take_pcm_loudness()[0]
        before = [pkg.launch_count(k, lib) for k in counters]
        got, ok_f = f.exactFrames(to_memory(frames), n_out, in_samples=nin, out=to_memory(fill()))
        got = to_host(got)
        assert [pkg.launch_count(k, lib) - n for k, n in zip(counters, before)] == [1, 1, 1]
        assert ok_p.tolist() == ok_f.tolist() == [s not in (short, left) for s in range(S)]
        mmax, smax, lra, low, high, ns, n = f.take_pcm_loudness_range()
        again = f.take_pcm_loudness_range()
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((mmax, smax, lra, low, high, ns, n), again))   # (a take resets nothing)
        lufs, blocks, gated = f.take_pcm_loudness()
        peaks, gains = f.take_pcm_peaks()
        low_r, count_r = f.take_pcm_limiter()
        overs = f.takePcmOvers()[0]
        expect = fill()
        for s in range(S):
            where = dict(fmt=fmt, dithered=dithered, call=call, stream=s)
            mode, gain, target, meter, caps, limiter = CLIP_STREAMS[s]
            metered = meter or (mode == LOUDNESS and any(map(math.isfinite, caps)))
            if s in (short, left):
                assert (mmax[s], smax[s], lra[s], low[s], high[s], ns[s], n[s]) == (-math.inf, -math.inf, 0.0, -math.inf, -math.inf, 0, 0), where
                assert lufs[s] == -math.inf and np.array_equal(got[s], plain[s]), where
                expect[s] = plain[s]
                continue
            x = want[s, :, :nout[s]]
            assert tp_same(peaks[s], lc.peak_of(x)), where
            if not metered:
                assert (ns[s], n[s], mmax[s], lra[s]) == (0, 0, -math.inf, 0.0), where
                assert tp_same(gains[s], plain_gains[s]) and np.array_equal(got[s], plain[s]) and (lufs[s] == plain_lufs[s] or mode == LOUDNESS), where
                expect[s] = plain[s]
                continue
            m, li = clip_mirrors(x, weights, target if target is not None else 0.0)
            assert gates_clear(m) and m["ns"] == nout[s]//CLIP_H - (WINDOW - 1) and m["n"] > 0, (where, m["ns"], m["n"])
            assert (int(ns[s]), int(n[s])) == (m["ns"], m["n"]), (where, int(ns[s]), int(n[s]), m["ns"], m["n"])
            for name, got_lufs, power in (("M", mmax[s], m["M"]), ("ST", smax[s], m["ST"]), ("lo", low[s], m["lo"]), ("hi", high[s], m["hi"])):
                assert close(power_of(got_lufs), power), (where, name, got_lufs, lufs_of(power))
            assert abs(lra[s] - m["lra"]) <= 1e-8 and close(power_of(lufs[s]), li["Z"]) and (int(blocks[s]), int(gated[s])) == (li["blocks"], li["gated"]), (where, lra[s], m["lra"])
            compared["powers"] += 5
            q = lc.gain_of(PROTECT, np.float32(np.inf), ceil, lc.peak_of(x))       # (ceiling/peak)
            if mode != LOUDNESS:
                assert tp_same(gains[s], plain_gains[s]) and tp_same(gains[s], lc.gain_of(mode, gain, ceil, lc.peak_of(x))), (where, float(gains[s]))
                assert np.array_equal(got[s], plain[s]), where
            else:
                gm, gs = cap_gain(caps[0], m["M"]), cap_gain(caps[1], m["ST"])
                capped = min(li["gain"], gm, gs)
                assert (capped < li["gain"]) == any(map(math.isfinite, caps)), (where, float(capped), float(li["gain"]))
                if limiter or not (capped > q and ld.ulps32(capped, q) > 1):
                    assert ld.ulps32(gains[s], capped) <= 1, (where, float(gains[s]), float(capped))
                else:
                    assert tp_same(gains[s], q), (where, float(gains[s]), float(q))
                if capped < li["gain"]:
                    assert gains[s] < plain_gains[s] or limiter, where
            if limiter:
                need, r, lowest, n_limited = lm.mirror(x, gains[s], ceil, lm.DEFAULT_H, win)
                assert n_limited > 0 and tp_same(low_r[s], lowest) and int(count_r[s]) == n_limited, (where, float(low_r[s]), float(lowest), int(count_r[s]), n_limited)
                codes, cm, _ = dc.mirror(lm.limited(x, gains[s], r), fmt, modes[s], CLIP_SEED + s, 0)
            else:
                assert low_r[s] == 1 and count_r[s] == 0, where
                codes, cm, _ = lc.mirror(x, fmt, gains[s], modes[s], CLIP_SEED + s, 0)
            assert overs[s] == int(cm.sum()), (where, int(overs[s]), int(cm.sum()))
            expect[s, :nout[s]] = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
        assert lc.same_bytes(got.reshape(-1).view(np.uint8), expect.reshape(-1).view(np.uint8), fmt), (fmt, dithered, call)
        assert (got[left] == 0x5A).all() and not got[short, :nout[short]].any()
    for b in (p, f, u):
        b.close()


def tp_same(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


def run_clips(lib, fmt=fc.S16):
    """the bytes and every meter of one metered call on a fresh batch"""
    pkg = package()
    frames, _ = clip_frames(fmt)
    b = pkg.StretchBatch(len(CLIPS["inputs"]), 2, lib=lib, seed=3, **pc.GEOMETRY)
    set_clip_streams(b, lc.ceiling(fmt, False))
    out, ok = b.exactFrames(frames, CLIPS["outputs"], in_samples=CLIPS["inputs"])
    res = [np.array(out, copy=True), ok] + list(b.take_pcm_loudness_range()) + list(b.take_pcm_loudness()) + list(b.take_pcm_peaks())
    b.close()
    return res


def check_two_runs(lib):
    a, b = run_clips(lib), run_clips(lib)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert a[0].any() and (a[8] > 0).sum() == 6                                  # (every stream but the short and the unflagged one has gated values)


# ---- 6. opt-in, steady state, refusals ---------------------------------------------------------------------------------------------------

def check_opt_in(lib, **memory):
    """without the flag or a cap the stage is never launched: the loudness mode's own whole-clip case runs as before; a flagged stream in a
    call that leaves it out does not start it either, nor the four passes"""
    pkg = package()
    before = pkg.launch_count(COUNTER, lib)
    assert before >= 0, "the library has no %s counter" % COUNTER
    ld.check_clips(lib, fc.S16, 8000, **memory)
    assert pkg.launch_count(COUNTER, lib) == before
    nin, nout = CLIPS["inputs"][:3], CLIPS["outputs"][:3]
    frames = memory.get("to_memory", lambda a: a)(clip_frames(fc.S16)[0][:3])
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_loudness_range(True, CLIP_FS, stream=1)
    for counts, ran in (([nout[0], -1, nout[2]], 0), (nout, 1)):
        before = [pkg.launch_count(k, lib) for k in (COUNTER, "clip_loudness")]
        b.exactFrames(frames, counts, in_samples=nin)
        b.synchronize()
        assert [pkg.launch_count(k, lib) - n for k, n in zip((COUNTER, "clip_loudness"), before)] == [ran, ran], counts
    mmax, smax, lra, low, high, ns, n = b.take_pcm_loudness_range()
    assert ns.tolist() == [0, nout[1]//CLIP_H - (WINDOW - 1), 0] and math.isfinite(mmax[1]) and mmax[0] == mmax[2] == -math.inf
    assert math.isfinite(b.take_pcm_loudness()[0][1]) and b.take_pcm_peaks()[1].tolist() == [1.0]*3       # (measured, and still FIXED at gain 1)
    b.close()


def check_steady_state(lib, to_memory=lambda a: a):
    """the first metering call grows the scratch (workspace bytes), a second call of the same shapes allocates nothing, nor do the takes"""
    pkg = package()
    nin, nout = CLIPS["inputs"][:3], CLIPS["outputs"][:3]
    clips = to_memory(clip_frames(fc.S16)[0][:3])
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_loudness(-23.0, 0.9, CLIP_FS)
    for _ in range(2):
        b.exactFrames(clips, nout, in_samples=nin)
    b.synchronize()
    plain = b.workspaceBytes()
    b.set_pcm_loudness_range(True, CLIP_FS)
    for _ in range(2):
        b.exactFrames(clips, nout, in_samples=nin)
    b.synchronize()
    events, grown = b.allocation_events(), b.workspaceBytes()
    assert grown > plain
    b.exactFrames(clips, nout, in_samples=nin)
    res = b.take_pcm_loudness_range()
    b.take_pcm_loudness()
    assert b.allocation_events() == events and b.workspaceBytes() == grown and res[5].tolist() == [nout[0]//CLIP_H - 29, nout[1]//CLIP_H - 29, 0]
    b.close()


def check_refusals(lib):
    pkg = package()
    b = pkg.StretchBatch(2, 3, lib=lib, **pc.GEOMETRY)
    inf, nan = float("inf"), float("nan")
    for args, word in (((0, 1, inf), b"rate"), ((0, 1, nan), b"rate"), ((0, 1, 0.0), b"rate"), ((0, 1, -48000.0), b"rate"), ((0, 1, 10.0*ld.CHUNK - 6), b"rate"),
                       ((2, 1, 8000.0), b"stream"), ((-2, 1, 8000.0), b"stream"), ((2, 0, 8000.0), b"stream")):
        assert lib.smst_batch_set_pcm_loudness_range(b.h, *args) == -1 and word in lib.smst_last_error(), (args, lib.smst_last_error())
    for args, word in (((0, nan, inf), b"cap"), ((0, inf, nan), b"cap"), ((0, -inf, inf), b"cap"), ((0, -20.0, -inf), b"cap"), ((2, -20.0, inf), b"stream"), ((-2, inf, inf), b"stream")):
        assert lib.smst_batch_set_pcm_loudness_caps(b.h, *args) == -1 and word in lib.smst_last_error(), (args, lib.smst_last_error())
    assert [b.pcm_loudness_range(s) for s in range(2)] == [(False, 0.0)]*2 and [b.pcm_loudness_caps(s) for s in range(2)] == [(inf, inf)]*2   # (a refused call changes nothing)
    assert lib.smst_batch_set_pcm_loudness_range(None, 0, 1, 8000.0) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_loudness_range(None, 0, None, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_set_pcm_loudness_caps(None, 0, inf, inf) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_loudness_caps(None, 0, None, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_take_pcm_loudness_range(None, None, None, None, None, None, None, None) == -1 and b"null" in lib.smst_last_error()
    for stream in (-1, 2):
        assert lib.smst_batch_pcm_loudness_range(b.h, stream, None, None) == -1 and b"stream" in lib.smst_last_error()
        assert lib.smst_batch_pcm_loudness_caps(b.h, stream, None, None) == -1 and b"stream" in lib.smst_last_error()
    # what is allowed: the lowest rate with h = CHUNK, a rate that is not read with on == 0, null pointers in the getters and the take
    b.set_pcm_loudness_range(True, 10.0*ld.CHUNK - 5, stream=1)
    assert lib.smst_batch_set_pcm_loudness_range(b.h, 1, 0, nan) == 0
    assert b.pcm_loudness_range(1) == (False, 10.0*ld.CHUNK - 5) and b.pcm_loudness_range(0) == (False, 0.0)
    b.set_pcm_loudness_caps(-18.0, inf, stream=0)
    b.set_pcm_loudness_caps()
    assert b.pcm_loudness_caps(0) == (inf, inf)
    assert lib.smst_batch_pcm_loudness_range(b.h, 0, None, None) == 0 and lib.smst_batch_pcm_loudness_caps(b.h, 0, None, None) == 0
    assert lib.smst_batch_take_pcm_loudness_range(b.h, None, None, None, None, None, None, None) == 0
    assert pkg.LOUDNESS_RANGE_TILE == TILE
    b.close()


def check_refused_in_streaming_calls(lib, **memory):
    """a stream with the meter flag or a finite cap makes processFrames and flushFrames fail before anything runs"""
    pkg = package()
    frames, _ = dc.session_inputs(fc.S16)
    to_memory = memory.get("to_memory", lambda a: a)
    x = to_memory(np.ascontiguousarray(frames[:, :600]))
    for setting in (lambda b: b.set_pcm_loudness_range(True, 8000, stream=1), lambda b: b.set_pcm_loudness_caps(-20.0, stream=1), lambda b: b.set_pcm_loudness_caps(INF, -20.0, stream=1)):
        b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
        setting(b)
        for call in (lambda: b.processFrames(x, [600, 300, 0]), lambda: b.flushFrames([100, 50, -1], like=to_memory(np.zeros((1,), np.float32)))):
            with dc.pytest_raises(pkg.StretchError) as e:
                call()
            assert "whole clip" in str(e.value) and "error -1" in str(e.value), str(e.value)
        b.flushFrames([100, -1, 100], like=to_memory(np.zeros((1,), np.float32)))     # (stream 1 takes no part: not refused)
        b.close()


# ---- 7. the command-line tool ------------------------------------------------------------------------------------------------------------

def range_lines(stdout):
    """the "range:" lines of a --loudness-range run -> [(file, momentary max, short-term max, LRA)]"""
    found = re.findall(r"^range: (\S+) momentary-max=(\S+) short-term-max=(\S+) lra=(\S+)$", stdout, re.M)
    return [(name, float(m), float(t), float(lra)) for name, m, t, lra in found]


def check_cli(cli, tmp_path):
    """--exact --loudness-range prints one line per file: what smst_batch_take_pcm_loudness_range reported, which is the mirror's of the
    --exact floats to the printed digits; the files and the other lines are those of a run without the option; --max-short-term with
    --loudness lowers the gain of the file whose short-term maximum would pass the cap, as the mirror says; the caps without --loudness and
    the meter without the exact flow are refused"""
    from test_cli import write_wav16
    sr, lengths = 8000, (30001, 33000)
    srcs = [str(tmp_path/("in%d.wav" % k)) for k in range(2)]
    write_wav16(srcs[0], 0.9*synth_input(1, 2, lengths[0], sr), sr)
    write_wav16(srcs[1], 0.2*synth_input(3, 2, lengths[1], sr), sr)

    def run(name, flags, expect=0):
        outs = [str(tmp_path/("%s%d.wav" % (name, k))) for k in range(2)]
        res = subprocess.run([cli, "--time=1.1"] + flags + [srcs[0], outs[0], srcs[1], outs[1]], capture_output=True, text=True)
        assert res.returncode == expect, (flags, res.returncode, res.stderr)
        return outs, res
    plain_outs, plain = run("out", ["--exact", "--out-format=f32"])
    assert "range:" not in plain.stdout
    floats = []
    for path in plain_outs:
        head, data = dc.data_chunk(path)
        assert head[:3] == (3, 2, sr)
        floats.append(np.ascontiguousarray(np.frombuffer(data, "<f4").reshape(-1, 2).T))
    wavs = [open(path, "rb").read() for path in plain_outs]
    mirrors = [mirror(x, sr) for x in floats]
    assert all(gates_clear(m) and m["n"] > 0 for m in mirrors)
    outs, res = run("out", ["--exact", "--out-format=f32", "--loudness-range"])
    lines = range_lines(res.stdout)
    assert len(lines) == 2 and "".join(l for l in res.stdout.splitlines(True) if not l.startswith("range: ")) == plain.stdout, res.stdout
    assert [open(path, "rb").read() for path in outs] == wavs                                      # (the meter changes no sample)
    for k, (path, mmax, smax, lra) in enumerate(lines):
        m = mirrors[k]
        assert path == outs[k] and abs(mmax - lufs_of(m["M"])) <= 5.1e-5 and abs(smax - lufs_of(m["ST"])) <= 5.1e-5 and abs(lra - m["lra"]) <= 5.1e-5, (k, mmax, smax, lra, m["lra"])
    target = -14.0
    gl = [ld.mirror(x, sr, None, target)["gain"] for x in floats]
    cap = round(lufs_of(mirrors[0]["ST"]) + 20*math.log10(float(gl[0])) - 4.0, 4)                   # (4 dB under what file 0 would reach)
    _, res = run("cap", ["--loudness=%g" % target, "--max-short-term=%.4f" % cap, "--out-format=s24", "--loudness-range"])
    lines, level = range_lines(res.stdout), ld.loudness_lines(res.stdout)
    assert len(lines) == len(level) == 2, res.stdout
    for k in range(2):
        want = min(gl[k], cap_gain(cap, mirrors[k]["ST"]))
        assert abs(float(level[k][3]) - float(want)) <= 1e-6*float(want), (k, float(level[k][3]), float(want), float(gl[k]))
        assert abs(lines[k][2] - lufs_of(mirrors[k]["ST"])) <= 5.1e-5
    assert float(level[0][3]) < 0.7*float(gl[0])
    for flags in (["--exact", "--max-short-term=-20"], ["--exact", "--max-momentary=-20"]):
        _, res = run("bad", flags, expect=2)
        assert "--loudness" in res.stderr
    _, res = run("bad", ["--loudness-range"], expect=2)
    assert "--exact" in res.stderr
