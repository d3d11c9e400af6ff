"""Shared cases of the loudness mode of the frame output (include/smst.h, "Loudness"): test_loudness_emu.py runs them on the CPU stand-in,
test_loudness_gpu.py on the device, next to level_cases.py.

The numpy mirror below restates the definition in float64: the two biquads as a plain sequential loop over time, the 400-ms blocks, the
two gates in the power domain, gL = float32(sqrt(P/Z)).  The device sums in another order (chunks of LOUDNESS_CHUNK frames), so the
comparison of a power is relative, within TOL = 1e-9: float64 round-off through this filter is far below that (about 1e-12; the noise gain at
these rates is about 1e3), a single-precision path gives about 1e-4.  The block counts are exact -- the case builders keep every block
1e-6 (relative) away from both gates --, gL is within 1 fp32 ulp, and the bytes of a whole clip are exactly level_cases.mirror of the planar
output at the gain the device reported."""
import math
import re
import subprocess

import numpy as np

import dither_cases as dc
import exact_cases as xc
import level_cases as lc
import pcm_cases as pc
import pcm_format_cases as fc
from conftest import package, synth_input

LOUDNESS = 3
CHUNK = 256                                          # frames one lane of the loudness passes filters (kLoudChunk, SMST_LOUDNESS_CHUNK)
TOL = 1e-9
GATE_CLEARANCE = 1e-6
ABS_GATE = 10**((-70 + 0.691)/10)
worst_seen = dict(power=0.0)                         # the largest |z/z_mirror - 1| a run met (printed by the tests; EXPERIMENTS.md)


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def hop(fs):
    return int(math.floor(fs/10 + 0.5))


def k_coefficients(fs):
    """-> (shelf b, shelf a, high-pass b, high-pass a), float64"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi*f0/fs)
    Vh = 10**(G/20)
    Vb = Vh**0.4996667741545416
    a0 = 1 + K/Q + K*K
    sb = [(Vh + Vb*K/Q + K*K)/a0, 2*(K*K - Vh)/a0, (Vh - Vb*K/Q + K*K)/a0]
    sa = [1.0, 2*(K*K - 1)/a0, (1 - K/Q + K*K)/a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi*f0/fs)
    d = 1 + K/Q + K*K
    return sb, sa, [1.0, -2.0, 1.0], [1.0, 2*(K*K - 1)/d, (1 - K/Q + K*K)/d]


def _biquad(x, b, a):
    """rows [R, n] float64 through one biquad from zero state, sample by sample (the rows side by side)"""
    y = np.empty_like(x)
    x1 = x2 = y1 = y2 = np.zeros(x.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(x.shape[1]):
            x0 = x[:, n]
            y0 = b[0]*x0 + b[1]*x1 + b[2]*x2 - a[1]*y1 - a[2]*y2
            y[:, n] = y0
            x2, x1, y2, y1 = x1, x0, y1, y0
    return y


def k_weight(x, fs):
    sb, sa, hb, ha = k_coefficients(fs)
    return _biquad(_biquad(np.asarray(x, np.float64), sb, sa), hb, ha)


def mirror(x, fs, weights=None, target=-23.0):
    """x [C, N] of one clip -> dict: z (block powers), blocks / gated (the counts past the absolute gate / past both), Z, lufs, gain (float32)"""
    x = np.asarray(x, np.float64)
    Cn, N = x.shape
    w = np.ones(Cn) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    h = hop(fs)
    nb = (N - 4*h)//h + 1 if N >= 4*h else 0
    y = k_weight(x, fs)
    with np.errstate(invalid="ignore", over="ignore"):
        z = np.array([sum(w[c]*float(np.sum(y[c, i*h:i*h + 4*h]**2)) for c in range(Cn))/(4*h) for i in range(nb)], np.float64)
        first = z > ABS_GATE
        rel = 0.1*z[first].mean() if first.any() else 0.0
        both = first & (z > rel)
        Z = float(z[both].mean()) if both.any() else 0.0
    defined = bool(both.any()) and Z > 0 and math.isfinite(Z)
    P = 10**((target + 0.691)/10)
    return dict(z=z, blocks=int(first.sum()), gated=int(both.sum()), Z=Z, rel=rel, defined=defined,
                lufs=-0.691 + 10*math.log10(Z) if defined else -math.inf, gain=np.float32(math.sqrt(P/Z)) if defined else np.float32(1.0))


def gates_clear(m):
    """no block of a mirror result within GATE_CLEARANCE (relative) of either gate"""
    z = m["z"][np.isfinite(m["z"])]
    for gate in (ABS_GATE, m["rel"]):
        if gate > 0 and z.size and np.min(np.abs(z/gate - 1)) < GATE_CLEARANCE:
            return False
    return True


def ulps32(a, b):
    """the distance of two positive finite float32 in units of the last place"""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def close(got, want):
    """|got/want - 1| <= TOL, elementwise; equal where want is 0, both NaN where it is NaN.  The largest deviation goes to worst_seen"""
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    ok = True
    for g, w in zip(got[~nan], want[~nan]):
        if w == 0 or not math.isfinite(w):
            ok = ok and g == w
            continue
        dev = abs(g/w - 1)
        worst_seen["power"] = max(worst_seen["power"], dev)
        ok = ok and dev <= TOL
    return ok


def check_mirror():
    """the mirror against the standard's 48-kHz table and the sine answers of include/smst.h's definition"""
    sb, sa, hb, ha = k_coefficients(48000)
    assert [round(v, 14) for v in sb] == [1.53512485958697, -2.69169618940638, 1.19839281085285], sb
    assert [round(v, 14) for v in sa[1:]] == [-1.69065929318241, 0.73248077421585], sa
    assert [round(v, 14) for v in ha[1:]] == [-1.99004745483398, 0.99007225036621] and hb == [1.0, -2.0, 1.0], ha
    sine = lambda fs: np.sin(2*np.pi*997*np.arange(fs)/fs)[None, :]
    m = mirror(sine(48000), 48000)
    assert abs(m["lufs"] + 3.0102) < 5e-5 and (len(m["z"]), m["blocks"], m["gated"]) == (7, 7, 7), m
    assert abs(mirror(sine(44100), 44100)["lufs"] + 3.0074) < 5e-5
    assert abs(mirror(sine(8000), 8000)["lufs"] + 2.9960) < 5e-5
    x = sine(48000)
    x[:, 24000:] *= 0.01
    m = mirror(x, 48000)
    assert abs(m["lufs"] + 4.5593) < 5e-5 and (len(m["z"]), m["blocks"], m["gated"]) == (7, 7, 5), m
    assert mirror(np.zeros((2, 1000)), 8000)["lufs"] == -math.inf and mirror(np.zeros((1, 5000)), 8000)["gain"] == 1.0


# ---- 1. the measurement hook against the mirror ----------------------------------------------------------------------------------------

WEIGHTS = {1: (1.41,), 2: (1.0, 1.41), 3: (1.0, 0.0, 1.41), 16: (1.0, 1.41, 0.0, 1.0)*4}
JOINS = (0, 1, CHUNK - 1, CHUNK + 1, 1003, 2*CHUNK, 3, 10**9)          # where segment 1 begins in the clip (clamped to its length: segment 1 empty)
SRC_OFFSETS = (1, 3, 0, 5, 511, 513, 4, 7)


def hook_lengths(fs):
    """4h - 1 (no block), 4h, 5h - 1, 5h, one chunk, a multiple of the chunk +-1 that is past 4h, and about 12000 frames"""
    h = hop(fs)
    k = -(-4*h//CHUNK) + 3
    return (4*h - 1, 4*h, 5*h - 1, 5*h, CHUNK, k*CHUNK - 1, k*CHUNK + 1, 12001)


def _clip(rng, Cn, n, stream):
    """noise and a tone, another level per stream and channel"""
    t = np.arange(n)
    x = rng.uniform(-1, 1, (Cn, n))*(0.05 + 0.04*stream) + 0.2*np.sin(2*np.pi*(0.011 + 0.003*stream)*t)[None, :]
    return (x*(1 + 0.1*np.arange(Cn))[:, None]).astype(np.float32)


def build_image(clips, joins, offsets, base_offset=1):
    """the clips [C, n_s] as the two segments of an image with rows at odd float offsets, 7.0 around them -> (image, segments, stream stride, channel stride)"""
    S, Cn = len(clips), clips[0].shape[0]
    segs = np.zeros((S, 2, 4), np.int32)
    for s, x in enumerate(clips):
        n0 = min(joins[s], x.shape[1])
        segs[s, 0] = (offsets[s], 0, n0, 0)
        segs[s, 1] = (offsets[s] + n0 + 5, n0, x.shape[1] - n0, 0)           # (the image has a gap between the two)
    end = int((segs[:, :, 0] + segs[:, :, 2]).max())
    ics = end + 3
    iss = Cn*ics + 5
    image = pc.aligned((S - 1)*iss + (Cn - 1)*ics + end, np.float32, base_offset)
    image[:] = 7.0
    for s, x in enumerate(clips):
        n0 = int(segs[s, 0, 2])
        for c in range(Cn):
            image[s*iss + c*ics + segs[s, 0, 0] + np.arange(n0)] = x[c, :n0]
            image[s*iss + c*ics + segs[s, 1, 0] + np.arange(x.shape[1] - n0)] = x[c, n0:]
    return image, segs, iss, ics


def compare_hook(lib, clips, fs, weights, target, joins, offsets, base_offset=1):
    """the hook on the clips' image against the mirror of every clip -> (the mirrors, the hook's results)"""
    pkg = package()
    S, Cn = len(clips), clips[0].shape[0]
    rates = np.broadcast_to(np.asarray(fs, np.float64), (S,))
    mirrors = [mirror(x, rates[s], weights, target) for s, x in enumerate(clips)]
    assert all(gates_clear(m) for m in mirrors), "a block lies on a gate: change the input"
    image, segs, iss, ics = build_image(clips, joins, offsets, base_offset)
    most = max(max(len(m["z"]) for m in mirrors), 1)
    before = pkg.launch_count("clip_loudness", lib)
    Z, blocks, gated, gains, powers = pkg.debug_clip_loudness(segs, Cn, image, iss, ics, rates, weights, target, most, lib=lib)
    assert pkg.launch_count("clip_loudness", lib) == before + 1
    for s, m in enumerate(mirrors):
        where = dict(stream=s, fs=float(rates[s]), C=Cn, n=clips[s].shape[1], join=int(segs[s, 0, 2]))
        assert (int(blocks[s]), int(gated[s])) == (m["blocks"], m["gated"]), (where, int(blocks[s]), int(gated[s]), m["blocks"], m["gated"])
        assert close(powers[s, :len(m["z"])], m["z"]), (where, powers[s, :len(m["z"])].tolist(), m["z"].tolist())
        assert close(Z[s], m["Z"]), (where, float(Z[s]), m["Z"])
        assert gains.dtype == np.float32 and ulps32(gains[s], m["gain"]) <= 1, (where, float(gains[s]), float(m["gain"]))
        if not m["defined"]:
            assert gains[s] == 1.0 and Z[s] == 0.0
    return mirrors, (Z, blocks, gated, gains, powers)


def check_hook(lib, fs, channels):
    """the four passes through smst_debug_clip_loudness against the mirror: eight streams of the lengths of hook_lengths, their joins at 0
    (segment 0 empty), 1, chunk +- 1, a position that is no multiple of 4, two chunks, 3 and the clip's end (segment 1 empty); rows at odd
    float offsets, the image itself one float behind a 16-byte boundary; weights that include 0 and 1.41"""
    rng = pc._rng(9201, int(fs), channels)
    lengths = hook_lengths(fs)
    clips = [_clip(rng, channels, n, s) for s, n in enumerate(lengths)]
    mirrors, _ = compare_hook(lib, clips, fs, WEIGHTS[channels], -23.0, JOINS, SRC_OFFSETS)
    h = hop(fs)
    assert [len(m["z"]) for m in mirrors[:5]] == [0, 1, 1, 2, 0] and len(mirrors[-1]["z"]) == (12001 - 4*h)//h + 1
    assert not mirrors[0]["defined"] and all(m["defined"] for m in mirrors[1:4])
    print("largest |z/z_mirror - 1| so far: %.3g" % worst_seen["power"])


def content_clips(fs, Cn=2):
    """-> the clips of check_content: loud then -40 dB; a stretch at 1e-4; silence; a NaN in the first 100 ms; a NaN in the middle"""
    n = 10*hop(fs)
    rng = pc._rng(9202, int(fs))
    loud = lambda: (rng.uniform(-0.3, 0.3, (Cn, n))).astype(np.float32)
    a = loud()
    a[:, 6*n//10:] *= np.float32(0.01)
    b = loud()
    b[:, n//4:n//4 + 5*hop(fs)] = rng.uniform(-1e-4, 1e-4, (Cn, 5*hop(fs))).astype(np.float32)
    c = np.zeros((Cn, n), np.float32)
    d = loud()
    d[1, 5] = np.nan
    e = loud()
    e[0, n//2 + 17] = np.nan
    return [a, b, c, d, e]


def check_content(lib, fs=8000):
    """what the gates and the undefined cases are for: the relative gate drops the blocks of the quiet part, the absolute gate those of the
    stretch at 1e-4, silence and a clip with a NaN in its first 100 ms have no loudness (gL = 1), a NaN further on leaves the blocks in
    front of it"""
    clips = content_clips(fs)
    mirrors, (Z, blocks, gated, gains, powers) = compare_hook(lib, clips, fs, None, -16.0, (1003, 0, 5, 257, 2), SRC_OFFSETS)
    a, b, c, d, e = mirrors
    assert a["blocks"] == len(a["z"]) and 0 < a["gated"] < a["blocks"]
    assert 0 < b["blocks"] < len(b["z"]) and b["gated"] == b["blocks"]
    assert not c["defined"] and c["blocks"] == 0 and not c["z"].any()
    assert not d["defined"] and np.isnan(d["z"]).all() and gains[3] == 1.0
    assert e["defined"] and 0 < e["gated"] < len(e["z"]) and np.isnan(e["z"][-1])


def check_reproducible(lib, fs=8000):
    """two runs of the hook give the same bits"""
    pkg = package()
    clips = content_clips(fs)[:2] + [_clip(pc._rng(9203), 2, 12001, 1)]
    image, segs, iss, ics = build_image(clips, (1003, 0, 257), SRC_OFFSETS)
    runs = [pkg.debug_clip_loudness(segs, 2, image, iss, ics, fs, (1.0, 1.41), -23.0, 12, lib=lib) for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert runs[0][2].min() > 0


# ---- 2. whole clips through smst_batch_exact_pcm ---------------------------------------------------------------------------------------

NORMALISE, FIXED = lc.NORMALISE, lc.FIXED
BITING = 3                                                                # the stream whose target is so high that the ceiling decides
#  per call: (mode per stream of exact_cases.CLIPS, the stream left out or None)
CLIP_CALLS = (((LOUDNESS,)*5, None), ((LOUDNESS, NORMALISE, LOUDNESS, LOUDNESS, FIXED), 0))
CLIP_TARGETS = (-23.0, -16.0, -14.0, 6.0, -18.5)
CLIP_SEED = 31


def check_clips(lib, fmt, fs, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """exactFrames of exact_cases.CLIPS (outputs of 7500, 5000, 300 -- too short --, 5000 and 4000 frames: 6, 3, 3 and 2 blocks at 8 kHz; at
    12 kHz the last clip has none) with the loudness mode on every stream, then mixed with NORMALISE and FIXED and one stream left out.
    The reported loudness and counts are the mirror's of smst_batch_exact's planar output; the gain is the mirror's within an ulp, or
    ceiling/peak exactly where the ceiling bites (stream 3: zero overs at the clip-free ceiling); the bytes are exactly level_cases.mirror
    of the planar output at the gain the device reported; the short clip is undithered zeros, the left-out clip untouched."""
    pkg = package()
    nin, nout, short = xc.CLIPS["inputs"], xc.CLIPS["outputs"], xc.CLIPS["short"]
    S, Cn, most = len(nin), 2, max(nout)
    dithered = fmt in dc.DITHERED_FORMATS
    frames = fc.encode_frames(pc.frames_of(xc.clip_inputs(Cn, nin, loud=0)), fmt)
    planar = np.ascontiguousarray(np.transpose(fc.decode_frames(frames, fmt), (0, 2, 1)))
    p, f = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(2))
    ceil = lc.ceiling(fmt, dithered)
    weights = (1.0, 1.41)
    f.set_pcm_loudness_weights(weights)
    modes = [dc.CLIP_MODES[s] if dithered else dc.NONE for s in range(S)]
    if dithered:
        for s in range(S):
            f.setPcmDither(modes[s], CLIP_SEED + s, stream=s)
    h = hop(fs)
    want_g = np.ones(S, np.float32)
    for call, (levels, left) in enumerate(CLIP_CALLS):
        n_out = [(-1 if s == left else n) for s, n in enumerate(nout)]
        for s in range(S):
            if levels[s] == LOUDNESS:
                f.set_pcm_loudness(CLIP_TARGETS[s], ceil, fs, stream=s)
                assert f.pcm_level(s) == (LOUDNESS, 1.0, float(ceil)) and f.pcm_loudness(s) == (CLIP_TARGETS[s], float(fs))
            else:
                f.set_pcm_level(levels[s], 0.5, ceil, stream=s)
        want, ok_p = p.exact(planar, n_out, in_samples=nin)
        want = np.array(want, copy=True)
        out = np.full(frames.shape[:1] + (most,) + frames.shape[2:], 0x5A, frames.dtype)
        before = [pkg.launch_count(k, lib) for k in ("clip_loudness", "clip_peak", "clip_out_levelled")]
        got, ok_f = f.exactFrames(to_memory(frames), n_out, in_samples=nin, out=to_memory(out))
        got = to_host(got)
        assert [pkg.launch_count(k, lib) - n for k, n in zip(("clip_loudness", "clip_peak", "clip_out_levelled"), before)] == [1, 1, 1]
        assert ok_p.tolist() == ok_f.tolist() == [s not in (short, left) for s in range(S)]
        lufs, blocks, gated = f.take_pcm_loudness()
        peaks, gains = f.take_pcm_peaks()
        overs = f.takePcmOvers()[0]
        expect = out.copy()
        for s in range(S):
            where = dict(fmt=fmt, fs=fs, call=call, stream=s)
            if s == left:
                assert lufs[s] == -math.inf and (blocks[s], gated[s]) == (0, 0) and gains[s] == want_g[s] and peaks[s] == 0, where
                continue
            x = want[s, :, :nout[s]]
            measured = levels[s] == LOUDNESS and s != short
            if measured:
                m = mirror(x, fs, weights, CLIP_TARGETS[s])
                assert gates_clear(m), where
                assert (int(blocks[s]), int(gated[s])) == (m["blocks"], m["gated"]) and len(m["z"]) == ((nout[s] - 4*h)//h + 1 if nout[s] >= 4*h else 0), (where, m)
                assert m["defined"] == (len(m["z"]) > 0) and (lufs[s] == -math.inf) == (not m["defined"]), (where, lufs[s], m)
                if m["defined"]:
                    assert close(10**((lufs[s] + 0.691)/10), m["Z"]), (where, lufs[s], m["lufs"])
                q = lc.gain_of(lc.PROTECT, np.float32(np.inf), ceil, lc.peak_of(x))      # (ceiling/peak)
                if m["gain"] > q and ulps32(m["gain"], q) > 1:
                    assert gains[s] == q and s == BITING, (where, float(gains[s]), float(q))
                else:
                    assert ulps32(gains[s], m["gain"]) <= 1 and s != BITING, (where, float(gains[s]), float(m["gain"]))
            else:
                assert lufs[s] == -math.inf and (blocks[s], gated[s]) == (0, 0), where
                if s != short:
                    assert gains[s] == lc.gain_of(levels[s], 0.5, ceil, lc.peak_of(x)), where
            if s != short:
                assert peaks[s] == lc.peak_of(x), where
                want_g[s] = gains[s]
            else:
                assert gains[s] == want_g[s] and peaks[s] == 0, where
            codes, cm, _ = lc.mirror(x, fmt, gains[s] if s != short else 1.0, dc.NONE if s == short else modes[s], CLIP_SEED + s, 0)
            assert overs[s] == int(cm.sum()) and (s != BITING or not cm.any()), (where, int(overs[s]))
            expect[s, :nout[s]] = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
        assert lc.same_bytes(got.reshape(-1).view(np.uint8), expect.reshape(-1).view(np.uint8), fmt), (fmt, fs, call)
        assert not got[short, :nout[short]].any()
        if left is not None:
            assert (got[left] == 0x5A).all()
        if call == 0 and fs == 8000:
            assert [int(b) for b in blocks] == [6, 3, 0, 3, 2]
        if call == 0 and fs == 12000:
            assert blocks[4] == 0 and gains[4] == 1.0 and lufs[4] == -math.inf
    for b in (p, f):
        b.close()


def run_clips(lib, fs=8000, fmt=fc.S16):
    """the bytes, the meters and the gains of one loudness call on a fresh batch (two runs are bit-identical)"""
    pkg = package()
    nin, nout = xc.CLIPS["inputs"], xc.CLIPS["outputs"]
    frames = fc.encode_frames(pc.frames_of(xc.clip_inputs(2, nin, loud=0)), fmt)
    b = pkg.StretchBatch(len(nin), 2, lib=lib, seed=3, **pc.GEOMETRY)
    b.set_pcm_loudness(-20.0, lc.ceiling(fmt, False), fs)
    out, ok = b.exactFrames(frames, nout, in_samples=nin)
    res = [np.array(out, copy=True), ok] + list(b.take_pcm_loudness()) + list(b.take_pcm_peaks())
    b.close()
    return res


def check_two_runs(lib):
    a, b = run_clips(lib), run_clips(lib)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert a[0].any() and (a[4] > 0).sum() == 4


# ---- 3. opt-in, steady state, refusals -------------------------------------------------------------------------------------------------

def check_opt_in(lib, **memory):
    """a levelled batch without the mode: the whole-clip cases of level_cases.py -- bytes, peaks and gains against their mirror -- launch
    the loudness passes zero times; one stream in the mode, in a call that leaves it out, does not start them either"""
    pkg = package()
    before = pkg.launch_count("clip_loudness", lib)
    assert before >= 0, "the library has no clip_loudness counter"
    lc.check_clips(lib, fc.S16, **memory)
    assert pkg.launch_count("clip_loudness", lib) == before
    nin, nout = xc.CLIPS["inputs"][:3], xc.CLIPS["outputs"][:3]
    frames = fc.encode_frames(pc.frames_of(xc.clip_inputs(2, nin)), fc.S16)
    to_memory = memory.get("to_memory", lambda a: a)
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_level(lc.NORMALISE, 1.0, 0.9)
    b.set_pcm_loudness(-23.0, 0.9, 8000, stream=1)
    for counts, ran in (([7500, -1, 300], 0), (nout, 1)):
        before = pkg.launch_count("clip_loudness", lib)
        b.exactFrames(to_memory(frames), counts, in_samples=nin)
        b.synchronize()
        assert pkg.launch_count("clip_loudness", lib) - before == ran, counts
    lufs, blocks, gated = b.take_pcm_loudness()
    assert lufs[0] == lufs[2] == -math.inf and math.isfinite(lufs[1]) and blocks[1] == 3
    b.close()


def check_steady_state(lib, to_memory=lambda a: a):
    """the first loudness call grows the scratch (workspace bytes), a second call of the same shapes allocates nothing, nor do the takes"""
    pkg = package()
    nin, nout = xc.CLIPS["inputs"][:3], xc.CLIPS["outputs"][:3]
    clips = to_memory(fc.encode_frames(pc.frames_of(xc.clip_inputs(2, nin)), fc.S16))
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_level(lc.NORMALISE, 1.0, 0.9)
    for _ in range(2):
        b.exactFrames(clips, nout, in_samples=nin)
    b.synchronize()
    plain = b.workspaceBytes()
    b.set_pcm_loudness(-23.0, 0.9, 8000)
    assert b.take_pcm_loudness()[0].tolist() == [-math.inf]*3                  # (nothing has measured yet)
    for _ in range(2):
        b.exactFrames(clips, nout, in_samples=nin)
    b.synchronize()
    events, grown = b.allocation_events(), b.workspaceBytes()
    assert grown > plain
    b.exactFrames(clips, nout, in_samples=nin)
    lufs, blocks, gated = b.take_pcm_loudness()
    b.take_pcm_peaks()
    assert b.allocation_events() == events and b.workspaceBytes() == grown and math.isfinite(lufs[0]) and blocks[0] == 6
    b.close()


def check_refusals(lib):
    pkg = package()
    b = pkg.StretchBatch(2, 3, lib=lib, **pc.GEOMETRY)
    inf, nan = float("inf"), float("nan")
    bad = [((0, inf, 1.0, 8000.0), b"target"), ((0, nan, 1.0, 8000.0), b"target"), ((0, -23.0, 1.0, inf), b"rate"), ((0, -23.0, 1.0, nan), b"rate"),
           ((0, -23.0, 1.0, 0.0), b"rate"), ((0, -23.0, 1.0, -48000.0), b"rate"), ((0, -23.0, 1.0, 10.0*CHUNK - 6), b"rate"),
           ((0, -23.0, 0.0, 8000.0), b"ceiling"), ((0, -23.0, -1.0, 8000.0), b"ceiling"), ((0, -23.0, nan, 8000.0), b"ceiling"),
           ((2, -23.0, 1.0, 8000.0), b"stream"), ((-2, -23.0, 1.0, 8000.0), b"stream")]
    for args, word in bad:
        assert lib.smst_batch_set_pcm_loudness(b.h, *args) == -1 and word in lib.smst_last_error(), (args, lib.smst_last_error())
    assert [b.pcm_level(s) for s in range(2)] == [(lc.FIXED, 1.0, 1.0)]*2       # (a refused call changes nothing)
    for w in ((1.0, -0.5, 1.0), (1.0, nan, 1.0), (inf, 1.0, 1.0)):
        with dc.pytest_raises(pkg.StretchError) as e:
            b.set_pcm_loudness_weights(w)
        assert "weight" in str(e.value)
    assert lib.smst_batch_set_pcm_loudness(None, 0, -23.0, 1.0, 8000.0) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_loudness(None, 0, None, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_set_pcm_loudness_weights(None, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_take_pcm_loudness(None, None, None, None) == -1 and b"null" in lib.smst_last_error()
    for stream in (-1, 2):
        assert lib.smst_batch_pcm_loudness(b.h, stream, None, None) == -1 and b"stream" in lib.smst_last_error()
    assert lib.smst_batch_pcm_loudness(b.h, 0, None, None) == -1 and b"LOUDNESS" in lib.smst_last_error()
    assert lib.smst_batch_set_pcm_level(b.h, 0, LOUDNESS, 1.0, 1.0) == -1 and b"mode" in lib.smst_last_error()
    # what is allowed: a ceiling of +inf, the lowest rate with h = CHUNK, null pointers in the getters, weights reset by null
    b.set_pcm_loudness(-14.0, inf, 10.0*CHUNK - 5, stream=1)
    b.set_pcm_loudness_weights((1.0, 0.0, 1.41))
    b.set_pcm_loudness_weights(None)
    assert b.pcm_level(1) == (LOUDNESS, 1.0, inf) and b.pcm_loudness(1) == (-14.0, 10.0*CHUNK - 5) and b.pcm_level(0)[0] == lc.FIXED
    assert lib.smst_batch_pcm_loudness(b.h, 1, None, None) == 0 and lib.smst_batch_take_pcm_loudness(b.h, None, None, None) == 0
    b.set_pcm_level(lc.FIXED, 1.0, stream=1)
    assert b.pcm_level(1)[0] == lc.FIXED
    assert (pkg.LEVEL_LOUDNESS, pkg.LOUDNESS_CHUNK) == (LOUDNESS, CHUNK)
    b.close()


def check_refused_in_streaming_calls(lib, **memory):
    """a stream in the loudness mode makes processFrames and flushFrames fail before anything runs, as the other whole-clip modes do"""
    pkg = package()
    frames, _ = dc.session_inputs(fc.S16)
    to_memory = memory.get("to_memory", lambda a: a)
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_loudness(-23.0, 0.9, 8000, stream=1)
    x = to_memory(np.ascontiguousarray(frames[:, :600]))
    for call in (lambda: b.processFrames(x, [600, 300, 0]), lambda: b.flushFrames([100, 50, -1], like=to_memory(np.zeros((1,), np.float32)))):
        with dc.pytest_raises(pkg.StretchError) as e:
            call()
        assert "whole-clip" in str(e.value) and "error -1" in str(e.value), str(e.value)
    b.flushFrames([100, -1, 100], like=to_memory(np.zeros((1,), np.float32)))     # (stream 1 takes no part: not refused)
    b.close()


# ---- 4. the command-line tool ----------------------------------------------------------------------------------------------------------

def loudness_lines(stdout):
    """the "level:" lines of a --loudness run -> [(file, lufs, peak, gain, overs)]"""
    found = re.findall(r"^level: (\S+) loudness=(\S+) peak=(\S+) gain=(\S+) overs=(-?\d+)$", stdout, re.M)
    return [(name, float(lufs), np.float32(peak), np.float32(gain), int(overs)) for name, lufs, peak, gain, overs in found]


def check_cli(cli, tmp_path):
    """--loudness=LUFS renders through the exact path at the WAV header's rate: the printed loudness is the mirror's of the --exact floats
    (to the printed digits), the gain the mirror's or -- with --protect as the ceiling -- ceiling/peak, and the file is level_cases.mirror
    of those floats at the printed gain; --loudness with --normalize is refused"""
    from test_cli import write_wav16
    sr, lengths = 8000, (6001, 7000)
    srcs = [str(tmp_path/("in%d.wav" % k)) for k in range(2)]
    write_wav16(srcs[0], 0.9*synth_input(1, 2, lengths[0], sr), sr)
    write_wav16(srcs[1], 0.2*synth_input(3, 2, lengths[1], sr), sr)

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
    db = -1.0
    for name, flags, fmt, mode, target, ceil in (("loud", ["--loudness=-20", "--out-format=s24"], fc.S24, dc.NONE, -20.0, None),
                                                 ("both", ["--loudness=-3", "--protect=%g" % db, "--out-format=s16", "--dither=tpdf"], fc.S16, dc.TPDF, -3.0, 10**(db/20))):
        outs, res = run(name, flags)
        lines = loudness_lines(res.stdout)
        assert len(lines) == 2, res.stdout
        limited = 0
        for k, (path, lufs, peak, gain, overs) in enumerate(lines):
            m = mirror(floats[k], sr, None, target)
            assert path == outs[k] and m["defined"] and gates_clear(m) and abs(lufs - m["lufs"]) <= 5.1e-5 and peak == lc.peak_of(floats[k]), (name, k, lufs, m["lufs"])
            q = float(ceil)/float(peak) if ceil else math.inf
            if float(m["gain"]) > q*(1 + 1e-6):
                limited += 1
                assert abs(float(gain) - q) <= 1e-6*q, (name, k, float(gain), q)
            else:
                assert abs(float(gain) - float(m["gain"])) <= 1e-6*float(m["gain"]), (name, k, float(gain), float(m["gain"]))
            head, data = dc.data_chunk(path)
            esz = fc.ELEM_BYTES[fmt]
            assert head == (1, 2, sr, sr*2*esz, 2*esz, 8*esz)
            codes, cm, _ = lc.mirror(floats[k], fmt, gain, mode, k, 0)
            assert np.array_equal(np.frombuffer(data, np.uint8), fc.to_rows(codes.reshape(-1), fmt).reshape(-1)) and overs == int(cm.sum()), (name, k)
        assert limited == (1 if ceil else 0), (name, lines)
    _, res = run("bad", ["--loudness=-20", "--normalize=-1"], expect=2)
    assert "exclude" in res.stderr
