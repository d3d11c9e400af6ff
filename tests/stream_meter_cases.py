"""The stream meter of the frame output (include/smst.h, "Stream meter"): what test_stream_meter_emu.py and test_stream_meter_gpu.py share.

The contract is an equality of bit patterns: after any sequence of calls the readings are what smst_debug_clip_loudness_range (and
smst_debug_clip_loudness, for Z and its counts) and smst_debug_clip_true_peak report of the clip v[0, Tm) -- the same operations in the same
order, so the tolerance is zero.  Every comparison below is one of bit patterns but those of check_against_mirrors, which holds one case
against the float64 numpy mirrors of loudness_cases, loudness_range_cases and true_peak_cases at those files' own tolerances.

Rates.  The base programme the feature was specified with has fs = 2570 (h = 257: chunks of 256 straddle sub-blocks at every offset).  At
that rate the K-weighting shelf's centre lies above the Nyquist frequency and its biquad is unstable (loudness_range_cases.LOWEST_FS has
the story): every power is inf or NaN, in the clip meters and here, so the comparison holds the bits of the overflow and the counts, and the
true peak.  The same programme therefore also runs at fs = 4010 (h = 401, odd as well, and the shelf is stable): there the relative gates
and both percentiles discriminate."""
import ctypes as C
import math

import numpy as np

import dither_cases as dc
import level_cases as lc
import loudness_cases as ld
import loudness_range_cases as lr
import pcm_cases as pc
import pcm_format_cases as fc
import true_peak_cases as tp
from conftest import package

FS, H = 2570.0, 257                                  # the base programme's rate: h = 257
FS_STABLE, H_STABLE = 4010.0, 401                    # ... and a rate at which the K-weighting is stable
CHUNK = ld.CHUNK
SUBS = 60                                            # sub-blocks of the base programme
LEVELS = (0.3, 0.1, 0.2, 0.003, 0.001, 0.002)        # its level steps, one per 10 sub-blocks: the last 3 s lie 40 dB below the first
STREAM_LEVELS = (1.0, 0.5, 0.25)
WEIGHTS = ld.WEIGHTS
COUNTERS = ("pcm_stream_meter", "pcm_stream_meter_read", "pcm_stream_meter_scan")
SCAN_FRAMES = 2048                                   # a call whose longest metered count reaches this takes the chunk-scan form (kStreamMeterScanFrames)
FORMS = (0, 1, 2)
KEYS = ("Z", "blocks", "gated", "M", "ST", "lo", "hi", "ns", "n", "true_peaks", "sample_peaks")
compared = dict(readings=0)

_programmes, _references = {}, {}


def hop(fs):
    return int(np.floor(fs/10 + 0.5))


def programme(fs, Cn, subs=SUBS, S=3):
    """seeded noise [S, Cn, subs*h] float32 with a level step every 10 sub-blocks; a case of C channels takes the first C of 16"""
    key = (fs, subs, S)
    if key not in _programmes:
        h = hop(fs)
        rng = pc._rng(9501, int(fs) + subs)
        x = rng.uniform(-1.0, 1.0, (S, 16, subs*h))
        env = np.repeat([LEVELS[(j//10) % len(LEVELS)] for j in range(subs)], h)
        _programmes[key] = np.ascontiguousarray((x*env[None, None, :]*np.array(STREAM_LEVELS[:S])[:, None, None]).astype(np.float32))
    return np.ascontiguousarray(_programmes[key][:, :Cn])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def clip_reference(lib, image, lengths, fs, weights=None, max_blocks=SUBS):
    """the clip meters of v[0, lengths[s]) of every stream of image [S, C, n] -> a dict with KEYS and block_powers, short_powers"""
    pkg = package()
    S, Cn, n = image.shape
    lengths = [int(v) for v in lengths]
    key = (id(lib), image.ctypes.data, image.shape, tuple(lengths), fs, None if weights is None else tuple(weights), max_blocks)
    if key in _references and _references[key][0] is image:
        return _references[key][1]
    segs = np.zeros((S, 2, 4), np.int32)
    segs[:, 0, 2] = lengths
    Z, blocks, gated, _, zp = pkg.debug_clip_loudness(segs, Cn, image, Cn*n, n, fs, weights, max_blocks=max_blocks, lib=lib)
    M, ST, lo, hi, ns, nn, _, sp = pkg.debug_clip_loudness_range(segs, Cn, image, Cn*n, n, fs, weights, max_blocks=max_blocks, lib=lib)
    true_peaks, sample_peaks = pkg.debug_clip_true_peak(segs, Cn, image, Cn*n, n, lib=lib)
    ref = dict(Z=Z, blocks=blocks, gated=gated, M=M, ST=ST, lo=lo, hi=hi, ns=ns, n=nn, true_peaks=true_peaks, sample_peaks=sample_peaks,
               block_powers=zp, short_powers=sp, nb=np.array([v//hop(fs) - 3 if v >= 4*hop(fs) else 0 for v in lengths]))
    _references[key] = (image, ref)                                              # (the image is kept: its address names the entry)
    return ref


def run(lib, image, counts, fs, max_sub=SUBS, weights=None, flags=None, read_after=None, form=0, max_blocks=SUBS):
    pkg = package()
    S, Cn, n = image.shape
    return pkg.debug_pcm_stream_meter(counts, Cn, image, Cn*n, n, [fs]*S, max_sub, weights, flags, read_after, form, max_blocks, lib=lib)


def assert_reading(got, r, ref, where, last=True):
    """reading r of a hook result against a clip reference, every value bit for bit"""
    for k in KEYS:
        assert same_bits(got[k][r], ref[k]), (where, "reading", r, k, got[k][r].tolist(), ref[k].tolist())
    if last:
        for k in ("block_powers", "short_powers"):
            assert same_bits(got[k], ref[k]), (where, k)
    compared["readings"] += 1


def totals(counts):
    return np.maximum(np.asarray(counts, np.int64), 0).sum(axis=0)


# ---- the cuts ----------------------------------------------------------------------------------------------------------------------------

def _stack(per_stream, fill=-1):
    """per-stream lists of counts -> [calls, S], a stream that has run out takes no part (fill)"""
    calls = max(len(c) for c in per_stream)
    return np.array([[c[k] if k < len(c) else fill for c in per_stream] for k in range(calls)], np.int32)


def _cut_at(points, n):
    points = sorted(set(p for p in points if 0 < p < n)) + [n]
    return [b - a for a, b in zip([0] + points[:-1], points)]


def cuts(kind, n, h, S=3):
    """the programme of n frames per stream cut into calls -> counts [calls, S]"""
    rng = pc._rng(9502, n + len(kind))
    if kind == "one":
        per = [[n]]*S
    elif kind == "ones_then_large":                                              # calls of 1 frame for the first 600 frames
        per = [[1]*600 + _cut_at(range(1000, n, 1000), n - 600)]*S
    elif kind == "short":                                                        # 5 ... 10 frames: shorter than the 11 carried frames
        head = []
        while sum(head) < 6*h + 40:                                              # (past the first chunks, sub-blocks and the first block)
            head.append(int(rng.integers(5, 11)))
        per = [head + _cut_at(range(999, n, 999), n - sum(head))]*S
    elif kind == "chunk":
        per = [_cut_at(range(CHUNK, n, CHUNK), n)]*S
    elif kind == "hop":
        per = [_cut_at(range(h, n, h), n)]*S
    elif kind == "edges":                                                        # calls that end exactly on chunk edges and on sub-block edges
        per = [_cut_at([CHUNK*k for k in range(1, 25)] + [h*k for k in range(1, 25)] + [CHUNK*h], n)]*S
    elif kind == "random":
        per = [_cut_at(np.cumsum(rng.integers(1, 3000, 64)).tolist(), n)]*S
    elif kind == "sits_out":                                                     # stream 1 sits out every other call, stream 2 has calls of 0
        a = _cut_at(range(700, n, 700), n)
        b, c = [], []
        for k, v in enumerate(_cut_at(range(1100, n, 1100), n)):
            b += [v, -1]
            c += [v, 0] if k % 3 else [0, v]
        per = [a, b, c][:S]
    elif kind == "ragged":
        per = [_cut_at(np.cumsum(rng.integers(1, 2500 + 900*s, 96)).tolist(), n) for s in range(S)]
    else:
        raise ValueError(kind)
    counts = _stack(per)
    assert (totals(counts) == n).all(), (kind, totals(counts).tolist())
    return counts


CUTS = ("one", "ones_then_large", "short", "chunk", "hop", "edges", "random", "sits_out", "ragged")


def check_cut(lib, fs, Cn, kind, weights=None, forms=FORMS):
    """the base programme in one cut, every form: the reading after the last call is the clip meters' of the whole programme"""
    pkg = package()
    image = programme(fs, Cn)
    n = image.shape[2]
    ref = clip_reference(lib, image, [n]*3, fs, weights)
    counts = cuts(kind, n, hop(fs))
    for form in forms:
        before = [pkg.launch_count(k, lib) for k in COUNTERS]
        assert min(before) >= 0, "the library has no stream meter counters"
        got = run(lib, image, counts, fs, weights=weights, form=form)
        moved = [pkg.launch_count(k, lib) - b for k, b in zip(COUNTERS, before)]
        launches = [int(c.max()) for c in counts if c.max() > 0]
        scans = sum(1 for c in launches if form == 2 or (form == 0 and c >= SCAN_FRAMES))
        assert moved == [len(launches), 1, scans], (kind, form, moved)               # (... so both forms really ran)
        assert got["metered"][0].tolist() == [n]*3
        assert_reading(got, 0, ref, dict(fs=fs, C=Cn, cut=kind, form=form))
    return ref


def check_discriminates(lib):
    """the stable rate's programme: blocks fail the relative gate, short-term powers fail theirs, and the percentiles differ"""
    image = programme(FS_STABLE, 2)
    ref = clip_reference(lib, image, [image.shape[2]]*3, FS_STABLE)
    for s in range(3):
        assert 0 < ref["gated"][s] < ref["blocks"][s] <= SUBS - 3, (ref["gated"].tolist(), ref["blocks"].tolist())
        assert 0 < ref["n"][s] < ref["ns"][s] == SUBS - 29 and 0 < ref["lo"][s] < ref["hi"][s] < ref["ST"][s] <= ref["M"][s], {k: ref[k].tolist() for k in KEYS}
        assert np.isfinite(ref["block_powers"][s, :SUBS - 3]).all() and ref["true_peaks"][s] >= ref["sample_peaks"][s] > 0


def check_mid_readings(lib, fs, Cn, form=0):
    """readings after several calls: T = 0, T < 12, T < 4h (no block), 4h <= T < 30h (no short-term power), then further on; reading r is the
    clip meters' of v[0, T_r), and the last one is what a run without the earlier readings gives"""
    image = programme(fs, Cn)
    n, h = image.shape[2], hop(fs)
    per = [[0, 7, 3*h, 2*h + 5, 26*h, 13, n - 31*h - 25], [0, 11, 4*h - 12, 9, 29*h, h - 8, n - 34*h], [-1, 5, h, 0, 31*h, -1, n - 32*h - 5]]
    counts = _stack(per)
    assert (totals(counts) == n).all()
    after = np.ones(len(counts), np.int32)
    got = run(lib, image, counts, fs, read_after=after, form=form)
    done = np.zeros(3, np.int64)
    for r in range(len(counts)):
        done += np.maximum(counts[r], 0)
        ref = clip_reference(lib, image, done, fs)
        assert got["metered"][r].tolist() == done.tolist()
        assert_reading(got, r, ref, dict(fs=fs, C=Cn, reading=r, T=done.tolist()), last=r + 1 == len(counts))
    assert got["blocks"][0].tolist() == [0, 0, 0] and got["ns"][3].tolist() == [0, 0, 0] and got["ns"][4].min() > 0
    plain = run(lib, image, counts, fs, form=form)
    for k in KEYS + ("block_powers", "short_powers"):
        assert same_bits(plain[k][0] if k in KEYS else plain[k], got[k][-1] if k in KEYS else got[k]), k


def edge_programme():
    """mono: quiet noise under an alternation that fades in slowly and reaches full scale where the clip ends -- the last windows, closed
    against zeros, overshoot --, then 12 more frames in which the alternation goes on and fades out gently"""
    rng = pc._rng(9503, 1)
    n = 700
    ramp = np.concatenate([np.zeros(n - 300), 0.5 - 0.5*np.cos(np.pi*np.arange(280)/280), np.ones(20)])
    x = (0.01*rng.uniform(-1, 1, n) + ramp*(-1.0)**np.arange(n)).clip(-1, 1).astype(np.float32)
    x[-20:] = (-1.0)**np.arange(n - 20, n)
    more = np.array([(-1.0)**(n + k)*a for k, a in enumerate([1, 1, 0.98, 0.93, 0.85, 0.73, 0.59, 0.43, 0.28, 0.15, 0.06, 0.01])], np.float32)
    return np.ascontiguousarray(np.concatenate([x, more])[None, None, :]), n


def check_true_peak_edge(lib, form=0):
    """the largest interpolated value lies in the last six windows against zeros: a reading there shows it; 12 frames later the reading is the
    longer clip's, which is LOWER -- the edge was not folded in"""
    image, n = edge_programme()
    total = image.shape[2]
    for counts in ([[n], [12]], [[n - 3], [3], [5], [7]], [[1]]*total):
        counts = np.array(counts, np.int32)
        after = np.zeros(len(counts), np.int32)
        after[np.flatnonzero(np.cumsum(counts[:, 0]) == n)[0]] = after[-1] = 1
        got = run(lib, image, counts, FS, read_after=after, form=form)
        for r, T in enumerate((n, total)):
            assert_reading(got, r, clip_reference(lib, image, [T], FS), dict(edge=T, calls=len(counts)), last=r == 1)
        first, second = float(got["true_peaks"][0, 0]), float(got["true_peaks"][1, 0])
        assert first > 1.1 and second < first and second >= 1.0 and got["sample_peaks"][:, 0].tolist() == [1.0, 1.0], (first, second)


def check_capacity(lib, form=0):
    """maxSubBlocks = 20 is fed 30 sub-blocks: the meter freezes at 20*257 frames, true peak too, and no call fails"""
    image = programme(FS, 2, subs=30)
    image[0, 0, 21*H + 5] = 3.0                                                  # (a peak behind the capacity: not metered)
    n = image.shape[2]
    for kind in ("random", "hop"):
        counts = cuts(kind, n, H)
        got = run(lib, image, counts, FS, max_sub=20, form=form)
        assert got["metered"][0].tolist() == [20*H]*3
        ref = clip_reference(lib, image, [20*H]*3, FS)
        assert_reading(got, 0, ref, dict(capacity=kind))
        assert got["sample_peaks"][0, 0] < 3.0


def check_nan_inf(lib, fs, form=0):
    """a NaN mid-programme (it poisons the filter from there on and is skipped by the peak) and two infs, against the clip hooks bit for bit.

    At FS = 2570 the K-weighting is unstable, so the state of every channel is inf or NaN long before the NaN comes in; the NaN then meets
    NaNs of the other sign, and the sign of a result is that of the operand the instruction names first.  This case is what holds the
    operand order of loudCarryStep and loudSumStep (csrc/smst_loudness.h): a build that left it to the compiler gave +NaN for -NaN in 52
    powers of stream 0 in the short-call form on the device"""
    image = programme(fs, 2).copy()
    n, h = image.shape[2], hop(fs)
    image[0, 1, 17*h + 31] = np.nan
    image[1, 0, 41*h + 3] = np.inf
    image[2, 1, 5] = -np.inf
    ref = clip_reference(lib, image, [n]*3, fs)
    for kind in ("random", "hop"):
        assert_reading(run(lib, image, cuts(kind, n, h), fs, form=form), 0, ref, dict(nan_inf=kind, fs=fs))
    if fs == FS_STABLE:
        assert np.isnan(ref["block_powers"][0, 20:]).all() and np.isfinite(ref["block_powers"][0, :13]).all()
        assert np.isfinite(ref["true_peaks"][0]) and np.isinf(ref["true_peaks"][1:]).all()


def check_second_rate(lib, form=0):
    """fs = 48000, 2 channels, 30 000 frames in 128-frame calls: the real-time shape, h not near the chunk"""
    fs, n = 48000.0, 30000
    rng = pc._rng(9504, 48000)
    image = np.ascontiguousarray((rng.uniform(-0.5, 0.5, (3, 2, n))*np.linspace(0.02, 1.0, n)[None, None, :]).astype(np.float32))
    counts = _stack([_cut_at(range(128, n, 128), n)]*3)
    got = run(lib, image, counts, fs, max_sub=8, form=form, max_blocks=8)
    ref = clip_reference(lib, image, [n]*3, fs, max_blocks=8)
    assert_reading(got, 0, ref, dict(fs=fs))
    assert ref["blocks"].tolist() == [3, 3, 3] and (ref["Z"] > 0).all()


def check_weights_and_unmetered(lib, Cn=3):
    """a non-trivial weight set, and a stream without the setting: its readings are those of nothing"""
    image = programme(FS_STABLE, Cn)
    n = image.shape[2]
    ref = clip_reference(lib, image, [n, 0, n], FS_STABLE, WEIGHTS[Cn])
    got = run(lib, image, cuts("ragged", n, H_STABLE), FS_STABLE, weights=WEIGHTS[Cn], flags=[1, 0, 1])
    assert got["metered"][0].tolist() == [n, 0, n]
    assert_reading(got, 0, ref, dict(weights=WEIGHTS[Cn]))
    plain = clip_reference(lib, image, [n]*3, FS_STABLE)
    assert not same_bits(plain["Z"][0], ref["Z"][0])


def check_against_mirrors(lib):
    """one base case against the float64 numpy mirrors, at the tolerances those files use for the clip hooks"""
    pkg = package()
    Cn = 2
    image = programme(FS_STABLE, Cn)
    n = image.shape[2]
    got = run(lib, image, cuts("random", n, H_STABLE), FS_STABLE, weights=WEIGHTS[Cn])
    taps = pkg.debug_true_peak_taps(lib=lib)
    for s in range(3):
        m, q = ld.mirror(image[s], FS_STABLE, WEIGHTS[Cn]), lr.mirror(image[s], FS_STABLE, WEIGHTS[Cn])
        assert ld.gates_clear(m) and lr.gates_clear(q), "a power lies on a gate: change the input"
        assert (int(got["blocks"][0, s]), int(got["gated"][0, s]), int(got["ns"][0, s]), int(got["n"][0, s])) == (m["blocks"], m["gated"], q["ns"], q["n"])
        assert ld.close(got["Z"][0, s], m["Z"]) and ld.close(got["block_powers"][s, :len(m["z"])], m["z"]) and ld.close(got["short_powers"][s, :q["ns"]], q["st"])
        for k in ("M", "ST", "lo", "hi"):
            assert ld.close(got[k][0, s], q[k]), (s, k)
        assert tp.same_bits(got["true_peaks"][0, s], tp.true_peak(image[s], taps)) and tp.same_bits(got["sample_peaks"][0, s], np.abs(image[s]).max())


def check_reproducible(lib):
    image = programme(FS_STABLE, 2)
    n = image.shape[2]
    a, b = (run(lib, image, cuts("ragged", n, H_STABLE), FS_STABLE, read_after=None) for _ in range(2))
    for k in a:
        assert same_bits(a[k], b[k]), k


def check_hook_refusals(lib):
    image = programme(FS, 1)
    n = image.shape[2]
    for kw, word in ((dict(max_sub=0), b"maxSubBlocks"), (dict(form=3), b"form"), (dict(fs=2000.0), b"rate"), (dict(max_sub=1 << 24, fs=48000.0), b"2^31")):
        try:
            run(lib, image, [[n]*3], kw.pop("fs", FS), **kw)
        except package().StretchError as e:
            assert word in str(e).encode() and "error -1" in str(e), str(e)
        else:
            raise AssertionError("not refused: %r" % (kw,))


# ---- end to end: processFrames and flushFrames ----------------------------------------------------------------------------------------------

E2E_FS = 2570.0                                      # what the meter is told: h = 257, so that the short session has blocks and short-term powers
E2E_FS_STABLE = 4010.0
E2E_CALLS = [([640, 640, 600], [512, 512, 480]), ([640, 0, 650], [512, 0, 520]), ([333, 640, 640], [266, 512, 512])] + [([640, 640, 640], [512, 512, 512])]*19
E2E_FLUSH = [200, -1, 300]
E2E_METERED = (True, False, True)                    # the second stream is unflagged; the third has the stream limiter on as well
E2E_GAINS = (0.5, 2.0, 4.0)
FORMATS = [(fc.S16, False), (fc.S16, True), (fc.S24, False), (fc.S24, True), (fc.F32, False)]
_e2e = {}


def e2e_inputs(fmt):
    """frames of the format [3, n, 2] and what they decode to: seeded noise with level steps"""
    n = sum(max(nin) for _, nin in E2E_CALLS)
    if fmt not in _e2e:
        rng = pc._rng(9505, 7)
        env = np.repeat([LEVELS[k % len(LEVELS)] for k in range(n//512 + 1)], 512)[:n]
        planar = (rng.uniform(-1, 1, (3, 2, n))*env[None, None, :]).astype(np.float32)
        _e2e[fmt] = fc.encode_frames(pc.frames_of(planar), fmt)
    return _e2e[fmt]


def e2e_run(lib, fmt, dithered, metered, fs=E2E_FS, take_after=None, **memory):
    """the session on a fresh batch -> (the calls' frames, the batch, the takes made on the way)"""
    b = package().StretchBatch(3, 2, lib=lib, seed=6, **pc.GEOMETRY)
    for s, g in enumerate(E2E_GAINS):
        b.set_pcm_level(lc.FIXED, g, stream=s)
    b.set_pcm_stream_limiter(True, lc.ceiling(fmt, dithered), stream=2)
    if dithered:
        dc.set_session_dither(b)
    if metered:
        for s, on in enumerate(E2E_METERED):
            b.set_pcm_stream_meter(on, fs, 64, stream=s)
    takes = []
    return frame_session(b, e2e_inputs(fmt), fmt, lambda k: takes.append(b.take_pcm_stream_meter()) if k == take_after else None, **memory), b, takes


def frame_session(batch, frames, fmt, between=None, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """E2E_CALLS through processFrames and E2E_FLUSH through flushFrames -> the outputs; between(k): called behind process call k"""
    outs, pos = [], 0
    for k, (nout, nin) in enumerate(E2E_CALLS):
        outs.append(to_host(batch.processFrames(to_memory(np.ascontiguousarray(frames[:, pos:pos + max(nin)])), nout, in_samples=nin)))
        pos += max(nin)
        if between:
            between(k)
    outs.append(to_host(batch.flushFrames(E2E_FLUSH, like=to_memory(np.zeros((1,), np.float32)), dtype=fc.frame_dtype(fmt))))
    return outs


def e2e_counts():
    return [nout for nout, _ in E2E_CALLS] + [[max(n, 0) for n in E2E_FLUSH]]


def e2e_totals():
    return totals(e2e_counts())


_e2e_refs = {}


def e2e_reference(lib, fs, upto=None):
    """the clip meters of the concatenated planar output of an F32 run of the same calls without the meter (the frames BEFORE the gain: the
    F32 frames divided by the fixed gains are not that, so the twin runs at gain 1 -- the engine's output does not depend on the level)"""
    key = (id(lib), fs, upto)
    if key not in _e2e_refs:
        t = package().StretchBatch(3, 2, lib=lib, seed=6, **pc.GEOMETRY)
        outs = frame_session(t, e2e_inputs(fc.F32), fc.F32)
        t.close()
        counts = e2e_counts()[:upto]
        n = int(totals(counts).max())
        image = np.zeros((3, 2, n), np.float32)
        for s in range(3):
            v = np.concatenate([np.ascontiguousarray(o[s, :c[s]].T) for o, c in zip(outs, counts)], axis=1)
            image[s, :, :v.shape[1]] = v
        lengths = [int(v) if E2E_METERED[s] else 0 for s, v in enumerate(totals(counts))]
        _e2e_refs[key] = (image, clip_reference(lib, image, lengths, fs, max_blocks=64), lengths)
    return _e2e_refs[key]


def lufs_of(P):
    """a power -> LUFS as the takes form it, -inf where it is 0 (math.log10: the C library's, as the host code's)"""
    return np.array([-0.691 + 10*math.log10(v) if v > 0 else -math.inf for v in np.atleast_1d(np.asarray(P, np.float64))])


def assert_take(take, ref, where):
    """a take against a clip reference: the counts and the peaks bit for bit, the LUFS values as the take forms them from the same powers"""
    for a, b in (("blocks", "blocks"), ("gated", "gated"), ("short_blocks", "ns"), ("range_blocks", "n"), ("true_peaks", "true_peaks"), ("sample_peaks", "sample_peaks")):
        assert same_bits(take[a], ref[b]), (where, a, take[a].tolist(), ref[b].tolist())
    defined = (ref["gated"] > 0) & (ref["Z"] > 0) & np.isfinite(ref["Z"])
    assert same_bits(take["lufs"], np.where(defined, lufs_of(ref["Z"]), -np.inf)), (where, take["lufs"].tolist())
    assert same_bits(take["momentary_max"], lufs_of(ref["M"])) and same_bits(take["short_term_max"], lufs_of(ref["ST"])), where
    some = ref["n"] > 0
    assert same_bits(take["low"], np.where(some, lufs_of(ref["lo"]), -np.inf)) and same_bits(take["high"], np.where(some, lufs_of(ref["hi"]), -np.inf)), where
    assert same_bits(take["range"], np.array([10*math.log10(hi/lo) if ok and lo > 0 else 0.0 for ok, lo, hi in zip(some, ref["lo"], ref["hi"])])), where
    for s in range(len(ref["Z"])):
        nb, ns = int(ref["nb"][s]), int(ref["ns"][s])
        newest_z = ref["block_powers"][s, nb - 1] if nb else 0.0
        newest_st = ref["short_powers"][s, ns - 1] if ns else 0.0
        assert same_bits(take["momentary"][s], lufs_of(newest_z)[0]) and same_bits(take["short_term"][s], lufs_of(newest_st)[0]), (where, s)


def check_e2e(lib, fs=E2E_FS_STABLE, **memory):
    """processFrames and flushFrames in chunks at stretch 1.25, three streams, the second unflagged, the third limited as well: the take is the
    clip meters' of the concatenated output of an F32 run without the meter; the counters match; a second take gives the same; a take
    mid-session changes nothing"""
    pkg = package()
    before = [pkg.launch_count(k, lib) for k in COUNTERS]
    got, b, _ = e2e_run(lib, fc.F32, False, True, fs, **memory)
    image, ref, lengths = e2e_reference(lib, fs)
    assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS, before)] == [len(E2E_CALLS) + 1, 0, 0]
    want = e2e_totals()
    for s in range(3):
        assert b.pcm_stream_meter_frames(s) == ((int(want[s]), int(want[s])) if E2E_METERED[s] else (0, 0))
        assert b.pcm_stream_meter(s) == ((True, fs, 64) if E2E_METERED[s] else (False, 0.0, 0))
    take = b.take_pcm_stream_meter()
    assert_take(take, ref, dict(e2e=fs))
    assert ref["blocks"][0] > 0 and ref["ns"][2] > 0 and ref["blocks"][1] == 0 and take["lufs"][1] == -np.inf and take["true_peaks"][1] == 0
    again = b.take_pcm_stream_meter()
    for k in take:
        assert same_bits(take[k], again[k]), k
    assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS, before)] == [len(E2E_CALLS) + 1, 2, 0]
    b.close()
    # a take mid-session: the clip meters' of the frames so far, and the end is what it is without it
    _, b2, takes = e2e_run(lib, fc.F32, False, True, fs, take_after=7, **memory)
    assert_take(takes[0], e2e_reference(lib, fs, upto=8)[1], dict(e2e=fs, mid=True))
    final = b2.take_pcm_stream_meter()
    for k in take:
        assert same_bits(take[k], final[k]), k
    b2.close()
    return got


def check_e2e_bytes(lib, fmt, dithered, **memory):
    """the meter changes no output byte of any stream, in any format"""
    with_meter, b, _ = e2e_run(lib, fmt, dithered, True, **memory)
    without, t, _ = e2e_run(lib, fmt, dithered, False, **memory)
    for k, (x, y) in enumerate(zip(with_meter, without)):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) and np.asarray(x).any(), (fmt, dithered, k)
    for x, y in zip(b.take_pcm_peaks() + b.take_pcm_stream_limiter() + b.takePcmOvers(), t.take_pcm_peaks() + t.take_pcm_stream_limiter() + t.takePcmOvers()):
        assert np.array_equal(x, y)
    if fmt == fc.F32:                                                            # (... and the meter saw the frames BEFORE the gain, whatever the format's)
        assert_take(b.take_pcm_stream_meter(), e2e_reference(lib, E2E_FS)[1], dict(bytes=fmt))
    b.close()
    t.close()


# ---- opt-in, steady state, refusals, clearing ------------------------------------------------------------------------------------------------

def check_opt_in(lib, **memory):
    """a batch that never calls the setter launches no meter kernel and its sessions give their own mirrors' bytes; a metered batch in a call
    in which no metered stream has frames launches none either"""
    pkg = package()
    before = [pkg.launch_count(k, lib) for k in COUNTERS]
    assert min(before) >= 0, "the library has no stream meter counters"
    lc.check_session(lib, fc.S16, True, **memory)
    dc.check_session(lib, fc.S16, **memory)
    pc.check_session(lib, 2, pc.F32, **memory)
    assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS, before)] == [0, 0, 0]
    to_memory = memory.get("to_memory", lambda a: a)
    frames = e2e_inputs(fc.S16)
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    b.set_pcm_stream_meter(True, E2E_FS, 8, stream=0)
    b.processFrames(to_memory(np.ascontiguousarray(frames[:, :512])), [0, 300, 200], in_samples=[512, 300, 200])
    b.flushFrames([-1, 10, 10], like=to_memory(np.zeros((1,), np.float32)))
    assert [pkg.launch_count(k, lib) - n for k, n in zip(COUNTERS, before)] == [0, 0, 0] and b.pcm_stream_meter_frames(0) == (0, 0)
    b.close()


def check_steady_state(lib, to_memory=lambda a: a):
    """the setter allocates the carried state, the histories and a reading's scratch outside any call; metered calls and takes leave
    allocation_events and workspaceBytes where they are"""
    pkg = package()
    S, Cn, subs = 3, 2, 40
    frames = e2e_inputs(fc.S16)
    x = to_memory(np.ascontiguousarray(frames[:, :512]))
    b = pkg.StretchBatch(S, Cn, lib=lib, **pc.GEOMETRY)
    for _ in range(2):
        b.processFrames(x, [600, 300, 128])
    b.synchronize()
    plain, events = b.workspaceBytes(), b.allocation_events()
    b.set_pcm_stream_meter(True, E2E_FS, subs, stream=1)
    grown = b.workspaceBytes()
    assert grown >= plain + S*Cn*subs*8 and b.allocation_events() == events + 1, (plain, grown)
    # what the header states: config + state + frames + words + histories + the reading's scratch and tables
    reading = 2*S + (S + 1)//2 + S*subs + (5*S + S*subs) + 3*S
    stated = S*(7 + 16 + 2)*8 + S*Cn*16*8 + S*Cn*11*4 + 2*S*4 + S*Cn*subs*8 + reading*8 + (2*S*16 + S*(7 + 16 + 2 + 1 + 2)*8 + 16*4)
    assert grown == plain + stated, (grown - plain, stated)
    b.set_pcm_stream_meter(True, E2E_FS, subs - 3)
    assert b.workspaceBytes() == grown and b.allocation_events() == events + 1
    b.processFrames(x, [600, 300, 128])
    b.synchronize()
    events = b.allocation_events()
    for _ in range(3):
        b.processFrames(x, [600, 300, 128])
        take = b.take_pcm_stream_meter()
    b.flushFrames([100, 100, 100], like=to_memory(np.zeros((1,), np.float32)))
    assert b.allocation_events() == events and b.workspaceBytes() == grown and (take["sample_peaks"] > 0).all()
    b.close()


def check_refusals(lib, **memory):
    pkg = package()
    to_memory = memory.get("to_memory", lambda a: a)
    b = pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY)
    state = lambda: ([b.pcm_stream_meter(s) for s in range(3)], b.workspaceBytes(), b.allocation_events())
    start = state()
    assert start[0] == [(False, 0.0, 0)]*3
    ll = C.POINTER(C.c_longlong)
    for stream in (3, -2):
        assert lib.smst_batch_set_pcm_stream_meter(b.h, stream, 1, 48000.0, 10) == -1 and b"stream" in lib.smst_last_error()
    for stream in (3, -1):
        assert lib.smst_batch_pcm_stream_meter(b.h, stream, None, None, None) == -1 and b"stream" in lib.smst_last_error()
        assert lib.smst_batch_pcm_stream_meter_frames(b.h, stream, None, None) == -1 and b"stream" in lib.smst_last_error()
    for rate in (float("nan"), 0.0, -48000.0, float("inf"), 2549.0, 2e9):
        assert lib.smst_batch_set_pcm_stream_meter(b.h, 0, 1, rate, 10) == -1 and b"rate" in lib.smst_last_error(), rate
        assert lib.smst_batch_set_pcm_loudness(b.h, 0, -23.0, 1.0, rate) == -1                       # (the loudness setter's rule)
    for blocks in (0, -5):
        assert lib.smst_batch_set_pcm_stream_meter(b.h, 0, 1, 48000.0, blocks) == -1 and b"maxSubBlocks" in lib.smst_last_error()
    assert lib.smst_batch_set_pcm_stream_meter(b.h, 0, 1, 48000.0, (1 << 31)//4800 + 1) == -1 and b"2^31" in lib.smst_last_error()
    assert state() == start                                                      # (a refused call changes nothing)
    assert lib.smst_batch_set_pcm_stream_meter(None, 0, 1, 48000.0, 10) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_stream_meter(None, 0, None, None, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_pcm_stream_meter_frames(None, 0, None, None) == -1 and b"null" in lib.smst_last_error()
    assert lib.smst_batch_take_pcm_stream_meter(None, *[None]*14) == -1 and b"null" in lib.smst_last_error()
    # what is allowed: null pointers in the getters and the take, a take before any setter, off with any rate
    assert lib.smst_batch_pcm_stream_meter(b.h, 0, None, None, None) == 0 and lib.smst_batch_pcm_stream_meter_frames(b.h, 0, None, None) == 0
    assert lib.smst_batch_take_pcm_stream_meter(b.h, *[None]*14) == 0
    assert b.take_pcm_stream_meter()["lufs"].tolist() == [-np.inf]*3
    assert lib.smst_batch_set_pcm_stream_meter(b.h, -1, 0, float("nan"), -1) == 0 and state() == start
    b.set_pcm_stream_meter(True, E2E_FS, 12, stream=1)
    assert [b.pcm_stream_meter(s) for s in range(3)] == [(False, 0.0, 0), (True, E2E_FS, 12), (False, 0.0, 0)]
    assert lib.smst_batch_set_pcm_stream_meter(b.h, 0, 1, E2E_FS, 13) == -1 and b"maxSubBlocks" in lib.smst_last_error()   # (the histories hold 12)
    # the whole-clip flags are still refused by the streaming calls, word for word
    frames = e2e_inputs(fc.S16)
    x = to_memory(np.ascontiguousarray(frames[:, :512]))
    like = to_memory(np.zeros((1,), np.float32))
    for setter, word in ((lambda on: b.set_pcm_true_peak(on, stream=0), "has the true-peak flag (smst_batch_set_pcm_true_peak): smst_batch_exact_pcm only"),
                         (lambda on: b.set_pcm_loudness_range(on, 48000.0, stream=0), "has the loudness-range meter flag or a loudness cap (smst_batch_set_pcm_loudness_range / _caps), which measure a whole clip: smst_batch_exact_pcm only")):
        setter(True)
        for call in (lambda: b.processFrames(x, [600, 300, 0]), lambda: b.flushFrames([100, 50, -1], like=like)):
            with dc.pytest_raises(pkg.StretchError) as e:
                call()
            assert "stream 0 " + word in str(e.value) and "error -1" in str(e.value), str(e.value)
        setter(False)
    # exactFrames refuses a participating metered stream and names the whole-clip forms; it accepts one that a negative count leaves out
    clip, n = to_memory(np.ascontiguousarray(frames[:, :2000])), 2000
    with dc.pytest_raises(pkg.StretchError) as e:
        b.exactFrames(clip, [n + 100]*3)
    assert "smst_batch_set_pcm_stream_meter" in str(e.value) and "smst_batch_set_pcm_true_peak" in str(e.value) and "error -1" in str(e.value), str(e.value)
    out, ok = b.exactFrames(clip, [n + 100, -1, n + 100])
    assert ok.tolist() == [True, False, True]
    # the weights: refused while a meter holds frames, accepted behind a clear
    b.reset()
    b.set_pcm_loudness_weights([1.0, 0.5])
    b.processFrames(x, [600, 300, 100])
    assert b.pcm_stream_meter_frames(1) == (300, 300)
    with dc.pytest_raises(pkg.StretchError) as e:
        b.set_pcm_loudness_weights([1.0, 1.0])
    assert "stream meter" in str(e.value) and "error -1" in str(e.value), str(e.value)
    b.set_pcm_stream_meter(True, E2E_FS, 12, stream=1)
    b.set_pcm_loudness_weights([1.0, 1.0])
    b.close()


def check_clearing(lib, action, **memory):
    """call A, the action, call B on a metered batch: the setter (for its stream) and reset clear the meter -- the take is the clip meters' of
    B's frames alone --, a level change does not: it is the clip meters' of A's and B's"""
    pkg = package()
    to_memory, to_host = memory.get("to_memory", lambda a: a), memory.get("to_host", lambda a: np.array(a, copy=True))
    fs = E2E_FS_STABLE
    frames = e2e_inputs(fc.F32)
    b, t = (pkg.StretchBatch(3, 2, lib=lib, **pc.GEOMETRY) for _ in range(2))
    b.set_pcm_level(lc.FIXED, 3.0)
    b.set_pcm_stream_meter(True, fs, 16)
    calls = [to_memory(np.ascontiguousarray(frames[:, k*1024:(k + 1)*1024])) for k in range(2)]
    nout = [[1280, 700, 20], [1300, 1280, 9]]
    a_t = to_host(t.processFrames(calls[0], nout[0]))
    b.processFrames(calls[0], nout[0])
    if action == "setter":
        b.set_pcm_stream_meter(True, fs, 16)
    elif action == "setter_one":
        b.set_pcm_stream_meter(True, fs, 16, stream=1)                            # (the other streams keep their meters)
    elif action == "reset":
        b.reset()
        t.reset()
    elif action == "level":
        b.set_pcm_level(lc.FIXED, -0.25)
        b.set_pcm_stream_limiter(False, 1.0)
    else:
        raise ValueError(action)
    b_t = to_host(t.processFrames(calls[1], nout[1]))
    b.processFrames(calls[1], nout[1])
    image = np.zeros((3, 2, 2600), np.float32)
    lengths = []
    for s in range(3):
        cleared = action in ("setter", "reset") or (action == "setter_one" and s == 1)
        parts = ([] if cleared else [a_t[s, :nout[0][s]]]) + [b_t[s, :nout[1][s]]]
        v = np.concatenate([np.ascontiguousarray(p.T) for p in parts], axis=1)
        image[s, :, :v.shape[1]] = v
        lengths.append(v.shape[1])
        assert b.pcm_stream_meter_frames(s) == (v.shape[1], v.shape[1])
    assert_take(b.take_pcm_stream_meter(), clip_reference(lib, image, lengths, fs, max_blocks=16), dict(action=action))
    b.close()
    t.close()
