"""Shared cases of the sample-rate converter in front of smst_batch_exact_pcm (include/smst.h, "Resample"): test_resample_emu.py runs them on
the CPU stand-in, test_resample_gpu.py on the device.

The mirror is a numpy restatement of the header's text: the Kaiser-windowed sinc in float64, one rounding to float32 per coefficient; per
resampled frame the float64 sum of the T products in the order j = 0 ... T-1, one rounding.  A product of two float32 values is exact in
float64, so the mirror reproduces the device bit for bit -- given the same table, which is why the signal checks read the library's own
table through smst_debug_resample_taps (a last-bit difference between the host's libm and numpy cannot reach them); the table itself is
checked against the formula to one float32 ulp."""
import math
import subprocess

import numpy as np

import dither_cases as dc
import exact_cases as xc
import level_cases as lc
import pcm_cases as pc
import pcm_format_cases as fc
from conftest import package, synth_input

MAX_TERM, MAX_RATIOS, TILE = 640, 8, 1024
COUNTER = "clip_resample"
RATIOS = ((2, 1), (1, 2), (3, 2), (2, 3), (160, 147), (147, 160), (147, 640), (640, 147))
TABLE_RATIOS = ((1, 1),) + RATIOS + ((9, 2), (2, 9))
TAPS = {(1, 1): 64, (2, 1): 64, (1, 2): 128, (3, 2): 64, (2, 3): 96, (160, 147): 64, (147, 160): 70, (147, 640): 280, (640, 147): 64, (9, 2): 64, (2, 9): 288}
# every launch counter of the library (smst_debug_launch_count), as csrc/smst_state.hip names them
COUNTERS = ("vocoder_aligned", "vocoder_twisted", "vocoder_interior", "vocoder_staged", "vocoder_gather", "vocoder_n", "vocoder_one", "vocoder_across", "vocoder_continuous",
            "chain_unfused", "analyse_teams", "analyse_pairs", "analyse_twist", "twist_rows", "analyse_fast", "analyse_generic", "synth_teams", "synth_fast", "synth_generic",
            "synth_emit", "emit_carried", "feed_one_pass", "pcm_in", "pcm_out", "clip_in", "clip_out", "pcm_out_dithered", "clip_out_dithered", "pcm_out_levelled",
            "clip_out_levelled", "clip_peak", "clip_loudness", "clip_true_peak", "clip_limit_need", "clip_limit_gain", "clip_out_limited", "clip_loudness_range", COUNTER)
ERR_INVALID = -1


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def reduced(up, down):
    g = math.gcd(up, down)
    return up//g, down//g


def shape_of(up, down):
    """-> (L, M, H, T) of the reduced ratio"""
    L, M = reduced(up, down)
    H = 32 if M <= L else -((-32*M)//L)
    return L, M, H, 2*H


def resampled_length(n, up, down):
    L, M = reduced(up, down)
    return (n*L + M - 1)//M


def formula_taps(up, down):
    """the header's formula in float64 -> float32 [L, T]"""
    L, M, H, T = shape_of(up, down)
    r = min(1.0, L/M)
    rho, W = 0.98*r, (32.0*M/L if M > L else 32.0)
    t = (np.arange(T, dtype=np.float64)[None, :] - (H - 1)) - np.arange(L, dtype=np.float64)[:, None]/L
    inside = np.abs(t) < W
    u = np.where(inside, t/W, 0.0)
    h = np.where(inside, rho*np.sinc(rho*t)*np.i0(10.0*np.sqrt(1.0 - u*u))/np.i0(10.0), 0.0)
    return (h/h.sum(axis=1, keepdims=True)).astype(np.float32)


def mirror(x, up, down, table):
    """x float32 [..., N] -> float32 [..., Nr]: frame n = float32(sum_j float64(c[p][j])*float64(x(i + j - (H - 1)))), j ascending from 0.0"""
    L, M, H, T = shape_of(up, down)
    assert table.shape == (L, T) and table.dtype == np.float32
    x = np.asarray(x, np.float32)
    N = x.shape[-1]
    Nr = resampled_length(N, L, M)
    n = np.arange(Nr, dtype=np.int64)
    i, p = (n*M)//L, (n*M) % L
    padded = np.zeros(x.shape[:-1] + (N + 2*T,), np.float64)
    padded[..., T:T + N] = x
    c = table.astype(np.float64)
    y = np.zeros(x.shape[:-1] + (Nr,), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(T):
            y = y + c[p, j]*padded[..., i + (j - (H - 1)) + T]
        return y.astype(np.float32)


def bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def same_floats(a, b):
    """bit patterns equal, any NaN equal to any other (its sign and payload are the adder's own)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def ulps(a, b):
    """distance in float32 ulps (both finite)"""
    def key(v):
        k = bits(v).astype(np.int64)
        return np.where(k & 0x80000000, 0x80000000 - k, k)
    return np.abs(key(a) - key(b))


def _hex(v):
    return " ".join("%08x" % w for w in bits(v).reshape(-1))


def response_db(up, down, table, nfft=1 << 21):
    """the float32 table as ONE prototype filter at L times the input rate -> (f in cycles per input sample, gain in dB); each phase has
    unit DC gain, so the prototype's is L"""
    L, M, H, T = shape_of(up, down)
    proto = np.zeros(L*T + L, np.float64)
    j, p = np.meshgrid(np.arange(T), np.arange(L))
    proto[(j*L - p + (L - 1)).reshape(-1)] = table.astype(np.float64).reshape(-1)       # (time (j - (H - 1))*L - p, shifted to begin at 0)
    G = np.abs(np.fft.rfft(proto, nfft))/L
    f = np.arange(G.size)*(L/nfft)
    return f, 20*np.log10(np.maximum(G, 1e-300))


def check_mirror():
    """the known answers of include/smst.h on the formula's table, the frequency response, and two sines 44.1 -> 48 kHz"""
    c = formula_taps(2, 1)
    assert ulps(c[0, 30:33], np.array([0x3ca2f978, 0x3f7ae0ea, 0x3ca2f978], np.uint32).view(np.float32)).max() <= 1, _hex(c[0, 30:33])
    assert ulps(c[1, 31:33], np.array([0x3f22b49c]*2, np.uint32).view(np.float32)).max() <= 1, _hex(c[1, 31:33])
    c = formula_taps(160, 147)
    assert c.shape == (160, 64) and ulps(c[0, 31], np.uint32(0x3f7ae0ea).view(np.float32)) <= 1
    assert ulps(c[80, 31:33], np.array([0x3f22b49c]*2, np.uint32).view(np.float32)).max() <= 1 and ulps(c[159, 0], np.float32(-3.198598506e-06)) <= 1, (_hex(c[80, 31:33]), float(c[159, 0]))
    c = formula_taps(147, 160)
    assert c.shape == (147, 70) and ulps(c[1, 34:36], np.array([0x3f667b0e, 0x3dd53ebb], np.uint32).view(np.float32)).max() <= 1, _hex(c[1, 34:36])
    assert ulps(c[0, 0], np.float32(8.022285328e-06)) <= 1, float(c[0, 0])
    for ratio, T in TAPS.items():
        assert shape_of(*ratio)[3] == T, (ratio, shape_of(*ratio))
    x = np.zeros(5, np.float32); x[2] = 1
    got = mirror(x, 3, 2, formula_taps(3, 2))
    assert _hex(got) == "bca067e3 be4717b5 3ed8327b 3f7ae0ea 3ed8327b be4717b5 bca067e3 3dddb185", _hex(got)
    x = np.zeros(7, np.float32); x[3] = 1
    got = mirror(x, 2, 3, formula_taps(2, 3))
    assert _hex(got) == "bc55dff0 3c594cd8 3f2740ad 3c594cd8 bc55dff0", _hex(got)
    got = mirror(np.ones(200, np.float32), 160, 147, formula_taps(160, 147))
    assert got.shape == (218,) and np.abs(got[40:170].astype(np.float64) - 1).max() <= 6.0e-8, float(np.abs(got[40:170].astype(np.float64) - 1).max())


def check_response():
    """passband within [-0.06, +0.001] dB up to 0.907 of the lower Nyquist, everything at or above 1.093 of it at or below -100 dB
    (measured: -0.0526 / +0.0001 dB and -100.6 dB at worst)"""
    for up, down in ((160, 147), (147, 160), (1, 2)):
        L, M, H, T = shape_of(up, down)
        f, db = response_db(up, down, formula_taps(up, down))
        nyquist = 0.5*min(1.0, L/M)
        passband, stop = db[f <= 0.907*nyquist], db[f >= 1.093*nyquist]
        print("resample %d/%d: passband %.4f ... %+.4f dB, stopband %.1f dB" % (up, down, passband.min(), passband.max(), stop.max()))
        assert -0.06 <= passband.min() and passband.max() <= 0.001, (up, down, passband.min(), passband.max())
        assert stop.max() <= -100.0, (up, down, stop.max())


def check_sines():
    """1 kHz and 19 kHz, 4000 frames at 44.1 kHz, resampled 160/147 against the ideal 48 kHz sine over the frames 100 ... Nr - 100
    (measured: 5.9e-6 and 1.8e-5; the bound is twice that, the margin for another libm's table)"""
    table = formula_taps(160, 147)
    for hz, bound in ((1000.0, 2*5.9e-6), (19000.0, 2*1.8e-5)):
        x = np.sin(2*np.pi*hz*np.arange(4000)/44100.0).astype(np.float32)
        y = mirror(x, 160, 147, table)
        ideal = np.sin(2*np.pi*hz*np.arange(y.size)/48000.0)
        err = float(np.abs(y.astype(np.float64) - ideal)[100:y.size - 100].max())
        print("resample 160/147, %g Hz: largest error %.3g (bound %.3g)" % (hz, err, bound))
        assert err <= bound, (hz, err, bound)


# ---- the table -----------------------------------------------------------------------------------------------------------------------

_tables = {}


def library_taps(lib, up, down):
    key = (id(lib),) + reduced(up, down)
    if key not in _tables:
        _tables[key] = package().debug_resample_taps(up, down, lib=lib)
    return _tables[key]


def check_table(lib, up, down):
    """T, every coefficient within one float32 ulp of the formula, every phase's float64 sum within 1e-6 of 1"""
    L, M, H, T = shape_of(up, down)
    got, want = library_taps(lib, up, down), formula_taps(up, down)
    assert got.shape == want.shape == (L, TAPS[reduced(up, down)]), (up, down, got.shape)
    assert got.shape == package().debug_resample_taps(2*up, 2*down, lib=lib).shape                 # (the library reduces the ratio)
    assert ulps(got, want).max() <= 1, (up, down, int(ulps(got, want).max()))
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1).max() <= 1e-6


# ---- the kernel against the mirror ---------------------------------------------------------------------------------------------------

SENTINEL = np.float32(-7.25)


def lengths_for(up, down):
    """clip lengths whose Nr lies on and beside tile edges, and clips shorter than a filter"""
    L, M, H, T = shape_of(up, down)
    out = []
    for target in (TILE - 1, TILE, TILE + 1, 2*TILE + 1):
        n = max((target*M)//L - 2, 1)
        while resampled_length(n, L, M) < target:
            n += 1
        out.append(n)
    return out + [1, 2, H - 1, H, T + 1]


def _float_buffer(n, offset):
    """n float32 whose first element lies `offset` floats behind a 16-byte boundary"""
    return fc.byte_buffer(4*n, 4*offset).view(np.float32)


def run_kernel(lib, clips, ratios, splits, dst_offsets=(1, 2, 3, 0), src_offset=1, out_offset=0):
    """clips: per stream float32 [C, N]; ratios: per stream (up, down); splits: per stream the frames of segment 0.  Source rows lie at
    every offset from a 16-byte boundary (an odd channel stride), the two destination runs at dst_offsets[s % 4] and a column of its own
    -> (out as the hook left it, the expected image: the mirror's frames inside the sentinel)"""
    pkg = package()
    S, Cn = len(clips), clips[0].shape[0]
    counts = [c.shape[1] for c in clips]
    nr = [resampled_length(n, *r) for n, r in zip(counts, ratios)]
    in_cs = max(counts) + 5                                                   # (odd against 4: a stream's rows lie at every offset)
    in_ss = Cn*in_cs + 1
    image = _float_buffer(S*in_ss + 8, src_offset)
    image[:] = np.float32(123.0)
    col = (max(splits) + 3)//4*4 + 8                                          # segment 1's column, a gap of sentinels in front of it
    out_cs = col + max(n - k for n, k in zip(nr, splits)) + 11
    out_ss = Cn*out_cs + 3
    out = _float_buffer(S*out_ss + 8, out_offset)
    out[:] = SENTINEL
    want = np.array(out, copy=True)
    segments = np.zeros((S, 2, 4), np.int32)
    before = pkg.launch_count(COUNTER, lib)
    for s in range(S):
        for c in range(Cn):
            image[s*in_ss + c*in_cs:s*in_ss + c*in_cs + counts[s]] = clips[s][c]
        off = dst_offsets[s % len(dst_offsets)]
        segments[s, 0] = (0, off, splits[s], 0)
        segments[s, 1] = (splits[s], col + (off + 1) % 4, nr[s] - splits[s], 0)
        if reduced(*ratios[s]) == (1, 1):
            continue
        y = mirror(clips[s], *ratios[s], library_taps(lib, *ratios[s]))
        for c in range(Cn):
            row = s*out_ss + c*out_cs
            want[row + segments[s, 0, 1]:row + segments[s, 0, 1] + splits[s]] = y[c, :splits[s]]
            want[row + segments[s, 1, 1]:row + segments[s, 1, 1] + nr[s] - splits[s]] = y[c, splits[s]:]
    pkg.debug_clip_resample(counts, ratios, Cn, image, in_ss, in_cs, segments, out, out_ss, out_cs, lib=lib)
    assert pkg.launch_count(COUNTER, lib) == before + 1
    return out, want


def check_kernel(lib, up, down, channels):
    """one launch per ratio and channel count: noise at full scale in clips of every length of lengths_for, every destination split (at frame
    0, inside a tile, on a tile edge, at Nr), a stream of zeros, one with a NaN in the middle, one with +-inf; bit for bit, sentinels kept"""
    L, M, H, T = shape_of(up, down)
    rng = np.random.default_rng(1000*up + down + channels)
    counts = lengths_for(up, down)
    clips = [rng.uniform(-1, 1, (channels, n)).astype(np.float32) for n in counts]
    special = 3*T + 37
    zeros, nan, inf = np.zeros((channels, special), np.float32), rng.uniform(-1, 1, (channels, special)).astype(np.float32), rng.uniform(-1, 1, (channels, special)).astype(np.float32)
    nan[0, special//2] = np.nan
    inf[channels - 1, 5] = np.inf
    inf[0, special - 9] = -np.inf
    clips += [zeros, nan, inf]
    ratios = [(up, down)]*len(clips)
    nr = [resampled_length(c.shape[1], L, M) for c in clips]
    choices = (lambda n: 0, lambda n: n//3, lambda n: TILE if n > TILE else n//2, lambda n: n)
    splits = [choices[(s + channels) % 4](n) for s, n in enumerate(nr)]
    splits[1], splits[3] = min(TILE, nr[1]), min(TILE, nr[3])              # (exactly on a tile edge where the clip reaches it)
    for src_offset, out_offset in ((1, 0), (3, 2)) if channels == 2 else ((2, 1),):
        got, want = run_kernel(lib, clips, ratios, splits, src_offset=src_offset, out_offset=out_offset)
        assert same_floats(got, want), (up, down, channels, np.flatnonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))[:8])
    # exactly the frames whose T taps reach the NaN are NaN: i - (H - 1) <= k <= i + H
    y = mirror(nan, up, down, library_taps(lib, up, down))
    i = (np.arange(y.shape[1], dtype=np.int64)*M)//L
    reached = (i - (H - 1) <= special//2) & (special//2 <= i + H)
    assert np.array_equal(np.isnan(y[0]), reached) and reached.any() and not reached.all() and not np.isnan(y[1:]).any(), (up, down)
    assert not mirror(zeros, up, down, library_taps(lib, up, down)).any()


def check_mixed(lib, channels=2):
    """eight streams with eight different ratios in one launch, two streams at 1/1 among them: their rows of the output stay as they were"""
    rng = np.random.default_rng(77)
    ratios = list(RATIOS[:3]) + [(1, 1)] + list(RATIOS[3:6]) + [(5, 5)] + list(RATIOS[6:])
    counts = [700, 2100, 1500, 900, 3000, 1100, 1300, 640, 5000, 300]
    clips = [rng.uniform(-1, 1, (channels, n)).astype(np.float32) for n in counts]
    nr = [resampled_length(n, *r) for n, r in zip(counts, ratios)]
    splits = [(n*(s + 1))//11 for s, n in enumerate(nr)]
    got, want = run_kernel(lib, clips, ratios, splits)
    assert same_floats(got, want)
    assert len(set(reduced(*r) for r in ratios) - {(1, 1)}) == 8


# ---- whole clips ---------------------------------------------------------------------------------------------------------------------

CLIP_RATIOS = ((160, 147), (1, 1), (1, 2), (2, 3), (147, 640), (3, 2))      # stream 2 becomes too short by its ratio alone, stream 5 is left out
CLIP_FACTORS = (1.25, 0.9, 1.0, 1.5, 1.1, 1.0)
SHORT, LEFT, PLAIN = 2, 5, 1
CLIP_SEED = 61
CHAIN_FS = 4000.0


def clip_case(lib, Cn=2):
    """-> (inputs N, resampled lengths Nr, outputs) of CLIP_RATIOS; stream SHORT has N at or above the seek length and Nr below it"""
    pkg = package()
    probe = pkg.StretchBatch(1, Cn, lib=lib, **pc.GEOMETRY)
    seek = probe.outputSeekLength(1.0)
    probe.close()
    nin = [5000, 6000, seek + seek//2, 7000, 20000, 4000]
    nr = [resampled_length(n, *r) for n, r in zip(nin, CLIP_RATIOS)]
    nout = [int(round(n*f)) for n, f in zip(nr, CLIP_FACTORS)]
    assert nr[SHORT] < seek <= nin[SHORT]
    return nin, nr, nout


def set_ratios(batch):
    for s, (up, down) in enumerate(CLIP_RATIOS):
        batch.set_pcm_resample(up, down, stream=s)
        assert batch.pcm_resample(s) == reduced(up, down)


def set_chain(batch, ceil=0.25):
    """LOUDNESS + true peak + limiter on every stream; the target is loud enough for the limiter to have work"""
    batch.set_pcm_loudness(-8.0, ceil, CHAIN_FS)
    batch.set_pcm_true_peak(True)
    batch.set_pcm_limiter(True)


def clip_inputs(fmt, nin, Cn=2):
    """-> (frames of the format [S, max N, C], the planar float32 [S, C, max N] they decode to)"""
    frames = fc.encode_frames(pc.frames_of(xc.clip_inputs(Cn, nin, loud=0)), fmt)
    return frames, np.ascontiguousarray(np.transpose(fc.decode_frames(frames, fmt), (0, 2, 1)))


def twin_inputs(lib, planar, nin, nr):
    """the mirror's resampled clips as F32 frames [S, max Nr, C]"""
    S, Cn = planar.shape[:2]
    y = np.zeros((S, Cn, max(nr)), np.float32)
    for s, (up, down) in enumerate(CLIP_RATIOS):
        y[s, :, :nr[s]] = mirror(planar[s, :, :nin[s]], up, down, library_taps(lib, up, down)) if reduced(up, down) != (1, 1) else planar[s, :, :nin[s]]
    return pc.frames_of(y)


def check_clips(lib, fmt, dithered, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True), chain=False, calls=2):
    """exactFrames of a batch with CLIP_RATIOS against a twin batch without resampling that is fed the mirror's resampled clips as F32 frames:
    the resampled batch's bytes are the twin's floats put through the format's own output rule (dithered where the format can be), byte for
    byte, as are status, overs and peaks.  chain: LOUDNESS + true peak + limiter on both, F32 on both sides: the bytes and every meter agree"""
    pkg = package()
    nin, nr, nout = clip_case(lib)
    S, Cn, most = len(nin), 2, max(nout)
    frames, planar = clip_inputs(fmt, nin)
    twin_frames = twin_inputs(lib, planar, nin, nr)
    r, t = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(2))
    set_ratios(r)
    modes = [dc.CLIP_MODES[s % len(dc.CLIP_MODES)] if dithered else dc.NONE for s in range(S)]
    for b in (r, t):
        if chain:
            set_chain(b)
        else:
            b.set_pcm_level(lc.FIXED, 1.0, 1.0)                                   # (a levelled batch meters peaks)
    if dithered:
        for s in range(S):
            r.setPcmDither(modes[s], CLIP_SEED + s, stream=s)
    n_out = [(-1 if s == LEFT else n) for s, n in enumerate(nout)]
    assert [r.resampled_length(s, nin[s]) for s in range(S)] == nr
    for call in range(calls):
        fill = lambda like: np.full(like.shape[:1] + (most,) + like.shape[2:], 0x5A, like.dtype)
        want, ok_t = t.exactFrames(to_memory(twin_frames), n_out, in_samples=nr, out=to_memory(fill(twin_frames)))
        want = to_host(want)
        before = pkg.launch_count(COUNTER, lib)
        got, ok_r = r.exactFrames(to_memory(frames), n_out, in_samples=nin, out=to_memory(fill(frames)))
        got = to_host(got)
        assert pkg.launch_count(COUNTER, lib) == before + 1
        assert ok_r.tolist() == ok_t.tolist() == [s not in (SHORT, LEFT) for s in range(S)], (ok_r.tolist(), ok_t.tolist())
        peaks_r, gains_r = r.take_pcm_peaks()
        peaks_t, gains_t = t.take_pcm_peaks()
        assert np.array_equal(bits(peaks_r), bits(peaks_t)) and np.array_equal(bits(gains_r), bits(gains_t)), (peaks_r, peaks_t, gains_r, gains_t)
        overs_r, nans_r = r.takePcmOvers()
        if chain:
            assert fmt == fc.F32 and np.array_equal(got.view(np.uint8), want.view(np.uint8)), call
            for take in ("take_pcm_loudness", "take_pcm_true_peaks", "take_pcm_limiter"):
                a, b = getattr(r, take)(), getattr(t, take)()
                for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                    assert np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)), (take, u, v)
            assert np.isfinite(r.take_pcm_loudness()[0][0]), r.take_pcm_loudness()
            assert (r.take_pcm_limiter()[1] > 0).any() and (r.take_pcm_true_peaks() > 0).any(), r.take_pcm_limiter()   # (the chain did work)
            continue
        expect = fill(frames)
        for s in range(S):
            if s == LEFT:
                continue
            x = np.ascontiguousarray(want[s, :nout[s]].T)                        # (the twin's floats: the engine's own output, gain 1)
            codes, cm, nm = dc.mirror(x, fmt, dc.NONE if s == SHORT else modes[s], CLIP_SEED + s, 0)     # (a too-short stream's zeros are not dithered)
            expect[s, :nout[s]] = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
            assert (int(overs_r[s]), int(nans_r[s])) == (int(cm.sum()), int(nm.sum())), (fmt, s, int(overs_r[s]), int(cm.sum()))
            assert s == SHORT or x.any()
        assert lc.same_bytes(got.reshape(-1).view(np.uint8), expect.reshape(-1).view(np.uint8), fmt), (fmt, dithered, call)
        assert (got[LEFT] == 0x5A).all() and not got[SHORT, :nout[SHORT]].any()
    for b in (r, t):
        b.close()


# ---- opt-in, steady state, reproducible ----------------------------------------------------------------------------------------------

def _counts(lib):
    pkg = package()
    return [pkg.launch_count(k, lib) for k in COUNTERS]


def check_opt_in(lib, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """a batch that never sets a ratio against a twin: the same bytes, the same launches, clip_resample where it was; in a mixed call the
    streams at 1/1 produce the bytes they produce in a batch with no resampled stream"""
    pkg = package()
    assert pkg.launch_count(COUNTER, lib) >= 0, "the library has no %s counter" % COUNTER
    nin, nr, nout = clip_case(lib)
    S, Cn = len(nin), 2
    frames, _ = clip_inputs(fc.S16, nin)
    a, b, m = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(3))
    b.set_pcm_resample(160, 147)                                                   # (the twin had a ratio once: 1/1 turns the stage off again)
    b.set_pcm_resample(1, 1)
    outs, deltas = [], []
    for batch in (a, b):
        before = _counts(lib)
        out, ok = batch.exactFrames(to_memory(frames), nout, in_samples=nin)
        batch.synchronize()
        outs.append(to_host(out))
        deltas.append([y - x for x, y in zip(before, _counts(lib))])
    assert np.array_equal(outs[0], outs[1]) and deltas[0] == deltas[1] and deltas[0][COUNTERS.index(COUNTER)] == 0 and deltas[0][COUNTERS.index("clip_in")] == 1
    set_ratios(m)
    n_out = [(-1 if s == LEFT else n) for s, n in enumerate(nout)]
    before = _counts(lib)
    mixed, ok = m.exactFrames(to_memory(frames), n_out, in_samples=nin)
    mixed = to_host(mixed)
    delta = dict(zip(COUNTERS, [y - x for x, y in zip(before, _counts(lib))]))
    assert delta[COUNTER] == 1 and delta["clip_in"] == 2
    assert n_out[PLAIN] == nout[PLAIN] and ok[PLAIN] and np.array_equal(mixed[PLAIN, :nout[PLAIN]], outs[0][PLAIN, :nout[PLAIN]]) and mixed[PLAIN].any()
    for batch in (a, b, m):
        batch.close()


def check_steady_state(lib, to_memory=lambda a: a):
    """after the first call the allocation events and the workspace bytes stand still over three more calls of the same shapes; setting a
    ratio that already has a table allocates nothing"""
    pkg = package()
    nin, nr, nout = clip_case(lib)
    frames = to_memory(clip_inputs(fc.S16, nin)[0])
    b = pkg.StretchBatch(len(nin), 2, lib=lib, seed=3, **pc.GEOMETRY)
    plain = b.workspaceBytes()
    set_ratios(b)
    assert b.workspaceBytes() > plain                                              # (the tables are in device memory from the setter on)
    for _ in range(2):
        b.exactFrames(frames, nout, in_samples=nin)
    b.synchronize()
    events, grown = b.allocation_events(), b.workspaceBytes()
    for _ in range(3):
        b.exactFrames(frames, nout, in_samples=nin)
    b.synchronize()
    assert (b.allocation_events(), b.workspaceBytes()) == (events, grown)
    b.set_pcm_resample(320, 294, stream=PLAIN)                                     # (160/147, which stream 0 has)
    assert (b.allocation_events(), b.workspaceBytes()) == (events, grown) and b.pcm_resample(PLAIN) == (160, 147)
    b.close()


def run_clips(lib, fmt=fc.S24):
    pkg = package()
    nin, nr, nout = clip_case(lib)
    frames, _ = clip_inputs(fmt, nin)
    b = pkg.StretchBatch(len(nin), 2, lib=lib, seed=3, **pc.GEOMETRY)
    set_ratios(b)
    res = []
    for _ in range(2):
        out, ok = b.exactFrames(frames, nout, in_samples=nin)
        res.append((np.array(out, copy=True), ok))
    b.close()
    return res


def check_reproducible(lib):
    """two runs of the same call are bit-identical, and so are two batches"""
    (a0, ok0), (a1, ok1) = run_clips(lib)
    (b0, okb), _ = run_clips(lib)
    assert np.array_equal(a0, a1) and np.array_equal(a0, b0) and ok0.tolist() == ok1.tolist() == okb.tolist() and a0.any()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def _refused(lib, rc, *words):
    msg = lib.smst_last_error() or b""
    assert rc == ERR_INVALID and all(w in msg for w in words), (rc, msg)


def check_refusals(lib, to_memory=lambda a: a):
    pkg = package()
    import ctypes as C
    S, Cn = 10, 2
    b = pkg.StretchBatch(S, Cn, lib=lib, **pc.GEOMETRY)
    for up, down, word in ((0, 1, b"640"), (1, 0, b"640"), (-3, 2, b"640"), (641, 640, b"640"), (640, 641, b"640"), (1283, 1281, b"640"), (2, 10, b"4.5"), (1, 5, b"4.5"), (6, 1, b"4.5")):
        _refused(lib, lib.smst_batch_set_pcm_resample(b.h, 0, up, down), word)
    for stream in (-2, S):
        _refused(lib, lib.smst_batch_set_pcm_resample(b.h, stream, 2, 1), b"stream")
    for stream in (-1, S):
        _refused(lib, lib.smst_batch_pcm_resample(b.h, stream, None, None), b"stream")
        _refused(lib, lib.smst_batch_resampled_length(b.h, stream, 100), b"stream")
    _refused(lib, lib.smst_batch_set_pcm_resample(None, 0, 2, 1), b"null")
    _refused(lib, lib.smst_batch_pcm_resample(None, 0, None, None), b"null")
    _refused(lib, lib.smst_batch_resampled_length(None, 0, 100), b"null")
    assert [b.pcm_resample(s) for s in range(S)] == [(1, 1)]*S                      # (a refused call changes nothing)
    assert lib.smst_batch_set_pcm_resample(b.h, 0, 1280, 1176) == 0 and b.pcm_resample(0) == (160, 147)   # (reduced first, then checked)
    assert lib.smst_batch_set_pcm_resample(b.h, 1, 9, 2) == 0 and lib.smst_batch_set_pcm_resample(b.h, 2, 2, 9) == 0
    b.set_pcm_resample(1, 1)
    # the ninth ratio, and the slot freed after a ratio is dropped
    for s, (up, down) in enumerate(RATIOS):
        b.set_pcm_resample(up, down, stream=s)
    _refused(lib, lib.smst_batch_set_pcm_resample(b.h, 8, 4, 3), b"8")
    _refused(lib, lib.smst_batch_set_pcm_resample(b.h, 9, 5, 4), b"8")
    assert b.pcm_resample(8) == b.pcm_resample(9) == (1, 1)
    b.set_pcm_resample(2, 1, stream=8)                                              # (a ratio that is live: no new slot)
    b.set_pcm_resample(1, 1, stream=3)                                              # 2/3 dropped: its slot is free
    b.set_pcm_resample(4, 3, stream=9)
    assert b.pcm_resample(9) == (4, 3)
    _refused(lib, lib.smst_batch_set_pcm_resample(b.h, 3, 2, 3), b"8")
    b.set_pcm_resample(5, 4, stream=9)                                              # (the stream's own ratio goes as the new one comes)
    b.set_pcm_resample(7, 8)                                                        # every stream: all eight go
    assert [b.pcm_resample(s) for s in range(S)] == [(7, 8)]*S
    # Nr that does not fit an int, without the clip
    b.set_pcm_resample(9, 2, stream=0)
    assert b.resampled_length(0, 477218588) == 2147483646 and b.resampled_length(1, 8) == 7 and b.resampled_length(0, 0) == 0
    _refused(lib, lib.smst_batch_resampled_length(b.h, 0, 477218589), b"2147483647")
    _refused(lib, lib.smst_batch_resampled_length(b.h, 0, 1 << 62), b"2147483647")
    _refused(lib, lib.smst_batch_resampled_length(b.h, 0, -1), b"negative")
    b.close()
    # the planar exact and the three streaming calls with a resampled stream taking part
    b = pkg.StretchBatch(3, Cn, lib=lib, **pc.GEOMETRY)
    b.set_pcm_resample(3, 2, stream=1)
    frames = to_memory(np.zeros((3, 2000, Cn), np.int16))
    planar = to_memory(np.zeros((3, Cn, 2000), np.float32))
    for call in (lambda: b.exact(planar, [2400, 2400, 2400]), lambda: b.processFrames(frames, [600, 600, 600]), lambda: b.seekFrames(frames, [1.0, 1.0, 1.0]),
                 lambda: b.outputSeekFrames(frames)):
        with dc.pytest_raises(pkg.StretchError) as e:
            call()
        assert "resample" in str(e.value) and "smst_batch_exact_pcm only" in str(e.value) and "error -1" in str(e.value), str(e.value)
    b.exact(planar, [2400, -1, 2400])                                               # (stream 1 takes no part: not refused)
    b.flushFrames([100, 50, 100], like=to_memory(np.zeros((1,), np.float32)))       # (no input: unaffected)
    b.close()
    # smst_resample_ratio
    assert pkg.resample_ratio(44100, 48000, lib=lib) == (160, 147) and pkg.resample_ratio(48000, 44100, lib=lib) == (147, 160)
    assert pkg.resample_ratio(192000, 44100, lib=lib) == (147, 640) and pkg.resample_ratio(44100, 192000, lib=lib) == (640, 147)
    assert pkg.resample_ratio(48000, 48000, lib=lib) == (1, 1)
    up, down = C.c_int(0), C.c_int(0)
    _refused(lib, lib.smst_resample_ratio(8000.0, 48000.0, C.byref(up), C.byref(down)), b"4.5")
    _refused(lib, lib.smst_resample_ratio(44100.5, 48000.0, C.byref(up), C.byref(down)), b"integer")
    _refused(lib, lib.smst_resample_ratio(0.0, 48000.0, C.byref(up), C.byref(down)), b"integer")
    _refused(lib, lib.smst_resample_ratio(44100.0, -48000.0, C.byref(up), C.byref(down)), b"integer")
    _refused(lib, lib.smst_resample_ratio(44100.0, 44101.0, C.byref(up), C.byref(down)), b"640")
    _refused(lib, lib.smst_debug_resample_taps(641, 1, None, None), b"640")
    assert (MAX_TERM, MAX_RATIOS, TILE) == (pkg.RESAMPLE_MAX_TERM, pkg.RESAMPLE_MAX_RATIOS, pkg.RESAMPLE_TILE)


# ---- the command-line tool -----------------------------------------------------------------------------------------------------------

def check_cli(cli, tmp_path, lib):
    """three short files at 44.1, 48 and 96 kHz through --exact --rate=48000 --time=1.25: written at 48 kHz, round(Nr*1.25) frames long and
    equal, byte for byte, to what the Python binding gives for the same clips; --rate without --exact fails with its message"""
    from test_cli import write_wav16
    pkg = package()
    rates, lengths, Cn = (44100, 48000, 96000), (22050, 24000, 48001), 2      # (half a second each: the tool runs the default preset at 48 kHz)
    srcs = [str(tmp_path/("in%d.wav" % k)) for k in range(3)]
    outs = [str(tmp_path/("out%d.wav" % k)) for k in range(3)]
    for k in range(3):
        write_wav16(srcs[k], 0.8*synth_input(k, Cn, lengths[k], rates[k]), rates[k])
    args = [a for pair in zip(srcs, outs) for a in pair]
    res = subprocess.run([cli, "--exact", "--rate=48000", "--time=1.25"] + args, capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    ratios = [pkg.resample_ratio(r, 48000, lib=lib) for r in rates]
    assert ratios == [(160, 147), (1, 1), (1, 2)]
    for k in range(3):
        assert "%d Hz" % rates[k] in res.stdout and "%d/%d" % ratios[k] in res.stdout, res.stdout
    frames = np.zeros((3, max(lengths), Cn), np.int16)
    for k in range(3):
        frames[k, :lengths[k]] = np.frombuffer(dc.data_chunk(srcs[k])[1], "<i2").reshape(-1, Cn)
    b = pkg.StretchBatch(3, Cn, lib=lib, preset="default", sample_rate=48000)
    b.setTransposeSemitones(0.0, 8000.0/48000)                                      # (the tool's defaults)
    b.setFormantSemitones(0.0)
    b.setFormantBase(100.0/48000)
    for k in range(3):
        b.set_pcm_resample(*ratios[k], stream=k)
    nr = [b.resampled_length(k, lengths[k]) for k in range(3)]
    nout = [int(round(n*1.25)) for n in nr]
    want, ok = b.exactFrames(frames, nout, in_samples=list(lengths))
    b.close()
    assert ok.all()
    for k in range(3):
        head, data = dc.data_chunk(outs[k])
        assert head[:3] == (1, Cn, 48000) and len(data) == nout[k]*Cn*2, (k, head, len(data), nout[k])
        assert data == np.ascontiguousarray(want[k, :nout[k]]).astype("<i2").tobytes(), k
    res = subprocess.run([cli, "--rate=48000", "--time=1.25"] + args, capture_output=True, text=True)
    assert res.returncode == 2 and "--exact" in res.stderr, (res.returncode, res.stderr)
