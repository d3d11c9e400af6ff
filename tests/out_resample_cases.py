"""Shared cases of the sample-rate converter behind the engine in smst_batch_exact_pcm (include/smst.h, "Output resample"):
test_out_resample_emu.py runs them on the CPU stand-in, test_out_resample_gpu.py on the device.

The mirror is resample_cases' mirror -- the header's arithmetic restated in numpy, bit for bit given the library's own table -- applied to
the first E rendered frames and cut to the Nd delivered ones.  Nothing here is a tolerance: every comparison is of bit patterns or bytes."""
import math
import subprocess

import numpy as np

import dither_cases as dc
import exact_cases as xc
import level_cases as lc
import limiter_cases as lm
import loudness_cases as ld
import loudness_range_cases as lr
import pcm_cases as pc
import pcm_format_cases as fc
import resample_cases as rs
from conftest import package, synth_input
from resample_cases import TILE, lengths_for, library_taps, mirror, same_floats

COUNTER = "clip_resample_out"
COUNTERS = rs.COUNTERS + (COUNTER,)
RATIOS = rs.RATIOS
ERR_INVALID = -1


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def render_length(nd, up, down):
    """E: the smallest count of rendered frames that holds the centre (n*M)//L of every delivered frame n < nd"""
    L, M = rs.reduced(up, down)
    return ((nd - 1)*M)//L + 1


def out_mirror(r, nd, up, down, table):
    """r float32 [..., >= E] -> float32 [..., nd]: "Resample" of the clip r[..., :E], whose right edge meets zeros at E, cut to nd frames"""
    E = render_length(nd, up, down)
    r = np.asarray(r, np.float32)
    assert r.shape[-1] >= E
    y = mirror(r[..., :E], up, down, table)
    assert y.shape[-1] >= nd
    return np.ascontiguousarray(y[..., :nd])


def check_mirror():
    """the known answers of include/smst.h on the formula's table, and what defines E, for every ratio of RATIOS and Nd = 1 ... 3000"""
    # (147/160, Nd = 441: the definition gives 440*160//147 + 1 = 479.  480 = ceil(441*160/147) is "Resample"'s Nr of the inverse direction, and
    # it would break (Nd - 1)*M//L == E - 1, which is asserted below for every Nd.)
    assert render_length(8, 3, 2) == 5 and render_length(5, 2, 3) == 7 and render_length(441, 147, 160) == 479 and render_length(480, 160, 147) == 441
    r = np.zeros(5, np.float32); r[2] = 1
    got = out_mirror(r, 8, 3, 2, rs.formula_taps(3, 2))
    assert rs._hex(got) == "bca067e3 be4717b5 3ed8327b 3f7ae0ea 3ed8327b be4717b5 bca067e3 3dddb185", rs._hex(got)
    r = np.zeros(7, np.float32); r[3] = 1
    got = out_mirror(r, 5, 2, 3, rs.formula_taps(2, 3))
    assert rs._hex(got) == "bc55dff0 3c594cd8 3f2740ad 3c594cd8 bc55dff0", rs._hex(got)
    for up, down in RATIOS:
        L, M = rs.reduced(up, down)
        for nd in range(1, 3001):
            E = render_length(nd, L, M)
            assert E >= 1 and ((nd - 1)*M)//L == E - 1 and -((-E*L)//M) >= nd, (up, down, nd, E)
            assert E == 1 or ((nd - 1)*M)//L > E - 2                                  # (no smaller count holds frame nd - 1's centre)


# ---- lengths -------------------------------------------------------------------------------------------------------------------------

def check_lengths(lib):
    """smst_batch_pcm_out_render_length against the formula, per ratio; Nd itself at 1/1; an Nd whose E does not fit an int is refused"""
    pkg = package()
    b = pkg.StretchBatch(len(RATIOS) + 1, 1, lib=lib, **pc.GEOMETRY)
    for s, (up, down) in enumerate(RATIOS):
        b.set_pcm_out_resample(up, down, stream=s)
        assert b.pcm_out_resample(s) == rs.reduced(up, down)
        for nd in list(range(1, 3001, 7)) + [2999, 3000, 1 << 20, (1 << 20) + 1]:
            assert b.out_render_length(s, nd) == render_length(nd, up, down), (up, down, nd)
        assert b.out_render_length(s, 0) == 0
    plain = len(RATIOS)
    assert b.pcm_out_resample(plain) == (1, 1) and [b.out_render_length(plain, n) for n in (0, 1, 77, 2147483647)] == [0, 1, 77, 2147483647]
    b.set_pcm_out_resample(2, 9, stream=0)                                            # E = (Nd - 1)*9//2 + 1
    assert b.out_render_length(0, 477218588) == 2147483642 and b.out_render_length(0, 477218589) == 2147483647
    _refused(lib, lib.smst_batch_pcm_out_render_length(b.h, 0, 477218590), b"2147483647")
    _refused(lib, lib.smst_batch_pcm_out_render_length(b.h, 0, 1 << 62), b"2147483647")
    _refused(lib, lib.smst_batch_pcm_out_render_length(b.h, 0, -1), b"negative")
    b.close()


# ---- the kernel against the mirror ---------------------------------------------------------------------------------------------------

SENTINEL = rs.SENTINEL


def _float_buffer(n, offset):
    """n float32 whose first element lies `offset` floats behind a 16-byte boundary"""
    return fc.byte_buffer(4*n, 4*offset).view(np.float32)


def tiles_of(nd, up, down):
    """per tile of TILE delivered frames: (i0, first, end) -- its first frame's centre and the rendered positions [first, end) its taps reach"""
    L, M, H, T = rs.shape_of(up, down)
    out = []
    for n0 in range(0, nd, TILE):
        last = min(n0 + TILE, nd) - 1
        i0, i_last = (n0*M)//L, (last*M)//L
        out.append((i0, i0 - (H - 1), i_last + H + 1))
    return out


def join_classes(nd, k, up, down):
    """which of the join's positions a stream has: at 0, at E, inside the first T frames, inside a tile's span, exactly at a later tile's i0"""
    L, M, H, T = rs.shape_of(up, down)
    E = render_length(nd, up, down)
    found = set()
    if k == 0:
        found.add("zero")
    if k == E:
        found.add("end")
    if 0 < k < min(T, E):
        found.add("early")
    for t, (i0, first, end) in enumerate(tiles_of(nd, up, down)):
        if max(first, 0) < k < min(end, E):
            found.add("straddled")
        if t > 0 and k == i0:
            found.add("tile start")
    return found


def run_kernel(lib, clips, counts, ratios, joins, splits, dst_offsets=(1, 2, 3, 0), src_offset=1, out_offset=0, col_shift=0):
    """clips: per stream float32 [C, E], the rendered frames; counts: per stream Nd; joins: per stream k, the frames of source piece 0;
    splits: per stream the delivered frames of destination segment 0.  The source rows lie at every offset from a 16-byte boundary (a
    channel stride of 1 mod 4), piece 0 at column (s + col_shift) % 4 and piece 1 at a column of its own whose offset differs; NaN fills the
    image around the pieces -- the gap between them, the room behind E --, so a read of it poisons the result.
    -> (out as the hook left it, the expected image: the mirror's frames inside the sentinel)"""
    pkg = package()
    S, Cn = len(clips), clips[0].shape[0]
    E = [render_length(n, *r) for n, r in zip(counts, ratios)]
    assert [c.shape[1] for c in clips] == E
    src = np.zeros((S, 2, 4), np.int32)
    for s in range(S):
        a0 = (s + col_shift) % 4
        b0 = (a0 + joins[s] + 3)//4*4 + 4 + (s + col_shift + 1 + joins[s]) % 4
        src[s, 0] = (a0, 0, joins[s], 0)
        src[s, 1] = (b0, joins[s], E[s] - joins[s], 0)
    in_cs = int((src[:, :, 0] + src[:, :, 2]).max()) + 5
    in_cs += (1 - in_cs) % 4                                                  # (1 mod 4: a stream's rows lie at every offset)
    in_ss = Cn*in_cs + 1
    image = _float_buffer(S*in_ss + 8, src_offset)
    image[:] = np.nan
    col = (max(splits) + 3)//4*4 + 8                                          # destination segment 1's column, a gap of sentinels in front of it
    out_cs = col + max(n - k for n, k in zip(counts, splits)) + 11
    out_ss = Cn*out_cs + 3
    out = _float_buffer(S*out_ss + 8, out_offset)
    out[:] = SENTINEL
    want = np.array(out, copy=True)
    dst = np.zeros((S, 2, 4), np.int32)
    before = pkg.launch_count(COUNTER, lib)
    assert before >= 0, "the library has no %s counter" % COUNTER
    for s in range(S):
        k = joins[s]
        for c in range(Cn):
            row = s*in_ss + c*in_cs
            image[row + src[s, 0, 0]:row + src[s, 0, 0] + k] = clips[s][c, :k]
            image[row + src[s, 1, 0]:row + src[s, 1, 0] + E[s] - k] = clips[s][c, k:]
        off = dst_offsets[s % len(dst_offsets)]
        dst[s, 0] = (0, off, splits[s], 0)
        dst[s, 1] = (splits[s], col + (off + 1) % 4, counts[s] - splits[s], 0)
        if rs.reduced(*ratios[s]) == (1, 1):
            continue
        y = out_mirror(clips[s], counts[s], *ratios[s], library_taps(lib, *ratios[s]))
        for c in range(Cn):
            row = s*out_ss + c*out_cs
            want[row + dst[s, 0, 1]:row + dst[s, 0, 1] + splits[s]] = y[c, :splits[s]]
            want[row + dst[s, 1, 1]:row + dst[s, 1, 1] + counts[s] - splits[s]] = y[c, splits[s]:]
    pkg.debug_clip_resample_out(counts, ratios, Cn, image, in_ss, in_cs, src, dst, out, out_ss, out_cs, lib=lib)
    assert pkg.launch_count(COUNTER, lib) == before + 1
    return out, want


def kernel_case(up, down, channels):
    """-> (Nd, E, k, destination split) per stream: Nd on and beside tile edges and 1, 2, H, T + 1, then three clips for the special
    values; the joins at 0, at E, inside the first T frames, inside a tile's span and exactly at the second tile's first input frame"""
    L, M, H, T = rs.shape_of(up, down)
    counts = [TILE - 1, TILE, TILE + 1, 2*TILE + 1, 1, 2, H, T + 1]
    special = 3*T + 37
    nd_special = max((special*L)//M, 1)                                      # (E is about `special`)
    counts += [nd_special]*3
    E = [render_length(n, L, M) for n in counts]
    i1 = (TILE*M)//L                                                          # the second tile's i0
    joins = [E[0], 0, i1, ((TILE + TILE//2)*M)//L + 1, (channels + 1) % 2, min(1, E[5]), min(max(E[6] - 1, 0), T//2), min(E[7], 5), E[8]//2, E[9]//3, E[10] - 1]
    assert all(0 <= k <= e for k, e in zip(joins, E)), (joins, E)
    found = set()
    for n, k in zip(counts, joins):
        found |= join_classes(n, k, L, M)
    assert found == {"zero", "end", "early", "straddled", "tile start"}, (up, down, found)
    choices = (lambda n: 0, lambda n: n//3, lambda n: TILE if n > TILE else n//2, lambda n: n)
    splits = [choices[(s + channels) % 4](n) for s, n in enumerate(counts)]
    splits[1], splits[3] = min(TILE, counts[1]), min(TILE, counts[3])        # (exactly on a tile edge where the clip reaches it)
    return counts, E, joins, splits


def check_kernel(lib, up, down, channels):
    """one launch per ratio and channel count -- four with two channels, one for each alignment of the source buffer, the output buffer and
    the source columns; with 1, 3 and 16 channels one alignment of those, the rows still at every offset --: noise at full scale, Nd and joins of kernel_case, every destination split, a
    stream of zeros, one with a NaN in the middle, one with +-inf; bit for bit, sentinels kept, no NaN read from around the pieces"""
    L, M, H, T = rs.shape_of(up, down)
    rng = np.random.default_rng(7000*up + 7*down + channels)
    counts, E, joins, splits = kernel_case(up, down, channels)
    clips = [rng.uniform(-1, 1, (channels, e)).astype(np.float32) for e in E]
    zeros, nan, inf = len(E) - 3, len(E) - 2, len(E) - 1
    clips[zeros][:] = 0
    at = E[nan]//2
    clips[nan][0, at] = np.nan
    clips[inf][channels - 1, 5] = np.inf
    clips[inf][0, E[inf] - 9] = -np.inf
    ratios = [(up, down)]*len(clips)
    alignments = ((1, 0, 0), (3, 2, 1), (0, 1, 2), (2, 3, 3)) if channels == 2 else ((2, 1, channels),)
    for src_offset, out_offset, col_shift in alignments:
        got, want = run_kernel(lib, clips, counts, ratios, joins, splits, src_offset=src_offset, out_offset=out_offset, col_shift=col_shift)
        assert same_floats(got, want), (up, down, channels, src_offset, np.flatnonzero(~((rs.bits(got) == rs.bits(want)) | (np.isnan(got) & np.isnan(want))))[:8])
    # exactly the frames whose T taps reach the NaN are NaN: i - (H - 1) <= at <= i + H
    y = out_mirror(clips[nan], counts[nan], up, down, library_taps(lib, up, down))
    i = (np.arange(counts[nan], dtype=np.int64)*M)//L
    reached = (i - (H - 1) <= at) & (at <= i + H)
    assert np.array_equal(np.isnan(y[0]), reached) and reached.any() and not reached.all() and not np.isnan(y[1:]).any(), (up, down)
    assert not out_mirror(clips[zeros], counts[zeros], up, down, library_taps(lib, up, down)).any()
    for s in range(len(E) - 3):
        assert not np.isnan(out_mirror(clips[s], counts[s], up, down, library_taps(lib, up, down))).any()    # (what a NaN in `got` would mean: a sentinel was read)


def check_mixed(lib, channels=2):
    """ten streams with eight different ratios in one launch, two streams at 1/1 among them: their rows of the output stay as they were"""
    rng = np.random.default_rng(78)
    ratios = list(RATIOS[:3]) + [(1, 1)] + list(RATIOS[3:6]) + [(5, 5)] + list(RATIOS[6:])
    counts = [700, 2100, 1500, 900, 3000, 1100, 1300, 640, 1500, 2300]
    E = [render_length(n, *r) for n, r in zip(counts, ratios)]
    clips = [rng.uniform(-1, 1, (channels, e)).astype(np.float32) for e in E]
    joins = [(e*(s + 2))//13 for s, e in enumerate(E)]
    splits = [(n*(s + 1))//11 for s, n in enumerate(counts)]
    got, want = run_kernel(lib, clips, counts, ratios, joins, splits)
    assert same_floats(got, want)
    assert len(set(rs.reduced(*r) for r in ratios) - {(1, 1)}) == 8


# ---- whole clips ---------------------------------------------------------------------------------------------------------------------

OUT_RATIOS = ((147, 160), (1, 1), (2, 1), (2, 3), (640, 147), (3, 2))
IN_RATIOS = ((160, 147), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1))         # stream 0: a 44.1 kHz file through a 48 kHz batch and back
CLIP_FACTORS = (1.25, 0.9, 1.5, 1.5, 1.1, 1.0)
SHORT, LEFT, PLAIN = 2, 5, 1
CLIP_SEED = 67
BATCH_FS = 6000.0                                                             # the batch's rate of the chain test: delivery rates are this times L/M, 4000 Hz
                                                                              # (loudness_range_cases' low rate) at 2/3; the shortest clip still has a 400 ms block


def exact_lengths(probe, frames, E):
    """Batch::exactLengths in its own float32 arithmetic -> (too short?, outputIndex)"""
    rate = np.float32(frames)/np.float32(E)
    seek = probe.outputSeekLength(float(rate))
    if frames < seek:
        return True, 0
    return False, min(max(int(np.float32(E) - np.float32(seek)/rate), 0), E)


_cases = {}


def clip_case(lib, Cn=2):
    """-> (inputs N, the engine's frames (Nr where the stream has an input ratio), delivered Nd, rendered E) of OUT_RATIOS; only stream
    SHORT is too short, and every other stream's join lies strictly inside its rendered clip"""
    if id(lib) in _cases:
        return _cases[id(lib)]
    pkg = package()
    probe = pkg.StretchBatch(1, Cn, lib=lib, **pc.GEOMETRY)
    nin = [4000, 3000, 200, 3500, 2500, 4000]
    frames = [rs.resampled_length(n, *r) for n, r in zip(nin, IN_RATIOS)]
    nd = [int(round(f*t*L/M)) for f, t, (L, M) in zip(frames, CLIP_FACTORS, OUT_RATIOS)]
    E = [render_length(n, *r) for n, r in zip(nd, OUT_RATIOS)]
    for s in range(len(nin)):
        short, k = exact_lengths(probe, frames[s], E[s])
        assert short == (s == SHORT), (s, frames[s], E[s])
        assert short or 0 < k < E[s], (s, k, E[s])
    probe.close()
    assert max(nd) > 2*TILE and rs.reduced(*OUT_RATIOS[PLAIN]) == (1, 1)
    _cases[id(lib)] = (nin, frames, nd, E)
    return _cases[id(lib)]


def set_ratios(batch, out=True):
    for s, (up, down) in enumerate(IN_RATIOS):
        batch.set_pcm_resample(up, down, stream=s)
    if out:
        for s, (up, down) in enumerate(OUT_RATIOS):
            batch.set_pcm_out_resample(up, down, stream=s)
            assert batch.pcm_out_resample(s) == rs.reduced(up, down)


def clip_inputs(fmt, nin, Cn=2):
    """-> (frames of the format [S, max N, C], the same values as F32 frames: what the format's input rule gives)"""
    frames = fc.encode_frames(pc.frames_of(xc.clip_inputs(Cn, nin, loud=0)), fmt)
    return frames, np.ascontiguousarray(fc.decode_frames(frames, fmt).astype(np.float32))


def rendered(lib, twin, f32_frames, nin, E, to_memory, to_host):
    """the twin batch -- no output ratio -- asked for E frames in F32 at gain 1, no dither -> (r planar [S, C, max E], its status)"""
    n_out = [(-1 if s == LEFT else e) for s, e in enumerate(E)]
    out, ok = twin.exactFrames(to_memory(f32_frames), n_out, in_samples=nin)
    return np.ascontiguousarray(np.transpose(to_host(out), (0, 2, 1))), ok


def delivered(lib, r, nd):
    """out_mirror of every stream of OUT_RATIOS -> list of float32 [C, Nd] (r itself at 1/1)"""
    out = []
    for s, (up, down) in enumerate(OUT_RATIOS):
        if rs.reduced(up, down) == (1, 1):
            out.append(np.ascontiguousarray(r[s, :, :nd[s]]))
        else:
            out.append(out_mirror(r[s], nd[s], up, down, library_taps(lib, up, down)))
    return out


def check_clips(lib, fmt, dithered, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True), calls=2):
    """exactFrames of a batch with OUT_RATIOS against a twin batch without them that renders E frames in F32: the bytes are the mirror's
    delivered frames put through the format's own output rule (dithered where the format can be, by the delivered frame's index), byte for
    byte, as are overs, NaNs, peaks and gains; status is the twin's; the bytes behind Nd and the left-out stream keep their fill; on the
    device the second call allocates nothing"""
    pkg = package()
    nin, frames_at, nd, E = clip_case(lib)
    S, Cn, most = len(nin), 2, max(nd)
    frames, f32 = clip_inputs(fmt, nin)
    o, t = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(2))
    set_ratios(o)
    set_ratios(t, out=False)
    modes = [dc.CLIP_MODES[s % len(dc.CLIP_MODES)] if dithered else dc.NONE for s in range(S)]
    for b in (o, t):
        b.set_pcm_level(lc.FIXED, 1.0, 1.0)                                       # (a levelled batch meters peaks)
    if dithered:
        for s in range(S):
            o.setPcmDither(modes[s], CLIP_SEED + s, stream=s)
    assert [o.out_render_length(s, nd[s]) for s in range(S)] == E and [o.resampled_length(s, nin[s]) for s in range(S)] == frames_at
    n_out = [(-1 if s == LEFT else n) for s, n in enumerate(nd)]
    events = None
    for call in range(calls):
        r, ok_t = rendered(lib, t, f32, nin, E, to_memory, to_host)
        want = delivered(lib, r, nd)
        fill = np.full(frames.shape[:1] + (most,) + frames.shape[2:], 0x5A, frames.dtype)
        before = pkg.launch_count(COUNTER, lib)
        got, ok_o = o.exactFrames(to_memory(frames), n_out, in_samples=nin, out=to_memory(fill.copy()))
        got = to_host(got)
        assert pkg.launch_count(COUNTER, lib) == before + 1
        assert ok_o.tolist() == ok_t.tolist() == [s not in (SHORT, LEFT) for s in range(S)], (ok_o.tolist(), ok_t.tolist())
        peaks, gains = o.take_pcm_peaks()
        overs, nans = o.takePcmOvers()
        expect = fill.copy()
        for s in range(S):
            if s == LEFT:
                continue
            x = np.zeros((Cn, nd[s]), np.float32) if s == SHORT else want[s]
            codes, cm, nm = dc.mirror(x, fmt, dc.NONE if s == SHORT else modes[s], CLIP_SEED + s, 0)     # (a too-short stream's zeros are not dithered)
            expect[s, :nd[s]] = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
            assert (int(overs[s]), int(nans[s])) == (int(cm.sum()), int(nm.sum())), (fmt, s, int(overs[s]), int(cm.sum()))
            assert s == SHORT or x.any()
            assert rs.bits(peaks[s]) == rs.bits(lc.peak_of(x)) and rs.bits(gains[s]) == rs.bits(np.float32(1)), (fmt, s, peaks[s], gains[s])
        assert lc.same_bytes(got.reshape(-1).view(np.uint8), expect.reshape(-1).view(np.uint8), fmt), (fmt, dithered, call)
        assert (got[LEFT] == 0x5A).all() and not got[SHORT, :nd[SHORT]].any()
        for s in range(S):
            assert (got[s, nd[s]:] == 0x5A).all(), s                                  # (nothing of the call is sized by E)
        if events is not None:
            assert (o.allocation_events(), o.workspaceBytes()) == events, call        # (the second call allocates nothing)
        events = (o.allocation_events(), o.workspaceBytes())
    for b in (o, t):
        b.close()


# ---- the chain behind the converter --------------------------------------------------------------------------------------------------

CHAIN_TARGET = 6.0                                                            # LUFS: loud enough for the limiter to have work


def check_chain(lib, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True), calls=2):
    """LOUDNESS + true peak + limiter + loudness range on every stream, F32, each stream's DELIVERY rate as sampleRate: the meters are, bit
    for bit, what the existing hooks (debug_clip_loudness, _true_peak, _limit, _loudness_range) report on the image out_mirror(r), and the
    bytes are that image levelled by the gains and the limiter curve those hooks returned -- (v*g)*r, the limited copy's two float32
    multiplies; where the curve is 1 that is smst_debug_clip_copy_levelled's output at the same gains, which is compared as well (the copy
    hook takes no curve)"""
    pkg = package()
    nin, frames_at, nd, E = clip_case(lib)
    S, Cn, most = len(nin), 2, max(nd)
    frames, f32 = clip_inputs(fc.F32, nin)
    o, t = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(2))
    set_ratios(o)
    set_ratios(t, out=False)
    ceil = np.float32(0.25)
    rates = [BATCH_FS*L/M for L, M in OUT_RATIOS]
    for s in range(S):
        o.set_pcm_loudness(CHAIN_TARGET, float(ceil), rates[s], stream=s)
        o.set_pcm_loudness_range(True, rates[s], stream=s)
    o.set_pcm_true_peak(True)
    o.set_pcm_limiter(True)
    H = o.pcm_limiter_lookahead()
    n_out = [(-1 if s == LEFT else n) for s, n in enumerate(nd)]
    running = [s for s in range(S) if s not in (SHORT, LEFT)]
    for call in range(calls):
        r, ok_t = rendered(lib, t, f32, nin, E, to_memory, to_host)
        y = delivered(lib, r, nd)
        fill = np.full((S, most, Cn), 0x5A5A5A5A, np.uint32).view(np.float32)
        got, ok_o = o.exactFrames(to_memory(frames), n_out, in_samples=nin, out=to_memory(fill.copy()))
        got = to_host(got)
        assert ok_o.tolist() == ok_t.tolist() == [s in running for s in range(S)]
        clips = [y[s] for s in running]
        fs = [rates[s] for s in running]
        image, segs, iss, ics = ld.build_image(clips, [x.shape[1] for x in clips], [0]*len(clips), 0)     # (one segment per stream from an aligned column, as the engine's third column)
        blocks_most = max(x.shape[1]//ld.hop(f) for x, f in zip(clips, fs)) + 1
        Z, blocks, gated, g_loud, _ = pkg.debug_clip_loudness(segs, Cn, image, iss, ics, fs, None, CHAIN_TARGET, blocks_most, lib=lib)
        M_, ST, lo, hi, ns, n, g_range, _ = pkg.debug_clip_loudness_range(segs, Cn, image, iss, ics, fs, None, CHAIN_TARGET, None, blocks_most, lib=lib)
        true_peaks, sample_peaks = pkg.debug_clip_true_peak(segs, Cn, image, iss, ics, lib=lib)
        assert np.array_equal(rs.bits(g_loud), rs.bits(g_range))                      # (no caps: the range stage leaves the gain)
        flags = [lm.TRUE_PEAK | lm.LIMITER]*len(clips)
        need, curve, low, limited = pkg.debug_clip_limit(segs, Cn, image, iss, ics, g_loud, [ceil]*len(clips), flags, H, max(x.shape[1] for x in clips), lib=lib)
        lufs_o, blocks_o, gated_o = o.take_pcm_loudness()
        mmax, smax, lra, low_o, high_o, ns_o, n_o = o.take_pcm_loudness_range()
        tp_o = o.take_pcm_true_peaks()
        min_o, limited_o = o.take_pcm_limiter()
        peaks_o, gains_o = o.take_pcm_peaks()
        copied = np.full((len(clips), most, Cn), 0x5A5A5A5A, np.uint32).view(np.float32)
        pkg.debug_clip_copy_levelled(fc.F32, segs, Cn, image, iss, ics, copied.reshape(-1), most*Cn, Cn, [lc.FIXED]*len(clips), g_loud, [ceil]*len(clips),
                                     [dc.NONE]*len(clips), [0]*len(clips), lib=lib)
        expect = fill.copy()
        expect[SHORT, :nd[SHORT]] = 0                                                 # (a too-short stream gets Nd zeros)
        for j, s in enumerate(running):
            where = dict(call=call, stream=s)
            assert (int(blocks_o[s]), int(gated_o[s])) == (int(blocks[j]), int(gated[j])) and lufs_o[s] == lr.lufs_of(Z[j]) and math.isfinite(lufs_o[s]), (where, lufs_o[s], Z[j])
            assert (int(ns_o[s]), int(n_o[s])) == (int(ns[j]), int(n[j])), where
            assert (mmax[s], smax[s]) == (lr.lufs_of(M_[j]), lr.lufs_of(ST[j])), (where, mmax[s], M_[j])
            if n[j] > 0:
                assert (low_o[s], high_o[s], lra[s]) == (lr.lufs_of(lo[j]), lr.lufs_of(hi[j]), 10*math.log10(hi[j]/lo[j])), where
            assert rs.bits(tp_o[s]) == rs.bits(true_peaks[j]) and rs.bits(peaks_o[s]) == rs.bits(sample_peaks[j]), (where, tp_o[s], true_peaks[j])
            assert rs.bits(gains_o[s]) == rs.bits(g_loud[j]), (where, gains_o[s], g_loud[j])
            assert rs.bits(min_o[s]) == rs.bits(low[j]) and int(limited_o[s]) == int(limited[j]), (where, min_o[s], low[j], limited_o[s], limited[j])
            rr = curve[j, :nd[s]]
            expect[s, :nd[s]] = lm.limited(y[s], g_loud[j], rr).T
            idle = rr == 1
            assert np.array_equal(rs.bits(got[s, :nd[s]][idle]), rs.bits(copied[j, :nd[s]][idle])), where
        assert (limited_o[running] > 0).any() and (blocks_o[running] > 0).all()      # (the limiter did work, every clip had a block to measure)
        assert np.array_equal(got.view(np.uint32), expect.view(np.uint32)), call
    for b in (o, t):
        b.close()


# ---- opt-in, steady state, reproducible ----------------------------------------------------------------------------------------------

def _counts(lib):
    pkg = package()
    return [pkg.launch_count(k, lib) for k in COUNTERS]


def check_opt_in(lib, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """a batch that never sets an output ratio against one that set it and then set 1/1: the same bytes, the same launches, none of
    clip_resample_out; in a mixed call the stream at 1/1 has the bytes of the plain batch and clip_resample_out moves by exactly 1"""
    pkg = package()
    assert pkg.launch_count(COUNTER, lib) >= 0, "the library has no %s counter" % COUNTER
    nin, frames_at, nd, E = clip_case(lib)
    S, Cn = len(nin), 2
    frames, _ = clip_inputs(fc.S16, nin)
    a, b, m = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(3))
    b.set_pcm_out_resample(147, 160)                                              # (the twin had a ratio once: 1/1 turns the stage off again)
    b.set_pcm_out_resample(1, 1)
    plain_out = [max(int(round(n*f)), 1) for n, f in zip(nin, CLIP_FACTORS)]
    plain_out[PLAIN] = nd[PLAIN]
    outs, deltas = [], []
    for batch in (a, b):
        before = _counts(lib)
        out, ok = batch.exactFrames(to_memory(frames), plain_out, in_samples=nin)
        batch.synchronize()
        outs.append(to_host(out))
        deltas.append([y - x for x, y in zip(before, _counts(lib))])
    assert np.array_equal(outs[0], outs[1]) and deltas[0] == deltas[1] and deltas[0][COUNTERS.index(COUNTER)] == 0 and deltas[0][COUNTERS.index("clip_out")] == 1
    for s, (up, down) in enumerate(OUT_RATIOS):
        m.set_pcm_out_resample(up, down, stream=s)
    n_out = [(-1 if s == LEFT else n) for s, n in enumerate(nd)]
    before = _counts(lib)
    mixed, ok = m.exactFrames(to_memory(frames), n_out, in_samples=nin)
    mixed = to_host(mixed)
    delta = dict(zip(COUNTERS, [y - x for x, y in zip(before, _counts(lib))]))
    assert delta[COUNTER] == 1 and delta["clip_out"] == 1 and delta["clip_in"] == 1 and delta["clip_resample"] == 0, delta
    assert ok[PLAIN] and np.array_equal(mixed[PLAIN, :nd[PLAIN]], outs[0][PLAIN, :nd[PLAIN]]) and mixed[PLAIN].any()
    for batch in (a, b, m):
        batch.close()


def check_steady_state(lib, to_memory=lambda a: a):
    """after the first calls the allocation events and the workspace bytes stand still over three more calls of the same shapes; an output
    ratio that an input setting already loaded allocates nothing; a ninth distinct ratio across the three settings is refused, and the slot
    is free again when its last user has left"""
    pkg = package()
    nin, frames_at, nd, E = clip_case(lib)
    frames = to_memory(clip_inputs(fc.S16, nin)[0])
    b = pkg.StretchBatch(len(nin), 2, lib=lib, seed=3, **pc.GEOMETRY)
    plain = b.workspaceBytes()
    set_ratios(b)
    assert b.workspaceBytes() > plain                                              # (the tables are in device memory from the setter on)
    for _ in range(2):
        b.exactFrames(frames, nd, in_samples=nin)
    b.synchronize()
    events, grown = b.allocation_events(), b.workspaceBytes()
    for _ in range(3):
        b.exactFrames(frames, nd, in_samples=nin)
    b.synchronize()
    assert (b.allocation_events(), b.workspaceBytes()) == (events, grown)
    b.set_pcm_out_resample(320, 294, stream=PLAIN)                                 # (160/147, which stream 0's input setting has)
    assert (b.allocation_events(), b.workspaceBytes()) == (events, grown) and b.pcm_out_resample(PLAIN) == (160, 147)
    b.close()
    # eight slots for the three settings together
    b = pkg.StretchBatch(10, 1, lib=lib, **pc.GEOMETRY)
    for s, (up, down) in enumerate(RATIOS):                                        # three by the input setting, two by the streaming one, three by the output one
        (b.set_pcm_resample if s < 3 else b.set_pcm_stream_resample if s < 5 else b.set_pcm_out_resample)(up, down, stream=s)
    _refused(lib, lib.smst_batch_set_pcm_out_resample(b.h, 8, 4, 3), b"8")
    _refused(lib, lib.smst_batch_set_pcm_resample(b.h, 8, 4, 3), b"8")
    assert b.pcm_out_resample(8) == (1, 1)
    b.set_pcm_out_resample(*RATIOS[0], stream=8)                                   # (a ratio that is live: no new slot)
    b.set_pcm_resample(1, 1, stream=0)                                             # ... and now stream 8's output setting alone holds it
    _refused(lib, lib.smst_batch_set_pcm_out_resample(b.h, 9, 4, 3), b"8")
    b.set_pcm_out_resample(1, 1, stream=8)                                         # the last user leaves: the slot is free
    b.set_pcm_out_resample(4, 3, stream=9)
    assert b.pcm_out_resample(9) == (4, 3) and b.pcm_out_resample(8) == (1, 1)
    _refused(lib, lib.smst_batch_set_pcm_stream_resample(b.h, 0, *RATIOS[0]), b"8")
    b.close()


def run_clips(lib, fmt=fc.S24):
    pkg = package()
    nin, frames_at, nd, E = clip_case(lib)
    frames, _ = clip_inputs(fmt, nin)
    b = pkg.StretchBatch(len(nin), 2, lib=lib, seed=3, **pc.GEOMETRY)
    set_ratios(b)
    res = []
    for _ in range(2):
        out, ok = b.exactFrames(frames, nd, in_samples=nin)
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
    S, Cn = 3, 2
    b = pkg.StretchBatch(S, Cn, lib=lib, **pc.GEOMETRY)
    for up, down, word in ((0, 1, b"640"), (1, 0, b"640"), (-3, 2, b"640"), (641, 640, b"640"), (640, 641, b"640"), (1283, 1281, b"640"), (2, 10, b"4.5"), (1, 5, b"4.5"), (6, 1, b"4.5")):
        _refused(lib, lib.smst_batch_set_pcm_out_resample(b.h, 0, up, down), word)
    for stream in (-2, S):
        _refused(lib, lib.smst_batch_set_pcm_out_resample(b.h, stream, 2, 1), b"stream")
    for stream in (-1, S):
        _refused(lib, lib.smst_batch_pcm_out_resample(b.h, stream, None, None), b"stream")
        _refused(lib, lib.smst_batch_pcm_out_render_length(b.h, stream, 100), b"stream")
    _refused(lib, lib.smst_batch_set_pcm_out_resample(None, 0, 2, 1), b"null")
    _refused(lib, lib.smst_batch_pcm_out_resample(None, 0, None, None), b"null")
    _refused(lib, lib.smst_batch_pcm_out_render_length(None, 0, 100), b"null")
    assert [b.pcm_out_resample(s) for s in range(S)] == [(1, 1)]*S                  # (a refused call changes nothing)
    assert lib.smst_batch_set_pcm_out_resample(b.h, 0, 1280, 1176) == 0 and b.pcm_out_resample(0) == (160, 147)   # (reduced first, then checked)
    b.set_pcm_out_resample(1, 1)
    # the planar exact, process_pcm and flush_pcm with an out-resampled stream taking part
    b.set_pcm_out_resample(3, 2, stream=1)
    frames = to_memory(np.zeros((S, 2000, Cn), np.int16))
    planar = to_memory(np.zeros((S, Cn, 2000), np.float32))
    like = to_memory(np.zeros((1,), np.float32))
    for call in (lambda: b.exact(planar, [2400, 2400, 2400]), lambda: b.processFrames(frames, [600, 600, 600]), lambda: b.flushFrames([100, 50, 100], like=like)):
        with dc.pytest_raises(pkg.StretchError) as e:
            call()
        assert "output resample" in str(e.value) and "smst_batch_exact_pcm only" in str(e.value) and "error -1" in str(e.value), str(e.value)
    b.exact(planar, [2400, -1, 2400])                                               # (stream 1 takes no part: not refused)
    b.flushFrames([100, -1, 100], like=like)
    b.seekFrames(frames, [1.0, 1.0, 1.0])                                           # (no output: unaffected)
    b.outputSeekFrames(frames)
    b.set_pcm_out_resample(1, 1, stream=1)
    b.processFrames(frames, [600, 600, 600])                                        # (1/1 again: served)
    b.close()


# ---- the command-line tool -----------------------------------------------------------------------------------------------------------

def check_cli(cli, tmp_path, lib):
    """two short files at 44.1 and 48 kHz through --exact --rate=48000 --out-rate=source --time=1.25: each written at its own rate,
    round(N*1.25) frames long and equal, byte for byte, to what the Python binding gives for the same settings; the two printed lines;
    --out-rate without --rate fails with its message"""
    from test_cli import write_wav16
    pkg = package()
    rates, lengths, Cn = (44100, 48000), (22052, 24000), 2                          # (half a second each: the tool runs the default preset at 48 kHz; N*1.25 is whole)
    srcs = [str(tmp_path/("in%d.wav" % k)) for k in range(2)]
    outs = [str(tmp_path/("out%d.wav" % k)) for k in range(2)]
    for k in range(2):
        write_wav16(srcs[k], 0.8*synth_input(k, Cn, lengths[k], rates[k]), rates[k])
    args = [a for pair in zip(srcs, outs) for a in pair]
    res = subprocess.run([cli, "--exact", "--rate=48000", "--out-rate=source", "--time=1.25"] + args, capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    in_ratios = [pkg.resample_ratio(r, 48000, lib=lib) for r in rates]
    out_ratios = [pkg.resample_ratio(48000, r, lib=lib) for r in rates]
    assert in_ratios == [(160, 147), (1, 1)] and out_ratios == [(147, 160), (1, 1)]
    for k in range(2):
        assert "out-resample: %s 48000 Hz -> %d Hz ratio=%d/%d\n" % ((srcs[k], rates[k]) + out_ratios[k]) in res.stdout, res.stdout
        assert "resample: %s %d Hz -> 48000 Hz ratio=%d/%d\n" % ((srcs[k], rates[k]) + in_ratios[k]) in res.stdout, res.stdout
    frames = np.zeros((2, max(lengths), Cn), np.int16)
    for k in range(2):
        frames[k, :lengths[k]] = np.frombuffer(dc.data_chunk(srcs[k])[1], "<i2").reshape(-1, Cn)
    b = pkg.StretchBatch(2, Cn, lib=lib, preset="default", sample_rate=48000)
    b.setTransposeSemitones(0.0, 8000.0/48000)                                      # (the tool's defaults)
    b.setFormantSemitones(0.0)
    b.setFormantBase(100.0/48000)
    for k in range(2):
        b.set_pcm_resample(*in_ratios[k], stream=k)
        b.set_pcm_out_resample(*out_ratios[k], stream=k)
    nout = [int(round(n*1.25)) for n in lengths]
    want, ok = b.exactFrames(frames, nout, in_samples=list(lengths))
    b.close()
    assert ok.all()
    for k in range(2):
        head, data = dc.data_chunk(outs[k])
        assert head[:3] == (1, Cn, rates[k]) and len(data) == nout[k]*Cn*2, (k, head, len(data), nout[k])
        assert data == np.ascontiguousarray(want[k, :nout[k]]).astype("<i2").tobytes(), k
    res = subprocess.run([cli, "--exact", "--out-rate=source", "--time=1.25"] + args, capture_output=True, text=True)
    assert res.returncode == 2 and "--rate" in res.stderr, (res.returncode, res.stderr)
