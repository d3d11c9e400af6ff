"""Shared cases of the sample-rate converter's streaming form behind smst_batch_process_pcm / _flush_pcm (include/smst.h, "Stream output
resample"): test_stream_out_resample_emu.py runs them on the CPU stand-in, test_stream_out_resample_gpu.py on the device.

The mirror is resample_cases.mirror -- the clip converter's restatement -- plus stream_out_mirror, a streaming model that reads only "the
line of LINE rendered frames + the call's rendered frames" and keeps `delivered` as a Python integer (positions as int64 arrays).
Everything is compared bit for bit: a product of two float32 values is exact in float64 and both sides add in the order j = 0 ... T - 1.
The signal checks read the library's own table through smst_debug_resample_taps, as resample_cases does."""
import numpy as np

import dither_cases as dc
import level_cases as lc
import limiter_cases as lm
import pcm_cases as pc
import pcm_format_cases as fc
import resample_cases as rs
import stream_limiter_cases as sl
import stream_meter_cases as sm
import stream_resample_cases as sr
from conftest import package, synth_input

COUNTER, COPY = "pcm_stream_resample_out", "pcm_stream_resample_out_copy"
OLD_COUNTERS = sr.COUNTERS + ("pcm_stream_meter", "pcm_stream_meter_read", "pcm_stream_meter_scan", "clip_resample_out")
COUNTERS = OLD_COUNTERS + (COUNTER, COPY)
TILE = rs.TILE
LINE = 296                                                                   # floats of a channel's carried line (kStreamResampleOutLine)
SENTINEL = rs.SENTINEL
ERR_INVALID = -1
LATENCIES = {(2, 1): 64, (1, 2): 32, (3, 2): 48, (2, 3): 32, (160, 147): 35, (147, 160): 33, (147, 640): 33, (640, 147): 140}
ANSWER_3_2 = "bca067e3 be4717b5 3ed8327b 3f7ae0ea 3ed8327b be4717b5 bca067e3 3dddb185"
ANSWER_2_3 = "bc55dff0 3c594cd8 3f2740ad 3c594cd8 bc55dff0"


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def due(delivered, L, M):
    """ceil(delivered*M/L): the frames rendered once `delivered` frames have been delivered"""
    return (delivered*M + L - 1)//L


def latency_of(up, down):
    """Dl = ceil(H*L/M)"""
    L, M, H, T = rs.shape_of(up, down)
    return (H*L + M - 1)//M


def render_of_call(delivered, nd, up, down):
    """E of a call that delivers nd frames behind `delivered`"""
    L, M, H, T = rs.shape_of(up, down)
    return due(delivered + nd, L, M) - due(delivered, L, M)


def line_bound(up, down):
    """T + ceil(M/L): how far below ceil(delivered*M/L) a call's first frame may reach"""
    L, M, H, T = rs.shape_of(up, down)
    return T + (M + L - 1)//L


def stream_out_mirror(r, cuts, up, down, table, delivered0=0):
    """r float32 [..., E total]: the frames rendered, in order; cuts: the calls' delivered counts (negative: no part); delivered0: the line
    starts as zeros at that position -> the delivered frames of each call, float32 [..., Nd].  A call reads the line and the frames rendered
    in it, nothing else"""
    L, M, H, T = rs.shape_of(up, down)
    Dl = latency_of(up, down)
    assert table.shape == (L, T) and table.dtype == np.float32 and line_bound(up, down) <= LINE
    r = np.asarray(r, np.float32)
    c = table.astype(np.float64)
    line = np.zeros(r.shape[:-1] + (LINE,), np.float32)
    delivered, pos, outs = int(delivered0), 0, []
    for n in cuts:
        n = max(int(n), 0)
        first = due(delivered, L, M)
        E = due(delivered + n, L, M) - first
        window = np.concatenate([line, r[..., pos:pos + E]], axis=-1)                   # the positions first - LINE ... first + E - 1
        assert window.shape[-1] == LINE + E, "the rendered frames handed are fewer than the calls consume"
        at = delivered + np.arange(n, dtype=np.int64)
        live = at >= Dl
        m = at[live] - Dl
        i, p = (m*M)//L, (m*M) % L
        base = i - (H - 1) - (first - LINE)
        if m.size:
            assert first - (i.min() - (H - 1)) <= line_bound(up, down), (delivered, n, up, down)   # (never below the line ...)
            assert base.min() >= 0 and base.max() + T - 1 < window.shape[-1], (delivered, n, E)       # (... never past what has been rendered)
        w = window.astype(np.float64)
        y = np.zeros(r.shape[:-1] + (m.size,), np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(T):
                y = y + c[p, j]*w[..., base + j]
            out = np.zeros(r.shape[:-1] + (n,), np.float32)                             # (the frames below Dl: +0.0)
            out[..., live] = y.astype(np.float32)
        outs.append(out)
        if n > 0:
            line = np.ascontiguousarray(window[..., window.shape[-1] - LINE:])
        delivered, pos = delivered + n, pos + E
    return outs


def rendered_total(cuts, up, down, delivered0=0):
    L, M, H, T = rs.shape_of(up, down)
    total = sum(max(int(n), 0) for n in cuts)
    return due(delivered0 + total, L, M) - due(delivered0, L, M)


def model_cuts(up, down, n):
    Dl = latency_of(up, down)
    head = [1, 0, 5, Dl - 7, 2, Dl, 3]
    assert n > sum(head)
    return head + [n - sum(head)]


def check_mirror():
    """the known answers of include/smst.h; the model against the clip mirror, shifted by Dl, for every ratio and several cuts; the line
    bound T + ceil(M/L) for every table ratio"""
    for q, Dl in LATENCIES.items():
        assert latency_of(*q) == Dl, (q, latency_of(*q))
    assert set(LATENCIES) == set(rs.RATIOS)
    assert [render_of_call(128*c, 128, 147, 160) for c in range(4)] == [140, 139, 139, 140]
    assert [render_of_call(480*c, 480, 160, 147) for c in range(6)] == [441]*6
    assert [render_of_call(16*c, 16, 3, 2) for c in range(3)] == [11, 11, 10]
    assert [render_of_call(d, n, 3, 2) for d, n in ((0, 20), (20, 28), (48, 8))] == [14, 18, 6]
    r = np.zeros(38, np.float32); r[2] = 1
    outs = np.concatenate(stream_out_mirror(r, [20, 28, 8], 3, 2, rs.formula_taps(3, 2)))
    assert not rs.bits(outs[:48]).any() and rs._hex(outs[48:]) == ANSWER_3_2, rs._hex(outs[48:])
    r = np.zeros(due(37, 2, 3), np.float32); r[3] = 1
    outs = np.concatenate(stream_out_mirror(r, [10, 27], 2, 3, rs.formula_taps(2, 3)))
    assert not rs.bits(outs[:32]).any() and rs._hex(outs[32:37]) == ANSWER_2_3, rs._hex(outs[32:37])
    rng = np.random.default_rng(6)
    for up, down in rs.RATIOS:
        L, M, H, T = rs.shape_of(up, down)
        Dl = latency_of(up, down)
        table = rs.formula_taps(up, down)
        n = 3*max(T*L//M, Dl) + 2*Dl + 41
        E = due(n, L, M)
        r = rng.uniform(-1, 1, (2, E)).astype(np.float32)
        clip = rs.mirror(r, up, down, table)                                            # frame m of "Resample" applied to r
        assert clip.shape[1] >= n - Dl
        want = np.concatenate([np.zeros((2, Dl), np.float32), clip[:, :n - Dl]], axis=1)
        for cuts in (model_cuts(up, down, n), [n], [n//3, -1, n - n//3], [7]*(n//7) + [n % 7]):
            assert rendered_total(cuts, up, down) == E
            got = np.concatenate(stream_out_mirror(r, cuts, up, down, table), axis=1)
            assert got.shape == want.shape and rs.same_floats(got, want), (up, down, cuts[:4])
        assert not rs.bits(got[:, :Dl]).any()                                           # (+0.0, not -0.0)
    # the line: for every delivered count, the first live frame reaches at most T + ceil(M/L) below ceil(delivered*M/L), and 293 at most
    worst = 0
    for up, down in rs.TABLE_RATIOS:
        L, M, H, T = rs.shape_of(up, down)
        Dl = latency_of(up, down)
        d = np.arange(Dl, Dl + 4*L*M + 3000, dtype=np.int64)
        reach = (d*M + L - 1)//L - (((d - Dl)*M)//L - (H - 1))
        assert reach.max() <= line_bound(up, down) <= LINE, (up, down, int(reach.max()))
        assert Dl*M >= H*L                                                              # (Dl*M/L >= H: the right edge never enters)
        i_plus_h = ((d - Dl)*M)//L + H
        assert (i_plus_h <= ((d + 1)*M + L - 1)//L - 1).all(), (up, down)
        worst = max(worst, int(reach.max()))
    assert worst <= line_bound(2, 9) == 293 == max(line_bound(*q) for q in rs.TABLE_RATIOS) <= LINE, worst


# ---- the kernel hook against the mirror ------------------------------------------------------------------------------------------------

def run_hook(lib, images, cuts, ratios, delivered0=None, src_offset=1, out_offset=2):
    """images: per stream float32 [C, E total], the rendered frames; cuts: per stream the calls' delivered counts (padded with "no part" to
    the longest list); ratios: per stream -> (out as the hook left it, the expected image: the mirror's frames, in order, inside the sentinel)"""
    pkg = package()
    S, Cn = len(images), images[0].shape[0]
    calls = max(len(c) for c in cuts)
    counts = np.full((calls, S), -1, np.int32)
    for s, c in enumerate(cuts):
        counts[:len(c), s] = c
    in_cs = max(x.shape[1] for x in images) + 5                               # (odd against 4: a stream's rows lie at every offset)
    in_ss = Cn*in_cs + 1
    image = rs._float_buffer(S*in_ss + 8, src_offset)
    image[:] = np.float32(123.0)
    expect, rendered, totals = [], [], []
    for s in range(S):
        d0 = 0 if delivered0 is None else delivered0[s]
        for c in range(Cn):
            image[s*in_ss + c*in_cs:s*in_ss + c*in_cs + images[s].shape[1]] = images[s][c]
        totals.append(sum(max(n, 0) for n in cuts[s]))
        if rs.reduced(*ratios[s]) == (1, 1):
            expect.append(None)
            rendered.append(0)
            continue
        assert rendered_total(cuts[s], *ratios[s], delivered0=d0) == images[s].shape[1], (s, images[s].shape)
        expect.append(np.concatenate(stream_out_mirror(images[s], cuts[s], *ratios[s], rs.library_taps(lib, *ratios[s]), delivered0=d0), axis=1))
        rendered.append(images[s].shape[1])
    max_frames = max(totals) + 9
    out_cs = max_frames + 6
    out_ss = Cn*out_cs + 3
    out = rs._float_buffer(S*out_ss + 8, out_offset)
    out[:] = SENTINEL
    want = np.array(out, copy=True)
    for s in range(S):
        for c in range(Cn):
            if expect[s] is not None:
                want[s*out_ss + c*out_cs:s*out_ss + c*out_cs + totals[s]] = expect[s][c]
    launches = sum(1 for k in range(calls) if any(counts[k, s] > 0 and expect[s] is not None for s in range(S)))
    before = [pkg.launch_count(k, lib) for k in (COUNTER, COPY)]
    got = pkg.debug_pcm_stream_resample_out(counts, ratios, Cn, image, in_ss, in_cs, out, out_ss, out_cs, max_frames, delivered0=delivered0, lib=lib)
    assert [pkg.launch_count(k, lib) - n for k, n in zip((COUNTER, COPY), before)] == [launches, 0]
    assert got.tolist() == rendered, (got.tolist(), rendered)
    return out, want, expect


def _differs(got, want):
    return np.flatnonzero(~((rs.bits(got) == rs.bits(want)) | (np.isnan(got) & np.isnan(want))))[:8]


def check_hook(lib, up, down, channels):
    """one sequence of calls per ratio and channel count, six streams: noise cut as 0, no part, 1, a call wholly below Dl, one that straddles
    it, T + 1, rest; noise in calls that end on a tile edge and one past it (1024, 1025, then 1 and 2049); noise in a run of calls of 7
    frames, so that a window spans many calls; zeros; one NaN; +-inf.  The delivered frames are Dl zeros and then the whole-clip mirror's
    of the rendered frames, bit for bit, sentinels kept"""
    L, M, H, T = rs.shape_of(up, down)
    Dl = latency_of(up, down)
    rng = np.random.default_rng(3000*up + down + channels)
    special = Dl + 3*max(T*L//M, 8) + 37
    cuts = [[0, -1, 1, Dl - 4, 9, T + 1, 2*Dl + 50],                          # (1 + Dl - 4 < Dl: zeros only; the 9 straddle Dl)
            [TILE, TILE + 1, 1, 2*TILE + 1],
            [7]*((2*Dl + 40)//7),
            [special//3, 0, special - special//3],
            [Dl + 3, 7, special - Dl - 10],
            [special - 5, -1, 5]]
    images = [rng.uniform(-1, 1, (channels, rendered_total(c, up, down))).astype(np.float32) for c in cuts]
    images[3][:] = 0
    nan_at = images[4].shape[1]//2
    images[4][0, nan_at] = np.nan
    images[5][channels - 1, 5] = np.inf
    images[5][0, images[5].shape[1] - 9] = -np.inf
    ratios = [(up, down)]*len(cuts)
    for src_offset, out_offset in ((1, 0), (3, 2)) if channels == 2 else ((2, 1),):
        got, want, expect = run_hook(lib, images, cuts, ratios, src_offset=src_offset, out_offset=out_offset)
        assert rs.same_floats(got, want), (up, down, channels, _differs(got, want))
    table = rs.library_taps(lib, up, down)
    for s, r in enumerate(images):
        n = expect[s].shape[1]
        clip = rs.mirror(r, up, down, table)
        assert not rs.bits(expect[s][:, :min(Dl, n)]).any() and rs.same_floats(expect[s][:, Dl:], clip[:, :max(n - Dl, 0)]), (up, down, s)
    # exactly the delivered frames whose T taps reach the NaN are NaN
    n = expect[4].shape[1]
    i = ((np.arange(n, dtype=np.int64) - Dl)*M)//L
    reached = (np.arange(n) >= Dl) & (i - (H - 1) <= nan_at) & (nan_at <= i + H)
    assert np.array_equal(np.isnan(expect[4][0]), reached) and reached.any() and not reached.all() and not np.isnan(expect[4][1:]).any(), (up, down)


def check_known_answers(lib):
    """the two impulse known answers of include/smst.h through the hook, as literal bit patterns"""
    r = np.zeros((1, 38), np.float32); r[0, 2] = 1
    got, want, expect = run_hook(lib, [r], [[20, 28, 8]], [(3, 2)])
    assert rs.same_floats(got, want) and not rs.bits(expect[0][0, :48]).any() and rs._hex(expect[0][0, 48:]) == ANSWER_3_2
    assert rs._hex(got[np.flatnonzero(rs.bits(got) != rs.bits(SENTINEL))][48:56]) == ANSWER_3_2
    r = np.zeros((1, due(37, 2, 3)), np.float32); r[0, 3] = 1
    got, want, expect = run_hook(lib, [r], [[10, 27]], [(2, 3)])
    assert rs.same_floats(got, want) and rs._hex(got[np.flatnonzero(rs.bits(got) != rs.bits(SENTINEL))][32:37]) == ANSWER_2_3


FAR = ((160, 147, (1 << 33) + 5), (147, 640, (1 << 33) + 5), (160, 147, (1 << 40) + 123457), (147, 640, (1 << 40) + 123457))


def check_far_positions(lib, channels=2):
    """lines that start as zeros at 2^33 + 5 and 2^40 + 123457 delivered frames (beyond 2^32 and beyond 2^32*L): the frames are the
    mirror's at those absolute n.  i, p and m*M have to be 64-bit: a 32-bit one gives another phase and another span"""
    rng = np.random.default_rng(34)
    ratios = [(up, down) for up, down, _ in FAR]
    d0 = [f for _, _, f in FAR]
    cuts = [[70, 300, 1, 0, 330] for _ in FAR]
    images = [rng.uniform(-1, 1, (channels, rendered_total(c, *q, delivered0=f))).astype(np.float32) for c, q, f in zip(cuts, ratios, d0)]
    got, want, expect = run_hook(lib, images, cuts, ratios, delivered0=d0)
    assert rs.same_floats(got, want), _differs(got, want)
    for (up, down, f), y in zip(FAR, expect):
        L, M, H, T = rs.shape_of(up, down)
        assert f > (1 << 32) and ((f - latency_of(up, down))*M)//L > (1 << 32) and y[:, 400:].any()
    assert FAR[2][2] > (1 << 32)*160 and FAR[3][2] > (1 << 32)*147


def check_mixed(lib, channels=2):
    """eight ratios and two plain streams in one sequence of calls: the plain streams' rows of the output stay as they were"""
    rng = np.random.default_rng(79)
    ratios = list(rs.RATIOS[:3]) + [(1, 1)] + list(rs.RATIOS[3:6]) + [(5, 5)] + list(rs.RATIOS[6:])
    totals = [700, 1500, 900, 400, 1200, 1100, 1300, 640, 600, 2100]
    cuts = []
    for s, n in enumerate(totals):
        first = (n*(s + 1))//13
        cuts.append([first, -1 if s % 3 == 0 else 0, 17, n - first - 17 - 100, 100])
    images = [rng.uniform(-1, 1, (channels, max(rendered_total(c, *q), 1))).astype(np.float32) for c, q in zip(cuts, ratios)]
    for s in (3, 7):
        images[s] = images[s][:, :1]
    got, want, expect = run_hook(lib, images, cuts, ratios)
    assert rs.same_floats(got, want), _differs(got, want)
    assert len(set(rs.reduced(*r) for r in ratios) - {(1, 1)}) == 8 and expect[3] is None and expect[7] is None


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

SESSION_RATIOS = ((147, 160), (1, 1), (160, 147), (2, 3))                      # stream 1 is a plain one
SESSION_OUT = ([20, 300, 12, 20], [300, 256, 1, 400], [400, 350, 128, 500], [0, 200, 333, 77], [512, 512, 512, 600], [128, 128, 128, 128])   # frames delivered per call
SESSION_IN = ([300, 300, 300, 300], [300, 256, 64, 400], [400, 350, 128, 500], [100, 200, 333, 77], [512, 512, 512, 600], [128, 128, 128, 128])
SESSION_TAIL = [200, 200, 150, -1]                                             # the flush: these and Dl frames more; stream 3 is left out
SESSION_SEED = 72
SEEK_IN = [700, 640, 800, 1200]
SEEK_RATES = [1.0, 0.8, 1.25, 1.0]
PLAIN = 1
METER_FS = 2570.0                                                              # what the meter is told: h = 257, so that the short session has blocks
IN_RATIO = (160, 147)                                                          # stream 0 of the variant that resamples the input too: 44.1 kHz in, 44.1 kHz out
_inputs = {}


def session_inputs(fmt, Cn=2):
    """-> (frames of the format [S, n, C], the planar float32 [S, C, n] they decode to) for the seek and the calls; computed once per format"""
    if fmt not in _inputs:
        S = len(SESSION_RATIOS)
        n = max(SEEK_IN) + sum(max(c) for c in SESSION_IN)
        x = np.stack([0.45*synth_input(s, Cn, n, 44100) + 0.2*synth_input(s + 5, Cn, n, 44100) for s in range(S)]).astype(np.float32)
        frames = fc.encode_frames(pc.frames_of(x), fmt)
        _inputs[fmt] = (frames, np.ascontiguousarray(np.transpose(fc.decode_frames(frames, fmt), (0, 2, 1))).astype(np.float32))
    return _inputs[fmt]


def set_session(batch):
    for s, (up, down) in enumerate(SESSION_RATIOS):
        batch.set_pcm_stream_out_resample(up, down, stream=s)


def check_session(lib, fmt, dithered, limiter=False, meter=False, resample_in=False, seek=False, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """processFrames and flushFrames of a batch with the setting against a twin without it that gets the same input and is asked, per call,
    for the E frames that smst_batch_pcm_stream_out_resample_render reports, in float32: six calls of uneven sizes -- calls wholly below
    Dl, one with E = 0, a stream with no frame -- and a flush of tail + Dl frames that leaves a stream out.  The model resamples the twin's
    output; the delivered bytes are the model's frames put through the format's output rule, dithered at the delivered frame's index where
    the format can be; overs and peaks agree.  limiter: the stream limiter on, F32 -- the bytes are the limiter's mirror on the delivered
    frames, Dl and 2H late, and its meters agree.  meter: the stream meter on at the delivery rate -- its take is the clip meters' of the
    delivered frames, the Dl zeros included.  resample_in: stream 0 carries the input setting as well, in both batches.  seek: a call,
    reset(), the same call again (the reset clears the line), then seekFrames (which does not) and the session"""
    pkg = package()
    S, Cn = len(SESSION_RATIOS), 2
    frames, planar = session_inputs(fmt)
    tables = [None if rs.reduced(*q) == (1, 1) else rs.library_taps(lib, *q) for q in SESSION_RATIOS]
    latency = [0 if tb is None else latency_of(*q) for tb, q in zip(tables, SESSION_RATIOS)]
    r, t = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(2))
    set_session(r)
    assert [r.pcm_stream_out_resample(s) for s in range(S)] == [rs.reduced(*q) for q in SESSION_RATIOS]
    assert [r.stream_out_resample_latency(s) for s in range(S)] == latency
    assert [t.pcm_stream_out_resample(s) for s in range(S)] == [(1, 1)]*S and [t.stream_out_resample_latency(s) for s in range(S)] == [0]*S
    gain, ceil, H = (6.0, 0.5, lm.DEFAULT_H) if limiter else (1.0, 1.0, 0)
    r.set_pcm_level(lc.FIXED, gain, 1.0)                                        # (a levelled batch meters peaks)
    if limiter:
        assert fmt == fc.F32
        r.set_pcm_stream_limiter(True, ceil)
        win = lm.library_window(lib, H)
        assert r.pcm_stream_limiter_latency() == 2*H
    if meter:
        r.set_pcm_stream_meter(True, METER_FS, 64)
    if resample_in:
        for b in (r, t):
            b.set_pcm_stream_resample(*IN_RATIO, stream=0)
    modes = [dc.MODES[s % 2] if dithered else dc.NONE for s in range(S)]
    if dithered:
        for s in range(S):
            r.setPcmDither(modes[s], SESSION_SEED + s, stream=s)
    model = dict(rendered=[planar[s, :, :0] for s in range(S)], delivered=[planar[s, :, :0] for s in range(S)], first=[0]*S, zero_e=False, below=False)

    def clear():
        model.update(rendered=[planar[s, :, :0] for s in range(S)], delivered=[planar[s, :, :0] for s in range(S)])

    def deliver(s, fresh, nd):
        """the model on everything rendered since the clear, cut at the call: its last call's frames are this call's"""
        if tables[s] is None:
            y = fresh[:, :nd]
        else:
            done = model["delivered"][s].shape[1]
            history = np.concatenate([model["rendered"][s], fresh], axis=1)
            y = stream_out_mirror(history, [done, nd], *SESSION_RATIOS[s], tables[s])[1]
            model["rendered"][s] = history
            model["zero_e"] = model["zero_e"] or (nd > 0 and fresh.shape[1] == 0)
            model["below"] = model["below"] or (nd > 0 and done + nd <= latency[s])
        model["delivered"][s] = np.concatenate([model["delivered"][s], y], axis=1)
        return y

    def written(s, nd):
        """what the conversion is handed for the call's nd frames of stream s (after the gain; the limiter's u where it is on), and the peak before the gain"""
        v = model["delivered"][s]
        total = v.shape[1]
        if limiter:
            _, u = sl.mirror(v, gain, ceil, H, win)
            seen = np.concatenate([np.zeros((Cn, 2*H), np.float32), v], axis=1)[:, total - nd:total]
            return u[:, total - nd:], seen
        return lc.levelled(v[:, total - nd:], gain), v[:, total - nd:]

    def check_call(got, nd, ys, tag):
        peaks, gains = r.take_pcm_peaks()
        overs, nans = r.takePcmOvers()
        for s in range(S):
            if nd[s] < 0:
                continue
            u, seen = written(s, nd[s])
            assert sl.same_bits(peaks[s], lc.peak_of(seen) if nd[s] else np.float32(0)), (fmt, tag, s, float(peaks[s]))
            codes, cm, nm = dc.mirror(u, fmt, modes[s], SESSION_SEED + s, model["first"][s])
            want = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
            assert (int(overs[s]), int(nans[s])) == (int(cm.sum()), int(nm.sum())), (fmt, tag, s)
            assert lc.same_bytes(np.ascontiguousarray(got[s, :nd[s]]).reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8), fmt), (fmt, dithered, tag, s)
            model["first"][s] += nd[s]

    def process_call(pos, nin, nd, tag):
        E = [r.stream_out_resample_render(s, nd[s]) for s in range(S)]
        for s in range(S):
            done = model["delivered"][s].shape[1]
            assert E[s] == (nd[s] if tables[s] is None else render_of_call(done, nd[s], *SESSION_RATIOS[s])), (tag, s, E[s])
            assert t.stream_out_resample_render(s, nd[s]) == nd[s]
        x = np.ascontiguousarray(frames[:, pos:pos + max(nin)])
        twin_in = np.ascontiguousarray(np.transpose(planar[:, :, pos:pos + max(nin)], (0, 2, 1)))
        fill = lambda like, n: np.full(like.shape[:1] + (max(max(n), 1),) + like.shape[2:], 0x5A if like.dtype != np.float32 else 0, like.dtype)
        rendered = to_host(t.processFrames(to_memory(twin_in), E, in_samples=nin, out=to_memory(fill(twin_in, E))))
        before = [pkg.launch_count(k, lib) for k in (COUNTER, COPY)]
        got = to_host(r.processFrames(to_memory(x), nd, in_samples=nin, out=to_memory(fill(x, nd))))
        ran = int(any(tables[s] is not None and nd[s] > 0 for s in range(S)))
        assert [pkg.launch_count(k, lib) - n for k, n in zip((COUNTER, COPY), before)] == [ran, ran], tag
        ys = [deliver(s, np.ascontiguousarray(rendered[s, :E[s]].T), nd[s]) for s in range(S)]
        check_call(got, nd, ys, tag)
        return got

    pos = 0
    if seek:
        junk_in, junk_out = [300]*S, [200, 200, 200, 200]
        process_call(0, junk_in, junk_out, "before the reset")
        for b in (r, t):
            b.reset()
        clear()
        assert [r.stream_out_resample_render(s, 100) for s in range(S)] == [r.stream_out_resample_render(s, 100, fresh=True) for s in range(S)]
        process_call(0, junk_in, junk_out, "behind the reset")                 # (the same frames again: a line that was kept would show)
        x = to_memory(np.ascontiguousarray(frames[:, :max(SEEK_IN)]))
        twin_in = to_memory(np.ascontiguousarray(np.transpose(planar[:, :, :max(SEEK_IN)], (0, 2, 1))))
        r.seekFrames(x, SEEK_RATES, in_samples=SEEK_IN)                         # (emits nothing: the line and the count go on)
        t.seekFrames(twin_in, SEEK_RATES, in_samples=SEEK_IN)
        assert [r.stream_out_resample_render(s, 100) for s in range(S)] == [100 if tables[s] is None else render_of_call(200, 100, *SESSION_RATIOS[s]) for s in range(S)]
        pos = max(SEEK_IN)
    heard = False
    for call, (nin, nd) in enumerate(zip(SESSION_IN, SESSION_OUT)):
        got = process_call(pos, list(nin), list(nd), "call %d" % call)
        heard = heard or bool(got.view(np.uint8).any())
        pos += max(nin)
    assert heard and (seek or (model["zero_e"] and model["below"]))            # (a call with E = 0 and one wholly below Dl were among them)
    # the flush: tail + Dl frames, stream 3 left out
    nd = [n if n < 0 else n + latency[s] + 2*H for s, n in enumerate(SESSION_TAIL)]
    E = [n if n < 0 else r.stream_out_resample_render(s, n) for s, n in enumerate(nd)]
    like = to_memory(np.zeros((1,), np.float32))
    rendered = to_host(t.flushFrames(E, like=like, dtype=np.float32))
    got = to_host(r.flushFrames(nd, like=like, dtype="s24" if fmt == fc.S24 else fc.frame_dtype(fmt)))
    ys = [None if nd[s] < 0 else deliver(s, np.ascontiguousarray(rendered[s, :E[s]].T), nd[s]) for s in range(S)]
    check_call(got, nd, ys, "flush")
    # ending a stream: behind the flush the delivered frames are Dl zeros and then the clip form's of everything rendered
    for s in range(S):
        if tables[s] is not None and nd[s] >= 0:
            v, clip = model["delivered"][s], rs.mirror(model["rendered"][s], *SESSION_RATIOS[s], tables[s])
            assert rs.same_floats(v[:, latency[s]:], clip[:, :v.shape[1] - latency[s]]) and v.shape[1] - latency[s] <= clip.shape[1], s
    if limiter:
        low, count = r.take_pcm_stream_limiter()
        for s in range(S):
            ml, mc = sl.meters_of(sl.mirror(model["delivered"][s], gain, ceil, H, win)[0])
            assert sl.same_bits(low[s], ml) and int(count[s]) == mc and mc > 0, (s, float(low[s]), float(ml), int(count[s]), mc)
    if meter:
        totals = [v.shape[1] for v in model["delivered"]]
        image = np.zeros((S, Cn, max(totals)), np.float32)
        for s, v in enumerate(model["delivered"]):
            image[s, :, :v.shape[1]] = v
        ref = sm.clip_reference(lib, image, totals, METER_FS, max_blocks=64)
        assert [r.pcm_stream_meter_frames(s) for s in range(S)] == [(n, n) for n in totals]
        sm.assert_take(r.take_pcm_stream_meter(), ref, dict(stream_out_resample=fmt))
        assert (ref["blocks"] > 0).all()
    for b in (r, t):
        b.close()


# ---- opt-in, steady state, reproducible ----------------------------------------------------------------------------------------------

def _counts(lib):
    pkg = package()
    return [pkg.launch_count(k, lib) for k in COUNTERS]


def check_opt_in(lib, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """a batch that never set the ratio and one that set it and went back to 1/1: the same bytes, the same launches, none of the new
    kernels; in a mixed call the plain stream's bytes are those of a batch with no setting"""
    pkg = package()
    assert all(pkg.launch_count(k, lib) >= 0 for k in (COUNTER, COPY)), "the library has no %s counter" % COUNTER
    S, Cn = len(SESSION_RATIOS), 2
    frames, _ = session_inputs(fc.S16)
    a, b, m = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(3))
    b.set_pcm_stream_out_resample(147, 160)                                       # (the twin had a ratio once: 1/1 turns the stage off again)
    b.set_pcm_stream_out_resample(1, 1)
    x = [np.ascontiguousarray(frames[:, :700]), np.ascontiguousarray(frames[:, 700:1300])]
    like = to_memory(np.zeros((1,), np.float32))
    outs, deltas = [], []
    for batch in (a, b):
        before = _counts(lib)
        out = [to_host(batch.processFrames(to_memory(x[0]), [700]*S)), to_host(batch.processFrames(to_memory(x[1]), [500, 600, 700, 600])), to_host(batch.flushFrames([100, 200, -1, 50], like=like))]
        batch.synchronize()
        outs.append(out)
        deltas.append([y - w for w, y in zip(before, _counts(lib))])
    assert all(np.array_equal(u, v) for u, v in zip(*outs)) and deltas[0] == deltas[1], (deltas[0], deltas[1])
    delta = dict(zip(COUNTERS, deltas[0]))
    assert delta[COUNTER] == delta[COPY] == 0 and delta["pcm_in"] == 2 and delta["pcm_out"] == 3, delta
    set_session(m)
    before = _counts(lib)
    mixed = [to_host(m.processFrames(to_memory(x[0]), [700]*S)), to_host(m.processFrames(to_memory(x[1]), [500, 600, 700, 600])), to_host(m.flushFrames([100, 200, -1, 50], like=like))]
    m.synchronize()
    got = dict(zip(COUNTERS, [y - w for w, y in zip(before, _counts(lib))]))
    assert got[COUNTER] == got[COPY] == 3 and got["pcm_in"] == 2 and got["pcm_out"] == 3, got
    for k, n in enumerate((700, 600, 200)):
        assert np.array_equal(mixed[k][PLAIN, :n], outs[0][k][PLAIN, :n]) and mixed[k][PLAIN, :n].any(), k
    assert not np.array_equal(mixed[1][0, :500], outs[0][1][0, :500])
    for batch in (a, b, m):
        batch.close()


def check_steady_state(lib, to_memory=lambda a: a):
    """the setter allocates the lines and the call tables, outside any call; after one warm-up call the allocation events and the workspace
    bytes stand still over three more calls and a flush; setting a ratio that already has a table allocates nothing"""
    pkg = package()
    S, Cn = len(SESSION_RATIOS), 2
    frames = to_memory(np.ascontiguousarray(session_inputs(fc.S16)[0][:, :600]))
    like = to_memory(np.zeros((1,), np.float32))
    b = pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY)
    plain = b.workspaceBytes()
    set_session(b)
    assert b.workspaceBytes() >= plain + 2*S*Cn*LINE*4                              # (the lines are in device memory from the setter on)
    b.processFrames(frames, [600, 500, 450, 300], in_samples=[600, 500, 512, 480])
    b.flushFrames([100, 100, 100, 100], like=like)
    b.synchronize()
    events, grown = b.allocation_events(), b.workspaceBytes()
    for _ in range(3):
        b.processFrames(frames, [600, 500, 450, 300], in_samples=[600, 500, 512, 480])
    b.flushFrames([100, 100, 100, 100], like=like)
    b.synchronize()
    assert (b.allocation_events(), b.workspaceBytes()) == (events, grown)
    b.set_pcm_stream_out_resample(294, 320, stream=PLAIN)                          # (147/160, which stream 0 has)
    assert (b.allocation_events(), b.workspaceBytes()) == (events, grown) and b.pcm_stream_out_resample(PLAIN) == (147, 160)
    b.close()


def run_session(lib, fmt=fc.S24):
    """-> (the calls' frames, the E the calls rendered according to stream_out_resample_render)"""
    pkg = package()
    S = len(SESSION_RATIOS)
    frames, _ = session_inputs(fmt)
    b = pkg.StretchBatch(S, 2, lib=lib, seed=3, **pc.GEOMETRY)
    set_session(b)
    outs, Es, pos = [], [], 0
    for nin, nd in zip(SESSION_IN, SESSION_OUT):
        Es.append([b.stream_out_resample_render(s, nd[s]) for s in range(S)])
        outs.append(np.array(b.processFrames(np.ascontiguousarray(frames[:, pos:pos + max(nin)]), list(nd), in_samples=list(nin)), copy=True))
        pos += max(nin)
    b.close()
    return outs, Es


def check_reproducible(lib):
    """two runs of the same session are bit-identical, and so are two batches; _render and _latency agree with the definition, `fresh`
    included"""
    pkg = package()
    (a, ea), (b, eb) = run_session(lib), run_session(lib)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and ea == eb and any(u.any() for u in a)
    done = [0]*len(SESSION_RATIOS)
    for nd, E in zip(SESSION_OUT, ea):
        for s, q in enumerate(SESSION_RATIOS):
            assert E[s] == (nd[s] if rs.reduced(*q) == (1, 1) else render_of_call(done[s], nd[s], *q)), (s, nd, E)
            done[s] += nd[s]
    bt = pkg.StretchBatch(2, 1, lib=lib, **pc.GEOMETRY)
    x = np.zeros((2, 64, 1), np.float32)
    for up, down in rs.RATIOS:
        bt.set_pcm_stream_out_resample(up, down, stream=0)
        assert bt.stream_out_resample_latency(0) == LATENCIES[(up, down)]
        for n in (0, 1, 16, 128, 441, 480, 48000):
            assert bt.stream_out_resample_render(0, n) == render_of_call(0, n, up, down)
        bt.processFrames(x, [13, 13], in_samples=[64, 64])                         # 13 frames delivered: the next call's E moves, a fresh one's does not
        for n in (0, 1, 16, 128):
            assert bt.stream_out_resample_render(0, n) == render_of_call(13, n, up, down)
            assert bt.stream_out_resample_render(0, n, fresh=True) == render_of_call(0, n, up, down)
        assert bt.stream_out_resample_render(1, 77) == 77 and bt.stream_out_resample_latency(1) == 0
    bt.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def _refused(lib, rc, *words):
    msg = lib.smst_last_error() or b""
    assert rc == ERR_INVALID and all(w in msg for w in words), (rc, msg)


def check_refusals(lib, to_memory=lambda a: a):
    pkg = package()
    S, Cn = 10, 2
    b = pkg.StretchBatch(S, Cn, lib=lib, **pc.GEOMETRY)
    for up, down, word in ((0, 1, b"640"), (1, 0, b"640"), (-3, 2, b"640"), (641, 640, b"640"), (640, 641, b"640"), (1283, 1281, b"640"), (2, 10, b"4.5"), (1, 5, b"4.5"), (6, 1, b"4.5")):
        _refused(lib, lib.smst_batch_set_pcm_stream_out_resample(b.h, 0, up, down), word)
    for stream in (-2, S):
        _refused(lib, lib.smst_batch_set_pcm_stream_out_resample(b.h, stream, 2, 1), b"stream")
    for stream in (-1, S):
        _refused(lib, lib.smst_batch_pcm_stream_out_resample(b.h, stream, None, None), b"stream")
        _refused(lib, lib.smst_batch_pcm_stream_out_resample_latency(b.h, stream, None), b"stream")
        _refused(lib, lib.smst_batch_pcm_stream_out_resample_render(b.h, stream, 100, 0), b"stream")
    _refused(lib, lib.smst_batch_set_pcm_stream_out_resample(None, 0, 2, 1), b"null")
    _refused(lib, lib.smst_batch_pcm_stream_out_resample(None, 0, None, None), b"null")
    _refused(lib, lib.smst_batch_pcm_stream_out_resample_latency(None, 0, None), b"null")
    _refused(lib, lib.smst_batch_pcm_stream_out_resample_render(None, 0, 100, 0), b"null")
    assert [b.pcm_stream_out_resample(s) for s in range(S)] == [(1, 1)]*S           # (a refused call changes nothing)
    assert lib.smst_batch_set_pcm_stream_out_resample(b.h, 0, 1280, 1176) == 0 and b.pcm_stream_out_resample(0) == (160, 147)   # (reduced first, then checked)
    assert b.pcm_resample(0) == b.pcm_stream_resample(0) == b.pcm_out_resample(0) == (1, 1)   # (the three other settings are other ones)
    b.set_pcm_stream_out_resample(1, 1)
    # the shared slots: a ninth ratio across all four settings is refused, and a slot is free once all its users have gone
    setters = (b.set_pcm_stream_out_resample, b.set_pcm_resample, b.set_pcm_stream_resample, b.set_pcm_out_resample)
    for s, (up, down) in enumerate(rs.RATIOS):
        setters[s % 4](up, down, stream=s)
    _refused(lib, lib.smst_batch_set_pcm_stream_out_resample(b.h, 8, 4, 3), b"8")
    _refused(lib, lib.smst_batch_set_pcm_out_resample(b.h, 9, 5, 4), b"8")
    assert b.pcm_stream_out_resample(8) == b.pcm_out_resample(9) == (1, 1)
    b.set_pcm_stream_out_resample(1, 2, stream=8)                                   # (a ratio that is live through another setting: no new slot)
    b.set_pcm_resample(1, 1, stream=1)                                              # 1/2 has lost one of its two users ...
    _refused(lib, lib.smst_batch_set_pcm_stream_out_resample(b.h, 9, 4, 3), b"8")
    b.set_pcm_stream_out_resample(1, 1, stream=8)                                   # ... and now both: its slot is free
    b.set_pcm_stream_out_resample(4, 3, stream=9)
    assert b.pcm_stream_out_resample(9) == (4, 3)
    _refused(lib, lib.smst_batch_set_pcm_resample(b.h, 1, 1, 2), b"8")
    for setter in setters:
        setter(1, 1)
    # an E that does not fit an int
    b.set_pcm_stream_out_resample(2, 9, stream=0)
    assert b.stream_out_resample_render(0, 477218588) == 2147483646
    _refused(lib, lib.smst_batch_pcm_stream_out_resample_render(b.h, 0, 477218589, 0), b"2147483647")
    _refused(lib, lib.smst_batch_pcm_stream_out_resample_render(b.h, 0, 1 << 62, 1), b"2147483647")
    _refused(lib, lib.smst_batch_pcm_stream_out_resample_render(b.h, 0, -1, 0), b"negative")
    counts = (pkg.C.c_int*S)(*([477218589] + [0]*(S - 1)))
    rates = (pkg.C.c_float*S)(*([0.0]*S))
    tiny = to_memory(np.zeros((S, 4, Cn), np.float32))
    ptr = pkg.C.c_void_p(tiny.ctypes.data if isinstance(tiny, np.ndarray) else tiny.data_ptr())
    memory = pkg.MEM_HOST if isinstance(tiny, np.ndarray) else pkg.MEM_DEVICE
    _refused(lib, lib.smst_batch_flush_pcm(b.h, ptr, 4*Cn, Cn, counts, rates, pkg.PCM_F32, memory), b"2147483647")   # (refused before anything runs)
    assert b.stream_out_resample_render(0, 9) == 41                                 # (... and before the count moves)
    b.close()
    # the call that does not serve the setting, and the whole-clip output ratio in the streaming calls
    b = pkg.StretchBatch(3, Cn, lib=lib, **pc.GEOMETRY)
    b.set_pcm_stream_out_resample(3, 2, stream=1)
    frames = to_memory(np.zeros((3, 2000, Cn), np.int16))
    like = to_memory(np.zeros((1,), np.float32))
    with dc.pytest_raises(pkg.StretchError) as e:
        b.exactFrames(frames, [2400, 2400, 2400])
    assert "smst_batch_set_pcm_stream_out_resample" in str(e.value) and "smst_batch_set_pcm_out_resample" in str(e.value) and "error -1" in str(e.value), str(e.value)
    b.exactFrames(frames, [2400, -1, 2400])                                         # (stream 1 takes no part: not refused)
    b.processFrames(frames, [600, 600, 600])
    b.seekFrames(frames, [1.0, 1.0, 1.0])                                           # (no output: unaffected)
    b.outputSeekFrames(frames)
    b.flushFrames([100, 50, 100], like=like)
    b.set_pcm_out_resample(3, 2, stream=1)                                          # (both output settings on one stream: each call family reads its own)
    for call in (lambda: b.processFrames(frames, [600, 600, 600]), lambda: b.flushFrames([100, 50, 100], like=like)):
        with dc.pytest_raises(pkg.StretchError) as e:
            call()
        assert "smst_batch_set_pcm_out_resample" in str(e.value) and "smst_batch_exact_pcm only" in str(e.value), str(e.value)
    b.flushFrames([100, -1, 100], like=like)                                        # (stream 1 takes no part)
    b.close()
    _refused(lib, lib.smst_debug_pcm_stream_resample_out(0, 1, 1, 0, None, None, None, None, 0, 0, None, 0, 0, 0, None), b"bad arguments")
