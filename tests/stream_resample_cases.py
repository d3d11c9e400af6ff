"""Shared cases of the sample-rate converter's streaming form in front of smst_batch_process_pcm / _seek_pcm (include/smst.h, "Stream
resample"): test_stream_resample_emu.py runs them on the CPU stand-in, test_stream_resample_gpu.py on the device.

The mirror is resample_cases.mirror -- the clip converter's restatement -- plus stream_mirror, a streaming model that reads only "the line
of T - 1 frames + the call's frames" and keeps fed and made as Python integers (positions as int64 arrays).  Everything is compared bit for
bit: a product of two float32 values is exact in float64 and both sides add in the order j = 0 ... T - 1.  The signal checks read the
library's own table through smst_debug_resample_taps, as resample_cases does."""
import numpy as np

import dither_cases as dc
import level_cases as lc
import pcm_cases as pc
import pcm_format_cases as fc
import resample_cases as rs
from conftest import package, synth_input

COUNTER = "pcm_stream_resample"
COUNTERS = rs.COUNTERS + ("pcm_limit_feed", "pcm_limit_gain", "pcm_out_limited", COUNTER)
MODEL_RATIOS = ((160, 147), (147, 160), (3, 2), (2, 9), (147, 640), (640, 147))
TILE = rs.TILE
LINE = 288                                                                   # floats of a channel's carried line (kStreamResampleLine)
SENTINEL = rs.SENTINEL
ERR_INVALID = -1


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def due(q, L, M):
    """R(q) = ceil(max(q, 0)*L/M)"""
    return 0 if q <= 0 else (q*L + M - 1)//M


def frames_of_call(fed, n, up, down):
    """k of a call that hands n frames behind fed"""
    L, M, H, T = rs.shape_of(up, down)
    return due(fed + n - H, L, M) - due(fed - H, L, M)


def need_of(fed, made, frames, up, down):
    L, M, H, T = rs.shape_of(up, down)
    return max(0, ((made + frames - 1)*M)//L + H + 1 - fed)


def stream_mirror(x, cuts, up, down, table, fed0=0):
    """x float32 [..., N]: the frames handed, in order; cuts: the calls' counts (negative: no part); fed0: the line starts as zeros at that
    position -> the frames of each call, float32 [..., k].  A call reads the line and its own frames, nothing else"""
    L, M, H, T = rs.shape_of(up, down)
    assert table.shape == (L, T) and table.dtype == np.float32
    x = np.asarray(x, np.float32)
    c = table.astype(np.float64)
    line = np.zeros(x.shape[:-1] + (T - 1,), np.float32)
    fed, made, pos, outs = int(fed0), due(int(fed0) - H, L, M), 0, []
    for n in cuts:
        n = max(int(n), 0)
        k = due(fed + n - H, L, M) - made
        window = np.concatenate([line, x[..., pos:pos + n]], axis=-1)                  # the positions fed - (T - 1) ... fed + n - 1
        at = made + np.arange(k, dtype=np.int64)
        i, p = (at*M)//L, (at*M) % L
        base = i - (H - 1) - (fed - (T - 1))
        assert k == 0 or (base.min() >= 0 and base.max() + T - 1 < window.shape[-1]), (fed, n, k)   # (never below the line, never past the call)
        w = window.astype(np.float64)
        y = np.zeros(x.shape[:-1] + (k,), np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(T):
                y = y + c[p, j]*w[..., base + j]
            outs.append(y.astype(np.float32))
        if n > 0:
            line = np.ascontiguousarray(window[..., window.shape[-1] - (T - 1):])
        fed, made, pos = fed + n, made + k, pos + n
    return outs


def model_cuts(up, down, n):
    L, M, H, T = rs.shape_of(up, down)
    head = [1, 0, 5, H - 1, H, T + 1, 3]
    assert n > sum(head)
    return head + [n - sum(head)]


def check_mirror():
    """the known answers of include/smst.h, and the model against the clip mirror for six ratios: with H trailing zeros the calls' frames
    are the clip form's Nr frames"""
    assert [frames_of_call(441*c, 441, 160, 147) for c in range(4)] == [446, 480, 480, 480]
    assert rs.shape_of(147, 160)[2] == 35 and [frames_of_call(128*c, 128, 147, 160) for c in range(4)] == [86, 118, 117, 118]
    x = np.zeros(37, np.float32); x[2] = 1
    outs = stream_mirror(x, [3, 2, 32], 3, 2, rs.formula_taps(3, 2))
    assert [o.shape[-1] for o in outs] == [0, 0, 8]
    assert rs._hex(outs[2]) == "bca067e3 be4717b5 3ed8327b 3f7ae0ea 3ed8327b be4717b5 bca067e3 3dddb185", rs._hex(outs[2])
    rng = np.random.default_rng(5)
    for up, down in MODEL_RATIOS:
        L, M, H, T = rs.shape_of(up, down)
        table = rs.formula_taps(up, down)
        n = 3*T + 2*H + 41
        x = rng.uniform(-1, 1, (2, n)).astype(np.float32)
        fed = np.concatenate([x, np.zeros((2, H), np.float32)], axis=1)
        got = np.concatenate(stream_mirror(fed, model_cuts(up, down, n) + [H], up, down, table), axis=1)
        want = rs.mirror(x, up, down, table)
        assert got.shape == want.shape and rs.same_floats(got, want), (up, down, got.shape, want.shape)
        # ... and the model does not depend on the cuts
        again = np.concatenate(stream_mirror(fed, [n + H], up, down, table), axis=1)
        assert rs.same_floats(got, again), (up, down)
        assert need_of(0, 0, 1, up, down) == H + 1 and frames_of_call(0, H, up, down) == 0 and frames_of_call(0, H + 1, up, down) >= 1


# ---- the kernel hook against the mirror ------------------------------------------------------------------------------------------------

def run_hook(lib, clips, cuts, ratios, fed0=None, src_offset=1, out_offset=2):
    """clips: per stream float32 [C, N]; cuts: per stream the calls' counts (padded with "no part" to the longest list); ratios: per stream
    -> (out as the hook left it, the expected image: the mirror's frames, in order, inside the sentinel; made)"""
    pkg = package()
    S, Cn = len(clips), clips[0].shape[0]
    calls = max(len(c) for c in cuts)
    counts = np.full((calls, S), -1, np.int32)
    for s, c in enumerate(cuts):
        counts[:len(c), s] = c
        assert sum(max(n, 0) for n in c) == clips[s].shape[1], (s, c, clips[s].shape)
    in_cs = max(c.shape[1] for c in clips) + 5                                # (odd against 4: a stream's rows lie at every offset)
    in_ss = Cn*in_cs + 1
    image = rs._float_buffer(S*in_ss + 8, src_offset)
    image[:] = np.float32(123.0)
    expect, made = [], []
    for s in range(S):
        for c in range(Cn):
            image[s*in_ss + c*in_cs:s*in_ss + c*in_cs + clips[s].shape[1]] = clips[s][c]
        if rs.reduced(*ratios[s]) == (1, 1):
            expect.append(None)
            made.append(0)
            continue
        y = np.concatenate(stream_mirror(clips[s], cuts[s], *ratios[s], rs.library_taps(lib, *ratios[s]), fed0=0 if fed0 is None else fed0[s]), axis=1)
        expect.append(y)
        made.append(y.shape[1])
    max_frames = max(made) + 9
    out_cs = max_frames + 6
    out_ss = Cn*out_cs + 3
    out = rs._float_buffer(S*out_ss + 8, out_offset)
    out[:] = SENTINEL
    want = np.array(out, copy=True)
    for s in range(S):
        for c in range(Cn):
            if expect[s] is not None:
                want[s*out_ss + c*out_cs:s*out_ss + c*out_cs + made[s]] = expect[s][c]
    launches = sum(1 for k in range(calls) if any(counts[k, s] > 0 and expect[s] is not None for s in range(S)))
    before = pkg.launch_count(COUNTER, lib)
    got_made = pkg.debug_pcm_stream_resample(counts, ratios, Cn, image, in_ss, in_cs, out, out_ss, out_cs, max_frames, fed0=fed0, lib=lib)
    assert pkg.launch_count(COUNTER, lib) == before + launches
    assert got_made.tolist() == made, (got_made.tolist(), made)
    return out, want, made


def _differs(got, want):
    return np.flatnonzero(~((rs.bits(got) == rs.bits(want)) | (np.isnan(got) & np.isnan(want))))[:8]


def tile_cuts(up, down):
    """calls whose k lies on and beside tile edges: per target the smallest n whose k reaches it"""
    L, M, H, T = rs.shape_of(up, down)
    fed = made = 0
    cuts = []
    for target in (TILE - 1, TILE, TILE + 1, 2*TILE + 1):
        n = need_of(fed, made, target, up, down)
        k = frames_of_call(fed, n, up, down)
        assert k >= target and (n == 0 or frames_of_call(fed, n - 1, up, down) < target)
        cuts.append(n)
        fed, made = fed + n, made + k
    return cuts


def check_hook(lib, up, down, channels):
    """one sequence of calls per ratio and channel count, six streams: noise cut as 0, no part, 1, H - 1, H, T + 1, rest; noise in calls whose
    k crosses a tile edge (1023, 1024, 1025, 2049); noise in a run of calls shorter than H, so that a window spans three calls; zeros; one
    NaN; +-inf.  Every stream ends with H frames of zeros: the frames made are the whole-clip mirror's Nr, bit for bit, sentinels kept"""
    L, M, H, T = rs.shape_of(up, down)
    rng = np.random.default_rng(2000*up + down + channels)
    noise = lambda n: rng.uniform(-1, 1, (channels, n)).astype(np.float32)
    special = 3*T + 37
    short = max(2*H//3, 1)
    clips = [noise(4*T + 11), noise(sum(tile_cuts(up, down))), noise(9*short), np.zeros((channels, special), np.float32), noise(special), noise(special)]
    clips[4][0, special//2] = np.nan
    clips[5][channels - 1, 5] = np.inf
    clips[5][0, special - 9] = -np.inf
    tiles = tile_cuts(up, down)
    cuts = [[0, -1, 1, H - 1, H, T + 1, clips[0].shape[1] - (T + 1 + 2*H)],
            tiles,
            [short]*9,
            [special//3, 0, special - special//3],
            [T, 7, special - T - 7],
            [special - 5, -1, 5]]
    fed = [np.concatenate([x, np.zeros((channels, H), np.float32)], axis=1) for x in clips]
    cuts = [c + [H] for c in cuts]
    ratios = [(up, down)]*len(clips)
    for src_offset, out_offset in ((1, 0), (3, 2)) if channels == 2 else ((2, 1),):
        got, want, made = run_hook(lib, fed, cuts, ratios, src_offset=src_offset, out_offset=out_offset)
        assert rs.same_floats(got, want), (up, down, channels, _differs(got, want))
    table = rs.library_taps(lib, up, down)
    for s, x in enumerate(clips):
        y = rs.mirror(x, up, down, table)
        assert made[s] == y.shape[1] == rs.resampled_length(x.shape[1], up, down), (s, made[s], y.shape)
        assert rs.same_floats(np.concatenate(stream_mirror(fed[s], cuts[s], up, down, table), axis=1), y), (up, down, s)
    # exactly the frames whose T taps reach the NaN are NaN
    y = rs.mirror(clips[4], up, down, table)
    i = (np.arange(y.shape[1], dtype=np.int64)*M)//L
    reached = (i - (H - 1) <= special//2) & (special//2 <= i + H)
    assert np.array_equal(np.isnan(y[0]), reached) and reached.any() and not reached.all() and not np.isnan(y[1:]).any(), (up, down)


FAR = ((160, 147, (1 << 33) + 5), (147, 640, (1 << 33) + 5), (160, 147, (1 << 40) + 123457), (147, 640, (1 << 40) + 123457))


def check_far_positions(lib, channels=2):
    """lines that start as zeros at 2^33 + 5 and 2^40 + 123457: the frames are the mirror's at those absolute n.  i, p and n*M have to be
    64-bit: a 32-bit one gives another phase and another span"""
    rng = np.random.default_rng(33)
    ratios = [(up, down) for up, down, _ in FAR]
    fed0 = [f for _, _, f in FAR]
    cuts, clips = [], []
    for up, down in ratios:
        L, M, H, T = rs.shape_of(up, down)
        c = [T + 5, 300, 1, 0, 700]
        cuts.append(c)
        clips.append(rng.uniform(-1, 1, (channels, sum(c))).astype(np.float32))
    got, want, made = run_hook(lib, clips, cuts, ratios, fed0=fed0)
    assert rs.same_floats(got, want), _differs(got, want)
    for (up, down, f), c, m in zip(FAR, cuts, made):
        L, M, H, T = rs.shape_of(up, down)
        assert m == due(f + sum(c) - H, L, M) - due(f - H, L, M) > 0
        assert f - H > 1 << 32                                                  # (i does not fit 32 bits)


def check_mixed(lib, channels=2):
    """eight ratios and two plain streams in one sequence of calls: the plain streams' rows of the output stay as they were"""
    rng = np.random.default_rng(78)
    ratios = list(rs.RATIOS[:3]) + [(1, 1)] + list(rs.RATIOS[3:6]) + [(5, 5)] + list(rs.RATIOS[6:])
    totals = [700, 2100, 1500, 900, 3000, 1100, 1300, 640, 5000, 600]
    cuts = []
    for s, n in enumerate(totals):
        first = (n*(s + 1))//13
        cuts.append([first, -1 if s % 3 == 0 else 0, 17, n - first - 17 - 100, 100])
    clips = [rng.uniform(-1, 1, (channels, n)).astype(np.float32) for n in totals]
    got, want, made = run_hook(lib, clips, cuts, ratios)
    assert rs.same_floats(got, want), _differs(got, want)
    assert len(set(rs.reduced(*r) for r in ratios) - {(1, 1)}) == 8 and made[3] == made[7] == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

SESSION_RATIOS = ((160, 147), (1, 1), (147, 160), (2, 3))                      # stream 1 is a plain one
SESSION_IN = ([20, 20, 20, 20], [700, 650, 128, 900], [333, 0, 500, 333], [1, 300, 77, 1], [512, 512, 512, 600])   # frames handed per call
SESSION_FACTORS = (1.0, 1.25, 0.8, 1.1, 1.0)                                   # outSamples = round(factor*k), at least 64
SESSION_SEED = 71
SEEK_IN = [700, 640, 800, 1200]
SEEK_RATES = [1.0, 0.8, 1.25, 1.0]
PLAIN = 1


def session_inputs(fmt, Cn=2):
    """-> (frames of the format [S, n, C], the planar float32 [S, C, n] they decode to) for the seek and the five calls"""
    S = len(SESSION_RATIOS)
    n = max(SEEK_IN) + sum(max(c) for c in SESSION_IN)
    x = np.stack([0.45*synth_input(s, Cn, n, 44100) + 0.2*synth_input(s + 5, Cn, n, 44100) for s in range(S)]).astype(np.float32)
    frames = fc.encode_frames(pc.frames_of(x), fmt)
    return frames, np.ascontiguousarray(np.transpose(fc.decode_frames(frames, fmt), (0, 2, 1))).astype(np.float32)


def set_session(batch):
    for s, (up, down) in enumerate(SESSION_RATIOS):
        batch.set_pcm_stream_resample(up, down, stream=s)


JUNK = [300, 300, 300, 300]


def check_session(lib, fmt, dithered, limiter=False, seek=False, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """processFrames of a batch with the setting against a twin without it that is fed the mirror's frames as F32 frames, with the same k
    and outSamples per call: five calls of uneven sizes, the first with k = 0.  The bytes are the twin's floats put through the format's
    output rule (dithered where the format can be); overs and peaks agree.  limiter: the stream limiter on in both, F32 on both sides --
    the bytes and the limiter's meters agree.  seek: a call, reset(), the same call again, then seekFrames and the five calls -- the reset
    and the seek clear the line, so the model starts again at each of them and the frames handed before leave no trace"""
    pkg = package()
    S, Cn = len(SESSION_RATIOS), 2
    frames, planar = session_inputs(fmt)
    tables = [None if rs.reduced(*q) == (1, 1) else rs.library_taps(lib, *q) for q in SESSION_RATIOS]
    r, t = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(2))
    set_session(r)
    assert [r.pcm_stream_resample(s) for s in range(S)] == [rs.reduced(*q) for q in SESSION_RATIOS]
    assert [r.stream_resample_latency(s) for s in range(S)] == [0 if tb is None else rs.shape_of(*q)[2] for tb, q in zip(tables, SESSION_RATIOS)]
    modes = [dc.MODES[s % 2] if dithered else dc.NONE for s in range(S)]
    for b in (r, t):
        b.set_pcm_level(lc.FIXED, 6.0 if limiter else 1.0, 1.0)                  # (a levelled batch meters peaks)
        if limiter:
            b.set_pcm_stream_limiter(True, 0.5)
    if dithered:
        for s in range(S):
            r.setPcmDither(modes[s], SESSION_SEED + s, stream=s)
    model = dict(fed=[0]*S, made=[0]*S, handed=[planar[s, :, :0] for s in range(S)], first=[0]*S, zero_k=False)

    def clear():
        model.update(fed=[0]*S, made=[0]*S, handed=[planar[s, :, :0] for s in range(S)])

    def model_call(s, x):
        """the model on everything handed since the clear, cut at the call: its last call's frames are this call's"""
        if tables[s] is None:
            return x
        history = np.concatenate([model["handed"][s], x], axis=1)
        y = stream_mirror(history, [model["fed"][s], x.shape[1]], *SESSION_RATIOS[s], tables[s])[1]
        assert y.shape[1] == frames_of_call(model["fed"][s], x.shape[1], *SESSION_RATIOS[s])
        model["handed"][s] = history
        model["fed"][s] += x.shape[1]
        model["made"][s] += y.shape[1]
        model["zero_k"] = model["zero_k"] or (y.shape[1] == 0 and x.shape[1] > 0)
        return y

    def twin_frames(ys):
        twin = np.zeros((S, max(max(y.shape[1] for y in ys), 1), Cn), np.float32)
        for s, y in enumerate(ys):
            twin[s, :y.shape[1]] = y.T
        return twin

    def process_call(pos, nin, factor, tag):
        most = max(nin)
        for s in range(S):
            if tables[s] is not None:
                k = frames_of_call(model["fed"][s], nin[s], *SESSION_RATIOS[s])
                assert r.stream_resample_frames(s, nin[s]) == k, (tag, s)
                need = r.stream_resample_need(s, max(k, 1))
                assert need == need_of(model["fed"][s], model["made"][s], max(k, 1), *SESSION_RATIOS[s]) and (k == 0 or need <= nin[s]), (tag, s, need)
                assert r.stream_resample_frames(s, need) >= max(k, 1) and (need == 0 or r.stream_resample_frames(s, need - 1) < max(k, 1)), (tag, s, need)
        ys = [model_call(s, planar[s, :, pos:pos + nin[s]]) for s in range(S)]
        ks = [y.shape[1] for y in ys]
        nout = [max(int(round(factor*k)), 64) for k in ks]
        twin = twin_frames(ys)
        fill = lambda like: np.full(like.shape[:1] + (max(nout),) + like.shape[2:], 0x5A, like.dtype)
        want = to_host(t.processFrames(to_memory(twin), nout, in_samples=ks, out=to_memory(fill(twin))))
        before = pkg.launch_count(COUNTER, lib)
        x = np.ascontiguousarray(frames[:, pos:pos + most])
        got = to_host(r.processFrames(to_memory(x), nout, in_samples=nin, out=to_memory(fill(x))))
        assert pkg.launch_count(COUNTER, lib) == before + 1, tag
        peaks_r, gains_r = r.take_pcm_peaks()
        peaks_t, gains_t = t.take_pcm_peaks()
        assert np.array_equal(rs.bits(peaks_r), rs.bits(peaks_t)) and np.array_equal(rs.bits(gains_r), rs.bits(gains_t)), (tag, peaks_r, peaks_t)
        overs_r, nans_r = r.takePcmOvers()
        if limiter:
            assert fmt == fc.F32 and np.array_equal(got.view(np.uint8), want.view(np.uint8)), tag
            for u, v in zip(r.take_pcm_stream_limiter(), t.take_pcm_stream_limiter()):
                assert np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)), (tag, u, v)
            return want
        expect = fill(frames)
        for s in range(S):
            v = np.ascontiguousarray(want[s, :nout[s]].T)                        # (the twin's floats: the engine's own output, gain 1)
            codes, cm, nm = dc.mirror(v, fmt, modes[s], SESSION_SEED + s, model["first"][s])
            expect[s, :nout[s]] = fc.to_rows(codes, fc.S24).reshape(codes.shape + (3,)) if fmt == fc.S24 else codes
            assert (int(overs_r[s]), int(nans_r[s])) == (int(cm.sum()), int(nm.sum())), (fmt, tag, s)
            model["first"][s] += nout[s]
        assert lc.same_bytes(got.reshape(-1).view(np.uint8), expect.reshape(-1).view(np.uint8), fmt), (fmt, dithered, tag)
        return want

    pos = 0
    if seek:
        process_call(0, JUNK, 1.0, "before the reset")
        for b in (r, t):
            b.reset()
        clear()
        process_call(0, JUNK, 1.0, "behind the reset")                          # (the same frames again: a line that was kept would show)
        clear()                                                                 # the seek clears the line before its frames go in
        assert [r.stream_resample_frames(s, SEEK_IN[s], fresh=True) for s in range(S)] == [n if tb is None else frames_of_call(0, n, *q) for n, tb, q in zip(SEEK_IN, tables, SESSION_RATIOS)]
        ys = [model_call(s, planar[s, :, :SEEK_IN[s]]) for s in range(S)]
        r.seekFrames(to_memory(np.ascontiguousarray(frames[:, :max(SEEK_IN)])), SEEK_RATES, in_samples=SEEK_IN)
        t.seekFrames(to_memory(twin_frames(ys)), SEEK_RATES, in_samples=[y.shape[1] for y in ys])
        pos = max(SEEK_IN)
    heard = False
    for call, nin in enumerate(SESSION_IN):
        want = process_call(pos, list(nin), SESSION_FACTORS[call], "call %d" % call)
        heard = heard or bool(want[:, :64].any())
        pos += max(nin)
    assert model["zero_k"] and heard                                            # (a call with k = 0 was among them, and the session makes sound)
    for b in (r, t):
        b.close()


# ---- opt-in, steady state, reproducible ----------------------------------------------------------------------------------------------

def _counts(lib):
    pkg = package()
    return [pkg.launch_count(k, lib) for k in COUNTERS]


def check_opt_in(lib, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
    """a batch that never set the ratio and one that set it and went back to 1/1: the same bytes, the same launches, none of the new kernel;
    in a mixed call the plain stream's bytes are those of a batch with no setting"""
    pkg = package()
    assert pkg.launch_count(COUNTER, lib) >= 0, "the library has no %s counter" % COUNTER
    S, Cn = len(SESSION_RATIOS), 2
    frames, _ = session_inputs(fc.S16)
    a, b, m = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY) for _ in range(3))
    b.set_pcm_stream_resample(160, 147)                                           # (the twin had a ratio once: 1/1 turns the stage off again)
    b.set_pcm_stream_resample(1, 1)
    x = [np.ascontiguousarray(frames[:, :700]), np.ascontiguousarray(frames[:, 700:1300])]
    outs, deltas = [], []
    for batch in (a, b):
        before = _counts(lib)
        out = [to_host(batch.processFrames(to_memory(x[0]), [700]*S)), to_host(batch.processFrames(to_memory(x[1]), [500, 600, 700, 600]))]
        batch.synchronize()
        outs.append(out)
        deltas.append([y - w for w, y in zip(before, _counts(lib))])
    assert all(np.array_equal(u, v) for u, v in zip(*outs)) and deltas[0] == deltas[1], (deltas[0], deltas[1])
    assert deltas[0][COUNTERS.index(COUNTER)] == 0 and deltas[0][COUNTERS.index("pcm_in")] == 2
    set_session(m)
    before = _counts(lib)
    mixed = [to_host(m.processFrames(to_memory(x[0]), [700]*S)), to_host(m.processFrames(to_memory(x[1]), [500, 600, 700, 600]))]
    delta = dict(zip(COUNTERS, [y - w for w, y in zip(before, _counts(lib))]))
    assert delta[COUNTER] == 2 and delta["pcm_in"] == 4, delta
    assert np.array_equal(mixed[0][PLAIN], outs[0][0][PLAIN]) and np.array_equal(mixed[1][PLAIN, :600], outs[0][1][PLAIN, :600]) and mixed[1][PLAIN].any()
    for batch in (a, b, m):
        batch.close()


def check_steady_state(lib, to_memory=lambda a: a):
    """the setter allocates the lines and the call tables, outside any call; after two calls the allocation events and the workspace bytes
    stand still over three more; setting a ratio that already has a table allocates nothing"""
    pkg = package()
    S, Cn = len(SESSION_RATIOS), 2
    frames = to_memory(np.ascontiguousarray(session_inputs(fc.S16)[0][:, :600]))
    b = pkg.StretchBatch(S, Cn, lib=lib, seed=3, **pc.GEOMETRY)
    plain = b.workspaceBytes()
    set_session(b)
    assert b.workspaceBytes() >= plain + 2*S*Cn*LINE*4                              # (the lines are in device memory from the setter on)
    for _ in range(2):
        b.processFrames(frames, [600, 500, 450, 300], in_samples=[600, 500, 512, 480])
    b.synchronize()
    events, grown = b.allocation_events(), b.workspaceBytes()
    for _ in range(3):
        b.processFrames(frames, [600, 500, 450, 300], in_samples=[600, 500, 512, 480])
    b.synchronize()
    assert (b.allocation_events(), b.workspaceBytes()) == (events, grown)
    b.set_pcm_stream_resample(320, 294, stream=PLAIN)                              # (160/147, which stream 0 has)
    assert (b.allocation_events(), b.workspaceBytes()) == (events, grown) and b.pcm_stream_resample(PLAIN) == (160, 147)
    b.close()


def run_session(lib, fmt=fc.S24):
    """-> (the five calls' frames, the k the calls delivered according to stream_resample_frames)"""
    pkg = package()
    S = len(SESSION_RATIOS)
    frames, _ = session_inputs(fmt)
    b = pkg.StretchBatch(S, 2, lib=lib, seed=3, **pc.GEOMETRY)
    set_session(b)
    outs, ks, pos = [], [], 0
    for nin in SESSION_IN:
        ks.append([b.stream_resample_frames(s, nin[s]) for s in range(S)])
        outs.append(np.array(b.processFrames(np.ascontiguousarray(frames[:, pos:pos + max(nin)]), [400]*S, in_samples=nin), copy=True))
        pos += max(nin)
    b.close()
    return outs, ks


def check_reproducible(lib):
    """two runs of the same session are bit-identical, and so are two batches; _frames agrees with the k of the definition, and _need is its
    inverse: _need(_frames(n)) <= n and _frames(_need(f)) >= f"""
    pkg = package()
    (a, ka), (b, kb) = run_session(lib), run_session(lib)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and ka == kb and any(u.any() for u in a)
    fed = [0]*len(SESSION_RATIOS)
    for nin, k in zip(SESSION_IN, ka):
        for s, q in enumerate(SESSION_RATIOS):
            assert k[s] == (nin[s] if rs.reduced(*q) == (1, 1) else frames_of_call(fed[s], nin[s], *q)), (s, nin, k)
            fed[s] += nin[s]
    bt = pkg.StretchBatch(2, 1, lib=lib, **pc.GEOMETRY)
    for up, down in rs.RATIOS:
        bt.set_pcm_stream_resample(up, down, stream=0)
        H = bt.stream_resample_latency(0)
        assert H == rs.shape_of(up, down)[2]
        for n in (0, 1, H, H + 1, 118, 441, 48000):
            k = bt.stream_resample_frames(0, n)
            assert k == frames_of_call(0, n, up, down)
            assert k == 0 or bt.stream_resample_need(0, k) <= n
        for f in (1, 2, 118, 480, 100000):
            assert bt.stream_resample_frames(0, bt.stream_resample_need(0, f)) >= f
        assert bt.stream_resample_frames(1, 77) == 77 and bt.stream_resample_need(1, 77) == 77 and bt.stream_resample_latency(1) == 0
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
        _refused(lib, lib.smst_batch_set_pcm_stream_resample(b.h, 0, up, down), word)
    for stream in (-2, S):
        _refused(lib, lib.smst_batch_set_pcm_stream_resample(b.h, stream, 2, 1), b"stream")
    for stream in (-1, S):
        _refused(lib, lib.smst_batch_pcm_stream_resample(b.h, stream, None, None), b"stream")
        _refused(lib, lib.smst_batch_pcm_stream_resample_latency(b.h, stream, None), b"stream")
        _refused(lib, lib.smst_batch_pcm_stream_resample_frames(b.h, stream, 100, 0), b"stream")
        _refused(lib, lib.smst_batch_pcm_stream_resample_need(b.h, stream, 100, 0), b"stream")
    _refused(lib, lib.smst_batch_set_pcm_stream_resample(None, 0, 2, 1), b"null")
    _refused(lib, lib.smst_batch_pcm_stream_resample(None, 0, None, None), b"null")
    _refused(lib, lib.smst_batch_pcm_stream_resample_latency(None, 0, None), b"null")
    _refused(lib, lib.smst_batch_pcm_stream_resample_frames(None, 0, 100, 0), b"null")
    _refused(lib, lib.smst_batch_pcm_stream_resample_need(None, 0, 100, 0), b"null")
    assert [b.pcm_stream_resample(s) for s in range(S)] == [(1, 1)]*S               # (a refused call changes nothing)
    assert lib.smst_batch_set_pcm_stream_resample(b.h, 0, 1280, 1176) == 0 and b.pcm_stream_resample(0) == (160, 147)   # (reduced first, then checked)
    assert b.pcm_resample(0) == (1, 1)                                              # (the whole-clip setting is another one)
    b.set_pcm_stream_resample(1, 1)
    # the shared slots: a ninth ratio across both settings is refused, and a slot is free once both users have gone
    for s, (up, down) in enumerate(rs.RATIOS):
        if s % 2:
            b.set_pcm_resample(up, down, stream=s)
        else:
            b.set_pcm_stream_resample(up, down, stream=s)
    _refused(lib, lib.smst_batch_set_pcm_stream_resample(b.h, 8, 4, 3), b"8")
    _refused(lib, lib.smst_batch_set_pcm_resample(b.h, 9, 5, 4), b"8")
    assert b.pcm_stream_resample(8) == b.pcm_resample(9) == (1, 1)
    b.set_pcm_stream_resample(1, 2, stream=8)                                       # (a ratio that is live through the other setting: no new slot)
    b.set_pcm_resample(1, 1, stream=1)                                              # 1/2 has lost one of its two users ...
    _refused(lib, lib.smst_batch_set_pcm_stream_resample(b.h, 9, 4, 3), b"8")
    b.set_pcm_stream_resample(1, 1, stream=8)                                       # ... and now both: its slot is free
    b.set_pcm_stream_resample(4, 3, stream=9)
    assert b.pcm_stream_resample(9) == (4, 3)
    _refused(lib, lib.smst_batch_set_pcm_resample(b.h, 1, 1, 2), b"8")
    b.set_pcm_stream_resample(1, 1)
    b.set_pcm_resample(1, 1)
    # a k or a count that does not fit an int
    b.set_pcm_stream_resample(9, 2, stream=0)
    assert b.stream_resample_frames(0, 477218588 + 32, fresh=True) == 2147483646
    _refused(lib, lib.smst_batch_pcm_stream_resample_frames(b.h, 0, 477218589 + 32, 1), b"2147483647")
    _refused(lib, lib.smst_batch_pcm_stream_resample_frames(b.h, 0, 1 << 62, 1), b"2147483647")
    _refused(lib, lib.smst_batch_pcm_stream_resample_frames(b.h, 0, -1, 0), b"negative")
    _refused(lib, lib.smst_batch_pcm_stream_resample_need(b.h, 0, 0, 0), b"2147483647")
    _refused(lib, lib.smst_batch_pcm_stream_resample_need(b.h, 0, 1 << 31, 0), b"2147483647")
    b.close()
    # the calls that do not serve the setting, and the whole-clip ratio in the streaming calls
    b = pkg.StretchBatch(3, Cn, lib=lib, **pc.GEOMETRY)
    b.set_pcm_stream_resample(3, 2, stream=1)
    frames = to_memory(np.zeros((3, 2000, Cn), np.int16))
    for call, word in ((lambda: b.exactFrames(frames, [2400, 2400, 2400]), "smst_batch_set_pcm_resample"), (lambda: b.outputSeekFrames(frames), "smst_batch_output_seek_pcm")):
        with dc.pytest_raises(pkg.StretchError) as e:
            call()
        assert "smst_batch_set_pcm_stream_resample" in str(e.value) and word in str(e.value) and "error -1" in str(e.value), str(e.value)
    b.exactFrames(frames, [2400, -1, 2400])                                         # (stream 1 takes no part: not refused)
    b.processFrames(frames, [600, 600, 600])
    b.seekFrames(frames, [1.0, 1.0, 1.0])
    b.flushFrames([100, 50, 100], like=to_memory(np.zeros((1,), np.float32)))       # (no input: unaffected)
    b.set_pcm_resample(3, 2, stream=1)                                              # (both settings on one stream: each call family reads its own)
    for call in (lambda: b.processFrames(frames, [600, 600, 600]), lambda: b.seekFrames(frames, [1.0, 1.0, 1.0])):
        with dc.pytest_raises(pkg.StretchError) as e:
            call()
        assert "smst_batch_exact_pcm only" in str(e.value), str(e.value)
    b.close()
    _refused(lib, lib.smst_debug_pcm_stream_resample(0, 1, 1, 0, None, None, None, None, 0, 0, None, 0, 0, 0, None), b"bad arguments")
