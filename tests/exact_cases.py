"""Shared cases of the whole-clip calls (smst_batch_exact / smst_batch_exact_pcm, include/smst.h): test_exact_emu.py runs them on the CPU
stand-in, test_exact_gpu.py on the device.

Every comparison is exact.  The two copy kernels (csrc/smst_clip.h) are checked against a numpy mirror of "count frames from frame src to
frame dst", with pcm_format_cases.mirror as the conversion rule; the batch call is checked against S single-stream handles
(SignalsmithStretch(seed + s).exact, itself pinned to the compiled reference by parity_cases.case_api_surface), the frame form against the
planar form on the decoded samples."""
import ctypes as C

import numpy as np

import pcm_cases as pc
import pcm_format_cases as pf
from conftest import package, synth_input

PLANAR = 0                                           # `format` of a caller's buffer that is planar fp32 itself
FRAME_FORMATS = (pf.S16, pf.F32, pf.S24, pf.S32, pf.F16)
GEOMETRY = pc.GEOMETRY                               # block 512, interval 128: the PCM tests' small geometry
PLANAR_TILE = 2048                                   # floats of a row one workgroup step of kClipPlanar moves (kClipTileFloats)
COUNTS = pc.COUNTS                                   # 0, 1, 7, 8, 9, 63, 64, 65, tile - 1, tile, tile + 1 of the frame kernels' tile
PLANAR_COUNTS = COUNTS + (PLANAR_TILE - 1, PLANAR_TILE, PLANAR_TILE + 1)
OFFSETS = (0, 1, 3, 4, 5, 511, 513)
ERR_INVALID, ERR_SHORT = -1, -3


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def _vp(a):
    return C.c_void_p(a.ctypes.data)


# ---- 1. the copy kernels against a numpy mirror ---------------------------------------------------------------------------------------

def segment_tables(counts, channels, direction):
    """-> a list of int32 [4, 2, 4] tables (source frame, destination frame, count, zeros) for S = 4 streams that between them use every
    count and, on both sides, every offset of OFFSETS (asserted).  A stream's second segment lies 600 frames on in the source and behind
    its first one in the destination, so the two never overlap there; table 0 has a stream with both segments empty and (direction 1) a
    "zeros" segment."""
    counts = list(counts)
    rounds = -(-len(counts)//6)
    tables, k = [], 0
    src_seen, dst_seen = set(), set()
    for r in range(rounds):
        t = np.zeros((4, 2, 4), np.int32)
        for s in range(4):
            if r == 0 and s == 3:
                continue                                 # both segments empty
            for g in range(2):
                zeros = direction == 1 and r == 0 and s == 1 and g == 0
                n = 70 if zeros else counts[k % len(counts)]
                src_off, dst_off = OFFSETS[(k + channels) % len(OFFSETS)], OFFSETS[(3*k + 1 + direction) % len(OFFSETS)]
                t[s, g] = (src_off + g*600, dst_off + (0 if g == 0 else t[s, 0, 1] + t[s, 0, 2]), n, 1 if zeros else 0)
                if not zeros:
                    k += 1
                    src_seen.add(src_off)
                dst_seen.add(dst_off)
        tables.append(t)
    seen = {int(n) for t in tables for n in t[:, :, 2].reshape(-1)}
    assert set(counts) <= seen, sorted(set(counts) - seen)
    assert src_seen == set(OFFSETS) and dst_seen == set(OFFSETS), (sorted(src_seen), sorted(dst_seen))
    return tables


def clip_copy(lib, direction, fmt, channels, segs, src, src_ss, src_inner, dst, dst_ss, dst_inner, counted=False):
    segs = np.ascontiguousarray(segs, np.int32)
    S = segs.shape[0]
    clamped, nans = np.full(S, -1, np.int64), np.full(S, -1, np.int64)
    rc = lib.smst_debug_clip_copy(0, direction, fmt, S, channels, _ip(segs), _vp(src), src_ss, src_inner, _vp(dst), dst_ss, dst_inner,
                                  _lp(clamped) if counted else None, _lp(nans) if counted else None)
    assert rc == 0, (fmt, (lib.smst_last_error() or b"").decode())
    return clamped, nans


def _caller_values(fmt, n, rng):
    """n values of the caller's side as the input of a copy: any code / bit pattern of the format"""
    if fmt in (PLANAR, pf.F32):
        return rng.uniform(-1.5, 1.5, n).astype(np.float32)
    return pc._pcm_values(fmt, n, rng) if fmt == pf.S16 else pf._pcm_values(fmt, n, rng)


def _image_values(fmt, n, rng):
    """n floats of the image as the input of a copy: ties, values beyond full scale, NaN"""
    if fmt in (PLANAR, pf.F32, pf.S16):
        x = pc._planar_values(pf.S16, n, rng)
        x[rng.integers(0, n, max(n//200, 1))] = np.nan
        return x
    return pf._planar_values(fmt, n, rng)


def check_clip_kernels(lib, fmt, channels, byte_offsets, wide_frames=False, image_offsets=(1,)):
    """Both directions of one format (PLANAR: the caller's side is planar fp32) for S = 4 streams with different segment tables, the
    caller's buffer based at every given byte offset behind a 16-byte boundary and the image at every given offset in floats (each with
    each), deliberately odd strides on both sides; frames of frameStride = C + 1 with wide_frames.  The destination is filled with a sentinel: the copied elements equal the mirror's, every other
    byte comes back unchanged, and the overs counts equal the mirror's."""
    S, Cn = 4, channels
    planar = fmt == PLANAR
    esz = 4 if planar else pf.ELEM_BYTES[fmt]
    fs = Cn + 1 if wide_frames else Cn
    for direction in (0, 1):
        for table_no, segs in enumerate(segment_tables(PLANAR_COUNTS if planar else COUNTS, Cn, direction)):
            live = segs[:, :, 2] > 0
            src_end = int(np.max(np.where(live & (segs[:, :, 3] == 0), segs[:, :, 0] + segs[:, :, 2], 0)))
            dst_end = int(np.max(np.where(live, segs[:, :, 1] + segs[:, :, 2], 0)))
            caller_end, image_end = (src_end, dst_end) if direction == 0 else (dst_end, src_end)
            caller_end, image_end = max(caller_end, 1), max(image_end, 1)
            # the image: rows of an odd pitch.  The caller's side: a planar buffer of other odd pitches, or frames
            ics, iss = image_end + 3, Cn*(image_end + 3) + 5
            image_len = (S - 1)*iss + (Cn - 1)*ics + image_end
            if planar:
                cin, css = caller_end + 1, Cn*(caller_end + 1) + 3           # (inner stride = channel stride)
                caller_len = (S - 1)*css + (Cn - 1)*cin + caller_end
                cidx = lambda s, c, f0, n: s*css + c*cin + f0 + np.arange(n)
            else:
                cin, css = fs, caller_end*fs + 3                              # (inner stride = frame stride)
                caller_len = (S - 1)*css + (caller_end - 1)*fs + Cn
                cidx = lambda s, c, f0, n: s*css + (f0 + np.arange(n))*fs + c
            iidx = lambda s, c, f0, n: s*iss + c*ics + f0 + np.arange(n)
            for offset, image_offset in ((o, i) for o in byte_offsets for i in image_offsets):
                rng = pc._rng(4242, fmt, Cn, direction, table_no, offset, fs)
                where = dict(fmt=fmt, C=Cn, direction=direction, table=table_no, byte_offset=offset, image_offset=image_offset, frame_stride=fs)
                if direction == 0:
                    values = _caller_values(fmt, caller_len, rng)
                    src = pf.byte_buffer(caller_len*esz, offset)
                    src.reshape(-1, esz)[:] = values.view(np.uint8).reshape(-1, 4) if planar else pf.to_rows(values, fmt)
                    dst = pc.aligned(image_len, np.float32, image_offset)
                    dst[:] = 777.0
                    want = dst.copy()
                    for s in range(S):
                        for a, b, n, z in segs[s]:
                            for c in range(Cn):
                                v = values[cidx(s, c, a, n)]
                                want[iidx(s, c, b, n)] = v if planar else pf.decode(v, fmt)
                    clip_copy(lib, 0, fmt, Cn, segs, src, css, cin, dst, iss, ics)
                    assert pf.same_values(dst, want, pf.F16 if fmt == pf.F16 else pf.F32), ("caller -> image", where)
                else:
                    src = pc.aligned(image_len, np.float32, image_offset)
                    src[:] = _image_values(fmt, image_len, rng)
                    dst = pf.byte_buffer(caller_len*esz, offset)
                    dst[:] = 0x5A
                    want = dst.copy()
                    rows = want.reshape(-1, esz)
                    want_c, want_n = np.zeros(S, np.int64), np.zeros(S, np.int64)
                    for s in range(S):
                        for a, b, n, z in segs[s]:
                            for c in range(Cn):
                                v = np.zeros(n, np.float32) if z else src[iidx(s, c, a, n)]
                                if planar:
                                    rows[cidx(s, c, b, n)] = np.ascontiguousarray(v).view(np.uint8).reshape(-1, 4)
                                else:
                                    codes, cm, nm = pf.mirror(v, fmt)
                                    rows[cidx(s, c, b, n)] = pf.to_rows(codes, fmt)
                                    want_c[s] += cm.sum()
                                    want_n[s] += nm.sum()
                    clamped, nans = clip_copy(lib, 1, fmt, Cn, segs, src, iss, ics, dst, css, cin, counted=not planar)
                    if fmt == pf.F16:
                        assert pf.same_values(pf.from_rows(dst.reshape(-1, esz), fmt), pf.from_rows(rows, fmt), fmt), ("image -> caller", where)
                    else:
                        assert np.array_equal(dst, want), ("image -> caller", where)
                    if not planar:
                        assert np.array_equal(clamped, want_c) and np.array_equal(nans, want_n), (where, clamped.tolist(), want_c.tolist(), nans.tolist(), want_n.tolist())


IMAGE_ALIGNMENTS = (0, 1, 2, 3)                      # floats behind a 16-byte boundary: every alignment the planar image can have


def sub_alignments(fmt):
    """every offset behind a 16-byte boundary a buffer of the format can have"""
    return tuple(range(0, 16, 1 if fmt == pf.S24 else 4 if fmt == PLANAR else pf.ELEM_BYTES[fmt]))


# ---- 2. the batch call against S single-stream handles --------------------------------------------------------------------------------

# Five clips of five lengths; one of them too short.  Rates 0.4 (beyond a 2x stretch: the seeded random time factors are drawn), 0.8 / 1.0,
# 2/3 on the short one, 1.25 and 1.7.  check_lengths() verifies on the host that the four others pass in >= outputSeekLength(rate):
# with block 512 / interval 128 that length is int(256 + rate*256), or int(256 + rate*384) with split computation -- at most 908.
CLIPS = dict(inputs=[3000, 4000, 200, 6250, 6800], outputs=[7500, 5000, 300, 5000, 4000], short=2)
CLIPS_UNITY = dict(inputs=[3000, 5000, 200, 6250, 6800], outputs=[7500, 5000, 300, 5000, 4000], short=2)   # (stream 1 at rate 1.0)


def check_lengths(batch, clips):
    for s, (n, m) in enumerate(zip(clips["inputs"], clips["outputs"])):
        need = batch.outputSeekLength(float(np.float32(n)/np.float32(m)))
        assert (n < need) == (s == clips["short"]), (s, n, m, need)


def clip_inputs(channels, lengths, loud=None):
    """[S, C, max length] float32: a clip of conftest.synth_input per stream, zero behind its length.  loud: that stream is normalised to a
    peak of 1.2 (it clips in every integer format)."""
    S, most = len(lengths), max(lengths)
    x = np.zeros((S, channels, most), np.float32)
    for s, n in enumerate(lengths):
        x[s, :, :n] = synth_input(s, channels, n, 48000) + 0.3*synth_input(s + 4, channels, n, 48000)
    if loud is not None:
        x[loud] *= np.float32(1.2)/np.abs(x[loud]).max()
    return x


def host_exact(batch, x, nout, nin, frames=False):
    out, ok = (batch.exactFrames if frames else batch.exact)(x, nout, in_samples=nin)
    return np.array(out, copy=True), ok


def single_handles(lib, channels, x, nin, nout, seed, split):
    """-> [(out [C, nout[s]], ok)] of SignalsmithStretch(seed + s).exact, one fresh handle per stream"""
    res = []
    for s in range(len(nin)):
        h = package().SignalsmithStretch(seed=seed + s, lib=lib)
        h.configure(channels, GEOMETRY["block"], GEOMETRY["interval"], split)
        res.append(h.exact(np.ascontiguousarray(x[s, :, :nin[s]]), nout[s]))
        h.close()
    return res


def check_equals_single_handles(lib, channels, clips, split, run=host_exact, seed=11):
    nin, nout, short = clips["inputs"], clips["outputs"], clips["short"]
    x = clip_inputs(channels, nin)
    b = package().StretchBatch(len(nin), channels, lib=lib, split=split, seed=seed, **GEOMETRY)
    check_lengths(b, clips)
    got, ok = run(b, x, nout, nin)
    b.close()
    want = single_handles(lib, channels, x, nin, nout, seed, split)
    assert ok.tolist() == [s != short for s in range(len(nin))] and [w[1] for w in want] == ok.tolist()
    for s, (w, _) in enumerate(want):
        assert np.array_equal(got[s, :, :nout[s]].view(np.uint32), np.ascontiguousarray(w).view(np.uint32)), ("stream", s, "C", channels, "split", split)
        assert (got[s, :, nout[s]:] == 0).all()
        assert (s == short) == (not np.any(got[s])), s                       # zeros for the short one, sound for every other
    return got


def check_against_reference(lib, ref, split):
    """two streams against the compiled reference's own exact(), with parity_cases' comparison and caps: the stream under test is stream 0
    of a two-stream batch of seed 0 (check_scenario's instances are of seed 0), the other stream a clip of another length and rate"""
    import parity_cases as pcs
    cfg = dict(preset="configure", split=split, **GEOMETRY)
    legs = [((6000, 7000), (4000, 3000)), ((4000, 3000), (6000, 7000))]
    for (n0, m0), (n1, m1) in legs:
        x0 = synth_input(0, 2, n0, 48000) + 0.3*synth_input(1, 2, n0, 48000)
        other = synth_input(2, 2, n1, 48000)

        def play(o, xx):
            if hasattr(o, "lib"):                                            # the product: the batch call stands in for the handle
                x = np.zeros((2, 2, max(n0, n1)), np.float32)
                x[0, :, :n0], x[1, :, :n1] = xx, other
                b = package().StretchBatch(2, 2, lib=lib, split=split, seed=0, **GEOMETRY)
                out, ok = b.exact(x, [m0, m1], in_samples=[n0, n1])
                b.close()
                assert ok.all()
                return np.array(out[0, :, :m0], copy=True)
            out, ok = o.exact(xx, m0)
            assert ok
            return out
        pcs.check_scenario(lib, ref, cfg, x0, play, "batch exact %d -> %d" % (n0, m0))


# ---- 3. masks -------------------------------------------------------------------------------------------------------------------------

def raw_exact(lib, batch, x, nin, nout, out, status, memory=0):
    """smst_batch_exact itself on [S, C, n] float32 arrays (the caller keeps out and status)"""
    nin, nout = np.ascontiguousarray(nin, np.int32), np.ascontiguousarray(nout, np.int32)
    Cn = x.shape[1]
    return lib.smst_batch_exact(batch.h, _vp(x), Cn*x.shape[2], x.shape[2], _ip(nin), _vp(out), Cn*out.shape[2], out.shape[2], _ip(nout), _ip(status), memory)


def check_masks(lib, split):
    """Two process calls on all streams, then exact with stream 1 too short and stream 3 left out, then process on all streams: streams 1
    and 3 go on bit for bit as in a twin batch that never saw the exact call, stream 3's output region and status entry keep their sentinel."""
    S, Cn = 5, 2
    pkg = package()
    a, twin = (pkg.StretchBatch(S, Cn, lib=lib, split=split, seed=5, **GEOMETRY) for _ in range(2))
    x = clip_inputs(Cn, [9000]*S)
    calls = [([700, 500, 300, 650, 0], [600, 500, 310, 700, 0]), ([400, 0, 515, 300, 129], [380, 5, 500, 300, 128])]      # (out, in)
    pos, outs = 0, {id(a): [], id(twin): []}
    def step(b, nout, nin):
        outs[id(b)].append(np.array(b.process(np.ascontiguousarray(x[:, :, pos:pos + max(nin)]), nout, in_samples=nin), copy=True))
    for nout, nin in calls:
        step(a, nout, nin), step(twin, nout, nin)
        pos += max(nin)
    nin, nout = [3000, 200, 4000, 5000, 3500], [3600, 300, 3000, -1, 4000]
    clip = np.ascontiguousarray(x[:, :, 1000:6000])
    out = np.full((S, Cn, 4000), 777.0, np.float32)
    status = np.full(S, 99, np.int32)
    assert raw_exact(lib, a, clip, nin, nout, out, status) == 0, lib.smst_last_error()
    assert status.tolist() == [0, ERR_SHORT, 0, 99, 0]
    assert (out[3] == 777.0).all() and (out[1, :, :300] == 0).all() and (out[1, :, 300:] == 777.0).all()
    for s in (0, 2, 4):
        assert np.any(out[s, :, :nout[s]] != 0) and (out[s, :, nout[s]:] == 777.0).all()
    for nout, nin in [([500, 640, 300, 700, 100], [500, 600, 310, 650, 100]), ([128, 300, 0, 257, 0], [128, 280, 0, 250, 0])]:
        step(a, nout, nin), step(twin, nout, nin)
        pos += max(nin)
    for k, (p, q) in enumerate(zip(outs[id(a)], outs[id(twin)])):
        for s in (1, 3):
            assert np.array_equal(p[s].view(np.uint32), q[s].view(np.uint32)), ("call", k, "stream", s)
        assert k < 2 or not np.array_equal(p[0], q[0])                       # (stream 0 did start afresh)
    for s in (1, 3):
        for which in range(4):
            assert np.array_equal(a.debug_state(s, which), twin.debug_state(s, which)), (s, which)
    a.close()
    twin.close()


# ---- 4. frames ------------------------------------------------------------------------------------------------------------------------

def check_frames_equal_planar(lib, fmt, run_frames=None, run_planar=host_exact):
    """exactFrames = the planar exact on the decoded input, encoded by the mirror -- overs included; stream 0 is loud enough to clip"""
    run_frames = run_frames or (lambda b, x, nout, nin: host_exact(b, x, nout, nin, frames=True))
    nin, nout, short = CLIPS["inputs"], CLIPS["outputs"], CLIPS["short"]
    S, Cn = len(nin), 2
    frames = pf.encode_frames(pc.frames_of(clip_inputs(Cn, nin, loud=0)), fmt)
    planar = np.ascontiguousarray(np.transpose(pf.decode_frames(frames, fmt), (0, 2, 1)))
    pkg = package()
    p, f = (pkg.StretchBatch(S, Cn, lib=lib, seed=3, **GEOMETRY) for _ in range(2))
    want, ok_p = run_planar(p, planar, nout, nin)
    assert f.takePcmOvers()[0].tolist() == [0]*S
    got, ok_f = run_frames(f, frames, nout, nin)
    assert ok_p.tolist() == ok_f.tolist() == [s != short for s in range(S)]
    expect = pf.encode_frames(pc.frames_of(want), fmt)
    assert got.dtype == expect.dtype and got.shape == expect.shape, (got.dtype, got.shape, expect.dtype, expect.shape)
    assert pf.same_values(got, expect, fmt), fmt
    want_c = np.zeros(S, np.int64)
    for s in range(S):
        _, cm, nm = pf.mirror(want[s, :, :nout[s]], fmt)
        want_c[s] = cm.sum()
        assert not nm.any()
    clamped, nans = f.takePcmOvers()
    assert clamped.tolist() == want_c.tolist() and nans.tolist() == [0]*S, (fmt, clamped.tolist(), want_c.tolist(), nans.tolist())
    assert (clamped[0] > 0) == (fmt in (pf.S16, pf.S24, pf.S32)) and clamped[short] == 0, (fmt, clamped.tolist())
    p.close()
    f.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------

def check_refusals(lib):
    S, Cn = 3, 2
    pkg = package()
    b, twin = (pkg.StretchBatch(S, Cn, lib=lib, seed=1, **GEOMETRY) for _ in range(2))
    x = clip_inputs(Cn, [3000]*S)
    for q in (b, twin):
        q.process(np.ascontiguousarray(x[:, :, :1000]), 900)
    out = np.full((S, Cn, 3000), 777.0, np.float32)
    status = np.full(S, 99, np.int32)
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    nin, nout = ints([3000]*S), ints([2500]*S)
    px, po, ps, null = _vp(x), _vp(out), _ip(status), C.c_void_p(None)
    planar = lambda pin, n_in, pout, n_out: lib.smst_batch_exact(b.h, pin, Cn*3000, 3000, _ip(n_in), pout, Cn*3000, 3000, _ip(n_out), ps, pkg.MEM_HOST)
    framed = lambda fmt, ifs, ofs, pin=px: lib.smst_batch_exact_pcm(b.h, pin, Cn*3000, ifs, _ip(nin), po, Cn*3000, ofs, _ip(nout), ps, fmt, pkg.MEM_HOST)
    refused = lambda rc, word: rc == ERR_INVALID and word in lib.smst_last_error()
    assert refused(planar(px, nin, po, ints([2500, 0, 2500])), b"outSamples")
    assert refused(planar(px, ints([3000, -1, 3000]), po, nout), b"negative")
    assert refused(planar(null, nin, po, nout), b"null buffer") and refused(planar(px, nin, null, nout), b"null buffer")
    assert refused(framed(7, Cn, Cn), b"format") and refused(framed(3, Cn, Cn), b"format")
    assert refused(framed(pf.S16, Cn - 1, Cn), b"frame stride") and refused(framed(pf.S16, Cn, Cn - 1), b"frame stride")
    assert refused(framed(pf.F32, Cn, Cn, null), b"null buffer")
    assert planar(px, ints([3000, -1, 3000]), po, ints([2500, -1, 2500])) == 0     # (a negative inSamples on a stream that is left out is no refusal)
    assert status.tolist() == [0, 99, 0]
    b.close()
    # the refusals happened before anything ran: a batch that saw only them goes on as its twin
    b = pkg.StretchBatch(S, Cn, lib=lib, seed=1, **GEOMETRY)
    b.process(np.ascontiguousarray(x[:, :, :1000]), 900)
    out[:], status[:] = 777.0, 99
    planar = lambda pin, n_in, pout, n_out: lib.smst_batch_exact(b.h, pin, Cn*3000, 3000, _ip(n_in), pout, Cn*3000, 3000, _ip(n_out), ps, pkg.MEM_HOST)
    assert planar(px, nin, po, ints([2500, 0, 2500])) == ERR_INVALID and planar(px, ints([3000, -1, 3000]), po, nout) == ERR_INVALID
    assert planar(null, nin, po, nout) == ERR_INVALID
    assert lib.smst_batch_exact_pcm(b.h, px, Cn*3000, Cn, _ip(nin), po, Cn*3000, Cn, _ip(nout), ps, 7, pkg.MEM_HOST) == ERR_INVALID
    assert lib.smst_batch_exact_pcm(b.h, px, Cn*3000, Cn - 1, _ip(nin), po, Cn*3000, Cn, _ip(nout), ps, pf.F32, pkg.MEM_HOST) == ERR_INVALID
    assert (out == 777.0).all() and (status == 99).all()
    y, z = (q.process(np.ascontiguousarray(x[:, :, 1000:2000]), 1100) for q in (b, twin))
    assert np.array_equal(np.asarray(y).view(np.uint32), np.asarray(z).view(np.uint32)) and np.any(y)
    for s in range(S):
        for which in range(4):
            assert np.array_equal(b.debug_state(s, which), twin.debug_state(s, which))
    b.close()
    twin.close()


# ---- 6. steady state and accounting ---------------------------------------------------------------------------------------------------

ANALYSE_COUNTERS = ("analyse_teams", "analyse_fast", "analyse_generic")


def analyse_launches(lib):
    return sum(package().launch_count(name, lib=lib) for name in ANALYSE_COUNTERS)


def image_bytes(batch, nin, nout, frames):
    """what the first exact call adds to workspaceBytes, restated from DESIGN.md section 4 / Batch::exact: the two images [S][C][pitch] --
    the column of a stage and the pitch rounded up to 4 floats, a caller's planar buffer serving the two stages at offset 0 itself --, each
    allocated with 1/8 + 1024 floats of room, and two sets of segment tables of 4 entries of 16 bytes per stream"""
    f32 = np.float32
    S, Cn = batch.streams, batch.channels
    seek, rest, index, tail = [0], [0], [0], [0]
    for n, m in zip(nin, nout):
        rate = f32(n)/f32(m)
        k = batch.outputSeekLength(float(rate))
        if m < 0 or n < k:
            continue
        i = min(max(int(f32(m) - f32(k)/rate), 0), m)
        seek.append(k), rest.append(n - k), index.append(i), tail.append(m - i)
    up4 = lambda v: (v + 3)//4*4
    room = lambda v: v + v//8 + 1024
    p, q = (up4(max(seek)), up4(max(index))) if frames else (0, 0)
    pitch_in, pitch_out = max(up4(p + max(rest)), 4), max(up4(q + max(tail)), 4)
    return 4*(room(S*Cn*pitch_in) + room(S*Cn*pitch_out)) + 2*4*S*16


def check_steady_state(lib, run, frames=False):
    """allocation_events stands still across the second and third call of the same shapes; workspaceBytes has grown by exactly what the
    first call allocated -- the two images and the segment tables (the staging of a host-memory call is no workspace: it is counted by
    allocation_events only, as the other host-memory calls' is) -- and stands still as well"""
    nin, nout = CLIPS["inputs"], CLIPS["outputs"]
    S, Cn = len(nin), 2
    x = clip_inputs(Cn, nin)
    if frames:
        x = pf.encode_frames(pc.frames_of(x), pf.S16)
    b = package().StretchBatch(S, Cn, lib=lib, seed=2, **GEOMETRY)
    ws0 = b.workspaceBytes()
    run(b, x, nout, nin)
    events, ws1 = b.allocation_events(), b.workspaceBytes()
    assert ws1 - ws0 == image_bytes(b, nin, nout, frames), (ws0, ws1, image_bytes(b, nin, nout, frames))
    for _ in range(2):                                                       # (the output differs from call to call where random time factors are
        run(b, x, nout, nin)                                                 # drawn: reset() leaves an instance's random engine alone, :49-60)
    assert b.allocation_events() == events and b.workspaceBytes() == ws1
    b.close()


def check_one_main_process(lib, run):
    """One exact call launches the engine's main process once however many distinct rates there are: the analysis launches of the call with
    five lengths and rates equal those of a call in which every stream has the longest clip's length and rate (a call per distinct
    input offset would multiply them); and the two copy kernels ran."""
    pkg = package()
    nin, nout = CLIPS["inputs"], CLIPS["outputs"]
    S, Cn = len(nin), 2
    assert nout[0] == max(nout)                                              # stream 0 has the most hops in every stage
    x = clip_inputs(Cn, nin)
    same = np.ascontiguousarray(np.broadcast_to(x[0], x.shape))
    counts = []
    for clip, n_in, n_out in ((same, [nin[0]]*S, [nout[0]]*S), (x, nin, nout)):
        b = pkg.StretchBatch(S, Cn, lib=lib, seed=2, **GEOMETRY)
        before = analyse_launches(lib), pkg.launch_count("clip_in", lib=lib), pkg.launch_count("clip_out", lib=lib)
        run(b, clip, n_out, n_in)
        b.synchronize()
        counts.append((analyse_launches(lib) - before[0], pkg.launch_count("clip_in", lib=lib) - before[1], pkg.launch_count("clip_out", lib=lib) - before[2]))
        b.close()
    assert counts[0][0] > 0 and counts[1][0] == counts[0][0], counts
    assert counts[0][1:] == (1, 1) and counts[1][1:] == (1, 1), counts
