#!/usr/bin/env python3
"""Whole clips in device memory: one smst_batch_exact call against the three-call sequence it replaces (smst_batch_output_seek,
smst_batch_process, smst_batch_flush with the stage lengths computed by the caller), and the call with a different rate per stream, for
which there is no three-call equivalent.  Prints one JSON line per mode: the median over --steps calls after --warmup, each call timed on
the host from its first entry point to the return of smst_batch_synchronize.

  python tools/bench_exact.py --mode three        # the yardstick (also runs on a build without smst_batch_exact: SMST_LIBRARY)
  python tools/bench_exact.py --mode exact --check   # ... and compares the first call's output with the three-call sequence, bit for bit
  python tools/bench_exact.py --mode ragged       # per-stream rates drawn from [0.5, 2.0)
  python tools/bench_exact.py --mode pcm          # smst_batch_exact_pcm on int16 frames (also on a build without the level calls: SMST_LIBRARY)
  python tools/bench_exact.py --mode level        # pcm, fixed (a gain of 0.5 on every stream) and protect (ceiling 32766/32768) alternating step by
                                                  # step, a batch each: fixed - pcm = the levelled copy kernel, protect - fixed = the peak pass
  python tools/bench_exact.py --mode normalise --loudness   # NORMALISE and LOUDNESS (-23 LUFS at --sample-rate) alternating: loudness - normalise =
                                                  # the four loudness passes (mode normalise alone also runs on a build without them: SMST_LIBRARY)
  python tools/bench_exact.py --mode normalise --true-peak  # NORMALISE without and with the true-peak flag alternating: true_peak - normalise =
                                                  # the true-peak pass
  python tools/bench_exact.py --mode protect --limit        # PROTECT (at --limit-gain, so that the ceiling bites) without and with the limiter flag
                                                  # alternating: limit - protect = the limiter's two passes and the limited copy's extra read
  python tools/bench_exact.py --mode pcm --resample=160/147   # pcm without and with that resample ratio on every stream alternating, the resampled
                                                  # batch's clips as long as resample to the plain batch's input length: resample - pcm = the raw
                                                  # image's copy and kClipResample
  python tools/bench_exact.py --mode normalise --loudness --loudness-range   # ... and LOUDNESS with the meter flag: loudness_range - loudness =
                                                  # the range stage (kLoudRange) behind the four passes
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # (INTEGRATION.md "Hardware queues"; before the HIP runtime starts)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

smst = importlib.import_module("signalsmith-stretch_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["three", "exact", "ragged", "pcm", "fixed", "protect", "level", "normalise"], required=True)
    ap.add_argument("--loudness", action="store_true", help="frame modes: a batch in LEVEL_LOUDNESS (-23 LUFS, ceiling 32766/32768) beside the mode's own")
    ap.add_argument("--true-peak", action="store_true", help="frame modes: a batch with the mode's own level setting and the true-peak flag on every stream beside the mode's own")
    ap.add_argument("--limit", action="store_true", help="frame modes protect / normalise: a batch with the mode's own level setting and the limiter flag on every stream beside the mode's own")
    ap.add_argument("--loudness-range", action="store_true", help="frame modes: a batch in LEVEL_LOUDNESS with the loudness-range meter flag on every stream beside the mode's own")
    ap.add_argument("--resample", default=None, metavar="UP/DOWN", help="frame modes: a batch whose streams all carry this resample ratio, fed clips that resample to the "
                    "mode's own input length, beside the mode's own")
    ap.add_argument("--limit-gain", type=float, default=4.0, help="--limit: the PROTECT gain of both batches (+12 dB: most tiles hold frames over the ceiling)")
    ap.add_argument("--limit-lookahead", type=int, default=72, help="--limit: the lookahead in frames")
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sample-rate", type=float, default=48000.0)
    ap.add_argument("--stretch", type=float, default=1.5, help="uniform modes: output length / input length")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="mode exact: the first call's output equals the three-call sequence of a twin batch")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lib = smst.load_library()
    S, Cn, n = a.streams, a.channels, int(a.seconds*a.sample_rate)
    if a.mode == "ragged":
        rates = np.random.default_rng(1).uniform(0.5, 2.0, S)
        nout = np.maximum((n/rates).astype(np.int64), 1).astype(np.int32)
    else:
        nout = np.full(S, int(n*a.stretch), np.int32)
    nin = np.full(S, n, np.int32)
    g = torch.Generator(device="cuda").manual_seed(7)
    t = torch.arange(n, device="cuda", dtype=torch.float32)/a.sample_rate
    f = 110.0*2**(torch.arange(S*Cn, device="cuda", dtype=torch.float32).reshape(S, Cn, 1) % 37/12)
    x = (0.4*torch.sin(2*np.pi*f*t) + 0.05*torch.rand((S, Cn, n), generator=g, device="cuda") - 0.025).contiguous()
    most = int(nout.max())
    out = torch.zeros((S, Cn, most), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int))

    def batch():
        return smst.StretchBatch(S, Cn, preset="default", sample_rate=a.sample_rate, seed=0)

    def three(b, y):
        """exact() by hand, one rate for all streams: the stage lengths of signalsmith-stretch.h:468-491"""
        rate = float(np.float32(n)/np.float32(nout[0]))
        seek = b.outputSeekLength(rate)
        index = int(np.float32(nout[0]) - np.float32(seek)/np.float32(rate))
        ints = lambda v: np.full(S, v, np.int32)
        k, r, m, tail = ints(seek), ints(n - seek), ints(index), ints(int(nout[0]) - index)
        rates32 = np.full(S, rate, np.float32)
        smst._check(lib, lib.smst_batch_output_seek(b.h, C.c_void_p(x.data_ptr()), Cn*n, n, ip(k), smst.MEM_DEVICE))
        smst._check(lib, lib.smst_batch_process(b.h, C.c_void_p(x.data_ptr() + 4*seek), Cn*n, n, ip(r), C.c_void_p(y.data_ptr()), Cn*most, most, ip(m), smst.MEM_DEVICE))
        smst._check(lib, lib.smst_batch_flush(b.h, C.c_void_p(y.data_ptr() + 4*index), Cn*most, most, ip(tail), rates32.ctypes.data_as(C.POINTER(C.c_float)), smst.MEM_DEVICE))

    def exact(b, y):
        status = np.zeros(S, np.int32)
        smst._check(lib, lib.smst_batch_exact(b.h, C.c_void_p(x.data_ptr()), Cn*n, n, ip(nin), C.c_void_p(y.data_ptr()), Cn*most, most, ip(nout), ip(status), smst.MEM_DEVICE))
        assert not status.any(), status

    if a.mode in ("pcm", "fixed", "protect", "level", "normalise"):
        return frames_modes(a, lib, x, nin, nout, batch)
    call = three if a.mode == "three" else exact
    b = batch()
    if a.check and a.mode == "exact":
        twin, y2 = batch(), torch.zeros_like(out)
        exact(b, out)
        three(twin, y2)
        b.synchronize()
        twin.synchronize()
        assert torch.equal(out, y2) and bool(out.abs().max() > 0), "exact differs from the three-call sequence"
        twin.close()
        del y2
    times = []
    for k in range(a.warmup + a.steps):
        b.synchronize()
        t0 = time.perf_counter()
        call(b, out)
        b.synchronize()
        times.append((time.perf_counter() - t0)*1e3)
    timed = times[a.warmup:]
    print(json.dumps(dict(mode=a.mode, library=os.path.relpath(smst.LIBRARY_PATH), streams=S, channels=Cn, in_samples=n, out_samples=[int(nout.min()), int(nout.max())],
                          median_ms=round(statistics.median(timed), 3), min_ms=round(min(timed), 3), max_ms=round(max(timed), 3), steps=a.steps, warmup=a.warmup,
                          checked=bool(a.check and a.mode == "exact"), device=torch.cuda.get_device_name(0), hw_queues=os.environ["GPU_MAX_HW_QUEUES"])))
    b.close()


def frames_modes(a, lib, x, nin, nout, batch):
    """smst_batch_exact_pcm on int16 frames in device memory: unlevelled, with a fixed gain, with PROTECT; `level` runs the three in turn within
    every step, each on a batch of its own"""
    S, Cn, n, most = a.streams, a.channels, x.shape[2], int(nout.max())
    frames = (x.transpose(1, 2)*32768.0).round().clamp(-32768, 32767).to(torch.int16).contiguous()
    out = torch.zeros((S, most, Cn), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int))
    runs = {}
    assert not (a.true_peak and a.mode == "level"), "--true-peak goes with one mode"
    assert not (a.limit and a.mode not in ("protect", "normalise")), "--limit goes with --mode protect (or normalise, where the flag is inert)"
    assert not (a.resample and a.mode == "level"), "--resample goes with one mode"
    inputs = {}
    for key in (("pcm", "fixed", "protect") if a.mode == "level" else (a.mode,)) + (("loudness",) if a.loudness else ()) + (("true_peak",) if a.true_peak else ()) + (("limit",) if a.limit else ()) + (("loudness_range",) if a.loudness_range else ()) + (("resample",) if a.resample else ()):
        b = batch()
        name = a.mode if key in ("true_peak", "limit", "resample") else key
        if key == "resample":
            up, down = (int(v) for v in a.resample.split("/"))
            b.set_pcm_resample(up, down)
            up, down = b.pcm_resample(0)
            src = (n*down)//up                                                     # the shortest clip whose Nr is the plain batch's input length
            while b.resampled_length(0, src) < n:
                src += 1
            assert b.resampled_length(0, src) == n, (src, b.resampled_length(0, src), n)
            ts = torch.arange(src, device="cuda", dtype=torch.float32)*(up/(down*a.sample_rate))   # the same tones, at the clips' rate
            f = 110.0*2**(torch.arange(S*Cn, device="cuda", dtype=torch.float32).reshape(S, 1, Cn) % 37/12)
            g = torch.Generator(device="cuda").manual_seed(8)
            xs = 0.4*torch.sin(2*np.pi*f*ts.reshape(1, src, 1)) + 0.05*torch.rand((S, src, Cn), generator=g, device="cuda") - 0.025
            inputs[key] = ((xs*32768.0).round().clamp(-32768, 32767).to(torch.int16).contiguous(), np.full(S, src, np.int32))
            del xs
        if key == "true_peak":
            b.set_pcm_true_peak(True)
        if key == "limit":
            b.set_pcm_limiter_lookahead(a.limit_lookahead)
            b.set_pcm_limiter(True)
        if name == "fixed":
            b.set_pcm_level(smst.LEVEL_FIXED, 0.5)
        if name == "protect":
            b.set_pcm_level(smst.LEVEL_PROTECT, a.limit_gain if a.limit else 1.0, 32766.0/32768.0)
        if name == "normalise":
            b.set_pcm_level(smst.LEVEL_NORMALISE, 1.0, 32766.0/32768.0)
        if name in ("loudness", "loudness_range"):
            b.set_pcm_loudness(-23.0, 32766.0/32768.0, a.sample_rate)
        if name == "loudness_range":
            b.set_pcm_loudness_range(True, a.sample_rate)
        runs[key] = b

    torch.cuda.synchronize()

    def call(b, key):
        status = np.zeros(S, np.int32)
        fr, counts = inputs.get(key, (frames, nin))
        smst._check(lib, lib.smst_batch_exact_pcm(b.h, C.c_void_p(fr.data_ptr()), fr.shape[1]*Cn, Cn, ip(counts), C.c_void_p(out.data_ptr()), most*Cn, Cn, ip(nout), ip(status), smst.PCM_S16, smst.MEM_DEVICE))
        assert not status.any(), status
    times = {name: [] for name in runs}
    for k in range(a.warmup + a.steps):
        for name, b in runs.items():
            b.synchronize()
            t0 = time.perf_counter()
            call(b, name)
            b.synchronize()
            if k >= a.warmup:
                times[name].append((time.perf_counter() - t0)*1e3)
    result = dict(mode=a.mode, library=os.path.relpath(smst.LIBRARY_PATH), streams=S, channels=Cn, in_samples=n, out_samples=[int(nout.min()), int(nout.max())], steps=a.steps,
                  warmup=a.warmup, device=torch.cuda.get_device_name(0), hw_queues=os.environ["GPU_MAX_HW_QUEUES"], step_ms={})
    for name, v in times.items():
        result["step_ms"][name] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    if a.mode == "level":
        med = lambda name: result["step_ms"][name]["median"]
        result["level"] = dict(fixed_minus_pcm_ms=round(med("fixed") - med("pcm"), 3), protect_minus_fixed_ms=round(med("protect") - med("fixed"), 3),
                               peak_pass_bytes=int(S)*Cn*int(nout.sum()//S)*4)
        peaks, gains = runs["protect"].take_pcm_peaks()
        result["level"]["protect_gain_range"] = [float(gains.min()), float(gains.max())]
    if a.loudness:
        lufs, blocks, gated = runs["loudness"].take_pcm_loudness()
        result["loudness"] = dict(lufs_range=[float(lufs.min()), float(lufs.max())], gated_blocks=[int(gated.min()), int(gated.max())],
                                  image_bytes=int(S)*Cn*int(nout.sum()//S)*4)
        if a.mode in result["step_ms"]:
            result["loudness"]["minus_%s_ms" % a.mode] = round(result["step_ms"]["loudness"]["median"] - result["step_ms"][a.mode]["median"], 3)
    if a.true_peak:
        tp = runs["true_peak"].take_pcm_true_peaks()
        peaks, gains = runs["true_peak"].take_pcm_peaks()
        result["true_peak"] = dict(true_peak_range=[float(tp.min()), float(tp.max())], sample_peak_range=[float(peaks.min()), float(peaks.max())],
                                   gain_range=[float(gains.min()), float(gains.max())], image_bytes=int(S)*Cn*int(nout.sum()//S)*4,
                                   launches=smst.launch_count("clip_true_peak", lib))
        result["true_peak"]["minus_%s_ms" % a.mode] = round(result["step_ms"]["true_peak"]["median"] - result["step_ms"][a.mode]["median"], 3)
    if a.limit:
        low, count = runs["limit"].take_pcm_limiter()
        peaks, gains = runs["limit"].take_pcm_peaks()
        result["limit"] = dict(lookahead=a.limit_lookahead, min_gain_range=[float(low.min()), float(low.max())], limited_frames=[int(count.min()), int(count.max())],
                               gain_range=[float(gains.min()), float(gains.max())], image_bytes=int(S)*Cn*int(nout.sum()//S)*4,
                               launches=[smst.launch_count(k, lib) for k in ("clip_limit_need", "clip_limit_gain", "clip_out_limited")])
        result["limit"]["minus_%s_ms" % a.mode] = round(result["step_ms"]["limit"]["median"] - result["step_ms"][a.mode]["median"], 3)
    if a.resample:
        up, down = runs["resample"].pcm_resample(0)
        result["resample"] = dict(ratio="%d/%d" % (up, down), in_samples=int(inputs["resample"][1][0]), resampled=n, launches=smst.launch_count("clip_resample", lib),
                                  raw_image_bytes=int(S)*Cn*int(inputs["resample"][1][0])*4, input_image_bytes=int(S)*Cn*n*4)
        result["resample"]["minus_%s_ms" % a.mode] = round(result["step_ms"]["resample"]["median"] - result["step_ms"][a.mode]["median"], 3)
    if a.loudness_range:
        mmax, smax, lra, low, high, ns, ng = runs["loudness_range"].take_pcm_loudness_range()
        result["loudness_range"] = dict(short_term_max_range=[float(smax.min()), float(smax.max())], lra_range=[float(lra.min()), float(lra.max())],
                                        short_blocks=[int(ns.min()), int(ns.max())], range_blocks=[int(ng.min()), int(ng.max())],
                                        launches=smst.launch_count("clip_loudness_range", lib))
        for other in ("loudness", a.mode):
            if other in result["step_ms"]:
                result["loudness_range"]["minus_%s_ms" % other] = round(result["step_ms"]["loudness_range"]["median"] - result["step_ms"][other]["median"], 3)
    print(json.dumps(result))
    for b in runs.values():
        b.close()


if __name__ == "__main__":
    main()
