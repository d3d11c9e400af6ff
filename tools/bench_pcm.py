#!/usr/bin/env python3
"""Wall time per step of the batch API fed with interleaved PCM frames, against the planar float calls (EXPERIMENTS.md, "Interleaved PCM").

Workload: 256 stereo streams, 48 kHz, presetDefault, 1.5x, 10-second steps.  Variants, alternated step by step inside every round so
that drift of the host or the device hits all of them alike:
  a  smst_batch_process, SMST_MEM_HOST, planar float        (the path before the frame calls; also runs on an older library:
                                                             SMST_LIBRARY=<libsmst_hip.so of that build> SMST_LIBRARY_ALLOW_MISSING=1 --variants a)
  b  smst_batch_process_pcm, SMST_MEM_HOST, float32 frames
  c  smst_batch_process_pcm, SMST_MEM_HOST, int16 frames
  d  smst_batch_process_pcm, SMST_MEM_DEVICE, int16 frames  (torch tensors, batch synchronised per step)
  e  smst_batch_process, SMST_MEM_DEVICE, planar float      (what d is compared with: d - e = the two conversion passes)
  f  d with TPDF dither (setPcmDither), g  d with high-passed TPDF dither       (f - d, g - d = what the dither adds to a step)
  h  smst_batch_process_pcm, SMST_MEM_DEVICE, packed int24 frames, i  h with TPDF dither, j  h with high-passed TPDF dither
  k  d with a fixed gain of 0.5 on every stream (set_pcm_level): the levelled kernel   (k - d = what the gain and the peak meter add to a step)
  l  d with a fixed gain of +12 dB and the stream limiter at -1 dBFS on every stream (set_pcm_stream_limiter): the two passes and the limited kernel
     (l - k = what the two passes and the delayed loader add to a step)
  m  l with the stream limiter's true-peak flag on every stream (set_pcm_stream_limiter_true_peak): the true-peak feed kernel in the place of
     the sample-peak one   (m - l = what the three phases of the detector add to a step)
The dithered, levelled and limited rows are not in the default set: --variants d,e,f,g,h,i,j,k,l,m.  The time of the output conversion KERNEL alone (kPcmOut<T, false> /
kPcmOut<T, true> per format) is read from a kernel trace of such a run.
A step's time is the host clock around one call that ends synchronised.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=float, default=1.5, help="time-stretch factor (output frames per input frame)")
    ap.add_argument("--steps", type=int, default=5, help="timed steps per variant")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variants", default="a,b,c,d,e")
    args = ap.parse_args()
    pkg = importlib.import_module("signalsmith-stretch_amd")
    variants = args.variants.split(",")
    S, Cn, sr = args.streams, 2, 48000
    n = int(args.seconds*sr)
    m = int(n*args.rate)
    rng = np.random.Generator(np.random.PCG64(7))
    t = np.arange(n)/sr
    base = np.stack([0.3*np.sin(2*np.pi*(110*2**(k/12))*t) for k in range(8)]).astype(np.float32)
    planar = np.empty((S, Cn, n), np.float32)
    for s in range(S):
        for c in range(Cn):
            planar[s, c] = base[(s + 3*c) % 8] + rng.uniform(-0.05, 0.05, n).astype(np.float32)
    f32 = np.ascontiguousarray(planar.transpose(0, 2, 1))
    s16 = np.clip(np.round(f32*32768.0), -32768, 32767).astype(np.int16)
    runs = {}
    if "a" in variants:
        b, out = pkg.StretchBatch(S, Cn, preset="default", sample_rate=sr), np.zeros((S, Cn, m), np.float32)
        runs["a"] = lambda b=b, out=out: b.process(planar, m, out=out)
    if "b" in variants:
        b, out = pkg.StretchBatch(S, Cn, preset="default", sample_rate=sr), np.zeros((S, m, Cn), np.float32)
        runs["b"] = lambda b=b, out=out: b.processFrames(f32, m, out=out)
    if "c" in variants:
        b, out = pkg.StretchBatch(S, Cn, preset="default", sample_rate=sr), np.zeros((S, m, Cn), np.int16)
        runs["c"] = lambda b=b, out=out: b.processFrames(s16, m, out=out)
    if any(k in variants for k in "defghijklm"):
        import torch
    if "d" in variants:
        b, x, out = pkg.StretchBatch(S, Cn, preset="default", sample_rate=sr), torch.from_numpy(s16).cuda(), torch.zeros((S, m, Cn), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        runs["d"] = lambda b=b, x=x, out=out: (b.processFrames(x, m, out=out, ordered=False), b.synchronize())
    for k, mode in (("f", pkg.DITHER_TPDF), ("g", pkg.DITHER_TPDF_HP)):
        if k in variants:
            b, x, out = pkg.StretchBatch(S, Cn, preset="default", sample_rate=sr), torch.from_numpy(s16).cuda(), torch.zeros((S, m, Cn), dtype=torch.int16, device="cuda")
            if mode != pkg.DITHER_NONE:
                b.setPcmDither(mode, seed=1)
            torch.cuda.synchronize()
            runs[k] = lambda b=b, x=x, out=out: (b.processFrames(x, m, out=out, ordered=False), b.synchronize())
    if "k" in variants:
        b, x, out = pkg.StretchBatch(S, Cn, preset="default", sample_rate=sr), torch.from_numpy(s16).cuda(), torch.zeros((S, m, Cn), dtype=torch.int16, device="cuda")
        b.set_pcm_level(pkg.LEVEL_FIXED, 0.5)
        torch.cuda.synchronize()
        runs["k"] = lambda b=b, x=x, out=out: (b.processFrames(x, m, out=out, ordered=False), b.synchronize())
    if "l" in variants:
        b, x, out = pkg.StretchBatch(S, Cn, preset="default", sample_rate=sr), torch.from_numpy(s16).cuda(), torch.zeros((S, m, Cn), dtype=torch.int16, device="cuda")
        b.set_pcm_level(pkg.LEVEL_FIXED, 10**(12/20))
        b.set_pcm_stream_limiter(True, 10**(-1/20))
        torch.cuda.synchronize()
        runs["l"] = lambda b=b, x=x, out=out: (b.processFrames(x, m, out=out, ordered=False), b.synchronize())
    if "m" in variants:
        b, x, out = pkg.StretchBatch(S, Cn, preset="default", sample_rate=sr), torch.from_numpy(s16).cuda(), torch.zeros((S, m, Cn), dtype=torch.int16, device="cuda")
        b.set_pcm_level(pkg.LEVEL_FIXED, 10**(12/20))
        b.set_pcm_stream_limiter(True, 10**(-1/20))
        b.set_pcm_stream_limiter_true_peak(True)
        torch.cuda.synchronize()
        runs["m"] = lambda b=b, x=x, out=out: (b.processFrames(x, m, out=out, ordered=False), b.synchronize())
    if any(k in variants for k in "hij"):
        codes = np.clip(np.round(f32.astype(np.float64)*8388608.0), -8388608, 8388607).astype(np.int32)
        s24 = np.stack([codes & 255, (codes >> 8) & 255, (codes >> 16) & 255], -1).astype(np.uint8)
    for k, mode in (("h", pkg.DITHER_NONE), ("i", pkg.DITHER_TPDF), ("j", pkg.DITHER_TPDF_HP)):
        if k in variants:
            b, x, out = pkg.StretchBatch(S, Cn, preset="default", sample_rate=sr), torch.from_numpy(s24).cuda(), torch.zeros((S, m, Cn, 3), dtype=torch.uint8, device="cuda")
            if mode != pkg.DITHER_NONE:
                b.setPcmDither(mode, seed=1)
            torch.cuda.synchronize()
            runs[k] = lambda b=b, x=x, out=out: (b.processFrames(x, m, out=out, ordered=False), b.synchronize())
    if "e" in variants:
        b, x, out = pkg.StretchBatch(S, Cn, preset="default", sample_rate=sr), torch.from_numpy(planar).cuda(), torch.zeros((S, Cn, m), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        runs["e"] = lambda b=b, x=x, out=out: (b.process(x, m, out=out, ordered=False), b.synchronize())
    times = {k: [] for k in runs}
    for step in range(args.warmup + args.steps):
        for k, run in runs.items():
            t0 = time.perf_counter()
            run()
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                times[k].append(dt*1e3)
    result = dict(streams=S, channels=Cn, in_frames=n, out_frames=m, steps=args.steps, warmup=args.warmup, library=pkg.library_path(), step_ms={})
    for k, v in times.items():
        v = sorted(v)
        result["step_ms"][k] = dict(median=v[len(v)//2], min=v[0], max=v[-1], msamples_per_s=S*n/(v[len(v)//2]*1e-3)/1e6)
    if "d" in times and "e" in times:
        extra = result["step_ms"]["d"]["median"] - result["step_ms"]["e"]["median"]
        moved = S*Cn*(n + m)*(2 + 4)  # each pass reads one format and writes the other
        result["conversion_passes"] = dict(extra_ms=extra, bytes=moved, gb_per_s=(moved/(extra*1e-3)/1e9 if extra > 0 else None))
    dither = {}
    for k, base in (("f", "d"), ("g", "d"), ("i", "h"), ("j", "h")):
        if k in times and base in times:
            extra = result["step_ms"][k]["median"] - result["step_ms"][base]["median"]
            dither[k] = dict(against=base, extra_ms=extra, share_of_step=extra/result["step_ms"][k]["median"])
    if dither:
        result["dither"] = dither
    if "k" in times and "d" in times:
        extra = result["step_ms"]["k"]["median"] - result["step_ms"]["d"]["median"]
        result["level"] = dict(k=dict(against="d", extra_ms=extra, share_of_step=extra/result["step_ms"]["k"]["median"]))
    for base in ("k", "d"):
        if "l" in times and base in times:
            extra = result["step_ms"]["l"]["median"] - result["step_ms"][base]["median"]
            result.setdefault("stream_limit", {})[base] = dict(against=base, extra_ms=extra, share_of_step=extra/result["step_ms"]["l"]["median"])
    if "m" in times and "l" in times:
        extra = result["step_ms"]["m"]["median"] - result["step_ms"]["l"]["median"]
        result.setdefault("stream_limit", {})["m"] = dict(against="l", extra_ms=extra, share_of_step=extra/result["step_ms"]["m"]["median"])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
