#!/usr/bin/env python3
"""The stream meter behind smst_batch_process_pcm (include/smst.h, "Stream meter"), int16 frames in device memory: a batch whose streams all
carry the setting against a plain batch of the same build that is handed the same calls -- so the difference between the two is the meter's
update.  The two batches alternate step by step; each call is timed on the host from its entry to the return of smst_batch_synchronize.
Prints one JSON line.

  python tools/bench_stream_meter.py --case clip      # 256 stereo streams, one call of 10 s (480 000 frames) per step: the chunk-scan form
  python tools/bench_stream_meter.py --case quantum   # 4096 stereo streams, one call of 128 frames per step (the real-time pattern): the short-call form
  python tools/bench_stream_meter.py --case take      # 4096 stereo streams with full histories of 36 000 sub-blocks (an hour at any rate): the cost of a take
  python tools/bench_stream_meter.py --case forms     # the update alone through the test hook, both forms, over call lengths: where they cross

The quantum case's p99 is held against the 2.67 ms budget of tools/bench_realtime.py (128 frames at 48 kHz).  Kernel times come from a run of
their own under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_stream_meter.py --case ... --steps N): the kernels are
kPcmStreamMeter*, kLoudGate and kLoudRange."""
import argparse
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

BUDGET_MS = 128/48000*1e3
CASES = dict(clip=dict(streams=256, frames=480000, steps=6, warmup=2, sub_blocks=36000),
             quantum=dict(streams=4096, frames=128, steps=2000, warmup=200, sub_blocks=36000),
             take=dict(streams=4096, frames=20000, steps=5, warmup=1, sub_blocks=36000, rate=4000.0))
q = lambda v, p: sorted(v)[min(len(v) - 1, int(p*len(v)))]
stats = lambda v: dict(median=statistics.median(v), p99=q(v, 0.99), min=min(v))


def forms(args):
    """the update alone: smst_debug_pcm_stream_meter (uploads and allocations included, the same for both forms) over `calls` calls of n
    frames, 64 stereo streams, form 1 against form 2 -> the difference per call"""
    S, Cn, calls = 64, args.channels, 16
    rows = []
    for n in (256, 512, 1024, 2048, 4096, 8192, 16384):
        rng = np.random.default_rng(2)
        image = ((rng.random((S, Cn, n*calls), dtype=np.float32) - 0.5)).astype(np.float32)
        row = dict(frames=n)
        for form in (1, 2):
            best = []
            for _ in range(args.steps or 5):
                t0 = time.perf_counter()
                smst.debug_pcm_stream_meter([[n]*S]*calls, Cn, image, Cn*n*calls, n*calls, [48000.0]*S, 64, form=form)
                best.append((time.perf_counter() - t0)*1e3)
            row["form%d_ms" % form] = min(best)
        row["scan_minus_short_ms_per_call"] = (row["form2_ms"] - row["form1_ms"])/calls
        rows.append(row)
    print(json.dumps(dict(case="forms", streams=S, channels=Cn, calls=calls, rows=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES) + ["forms"], required=True)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--sub-blocks", type=int, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    if args.case == "forms":
        return forms(args)
    case = CASES[args.case]
    S, Cn, n = case["streams"], args.channels, case["frames"]
    steps, warmup = args.steps or case["steps"], args.warmup if args.warmup is not None else case["warmup"]
    metered = smst.StretchBatch(S, Cn, preset="default", sample_rate=48000, device=0)
    plain = smst.StretchBatch(S, Cn, preset="default", sample_rate=48000, device=0) if args.case != "take" else None
    sub_blocks, rate = args.sub_blocks or case["sub_blocks"], case.get("rate", 48000.0)
    metered.set_pcm_stream_meter(True, rate, sub_blocks)
    rng = np.random.default_rng(1)
    x = torch.from_numpy(((rng.random((S, n, Cn), dtype=np.float32) - 0.5)*32767).astype(np.int16)).cuda()
    out = torch.zeros((S, n, Cn), dtype=torch.int16, device="cuda")
    result = dict(case=args.case, streams=S, channels=Cn, frames=n, steps=steps, warmup=warmup, sub_blocks=sub_blocks, rate=rate,
                  workspace_bytes=dict(plain=plain.workspaceBytes() if plain else None, metered=metered.workspaceBytes()))
    if args.case == "take":
        # fill the histories: the cost of a take is that of the gates and the selection over every sub-block, so the meter is fed until it is
        # full.  It is told a rate of 4 kHz (h = 400, the K-weighting still stable): 36 000 sub-blocks are then 720 calls of 20 000 frames
        h = int(rate/10 + 0.5)
        calls = -(-sub_blocks*h//n)
        for k in range(calls):
            metered.processFrames(x, [n]*S, out=out, ordered=False)
            if k % 40 == 0:
                metered.synchronize()
                print("filled %d of %d calls" % (k + 1, calls), file=sys.stderr, flush=True)
        metered.synchronize()
        assert metered.pcm_stream_meter_frames(0)[1] == sub_blocks*h
        takes = []
        for step in range(warmup + steps):
            t0 = time.perf_counter()
            reading = metered.take_pcm_stream_meter()
            if step >= warmup:
                takes.append((time.perf_counter() - t0)*1e3)
        result.update(take_ms=stats(takes), range_blocks=int(reading["range_blocks"][0]), lufs=float(reading["lufs"][0]))
        print(json.dumps(result))
        return
    times = dict(plain=[], metered=[])
    launches = smst.launch_count("pcm_stream_meter")
    for step in range(warmup + steps):
        for name, batch in (("plain", plain), ("metered", metered)):
            t0 = time.perf_counter()
            batch.processFrames(x, [n]*S, out=out, ordered=False)
            batch.synchronize()
            if step >= warmup:
                times[name].append((time.perf_counter() - t0)*1e3)
    assert smst.launch_count("pcm_stream_meter") == launches + warmup + steps
    t0 = time.perf_counter()
    reading = metered.take_pcm_stream_meter()
    result.update(plain_ms=stats(times["plain"]), metered_ms=stats(times["metered"]), take_ms=(time.perf_counter() - t0)*1e3,
                  scan_launches=smst.launch_count("pcm_stream_meter_scan"), metered_frames=metered.pcm_stream_meter_frames(0)[1], lufs=float(reading["lufs"][0]))
    if args.case == "quantum":
        result.update(budget_ms=BUDGET_MS, within_budget=result["metered_ms"]["p99"] < BUDGET_MS)
    print(json.dumps(result))
    plain.close()
    metered.close()


if __name__ == "__main__":
    main()
