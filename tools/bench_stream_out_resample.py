#!/usr/bin/env python3
"""The stream-output-resample stage behind smst_batch_process_pcm (include/smst.h, "Stream output resample"), int16 frames in device memory:
a batch whose streams all carry the ratio against a plain batch of the same build that is asked, per call, for as many frames as the
resampled one's engine renders -- so the difference between the two is kPcmStreamResampleOut, the copy back and the conversion of Nd
instead of E frames.  The two batches alternate step by step; each call is timed on the host from its entry to the return of
smst_batch_synchronize.  Prints one JSON line.

  python tools/bench_stream_out_resample.py --case clip      # 256 stereo streams at 147/160, one call that delivers 10 s at 44.1 kHz per step
  python tools/bench_stream_out_resample.py --case quantum   # 4096 stereo streams at 147/160, one call of 128 delivered frames per step (the real-time pattern)

Kernel times come from a run of their own under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_stream_out_resample.py
--case ... --steps N): the kernels are kPcmStreamResampleOut and kPcmStreamResampleOutCopy, the conversions kPcmOut*."""
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

CASES = dict(clip=dict(streams=256, ratio=(147, 160), frames=441000, steps=10, warmup=3),
             quantum=dict(streams=4096, ratio=(147, 160), frames=128, steps=2000, warmup=200))
DELIVERY_RATE = 44100.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    args = ap.parse_args()
    case = CASES[args.case]
    S, Cn, nd = case["streams"], args.channels, case["frames"]
    steps, warmup = args.steps or case["steps"], args.warmup if args.warmup is not None else case["warmup"]
    up, down = case["ratio"]
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    plain, resampled = (smst.StretchBatch(S, Cn, preset="default", sample_rate=48000, device=0) for _ in range(2))
    resampled.set_pcm_stream_out_resample(up, down)
    nominal = (nd*down + up - 1)//up + 1                                      # the most frames a call renders: the engine runs at a rate of about 1
    rng = np.random.default_rng(1)
    x = torch.from_numpy(((rng.random((S, nominal, Cn), dtype=np.float32) - 0.5)*32767).astype(np.int16)).cuda()
    out = torch.zeros((S, nominal, Cn), dtype=torch.int16, device="cuda")
    times = dict(plain=[], resampled=[])
    Es = []
    launches = [smst.launch_count(k) for k in ("pcm_stream_resample_out", "pcm_stream_resample_out_copy")]
    for step in range(warmup + steps):
        E = resampled.stream_out_resample_render(0, nd)
        for name, batch, count in (("plain", plain, E), ("resampled", resampled, nd)):
            t0 = time.perf_counter()
            batch.processFrames(x, [count]*S, in_samples=[E]*S, out=out, ordered=False)
            batch.synchronize()
            if step >= warmup:
                times[name].append((time.perf_counter() - t0)*1e3)
        Es.append(E)
    assert [smst.launch_count(k) for k in ("pcm_stream_resample_out", "pcm_stream_resample_out_copy")] == [n + warmup + steps for n in launches]
    q = lambda v, p: sorted(v)[min(len(v) - 1, int(p*len(v)))]
    result = dict(case=args.case, streams=S, channels=Cn, ratio="%d/%d" % (up, down), frames_delivered=nd, E_min=min(Es), E_max=max(Es),
                  steps=steps, warmup=warmup, latency_frames=resampled.stream_out_resample_latency(0), quantum_ms=nd/DELIVERY_RATE*1e3,
                  plain_ms=dict(median=statistics.median(times["plain"]), p99=q(times["plain"], 0.99), min=min(times["plain"])),
                  resampled_ms=dict(median=statistics.median(times["resampled"]), p99=q(times["resampled"], 0.99), min=min(times["resampled"])),
                  workspace_bytes=dict(plain=plain.workspaceBytes(), resampled=resampled.workspaceBytes()))
    print(json.dumps(result))
    plain.close()
    resampled.close()


if __name__ == "__main__":
    main()
