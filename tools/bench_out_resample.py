#!/usr/bin/env python3
"""The output-resample stage of smst_batch_exact_pcm (include/smst.h, "Output resample"), int16 frames in device memory: one exact call of
256 stereo 10-s clips in a 48 kHz batch, three ways --

  out      every stream delivered at 44.1 kHz (output ratio 147/160): 480000 frames in, 441000 delivered, E = 479999 rendered
  plain    the same call without the setting: 480000 frames in, 480000 out
  inverse  the same engine work with only the INPUT setting at the inverse ratio 160/147: 441000 frames in, 480000 out -- its
           kClipResample forms 480000 frames per clip from 441000, the like-for-like kernel of kClipResampleOut's 441000 from 479999

The three batches alternate step by step; each call is timed with HIP events around it on the caller's stream.  Prints one JSON line; the
new stage's share is (out - plain)/out.  Kernel times come from a run of their own under a kernel trace."""
import argparse
import importlib
import json
import os
import statistics
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # (INTEGRATION.md "Hardware queues"; before the HIP runtime starts)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

smst = importlib.import_module("signalsmith-stretch_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    S, Cn = args.streams, args.channels
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    at_batch = int(round(args.seconds*48000))
    at_delivery = (at_batch*147 + 159)//160                                   # the clip's frames at 44.1 kHz
    rendered = ((at_delivery - 1)*160)//147 + 1                               # E of "Output resample": 479999 for 441000 delivered frames
    batches = {name: smst.StretchBatch(S, Cn, preset="default", sample_rate=48000, device=0) for name in ("out", "plain", "inverse")}
    batches["out"].set_pcm_out_resample(147, 160)
    batches["inverse"].set_pcm_resample(160, 147)
    assert batches["out"].out_render_length(0, at_delivery) == rendered and batches["inverse"].resampled_length(0, at_delivery) == at_batch
    shapes = dict(out=(at_batch, at_delivery), plain=(at_batch, at_batch), inverse=(at_delivery, at_batch))   # (frames in, frames out)
    rng = np.random.default_rng(1)
    x = torch.from_numpy(((rng.random((S, at_batch, Cn), dtype=np.float32) - 0.5)*32767).astype(np.int16)).cuda()
    out = torch.zeros((S, at_batch, Cn), dtype=torch.int16, device="cuda")
    times = {name: [] for name in batches}
    counters = ("clip_resample_out", "clip_resample")
    before = [smst.launch_count(k) for k in counters]
    for step in range(args.warmup + args.steps):
        for name, batch in batches.items():
            n_in, n_out = shapes[name]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            _, ok = batch.exactFrames(x, [n_out]*S, in_samples=[n_in]*S, out=out)
            t1.record()
            t1.synchronize()
            assert ok.all()
            if step >= args.warmup:
                times[name].append(t0.elapsed_time(t1))
    assert [smst.launch_count(k) - n for k, n in zip(counters, before)] == [args.warmup + args.steps]*2
    med = {name: statistics.median(v) for name, v in times.items()}
    result = dict(streams=S, channels=Cn, seconds=args.seconds, frames=shapes, rendered=rendered, steps=args.steps, warmup=args.warmup,
                  ms={name: dict(median=med[name], min=min(v), max=max(v)) for name, v in times.items()},
                  out_stage_ms=med["out"] - med["plain"], out_stage_share=(med["out"] - med["plain"])/med["out"],
                  inverse_stage_ms=med["inverse"] - med["plain"],
                  workspace_bytes={name: b.workspaceBytes() for name, b in batches.items()})
    print(json.dumps(result))
    for b in batches.values():
        b.close()


if __name__ == "__main__":
    main()
