#!/usr/bin/env python3
"""Latency of the real-time calling pattern: every render quantum (128 frames at 48 kHz =
2.67 ms) each stream gets process(128 in, 128 out), device-resident buffers, one synchronisation per quantum.
Prints one JSON object: per batch size the median / p99 time per quantum and how many streams that sustains in real time.
This pattern is bound by kernel launches and the per-call host scheduling, not by the kernels.
--frames=s16|f32 runs the same pattern through processFrames on interleaved frames in device memory; --gain=dB gives every stream a fixed
gain and --stream-limit=dBFS turns the stream limiter on at that ceiling (include/smst.h, "Stream limiter"; both need --frames);
--stream-limit-true-peak gives that limiter its true-peak detector: the ceiling is then one in dBTP, met 6 frames later."""
import argparse, importlib, json, os, sys, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # the engine's pipeline streams get hardware queues of their own; before the HIP runtime starts
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quantum", type=int, default=128)
    ap.add_argument("--quanta", type=int, default=600)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 64, 256, 1024, 4096])
    ap.add_argument("--stretch", type=float, default=1.0)
    ap.add_argument("--preset", default="default", choices=["default", "cheaper"], help="cheaper = split computation, the preset real-time hosts use (signalsmith-stretch.h:66-68)")
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--frames", default=None, choices=["s16", "f32"], help="interleaved frames through processFrames instead of planar float32")
    ap.add_argument("--gain", type=float, default=None, help="dB: a fixed gain on every stream's frame output (needs --frames)")
    ap.add_argument("--stream-limit", type=float, default=None, help="dBFS: the stream limiter's ceiling (needs --frames)")
    ap.add_argument("--stream-limit-true-peak", action="store_true", help="the stream limiter's true-peak flag (needs --stream-limit)")
    ap.add_argument("--lookahead", type=int, default=None, help="the limiter's lookahead in frames (default: the library's, 72)")
    args = ap.parse_args()
    if (args.gain is not None or args.stream_limit is not None) and not args.frames:
        ap.error("--gain and --stream-limit act on the frame output: give --frames=s16 or --frames=f32")
    if args.stream_limit_true_peak and args.stream_limit is None:
        ap.error("--stream-limit-true-peak is a flag of the stream limiter: give --stream-limit=dBFS")
    import torch
    pkg = importlib.import_module("signalsmith-stretch_amd")
    sr, C, Q = 48000, args.channels, args.quantum
    n_in = int(round(Q/args.stretch))
    rows = []
    for S in args.streams:
        b = pkg.StretchBatch(S, C, preset=args.preset, sample_rate=sr)
        t = torch.arange(n_in*(args.quanta + 50), device="cuda", dtype=torch.float32)/sr
        x = (0.4*torch.sin(2*torch.pi*220.0*t)).expand(S, C, -1).contiguous()
        y = torch.empty((S, C, Q), dtype=torch.float32, device="cuda")
        call = b.process
        if args.frames:
            x = x.transpose(1, 2)
            x = (x*32767.0).round().to(torch.int16).contiguous() if args.frames == "s16" else x.contiguous()
            y = torch.empty((S, Q, C), dtype=x.dtype, device="cuda")
            call = b.processFrames
            if args.lookahead is not None:
                b.set_pcm_limiter_lookahead(args.lookahead)
            if args.gain is not None:
                b.set_pcm_level(pkg.LEVEL_FIXED, 10**(args.gain/20))
            if args.stream_limit is not None:
                b.set_pcm_stream_limiter(True, 10**(args.stream_limit/20))
            if args.stream_limit_true_peak:
                b.set_pcm_stream_limiter_true_peak(True)
        times = []
        for q in range(args.quanta + 50):
            xin = x[:, q*n_in:(q + 1)*n_in] if args.frames else x[:, :, q*n_in:(q + 1)*n_in]
            t0 = time.perf_counter()
            call(xin, Q, out=y, ordered=False)  # inputs complete, the batch is synchronised right below
            b.synchronize()
            if q >= 50:
                times.append(time.perf_counter() - t0)
        limited = b.take_pcm_stream_limiter() if args.stream_limit is not None else None
        b.close()
        times.sort()
        med, p99 = times[len(times)//2], times[int(len(times)*0.99)]
        budget = Q/sr
        rows.append({"streams": S, "median_ms": round(med*1e3, 4), "p99_ms": round(p99*1e3, 4), "mean_ms": round(sum(times)/len(times)*1e3, 4),
                     "realtime_budget_ms": round(budget*1e3, 4), "realtime_headroom_x": round(budget/p99, 2),
                     "Msamples_per_s": round(S*C*(n_in + Q)/(sum(times)/len(times))/1e6, 2)})
        if limited is not None:
            rows[-1].update(limited_frames=int(limited[1].sum()), min_gain=round(float(limited[0].min()), 6))
    what = "processFrames %s" % args.frames if args.frames else "process"
    out = {"pattern": "%s(%d, %d) per quantum, %d ch 48 kHz preset %s, device-resident, 1 sync per quantum" % (what, n_in, Q, C, args.preset),
           "stretch": args.stretch, "quanta_timed": args.quanta, "rows": rows}
    if args.frames:
        out.update(frames=args.frames, gain_db=args.gain, stream_limit_dbfs=args.stream_limit, stream_limit_true_peak=args.stream_limit_true_peak)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
