#!/usr/bin/env python
"""Latency of one tick of a sliding streaming session (pipeline.SlidingStreamEnhancer) beside its
yardstick, a slice-sized push of a plain session (pipeline.StreamEnhancer, K17).

Per (dtype, B):
  slide_tick    one video frame per stream at stride 1: q * hop samples (640 at 16 kHz) and one [128, 128] crop; every
                tick after the first F - 1 completes one window per stream (one forward of B clips)
  stream_push   one slice per stream through StreamEnhancer: spf * hop samples (3,200) and one [128, 128, F] slice; run it
                on the parent commit with --yardstick-only --root <checkout> (a tree without the sliding session)
  slide_stride_F  a slice-sized push of the sliding session at stride F: the same work as stream_push through K21's kernels
Per call, as tools/stream_latency.py: event_ms (HIP events around the call), host_call_ms (host clock around the enqueue),
host_sync_ms (call plus a synchronise); median and 99th percentile of `--pushes` calls after `--warmup`.  Every line also
gives device_ms_per_s, the event time per second of audio: the price of stride 1 against stride F is the ratio of the
slide_tick and slide_stride_F lines.  Nothing here is gated by a test.

  python tools/slide_latency.py --out profiles/slide_latency.jsonl
  python tools/slide_latency.py --yardstick-only --root <checkout of the parent commit> --label parent
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stream_latency import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", default="1,16,64")
    ap.add_argument("--dtypes", default="float32,float32_split,bfloat16")
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout to import the package from (default: this one)")
    ap.add_argument("--yardstick-only", action="store_true", help="time StreamEnhancer alone (a tree without K21)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    import avse_pkg
    avse_pkg.load()
    from avse_amd import ops
    from avse_amd.model import KerasModel
    from avse_amd.pipeline import StreamEnhancer
    if not torch.cuda.is_available():
        sys.exit("slide_latency: no ROCm GPU visible to torch; nothing is measured without one")

    rng = np.random.default_rng(0)
    sr, hop, spf, F = 16000, 160, 20, 5
    q = spf // F
    tick, sl = q * hop, spf * hop
    model = KerasModel.init(seed=0, randomize=True)
    n_calls = args.warmup + args.pushes
    lines = []
    for dtype in args.dtypes.split(","):
        dw = ops.DeviceWeights(model, dtype)
        for B in (int(b) for b in args.streams.split(",")):
            sig = ops.to_device(rng.normal(0, 3000, (B, sl * 8)).round().astype(np.float32))
            frames = ops.to_device(rng.integers(0, 256, (B, F, 128, 128)).astype(np.float32))
            video = frames.permute(0, 2, 3, 1).contiguous()[:, None]           # [B, 1, 128, 128, F]
            mean = ops.to_device(np.full((128, 128), 127.5, np.float32))
            std = ops.to_device(np.full((128, 128), 73.9, np.float32))
            ticks = [sig[:, tick * k:tick * k + tick].contiguous() for k in range(8 * F)]
            chunks = [sig[:, sl * k:sl * k + sl].contiguous() for k in range(8)]
            crops = [frames[:, i:i + 1].contiguous() for i in range(F)]
            cases = []
            plain = StreamEnhancer(dw, B)
            cases.append(("stream_push", sl, plain, lambda i, e=plain: e.push(chunks[i % 8], video, mean, std)))
            if not args.yardstick_only:
                from avse_amd.pipeline import SlidingStreamEnhancer
                s1, sF = SlidingStreamEnhancer(dw, B, stride=1), SlidingStreamEnhancer(dw, B, stride=F)
                cases.append(("slide_tick", tick, s1, lambda i, e=s1: e.push(ticks[i % (8 * F)], crops[i % F], mean, std)))
                cases.append(("slide_stride_F", sl, sF, lambda i, e=sF: e.push(chunks[i % 8], frames, mean, std)))
            for name, n_samples, enh, fn in cases:
                r = dict(what=name, dtype=dtype, sample_rate=sr, streams=B, samples_per_call=n_samples, pushes=args.pushes,
                         warmup=args.warmup, label=args.label, **timed(fn, args.warmup, args.pushes, torch))
                r["device_ms_per_s"] = round(r["event_ms"]["median"] * sr / n_samples, 4)
                c = enh.counts
                done = c["slices"] if name == "stream_push" else c["windows"]
                # every call after the first (slice-sized) / the first F (ticks) completed its window
                assert done == (n_calls - 1 if name != "slide_tick" else n_calls - F), (r, c)
                r["latency_samples"] = sl + 320 + hop if name != "slide_tick" else enh.latency_samples
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
