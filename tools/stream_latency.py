#!/usr/bin/env python
"""Latency of one slice-sized push of a streaming session (pipeline.StreamEnhancer) and of its
yardstick, the closest thing the whole-utterance path can do per 200-ms tick: pipeline.Enhancer on U = B utterances of
S = 1 slice (one STFT, one forward of B clips, one ISTFT).

Per (dtype, B): `--pushes` timed calls after `--warmup` untimed ones, each a 200-ms push (3,200 samples at 16 kHz; with
--sample-rate 32000 / 48000: 6,400 / 9,600) with its video slice (every push after the first completes one slice per
stream).  Per call:
  event_ms      HIP events recorded on the stream before and after the call: the device-side time of the tick, launch
                gaps included
  host_call_ms  host clock around the call alone (the enqueue; Enhancer's float32_split path waits for its range guard
                inside the call, the stream's pushes never wait)
  host_sync_ms  host clock around the call and a synchronise after it
The device is synchronised between calls, so no call queues behind the one before.  Prints one JSON line per case with
the median and the 99th percentile of each; --out appends them to a file.
--input-rate R adds the case stream_push_input_rate: the same tick through StreamEnhancer(input_rate=R), i.e. a push of
R / 5 samples (8,820 at 44.1 kHz) through resampler in -> session -> resampler out, beside the plain push of the same run.

  python tools/stream_latency.py --out profiles/stream_latency.jsonl
  python tools/stream_latency.py --sample-rate 48000 --streams 1,64                        # the 3-phase kernels
  python tools/stream_latency.py --fps 30 --sample-rate 24000 --streams 1,64               # 30-fps video: the 800-point kernels
  python tools/stream_latency.py --input-rate 44100 --streams 1,64                          # + resampler in and out (K18)
  python tools/stream_latency.py --input-fps 30 --streams 1,64                              # + retimer in front (K19)
  python tools/stream_latency.py --yardstick-only --root <checkout of the parent commit>   # the same script on the parent
"""
import argparse
import json
import os
import sys
import time


def stats(v):
    import numpy as np
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "p99": round(float(np.percentile(v, 99)), 4)}


def timed(fn, n_warm, n_timed, torch):
    ev, call, sync = [], [], []
    for i in range(n_warm + n_timed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn(i)
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= n_warm:
            ev.append(a.elapsed_time(b))
            call.append(1e3 * (t1 - t0))
            sync.append(1e3 * (t2 - t0))
    return {"event_ms": stats(ev), "host_call_ms": stats(call), "host_sync_ms": stats(sync)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", default="1,16,64")
    ap.add_argument("--dtypes", default="float32_split,bfloat16")
    ap.add_argument("--sample-rate", type=int, default=16000,
                    help="16000, 32000 or 48000 (25 fps: n_fft = rate / 25); with --fps 30: 24000 or 48000 (n_fft = rate / 30)")
    ap.add_argument("--fps", type=float, default=25.0, help="video frame rate: 25, or 30 (the [80, 24] x 6-frame network)")
    ap.add_argument("--input-rate", type=int, default=0,
                    help="also time the push through StreamEnhancer(input_rate=R): R / 5 samples per tick")
    ap.add_argument("--input-fps", type=int, default=0,
                    help="also time the push through StreamEnhancer(input_fps=R): R / 5 camera frames per tick (R a "
                         "multiple of 5, e.g. 30)")
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout to import the package from (default: this one)")
    ap.add_argument("--yardstick-only", action="store_true", help="time Enhancer alone (a tree without streaming)")
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
    from avse_amd.pipeline import Enhancer
    if not torch.cuda.is_available():
        sys.exit("stream_latency: no ROCm GPU visible to torch; nothing is measured without one")

    rng = np.random.default_rng(0)
    if args.fps not in (25.0, 30.0) or args.sample_rate not in ((16000, 32000, 48000) if args.fps == 25.0 else (24000, 48000)):
        sys.exit("stream_latency: --fps 25 takes --sample-rate 16000, 32000 or 48000; --fps 30 takes 24000 or 48000")
    T, F = (20, 5) if args.fps == 25.0 else (24, 6)
    model = KerasModel.init(seed=0, randomize=True) if args.fps == 25.0 else \
        KerasModel.init(seed=0, randomize=True, audio_shape=(80, T), video_shape=(128, 128, F))
    n_calls = args.warmup + args.pushes
    sr = args.sample_rate
    sl = sr // 5                      # samples per 200-ms slice
    rate = {} if sr == 16000 else {"sample_rate": sr}      # (a parent tree's Enhancer defaults to 16 kHz as well)
    if args.fps != 25.0:
        rate["video_frame_rate"] = args.fps
    lines = []
    for dtype in args.dtypes.split(","):
        dw = ops.DeviceWeights(model, dtype)
        for B in (int(b) for b in args.streams.split(",")):
            sig = ops.to_device(rng.normal(0, 3000, (B, sl * 8)).round().astype(np.float32))
            video = ops.to_device(rng.integers(0, 256, (B, 1, 128, 128, F)).astype(np.float32))
            mean = ops.to_device(np.full((128, 128), 127.5, np.float32))
            std = ops.to_device(np.full((128, 128), 73.9, np.float32))
            chunks = [sig[:, sl * k:sl * k + sl].contiguous() for k in range(8)]
            cases = []
            if not args.yardstick_only:
                from avse_amd.pipeline import StreamEnhancer
                enh = StreamEnhancer(dw, B, **rate)
                cases.append(("stream_push", lambda i, enh=enh: enh.push(chunks[i % 8], video, mean, std)))
                if args.input_rate:
                    R = args.input_rate
                    sig_r = ops.to_device(rng.normal(0, 3000, (B, (R // 5) * 8)).round().astype(np.float32))
                    chunks_r = [sig_r[:, (R // 5) * k:(R // 5) * (k + 1)].contiguous() for k in range(8)]
                    enh_r = StreamEnhancer(dw, B, input_rate=R, **rate)
                    cases.append(("stream_push_input_rate",
                                  lambda i, enh_r=enh_r, chunks_r=chunks_r: enh_r.push(chunks_r[i % 8], video, mean, std)))
                if args.input_fps:
                    nf = args.input_fps // 5
                    cam = ops.to_device(rng.integers(0, 256, (B, nf, 128, 128)).astype(np.float32))
                    enh_f = StreamEnhancer(dw, B, input_fps=args.input_fps, **rate)
                    cases.append(("stream_push_input_fps", lambda i, enh_f=enh_f, cam=cam: enh_f.push(chunks[i % 8], cam, mean, std)))
            off = Enhancer(dw, **rate)
            cases.append(("enhancer_1_slice", lambda i, off=off: off(chunks[i % 8], video, mean, std)))
            for name, fn in cases:
                r = dict(what=name, dtype=dtype, sample_rate=sr, fps=args.fps, streams=B, pushes=args.pushes, warmup=args.warmup, label=args.label,
                         **timed(fn, args.warmup, args.pushes, torch))
                if name == "stream_push":
                    r["emitted_samples"] = enh.counts["emitted"]
                    assert r["emitted_samples"] == sl * (n_calls - 1) - 2 * (sl // T), r   # every push completed its slice
                if name == "stream_push_input_rate":
                    r["input_rate"] = args.input_rate
                    r["returned_samples"] = enh_r.counts["returned"]
                    assert enh_r.counts["slices"] == n_calls - 1, r                         # every push completed its slice
                if name == "stream_push_input_fps":
                    r["input_fps"] = args.input_fps
                    r["video_frames"] = enh_f.counts["video_frames"]
                    assert enh_f.counts["slices"] == n_calls - 1, r                         # every push completed its slice
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
