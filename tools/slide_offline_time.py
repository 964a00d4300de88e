#!/usr/bin/env python
"""Throughput of the offline sliding path (pipeline.Enhancer(stride=)) beside the only other way to a
flushed sliding session's output: ticking a session.

A fixed corpus (default 64 utterances of 3 s at 16 kHz / 25 fps: 15 slices, 75 video frames each) at stride 1, per dtype:
  offline   Enhancer(weights, stride=1, chunk=C)(signals, video): one ragged STFT, clamp + window gather, forwards over
            chunks of C windows with each chunk's video windows staged, keep, one ragged ISTFT
  session   SlidingStreamEnhancer(weights, U, stride=1, max_windows=M) fed lock-step in calls of M video frames (and their
            samples) per stream, then flushed: U M windows per call at most
Per line: wall_ms (host clock around the whole run plus a synchronise; the median of --repeats runs after one warm-up),
utterances, windows, audio seconds per wall second.  The offline line adds the stage split from HIP events (stft_ms,
windows_ms: clamp + window gather, forward_ms: the chunks' video gathers and forwards together, keep_ms, istft_ms),
video_gather_ms (every chunk's video gather timed again in a loop of its own: the part of forward_ms that is staging),
staged_video_bytes (the staging buffer: one chunk of windows) and whether its output equals the session's bit for bit.
Nothing here is gated by a test, and no ratio is fixed in advance.

  python tools/slide_offline_time.py --label "<box>, <commit>" --out profiles/slide_offline.jsonl
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--slices", type=int, default=15, help="slices per utterance (15: 3 s)")
    ap.add_argument("--dtypes", default="float32_split,bfloat16")
    ap.add_argument("--chunk", type=int, default=1024, help="windows per forward of the offline path")
    ap.add_argument("--max-windows", type=int, default=16, help="the session's max_windows, and video frames per call")
    ap.add_argument("--video", default="uint8", choices=["uint8", "float32"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import avse_pkg
    avse_pkg.load()
    from avse_amd import _lib, ops
    from avse_amd.model import KerasModel
    from avse_amd.pipeline import Enhancer, SlidingStreamEnhancer
    if not torch.cuda.is_available():
        sys.exit("slide_offline_time: no ROCm GPU visible to torch; nothing is measured without one")

    rng = np.random.default_rng(0)
    sr, hop, spf, F, stride = 16000, 160, 20, 5, 1
    q = spf // F
    U, S, M = args.utterances, args.slices, args.max_windows
    L, f = spf * hop * S, F * S
    vdt = np.uint8 if args.video == "uint8" else np.float32
    sig = ops.to_device(rng.normal(0, 3000, (U, L)).round().astype(np.float32))
    video = ops.video_to_device(rng.integers(0, 256, (U, S, 128, 128, F)).astype(vdt))
    frames = video.permute(0, 1, 4, 2, 3).reshape(U, f, 128, 128).contiguous()      # the same crops, frame by frame
    mean = ops.to_device(np.full((128, 128), 127.5, np.float32))
    std = ops.to_device(np.full((128, 128), 73.9, np.float32))
    model = KerasModel.init(seed=0, randomize=True)
    W, P = ops.slide_window_counts([S] * U, spf, F, stride)
    common = dict(sample_rate=sr, stride=stride, utterances=U, slices=S, windows=int(W.sum()), video=args.video,
                  audio_s=round(U * L / sr, 3), repeats=args.repeats, label=args.label, device=torch.cuda.get_device_name(0),
                  source_digest=_lib.source_digest())

    def wall(fn):
        fn()                                   # warm-up: scratch grows, tables load
        torch.cuda.synchronize()
        ts, out = [], None
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), out

    lines = []
    for dtype in args.dtypes.split(","):
        dw = ops.DeviceWeights(model, dtype)
        enh = Enhancer(dw, stride=stride, chunk=args.chunk)
        off_ms, off = wall(lambda: enh(sig, video, mean, std))
        stages = {}
        enh(sig, video, mean, std, timings=stages)
        flat = video.view((U * S,) + tuple(video.shape[2:]))
        stage = torch.empty((min(args.chunk, int(W.sum())),) + tuple(flat.shape[1:]), dtype=flat.dtype, device=flat.device)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for a in range(0, int(W.sum()), args.chunk):
            ops.slide_video_windows(flat, [S] * U, stride=stride, w0=a, n=min(args.chunk, int(W.sum()) - a), out=stage)
        ev[1].record()
        ev[1].synchronize()

        sess = SlidingStreamEnhancer(dw, U, stride=stride, max_windows=M, video_dtype=frames.dtype)

        def ticked():
            sess.reset()
            outs = []
            for a in range(0, f, M):
                b = min(f, a + M)
                outs.append(sess.push(sig[:, q * hop * a:q * hop * b].contiguous(), frames[:, a:b].contiguous(), mean, std))
            outs.append(sess.flush(mean, std))
            return torch.cat(outs, dim=1)
        ses_ms, ses = wall(ticked)
        same = tuple(off.shape) == tuple(ses.shape) and bool(torch.equal(off.view(torch.int32), ses.view(torch.int32)))
        r = dict(what="offline", dtype=dtype, chunk=args.chunk, wall_ms=round(off_ms, 3),
                 audio_s_per_s=round(U * L / sr / (off_ms * 1e-3), 1), **{k: round(v, 3) for k, v in stages.items()},
                 video_gather_ms=round(ev[0].elapsed_time(ev[1]), 3), staged_video_bytes=enh.staged_video_bytes,
                 equals_session_bits=same, **common)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        r = dict(what="session", dtype=dtype, max_windows=M, calls=(f + M - 1) // M + 1, wall_ms=round(ses_ms, 3),
                 audio_s_per_s=round(U * L / sr / (ses_ms * 1e-3), 1), **common)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
