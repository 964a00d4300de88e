#!/usr/bin/env python
"""Latency of one 200-ms tick (3,200 samples and one video slice per active stream) of a streaming session whose
streams move independently (pipeline.StreamEnhancer.push_each, DESIGN.md §3 K17 "Independent streams"), against the
lock-step push it generalises and against the alternative it replaces.  sibling of tools/stream_latency.py (same
timing: HIP events around the call, a host clock around the call and around call + synchronise, the device
synchronised between calls).

Cases, at B streams of one dtype:
  a_lock_step       StreamEnhancer(B).push: the lock-step kernels, the yardstick
  b_each_uniform    StreamEnhancer(B).push_each with the same counts for every stream: the same work through the item
                    tables (adds the packing of B tensors, one table upload, the item indirection)
  c_each_one_of_B   StreamEnhancer(B).push_each with one active stream, the others idle
  c_single_session  StreamEnhancer(1).push: what c should be close to
  d_B_sessions      B single-stream sessions pushed one after another: the alternative
The cases are timed in turn within every round (a, b, c, c1, d, a, b, ..), so drift of the machine falls on all of them
alike.  Prints one JSON line per case: median, 10th / 90th / 99th percentile of each clock; --out appends them to a file.

  python tools/stream_each_latency.py --out profiles/stream_each_latency.jsonl
"""
import argparse
import json
import os
import sys
import time


def stats(v):
    import numpy as np
    v = np.asarray(v, np.float64)
    return {k: round(float(f(v)), 4) for k, f in (("median", np.median), ("p10", lambda a: np.percentile(a, 10)),
                                                  ("p90", lambda a: np.percentile(a, 90)),
                                                  ("p99", lambda a: np.percentile(a, 99)))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--dtype", default="float32_split")
    ap.add_argument("--sample-rate", type=int, default=16000,
                    help="16000, 32000 or 48000 (25 fps: n_fft = rate / 25); with --fps 30: 24000 or 48000 (n_fft = rate / 30)")
    ap.add_argument("--fps", type=float, default=25.0, help="video frame rate: 25, or 30 (the [80, 24] x 6-frame network)")
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import avse_pkg
    avse_pkg.load()
    from avse_amd import ops
    from avse_amd.model import KerasModel
    from avse_amd.pipeline import StreamEnhancer
    if not torch.cuda.is_available():
        sys.exit("stream_each_latency: no ROCm GPU visible to torch; nothing is measured without one")

    B = args.streams
    rng = np.random.default_rng(0)
    if args.fps not in (25.0, 30.0) or args.sample_rate not in ((16000, 32000, 48000) if args.fps == 25.0 else (24000, 48000)):
        sys.exit("stream_each_latency: --fps 25 takes --sample-rate 16000, 32000 or 48000; --fps 30 takes 24000 or 48000")
    T, F = (20, 5) if args.fps == 25.0 else (24, 6)
    dw = ops.DeviceWeights(KerasModel.init(seed=0, randomize=True, audio_shape=(80, T), video_shape=(128, 128, F)), args.dtype)
    sr = args.sample_rate
    sl = sr // 5                      # samples per 200-ms slice
    sig = ops.to_device(rng.normal(0, 3000, (B, sl * 8)).round().astype(np.float32))
    video = ops.to_device(rng.integers(0, 256, (B, 1, 128, 128, F)).astype(np.float32))
    mean = ops.to_device(np.full((128, 128), 127.5, np.float32))
    std = ops.to_device(np.full((128, 128), 73.9, np.float32))
    chunks = [sig[:, sl * k:sl * k + sl].contiguous() for k in range(8)]
    rows = [[c[b] for b in range(B)] for c in chunks]                  # per-stream 1-D views of the same samples
    vrows = [video[b] for b in range(B)]
    active = B // 2 + 1
    one = [[c[b] if b == active else None for b in range(B)] for c in chunks]
    vone = [video[b] if b == active else None for b in range(B)]

    make = lambda n: StreamEnhancer(dw, n, video_frame_rate=args.fps, sample_rate=sr)
    lock, each, sparse, single = make(B), make(B), make(B), make(1)
    many = [make(1) for _ in range(B)]

    def d_tick(i):
        for b, e in enumerate(many):
            e.push(chunks[i % 8][b:b + 1], video[b:b + 1], mean, std)

    cases = [
        ("a_lock_step", lambda i: lock.push(chunks[i % 8], video, mean, std)),
        ("b_each_uniform", lambda i: each.push_each(rows[i % 8], vrows, None, mean, std)),
        ("c_each_one_of_B", lambda i: sparse.push_each(one[i % 8], vone, None, mean, std)),
        ("c_single_session", lambda i: single.push(chunks[i % 8][active:active + 1], video[active:active + 1], mean, std)),
        ("d_B_sessions", d_tick),
    ]
    times = {name: dict(event_ms=[], host_call_ms=[], host_sync_ms=[]) for name, _ in cases}
    for i in range(args.warmup + args.rounds):
        for name, fn in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn(i)
            b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= args.warmup:
                t = times[name]
                t["event_ms"].append(a.elapsed_time(b))
                t["host_call_ms"].append(1e3 * (t1 - t0))
                t["host_sync_ms"].append(1e3 * (t2 - t0))
    n_calls = args.warmup + args.rounds
    want = sl * (n_calls - 1) - 2 * (sl // T)                                # every push after the first completed its slice
    assert lock.counts["emitted"] == want and single.counts["emitted"] == want and many[-1].counts["emitted"] == want
    assert each.counts["emitted"] == want, each.counts                 # (uniform counts: the streams stayed in step)
    assert sparse.counts["emitted"][active] == want and sum(sparse.counts["samples"]) == sl * n_calls
    lines = []
    for name, _ in cases:
        lines.append(json.dumps(dict(what=name, dtype=args.dtype, sample_rate=sr, fps=args.fps, streams=B, rounds=args.rounds, warmup=args.warmup,
                                     label=args.label, **{k: stats(v) for k, v in times[name].items()})))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
