"""What the evaluate stage costs: ops.eval_pairs on 667 pairs of 47,840 samples (BASELINE
configs[4]'s utterance count, the ISTFT's output length for 15 slices) between HIP events, 20 calls after 3 warm-ups,
beside the float64 numpy reference tests/eval_ref.py on the same pairs on the host.
    python tools/eval_time.py [--pairs 667] [--samples 47840] [--reps 20] [--host-pairs 667] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import avse_pkg  # noqa: E402

avse_pkg.load()
from avse_amd import _lib, ops  # noqa: E402
import eval_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=667)
    ap.add_argument("--samples", type=int, default=47840)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-pairs", type=int, default=667, help="pairs the host reference is timed on (scaled up)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_time.py measures on the GPU: none visible")
    dev = torch.device("cuda", 0)
    U, n = a.pairs, a.samples
    base = [eval_ref.speech_like(1000 + k, n, 16000, snr_db=(0.0, 5.0, 10.0)[k % 3]) for k in range(min(U, 24))]
    rng = np.random.default_rng(0)
    ref, deg = [], []
    for u in range(U):          # 24 generated pairs, each reused with fresh rounded noise so no two pairs are equal
        s, y = base[u % len(base)]
        ref.append(s)
        deg.append(y if u < len(base) else np.round(y + rng.normal(0.0, 30.0, n)).astype(np.float32))
    off = np.arange(U + 1, dtype=np.int64) * n
    rp = torch.from_numpy(np.concatenate(ref)).to(dev)
    dp = torch.from_numpy(np.concatenate(deg)).to(dev)

    def call():
        return ops.eval_pairs((rp, off), dp, 16000)

    for _ in range(a.warmup):
        out = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    got = out.cpu().numpy()

    hp = max(1, min(U, a.host_pairs))
    t0 = time.perf_counter()
    want = eval_ref.eval_pairs(ref[:hp], deg[:hp], 16000)
    host_s = time.perf_counter() - t0
    diff = np.abs(got[:hp] - want)
    res = {"device": torch.cuda.get_device_name(0), "source_digest": _lib.source_digest(), "pairs": U, "samples": n,
           "sample_rate": 16000, "reps": a.reps, "warmup": a.warmup,
           "device_ms_events_median": float(np.median(times)), "device_ms_events_min": float(np.min(times)),
           "device_ms_events_max": float(np.max(times)),
           "input_bytes": int(2 * 4 * U * n),
           "includes": "offset upload and output allocation of ops.eval_pairs (packed inputs already on the device)",
           "host_reference_pairs": hp, "host_reference_s": host_s,
           "host_ms_per_pair": host_s * 1e3 / hp,
           "speedup_vs_host_reference": host_s * U / hp * 1e3 / float(np.median(times)),
           "kept_equal": bool(np.array_equal(got[:hp, 4], want[:, 4])),
           "max_abs_diff_db": float(diff[:, :3].max()), "max_abs_diff_stoi": float(diff[:, 3].max()),
           "stoi_range": [float(got[:, 3].min()), float(got[:, 3].max())]}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fd:
            json.dump(res, fd, indent=1)


if __name__ == "__main__":
    main()
