"""What avse_eval_pairs_ext costs, on tools/eval_time.py's workload (667 pairs, HIP events, 20 calls
after 3 warm-ups): ops.eval_pairs and ops.eval_pairs_ext at 16 kHz on pairs of 47,840 samples, and ops.eval_pairs_ext
with any_rate at 44.1 kHz on the same pair count and duration (131,859 samples each).
    python tools/eval_ext_time.py [--pairs 667] [--reps 20] [--only default16|ext16|ext44] [--out FILE.json]
--only runs one workload (for a kernel trace of its own)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import avse_pkg  # noqa: E402

avse_pkg.load()
from avse_amd import _lib, ops  # noqa: E402
import eval_ref  # noqa: E402


def packed(U, n, sr, dev):
    """eval_time.py's pairs: 24 generated ones, each reused with fresh rounded noise so no two pairs are equal."""
    base = [eval_ref.speech_like(1000 + k, n, sr, snr_db=(0.0, 5.0, 10.0)[k % 3]) for k in range(min(U, 24))]
    rng = np.random.default_rng(0)
    ref, deg = [], []
    for u in range(U):
        s, y = base[u % len(base)]
        ref.append(s)
        deg.append(y if u < len(base) else np.round(y + rng.normal(0.0, 30.0, n)).astype(np.float32))
    off = np.arange(U + 1, dtype=np.int64) * n
    return torch.from_numpy(np.concatenate(ref)).to(dev), torch.from_numpy(np.concatenate(deg)).to(dev), off


def timed(call, warmup, reps):
    for _ in range(warmup):
        out = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return out, {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_max": float(np.max(times))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=667)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("default16", "ext16", "ext44"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_ext_time.py measures on the GPU: none visible")
    dev = torch.device("cuda", 0)
    U = a.pairs
    res = {"device": torch.cuda.get_device_name(0), "source_digest": _lib.source_digest(), "pairs": U, "reps": a.reps,
           "warmup": a.warmup, "timing": "HIP events around the ops call (offset upload and output allocation included)"}
    want = (a.only,) if a.only else ("default16", "ext16", "ext44")
    if "default16" in want or "ext16" in want:
        rp, dp, off = packed(U, 47840, 16000, dev)
        if "default16" in want:
            base, res["eval_pairs_16000"] = timed(lambda: ops.eval_pairs((rp, off), dp, 16000), a.warmup, a.reps)
            res["eval_pairs_16000"]["samples"] = 47840
        if "ext16" in want:
            ext, res["eval_pairs_ext_16000"] = timed(lambda: ops.eval_pairs_ext((rp, off), dp, 16000), a.warmup, a.reps)
            res["eval_pairs_ext_16000"]["samples"] = 47840
            res["eval_pairs_ext_16000"]["estoi_range"] = [float(ext[:, 5].min()), float(ext[:, 5].max())]
        if "default16" in want and "ext16" in want:
            res["slots_0_to_4_same_bits"] = bool(torch.equal(ext[:, :5].contiguous().view(torch.int64),
                                                             base.view(torch.int64)))
        del rp, dp
    if "ext44" in want:
        rp, dp, off = packed(U, 131859, 44100, dev)
        ext, res["eval_pairs_ext_44100_any_rate"] = timed(lambda: ops.eval_pairs_ext((rp, off), dp, 44100), a.warmup,
                                                          a.reps)
        r = res["eval_pairs_ext_44100_any_rate"]
        r["samples"] = 131859
        r["stoi_range"] = [float(ext[:, 3].min()), float(ext[:, 3].max())]
        r["estoi_range"] = [float(ext[:, 5].min()), float(ext[:, 5].max())]
        hp = 4                       # the float64 reference on the first pairs
        import eval_ext_ref
        host = eval_ext_ref.eval_pairs_ext([rp[off[k]:off[k + 1]].cpu().numpy() for k in range(hp)],
                                           [dp[off[k]:off[k + 1]].cpu().numpy() for k in range(hp)], 44100)
        diff = np.abs(ext[:hp].cpu().numpy() - host)
        r["reference_pairs"] = hp
        r["kept_equal"] = bool(np.array_equal(ext[:hp, 4].cpu().numpy(), host[:, 4]))
        r["max_abs_diff_db"], r["max_abs_diff_stoi"], r["max_abs_diff_estoi"] = \
            float(diff[:, :3].max()), float(diff[:, 3].max()), float(diff[:, 5].max())
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fd:
            json.dump(res, fd, indent=1)


if __name__ == "__main__":
    main()
