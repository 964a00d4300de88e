"""What uint8 video costs and saves in time (DESIGN.md §3 "uint8 video"), one box, batch B, split dtype.  Every arm
alternates its two sides round by round after a warm-up and reports medians with the min-to-max spread.
  (a) bench.py, unchanged, run as a child process in a checkout of the parent commit (--parent-root, its library built)
      and in this tree, alternated --rounds times: the float path's ms_per_step, which is the same code in both;
  (b) ops.forward_profile with uint8 and with float32 video: the v_conv1 stage and the sum of all stages (HIP events);
  (c) wall time per step including the upload of the video from pinned host memory (copy, forward, synchronise), for
      both dtypes; the bytes uploaded per step beside it;
  (d) the normaliser fit (ops.video_stats) on [--slices, 128, 128, 5] in both dtypes (HIP events, bytes read / time).
    python tools/video_u8_time.py [--parent-root DIR] [--batch 512] [--rounds 3] [--reps 30] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(xs):
    xs = [float(x) for x in xs]
    return {"median": float(np.median(xs)), "min": min(xs), "max": max(xs), "n": len(xs)}


def bench_once(root, steps, warmup, batch):
    """One plain bench.py run in `root` (a fresh child process) -> its JSON result line."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--batch", str(batch)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"bench.py failed in {root}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def arm_a(a):
    if not a.parent_root:
        return {"measured": False, "why": "no --parent-root given"}
    sides = {"parent": os.path.abspath(a.parent_root), "this": ROOT}
    ms = {k: [] for k in sides}
    bench_once(sides["this"], a.steps, a.warmup, a.batch)          # warm-up: code objects, file caches
    for _ in range(a.rounds):
        for k, root in sides.items():
            ms[k].append(bench_once(root, a.steps, a.warmup, a.batch)["ms_per_step"])
            print(f"bench {k}: {ms[k][-1]} ms/step", flush=True)
    out = {"measured": True, "steps": a.steps, "warmup": a.warmup, "ms_per_step": {k: spread(v) for k, v in ms.items()},
           "runs": ms}
    lo = min(ms["parent"] + ms["this"]), max(ms["parent"] + ms["this"])
    out["this_median_within_parent_min_max"] = bool(min(ms["parent"]) <= out["ms_per_step"]["this"]["median"]
                                                    <= max(ms["parent"]))
    out["all_runs_min_max"] = list(lo)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit with libavse.so built (arm a)")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30, help="timed steps per side and round (arms b, c)")
    ap.add_argument("--steps", type=int, default=100, help="bench.py --steps (arm a)")
    ap.add_argument("--warmup", type=int, default=10, help="bench.py --warmup (arm a)")
    ap.add_argument("--slices", type=int, default=4096, help="slices of the normaliser-fit set (arm d)")
    ap.add_argument("--dtype", default="float32_split")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("video_u8_time.py measures on the GPU: none visible")
    res = {"batch": a.batch, "dtype": a.dtype, "rounds": a.rounds, "reps": a.reps}
    res["bench_float_path"] = arm_a(a)          # before this process opens the GPU: the children have it alone
    res["device"] = torch.cuda.get_device_name(0)

    sys.path.insert(0, ROOT)
    import avse_pkg
    avse_pkg.load()
    from avse_amd import _lib, ops
    from avse_amd.model import KerasModel
    res["source_digest"] = _lib.source_digest()
    dev = torch.device("cuda", 0)
    B = a.batch
    rng = np.random.default_rng(0)
    dw = ops.DeviceWeights(KerasModel.init(seed=0, randomize=True), a.dtype)
    mel = torch.from_numpy(rng.normal(-40, 12, (B, 80, 20)).astype(np.float32)).to(dev)
    host = {"u8": torch.from_numpy(rng.integers(0, 256, (B, 128, 128, 5), dtype=np.uint8)).pin_memory()}
    host["f32"] = host["u8"].float().pin_memory()
    video = {k: v.to(dev) for k, v in host.items()}
    mean = torch.from_numpy(rng.uniform(90, 160, (128, 128)).astype(np.float32)).to(dev)
    std = torch.from_numpy(rng.uniform(40, 90, (128, 128)).astype(np.float32)).to(dev)
    out = torch.empty((B, 80, 20), dtype=torch.float32, device=dev)
    outs = {k: ops.forward(dw, mel, video[k], mean, std).clone() for k in video}
    res["outputs_bit_equal"] = bool(torch.equal(outs["u8"], outs["f32"]))

    # (b) stage times
    stage = {k: {"v_conv1": [], "all_stages": []} for k in video}
    for k in video:
        for _ in range(5):
            ops.forward_profile(dw, mel, video[k], mean, std, out=out)
    for _ in range(a.rounds):
        for k in video:
            for _ in range(a.reps):
                _, ms = ops.forward_profile(dw, mel, video[k], mean, std, out=out)
                stage[k]["v_conv1"].append(ms["v_conv1"])
                stage[k]["all_stages"].append(sum(ms.values()))
    res["forward_profile_ms"] = {k: {s: spread(v) for s, v in d.items()} for k, d in stage.items()}
    print(json.dumps(res["forward_profile_ms"]), flush=True)

    # (c) upload-inclusive wall time per step
    def step(k):
        video[k].copy_(host[k], non_blocking=True)
        ops.forward(dw, mel, video[k], mean, std, out=out)

    wall = {k: [] for k in video}
    for k in video:
        for _ in range(5):
            step(k)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k in video:
            for _ in range(a.reps):
                t0 = time.perf_counter()
                step(k)
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
    res["upload_inclusive_wall_ms_per_step"] = {k: spread(v) for k, v in wall.items()}
    res["video_bytes_per_step"] = {k: int(host[k].numel() * host[k].element_size()) for k in host}
    res["upload_inclusive_clips_per_s"] = {k: B / (res["upload_inclusive_wall_ms_per_step"][k]["median"] * 1e-3)
                                           for k in wall}
    print(json.dumps(res["upload_inclusive_wall_ms_per_step"]), flush=True)
    # (d) normaliser fit
    del video, host
    fit_set = {"u8": torch.from_numpy(rng.integers(0, 256, (a.slices, 128, 128, 5), dtype=np.uint8)).to(dev)}
    fit_set["f32"] = fit_set["u8"].float()
    fit_ms = {k: [] for k in fit_set}
    for k in fit_set:
        for _ in range(5):
            ops.video_stats(fit_set[k])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for k in fit_set:
            for _ in range(a.reps):
                e0.record()
                ops.video_stats(fit_set[k])
                e1.record()
                e1.synchronize()
                fit_ms[k].append(e0.elapsed_time(e1))
    res["video_stats"] = {k: {"ms": spread(v), "bytes": int(fit_set[k].numel() * fit_set[k].element_size()),
                              "GBps_at_median": fit_set[k].numel() * fit_set[k].element_size() / np.median(v) / 1e6}
                          for k, v in fit_ms.items()}
    print(json.dumps(res["video_stats"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fd:
            json.dump(res, fd, indent=1)
    print(json.dumps({k: res[k] for k in ("outputs_bit_equal", "video_bytes_per_step", "upload_inclusive_clips_per_s")}))


if __name__ == "__main__":
    main()
