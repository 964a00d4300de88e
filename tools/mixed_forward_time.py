"""Step time of the bench workload (B clips, STFT + forward) when only some clips have video (avse_forward_mixed):
100, 75, 50, 25 and 0 % present against the plain forward and the video=None forward of the same build, in
float32_split and bf16.  The legs alternate round by round, so the box's drift lands on all of them; each figure is the
median over the rounds of a round's mean step (HIP events), and `spread` is min..max of the plain leg's rounds.
    python tools/mixed_forward_time.py [--batch 512] [--rounds 7] [--reps 20] [--plain-only] [--out FILE]
--plain-only times the plain forward alone (it needs no mixed entry point, so it also runs on an older build).
Prints one JSON line; --out appends it to FILE."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import avse_pkg  # noqa: E402

avse_pkg.load()
import bench  # noqa: E402
from avse_amd import _lib, ops  # noqa: E402
from avse_amd.model import KerasModel  # noqa: E402

SHARES = (100, 75, 50, 25, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--dtypes", nargs="*", default=["float32_split", "bf16"])
    ap.add_argument("--out")
    args = ap.parse_args()
    B = args.batch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1234)
    a, v = bench.synth(rng, B)
    audio, video = torch.from_numpy(a).to(dev), torch.from_numpy(v).to(dev)
    mean = torch.from_numpy(v.mean(axis=(0, 3)).astype(np.float32)).to(dev)
    std = torch.from_numpy(v.std(axis=(0, 3)).astype(np.float32)).to(dev)
    model = KerasModel.init(seed=0, randomize=True)
    mel = torch.empty((B, 1, 80, 20), dtype=torch.float32, device=dev)
    out = torch.empty((B, 80, 20), dtype=torch.float32, device=dev)
    result = {"tool": "mixed_forward_time", "batch": B, "rounds": args.rounds, "reps": args.reps,
              "source": _lib.source_digest(), "device": torch.cuda.get_device_name(0), "ms": {}}
    for dt in args.dtypes:
        dw = ops.DeviceWeights(model, dt, dev)
        dw.ctx.reserve_for(dw, B)
        clips = mel.view(B, 80, 20)
        legs = {"plain": lambda: ops.forward(dw, clips, video, mean, std, out=out)}
        if not args.plain_only:
            legs["none"] = lambda: ops.forward(dw, clips, None, out=out)
            for share in SHARES:
                mask = np.zeros(B, bool)
                mask[rng.permutation(B)[:B * share // 100]] = True
                packed = video[torch.from_numpy(mask).to(dev)].contiguous() if mask.any() else None
                legs[f"mixed_{share}"] = (lambda m=mask, p=packed:
                                          ops.forward(dw, clips, p, mean, std, out=out, video_present=m))

        def step(fwd):
            ops.spectrogram(audio, frames_per_slice=20, out=mel)
            fwd()
        for fwd in legs.values():      # every shape the timed window uses
            for _ in range(3):
                step(fwd)
        times = {k: [] for k in legs}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for name, fwd in legs.items():
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    step(fwd)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.reps)
        ms = {k: round(float(np.median(t)), 4) for k, t in times.items()}
        ms["plain_spread"] = [round(min(times["plain"]), 4), round(max(times["plain"]), 4)]
        result["ms"][dt] = ms
        del dw
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
