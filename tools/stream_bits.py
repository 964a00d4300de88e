#!/usr/bin/env python
"""The bits of a fixed, seeded streaming schedule (pipeline.StreamEnhancer), as one SHA-256 per
output: run it on two checkouts and compare the lines (a refactor of csrc/stream.hip must leave every one as it was;
profiles/stream_refactor_identity.txt holds such a comparison).

Per sample rate (16, 32, 48 kHz; P = rate / 16000), B = 3 streams of 4 slices, float32 weights:
  lockstep  pushes of [3360, 3200, 3200, 3040] P samples with one video slice each, then the flush
  each      push_each calls in which the streams' counts differ and one stream is idle, video runs ahead of the samples
            (stream 0) and behind them (stream 1), stream 2 is reset mid-way (reset_streams) and starts again, and the
            streams are flushed in two different calls
Hashed: the waveform, `mel_db` and `pred_db` of every call, concatenated per stream in call order.

  python tools/stream_bits.py --out bits_branch.txt
  python tools/stream_bits.py --root <checkout of the parent commit> --out bits_parent.txt
"""
import argparse
import hashlib
import os
import sys

LOCKSTEP = [3360, 3200, 3200, 3040]
# per call, per stream: (samples / P, video slices), None (idle) or "flush"; "reset" before a call: the streams to reset
EACH = [
    dict(push=[(3200, 2), (5000, 0), None]),
    dict(push=[(4000, 0), (1400, 2), (3200, 1)]),
    dict(reset=[2], push=[None, (3200, 1), (6400, 2)]),
    dict(push=[(5600, 2), (3200, 1), (777, 0)]),
    dict(push=["flush", None, (5623, 2)]),
    dict(push=[None, "flush", "flush"]),
]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout to import the package from (default: this one)")
    ap.add_argument("--rates", default="16000,32000,48000")
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
        sys.exit("stream_bits: no ROCm GPU visible to torch")

    B, S = 3, 4
    dw = ops.DeviceWeights(KerasModel.init(seed=8, randomize=True), "float32")
    mean = ops.to_device(np.full((128, 128), 127.5, np.float32))
    std = ops.to_device(np.full((128, 128), 73.9, np.float32))
    lines = []

    def digest(rate, case, key, parts):
        a = np.ascontiguousarray(torch.cat([p.reshape(-1) for p in parts]).cpu().numpy())
        assert np.isfinite(a).all(), (rate, case, key)
        lines.append(f"{rate:6d}  {case:9s} {key:5s} {a.size:7d} values  {hashlib.sha256(a.tobytes()).hexdigest()}")
        print(lines[-1], flush=True)

    for rate in (int(r) for r in args.rates.split(",")):
        P = rate // 16000
        rng = np.random.default_rng(rate)
        t = np.arange(12800 * P) / rate
        x = rng.normal(0, 3000, (B, 12800 * P)) + 4000 * np.sin(2 * np.pi * 440 * t) * np.linspace(0.05, 1, B)[:, None]
        xd = ops.to_device(x.round().astype(np.float32))
        vd = ops.to_device(rng.integers(0, 256, (B, S, 128, 128, 5)).astype(np.float32))
        enh = StreamEnhancer(dw, B, sample_rate=rate, max_slices=4)

        got, a = [], 0
        for k, n in enumerate(LOCKSTEP):
            got.append(enh.push(xd[:, a:a + n * P].contiguous(), vd[:, k:k + 1].contiguous(), mean, std, return_spectrograms=True))
            a += n * P
        got.append(enh.flush(mean, std, return_spectrograms=True))
        for i, key in enumerate(("out", "mel", "pred")):
            digest(rate, "lockstep", key, [torch.cat([g[i] for g in got], dim=1)])

        enh.reset()
        pos, vpos = [0] * B, [0] * B
        got = [([], [], []) for _ in range(B)]
        for call in EACH:
            if "reset" in call:
                enh.reset_streams(call["reset"])
                for b in call["reset"]:
                    pos[b] = vpos[b] = 0
            samples, vids, flush = [None] * B, [None] * B, [False] * B
            for b, what in enumerate(call["push"]):
                if what == "flush":
                    flush[b] = True
                elif what is not None:
                    n, v = what[0] * P, what[1]
                    samples[b] = xd[b, pos[b]:pos[b] + n]
                    vids[b] = vd[b, vpos[b]:vpos[b] + v] if v else None
                    pos[b], vpos[b] = pos[b] + n, vpos[b] + v
            res = enh.push_each(samples, vids, flush, mean, std, return_spectrograms=True)
            for b in range(B):
                for i in range(3):
                    got[b][i].append(res[i][b])
        assert pos == [12800 * P] * B and vpos == [S] * B
        for b in range(B):
            for i, key in enumerate(("out", "mel", "pred")):
                digest(rate, f"each[{b}]", key, got[b][i])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
