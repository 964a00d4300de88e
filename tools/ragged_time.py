"""Ragged STFT / ISTFT timing on the GPU box (modelled on tools/stft_time.py): one ragged call against the way the
same work ran before it.

  (a) 64 utterances of 64 distinct lengths between 1 s and 4 s: ops.spectrogram_ragged / ops.istft_ragged against the
      per-length loop of equal-length calls (64 launches each, one utterance per launch);
  (b) 64 utterances of one length (3 s): the ragged calls against the single equal-length call (the same launch).

Both sides get their inputs packed beforehand (the ragged side as (buffer, offsets, lengths), the loop as [1, L]
tensors); the STFT keeps the complex output and slices to 20 frames, as the predictors use it.  HIP events around
`reps` back-to-back calls after a warm-up of every shape (python launch overhead included, as in stft_time.py); the two
sides alternate over `rounds` rounds and the report gives each side's median and its min .. max over the rounds.
Usage: python tools/ragged_time.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import avse_pkg  # noqa: E402

avse_pkg.load()
from avse_amd import ops  # noqa: E402

SPF = 20


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def compare(sides, reps=20, rounds=7):
    """sides: {name: fn} -> {name: dict(median_ms, min_ms, max_ms)}; the sides alternate inside every round."""
    for fn in sides.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed(fn, reps))
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v))) for k, v in ms.items()}


def batch(dev, lens, seed):
    rng = np.random.default_rng(seed)
    sigs = []
    for L in lens:
        t = np.arange(L) / 16000.0
        sigs.append(torch.from_numpy((rng.normal(0, 3000, L) + 3000 * np.sin(2 * np.pi * 440 * t)).astype(np.float32)).to(dev))
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return sigs, (torch.cat(sigs), off, np.asarray(lens, np.int64))


def measure(dev, lens, seed, equal):
    sigs, packed = batch(dev, lens, seed)
    rows = [s[None].contiguous() for s in sigs]
    stacked = torch.stack(sigs) if equal else None
    box = {}

    def ragged_stft():
        box["r"] = ops.spectrogram_ragged(packed, frames_per_slice=SPF, return_stft=True)

    def loop_stft():
        box["l"] = [ops.spectrogram(r, frames_per_slice=SPF, return_stft=True) for r in rows]

    def one_stft():
        box["o"] = ops.spectrogram(stacked, frames_per_slice=SPF, return_stft=True)

    old_stft = one_stft if equal else loop_stft
    out = {"stft": compare({"ragged": ragged_stft, "parent": old_stft})}
    mel, counts, views, stft, sviews = box["r"]
    frames = [sh[1] for sh in sviews.shapes]
    if equal:
        pm, pd = box["o"]
        assert torch.equal(pm.view(-1), mel.view(-1)) and torch.equal(pd.reshape(-1), stft)
    else:
        for u, (m, d) in enumerate(box["l"]):
            assert torch.equal(m[0], views[u]) and torch.equal(d[0], sviews[u]), u
    pred = mel + 1.0        # any prediction: the ISTFT's time does not depend on the values

    def ragged_istft():
        box["ri"] = ops.istft_ragged(pred, counts, stft, frames)

    pieces = [(pred[int(e - c):int(e)][None].contiguous(), sviews[u][None].contiguous())
              for u, (e, c) in enumerate(zip(np.cumsum(counts), counts))]

    def loop_istft():
        box["li"] = [ops.istft(m, d) for m, d in pieces]

    if equal:
        pm4, pd3 = pred.view(len(lens), -1, 80, SPF), stft.view(len(lens), 321, -1)

    def one_istft():
        box["oi"] = ops.istft(pm4, pd3)

    out["istft"] = compare({"ragged": ragged_istft, "parent": one_istft if equal else loop_istft})
    if equal:
        assert torch.equal(torch.cat(box["ri"]), box["oi"].view(-1))
    else:
        for u, y in enumerate(box["li"]):
            assert torch.equal(y[0], box["ri"][u]), u
    out["utterances"] = len(lens)
    out["seconds_of_audio"] = float(sum(lens) / 16000.0)
    return out


def main():
    dev = torch.device("cuda", 0)
    res = {
        "a_64_distinct_lengths_1s_to_4s_vs_per_length_loop": measure(dev, [int(v) for v in np.linspace(16000, 64000, 64)], 1, False),
        "b_64_equal_lengths_3s_vs_single_equal_length_call": measure(dev, [48000] * 64, 2, True),
    }
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
