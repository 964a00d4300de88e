#!/usr/bin/env python
"""Why a 44.1 kHz stream is resampled to the session's rate instead of framed natively: the mel-dB
features of a native 44.1 kHz geometry (n_fft 1764, hop 441) against those of the same signal resampled to 16 kHz
(n_fft 640, hop 160), both from the float64 oracle (oracle/librosa_ref.py, tests/eval_ref.py resample).  CPU only.

Prints the constant offset 20 log10(1764 / 640), the residual in bands 0 .. 74 of the interior frames, and the RMS
deficit of the top bands, which sit in the transition band of the resampler's anti-alias filter at 8 kHz.

  python tools/anyrate_feature_scale.py [--seconds 1.0] [--seed 7] [--snr-db 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--snr-db", type=float, default=5.0)
    args = ap.parse_args()
    import eval_ref
    from oracle import librosa_ref as R

    n = int(round(args.seconds * 44100))
    _, x = eval_ref.speech_like(args.seed, n, 44100, args.snr_db)
    y = eval_ref.resample(x, 160, 441)

    def mel_db(sig, sr, n_fft):
        mag, _ = R.magphase(R.stft(np.asarray(sig, np.float64), n_fft=n_fft, hop_length=n_fft // 4))
        return R.amplitude_to_db(np.dot(R.mel_filterbank(sr, n_fft, n_mels=80, fmin=0, fmax=8000), mag), top_db=None)

    native, resampled = mel_db(x, 44100, 1764), mel_db(y, 16000, 640)
    T = min(native.shape[1], resampled.shape[1])
    d = native[:, :T] - resampled[:, :T]
    scale = 20.0 * np.log10(1764.0 / 640.0)
    inner = d[:, 2:T - 2] - scale
    print(f"{n} samples at 44.1 kHz -> {y.size} at 16 kHz, {T} frames")
    print(f"window-length offset 20 log10(1764 / 640) = {scale:.3f} dB; measured mean over bands 0..74, interior frames: "
          f"{d[:75, 2:T - 2].mean():.3f} dB")
    print(f"bands 0..74, interior frames, offset removed: max |d| {np.abs(inner[:75]).max():.3f} dB, RMS "
          f"{np.sqrt(np.mean(inner[:75] ** 2)):.3f} dB")
    for b in (75, 76, 77, 78, 79):
        print(f"band {b}: resampled features lower by {np.sqrt(np.mean(inner[b] ** 2)):.2f} dB RMS (mean {inner[b].mean():+.2f} dB)")
    edge = np.abs(d[:75, [0, 1, T - 2, T - 1]] - scale).max()
    print(f"first and last two frames, bands 0..74: max |d - offset| {edge:.2f} dB (the filter sees zeros past the ends)")


if __name__ == "__main__":
    main()
