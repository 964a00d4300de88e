"""Writes the evaluate stage's parity record (profiles/eval_checks.txt): for every case of tests/test_gpu_eval.py, the
float32 yardstick of the reference (|float32 - float64| STOI of tests/eval_ref.py), the mask margin, and the device's
measured errors against the float64 reference, next to the gates the tests assert.
    python tools/eval_checks.py [--out profiles/eval_checks.txt]"""
import argparse
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
import eval_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_checks.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_checks.py measures on the GPU: none visible")
    cases = [(name, 16000, s, y) for name, s, y in R.ragged_cases()] + R.boundary_cases()
    got = ops.eval_pairs([c[2] for c in cases[:len(R.RAGGED_LENGTHS)]], [c[3] for c in cases[:len(R.RAGGED_LENGTHS)]],
                         16000).cpu().numpy()
    got = np.concatenate([got] + [ops.eval_pairs([s], [y], sr).cpu().numpy() for _, sr, s, y in cases[len(got):]])
    lines = [f"evaluate stage, {torch.cuda.get_device_name(0)}, source digest {_lib.source_digest()}",
             "device: ops.eval_pairs (the ragged cases in one launch, the boundary cases one launch each)",
             "reference: tests/eval_ref.py float64; yardstick: the same with STOI's framing, FFT and bands in float32",
             "", "%-22s %6s %9s %5s %11s %11s %11s %11s %11s %11s" %
             ("case", "sr", "samples", "K", "margin dB", "STOI f64", "yardstick", "dev STOI", "dev dB max", "K equal")]
    worst_y, worst_d, worst_db = 0.0, 0.0, 0.0
    for (name, sr, s, y), g in zip(cases, got):
        w64, w32 = R.eval_pair(s, y, sr), R.eval_pair(s, y, sr, dtype=np.float32)
        fin = np.isfinite(w64[:3])
        db = float(np.abs(g[:3][fin] - w64[:3][fin]).max()) if fin.any() else 0.0
        yard = abs(w32[R.STOI] - w64[R.STOI]) if np.isfinite(w64[R.STOI]) else float("nan")
        derr = abs(g[R.STOI] - w64[R.STOI]) if np.isfinite(w64[R.STOI]) else float("nan")
        if np.isfinite(yard):
            worst_y, worst_d = max(worst_y, yard), max(worst_d, derr)
        worst_db = max(worst_db, db)
        same = np.array_equal(np.isnan(g), np.isnan(w64)) and np.array_equal(np.isinf(g), np.isinf(w64)) and \
            g[R.STOI_KEPT] == w64[R.STOI_KEPT]
        lines.append("%-22s %6d %9d %5d %11.3f %11.8f %11.3e %11.3e %11.3e %11s" %
                     (name, sr, s.size, int(w64[R.STOI_KEPT]), R.mask_margin(s, sr), w64[R.STOI], yard, derr, db, same))
    lines += ["", f"largest yardstick |float32 - float64| STOI: {worst_y:.3e}; STOI gate = min(8 x that, 1e-5) = "
              f"{min(8 * worst_y, 1e-5):.3e}", f"largest device STOI error: {worst_d:.3e}",
              f"largest device SNR / SI-SDR / segmental SNR error: {worst_db:.3e} dB (gate 1e-9 dB)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fd:
        fd.write(text)


if __name__ == "__main__":
    main()
