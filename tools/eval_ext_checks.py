"""Writes avse_eval_pairs_ext's parity record (profiles/eval_ext_checks.txt): for every case of
tests/test_gpu_eval_ext.py, the float32 yardsticks of the reference (|float32 - float64| STOI and ESTOI of
tests/eval_ext_ref.py), the mask margin, and the device's measured errors against the float64 reference, next to the
gates the tests assert.
    python tools/eval_ext_checks.py [--out profiles/eval_ext_checks.txt]"""
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
import eval_ext_ref as E  # noqa: E402
import eval_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_ext_checks.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_ext_checks.py measures on the GPU: none visible")
    cases = [(name, sr, s, y) for name, sr, s, y, _ in E.cases()] + \
            [(name, 16000, s, y) for name, s, y in R.ragged_cases()]
    got = {}
    for sr in sorted({c[1] for c in cases}):       # one ragged launch per rate
        group = [c for c in cases if c[1] == sr]
        rows = ops.eval_pairs_ext([c[2] for c in group], [c[3] for c in group], sr).cpu().numpy()
        got.update({c[0]: r for c, r in zip(group, rows)})
    lines = [f"evaluate stage, avse_eval_pairs_ext, {torch.cuda.get_device_name(0)}, source digest {_lib.source_digest()}",
             "device: ops.eval_pairs_ext with any_rate (the cases of one rate in one ragged launch)",
             "reference: tests/eval_ext_ref.py float64; yardsticks: the same with the framing, FFT, bands and segments in "
             "float32", "",
             "%-22s %6s %8s %4s %10s %11s %10s %10s %11s %10s %10s %10s %6s" %
             ("case", "sr", "samples", "K", "margin dB", "STOI f64", "yardstick", "dev STOI", "ESTOI f64", "yardstick",
              "dev ESTOI", "dev dB max", "equal")]
    worst = {R.STOI: [0.0, 0.0], E.ESTOI: [0.0, 0.0]}
    worst_db = 0.0
    for name, sr, s, y in cases:
        g = got[name]
        w64, w32 = E.eval_pair_ext(s, y, sr), E.eval_pair_ext(s, y, sr, dtype=np.float32)
        fin = np.isfinite(w64[:3])
        db = float(np.abs(g[:3][fin] - w64[:3][fin]).max()) if fin.any() else 0.0
        worst_db = max(worst_db, db)
        col = {}
        for slot in (R.STOI, E.ESTOI):
            ok = np.isfinite(w64[slot])
            col[slot] = (abs(w32[slot] - w64[slot]) if ok else float("nan"), abs(g[slot] - w64[slot]) if ok else float("nan"))
            if ok:
                worst[slot] = [max(worst[slot][0], col[slot][0]), max(worst[slot][1], col[slot][1])]
        same = np.array_equal(np.isnan(g), np.isnan(w64)) and np.array_equal(np.isinf(g), np.isinf(w64)) and \
            g[R.STOI_KEPT] == w64[R.STOI_KEPT]
        lines.append("%-22s %6d %8d %4d %10.3f %11.8f %10.3e %10.3e %11.8f %10.3e %10.3e %10.3e %6s" %
                     (name, sr, s.size, int(w64[R.STOI_KEPT]), E.mask_margin(s, sr), w64[R.STOI], col[R.STOI][0],
                      col[R.STOI][1], w64[E.ESTOI], col[E.ESTOI][0], col[E.ESTOI][1], db, same))
    lines.append("")
    for slot, label in ((R.STOI, "STOI"), (E.ESTOI, "ESTOI")):
        lines.append(f"largest yardstick |float32 - float64| {label}: {worst[slot][0]:.3e}; gate = min(8 x that, 1e-5) = "
                     f"{min(8 * worst[slot][0], 1e-5):.3e}; largest device {label} error: {worst[slot][1]:.3e}")
    lines.append(f"largest device SNR / SI-SDR / segmental SNR error: {worst_db:.3e} dB (gate 1e-9 dB)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fd:
        fd.write(text)


if __name__ == "__main__":
    main()
