"""k_gemm's split-K ticket bound on the CPU (csrc/layer_geom.h gemm_tickets_fit): the split dtype's dense layers always
take the ticket path, one counter per 128 x 128 output tile of a fixed per-context array, so a forward of more clips than
the array has tiles for (dec_dense2: past 41,856) must be declined by launch_gemm and run on k_conv.  The bound is host
arithmetic, checked here by tests/native/gemm_tickets_check.cpp without a GPU (no such batch is run on one)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_gemm_ticket_bound(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found")
    exe = str(tmp_path / "gemm_tickets_check")
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++20", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tests", "native", "gemm_tickets_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"exit status {run.returncode}\n{run.stdout[-4000:]}\n{run.stderr[-4000:]}"
    assert run.stdout.rstrip().endswith("OK"), run.stdout[-2000:]
