"""The forward plan on the CPU (csrc/forward_plan.h): the arena layout and the split-K plans of v_conv6 and the dense
layers, for every recorded network shape, dtype, gemm_ksplit_cap and batch, must be exactly what
tests/golden/forward_plan.json records (written by the code before the plan moved into one header), and
tests/native/forward_plan_check.cpp asserts on every row that the offsets are aligned and increasing, that the
partial-sum workspace holds what each layer's launch writes, and that a k_gemm split plan is one launch_gemm accepts."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_forward_plan_matches_fixture(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found")
    exe = str(tmp_path / "forward_plan_check")
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++20", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tests", "native", "forward_plan_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"exit status {run.returncode}\n{run.stdout[-4000:]}\n{run.stderr[-4000:]}"
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK", run.stdout[-2000:]
    with open(os.path.join(ROOT, "tests", "golden", "forward_plan.json")) as f:
        want = json.load(f)["rows"]
    got = [[int(x) for x in line.split()] for line in lines[:-1]]
    assert len(want) == 5 * 3 * 2 * 11
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, f"(T, F, dtype, cap, N) = {w[:5]}:\n got {g}\nwant {w}"
