"""CPU tests of the frame retimer (avse_retime_* / avse_retimer_*): the exports, the rule of which
rate pairs are served, the counts of final frames and slices against a brute-force count from the definition, the
prefix property on the numpy reference itself (tests/retime_ref.py), the float -> rational conversion of a rate, and
the host geometry (csrc/retime_geom.h) under AddressSanitizer / UndefinedBehaviorSanitizer in a stand-alone program
(tests/native/retime_geom_check.cpp).  The device arithmetic is in tests/test_gpu_retime.py."""
import ctypes
import inspect
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import retime_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-visual-speech-enhancement_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INVALID, UNSUPPORTED = 1, 3
NEW = ("avse_retime_supported", "avse_retime_counts", "avse_retime_ragged", "avse_retimer_create",
       "avse_retimer_push_each", "avse_retimer_reset_each", "avse_retimer_state", "avse_retimer_destroy")
# (p, q) -> a rate pair (fps_in, fps_out) that reduces to it
RATIOS = {(6, 5): (30, 25), (1200, 1001): ((30000, 1001), 25), (3, 5): (15, 25), (12, 5): (60, 25), (5, 6): (25, 30),
          (24, 25): (24, 25), (2997, 2500): ((2997, 100), 25), (5, 4): (5, 4), (2, 1): (50, 25), (1, 1): (25, 25)}


def test_library_exports_the_retimer():
    from avse_amd import _lib
    lib = _lib.load()
    for f in NEW:
        assert hasattr(lib, f) and f in _lib.SIGNATURES, f
    assert len(_lib.SIGNATURES["avse_retime_ragged"][1]) == 15
    assert len(_lib.SIGNATURES["avse_retimer_push_each"][1]) == 9
    assert len(_lib.SIGNATURES["avse_retimer_create"][1]) == 9
    assert lib.avse_abi_version() == 3          # additive: the ABI version did not move
    with open(os.path.join(ROOT, "include", "avse.h")) as fh:
        header = fh.read()
    assert "#define AVSE_ABI_VERSION 3" in header
    version_comment = header[:header.index("#define AVSE_ABI_VERSION")]
    for f in NEW:
        assert f"{f}(" in header and f in version_comment, f


def test_python_surface():
    from avse_amd import ops, pipeline
    for f in ("retime", "retime_supported", "retime_counts", "retimer_create", "retimer_push_each", "retimer_reset_each"):
        assert callable(getattr(ops, f)), f
    assert callable(ops.Retimer.expect)
    assert inspect.signature(pipeline.StreamEnhancer.__init__).parameters["input_fps"].default is None
    assert list(inspect.signature(pipeline.StreamEnhancer.__init__).parameters)[-1] == "input_fps"
    with pytest.raises(TypeError):              # CPU tensors are refused, as everywhere
        import torch
        ops.retime(torch.zeros(1, 6, 128, 128), 30, 25, 5)


def test_the_rule():
    from avse_amd import _lib, ops
    for (p, q), (a, b) in RATIOS.items():
        assert retime_ref.ratio(a, b) == (p, q)
        assert ops.retime_supported(a, b) == 0, (a, b)
        assert ops.retime_supported(b, a) == 0, (b, a)
    rc, msg = ops.retime_supported(65537, 1, return_message=True)
    assert rc == UNSUPPORTED and "65537 / 1" in msg, msg
    assert ops.retime_supported(65536, 1) == 0
    rc, msg = ops.retime_supported(0, 25, return_message=True)
    assert rc == INVALID and msg
    assert ops.retime_supported(30, -25) == INVALID
    assert ops.retime_supported((30, -1), 25) == INVALID
    lib = _lib.load()
    assert lib.avse_retime_supported(30, 0, 25, 1) == INVALID
    f, k = ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert lib.avse_retime_counts(65537, 1, 1, 1, 5, 10, 0, ctypes.byref(f), ctypes.byref(k)) == UNSUPPORTED
    assert b"65537 / 1" in lib.avse_last_error()
    assert lib.avse_retime_counts(30, 1, 25, 1, 5, -1, 0, ctypes.byref(f), ctypes.byref(k)) == INVALID
    assert lib.avse_retime_counts(30, 1, 0, 1, 5, 10, 0, ctypes.byref(f), ctypes.byref(k)) == INVALID
    assert lib.avse_retime_counts(30, 1, 25, 1, 7, 10, 0, ctypes.byref(f), ctypes.byref(k)) == UNSUPPORTED
    assert lib.avse_retime_counts(30, 1, 25, 1, 5, 10, 0, None, None) == INVALID and b"NULL" in lib.avse_last_error()
    for flushed in (0, 1):                      # totals past 2^40 frames
        assert lib.avse_retime_counts(30, 1, 25, 1, 5, 2 ** 40 + 1, flushed, ctypes.byref(f), ctypes.byref(k)) == INVALID
        assert b"too large" in lib.avse_last_error()
    assert (f.value, k.value) == (-7, -7)       # no refused call wrote a count
    assert lib.avse_retime_counts(30, 1, 25, 1, 5, 13, 0, ctypes.byref(f), None) == 0 and f.value == 11
    assert lib.avse_retime_counts(30, 1, 25, 1, 5, 13, 0, None, ctypes.byref(k)) == 0 and k.value == 2
    assert lib.avse_retime_counts(6, 5, 1, 1, 5, 2 ** 40, 1, ctypes.byref(f), ctypes.byref(k)) == 0   # the last n served
    assert (f.value, k.value) == (-(-2 ** 40 * 5 // 6), -(-2 ** 40 * 5 // 6) // 5)
    assert lib.avse_retimer_create(None, 1, 30, 1, 25, 1, 5, 0, None) == INVALID
    assert lib.avse_retimer_push_each(None, None, None, None, None, None, 0, None, None) == INVALID
    assert lib.avse_retimer_state(None, None, None, None) == INVALID
    assert lib.avse_retime_ragged(None, None, None, None, 0, 0, 30, 1, 25, 1, 5, None, 0, None, None) == INVALID


@pytest.mark.parametrize("F", [5, 6])
@pytest.mark.parametrize("ratio", sorted(RATIOS))
def test_counts_match_the_definition(ratio, F):
    """G(n): the outputs j with ceil(j p / q) <= n - 1; flushed: those with j p < n q; for every n in 0..600."""
    from avse_amd import ops
    p, q = ratio
    a, b = RATIOS[ratio]
    n = np.arange(601, dtype=np.int64)
    j = np.arange(600 * q // p + 3, dtype=np.int64)
    last = -(-j * p // q)                                        # ceil(j p / q): ascending in j
    brute = np.searchsorted(last, n - 1, side="right")          # outputs with last <= n - 1
    brute_flushed = np.searchsorted(j * p, n * q, side="left")  # outputs with j p < n q
    assert brute.max() < j.size and brute_flushed.max() < j.size
    for i in n:
        got = ops.retime_counts(a, b, F, int(i))
        assert got == (brute[i], brute[i] // F), (ratio, i, got)
        got = ops.retime_counts(a, b, F, int(i), True)
        assert got == (brute_flushed[i], brute_flushed[i] // F), (ratio, i, got)
        assert got[0] == retime_ref.total(p, q, int(i), True) and brute[i] == retime_ref.total(p, q, int(i), False)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("ratio", sorted(RATIOS))
def test_the_prefix_property_holds_for_the_reference(ratio, dtype):
    """The first G(n) outputs of the reference on a prefix A[:n] are those on the whole sequence, bit for bit, and the
    frames a flush adds are copies of the prefix's last frame; G(n) and the flushed total are the library's
    (avse_retime_counts), so the property is stated for the counts the device code uses."""
    from avse_amd import ops
    p, q = ratio
    a, b = RATIOS[ratio]
    rng = np.random.default_rng(p * 100003 + q)
    A = rng.integers(0, 256, (23, 4, 4)).astype(dtype) if dtype == np.uint8 else \
        (rng.normal(0, 50, (23, 4, 4))).astype(np.float32)
    whole = retime_ref.frames(A, p, q)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint8)
    for n in (1, 2, 5, 6, 7, 22):
        G = retime_ref.total(p, q, n, False)
        part = retime_ref.frames(A[:n], p, q)
        assert G == ops.retime_counts(a, b, 5, n)[0] and part.shape[0] == ops.retime_counts(a, b, 5, n, True)[0]
        assert part.shape[0] == retime_ref.total(p, q, n, True) >= G >= 1
        assert np.array_equal(bits(part[:G]), bits(whole[:G])), (ratio, n)
        assert np.array_equal(bits(retime_ref.frames(A[:n], p, q, flushed=False)), bits(whole[:G]))
        for j in range(G, part.shape[0]):
            assert np.array_equal(bits(part[j]), bits(A[n - 1])), (ratio, n, j)
        if G < whole.shape[0]:                  # and G is tight: the next output reads A[n]
            assert -(-G * p // q) >= n
    if (p, q) == (1, 1):                        # equal rates regroup the bits
        assert np.array_equal(bits(whole), bits(A))
        assert np.array_equal(retime_ref.slices(A, 1, 1, 5)[1, :, :, 2], A[7])


def test_a_float_rate_becomes_a_rational():
    from avse_amd import ops
    assert ops.frame_rate(29.97) == Fraction(2997, 100)
    assert ops.frame_rate(30000 / 1001) == Fraction(30000, 1001)
    assert ops.frame_rate(25.0) == 25 and ops.frame_rate(30) == 30
    assert ops.frame_rate((30000, 1001)) == Fraction(30000, 1001) == ops.frame_rate(Fraction(30000, 1001))
    assert ops.retime_counts(30000 / 1001, 25, 5, 1201, True) == ops.retime_counts((30000, 1001), 25.0, 5, 1201, True)
    assert ops.retime_counts(29.97, 25, 5, 2998) == (2501, 500)


def test_retime_geometry_sanitized(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host sources are built with the kernels' compiler")
    exe = str(tmp_path / "retime_geom_check")
    # host code only: the sanitizers are named for the host side of the compiler, never for a GPU code object
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++20", "-O2", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                         "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC,
                         os.path.join(ROOT, "tests", "native", "retime_geom_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"exit status {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100000
