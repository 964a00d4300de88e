"""CPU tests of the sliding streaming session's host side (avse_slide_*, include/avse.h; csrc/slide_geom.h): the
exports, avse_slide_supported, the host-only totals against the closed forms of the definitions, stride F against
avse_stream_counts, every refusal the C-ABI decides before it touches a session, and the host geometry under
AddressSanitizer / UndefinedBehaviorSanitizer against a brute-force definition (a stand-alone program,
tests/native/slide_geom_check.cpp).  What needs a live session is in tests/test_gpu_slide.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from slide_ref import totals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-visual-speech-enhancement_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INVALID, UNSUPPORTED = 1, 3
SYMBOLS = {"avse_slide_supported": 9, "avse_slide_create": 16, "avse_slide_counts": 9, "avse_slide_counts_geom": 12,
           "avse_slide_push_each": 16, "avse_slide_reset_each": 3, "avse_slide_reset": 2, "avse_slide_state": 4,
           "avse_slide_destroy": 1}
GEOMS = ((640, 160, 20, 5), (800, 200, 24, 6))


def test_library_exports_the_sliding_entry_points():
    from avse_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "avse.h")).read()
    assert "typedef struct avse_slide avse_slide;" in header
    for f, arity in SYMBOLS.items():
        assert hasattr(lib, f) and f in _lib.SIGNATURES, f
        assert len(_lib.SIGNATURES[f][1]) == arity, f
        m = re.search(r"\b(int|void)\s+%s\s*\(([^;]*)\);" % f, header)
        assert m, f"include/avse.h does not declare {f}"
        assert len(re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",")) == arity, f
        assert f in header.split("#define AVSE_ABI_VERSION")[0], f      # listed in the version comment
    assert lib.avse_abi_version() == 3          # additive: the ABI version did not move
    assert "avse_slide_push_each" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_supported_geometries_and_strides():
    from avse_amd import ops
    built = [(16000, 640, 160, 20, 5), (32000, 1280, 320, 20, 5), (48000, 1920, 480, 20, 5), (24000, 800, 200, 24, 6),
             (48000, 1600, 400, 24, 6)]
    for sr, n_fft, hop, spf, F in built:
        assert ops.stream_supported(sr, n_fft, hop, spf) == 0
        for stride in range(1, F + 1):
            assert ops.slide_supported(sr, n_fft, hop, spf, F, stride) == 0, (sr, n_fft, stride)
        for stride in (0, -1, F + 1):
            rc, why = ops.slide_supported(sr, n_fft, hop, spf, F, stride, return_message=True)
            assert rc == INVALID and "stride" in why, (sr, stride, why)
    # what avse_stream_supported refuses stays refused, with its status: 800 / 200 at 16 kHz, 29.97 fps, 44.1 kHz
    for sr, n_fft, hop, spf, F in [(16000, 800, 200, 24, 6), (16000, 533, 133, 24, 6), (44100, 1764, 441, 20, 5)]:
        assert ops.slide_supported(sr, n_fft, hop, spf, F, 1) == ops.stream_supported(sr, n_fft, hop, spf) == UNSUPPORTED
    rc, why = ops.slide_supported(16000, 640, 160, 20, 6, 1, return_message=True)      # 20 % 6 != 0
    assert rc == UNSUPPORTED and "frames_per_slice % video_frames" in why
    assert ops.slide_supported(16000, 640, 160, 20, 4, 1) == UNSUPPORTED                # no 4-frame gather is built
    assert ops.slide_supported(16000, 640, 160, 20, 0, 1) == INVALID
    assert ops.slide_supported(16000, 640, 160, 20, 5, 1, n_mels=64) == UNSUPPORTED
    for fmin, fmax in ((0.0, 4000.0), (0.0, 7999.0), (300.0, 8000.0), (0.0, 12000.0)):     # the bank rule is the session's
        assert ops.slide_supported(16000, 640, 160, 20, 5, 1, fmin=fmin, fmax=fmax) == \
            ops.stream_supported(16000, 640, 160, 20, fmin=fmin, fmax=fmax), (fmin, fmax)


@pytest.mark.parametrize("geometry", GEOMS)
def test_counts_follow_the_closed_forms(geometry):
    """n and f swept through the first three windows (and a little past), not flushed and flushed, for every stride."""
    from avse_amd import ops
    n_fft, hop, spf, F = geometry
    q = spf // F
    for stride in range(1, F + 1):
        n_top = hop * (spf + 3 * q * stride) + n_fft
        for f in range(0, F + 3 * stride + 2):
            for n in sorted(set(range(0, n_top, 61)) | {n_fft // 2, n_fft // 2 + 1, hop * spf + n_fft // 2 - hop - 1,
                                                        hop * spf + n_fft // 2 - hop, hop * q * f}):
                want = totals(n, f, stride, False, n_fft, hop, spf, F)
                assert ops.slide_counts(n, f, False, stride, geometry=geometry) == want, (stride, n, f)
                if n <= hop * q * f:
                    want = totals(n, f, stride, True, n_fft, hop, spf, F)
                    assert ops.slide_counts(n, f, True, stride, geometry=geometry) == want, (stride, n, f)
                    assert want[0] == q * f and want[1] == ((f - F) // stride + 1 if f >= F else 0)
                if geometry == GEOMS[0]:      # a NULL session is this geometry
                    assert ops.slide_counts(n, f, False, stride) == totals(n, f, stride)
    # the figures of the 20-frame stream the GPU tests use
    if geometry == GEOMS[0]:
        assert ops.slide_counts(12800, 20, True, 1) == (80, 16, 80, 12640)
        assert ops.slide_counts(12800, 20, False, 2) == (79, 8, 76, 11840)
        assert ops.slide_counts(12800, 20, True, 2) == (80, 8, 76, 12000)


@pytest.mark.parametrize("geometry", GEOMS)
def test_stride_F_is_the_existing_session(geometry):
    """Every formula reduces to stream_totals at v = f / F: the same frames, windows == slices, the same samples."""
    from avse_amd import _lib
    lib = _lib.load()
    n_fft, hop, spf, F = geometry
    q = spf // F
    out = [ctypes.c_int64() for _ in range(3)]
    refs = [ctypes.byref(o) for o in out]

    def stream_counts(n, v, flushed):
        if geometry == GEOMS[0]:
            assert lib.avse_stream_counts(None, n, v, int(flushed), *refs) == 0
            return tuple(o.value for o in out)
        # avse_stream_counts without a session is the 640-point geometry: the (24, 6) pair by its closed form
        if flushed:
            return spf * v, v, hop * (spf * v - 1) if v else 0
        frames = 0 if n < n_fft // 2 + 1 else (n - n_fft // 2) // hop + 1
        k = min(frames // spf, v)
        return frames, k, max(0, spf * hop * k - n_fft // 2)
    from avse_amd import ops
    for v in range(0, 4):
        for n in range(0, hop * spf * 3 + n_fft, 53):
            for flushed in (False, True):
                if flushed and n > hop * q * F * v:
                    continue
                frames, windows, predicted, emitted = ops.slide_counts(n, F * v, flushed, F, geometry=geometry)
                assert (frames, windows, emitted) == stream_counts(n, v, flushed), (n, v, flushed)
                assert predicted == spf * windows


def test_counts_refusals():
    from avse_amd import _lib
    lib = _lib.load()
    out = [ctypes.c_int64(-7) for _ in range(4)]
    refs = [ctypes.byref(o) for o in out]
    assert lib.avse_slide_counts(None, 1, -1, 0, 0, *refs) == INVALID
    assert lib.avse_slide_counts(None, 1, 0, -1, 0, *refs) == INVALID
    assert lib.avse_slide_counts(None, 0, 100, 5, 0, *refs) == INVALID and b"stride" in lib.avse_last_error()
    assert lib.avse_slide_counts(None, 6, 100, 5, 0, *refs) == INVALID and b"stride" in lib.avse_last_error()
    assert lib.avse_slide_counts(None, 1, 3201, 5, 1, *refs) == INVALID and b"flush" in lib.avse_last_error()
    assert lib.avse_slide_counts_geom(640, 160, 20, 6, 1, 0, 0, 0, *refs) == INVALID       # 20 % 6
    assert all(o.value == -7 for o in out)                       # no refused call wrote a count
    assert lib.avse_slide_counts(None, 1, 3200, 5, 1, *refs) == 0 and [o.value for o in out] == [20, 1, 20, 3040]
    assert lib.avse_slide_counts(None, 1, 3200, 5, 0, None, None, None, None) == 0         # every output is optional


def test_null_and_negative_arguments_are_rejected_without_gpu_work():
    from avse_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    host = np.zeros(4, np.int64)
    h = ctypes.c_void_p(host.ctypes.data)
    cnt = np.zeros(4, np.int64)
    c = ctypes.c_void_p(cnt.ctypes.data)
    out = ctypes.c_void_p()

    def create(ctx, w, ref, n_streams=2, stride=1, max_windows=8, vdt=0, sr=16000, n_fft=640, hop=160, spf=20):
        return lib.avse_slide_create(ctx, w, n_streams, sr, n_fft, hop, spf, stride, 80, 0.0, 8000.0, 1e-5, 80.0, vdt,
                                     max_windows, ref)
    for ctx, w, ref in ((None, p, ctypes.byref(out)), (p, None, ctypes.byref(out)), (p, p, None)):
        assert create(ctx, w, ref) == INVALID and b"NULL" in lib.avse_last_error()
    # bad extents with non-NULL pointers that are never read: refused first
    for kw in (dict(n_streams=0), dict(n_streams=-1), dict(max_windows=0), dict(max_windows=-3), dict(vdt=7),
               dict(stride=0), dict(stride=-2)):
        assert create(p, p, ctypes.byref(out), **kw) == INVALID and lib.avse_last_error(), kw
    # geometries no kernel serves are refused before the weights are read too
    assert create(p, p, ctypes.byref(out), n_fft=533, hop=133, spf=24) == UNSUPPORTED
    assert create(p, p, ctypes.byref(out), n_fft=800, hop=200, spf=24) == UNSUPPORTED     # 800 / 200 at 16 kHz
    assert not out.value

    def push(s, n_new, f_new, n_out, stride=16, vm=None, vs=None):
        return lib.avse_slide_push_each(s, p, h, n_new, p, f_new, None, vm, vs, p, stride, n_out, None, None, None, None)
    assert push(None, h, h, c) == INVALID and b"NULL" in lib.avse_last_error()
    assert push(p, None, h, c) == INVALID and b"NULL" in lib.avse_last_error()
    assert push(p, h, None, c) == INVALID and b"NULL" in lib.avse_last_error()
    assert push(p, h, h, None) == INVALID and b"NULL" in lib.avse_last_error()
    assert push(p, h, h, c, stride=-1) == INVALID and lib.avse_last_error()
    assert push(p, h, h, c, vm=p) == INVALID and push(p, h, h, c, vs=p) == INVALID      # half a normaliser
    assert lib.avse_slide_reset_each(None, h, None) == INVALID and b"NULL" in lib.avse_last_error()
    assert lib.avse_slide_reset_each(p, None, None) == INVALID and b"NULL" in lib.avse_last_error()
    assert lib.avse_slide_reset(None, None) == INVALID
    assert lib.avse_slide_state(None, h, h, None) == INVALID and b"NULL" in lib.avse_last_error()
    assert not cnt.any()                          # no refused call wrote a count
    lib.avse_slide_destroy(None)                  # a NULL session is a no-op


def test_python_bindings_check_their_arguments_on_the_host():
    from avse_amd import _lib, ops, pipeline
    with pytest.raises(TypeError):
        ops.slide_create(object(), 2)            # weights must be DeviceWeights
    with pytest.raises(_lib.AvseError, match="status 1"):
        ops.slide_counts(-5, 0)
    for kw in (dict(input_rate=44100), dict(input_fps=30)):
        with pytest.raises(ValueError, match="not built around a sliding session"):
            pipeline.SlidingStreamEnhancer(object(), 1, **kw)


def test_slide_geometry_sanitized(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host sources are built with the kernels' compiler")
    exe = str(tmp_path / "slide_geom_check")
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++20", "-O2", "-g", "-ffp-contract=off",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                         os.path.join(ROOT, "tests", "native", "slide_geom_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"exit status {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100000
