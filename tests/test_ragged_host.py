"""CPU tests of the ragged STFT / ISTFT: what the C-ABI decides on the host (exports, every refusal of
avse_spectrogram_ragged / avse_istft_ragged before any GPU work) and the host geometry (csrc/ragged_geom.h) under
AddressSanitizer / UndefinedBehaviorSanitizer against a brute-force definition (a stand-alone program,
tests/native/ragged_geom_check.cpp)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-visual-speech-enhancement_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INVALID = 1


def test_library_exports_the_ragged_calls():
    from avse_amd import _lib
    lib = _lib.load()
    for f in ("avse_spectrogram_ragged", "avse_istft_ragged"):
        assert hasattr(lib, f) and f in _lib.SIGNATURES
    assert lib.avse_abi_version() == 3          # additive: the ABI version did not move
    with open(os.path.join(ROOT, "include", "avse.h")) as fh:
        header = fh.read()
    assert "int avse_spectrogram_ragged(" in header and "int avse_istft_ragged(" in header


def _i64(*v):
    return np.array(v, dtype=np.int64)


def _spec(lib, ctx, sig, off, lens, n_utt, mel, n_fft=640, hop=160, pad=0, spf=0):
    return lib.avse_spectrogram_ragged(ctx, sig, None if off is None else off.ctypes.data,
                                       None if lens is None else lens.ctypes.data, n_utt, 16000, n_fft, hop, 80, 0.0,
                                       8000.0, 1e-5, 80.0, pad, spf, mel, None, None)


def _istft(lib, ctx, mel, stft, nf, sf, n_utt, sig, spf=0):
    return lib.avse_istft_ragged(ctx, mel, stft, None if nf is None else nf.ctypes.data,
                                 None if sf is None else sf.ctypes.data, n_utt, spf, 16000, 640, 160, 80, 0.0, 8000.0,
                                 sig, None)


def test_spectrogram_ragged_refusals_need_no_gpu():
    """NULL arrays, a negative count, reflect padding on an utterance of at most n_fft / 2 samples and totals past int32
    items: AVSE_ERR_INVALID with a message, with a NULL context too, before the context or a buffer is touched."""
    from avse_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)        # stands for a context / a device buffer: never read
    off, lens = _i64(0, 3200), _i64(3200, 4000)
    assert _spec(lib, None, p, off, lens, 2, p) == INVALID and b"NULL" in lib.avse_last_error()
    for hole in ("sig", "off", "lens", "mel"):
        rc = _spec(lib, p, None if hole == "sig" else p, None if hole == "off" else off,
                   None if hole == "lens" else lens, 2, None if hole == "mel" else p)
        assert rc == INVALID and b"NULL" in lib.avse_last_error(), hole
    for ctx in (None, p):                         # the same answers with a NULL context
        assert _spec(lib, ctx, p, off, lens, -1, p) == INVALID and lib.avse_last_error()
        assert _spec(lib, ctx, p, off, _i64(3200, -5), 2, p) == INVALID and lib.avse_last_error()
        assert _spec(lib, ctx, p, off, _i64(3200, 0), 2, p) == INVALID and lib.avse_last_error()
        assert _spec(lib, ctx, p, off, lens, 2, p, spf=-1) == INVALID and lib.avse_last_error()
    rc = _spec(lib, p, p, off, _i64(3200, 320), 2, p, pad=0)              # AVSE_PAD_REFLECT = 0
    assert rc == INVALID and b"reflect" in lib.avse_last_error() and b"utterance 1" in lib.avse_last_error()
    rc = _spec(lib, p, p, off, _i64(3200, 1 << 31), 2, p, pad=1)
    assert rc == INVALID and b"too large" in lib.avse_last_error()
    # items past int32: 2^16 utterances of (2^31 - 1281) samples at hop 1 are 2^47 frames in chunks of 21
    n = 1 << 16
    rc = _spec(lib, p, p, np.zeros(n, np.int64), np.full(n, (1 << 31) - 1281, np.int64), n, p, hop=1, pad=1)
    assert rc == INVALID and b"too large" in lib.avse_last_error()
    assert _lib.AVSE_PAD_REFLECT == 0


def test_istft_ragged_refusals_need_no_gpu():
    from avse_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nf, sf = _i64(20, 40), _i64(21, 41)
    assert _istft(lib, None, p, p, nf, sf, 2, p) == INVALID and b"NULL" in lib.avse_last_error()
    for hole in ("mel", "stft", "nf", "sf", "sig"):
        rc = _istft(lib, p, None if hole == "mel" else p, None if hole == "stft" else p, None if hole == "nf" else nf,
                    None if hole == "sf" else sf, 2, None if hole == "sig" else p)
        assert rc == INVALID and b"NULL" in lib.avse_last_error(), hole
    assert _istft(lib, p, p, p, nf, sf, -2, p) == INVALID and lib.avse_last_error()
    assert _istft(lib, p, p, p, _i64(20, -1), sf, 2, p) == INVALID and lib.avse_last_error()
    rc = _istft(lib, p, p, p, _i64(20, 30), sf, 2, p, spf=20)              # 30 is no multiple of 20
    assert rc == INVALID and b"multiple" in lib.avse_last_error() and b"utterance 1" in lib.avse_last_error()
    rc = _istft(lib, p, p, p, _i64(20, 42), sf, 2, p)                      # more frames than the STFT holds
    assert rc == INVALID and b"stft_frames" in lib.avse_last_error()
    assert _istft(lib, p, p, p, nf, sf, 2, p, spf=-1) == INVALID
    big = _i64(1 << 40)
    assert _istft(lib, p, p, p, big, big, 1, p) == INVALID and b"too large" in lib.avse_last_error()


def test_ops_refuse_bad_ragged_arguments_on_the_host():
    import torch
    from avse_amd import ops
    with pytest.raises(TypeError):                  # host tensors: the transforms run on the device
        ops.spectrogram_ragged([torch.zeros(3200)])
    with pytest.raises(TypeError):
        ops.spectrogram_ragged((torch.zeros(6400), [0, 3200], [3200, 3200]))
    with pytest.raises(TypeError):
        ops.istft_ragged(torch.zeros(2, 80, 20), [1, 1], torch.zeros(10, 2), [21, 21])


def test_ragged_geometry_sanitized(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host sources are built with the kernels' compiler")
    exe = str(tmp_path / "ragged_geom_check")
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++20", "-O2", "-g", "-ffp-contract=off",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                         os.path.join(ROOT, "tests", "native", "ragged_geom_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"exit status {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 1000
