"""avse_forward_mixed (include/avse.h): one forward for a batch in which some clips have no video.

A clip without video is the all-zero normalised input, the input of ops.forward(video=None).  The float32 and
float32_split forwards are batch-invariant bit for bit (test_gpu_split.py test_fp32_forward_is_batch_invariant), so the
acceptance criterion is exact: out[i] has the bits of ops.forward(full video)[i] where the clip has video and of
ops.forward(video=None)[i] where it has not.  bfloat16 is held to the float64 oracle (zero normalised video for the
clips without) under the bound test_gpu_forward.py applies to the plain few-clip bf16 forward.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import keras_ref as K
from oracle import librosa_ref as R
from test_gpu_forward import BF16_REL, make_inputs, rel_rms

pytestmark = pytest.mark.gpu

SPLIT = "float32_split"
MASK7 = np.array([1, 0, 0, 1, 1, 0, 1], bool)      # first and last rows, consecutive blanks


def _mask37():
    """19 of 37 present (odd M; tile boundaries of the 4- and 8-clip tiles fall inside runs of either kind)"""
    m = np.zeros(37, bool)
    m[np.random.default_rng(37).permutation(37)[:19]] = True
    return m


MASKS = {7: MASK7, 37: _mask37()}


@functools.lru_cache(maxsize=None)
def _case(N):
    """Inputs of one batch size, shared by every test (never written to): mel, whole-number video, normaliser."""
    mel, video = make_inputs(N, 400 + N)
    mean, std = R.video_normalizer_fit(video)
    return mel, video, mean, std


@functools.lru_cache(maxsize=None)
def _model(seed=31):
    from avse_amd.model import KerasModel
    return KerasModel.init(seed=seed, randomize=True)


@functools.lru_cache(maxsize=None)
def _oracle(N, normalize):
    """float64 oracle of the mixed batch: zero normalised video for the clips without video"""
    mel, video, mean, std = _case(N)
    vn = R.video_normalize(video, mean, std).astype(np.float32) if normalize else video.copy()
    vn[~MASKS[N]] = 0
    return K.forward(_model().layer_dict(), mel, vn)


def _dev_video(video, u8):
    from avse_amd import ops
    return ops.video_to_device(video.astype(np.uint8)) if u8 else ops.to_device(video)


def _mixed(dw, N, mask, u8, normalize, **kw):
    from avse_amd import ops
    mel, video, mean, std = _case(N)
    norm = [ops.to_device(mean), ops.to_device(std)] if normalize else []
    packed = _dev_video(np.ascontiguousarray(video[mask]), u8) if mask.any() else None
    return ops.forward(dw, ops.to_device(mel), packed, *norm, video_present=mask, **kw).cpu().numpy()


def _alone(dw, N, u8, normalize):
    """What every clip gets on its own: (forward(full video), forward(video=None))"""
    from avse_amd import ops
    mel, video, mean, std = _case(N)
    norm = [ops.to_device(mean), ops.to_device(std)] if normalize else []
    full = ops.forward(dw, ops.to_device(mel), _dev_video(video, u8), *norm).cpu().numpy()
    none = ops.forward(dw, ops.to_device(mel), None).cpu().numpy()
    return full, none


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("N", [7, 37])
@pytest.mark.parametrize("dtype", ["float32", SPLIT])
def test_every_clip_has_the_bits_of_its_own_call(gpu, dtype, N, u8, normalize):
    from avse_amd import ops
    dw = ops.DeviceWeights(_model(), dtype)
    mask = MASKS[N]
    full, none = _alone(dw, N, u8, normalize)
    got = _mixed(dw, N, mask, u8, normalize)
    assert not np.array_equal(full[~mask], none[~mask])      # the video matters: the two references differ
    assert np.array_equal(got[mask], full[mask])
    assert np.array_equal(got[~mask], none[~mask])
    # a second call (the next slot of the row-map ring) with the complementary mask
    got = _mixed(dw, N, ~mask, u8, normalize)
    assert np.array_equal(got[~mask], full[~mask]) and np.array_equal(got[mask], none[mask])


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("N", [7, 37])
def test_bf16_mixed_matches_oracle(gpu, N, u8, normalize):
    from avse_amd import ops
    dw = ops.DeviceWeights(_model(), "bfloat16")
    got = _mixed(dw, N, MASKS[N], u8, normalize)
    ref = _oracle(N, normalize)
    err = rel_rms(got, ref)
    blank = rel_rms(got[~MASKS[N]], ref[~MASKS[N]])
    print(f"bf16 mixed N={N} u8={u8} normalize={normalize}: rel RMS {err:.3e} (clips without video {blank:.3e})")
    assert np.isfinite(got).all()
    assert err <= BF16_REL and blank <= BF16_REL


@pytest.mark.parametrize("dtype", ["float32", SPLIT, "bfloat16"])
def test_degenerate_masks(gpu, dtype):
    """All present is the plain forward, none present (a normaliser given) the video=None forward, launch for launch;
    M = 1 of N = 6 is the smallest packed encoder batch."""
    from avse_amd import ops
    dw = ops.DeviceWeights(_model(), dtype)
    mel7, video7, mean, std = _case(7)
    m, s = ops.to_device(mean), ops.to_device(std)
    mel, video = ops.to_device(mel7[:5]), ops.to_device(np.ascontiguousarray(video7[:5]))
    full = ops.forward(dw, mel, video, m, s).cpu().numpy()
    none = ops.forward(dw, mel, None).cpu().numpy()
    assert np.array_equal(ops.forward(dw, mel, video, m, s, video_present=[True] * 5).cpu().numpy(), full)
    assert np.array_equal(ops.forward(dw, mel, None, m, s, video_present=np.zeros(5, bool)).cpu().numpy(), none)
    mel6 = ops.to_device(mel7[:6])
    mask = np.array([0, 0, 0, 0, 1, 0], bool)
    got = ops.forward(dw, mel6, ops.to_device(np.ascontiguousarray(video7[4:5])), m, s, video_present=mask).cpu().numpy()
    if dtype == "bfloat16":
        vn = R.video_normalize(video7[:6], mean, std).astype(np.float32)
        vn[~mask] = 0
        assert rel_rms(got, K.forward(_model().layer_dict(), mel7[:6], vn)) <= BF16_REL
    else:
        full6 = ops.forward(dw, mel6, ops.to_device(np.ascontiguousarray(video7[:6])), m, s).cpu().numpy()
        none6 = ops.forward(dw, mel6, None).cpu().numpy()
        assert np.array_equal(got[4], full6[4]) and np.array_equal(got[~mask], none6[~mask])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_first_call_on_fresh_weights_is_mixed(gpu, dtype):
    """The constant embedding is computed by the first call that needs it, in the N = 1 arena layout: with the
    per-layer audio branch on the side stream (no_audenc) it must be done before that branch is launched (the race of
    test_gpu_framerates.py test_zero_video_with_layer_by_layer_audio_branch)."""
    from avse_amd import ops
    mel7, video7, _, _ = _case(7)
    mel, video = mel7[:6], np.ascontiguousarray(video7[:6])
    mask = np.array([0, 1, 0, 0, 1, 1], bool)
    ctx = ops.DeviceWeights(_model(), dtype).ctx
    with ctx.options(no_audenc=1):
        dw = ops.DeviceWeights(_model(), dtype)
        got = ops.forward(dw, ops.to_device(mel), ops.to_device(np.ascontiguousarray(video[mask])),
                          video_present=mask).cpu().numpy()
        if dtype == "float32":
            other = ops.DeviceWeights(_model(), dtype)
            full = ops.forward(other, ops.to_device(mel), ops.to_device(video)).cpu().numpy()
            none = ops.forward(other, ops.to_device(mel), None).cpu().numpy()
    if dtype == "float32":
        assert np.array_equal(got[mask], full[mask]) and np.array_equal(got[~mask], none[~mask])
    else:
        vz = video.copy()
        vz[~mask] = 0
        assert rel_rms(got, K.forward(_model().layer_dict(), mel, vz)) <= BF16_REL


def test_checked_mixed_call_recomputes_on_exact_fp32(gpu):
    """A present clip whose input leaves the f16 pair range (test_gpu_range.py test_input_overflow_is_recomputed: video
    x 1000): the checked mixed forward reports the video input and returns the mixed forward of float32 weights."""
    from avse_amd import _lib, ops
    mel7, video7, _, _ = _case(7)
    mask = np.array([1, 0, 1, 1, 0], bool)
    mel = ops.to_device(mel7[:5])
    packed = np.ascontiguousarray(video7[:5][mask])
    packed[1] *= 1000.0
    packed = ops.to_device(packed)
    f32 = ops.forward(ops.DeviceWeights(_model(), "float32"), mel, packed, video_present=mask).cpu().numpy()
    dw = ops.DeviceWeights(_model(), SPLIT)
    with pytest.warns(RuntimeWarning):
        got = ops.forward(dw, mel, packed, video_present=mask, checked=True).cpu().numpy()
    assert dw.last_range_bits >> 25 & 1, hex(dw.last_range_bits)
    assert np.isfinite(got).all() and np.array_equal(got, f32)
    with pytest.raises(_lib.RangeError):
        ops.forward(dw, mel, packed, video_present=mask, checked=True, on_range="error")
    # in range: the checked call is the unchecked one
    ok = ops.to_device(np.ascontiguousarray(video7[:5][mask]))
    a = ops.forward(dw, mel, ok, video_present=mask, checked=True).cpu().numpy()
    assert dw.last_range_bits == 0
    assert np.array_equal(a, ops.forward(dw, mel, ok, video_present=mask).cpu().numpy())


def test_library_refuses_a_mask_without_its_video(gpu):
    """video == NULL while the mask marks a clip, and present == NULL: AVSE_ERR_INVALID with nothing enqueued, so the
    output buffer is untouched and a following plain forward gives what it gave before."""
    import torch
    from avse_amd import _lib, ops
    dw = ops.DeviceWeights(_model(), "float32")
    mel7, video7, _, _ = _case(7)
    mel, video = ops.to_device(mel7[:5]), ops.to_device(np.ascontiguousarray(video7[:5]))
    before = ops.forward(dw, mel, video).cpu().numpy()
    out = torch.full((5, 80, 20), 7.0, device=mel.device)
    present = np.array([0, 1, 0, 0, 0], np.uint8)
    lib = _lib.load()
    with torch.cuda.device(mel.device):
        st = _lib.stream_handle(mel.device)
        rc = lib.avse_forward_mixed(dw.ctx.handle, dw.handle, _lib.ptr(mel), None, 0, None, None,
                                    present.ctypes.data_as(ctypes.c_void_p), 5, _lib.ptr(out), st)
        assert rc == 1 and b"video == NULL" in lib.avse_last_error()
        rc = lib.avse_forward_mixed(dw.ctx.handle, dw.handle, _lib.ptr(mel), _lib.ptr(video), 0, None, None, None, 5,
                                    _lib.ptr(out), st)
        assert rc == 1 and b"present" in lib.avse_last_error()
        bits = ctypes.c_uint32(5)
        rc = lib.avse_forward_mixed_checked(dw.ctx.handle, dw.handle, _lib.ptr(mel), None, 0, None, None,
                                            present.ctypes.data_as(ctypes.c_void_p), 5, _lib.ptr(out), st, 0,
                                            ctypes.byref(bits))
        assert rc == 1 and bits.value == 0
    assert float(out.min()) == float(out.max()) == 7.0
    assert np.array_equal(ops.forward(dw, mel, video).cpu().numpy(), before)
