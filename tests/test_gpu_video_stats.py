"""VideoNormalizer's fit on the device (avse_video_stats, ops.video_stats, VideoNormalizer.fit_device) against numpy in
float64: np.mean(v.astype(np.float64), axis=(0, 3)) and the matching np.std, rounded to float32.

Bound: 2 float32 ulps.  The kernel accumulates in float64 about each pixel's first value, so its accumulation error is
far below a float32 ulp; what remains is the final rounding to float32 (and the square root's, for std)."""
import numpy as np
import pytest
import torch

from conftest import synth_video

pytestmark = pytest.mark.gpu

MAX_ULPS = 2


def reference_normalize(video, mean, std):
    """data_processor.py:208-212, restated loop for loop (float32 numpy, in place on a copy)."""
    v = np.array(video, dtype=np.float32, copy=True)
    for s in range(v.shape[0]):
        for f in range(v.shape[3]):
            v[s, :, :, f] -= mean
            v[s, :, :, f] /= std
    return v


def ulps(a, b):
    """Distance of two float32 arrays in units in the last place (ordered-integer view)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def yardstick(v):
    v64 = v.astype(np.float64)
    return np.mean(v64, axis=(0, 3)).astype(np.float32), np.std(v64, axis=(0, 3)).astype(np.float32)


def device_stats(v, gpu):
    from avse_amd import ops
    mean, std = ops.video_stats(torch.from_numpy(v).to(gpu))
    assert mean.dtype == std.dtype == torch.float32 and tuple(mean.shape) == tuple(std.shape) == v.shape[1:3]
    return mean.cpu().numpy(), std.cpu().numpy()


def check(v, gpu):
    mean, std = device_stats(v, gpu)
    ref_mean, ref_std = yardstick(v)
    um, us = ulps(mean, ref_mean), ulps(std, ref_std)
    print("shape %s: max ulps mean %d std %d" % (v.shape, um.max(), us.max()))
    assert um.max() <= MAX_ULPS, (um.max(), np.unravel_index(um.argmax(), um.shape))
    assert us.max() <= MAX_ULPS, (us.max(), np.unravel_index(us.argmax(), us.shape))
    return mean, std


# 4099 slices: 32 chunks of 129 slices with a ragged last one of 100; (5, 6, 10, 1) and (2, 3, 7, 4): one partial pixel
# tile, spans of 60 and 84 floats
@pytest.mark.parametrize("shape", [(1, 128, 128, 5), (3, 128, 128, 6), (37, 128, 128, 5), (4099, 8, 8, 5),
                                   (5, 6, 10, 1), (2, 3, 7, 4)])
def test_moments_within_two_ulps_of_float64_numpy(gpu, shape):
    S, H, W, F = shape
    v = synth_video(np.random.default_rng(S + 7 * F), S, h=H, w=W, f=F)
    check(v, gpu)


def test_unaligned_base_and_odd_span(gpu):
    """A span H W F that is no multiple of 4 floats, and a view whose first element is not 16-byte aligned: the
    element-wise loader."""
    from avse_amd import ops
    v = synth_video(np.random.default_rng(2), 9, h=5, w=7, f=3)
    check(v, gpu)
    w = synth_video(np.random.default_rng(3), 4, h=8, w=8, f=5)
    buf = torch.empty(w.size + 1, dtype=torch.float32, device=gpu)
    t = buf[1:].view(w.shape)
    t.copy_(torch.from_numpy(w))
    assert t.data_ptr() % 16 != 0
    mean, std = ops.video_stats(t)
    ref_mean, ref_std = yardstick(w)
    assert ulps(mean.cpu().numpy(), ref_mean).max() <= MAX_ULPS and ulps(std.cpu().numpy(), ref_std).max() <= MAX_ULPS


def test_constant_pixel_and_small_spread_about_a_large_mean(gpu):
    rng = np.random.default_rng(1)
    v = synth_video(rng, 41)
    v[:, 3, 4, :] = np.float32(0.1)          # not exactly summable in float32: the pivot shift makes every d zero
    v[:, 5, 6, :] = (200.0 + rng.uniform(-1e-2, 1e-2, (41, 5))).astype(np.float32)   # fails without the pivot shift
    mean, std = check(v, gpu)
    assert std[3, 4] == 0.0 and mean[3, 4] == np.float32(0.1)
    assert 1e-3 < std[5, 6] < 1e-2


def test_two_calls_are_bit_equal(gpu):
    from avse_amd import ops
    v = torch.from_numpy(synth_video(np.random.default_rng(4), 300, h=16, w=16)).to(gpu)
    a, b = ops.video_stats(v), ops.video_stats(v)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_fit_device_then_normalize_equals_the_reference_loop(gpu):
    from avse_amd.data_processor import VideoNormalizer
    rng = np.random.default_rng(6)
    video, other = synth_video(rng, 11), synth_video(rng, 4)
    norm = VideoNormalizer.fit_device(torch.from_numpy(video).to(gpu))
    assert norm.mean_image.dtype == norm.std_image.dtype == np.float32 and norm.mean_image.shape == (128, 128)
    ref_mean, ref_std = yardstick(video)
    assert ulps(norm.mean_image, ref_mean).max() <= MAX_ULPS and ulps(norm.std_image, ref_std).max() <= MAX_ULPS
    t2 = torch.from_numpy(other.copy()).to(gpu)
    norm.normalize(t2)
    np.testing.assert_array_equal(t2.cpu().numpy(), reference_normalize(other, norm.mean_image, norm.std_image))
