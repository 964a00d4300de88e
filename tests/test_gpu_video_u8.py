"""uint8 video end to end (include/avse.h AVSE_VIDEO_U8): forward, checked forward, normaliser fit, training step and
fit, pipeline and CLI.  float32(uint8) is exact and the kernels convert on load, so every output of a uint8 run must
equal the float32 run on the same pixel values BIT FOR BIT; one independent check against the float64 oracle (and the
float path's own oracle tests) shows that the two paths are not wrong alike.

Pixel values are seeded random bytes; every case holds 0 and 255, and the first and last pixel of the first and last
clip are 255, so a dropped leading or trailing byte is visible."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import keras_ref as K

pytestmark = pytest.mark.gpu

DTYPES = ("float32_split", "float32", "bfloat16")


def u8_video(seed, n, f=5):
    v = np.random.default_rng(seed).integers(0, 256, (n, 128, 128, f), dtype=np.uint8)
    v[0, 0, 1, 0], v[-1, -1, -2, -1] = 0, 0
    for c in (0, -1):
        v[c, 0, 0, :] = 255
        v[c, -1, -1, :] = 255
    assert v.min() == 0 and v.max() == 255
    return v


def mel_batch(seed, n, t=20):
    return np.random.default_rng(seed).normal(-40, 12, (n, 80, t)).astype(np.float32)


def normaliser(seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(90, 160, (128, 128)).astype(np.float32), rng.uniform(40, 90, (128, 128)).astype(np.float32))


def pipeline_batches():
    """Batch sizes for the persistent v_conv1 kernels (one workgroup per CU, a multiple of 8; 64 tiles of 16 x 16 per
    clip), from the device's CU count.  N3: every workgroup takes at least three tiles and some a fourth, so the
    two-ahead window pipeline runs with both parities of the last tile — 3 * workgroups / 64 + 1 = 13 on 256 CUs.
    N5: every workgroup takes at least five, the first count at which a register set freed by a window store is
    loaded again (window k + 4) — 21 on 256 CUs."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    wgs = ncu // 8 * 8 if ncu >= 8 else ncu
    return -(-3 * wgs // 64) + 1, -(-5 * wgs // 64) + 1


_models = {}


def weights(dtype, T=20, F=5):
    from avse_amd import ops
    from avse_amd.model import KerasModel
    key = (dtype, T, F)
    if key not in _models:
        model = KerasModel.init(seed=11, randomize=True, audio_shape=(80, T), video_shape=(128, 128, F))
        _models[key] = (model, ops.DeviceWeights(model, dtype))
    return _models[key]


def both(dw, mel, v8, norm, **kw):
    """forward(u8) and forward(u8.float()) on the same device tensors."""
    from avse_amd import ops
    m, s = norm if norm is not None else (None, None)
    a = ops.forward(dw, mel, v8, m, s, **kw)
    b = ops.forward(dw, mel, v8.float(), m, s, **kw)
    return a, b


# ---- 1. forward, bitwise ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,F", [(20, 5), (24, 6)])
@pytest.mark.parametrize("fused_norm", [False, True])
def test_forward_u8_equals_float_bitwise(gpu, dtype, T, F, fused_norm):
    """N = 1 and the two sizes of pipeline_batches() (the larger N for the split and bf16 dtypes only: their v_conv1
    kernels are the persistent ones; exact fp32 runs the element-wise prep kernel, which has no tile pipeline)."""
    _, dw = weights(dtype, T, F)
    norm = tuple(torch.from_numpy(a).to(gpu) for a in normaliser(3)) if fused_norm else None
    for N in (1,) if dtype == "float32" else (1,) + pipeline_batches():
        mel = torch.from_numpy(mel_batch(N, N, T)).to(gpu)
        v8 = torch.from_numpy(u8_video(10 * N + F, N, F)).to(gpu)
        a, b = both(dw, mel, v8, norm)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (dtype, F, N, float((a - b).abs().max()))


@pytest.mark.parametrize("fused_norm", [False, True])
def test_forward_u8_split_v1s_at_five_frames(gpu, fused_norm):
    """Context option no_v1p: the 5-frame split v_conv1 on k_conv_v1s (K 160) instead of k_conv_v1p."""
    from avse_amd import _lib, ops
    from avse_amd.model import KerasModel
    norm = tuple(torch.from_numpy(a).to(gpu) for a in normaliser(4)) if fused_norm else None
    with _lib.context().options(no_v1p=1):
        dw = ops.DeviceWeights(KerasModel.init(seed=11, randomize=True), "float32_split")   # applies at load time
        for N in (1,) + pipeline_batches():
            mel = torch.from_numpy(mel_batch(N, N)).to(gpu)
            v8 = torch.from_numpy(u8_video(77 + N, N)).to(gpu)
            a, b = both(dw, mel, v8, norm)
            assert torch.equal(a, b), N


# ---- 2. independent check ---------------------------------------------------------------------
def test_forward_u8_matches_the_float64_oracle(gpu):
    """Split dtype, N = 2, fused normaliser, against oracle.keras_ref.forward on the float64 pixel values: the
    absolute-RMS bound of tests/test_gpu_split.py (FP32_ABS = 1e-4, tests/test_gpu_forward.py:22, as asserted at
    tests/test_gpu_split.py:129) and its relative bound FP32_REL."""
    from test_gpu_forward import FP32_ABS, FP32_REL, abs_rms, rel_rms
    from avse_amd import ops
    model, dw = weights("float32_split")
    mel, v8 = mel_batch(5, 2), u8_video(6, 2)
    mean, std = normaliser(7)
    vref = (v8.astype(np.float64) - mean[None, :, :, None].astype(np.float64)) / std[None, :, :, None].astype(np.float64)
    ref = K.forward(model.layer_dict(), mel, vref)
    got = ops.forward(dw, torch.from_numpy(mel).to(gpu), torch.from_numpy(v8).to(gpu), torch.from_numpy(mean).to(gpu),
                      torch.from_numpy(std).to(gpu)).cpu().numpy()
    print(f"u8 split vs float64 oracle: abs RMS {abs_rms(got, ref):.3e}, rel {rel_rms(got, ref):.3e}")
    assert abs_rms(got, ref) <= FP32_ABS and rel_rms(got, ref) <= FP32_REL


# ---- 3. checked forward and guard -------------------------------------------------------------
def test_checked_forward_u8_recomputes_and_reports_like_float(gpu):
    """A std image with one entry of 1e-6: that pixel's normalised values leave the f16 pair range.  The checked u8
    forward returns the exact-fp32 forward of the same input bit for bit, and the guard bits (checked and unchecked)
    equal the float-input run's."""
    import warnings
    from avse_amd import _lib, ops
    _, dw = weights("float32_split")
    _, dw32 = weights("float32")
    mean, std = normaliser(8)
    std[64, 64] = 1e-6
    m, s = torch.from_numpy(mean).to(gpu), torch.from_numpy(std).to(gpu)
    mel = torch.from_numpy(mel_batch(9, 2)).to(gpu)
    v8 = torch.from_numpy(u8_video(12, 2)).to(gpu)
    vf = v8.float()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got8 = ops.forward(dw, mel, v8, m, s, checked=True)
        bits8 = dw.last_range_bits
        gotf = ops.forward(dw, mel, vf, m, s, checked=True)
        bitsf = dw.last_range_bits
    exact8, exactf = ops.forward(dw32, mel, v8, m, s), ops.forward(dw32, mel, vf, m, s)
    assert bits8 >> 25 & 1 and bits8 == bitsf, (hex(bits8), hex(bitsf))
    assert torch.equal(got8, exact8) and torch.equal(exact8, exactf) and torch.equal(got8, gotf)
    ctx = _lib.context()
    ctx.range_status()
    ops.forward(dw, mel, v8, m, s)
    st8 = ctx.range_status()
    ops.forward(dw, mel, vf, m, s)
    stf = ctx.range_status()
    assert st8 >> 25 & 1 and st8 == stf, (hex(st8), hex(stf))


# ---- 4. normaliser fit ------------------------------------------------------------------------
@pytest.mark.parametrize("S,F", [(3, 5), (7, 6), (1, 5)])
def test_video_stats_u8_within_two_ulps_and_repeatable(gpu, S, F):
    """The bound of tests/test_gpu_video_stats.py: 2 float32 ulps from numpy's float64 mean / std over axes (0, 3)."""
    from test_gpu_video_stats import MAX_ULPS, ulps, yardstick
    from avse_amd import ops
    v = u8_video(20 + S, S, F)
    t = torch.from_numpy(v).to(gpu)
    mean, std = ops.video_stats(t)
    again = ops.video_stats(t)
    assert mean.dtype == std.dtype == torch.float32 and tuple(mean.shape) == (128, 128)
    ref_mean, ref_std = yardstick(v)
    um, us = ulps(mean.cpu().numpy(), ref_mean).max(), ulps(std.cpu().numpy(), ref_std).max()
    print(f"u8 stats S={S} F={F}: max ulps mean {um} std {us}")
    assert um <= MAX_ULPS and us <= MAX_ULPS
    assert torch.equal(mean, again[0]) and torch.equal(std, again[1])


def test_fit_device_u8_agrees_with_the_host_fit(gpu):
    from test_gpu_video_stats import MAX_ULPS, ulps
    from avse_amd.data_processor import VideoNormalizer
    v = u8_video(31, 5)
    dev, host = VideoNormalizer.fit_device(torch.from_numpy(v).to(gpu)), VideoNormalizer(v)
    assert host.mean_image.dtype == host.std_image.dtype == np.float32
    assert ulps(dev.mean_image, host.mean_image).max() <= MAX_ULPS
    assert ulps(dev.std_image, host.std_image).max() <= MAX_ULPS
    with pytest.raises(TypeError, match="fused"):
        host.normalize(v)
    with pytest.raises(TypeError, match="fused"):
        host.normalize(torch.from_numpy(v).to(gpu))


# ---- 5. training ------------------------------------------------------------------------------
def train_batch(seed, n):
    mel = mel_batch(seed, n)
    target = (mel + np.random.default_rng(seed + 1).normal(0, 3, mel.shape)).astype(np.float32)
    return mel, u8_video(seed + 2, n), target


def test_trainer_step_u8_equals_float_bitwise(gpu):
    """Batch 2: a gradients-only step, then one full Adam step; loss, every gradient and the updated parameters."""
    from avse_amd import ops
    from avse_amd.model import KerasModel
    model = KerasModel.init(seed=21, randomize=True)
    mel, v8, target = train_batch(40, 2)
    m, s = (torch.from_numpy(a).to(gpu) for a in normaliser(41))
    a, tgt, v8d = torch.from_numpy(mel).to(gpu), torch.from_numpy(target).to(gpu), torch.from_numpy(v8).to(gpu)
    res = {}
    for name, video in (("u8", v8d), ("f32", v8d.float())):
        tr = ops.Trainer(model, max_batch=2, device=gpu)
        l0 = tr.step(a, video, tgt, m, s, dropout=0.25, seed=7, grads_only=True).item()
        g0 = tr.gradients()
        l1 = tr.step(a, video, tgt, m, s, dropout=0.25, seed=8).item()
        res[name] = (l0, g0, l1, tr.gradients(), tr.model().to_blob())
        del tr
    u, f = res["u8"], res["f32"]
    assert np.isfinite(u[0]) and u[0] == f[0] and u[2] == f[2]
    for gu, gf in ((u[1], f[1]), (u[3], f[3])):
        assert gu.keys() == gf.keys()
        for k in gu:
            assert np.array_equal(gu[k], gf[k]), k
    assert np.array_equal(u[4], f[4])


def test_fit_u8_with_normaliser_follows_the_prenormalised_float_fit(gpu):
    """2 epochs on 4 slices: fit(u8 set, normalizer=...) against fit on the float set normalised in place beforehand.
    Tolerance: the relative 1e-3 tests/test_gpu_train.py holds loss trajectories to (test_adam_steps_match_oracle).
    Measured on an MI355X: 0 (both paths divide by std: train.hip k_prep_video, conv.hip k_video_normalize; the
    validation forward's fused normaliser in the exact-fp32 k_video_prep divides too)."""
    from avse_amd.data_processor import VideoNormalizer
    from avse_amd.fit import fit
    from avse_amd.model import KerasModel
    mel, v8, target = train_batch(50, 4)
    norm = VideoNormalizer(v8)
    vf = v8.astype(np.float32)
    norm.normalize(vf)
    _, h8 = fit(KerasModel.init(seed=5), (mel, v8, target), (mel, v8, target), batch_size=2, epochs=2, seed=3,
                device=gpu, verbose=0, normalizer=norm)
    _, hf = fit(KerasModel.init(seed=5), (mel, vf, target), (mel, vf, target), batch_size=2, epochs=2, seed=3,
                device=gpu, verbose=0)
    a8 = np.array([[h["loss"], h["val_loss"]] for h in h8])
    af = np.array([[h["loss"], h["val_loss"]] for h in hf])
    print("fit u8 vs float: max relative difference of loss / val_loss %.3e" % np.max(np.abs(a8 - af) / np.abs(af)))
    assert len(h8) == 2
    np.testing.assert_allclose(a8, af, rtol=1e-3)


# ---- 6. alignment and arguments ---------------------------------------------------------------
def test_u8_alignment_and_argument_errors(gpu):
    from avse_amd import _lib, ops
    _, dw = weights("float32_split")
    mel = torch.from_numpy(mel_batch(60, 2)).to(gpu)
    v8 = torch.from_numpy(u8_video(61, 2)).to(gpu)
    buf = torch.empty(v8.numel() + 4, dtype=torch.uint8, device=gpu)
    off = buf[1:1 + v8.numel()].view(v8.shape)
    off.copy_(v8)
    assert off.is_contiguous() and off.data_ptr() % 4 == 1
    with pytest.raises(ValueError, match="align"):
        ops.forward(dw, mel, off)
    assert b"align" in _lib.load().avse_last_error()
    with pytest.raises(ValueError, match="align"):
        ops.video_stats(off)
    tr = ops.Trainer(weights("float32")[0], max_batch=2, device=gpu)
    with pytest.raises(ValueError, match="align"):
        tr.step(mel, off, mel)
    # refused as the float path refuses them: wrong F, a non-contiguous view, mismatched N
    v6 = torch.zeros((2, 128, 128, 6), dtype=torch.uint8, device=gpu)
    f6 = v6.float()
    for bad, bad_float in ((v6, f6), (v6[..., :5], f6[..., :5]), (v8[:1], v8[:1].float())):
        assert bad_float.stride() == bad.stride()
        with pytest.raises(ValueError):
            ops.forward(dw, mel, bad)
        with pytest.raises(ValueError):
            ops.forward(dw, mel, bad_float)
    with pytest.raises(TypeError):
        ops.forward(dw, mel, v8.to(torch.int16))
    with pytest.raises(TypeError):
        ops.forward(dw, mel, v8.cpu())


@pytest.mark.parametrize("first", ["u8", "f32"])
def test_graph_cache_keeps_u8_and_float_forwards_apart(gpu, first):
    """Option graph: a float forward and a u8 forward at the same N on one context, in both orders, three calls each
    (direct, capture, replay), still match their solo runs — first with two tensors, then with a u8 view of the float
    tensor's own storage: one address and one N, so only the dtype in the cache key tells the two graphs apart."""
    from avse_amd import _lib, ops
    _, dw = weights("float32_split")
    mel = torch.from_numpy(mel_batch(70, 2)).to(gpu)
    v8 = torch.from_numpy(u8_video(71, 2)).to(gpu)
    vf = v8.float()
    solo = ops.forward(dw, mel, vf).clone()
    out = torch.empty_like(solo)
    with _lib.context().options(graph=1):
        order = (v8, vf) if first == "u8" else (vf, v8)
        for _ in range(3):
            for v in order:
                out.zero_()
                ops.forward(dw, mel, v, out=out)
                assert torch.equal(out, solo), v.dtype
    # the same buffer reinterpreted: one address, two dtypes, N clips of u8 inside the float tensor's storage
    alias = vf.view(torch.uint8).view(-1)[:v8.numel()].view(v8.shape)
    alias_solo = ops.forward(dw, mel, alias).clone()
    with _lib.context().options(graph=1):
        for _ in range(3):
            for v, want in ((vf, solo), (alias, alias_solo)) if first == "f32" else ((alias, alias_solo), (vf, solo)):
                out.zero_()
                ops.forward(dw, mel, v, out=out)
                assert torch.equal(out, want), v.dtype


# ---- 7. pipeline and CLI ----------------------------------------------------------------------
def test_enhancer_u8_equals_float_bitwise(gpu):
    from conftest import synth_audio
    from avse_amd import ops
    from avse_amd.pipeline import Enhancer
    _, dw = weights("float32_split")
    sig = torch.from_numpy(synth_audio(np.random.default_rng(80), 2, 3 * 3200)).to(gpu)
    v8 = torch.from_numpy(u8_video(81, 6).reshape(2, 3, 128, 128, 5)).to(gpu)
    m, s = (torch.from_numpy(a).to(gpu) for a in normaliser(82))
    enh = Enhancer(dw)
    a, b = enh(sig, v8, m, s), enh(sig, v8.float(), m, s)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_network_predict_and_evaluate_take_numpy_uint8(gpu):
    """The reference-shaped API on numpy arrays: predict / evaluate of uint8 crops with the normaliser fused equal the
    float32 calls (the per-sample path of the CLI's predict)."""
    from avse_amd.data_processor import VideoNormalizer
    from avse_amd.network import SpeechEnhancementNetwork
    model, _ = weights("float32_split")
    net = SpeechEnhancementNetwork(model, "float32_split")
    mel, v8 = mel_batch(90, 3), u8_video(91, 3)
    norm = VideoNormalizer(v8)
    vf = v8.astype(np.float32)
    a, b = net.predict(mel, v8, norm), net.predict(mel, vf, norm)
    assert a.shape == (3, 80, 20) and np.array_equal(a, b)
    assert net.evaluate(mel, v8, mel, norm) == net.evaluate(mel, vf, mel, norm)
    pa, la = net.predict_and_evaluate(mel, torch.from_numpy(v8).to(gpu), mel, norm)
    assert np.array_equal(pa, a) and la == net.evaluate(mel, vf, mel, norm)


def test_cli_u8_cache_predicts_the_float_cache_wavs(gpu, tmp_path):
    """preprocess --video-u8 -> predict writes enhanced.wav files byte-equal to the float-cache run's (same model and
    normaliser, fitted once on the float cache)."""
    from test_gpu_cli import make_dataset, run
    tmp = str(tmp_path)
    ds, noise = make_dataset(tmp, n_noise=2)
    base = os.path.join(tmp, "base")
    os.makedirs(base)
    pre = ["-bd", base, "preprocess", "-ds", ds, "-n", noise]
    # preprocess pairs clips with noises through the global random state: run it in this process, seeded, so that both
    # caches hold the same pairs; train and predict then run through the command line as in tests/test_gpu_cli.py
    import random
    from avse_amd import speech_enhancer as se
    from avse_amd.corpus import Layout
    for name, flag in (("f", []), ("u", ["--video-u8"])):
        random.seed(5)
        se.main(pre + ["-dn", name] + flag)
    sf = se.load_preprocessed_blob(Layout(base).preprocessed("f"))
    su = se.load_preprocessed_blob(Layout(base).preprocessed("u"))
    assert len(sf) == len(su) == 2
    assert [(a.video_file_path, a.noise_file_path) for a in sf] == [(a.video_file_path, a.noise_file_path) for a in su]
    assert all(s.video_samples.dtype == np.uint8 for s in su) and all(s.video_samples.dtype == np.float32 for s in sf)
    run(["-bd", base, "train", "-mn", "m", "-tdn", "f", "-vdn", "f", "--init-only"], tmp)
    wavs = {}
    for name in ("f", "u"):
        run(["-bd", base, "predict", "-mn", "m", "-dn", name], tmp)
        found = sorted(glob.glob(os.path.join(base, "out", "m", name, "*", "*", "*", "enhanced.wav")))
        assert len(found) == 2
        wavs[name] = {os.path.join(*w.split(os.sep)[-3:]): open(w, "rb").read() for w in found}
    assert wavs["f"].keys() == wavs["u"].keys()
    for k in wavs["f"]:
        assert wavs["f"][k] == wavs["u"][k], k
