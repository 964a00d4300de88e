"""The inference forward on a model with negative and zero BatchNormalization gammas, in all three dtypes.

KerasModel.init(randomize=True) draws gamma ~ U(0.5, 1.5): with it the sign fold of weight_pack.cpp (a channel whose
folded scale is negative gets negated weights and |scale|, because conv_v1r.hip and conv_stream.hip pool the raw
accumulators and apply one FMA afterwards) is dead code on the device, and so are negative scales in the pooled
epilogues of k_conv and k_gemm<1>, in the fused per-clip kernels, in the split dtype's scale / scale_h / per-channel
exponents, and channel_exponents' all-zero channel.  forward_local_ref.signed_model negates gamma on channels 1::3,
zeroes it on 5::17 and zeroes one output channel's kernel in v_conv3 and a_conv3; a trained checkpoint may hold any of
these.  It stays an ordinary network (float64 oracle at N = 2, seed 3: every layer's RMS is 0.64 .. 1.04 x the unsigned
model's; v_conv1 43 against 45, the output 0.19 against 0.23), so the gates are the project's own, imported: FP32_REL / FP32_ABS on dB-scale outputs for float32 and
float32_split (every layer FP32_REL, last_range_bits == 0 on the checked split forwards), BF16_REL / BF16_LAYER_REL for
bf16.

Shapes: 25 fps at N = 5 (a ragged last 4-clip v_conv5 tile, two v_conv1 / stream tiles per clip boundary); (T, F) =
(24, 5) and (24, 6) at N = 2 (k_conv_v1s<8, 6> and k_conv_v1r / k_conv_v1p on 5 and 6 frames, the generic k_conv audio
branch and decoder); video=None at N = 3 (the cached one-clip embedding).  Every kernel-path switch runs against the
oracle and against its alternate path under the bound of the existing pairwise test of that switch.
"""
import functools

import numpy as np
import pytest

from forward_local_ref import signed_model
from oracle import keras_ref as K
from oracle import librosa_ref as R
from test_gpu_forward import (BF16_LAYER_REL, BF16_REL, FP32_ABS, FP32_REL, abs_rms, db_scale, make_inputs, rel_rms,
                              scratch)
from test_gpu_range import _rescaled

pytestmark = pytest.mark.gpu

SPLIT = "float32_split"
V15 = ["v_conv1", "v_conv2", "v_conv3", "v_conv4", "v_conv5"]
DENSE = ["concat", "enc_dense", "dec_dense1", "dec_dense2"]
A14 = ["a_conv1", "a_conv2", "a_conv3", "a_conv4"]
D13 = ["d_deconv1", "d_deconv2", "d_deconv3"]


def materialised(dtype, T):
    """The arena buffers the production path of a dtype writes (the others hold another forward's values): the fused
    d_deconv5 + d_deconv6 epilogue never stores d_deconv5; bf16 at 25 fps fuses a_conv1..5 (conv_aud.hip), d_deconv1..3
    (conv_dech.hip: only d_deconv3 is stored) and d_deconv4..6 (conv_dec.hip); the split tail keeps d_deconv4 in LDS."""
    if dtype == "float32":
        return A14 + V15 + DENSE + D13 + ["d_deconv4"]
    if dtype == SPLIT or T != 20:
        return A14 + V15 + DENSE + D13
    return V15 + DENSE + ["d_deconv3"]


def _copy(model):
    from avse_amd.model import KerasModel
    return KerasModel({k: v.copy() for k, v in model.tensors.items()})


@functools.lru_cache(maxsize=None)
def case(T, F, N, video=True):
    """One signed model per shape and its float64 oracle, shared by every test: `model` with the random-init output
    layer (bf16: relative gates), `model_db` with d_deconv6 at dB scale (fp32: the absolute gate where it is hardest).
    db_scale only changes the 64 -> 1 output layer, so one oracle run serves both."""
    from avse_amd.model import KerasModel
    model = signed_model(KerasModel.init(seed=3, randomize=True, audio_shape=(80, T), video_shape=(128, 128, F)))
    model_db = db_scale(_copy(model))
    if T == 20:
        mel, vid = make_inputs(N, 200 + N)
    else:
        from test_gpu_framerates import inputs
        mel, vid = inputs(np.random.default_rng(200 + T + F), N, T, F)
    c = dict(T=T, F=F, N=N, model=model, model_db=model_db, mel=mel, video=None, mean=None, std=None)
    vref = None
    if video:
        mean, std = R.video_normalizer_fit(vid)
        vref = R.video_normalize(vid, mean, std).astype(np.float32)
        c.update(video=vid, mean=mean, std=std)
    inter = {}
    c["ref_db"] = K.forward(model_db.layer_dict(), mel, vref, intermediates=inter)
    k6 = model.tensors["d_deconv6/kernel"].astype(np.float64)[0, 0, 0, :]
    c["ref"] = inter["d_deconv5"].astype(np.float64) @ k6 + float(model.tensors["d_deconv6/bias"][0])
    c["inter"] = inter
    return c


def run(c, dtype, load_opts=None, opts=None, names=(), checked=None, model=None, dw=None):
    """One forward of case c: (output, {layer: activation}, weights).  load_opts hold while the weights are packed;
    dw: weights of an earlier run."""
    from avse_amd import _lib, ops
    ctx = _lib.context()
    fp32 = dtype != "bfloat16"
    model = model or (c["model_db"] if fp32 else c["model"])
    if dw is None:
        with ctx.options(**(load_opts or {})):
            dw = ops.DeviceWeights(model, dtype)
    args = [ops.to_device(c["mel"]), None if c["video"] is None else ops.to_device(c["video"])]
    if c["video"] is not None:
        args += [ops.to_device(c["mean"]), ops.to_device(c["std"])]
    checked = dtype == SPLIT if checked is None else checked
    with ctx.options(**(opts or {})):
        got = ops.forward(dw, *args, checked=checked).cpu().numpy()
        sc = scratch(dw, c["N"], names=list(names)) if names else {}
    if checked:
        assert dw.last_range_bits == 0, hex(dw.last_range_bits)
    return got, sc, dw


def check_oracle(c, dtype, got, sc, what):
    """The project's gates of a dtype against the float64 oracle: the output and every layer read."""
    fp32 = dtype != "bfloat16"
    ref = c["ref_db"] if fp32 else c["ref"]
    assert np.isfinite(got).all()
    e, ae = rel_rms(got, ref), abs_rms(got, ref)
    layers = {k: rel_rms(v, c["inter"][k]) for k, v in sc.items()}
    print(f"{what} {dtype} T={c['T']} F={c['F']} N={c['N']}: output rel {e:.2e} abs {ae:.2e}; layers "
          + " ".join(f"{k} {v:.1e}" for k, v in layers.items()))
    if fp32:
        assert e <= FP32_REL and ae <= FP32_ABS, (what, e, ae)
    else:
        assert e <= BF16_REL, (what, e)
    tol = FP32_REL if fp32 else BF16_LAYER_REL
    bad = {k: v for k, v in layers.items() if not v <= tol}
    assert not bad, (what, bad)


@pytest.mark.parametrize("T,F,N", [(20, 5, 5), (24, 5, 2), (24, 6, 2)])
@pytest.mark.parametrize("dtype", ["float32", SPLIT, "bfloat16"])
def test_signed_forward_matches_oracle(gpu, dtype, T, F, N):
    """The production path: the output and every layer it materialises."""
    c = case(T, F, N)
    got, sc, _ = run(c, dtype, names=materialised(dtype, T))
    assert set(sc) == set(materialised(dtype, T))
    check_oracle(c, dtype, got, sc, "production")


@pytest.mark.parametrize("dtype", ["float32", SPLIT])
def test_signed_zero_video(gpu, dtype):
    """video=None at N = 3: the one-clip encoder on the all-zero clip (its N = 1 arena layout, the 36-way split
    v_conv6), cached and broadcast into concat's video half — twice, so the second forward reads the cache."""
    c = case(20, 5, 3, video=False)
    names = [n for n in materialised(dtype, 20) if n not in V15]
    dw = None
    for which in ("first", "cached"):
        got, sc, dw = run(c, dtype, names=names, dw=dw)
        check_oracle(c, dtype, got, sc, f"video=None {which}")


# name: (dtype, whether the switch is read while the weights are packed, options of both runs, the switch, layers both
# paths materialise, pair bound per layer, pair bound of the output).  The pair bounds are the existing pairwise
# test's: test_bf16_halo_video_convs_match_generic_kernel (BF16_LAYER_REL / BF16_REL),
# test_split_packed_v1_matches_v1s_and_oracle, test_bf16_mfma32_variant_agrees, test_gpu_stream_planar GROUPING_REL,
# test_gpu_generic_planar FORMS_REL, test_bf16_fused_per_clip_kernels_match_layer_path /
# test_split_gemm_matches_kconv_and_oracle, test_gemm_ksplit1_small_batch,
# test_split_windowed_layers_match_kconv_and_oracle, test_split_valu_aconv1_matches_kconv_and_oracle,
# test_fused_tail_matches_unfused.  The split no_halo pair has no earlier test: both paths sum the same products in
# fp32 blocks, as the other split pairs, hence their 1e-6.
SWITCHES = {
    "no_halo-bf16": ("bfloat16", True, {}, dict(no_halo=1), V15 + ["concat"], BF16_LAYER_REL, BF16_REL),
    "no_halo-split": (SPLIT, True, {}, dict(no_halo=1), V15 + ["concat"], 1e-6, 1e-6),
    "no_v1p-split": (SPLIT, True, {}, dict(no_v1p=1), ["v_conv1", "v_conv2"], 1e-6, 1e-6),
    "mfma32-bf16": ("bfloat16", False, {}, dict(mfma32=1), V15, 1e-2, 1e-2),
    "no_planar-split": (SPLIT, False, {}, dict(no_planar=1), V15[1:], 1e-6, 1e-6),
    "four_products-split": (SPLIT, False, {}, dict(four_products=1), DENSE + D13, 1e-6, 1e-6),
    "no_gemm-bf16": ("bfloat16", False, {}, dict(no_gemm=1), DENSE, 1e-2, 1e-2),
    "no_gemm-split": (SPLIT, False, {}, dict(no_gemm=1), DENSE + ["d_deconv1"], 1e-6, 1e-6),
    "gemm_ksplit_cap-bf16": ("bfloat16", False, {}, dict(gemm_ksplit_cap=1), DENSE, 1e-2, 1e-2),
    "no_win-split": (SPLIT, False, dict(no_dectail=1), dict(no_win=1), ["a_conv2"] + D13 + ["d_deconv4"], 1e-6, 1e-6),
    "no_a1valu-split": (SPLIT, False, {}, dict(no_a1valu=1), ["a_conv1", "a_conv2"], 1e-6, 1e-6),
    "layer_path-bf16": ("bfloat16", False, {}, dict(no_audenc=1, no_dechead=1, no_dectail=1), ["concat", "d_deconv3"],
                        1e-2, 1e-2),
    "unfused_tail-bf16": ("bfloat16", False, {}, dict(unfused_tail=1), ["d_deconv3"], 2e-3, 2e-3),
    "unfused_tail-float32": ("float32", False, {}, dict(unfused_tail=1), D13 + ["d_deconv4"], 1e-6, 1e-6),
}


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_signed_switch_matches_oracle_and_alternate_path(gpu, switch):
    """25 fps, N = 5: the production path and the path behind one switch, each against the oracle under the dtype's
    gates, and against each other under the bound of the switch's own pairwise test."""
    dtype, at_load, base, opt, names, pair_layer, pair_out = SWITCHES[switch]
    c = case(20, 5, 5)
    got_a, sc_a, _ = run(c, dtype, opts=base, names=names)
    got_b, sc_b, _ = run(c, dtype, load_opts=opt if at_load else None, opts=dict(base, **({} if at_load else opt)),
                         names=names)
    check_oracle(c, dtype, got_a, sc_a, "production")
    check_oracle(c, dtype, got_b, sc_b, switch)
    pairs = {k: rel_rms(sc_b[k], sc_a[k]) for k in names}
    po = rel_rms(got_b, got_a)
    print(f"{switch}: alternate vs production, output {po:.2e}; " + " ".join(f"{k} {v:.1e}" for k, v in pairs.items()))
    bad = {k: v for k, v in pairs.items() if not v <= pair_layer}
    assert not bad, (switch, bad)
    assert po <= pair_out, (switch, po)


def test_signed_split_with_activation_exponents(gpu):
    """Activation exponents away from 0 on signed layers: v_conv2's BN x 2^12 (v_conv3's kernel x 2^-12) and a_conv3's
    x 2^-8 (a_conv4's kernel x 2^8) — powers of two, the same network function, so the oracle is the shared one.  The
    exponents then scale negative scales, |scale| of the tiled layers and the all-zero a_conv3 / v_conv3 channels."""
    c = case(20, 5, 5)
    model = _rescaled(_rescaled(_copy(c["model_db"]), "v_conv2", "v_conv3", 12), "a_conv3", "a_conv4", -8)
    names = [n for n in materialised(SPLIT, 20)]
    got, sc, dw = run(c, SPLIT, names=names, model=model)
    e = dw.act_exponents()
    assert e["v_conv2"] < 0 and e["a_conv3"] > 0 and all(v == 0 for k, v in e.items() if k not in ("v_conv2", "a_conv3")), e
    inter = dict(c["inter"])
    inter["v_conv2"] = inter["v_conv2"] * 2.0 ** 12
    inter["a_conv3"] = inter["a_conv3"] * 2.0 ** -8
    check_oracle(dict(c, inter=inter), SPLIT, got, sc, "exponents v_conv2 +12 / a_conv3 -8")
