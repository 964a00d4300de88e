"""Every materialised layer of the bf16 forward, elementwise, on the device's own input (forward_local_ref.py).

tests/test_gpu_forward.py holds a bf16 layer to a relative RMS of 1.5e-2 over the tensor and the fused kernels to 1e-2
against the layer path: a tap dropped at one tile corner passes, and so does a channel reading its neighbour's shift
in more than a third of v_conv3's channels (tests/test_forward_local_ref.py asserts both).  Here layer i is fed the DEVICE'S OWN previous
buffer x (read with test_gpu_forward.scratch; bf16 values are exact in float64), the expectation is the float64 layer
on x with the bf16-rounded kernel, and per element

    E = max(0, |got - ref| - 1/2 ulp_bf16(max(|got|, |ref|))) / (2^-24 S),     S = |scale| sum |w| |x| + |shift|

is the device's fp32 accumulation error in units of one fp32 rounding of the absolute sum (the half ulp is the exact
cost of the final rounding, not a tolerance).  Gate per (case, layer): max E <= max(1, 8 x the float32 stand-in's max E
on the same x), never above the reduction length K.  One dropped tap is E ~ 2^24 / K.

The model is forward_local_ref.signed_model (negative and zero gammas, two all-zero output channels); the inputs are
rounded to bf16 on the host and no normaliser runs, so the first layers' inputs are exact and unique (the normaliser is
covered by tests/test_gpu_forward_signed.py).  Shapes as there: 25 fps at N = 5, (24, 5) and (24, 6) at N = 2.

Paths:
  layer       no_audenc + no_dechead + no_dectail + unfused_tail: all 20 buffers materialised (k_conv for the audio
              branch and decoder, conv_v1r.hip / conv_stream.hip, k_gemm<1> for v_conv6, k_gemm for the dense layers,
              launch_out_conv for d_deconv6)
  generic     the same with no_gemm and, at load, no_halo: v_conv1..6 and the dense layers on k_conv (pooled epilogue,
              split-K reduce)
  production  the layers it materialises: v_conv1..v_conv5, concat's video half (v_conv6), enc_dense, dec_dense1,
              dec_dense2
  mfma32      v_conv2..v_conv5 on the 32x32x16 waves (25 fps)
  chains      the fused per-clip kernels at 25 fps, from the device's materialised chain input to its materialised
              output: conv_aud.hip a_conv1..a_conv5 -> concat[:, :3200]; conv_dech.hip d_deconv1..d_deconv3;
              conv_dec.hip d_deconv4..d_deconv6 -> the output (float32: no ulp term).  The reference rounds to bf16
              after each inner layer; an inner rounding the device takes the other way moves the result by
              |scale w| ulp(x), which no widened ulp term of the OUTPUT can bound (forward_local_ref's docstring: the
              stand-in chain itself would need 1/2 + 400 ulps), so the chain carries the exact interval of every inner
              activation and grants rho = spread of those intervals through the last layer.  E = excess(.., slack=rho)
              is held to the last layer's own gate.  For the decoder chains rho is a few tens of roundings at the
              median; over the five audio layers the intervals compound to the size of a dropped tap, so that chain
              only bounds gross defects here (its layers are held elementwise on the layer path, the fused kernel to
              the RMS gates of tests/test_gpu_forward.py and tests/test_gpu_forward_signed.py).

Measured on an MI355X (profiles/forward_local_checks.txt has every layer, its gate and the worst element):

  largest E per path and shape, device | float32 stand-in, and the layer closest to its gate (118 layer checks, all pass):

  layer      25fps    device 2.561 | stand-in 2.561   closest: d_deconv4 0.270 against 1.3
  layer      2997fps  device 2.151 | stand-in 2.151   closest: a_conv4 0.210 against 1.0
  layer      30fps    device 2.512 | stand-in 2.512   closest: d_deconv3 0.295 against 1.3
  generic    25fps    device 0.349 | stand-in 1.334   closest: v_conv1 0.303 against 2.4
  generic    2997fps  device 0.231 | stand-in 0.522   closest: v_conv5 0.148 against 1.0
  generic    30fps    device 0.501 | stand-in 1.832   closest: v_conv5 0.331 against 2.0
  production 25fps    device 0.413 | stand-in 0.670   closest: v_conv4 0.406 against 3.2
  production 2997fps  device 0.238 | stand-in 0.522   closest: v_conv3 0.173 against 1.9
  production 30fps    device 0.403 | stand-in 0.625   closest: v_conv1 0.178 against 1.9
  mfma32     25fps    device 0.413 | stand-in 0.670   closest: v_conv4 0.406 against 3.2

  The 2.5 of the layer path is d_deconv6 (K = 64, float32 output: no ulp term), equal to the stand-in's; among the bf16
  outputs the largest device E is 0.501.  mfma32 returned v_conv2..v_conv5 bit for bit equal to the 16x16x32 waves.

  chains (production, 25 fps), device E with the interval slack | plain E without it | stand-in chain | gate, and
  rho in units of 2^-24 S (median, max):
    a_conv1..a_conv5     0.000 | 3.5e3 | 0.000 |  1.0    rho 1.2e6, 1.0e7  (the size of a dropped tap: gross defects only)
    d_deconv1..d_deconv3 0.401 | 1.6e3 | 0.056 |  1.6    rho 13, 2.3e4
    d_deconv4..d_deconv6 1.202 | 6.4e3 | 2.929 | 23.4    rho 12, 2.6e4
  Closest approach to a gate overall: the d_deconv1..d_deconv3 chain, 0.401 against 1.6.  No defect found.
"""
import functools

import numpy as np
import pytest

import forward_local_ref as R
from test_gpu_forward import make_inputs, scratch

pytestmark = pytest.mark.gpu

SHAPES = {"25fps": (20, 5, 5), "2997fps": (24, 5, 2), "30fps": (24, 6, 2)}     # T, F, N
LAYER_PATH = dict(no_audenc=1, no_dechead=1, no_dectail=1, unfused_tail=1)
VIDEO_DENSE = R.NAMES[R.V1:R.D1]                                    # v_conv1 .. v_conv6, enc_dense .. dec_dense2
VIDEO_BUFS = R.BUF_NAMES[6:15]                                       # v_conv1 .. v_conv5, concat, enc_dense .. dec_dense2
# path: (options of the forward, options while the weights are packed, layers checked, arena buffers it writes)
PATHS = {
    "layer": (LAYER_PATH, {}, R.NAMES, R.BUF_NAMES[2:]),
    "generic": (dict(LAYER_PATH, no_gemm=1), dict(no_halo=1), VIDEO_DENSE, R.BUF_NAMES[2:]),
    "production": ({}, {}, VIDEO_DENSE, VIDEO_BUFS + ["d_deconv3"]),
    "mfma32": (dict(mfma32=1), {}, ["v_conv2", "v_conv3", "v_conv4", "v_conv5"], VIDEO_BUFS),
}
CASES = [(s, p, n) for p, (_, _, names, _) in PATHS.items() for s in SHAPES for n in names if p != "mfma32" or s == "25fps"]
CHAINS = [("a_conv1", "a_conv5"), ("d_deconv1", "d_deconv3"), ("d_deconv4", "d_deconv6")]


@functools.lru_cache(maxsize=None)
def reference(shape):
    from avse_amd.model import KerasModel
    T, F, N = SHAPES[shape]
    model = R.signed_model(KerasModel.init(seed=3, randomize=True, audio_shape=(80, T), video_shape=(128, 128, F)))
    rng = np.random.default_rng(300 + T + F)
    mel = R.round_bf16(rng.normal(-40, 12, (N, 80, T))).astype(np.float32)
    if T == 20:
        mel = R.round_bf16(make_inputs(N, 300)[0]).astype(np.float32)
    video = R.round_bf16((rng.integers(0, 256, (N, 128, 128, F)) - 127.5) / 74.0).astype(np.float32)
    return model, R.LocalRef(model.tensors), mel, video


@functools.lru_cache(maxsize=2)
def device(shape, path):
    """One forward of a path; every buffer of the arena as [N, ...] float64 (bf16 values are exact), with a_conv5 /
    v_conv6 taken from concat's halves and d_deconv6 the float32 output.  Only what the path writes is read (the other
    buffers hold another forward's values)."""
    from avse_amd import _lib, ops
    T, F, N = SHAPES[shape]
    model, ref, mel, video = reference(shape)
    opts, load_opts, _, bufs = PATHS[path]
    ctx = _lib.context()
    with ctx.options(**load_opts):
        dw = ops.DeviceWeights(model, "bfloat16")
    with ctx.options(**opts):
        out = ops.forward(dw, ops.to_device(mel), ops.to_device(video)).cpu().numpy()
        sc = scratch(dw, N, names=bufs)
    outs = {k: v.astype(np.float64) for k, v in sc.items()}
    aemb = outs["dec_dense2"][0].size
    outs["a_conv5"] = outs["concat"][:, :aemb].reshape(outs["dec_dense2"].shape)     # Flatten of [5, W5, 128]
    outs["v_conv6"] = outs["concat"][:, aemb:].reshape(N, 2, 2, 512)
    outs["d_deconv6"] = out.astype(np.float64)[..., None]
    assert np.isfinite(out).all()
    return outs


@pytest.mark.parametrize("shape,path,layer", CASES)
def test_layer_matches_local_reference(gpu, shape, path, layer):
    model, ref, mel, video = reference(shape)
    outs = device(shape, path)
    i = R.NAMES.index(layer)
    x = R.inputs_of(i, outs, mel, video)
    want, S = ref.layer(i, x), ref.abs_sum(i, x)
    ulp = i != R.D6
    E = R.excess(outs[layer], want, S, ulp=ulp)
    cal = float(R.excess(ref.standin(i, x), want, S, ulp=ulp).max())
    g = R.gate(cal, ref.layers[i].K)
    worst = np.unravel_index(int(np.argmax(E)), E.shape)
    print(f"\nLOCAL {shape:7s} {path:10s} {layer:11s} K {ref.layers[i].K:5d}  device E {E.max():8.3f}  stand-in {cal:7.3f}  "
          f"gate {g:6.1f}  worst at {tuple(int(v) for v in worst)}")
    assert E.max() <= g, (shape, path, layer, float(E.max()), g, worst)


@pytest.mark.parametrize("first,last", CHAINS)
def test_fused_chain_matches_local_reference(gpu, first, last):
    """The production path's fused per-clip kernels at 25 fps (module docstring, chains)."""
    shape = "25fps"
    model, ref, mel, video = reference(shape)
    outs = device(shape, "production")
    a, b = R.NAMES.index(first), R.NAMES.index(last)
    x = R.inputs_of(a, outs, mel, video)
    want, S, rho, g, cal = ref.chain(a, b, x)
    ulp = b != R.D6
    got = outs[last]
    E = R.excess(got, want, S, slack=rho, ulp=ulp)
    plain = float(R.excess(got, want, S, ulp=ulp).max())
    std = ref.chain_standin(a, b, x)
    E_std = float(R.excess(std, want, S, slack=rho, ulp=ulp).max())
    rho_E = rho / (R.EPS24 * S)
    print(f"\nCHAIN {first}..{last}: device E {E.max():.3f} (without the interval slack {plain:.3g}), stand-in chain "
          f"{E_std:.3f}, last-layer stand-in {cal:.3f}, gate {g:.1f}; rho > 0 on {float((rho > 0).mean()):.1%}, in units of "
          f"2^-24 S median {np.median(rho_E):.3g} max {rho_E.max():.3g}")
    assert E.max() <= g, (first, last, float(E.max()), g)
