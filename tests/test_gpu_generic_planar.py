"""The split dtype's generic layers on planar slab pairs with three products (Ah Wh + Al Wh + Ah Wl per pair of 16-k
slabs): k_gemm (gemm.hip: v_conv6 and the three dense layers) and the fused decoder tail k_dec_tail_s16 (conv_dects.hip:
d_deconv4..6), against the float64 oracle and against the slab-by-slab four-product form of both kernels (option
four_products), layer by layer and at the output.  d_deconv1..3 (k_conv) form four products under both settings: they
are compared as consumers of the k_gemm layers' outputs.

N = 1: v_conv6's 36-way split (one summation block = four pairs per split), a ragged 128-row tile in every launch, both
halves of the clip and the seam rows 36..43 of the fused decoder tail.  N = 3 and N = 37: v_conv6 tiles that span clips
(8 clips per tile) and dense tiles with rows past M.  T = 24, F = 5 is the other audio geometry (W5 = 6: wider concat and dec_dense2,
so other split plans).

Bounds: the fp32 path's own (test_gpu_forward.py FP32_REL / FP32_ABS, dB-scaled model) against the oracle; 1e-6 relative
RMS between the two forms, the bound the suite uses for "the same products in another grouping": the dropped Al Wl terms
are <= 2^-22 of their products, below the pairs' own representation error.
"""
import numpy as np
import pytest

from oracle import keras_ref as K
from test_gpu_forward import FP32_ABS, FP32_REL, abs_rms, db_scale, make_inputs, rel_rms, scratch

pytestmark = pytest.mark.gpu

SPLIT = "float32_split"
LAYERS = ["concat", "enc_dense", "dec_dense1", "dec_dense2", "d_deconv1", "d_deconv2", "d_deconv3"]
FORMS_REL = 1e-6
SEED = 80

_cases = {}


def case(gpu, N):
    """One oracle run and one forward per form for batch N, shared by the tests below."""
    if N in _cases:
        return _cases[N]
    from avse_amd import _lib, ops
    from avse_amd.model import KerasModel
    ctx = _lib.context()
    model = db_scale(KerasModel.init(seed=SEED + N, randomize=True))
    mel, video = make_inputs(N, SEED + N + 100)
    inter = {}
    ref = K.forward(model.layer_dict(), mel, video, intermediates=inter)
    dw = ops.DeviceWeights(model, SPLIT)
    out = {}
    for four in (0, 1):
        with ctx.options(four_products=four):
            got = ops.forward(dw, ops.to_device(mel), ops.to_device(video), checked=True).cpu().numpy()
            out[four] = dict(got=got, sc=scratch(dw, N, names=LAYERS), bits=dw.last_range_bits)
    _cases[N] = dict(model=model, mel=mel, video=video, ref=ref, inter=inter, dw=dw, three=out[0], four=out[1])
    return _cases[N]


@pytest.mark.parametrize("N", [1, 3, 37])
@pytest.mark.parametrize("form", ["three", "four"])
def test_forms_match_oracle(gpu, N, form):
    c = case(gpu, N)
    r = c[form]
    assert r["bits"] == 0, hex(r["bits"])
    for k in LAYERS:
        e = rel_rms(r["sc"][k], c["inter"][k])
        print(f"{form} N={N} {k}: rel {e:.2e}")
        assert e <= FP32_REL, (k, e)
    e, ae = rel_rms(r["got"], c["ref"]), abs_rms(r["got"], c["ref"])
    print(f"{form} N={N} output: RMS {np.sqrt(np.mean(c['ref'] ** 2)):.3g}, abs {ae:.3e}, rel {e:.2e}")
    assert np.isfinite(r["got"]).all()
    assert e <= FP32_REL and ae <= FP32_ABS, (e, ae)


@pytest.mark.parametrize("N", [1, 3, 37])
def test_three_products_match_four(gpu, N):
    c = case(gpu, N)
    for k in LAYERS:
        e = rel_rms(c["three"]["sc"][k], c["four"]["sc"][k])
        print(f"three vs four N={N} {k}: rel {e:.2e}")
        assert e <= FORMS_REL, (k, e)
    e = rel_rms(c["three"]["got"], c["four"]["got"])
    seam = rel_rms(c["three"]["got"][:, 36:44], c["four"]["got"][:, 36:44])
    print(f"three vs four N={N} output: rel {e:.2e}, seam rows 36..43 {seam:.2e}")
    assert e <= FORMS_REL and seam <= FORMS_REL, (e, seam)


def test_layer_path_tail_matches_oracle_and_four(gpu):
    """d_deconv4 materialised (option no_dectail with unfused_tail: the layer-by-layer tail) under both forms."""
    from avse_amd import _lib, ops
    c = case(gpu, 3)
    ctx = _lib.context()
    sc = {}
    for four in (0, 1):
        with ctx.options(four_products=four, no_dectail=1, unfused_tail=1):
            got = ops.forward(c["dw"], ops.to_device(c["mel"]), ops.to_device(c["video"])).cpu().numpy()
            sc[four] = scratch(c["dw"], 3, names=["d_deconv4"])["d_deconv4"]
        assert rel_rms(got, c["ref"]) <= FP32_REL and abs_rms(got, c["ref"]) <= FP32_ABS
        e = rel_rms(sc[four], c["inter"]["d_deconv4"])
        print(f"four_products={four} d_deconv4: rel {e:.2e}")
        assert e <= FP32_REL, e
    e = rel_rms(sc[0], sc[1])
    print(f"three vs four d_deconv4: rel {e:.2e}")
    assert e <= FORMS_REL, e


def test_range_guard_still_reports_d_deconv4(gpu):
    """d_deconv4's activations x 2^15 with the activation exponents off (test_gpu_range.py's recipe): its pairs leave the
    f16 range in both halves of the clip, and the checked forward reports that layer and returns the exact-fp32 forward."""
    from avse_amd import _lib, ops
    from avse_amd.model import KerasModel
    from test_gpu_range import _rescaled
    model = _rescaled(db_scale(KerasModel.init(seed=10, randomize=True)), "d_deconv4", "d_deconv5", 15)
    mel, video = make_inputs(1, 65)
    inter = {}
    K.forward(model.layer_dict(), mel, video, intermediates=inter)
    big = np.abs(inter["d_deconv4"][0]).max(axis=(1, 2))
    assert big[:20].max() > 65520.0 and big[20:].max() > 65520.0
    f32 = ops.forward(ops.DeviceWeights(model, "float32"), ops.to_device(mel), ops.to_device(video)).cpu().numpy()
    with _lib.context().options(no_act_scale=1):
        dw = ops.DeviceWeights(model, SPLIT)
        with pytest.warns(RuntimeWarning, match="d_deconv4"):
            got = ops.forward(dw, ops.to_device(mel), ops.to_device(video), checked=True).cpu().numpy()
    assert dw.last_range_bits >> 17 & 1, hex(dw.last_range_bits)
    assert np.array_equal(got, f32)


def test_batch_invariant(gpu):
    """Clips 0 and 4 of an N = 5 forward equal their own N = 1 forwards bit for bit (output and the k_gemm layers)."""
    from avse_amd import ops
    from avse_amd.model import KerasModel
    model = db_scale(KerasModel.init(seed=SEED + 5, randomize=True))
    mel, video = make_inputs(5, SEED + 105)
    dw = ops.DeviceWeights(model, SPLIT)
    full = ops.forward(dw, ops.to_device(mel), ops.to_device(video)).cpu().numpy()
    sc = scratch(dw, 5, names=LAYERS)
    for i in (0, 4):
        one = ops.forward(dw, ops.to_device(mel[i:i + 1]), ops.to_device(video[i:i + 1])).cpu().numpy()
        sc1 = scratch(dw, 1, names=LAYERS)
        assert np.array_equal(one[0], full[i]), i
        for k in LAYERS:
            assert np.array_equal(sc1[k][0], sc[k][i]), (i, k)


def test_other_audio_geometry(gpu):
    """T = 24, F = 5, N = 2: W5 = 6, so concat and dec_dense2 are wider than at T = 20 and the dense layers split otherwise."""
    from avse_amd import _lib, ops
    from avse_amd.model import KerasModel
    from conftest import synth_video
    model = db_scale(KerasModel.init(seed=SEED + 2, randomize=True, audio_shape=(80, 24), video_shape=(128, 128, 5)))
    rng = np.random.default_rng(SEED + 3)
    mel = rng.normal(-40, 15, (2, 80, 24)).astype(np.float32)
    video = synth_video(rng, 2, f=5)
    ref = K.forward(model.layer_dict(), mel, video)
    dw = ops.DeviceWeights(model, SPLIT)
    got = {}
    for four in (0, 1):
        with _lib.context().options(four_products=four):
            got[four] = ops.forward(dw, ops.to_device(mel), ops.to_device(video), checked=True).cpu().numpy()
        assert dw.last_range_bits == 0
        e, ae = rel_rms(got[four], ref), abs_rms(got[four], ref)
        print(f"T=24 F=5 four_products={four}: abs {ae:.3e} rel {e:.2e}")
        assert e <= FP32_REL and ae <= FP32_ABS, (e, ae)
    assert rel_rms(got[0], got[1]) <= FORMS_REL
