"""Split stream convolutions (conv_stream.hip, v_conv2..v_conv5 in AVSE_F32_SPLIT) on planar slice-pair operands against the
float64 oracle and against the slice-by-slice lane-swap grouping (option no_planar), which forms the same three products.

N = 1: fewer tiles than workgroups in v_conv4 / v_conv5 (some workgroups have no tile and leave before the first barrier).
N = 5: a ragged last 4-clip tile in v_conv5's 8x8x4 geometry, more than one tile per workgroup in v_conv2.  Both run the
25-tap kernel (an odd tap count: slice pairs straddle chunk boundaries, so a pair's two halves of the wave read different
halo slots) and the 9-tap kernels.

Bounds: the fp32 path's own (test_gpu_forward.py FP32_REL / FP32_ABS, dB-scaled model) against the oracle; 1e-6 relative RMS
between the two groupings (they differ only in which 32 exact products share one rounding into the fp32 accumulator).
"""
import numpy as np
import pytest

from test_gpu_forward import FP32_ABS, FP32_REL, abs_rms, make_inputs, rel_rms, run_case, scratch

pytestmark = pytest.mark.gpu

SPLIT = "float32_split"
LAYERS = ["v_conv2", "v_conv3", "v_conv4", "v_conv5"]
GROUPING_REL = 1e-6
SEED = 40

_cases = {}


def case(gpu, N):
    """One oracle run and one forward per grouping for batch N, shared by the tests below."""
    if N in _cases:
        return _cases[N]
    from avse_amd import _lib, ops
    ctx = _lib.context()
    ctx.range_status()   # clear what earlier forwards raised
    with ctx.options(no_planar=0):
        got, ref, inter, dw = run_case(gpu, N, SPLIT, seed=SEED + N, db=True)
        sc = scratch(dw, N, names=LAYERS)
    bits = ctx.range_status()
    mel, video = make_inputs(N, SEED + N + 100)
    with ctx.options(no_planar=1):
        got_swap = ops.forward(dw, ops.to_device(mel), ops.to_device(video)).cpu().numpy()
        sc_swap = scratch(dw, N, names=LAYERS)
    bits_swap = ctx.range_status()
    _cases[N] = dict(got=got, ref=ref, inter=inter, dw=dw, sc=sc, bits=bits, mel=mel, video=video, got_swap=got_swap,
                     sc_swap=sc_swap, bits_swap=bits_swap)
    return _cases[N]


@pytest.mark.parametrize("N", [1, 5])
def test_planar_matches_oracle(gpu, N):
    c = case(gpu, N)
    for k in LAYERS:
        e = rel_rms(c["sc"][k], c["inter"][k])
        print(f"planar N={N} {k}: rel {e:.2e}")
        assert e <= FP32_REL, (k, e)
    e, ae = rel_rms(c["got"], c["ref"]), abs_rms(c["got"], c["ref"])
    print(f"planar N={N} output: RMS {np.sqrt(np.mean(c['ref'] ** 2)):.3g}, abs {ae:.3e}, rel {e:.2e}")
    assert np.isfinite(c["got"]).all()
    assert e <= FP32_REL and ae <= FP32_ABS, (e, ae)


@pytest.mark.parametrize("N", [1, 5])
def test_planar_matches_swap_grouping(gpu, N):
    c = case(gpu, N)
    for k in LAYERS:
        e = rel_rms(c["sc"][k], c["sc_swap"][k])
        print(f"planar vs no_planar N={N} {k}: rel {e:.2e}")
        assert e <= GROUPING_REL, (k, e)
    e = rel_rms(c["got"], c["got_swap"])
    print(f"planar vs no_planar N={N} output: rel {e:.2e}")
    assert e <= GROUPING_REL, e
    # the lane-swap grouping itself stays within the oracle bounds
    assert rel_rms(c["got_swap"], c["ref"]) <= FP32_REL and abs_rms(c["got_swap"], c["ref"]) <= FP32_ABS


@pytest.mark.parametrize("N", [1, 5])
def test_range_guard_clear(gpu, N):
    c = case(gpu, N)
    assert c["bits"] == 0 and c["bits_swap"] == 0, (hex(c["bits"]), hex(c["bits_swap"]))


def test_planar_batch_invariant(gpu):
    """Each clip of the N = 5 planar forward equals its own N = 1 forward bit for bit (output and v_conv2..v_conv5)."""
    from avse_amd import ops
    c = case(gpu, 5)
    dw = c["dw"]
    with dw.ctx.options(no_planar=0):
        for i in range(5):
            one = ops.forward(dw, ops.to_device(c["mel"][i:i + 1]), ops.to_device(c["video"][i:i + 1])).cpu().numpy()
            sc1 = scratch(dw, 1, names=LAYERS)
            assert np.array_equal(one[0], c["got"][i]), i
            for k in LAYERS:
                assert np.array_equal(sc1[k][0], c["sc"][k][i]), (i, k)
