"""Every training backward kernel of csrc/train.hip against the float64 layer-local reference (train_local_ref.py):
k_act_bwd, k_colreduce<2> + k_colfinish<2>, k_bn_bwd / k_bn_bwd_colsum + k_colfinish<3>, k_colreduce<0>, k_wgrad /
k_wgrad_na / k_wgrad_nat + k_sum_splits and the dgrad launches of k_conv, layer by layer.

tests/test_gpu_train.py compares gradients end to end, where one LeakyReLU slope or pool winner flipped by float32
rounding moves every upstream gradient and the gate has to be 1e-2.  Here every expectation is computed from the
DEVICE'S OWN upstream quantity (read back through the trainer's test aids AVSE_TRAIN_DEBUG_GHAT / _STOP / _GIN) plus
the float64 forward state, so no flip leaks in and each stage is held to float32 rounding:

  a  ghat (DEBUG_GHAT)          = act_bwd(i, g_out_dev), g_out_dev the next layer's DEBUG_GIN (a_conv5 / v_conv6:
                                  their slices of enc_dense's; d_deconv5: d_deconv6's), elementwise outside the
                                  ambiguous elements (|BN output| or pool gap <= 1e-3 x RMS); those must lie between
                                  the two slopes, a pool window must hold one entry; ambiguous share <= 1% asserted
  b  dgamma, dbeta, dz (STOP)   = bn_bwd(i, ghat_dev)
  c  dW, dbias                  = param_grads(i, dz_dev); pre-BN biases (true gradient 0) absolutely against the
                                  float64 sum of dz_dev on the scale of sum |dz_dev|
  d  DEBUG_GIN                  = input_grad(i, dz_dev)                (not a_conv1 / v_conv1: their input is data)

d_deconv6 has no BatchNormalization: its dz is dL/dy, which AVSE_TRAIN_DEBUG_STOP at layer 19 copies to the scratch
(the device's own g6, not the oracle's 2 (y - t) / n).

Metric: relative RMS per tensor.  Gate per (case, layer, check): max(1e-5, 8 x the error of the float32 stand-in — the
oracle in torch-CPU float32 — on the same check and case), never above 5e-4 (train_local_ref.gate; the factor covers
another float32 summation order over up to 262k rows and a forward whose x differs from torch's).  The checks combine
reads of separate grads-only steps, so the first test asserts that such steps are bit-identical.

Cases (train_local_ref.CASES): N = 3 (ragged row counts everywhere, short train_split grids), N = 2 of the
(80, 24) / (128, 128, 6) plan without dropout, N = 16 with max_batch 16 (the reference's fit batch), and n3s: N = 3
with every gamma negated on channels 1::3, as a trained checkpoint may hold (measured, largest over its 20 layers:
ghat 3.8e-8, dgamma 3.2e-6, dbeta 1.9e-7, dz 1.2e-5 at dec_dense1 against a gate of 3.3e-4, dW 3.0e-6, dbias 3.3e-8,
gin 2.3e-7, ambiguous share <= 2.9e-3; all pass).

Measured on an MI355X (profiles/train_local_checks.txt has every layer and its gate), largest relative RMS over the
layers of a case, device | float32 stand-in; all 3 x 20 layers pass, two grads-only steps are bit-equal, no defect:

             N = 3                  N = 2, (80, 24) / (128, 128, 6)   N = 16
  a ghat     3.8e-8 | 3.8e-8        1.4e-8 | 1.4e-8                   3.9e-8 | 3.9e-8
  b dgamma   1.8e-6 | 9.2e-6        2.5e-5 | 7.3e-5                   1.2e-6 | 3.6e-6
  b dbeta    2.3e-7 | 2.5e-7        3.1e-7 | 6.4e-7                   2.1e-7 | 2.5e-7
  b dz       6.6e-6 | 3.4e-5        1.2e-4 | 3.8e-4                   1.1e-6 | 3.2e-6
  c dW       1.8e-6 | 8.5e-6        2.1e-5 | 6.1e-5                   1.1e-6 | 3.2e-6
  c dbias    3.4e-8 | 3.6e-7        2.7e-8 | 2.9e-7                   5.8e-8 | 2.1e-7
  d gin      2.3e-7 | 7.7e-7        2.3e-7 | 8.5e-7                   2.3e-7 | 7.8e-7
  ambiguous  <= 2.6e-3              <= 2.5e-3                         <= 2.5e-3      (share, asserted <= 1e-2)

Closest to its gate: a_conv5's dgamma at N = 3 (8.1e-7 against 1e-5).  The N = 2 column is the dense layers'
BatchNormalization over M = 2 rows, whose dz cancels to ~1e-3 of its terms (train_local_ref.gate): dec_dense1's dz,
1.2e-4 on the device against 3.8e-4 for the stand-in, is the one place where the 5e-4 ceiling is the gate.
"""
import ctypes

import numpy as np
import pytest
import torch

import train_local_ref as R

pytestmark = pytest.mark.gpu


class Device:
    """Grads-only steps of one trainer with a debug flag, and the reads they leave in the dz scratch."""

    def __init__(self, gpu, case, ref):
        from avse_amd import _lib, ops
        c = R.CASES[case]
        model, mel, video, target = R.case_inputs(case)
        self._lib, self.ref, self.c, self.N = _lib, ref, c, c["N"]
        self.tr = ops.Trainer(model, max_batch=c["max_batch"], device=gpu)
        self.inputs = [torch.from_numpy(a).to(gpu) for a in (mel, video, target)]
        self.loss = torch.zeros((), dtype=torch.float32, device=gpu)
        self.gpu = gpu
        self._gin = {}

    def step(self, flags=0):
        L = self._lib
        a, v, t = self.inputs
        L.check(L.load().avse_trainer_step(self.tr.handle, L.ptr(a), L.ptr(v), L.ptr(t), None, None, self.N, 5e-4,
                                           self.c["rate"], self.c["drop_seed"], L.AVSE_TRAIN_GRADS_ONLY | flags,
                                           L.ptr(self.loss), L.stream_handle(self.gpu)), "avse_trainer_step")

    def blob(self):
        return self.tr._read(self._lib.AVSE_TRAIN_GRADS)

    def scratch(self, flag, layer, count):
        self.step(flag | (layer << 8))
        out = np.empty(count, np.float32)
        L = self._lib
        L.check(L.load().avse_trainer_read(self.tr.handle, L.AVSE_TRAIN_DEBUG_DZ, out.ctypes.data_as(ctypes.c_void_p),
                                           count), "avse_trainer_read")
        return out

    def ghat(self, i):
        return self.ref.unpack_z(i, self.scratch(self._lib.AVSE_TRAIN_DEBUG_GHAT, i, self.ref.z_floats(i)))

    def dz(self, i):
        return self.ref.unpack_z(i, self.scratch(self._lib.AVSE_TRAIN_DEBUG_STOP, i, self.ref.z_floats(i)))

    def gin(self, i):
        if i not in self._gin:
            self._gin[i] = self.ref.unpack_gin(i, self.scratch(self._lib.AVSE_TRAIN_DEBUG_GIN, i, self.ref.gin_floats(i)))
        return self._gin[i]


@pytest.fixture(scope="module", params=list(R.CASES))
def case(request, gpu):
    name = request.param
    c = R.CASES[name]
    model, mel, video, target = R.case_inputs(name)
    ref = R.LocalRef(model.tensors, mel, video, target, c["rate"], c["drop_seed"])
    _, standin = R.standin(model.tensors, mel, video, target, c["rate"], c["drop_seed"])
    dev = Device(gpu, name, ref)
    dev.step()
    blob = dev.blob()
    from avse_amd.model import KerasModel
    grads = KerasModel.from_blob(blob, c["T"], c["F"]).tensors
    yield name, ref, standin, dev, blob, grads
    del dev
    torch.cuda.empty_cache()


def test_grads_only_steps_are_bit_equal(case):
    """Checks a-d combine reads of separate steps (a full one, and one per debug flag and layer): two grads-only steps
    with the same seed must return the same gradient blob bit for bit, and a step cut short by a debug flag must
    leave what it did compute (here: everything after d_deconv3's BN backward) equal to the full step's."""
    name, ref, _, dev, blob, grads = case
    assert np.isfinite(blob).all()
    dev.step()
    again = dev.blob()
    assert np.array_equal(blob.view(np.uint32), again.view(np.uint32))
    from avse_amd.model import KerasModel
    i = R.NAMES.index("d_deconv3")
    dev.step(dev._lib.AVSE_TRAIN_DEBUG_STOP | (i << 8))
    part = KerasModel.from_blob(dev.blob(), dev.c["T"], dev.c["F"]).tensors
    for n in R.NAMES[i + 1:]:
        for k in ("/kernel", "/bias"):
            assert np.array_equal(part[n + k], grads[n + k]), n + k
    assert np.array_equal(part["d_deconv3_bn/gamma"], grads["d_deconv3_bn/gamma"])
    assert not np.any(part["d_deconv2/kernel"])


def test_dz_read_covers_the_whole_scratch(case):
    """avse_trainer_read(AVSE_TRAIN_DEBUG_DZ) is bounded by the dz scratch (the largest pre-pool z of a max_batch
    batch: v_conv1's, 33.5M floats at 16 clips, more than the 18.6M parameters), not by the parameter count."""
    name, ref, _, dev, _, _ = case
    L = dev._lib
    i = R.NAMES.index("v_conv1")
    most = ref.z_floats(i) // dev.N * dev.c["max_batch"]
    out = np.empty(most + 1, np.float32)
    read = lambda n: L.load().avse_trainer_read(dev.tr.handle, L.AVSE_TRAIN_DEBUG_DZ,               # noqa: E731
                                                 out.ctypes.data_as(ctypes.c_void_p), n)
    assert read(most) == 0
    assert read(most + 1) != 0
    assert read(-1) != 0


@pytest.mark.parametrize("layer", R.NAMES)
def test_layer_backward_matches_local_reference(case, layer):
    name, ref, standin, dev, _, grads = case
    i = R.NAMES.index(layer)
    q = {"dz": dev.dz(i), "dW": grads[layer + "/kernel"], "dbias": grads[layer + "/bias"]}
    if ref.layers[i].bn:
        q["g_out"] = ref.g_out_of(i, dev.gin)
        q["ghat"] = dev.ghat(i)
        q["dgamma"], q["dbeta"] = grads[layer + "_bn/gamma"], grads[layer + "_bn/beta"]
    if i not in R.NO_DGRAD:
        q["gin"] = dev.gin(i)
    calib = R.check_layer(ref, i, standin[i])
    err = R.check_layer(ref, i, q)
    print(f"\n{name:3s} {layer:11s} " + "  ".join(
        f"{k} {err[k]:.2e} (stand-in {calib[k]:.2e}, gate {R.gate(calib[k]):.1e})" if k in R.GATED
        else f"{k} {err[k]:.2e} ({calib[k]:.2e})" for k in err))
    assert set(err) == set(calib)
    R.assert_within_gates(f"{name} {layer}", err, calib)
