"""Float64 layer-local reference of the training backward pass — TEST INFRASTRUCTURE ONLY (a helper module, like
isa_forms.py; tests/test_train_local_ref.py checks it on the CPU, tests/test_gpu_train_local.py uses it on the device).

End to end, a gradient can only be compared with float64 autograd at ~1e-2: a BN output within float32 rounding of zero
takes the other LeakyReLU slope (or a pool tie the other winner) and the change reaches every upstream gradient.  Given
their inputs, though, every backward stage is linear, or elementwise with a known mask.  LocalRef runs the float64
training forward once (geometry of oracle/keras_ref.py and oracle/keras_train_ref.py: TF 'SAME' pads, transposed-conv
crop, HWC flatten, audio-first concat, dec_dense2 -> Reshape(5, W5, 128) with BN over the 128) and keeps, per layer,
its input x, pre-BN z, xhat, batch mean and inv, and the bit-exact dropout scale.  For layer i it then offers

    act_bwd(i, g_out)     -> (ghat, ambiguous)   LeakyReLU slope, 2x2 pool winner, dropout scale
    bn_bwd(i, ghat)       -> (dgamma, dbeta, dz) Keras training-mode BN backward (biased variance, eps 1e-3)
    param_grads(i, dz)    -> (dW, dbias)         from the oracle's x and the given dz
    input_grad(i, dz)     -> dL/dx

each a pure float64 function of its arguments, so a float32 implementation fed ITS OWN upstream quantity can be held
to float32 rounding per stage (check_layer), and no flip leaks from one stage into the next.

Arrays are numpy float64, NHWC without channel padding: z / ghat / dz [N, hq, wq, cout] at the full pre-pool
resolution, g_out [N, ho, wo, cout] (after the pool), x / dL/dx [N, hin, win, cin]; dense layers [N, features]
(dec_dense2's 3200 features are Reshape's (5, W5, 128) row-major, so its BN rows are reshape(-1, 128)).
unpack_z / unpack_gin turn the trainer's debug reads (channel stride zc resp. cin_pad) into these.
"""
import numpy as np
import torch
import torch.nn.functional as F

from forward_local_ref import negated_gammas
from oracle import keras_ref as K
from oracle import keras_train_ref as KT

ALPHA = K.LRELU_ALPHA
AMBIGUOUS_TAU = 1e-3          # x the RMS of the layer's BN output
AMBIGUOUS_SHARE = 1e-2        # at most this share of a layer's elements (windows) may be ambiguous
GATE_FLOOR, GATE_FACTOR, GATE_CEILING = 1e-5, 8.0, 5e-4

LAYERS = ([(n, "conv", s, True, False) for n, _, _, _, s, _, _, _ in K.AUDIO_ENCODER]
          + [(n, "conv", s, True, True) for n, _, _, _, s, _, _, _ in K.VIDEO_ENCODER]
          + [(n, "dense", (1, 1), True, False) for n in ("enc_dense", "dec_dense1", "dec_dense2")]
          + [(n, "deconv", s, bn, False) for n, _, _, _, s, bn, _, _ in K.AUDIO_DECODER])
NAMES = [L[0] for L in LAYERS]
assert NAMES == sorted(KT.LAYER_INDEX, key=KT.LAYER_INDEX.get)
NO_DGRAD = (NAMES.index("a_conv1"), NAMES.index("v_conv1"))     # the first layer of a branch: its input is data
ENC_DENSE = NAMES.index("enc_dense")


# The cases of tests/test_gpu_train_local.py (n3, n2 and n3s also run on the CPU, tests/test_train_local_ref.py):
#   n3   every row count a ragged multiple for rows_per_split and colred_grid; 3 clips give train_split its short grids
#   n2   the other plan ((80, 24) / (128, 128, 6)), with the row-run v_conv1 shapes, no dropout
#   n16  the reference's fit batch: wg_splits, k_wgrad_nat's 2048-row cap and the column-reduction grids change here
#   n3s  n3 with every BatchNormalization gamma negated on channels 1::3 (forward_local_ref.negated_gammas), as a
#        trained checkpoint may hold: the forward's sign handling, dgamma and dz with gamma < 0.  No zero gammas: a
#        constant channel ties every pool window, and the ambiguous share would measure the input, not the kernel
CASES = {
    "n3": dict(N=3, rate=0.25, T=20, F=5, max_batch=8, model_seed=21, data_seed=8, drop_seed=1234),
    "n3s": dict(N=3, rate=0.25, T=20, F=5, max_batch=8, model_seed=21, data_seed=8, drop_seed=1234, signed=True),
    "n2": dict(N=2, rate=0.0, T=24, F=6, max_batch=8, model_seed=21, data_seed=7, drop_seed=1234),
    "n16": dict(N=16, rate=0.25, T=20, F=5, max_batch=16, model_seed=21, data_seed=21, drop_seed=1234),
}


def case_inputs(case):
    """(model, mel, video, target) of a case: KerasModel.init(seed, randomize=True), inputs as test_gpu_train.batch."""
    from avse_amd.model import KerasModel
    c = CASES[case]
    model = KerasModel.init(seed=c["model_seed"], randomize=True, audio_shape=(80, c["T"]), video_shape=(128, 128, c["F"]))
    if c.get("signed"):
        negated_gammas(model)
    rng = np.random.default_rng(c["data_seed"])
    mel = rng.normal(-40, 12, (c["N"], 80, c["T"])).astype(np.float32)
    video = rng.normal(0, 1, (c["N"], 128, 128, c["F"])).astype(np.float32)      # normalised crops
    target = (mel + rng.normal(0, 3, mel.shape)).astype(np.float32)
    return model, mel, video, target


def rel_rms(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-300))


def pre_bn_bias(i):
    """Biases whose true gradient is exactly zero: a BatchNormalization over the same channels follows the layer
    (dec_dense2's bias is per feature of the 3200-vector, its BN per channel of the Reshape: not zero)."""
    return NAMES[i] not in ("d_deconv6", "dec_dense2")


def gate(standin_error):
    """The bound of one (layer, check): the float32 stand-in's own error on it, x 8, floor 1e-5 — and never above the
    5e-4 ceiling.  The ceiling binds in one place, dz (and what the forward's rounding leaves of it downstream) of the
    dense BatchNormalizations at N = 2: with M = 2 rows xhat = +-a, a^2 = d^2 / (d^2 + eps), and
    dz = gamma inv (g - mean g - xhat mean(g xhat)) = +-gamma inv delta (1 - a^2) cancels to eps / (d^2 + eps) ~ 1e-3 of
    its terms, so float32 lands at ~1e-7 / 1e-3 whatever the seed (stand-in 2.9e-4 .. 4.2e-4 over 12 seed pairs).
    There the gate is the ceiling itself, less than 2 x the stand-in's own error."""
    return min(GATE_CEILING, max(GATE_FLOOR, GATE_FACTOR * standin_error))


def _nhwc(t):
    t = t.detach().double()
    return (t.permute(0, 2, 3, 1) if t.dim() == 4 else t).contiguous().numpy()


def _windows(a):
    """[N, H, W, C] -> [N, H/2, W/2, C, 4], window entry e = 2 * dy + dx (k_act_bwd's scan order)."""
    N, H, W, C = a.shape
    return a.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)


def _unwindows(w):
    N, Ho, Wo, C, _ = w.shape
    return w.reshape(N, Ho, Wo, C, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(N, 2 * Ho, 2 * Wo, C)


class _Layer:
    pass


class LocalRef:
    def __init__(self, tensors, mel, video, target, rate=0.25, seed=0):
        dt = torch.float64
        p = {n: torch.tensor(np.asarray(a, np.float64), dtype=dt, requires_grad=n.endswith(("/kernel", "/bias")))
             for n, a in tensors.items()}
        self.N = N = int(np.shape(mel)[0])
        self.layers = []
        a = np.asarray(mel, np.float64)[..., None]            # NHWC
        v = np.asarray(video, np.float64)
        cur, audio_emb = a, None
        for i, (name, kind, s, has_bn, pool) in enumerate(LAYERS):
            L = _Layer()
            L.name, L.kind, L.stride, L.bn, L.pool = name, kind, s, has_bn, pool
            L.W, L.b = p[name + "/kernel"], p[name + "/bias"]
            if name == "v_conv1":
                audio_emb, cur = cur, v
            if name == "enc_dense":                           # Flatten is NHWC row-major; audio first (network.py:53)
                self.aemb_shape = audio_emb.shape
                cur = np.concatenate([audio_emb.reshape(N, -1), cur.reshape(N, -1)], axis=1)
            L.in_shape = cur.shape
            xt = torch.from_numpy(np.ascontiguousarray(cur))
            L.x = (xt.permute(0, 3, 1, 2) if kind != "dense" else xt).contiguous().requires_grad_(True)
            L.z = self._op(L, L.x)
            z = _nhwc(L.z)
            L.z_shape = z.shape
            L.cout = z.shape[-1]
            if not has_bn:
                cur = z
                self.layers.append(L)
                continue
            L.C = C = 128 if name == "dec_dense2" else L.cout
            zm = z.reshape(-1, C)
            L.M = zm.shape[0]
            L.mean = zm.mean(axis=0)
            L.var = ((zm - L.mean) ** 2).mean(axis=0)          # biased (tf.nn.moments)
            L.inv = 1.0 / np.sqrt(L.var + K.BN_EPS)
            L.xhat = (zm - L.mean) * L.inv
            L.gamma = np.asarray(tensors[name + "_bn/gamma"], np.float64)
            L.beta = np.asarray(tensors[name + "_bn/beta"], np.float64)
            yh = self.bn_out(L)
            L.tau = AMBIGUOUS_TAU * float(np.sqrt(np.mean(yh ** 2)))
            y = np.where(yh >= 0, yh, ALPHA * yh).reshape(z.shape)
            L.drop = None
            if pool:
                y = _windows(y).max(axis=-1)
                L.drop = KT.dropout_scale(seed, i, y.shape, rate)
                y = y * L.drop
            if name == "dec_dense2":
                y = y.reshape(self.aemb_shape)
            cur = y
            self.layers.append(L)
        self.y = cur[..., 0]
        t = np.asarray(target, np.float64)
        self.loss = float(np.mean((self.y - t) ** 2))
        self.dLdy = (2.0 * (self.y - t) / t.size)[..., None]   # dz of d_deconv6 (no BN): 2 (y - t) / n

    # ---- the four layer-local operators ---------------------------------------------------------------------
    @staticmethod
    def _op(L, x):
        if L.kind == "dense":
            return x @ L.W + L.b
        kh, kw = L.W.shape[:2]
        s = L.stride
        w = L.W.permute(3, 2, 0, 1)
        if L.kind == "conv":
            pt, pb = K._same_pads(x.shape[2], kh, s[0])
            pl, pr = K._same_pads(x.shape[3], kw, s[1])
            return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, L.b, stride=s)
        H, Wd = x.shape[2], x.shape[3]
        y = F.conv_transpose2d(x, w, L.b, stride=s)
        pt, pl = max(kh - s[0], 0) // 2, max(kw - s[1], 0) // 2
        return y[:, :, pt:pt + H * s[0], pl:pl + Wd * s[1]]

    @staticmethod
    def bn_out(L):
        """[M, C] BN output of the float64 forward."""
        return L.xhat * L.gamma + L.beta

    def _zt(self, L, dz):
        dz = np.ascontiguousarray(np.asarray(dz, np.float64).reshape(L.z_shape))
        t = torch.from_numpy(dz)
        return t.permute(0, 3, 1, 2) if L.kind != "dense" else t

    def act_bwd(self, i, g_out):
        """dL/d(BN output) from dL/d(layer output): (ghat, ambiguous), both shaped like z.  An element is ambiguous
        when |BN output| <= tau; a pool window (all four of its elements) when the gap between its two largest
        LeakyReLU values <= tau or its winner's |BN output| <= tau; tau = 1e-3 x the RMS of the layer's BN output."""
        L = self.layers[i]
        yh = self.bn_out(L).reshape(L.z_shape)
        if not L.pool:
            g = np.asarray(g_out, np.float64).reshape(L.z_shape)
            return g * np.where(yh >= 0, 1.0, ALPHA), np.abs(yh) <= L.tau
        yw = _windows(yh)
        lw = np.where(yw >= 0, yw, ALPHA * yw)
        win = np.argmax(lw, axis=-1)[..., None]               # the first maximum, as MaxPooling's gradient
        top = np.sort(lw, axis=-1)
        yh_win = np.take_along_axis(yw, win, -1)[..., 0]
        g = np.asarray(g_out, np.float64).reshape(L.drop.shape) * L.drop
        gw = np.zeros_like(yw)
        np.put_along_axis(gw, win, (g * np.where(yh_win >= 0, 1.0, ALPHA))[..., None], -1)
        amb = ((top[..., -1] - top[..., -2]) <= L.tau) | (np.abs(yh_win) <= L.tau)
        return _unwindows(gw), _unwindows(np.broadcast_to(amb[..., None], yw.shape))

    def bn_bwd(self, i, ghat):
        """(dgamma, dbeta, dz): y = gamma xhat + beta over M rows, xhat from the batch mean and biased variance."""
        L = self.layers[i]
        g = np.asarray(ghat, np.float64).reshape(-1, L.C)
        dbeta = g.sum(axis=0)
        dgamma = (g * L.xhat).sum(axis=0)
        dz = L.gamma * L.inv * (g - dbeta / L.M - L.xhat * (dgamma / L.M))
        return dgamma, dbeta, dz.reshape(L.z_shape)

    def param_grads(self, i, dz):
        """(dW, dbias) in the Keras layouts, from the oracle's x and the given dz."""
        L = self.layers[i]
        gw, gb = torch.autograd.grad(L.z, [L.W, L.b], self._zt(L, dz), retain_graph=True)
        return gw.numpy().copy(), gb.numpy().copy()

    def input_grad(self, i, dz):
        L = self.layers[i]
        gx, = torch.autograd.grad(L.z, [L.x], self._zt(L, dz), retain_graph=True)
        return _nhwc(gx)

    # ---- device layouts -------------------------------------------------------------------------------------
    def zc(self, i):
        """Channel stride of the trainer's z / dz / ghat: cout rounded up to 8, dense layers unpadded."""
        L = self.layers[i]
        return L.cout if L.kind == "dense" else -(-L.cout // 8) * 8

    def z_floats(self, i):
        L = self.layers[i]
        return int(np.prod(L.z_shape[:-1])) * self.zc(i)

    def unpack_z(self, i, flat):
        L = self.layers[i]
        a = np.asarray(flat, np.float64).reshape(L.z_shape[:-1] + (self.zc(i),))
        return np.ascontiguousarray(a[..., :L.cout])

    def cin_pad(self, i):
        L = self.layers[i]
        return L.in_shape[-1] if L.kind == "dense" else -(-L.in_shape[-1] // 8) * 8

    def gin_floats(self, i):
        L = self.layers[i]
        return int(np.prod(L.in_shape[:-1])) * self.cin_pad(i)

    def unpack_gin(self, i, flat):
        """N x in_clip with pixel stride cin_pad -> [N, hin, win, cin]; enc_dense: the [N, cat] concat, audio first."""
        L = self.layers[i]
        a = np.asarray(flat, np.float64).reshape(L.in_shape[:-1] + (self.cin_pad(i),))
        return np.ascontiguousarray(a[..., :L.in_shape[-1]])

    def g_out_of(self, i, gin):
        """dL/d(output of layer i) from gin(j) = the input gradient of layer j (a callable): the next layer's, for
        a_conv5 and v_conv6 their slices of enc_dense's, audio first."""
        if NAMES[i] in ("a_conv5", "v_conv6"):
            g = gin(ENC_DENSE)
            na = int(np.prod(self.aemb_shape[1:]))
            return g[:, :na] if NAMES[i] == "a_conv5" else g[:, na:]
        return gin(i + 1)


def standin(tensors, mel, video, target, rate, seed):
    """The float32 stand-in for the device: oracle/keras_train_ref.gradients in torch-CPU float32 with every layer's
    x, z and BN output tapped.  Returns (loss, [per-layer quantities for check_layer])."""
    taps = {}
    loss, grads, _ = KT.gradients(tensors, mel, video, target, rate=rate, seed=seed, dtype=torch.float32, taps=taps)
    gin = lambda j: _nhwc(taps[NAMES[j]][0].grad)                                           # noqa: E731
    out = []
    for i, name in enumerate(NAMES):
        x, z, y = taps[name]
        q = {"dz": _nhwc(z.grad), "dW": grads[name + "/kernel"], "dbias": grads[name + "/bias"]}
        if y is not None:
            q["ghat"] = _nhwc(y.grad) if name != "dec_dense2" else y.grad.double().reshape(z.shape).numpy()
            q["dgamma"], q["dbeta"] = grads[name + "_bn/gamma"], grads[name + "_bn/beta"]
        if i not in NO_DGRAD:
            q["gin"] = gin(i)
        out.append(q)
    na = int(np.prod(taps["a_conv5"][1].shape[1:]))
    for i, q in enumerate(out):             # g_out: the next layer's input gradient (a_conv5 / v_conv6: enc_dense's)
        if "ghat" not in q:
            continue
        if NAMES[i] in ("a_conv5", "v_conv6"):
            g = out[ENC_DENSE]["gin"]
            q["g_out"] = g[:, :na] if NAMES[i] == "a_conv5" else g[:, na:]
        else:
            q["g_out"] = out[i + 1]["gin"]
    return loss, out


def check_layer(ref, i, q, log=None):
    """Checks a-d of one layer on quantities q (arrays as described in the module docstring):
         a  ghat                   against act_bwd(i, g_out)           needs g_out, ghat
         b  dgamma, dbeta, dz      against bn_bwd(i, ghat)             needs ghat, dz, dgamma, dbeta
         c  dW, dbias              against param_grads(i, dz)          needs dz, dW, dbias
         d  gin                    against input_grad(i, dz)           needs dz, gin
    each expectation computed from q's OWN upstream quantity.  Returns {check: relative RMS error}; the structural
    conditions of check a (ambiguous share, ambiguous elements within the two slopes, one entry per pool window) are
    asserted here.  Pre-BN biases (true gradient exactly zero) are measured absolutely:
    RMS_c(dbias - sum dz) / RMS_c(sum |dz|)."""
    L = ref.layers[i]
    err = {}
    if "ghat" in q and "g_out" in q:
        want, amb = ref.act_bwd(i, q["g_out"])
        got = np.asarray(q["ghat"], np.float64).reshape(want.shape)
        share = float(amb.mean())
        err["a:ambiguous_share"] = share
        assert share <= AMBIGUOUS_SHARE, f"{L.name}: ambiguous share {share:.3e} > {AMBIGUOUS_SHARE}"
        keep = ~amb
        err["a:ghat"] = rel_rms(got[keep], want[keep])
        if L.pool:
            gw, ambw = _windows(got), _windows(amb)[..., 0]
            assert int((np.count_nonzero(gw, axis=-1) > 1).sum()) == 0, f"{L.name}: a pool window with two gradient entries"
            gs = np.abs(np.asarray(q["g_out"], np.float64).reshape(L.drop.shape) * L.drop)[ambw]
            tot = np.abs(gw).sum(axis=-1)[ambw]
        else:
            gs = np.abs(np.asarray(q["g_out"], np.float64).reshape(want.shape))[amb]
            tot = np.abs(got)[amb]
        bad = (tot < ALPHA * gs * (1 - 1e-6)) | (tot > gs * (1 + 1e-6))
        assert not bad.any(), f"{L.name}: {int(bad.sum())} ambiguous elements outside [0.3, 1] x |g_out x dropout scale|"
    if "ghat" in q and "dz" in q and L.bn:
        dgamma, dbeta, dz = ref.bn_bwd(i, q["ghat"])
        err["b:dgamma"] = rel_rms(q["dgamma"], dgamma)
        err["b:dbeta"] = rel_rms(q["dbeta"], dbeta)
        err["b:dz"] = rel_rms(np.asarray(q["dz"]).reshape(dz.shape), dz)
    if "dW" in q:
        dW, dbias = ref.param_grads(i, q["dz"])
        err["c:dW"] = rel_rms(q["dW"], dW)
        err["c:dbias"] = bias_error(i, q["dbias"], q["dz"], dbias)
    if "gin" in q:
        want = ref.input_grad(i, q["dz"])
        err["d:gin"] = rel_rms(np.asarray(q["gin"]).reshape(want.shape), want)
    if log is not None:
        log(f"{L.name:11s} " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    return err


def bias_error(i, dbias, dz, want):
    """Relative RMS against `want` (= the float64 sum of dz), or, for a pre-BN bias, absolute against it on the scale
    of sum |dz|."""
    if not pre_bn_bias(i):
        return rel_rms(dbias, want)
    scale = np.abs(np.asarray(dz, np.float64)).reshape(-1, np.size(want)).sum(axis=0)
    return float(np.sqrt(np.mean((np.asarray(dbias, np.float64) - want) ** 2)) / max(np.sqrt(np.mean(scale ** 2)), 1e-300))


GATED = ("a:ghat", "b:dgamma", "b:dbeta", "b:dz", "c:dW", "c:dbias", "d:gin")


def assert_within_gates(name, err, calib):
    """err within gate(the stand-in's error) per check."""
    bad = {}
    for k in GATED:
        if k not in err:
            assert k not in calib, (name, k)
            continue
        g = gate(calib[k])
        if not err[k] <= g:
            bad[k] = (err[k], g)
    assert not bad, f"{name}: (error, gate) {bad}"
