"""Float64 layer-local reference of the bf16 inference forward — TEST INFRASTRUCTURE ONLY (a helper module, like
train_local_ref.py; tests/test_forward_local_ref.py checks it on the CPU, tests/test_gpu_forward_local.py and
tests/test_gpu_forward_signed.py use it on the device).

Over a whole tensor a bf16 layer can only be held to a relative RMS of ~1e-2 (test_gpu_forward.BF16_LAYER_REL): the
output rounding alone is 2^-9 per element, and a tap dropped at one tile corner (2e-3 of v_conv2) or a channel taking
its neighbour's shift (under 1.5e-2 for 98 of v_conv3's 256 channels) disappear in it; one halo column of one tile read
as zero costs 3e-2 at two clips and sinks below the gate with a few more.  Given its input, though, a layer is a fixed sum of exact
products: bf16 x bf16 is exact in fp32, so all the device adds to the float64 value is (a) its fp32 accumulation and
epilogue error and (b) one final round-to-nearest to bf16.  LocalRef offers, per layer i of a (T, F) plan,

    layer(i, x)     the float64 layer (conv / deconv / dense, BN fold, LeakyReLU, 2x2 pool) on a given input x; the
                    kernel rounded to bf16 as weight_pack.cpp f2bf does (round to nearest even), scale and shift as its
                    fold_bn, in float64.  d_deconv6's 64 weights stay float32: the device keeps them so (weights.hip)
    abs_sum(i, x)   per output element S = |scale| . sum |w| |x| + |shift|, for pooled layers the largest S of the window
    standin(i, x)   the same layer in torch-CPU float32, the result rounded to bf16 (d_deconv6: float32, as the device)
    excess(got, ref, S)   per element E = max(0, |got - ref| - 1/2 ulp_bf16(max(|got|, |ref|))) / (2^-24 S)

The 1/2 ulp is exact arithmetic, not a tolerance: the device rounds an fp32 value that lies within its accumulation
error of ref.  E is that accumulation error in units of ONE fp32 rounding of the absolute sum.  The gate of one (case,
layer) is gate(stand-in's max E, K) = min(K, max(1, 8 x stand-in)): the stand-in is what float32 accumulation costs, the
factor 8 is train_local_ref.GATE_FACTOR (another summation order, the matrix cores' internal accumulation), and K, the
layer's reduction length, bounds the error of ANY fp32 summation order: beyond it the result is wrong by arithmetic.
One dropped tap is E ~ 2^24 / K, thousands.

Fused per-clip kernels never materialise their inner layers: chain(first, last, x) applies layer in sequence with a
round to bf16 after each inner layer, chain_standin the same in float32.  An inner rounding can flip (the fp32 value
lies across a bf16 rounding boundary from the float64 one); the flipped activation is one bf16 ulp off, and the last
layer's result moves by |scale w| x that ulp — any number of ulps of an output that cancels to near zero (the stand-in
chain itself needs 400 ulps on a_conv1..a_conv5, tests/test_forward_local_ref.py), and d_deconv6's float32 output has
no ulp term at all.  A widened ulp term therefore cannot express it.  chain instead carries, per inner element, the
exact interval the device's activation can lie in (its docstring) and returns rho, the most the last layer's result
can move for it: zero wherever no inner rounding in the element's receptive field can flip.  E of a chain is
excess(got, ref, S, slack=rho), held to the last layer's own gate.

Arrays are numpy float64, NHWC: conv / deconv layers [N, H, W, C], dense layers [N, features]; dec_dense2 returns
Reshape's [N, 5, W5, 128], the arena's layout.  inputs_of(i, outs) names the input of a layer among the materialised
buffers (enc_dense reads concat = [a_conv5 | v_conv6] flattened, audio first).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import keras_ref as K

ALPHA = K.LRELU_ALPHA
GATE_FACTOR = 8.0              # train_local_ref.GATE_FACTOR
EPS24 = 2.0 ** -24

LAYERS = ([(n, "conv", s, True, False) for n, _, _, _, s, _, _, _ in K.AUDIO_ENCODER]
          + [(n, "conv", s, True, True) for n, _, _, _, s, _, _, _ in K.VIDEO_ENCODER]
          + [(n, "dense", (1, 1), True, False) for n in ("enc_dense", "dec_dense1", "dec_dense2")]
          + [(n, "deconv", s, bn, False) for n, _, _, _, s, bn, _, _ in K.AUDIO_DECODER])
NAMES = [L[0] for L in LAYERS]
A1, V1, ENC_DENSE, D1, D6 = (NAMES.index(n) for n in ("a_conv1", "v_conv1", "enc_dense", "d_deconv1", "d_deconv6"))

# the arena's buffers (csrc/forward_plan.h Buf), in its order; per-clip shapes from buf_shapes(T, F)
BUF_NAMES = ["video_in", "audio_in", "a_conv1", "a_conv2", "a_conv3", "a_conv4", "v_conv1", "v_conv2", "v_conv3",
             "v_conv4", "v_conv5", "concat", "enc_dense", "dec_dense1", "dec_dense2", "d_deconv1", "d_deconv2",
             "d_deconv3", "d_deconv4", "d_deconv5"]


def buf_shapes(T=20, F=5):
    """Per-clip shapes of the forward arena's buffers for the (80, T) / (128, 128, F) network (forward_plan.h
    buf_elems): the audio widths follow T (w1 = ceil(T / 2), w3 = ceil(w1 / 2)), the video encoder's never change;
    the two preps pad their channels to 8 whatever F is."""
    w1 = -(-T // 2)
    w3 = -(-w1 // 2)
    aemb = 5 * w3 * 128
    cat = aemb + 2048
    return {"video_in": (128, 128, 8), "audio_in": (80, T, 8), "a_conv1": (40, w1, 64), "a_conv2": (40, w1, 64),
            "a_conv3": (20, w3, 128), "a_conv4": (10, w3, 128), "v_conv1": (64, 64, 128), "v_conv2": (32, 32, 128),
            "v_conv3": (16, 16, 256), "v_conv4": (8, 8, 256), "v_conv5": (4, 4, 512), "concat": (cat,),
            "enc_dense": (cat // 4,), "dec_dense1": (cat // 4,), "dec_dense2": (5, w3, 128), "d_deconv1": (10, w3, 128),
            "d_deconv2": (20, w3, 128), "d_deconv3": (40, 2 * w3, 128), "d_deconv4": (40, 2 * w3, 64),
            "d_deconv5": (80, 4 * w3, 64)}


def signed_model(model):
    """Edit a KerasModel in place: every BatchNormalization gamma x -1 on channels 1::3 and exactly 0 on channels
    5::17 (the zero wins where both apply), and the whole kernel of one output channel zeroed in v_conv3 (a tiled
    layer) and in a_conv3 (a generic one; the split dtype's channel_exponents then takes its all-zero branch).  A
    trained Keras checkpoint may hold any of these; KerasModel.init(randomize=True) draws gamma ~ U(0.5, 1.5) only."""
    t = model.tensors
    for name in list(t):
        if name.endswith("_bn/gamma"):
            g = t[name].copy()
            g[1::3] *= np.float32(-1.0)
            g[5::17] = np.float32(0.0)
            t[name] = g
    for layer, ch in (("v_conv3", 7), ("a_conv3", 10)):
        k = t[layer + "/kernel"].copy()
        k[..., ch] = 0.0
        t[layer + "/kernel"] = k
    return model


def negated_gammas(model):
    """Gammas x -1 on channels 1::3 only (training: a zero gamma makes a constant channel, which ties every pool
    window)."""
    t = model.tensors
    for name in list(t):
        if name.endswith("_bn/gamma"):
            g = t[name].copy()
            g[1::3] *= np.float32(-1.0)
            t[name] = g
    return model


def round_bf16(a):
    """float64 / float32 array -> the nearest bfloat16 (ties to even) of its float32 value, as float64: the integer
    arithmetic of weight_pack.cpp f2bf on finite values."""
    u = np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return (u & 0xffffffff).astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(a))


def ulp_bf16(m):
    """The spacing of bfloat16 at magnitude m >= 0 (8 significant bits; the smallest normal binade below 2^-126)."""
    m = np.asarray(m, np.float64)
    _, e = np.frexp(m)                                  # m = f 2^e, f in [0.5, 1); frexp(0) = (0, 0)
    return np.ldexp(1.0, np.maximum(np.where(m > 0, e - 1, -126), -126) - 7)


def excess(got, ref, S, slack=0.0, ulp=True):
    """E per element (module docstring).  slack: a further exact allowance per element (chain's rho); ulp=False: the
    output is float32 (d_deconv6), no rounding term."""
    got, ref, S = (np.asarray(a, np.float64) for a in (got, ref, S))
    d = np.abs(got - ref) - slack
    if ulp:
        d = d - 0.5 * ulp_bf16(np.maximum(np.abs(got), np.abs(ref)))
    d = np.maximum(0.0, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0, d / (EPS24 * S), 0.0)


def gate(standin_E, K_len):
    return float(min(K_len, max(1.0, GATE_FACTOR * standin_E)))


def _pool(y):
    N, H, W, C = y.shape
    return y.reshape(N, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


class _Layer:
    pass


class LocalRef:
    def __init__(self, tensors):
        """tensors: KerasModel.tensors (Keras layouts, float32)."""
        self.layers = []
        for i, (name, kind, s, has_bn, pool) in enumerate(LAYERS):
            L = _Layer()
            L.name, L.kind, L.stride, L.bn, L.pool = name, kind, s, has_bn, pool
            w = np.asarray(tensors[name + "/kernel"], np.float32)
            L.w_exact = w.astype(np.float64)
            L.w = L.w_exact if i == D6 else round_bf16(w)
            bias = np.asarray(tensors[name + "/bias"], np.float64)
            L.cout = bias.size
            if has_bn:                                              # weight_pack.cpp fold_bn, in float64
                g, b, mu, var = (np.asarray(tensors[f"{name}_bn/{p}"], np.float64)
                                 for p in ("gamma", "beta", "moving_mean", "moving_variance"))
                c = np.arange(L.cout) % g.size                      # dec_dense2: BN over Reshape's 128 channels
                L.scale = g[c] / np.sqrt(var[c] + K.BN_EPS)
                L.shift = (bias - mu[c]) * L.scale + b[c]
            else:
                L.scale, L.shift = np.ones(L.cout), bias
            if kind == "dense":
                L.K = w.shape[0]
            elif kind == "conv":
                L.K = w.shape[0] * w.shape[1] * w.shape[2]
            else:                                                   # taps of one output phase x input channels
                L.K = -(-w.shape[0] // s[0]) * -(-w.shape[1] // s[1]) * w.shape[3]
            self.layers.append(L)

    # ---- the linear part, in any dtype -----------------------------------------------------------------------
    @staticmethod
    def _lin(L, x, w):
        """x [N, H, W, C] (dense: [N, features]) and w in the Keras layout, both torch tensors of one dtype."""
        if L.kind == "dense":
            return x.reshape(x.shape[0], -1) @ w
        x = x.permute(0, 3, 1, 2)
        kh, kw = w.shape[:2]
        s = L.stride
        wt = w.permute(3, 2, 0, 1).contiguous()
        if L.kind == "conv":
            pt, pb = K._same_pads(x.shape[2], kh, s[0])
            pl, pr = K._same_pads(x.shape[3], kw, s[1])
            y = F.conv2d(F.pad(x, (pl, pr, pt, pb)), wt, stride=tuple(s))
        else:
            H, W = x.shape[2], x.shape[3]
            y = F.conv_transpose2d(x, wt, stride=tuple(s))
            pt, pl = max(kh - s[0], 0) // 2, max(kw - s[1], 0) // 2
            y = y[:, :, pt:pt + H * s[0], pl:pl + W * s[1]]
        return y.permute(0, 2, 3, 1)

    def _shape_out(self, L, y):
        if L.name == "dec_dense2":
            return y.reshape(y.shape[0], 5, -1, 128)
        return y

    def _apply(self, L, x, w, scale, shift, dtype, mutate=None, pool_first=False):
        with torch.no_grad():
            xt = torch.as_tensor(np.ascontiguousarray(x), dtype=dtype)
            z = self._lin(L, xt, torch.as_tensor(np.ascontiguousarray(w), dtype=dtype))
            if mutate is not None:                  # a seeded defect on the pre-BN sums (tests/test_forward_local_ref.py)
                z = torch.as_tensor(mutate(z.numpy().copy()), dtype=dtype)
            if pool_first:                          # the tiled kernels' order: pool the raw sums, then one FMA
                z = torch.as_tensor(_pool(z.numpy()), dtype=dtype)
            y = z * torch.as_tensor(scale, dtype=dtype) + torch.as_tensor(shift, dtype=dtype)
            if L.bn:
                y = torch.where(y >= 0, y, torch.as_tensor(ALPHA, dtype=dtype) * y)
            y = y.numpy()
        if L.pool and not pool_first:
            y = _pool(y)
        return self._shape_out(L, y)

    # ---- the four operators ----------------------------------------------------------------------------------
    def layer(self, i, x, round_w=True):
        L = self.layers[i]
        return self._apply(L, np.asarray(x, np.float64), L.w if round_w else L.w_exact, L.scale, L.shift, torch.float64)

    def spread(self, i, r):
        """Per output element the most the layer's result can move when input element j moves by at most r_j >= 0:
        |scale| . sum |w| r (LeakyReLU and the pool's max are 1-Lipschitz), for pooled layers the largest of the window."""
        L = self.layers[i]
        with torch.no_grad():
            z = self._lin(L, torch.as_tensor(np.ascontiguousarray(r), dtype=torch.float64), torch.as_tensor(np.abs(L.w))).numpy()
        z = z * np.abs(L.scale)
        return _pool(z) if L.pool else z

    def abs_sum(self, i, x):
        L = self.layers[i]
        S = self.spread(i, np.abs(np.asarray(x, np.float64)))
        return self._shape_out(L, S + np.abs(L.shift))

    def standin(self, i, x, w=None, scale=None, shift=None, mutate=None, pool_first=False):
        """w / scale / shift / mutate / pool_first: a seeded defect in place of the layer's own (CPU tests only)."""
        L = self.layers[i]
        w, scale, shift = (d if o is None else o for o, d in ((w, L.w), (scale, L.scale), (shift, L.shift)))
        y = self._apply(L, np.asarray(x, np.float32), np.asarray(w, np.float32), np.asarray(scale, np.float32),
                        np.asarray(shift, np.float32), torch.float32, mutate, pool_first)
        return y.astype(np.float64) if i == D6 else round_bf16(y)

    # ---- chains (fused kernels) ------------------------------------------------------------------------------
    def chain(self, first, last, x):
        """(ref, S, rho, gate, standin_E) of layers first..last on the input x, the inner activations rounded to bf16.

        Interval arithmetic over the inner roundings: x_i is the float64 chain's bf16 activation, rho_i >= 0 bounds how
        far the device's can lie from it.  With v = layer(i, x_i), the device's fp32 value lies within
        spread(i, rho_i) + g_i 2^-24 S_i of v (g_i: layer i's own gate on x_i), rounding is monotone, so its bf16
        activation lies between the roundings of the interval's ends: rho_{i+1} is the larger distance of the two from
        round(v) — zero wherever the whole interval rounds to one value, i.e. almost everywhere.  The last layer's
        spread(rho) is returned as rho: excess(got, ref, S, slack=rho) <= gate is then exact arithmetic again."""
        x = np.asarray(x, np.float64)
        rho = np.zeros_like(x)
        for i in range(first, last + 1):
            L = self.layers[i]
            v, S = self.layer(i, x), self.abs_sum(i, x)
            cal = float(excess(self.standin(i, x), v, S, ulp=i != D6).max())
            g = gate(cal, L.K)
            r = self._shape_out(L, self.spread(i, rho))
            if i == last:
                return v, S, r, g, cal
            w = r + g * EPS24 * S
            xn = round_bf16(v)
            rho = np.maximum(round_bf16(v + w) - xn, xn - round_bf16(v - w))
            x = xn

    def chain_standin(self, first, last, x):
        x = np.asarray(x, np.float64)
        for i in range(first, last + 1):
            x = self.standin(i, x)
        return x


def inputs_of(i, outs, mel=None, video=None):
    """The input of layer i: `outs` maps buffer names (BUF_NAMES; plus 'a_conv5' / 'v_conv6' where concat is not given)
    to [N, ...] arrays; the first layers read mel [N, 80, T] / video [N, 128, 128, F]."""
    if i == A1:
        return np.asarray(mel, np.float64)[..., None]
    if i == V1:
        return np.asarray(video, np.float64)
    if i == ENC_DENSE:
        if "concat" in outs:
            return outs["concat"]
        N = outs["a_conv5"].shape[0]
        return np.concatenate([outs["a_conv5"].reshape(N, -1), outs["v_conv6"].reshape(N, -1)], axis=1)
    return outs[NAMES[i - 1]]


def forward_chain(ref, mel, video, round_w=False):
    """Every layer's float64 output by chaining LocalRef.layer without any activation rounding (K.forward's
    intermediates when round_w is False)."""
    outs = {}
    for i, name in enumerate(NAMES):
        outs[name] = ref.layer(i, inputs_of(i, outs, mel, video), round_w=round_w)
        if i == ENC_DENSE - 1:
            outs["concat"] = inputs_of(ENC_DENSE, {k: outs[k] for k in ("a_conv5", "v_conv6")})
    return outs
