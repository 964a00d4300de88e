"""CPU emulation: output error of fp32-accurate split-bf16 arithmetic schemes for the video convolutions, against
the float64 oracle, next to the plain-fp32 scheme — which scheme can carry the north star's 1e-4 absolute RMS bound
on dB-scale outputs (DESIGN.md §3 "split-bf16").  Every conv is evaluated in float64 over the products the scheme
keeps (products of bf16 pieces are exact in float64), its output rounded to float32 like an fp32 accumulator + fp32
epilogue; so the differences between schemes are representation / dropped-product errors, not accumulation order.

    python tools/split_err.py [N] [seed]
    python tools/split_err.py [N] [seed] groupings    # the stream kernels' two MFMA groupings, accumulation order included

"groupings" emulates v_conv2..v_conv5 as conv_stream.hip runs them in the split dtype, under the MFMA accumulation
model (one v_mfma_f32_16x16x32_f16 sums its 32 products exactly and rounds once into the fp32 accumulator): K-slices of
16 channels in the kernel's order (slice = chunk * KS^2 + tap), taken in pairs t, t+1 with three roundings per pair:
    pair:   [Ah Bh + Al Bh](t) | [Ah Bh + Al Bh](t+1) | Ah Bl (t) + Ah Bl (t+1)
    planar: Ah Bh (t) + Ah Bh (t+1) | Al Bh (t) + Al Bh (t+1) | Ah Bl (t) + Ah Bl (t+1)
(v_conv1 keeps the fp16x3 scheme above in both.)

    python tools/split_err.py [N] [seed] generic      # the generic layers' two forms, accumulation order included

"generic" emulates the layers that run on gemm.hip k_gemm (v_conv6, enc_dense, dec_dense1, dec_dense2) and on the fused
decoder tail conv_dects.hip (d_deconv4, d_deconv5) under the same MFMA accumulation model, with 16-k slabs in each
kernel's K order, k_conv's blocked summation (8 slabs from zero, then into the running sum), the dense layers' split-K
plan (gemm_s16_ksplit: groups of blocks per split, the splits added in order) and activations passed on as f16 pairs:
    four:   slab by slab, [Ah Wh + Al Wh](t) | [Ah Wl + Al Wl](t)                            (two roundings per slab)
    three:  slab pairs,   Ah Wh (t, t+1) | Al Wh (t, t+1) | Ah Wl (t, t+1)                   (three roundings per pair)
(the tail takes Al Wh first).  The layers before v_conv6 and a_conv5's embedding come from the float64 oracle rounded
to float32, d_deconv1..3 and d_deconv6 are float64 on float32-rounded inputs: the figures isolate the two kernels' forms.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import avse_pkg  # noqa: E402

avse_pkg.load()
from avse_amd.model import KerasModel  # noqa: E402
from oracle import keras_ref as K  # noqa: E402
from oracle import librosa_ref as R  # noqa: E402
from conftest import synth_audio, synth_video  # noqa: E402


def split(t, n, dt=torch.bfloat16):
    """t (float64 holding float32 values) -> n pieces of dtype dt, t ~= sum(pieces) (each piece rounds the residual)."""
    out, r = [], t
    for _ in range(n):
        p = r.to(dt).to(torch.float64)
        out.append(p)
        r = r - p
    return out


SCHEMES = {
    # name: (pieces of x, pieces of w, kept (i, j) products)
    "fp32": None,
    "bf16x9": (3, 3, [(i, j) for i in range(3) for j in range(3)]),
    "bf16x6": (3, 3, [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]),
    "bf16x5-nomm": (3, 3, [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0)]),
    "bf16x5-a2": (2, 3, [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2)]),
    "bf16x4-a2": (2, 3, [(0, 0), (0, 1), (1, 0), (0, 2)]),
    "bf16x3": (2, 2, [(0, 0), (0, 1), (1, 0)]),
    "fp16x3": (2, 2, [(0, 0), (0, 1), (1, 0)], torch.float16, True),
    "fp16x3-noscale": (2, 2, [(0, 0), (0, 1), (1, 0)], torch.float16, False),
    "fp16x4": (2, 2, [(0, 0), (0, 1), (1, 0), (1, 1)], torch.float16, True),
}


def make_conv(scheme, layers):
    orig = K.conv_same

    def conv(x, kernel, bias, strides, dtype):
        kh, kw, cin, cout = kernel.shape
        is_video = x.shape[2] >= 4 and x.shape[2] == x.shape[3] and x.shape[2] in (128, 64, 32, 16, 8, 4)
        name = {128: "v_conv1", 64: "v_conv2", 32: "v_conv3", 16: "v_conv4", 8: "v_conv5", 4: "v_conv6"}.get(x.shape[2])
        w = torch.as_tensor(np.asarray(kernel, np.float32), dtype=torch.float64)
        if scheme is None or not is_video or name not in layers:
            y = orig(x.to(torch.float32).to(torch.float64), w.numpy(), bias, strides, torch.float64)
        else:
            sch = SCHEMES[scheme]
            na, nb, prods = sch[:3]
            dt = sch[3] if len(sch) > 3 else torch.bfloat16
            wsc = 1.0
            if len(sch) > 4 and sch[4]:
                wsc = 2.0 ** (14 - int(np.ceil(np.log2(float(w.abs().max())))))
            xs = split(x.to(torch.float32).to(torch.float64), na, dt)
            ws = [p / wsc for p in split(w * wsc, nb, dt)]
            y = None
            for i, j in prods:
                t = orig(xs[i], ws[j].numpy(), np.zeros_like(bias), strides, torch.float64)
                y = t if y is None else y + t
            y = y + torch.as_tensor(bias, dtype=torch.float64).view(1, -1, 1, 1)
        return y.to(torch.float32).to(torch.float64)
    return conv


def f32(t):
    return t.to(torch.float32).to(torch.float64)


def make_grouped_conv(grouping, fallback):
    """conv_same for v_conv2..v_conv5 with the stream kernels' slice pairs and accumulator roundings."""
    def conv(x, kernel, bias, strides, dtype):
        kh, kw, cin, cout = kernel.shape
        if not (x.shape[2] == x.shape[3] and x.shape[2] in (64, 32, 16, 8) and cin % 16 == 0):
            return fallback(x, kernel, bias, strides, dtype)
        w = torch.as_tensor(np.asarray(kernel, np.float32), dtype=torch.float64)
        # weights x 2^e_n per output channel, max |w| 2^e_n in [2^14, 2^15) (weight_pack.cpp packing)
        wmax = w.abs().amax(dim=(0, 1, 2)).clamp_min(1e-30)
        wsc = torch.pow(2.0, 14 - torch.floor(torch.log2(wmax)))
        wh, wl = split(w * wsc, 2, torch.float16)
        n, _, hh, ww = x.shape
        pad = (kh - 1) // 2
        xh, xl = (F.pad(p, (pad, pad, pad, pad)) for p in split(f32(x), 2, torch.float16))
        ntap = kh * kw

        def prods(t):
            c, tap = divmod(t, ntap)
            ky, kx = divmod(tap, kw)
            cs = slice(16 * c, 16 * c + 16)
            ah = xh[:, cs, ky:ky + hh, kx:kx + ww].permute(0, 2, 3, 1).reshape(-1, 16)
            al = xl[:, cs, ky:ky + hh, kx:kx + ww].permute(0, 2, 3, 1).reshape(-1, 16)
            bh, bl = wh[ky, kx, cs, :], wl[ky, kx, cs, :]
            return ah @ bh, al @ bh, ah @ bl

        acc = torch.zeros(n * hh * ww, cout, dtype=torch.float64)
        for t in range(0, (cin // 16) * ntap, 2):   # an even slice count (conv_stream.hip: divisible by 4)
            hh0, lh0, hl0 = prods(t)
            hh1, lh1, hl1 = prods(t + 1)
            if grouping == "pair":
                acc = f32(acc + (hh0 + lh0))
                acc = f32(acc + (hh1 + lh1))
            else:
                acc = f32(acc + (hh0 + hh1))
                acc = f32(acc + (lh0 + lh1))
            acc = f32(acc + (hl0 + hl1))
        y = f32(acc / wsc) + torch.as_tensor(bias, dtype=torch.float64)
        return f32(y.reshape(n, hh, ww, cout).permute(0, 3, 1, 2))
    return conv


def pairs16(x):
    """float64 holding float32 values -> the f16 pair (h, l) a split layer stores and the next one reads"""
    return split(f32(x), 2, torch.float16)


def emu_gemm(slabs, M, cout, form, lh_first=False, blocks_per_split=0):
    """slabs: list of callables -> (ah, al [M, 16], wh, wl [16, cout]) in the kernel's K order; returns the fp32
    accumulator [M, cout] under the MFMA model (each MFMA's products exact, one rounding into the accumulator)."""
    nslab = len(slabs)
    parts, acc = [], torch.zeros(M, cout, dtype=torch.float64)
    for b0 in range(0, nslab, 8):
        blk = torch.zeros(M, cout, dtype=torch.float64)
        if form == "four":
            for t in range(b0, min(b0 + 8, nslab)):
                ah, al, wh, wl = slabs[t]()
                blk = f32(blk + (ah @ wh + al @ wh))
                blk = f32(blk + (ah @ wl + al @ wl))
        else:
            for t in range(b0, min(b0 + 8, nslab), 2):
                ah0, al0, wh0, wl0 = slabs[t]()
                if t + 1 < nslab:
                    ah1, al1, wh1, wl1 = slabs[t + 1]()
                else:   # an odd tail pairs with a zero slab
                    ah1, al1, wh1, wl1 = (torch.zeros_like(v) for v in (ah0, al0, wh0, wl0))
                hh, lh, hl = ah0 @ wh0 + ah1 @ wh1, al0 @ wh0 + al1 @ wh1, ah0 @ wl0 + ah1 @ wl1
                for term in ((lh, hh, hl) if lh_first else (hh, lh, hl)):
                    blk = f32(blk + term)
        acc = f32(acc + blk)
        if blocks_per_split and (b0 // 8 + 1) % blocks_per_split == 0:
            parts.append(acc)
            acc = torch.zeros(M, cout, dtype=torch.float64)
    if not blocks_per_split:
        return acc
    if nslab and ((nslab + 7) // 8) % blocks_per_split:
        parts.append(acc)
    tot = torch.zeros(M, cout, dtype=torch.float64)
    for q in parts:   # the tile's last workgroup adds the splits' partials in split order
        tot = f32(tot + q)
    return tot


def wpairs(w):
    """[K, cout] weights -> (wh, wl, scale): x 2^e per output channel with max |w| 2^e in [2^14, 2^15) (weight_pack.cpp)"""
    wmax = w.abs().amax(dim=0).clamp_min(1e-30)
    wsc = torch.pow(2.0, 14 - torch.floor(torch.log2(wmax)))
    wh, wl = split(w * wsc, 2, torch.float16)
    return wh, wl, wsc


def emu_dense(x, kernel, bias, form):
    K_, cout = kernel.shape
    kp = (K_ + 15) // 16 * 16
    w = torch.zeros(kp, cout, dtype=torch.float64)
    w[:K_] = torch.as_tensor(np.asarray(kernel, np.float32), dtype=torch.float64)
    wh, wl, wsc = wpairs(w)
    xp = torch.zeros(x.shape[0], kp, dtype=torch.float64)
    xp[:, :K_] = x
    xh, xl = pairs16(xp)
    slabs = [lambda t=t: (xh[:, 16 * t:16 * t + 16], xl[:, 16 * t:16 * t + 16], wh[16 * t:16 * t + 16], wl[16 * t:16 * t + 16])
             for t in range(kp // 16)]
    nblocks, tiles_n = (kp // 16 + 7) // 8, (cout + 127) // 128   # forward_plan.h gemm_s16_ksplit
    ks = max(1, min(nblocks, 256 // (4 * tiles_n)))
    G = (nblocks + ks - 1) // ks
    acc = emu_gemm(slabs, x.shape[0], cout, form, blocks_per_split=G if (nblocks + G - 1) // G > 1 else 0)
    return f32(acc / wsc + torch.as_tensor(bias, dtype=torch.float64))


def emu_gather(x, taps, wk, order, form, lh_first=False):
    """One stride phase as a GEMM: x NHWC [n, H, W, cin] (float64 of float32), taps [(dy, dx)] with wk[i] the [cin, cout]
    weights of tap i, output pixel (y, x) reads input (y + dy, x + dx) (zero outside); order: list of (tap, chunk)."""
    n, H, W, cin = x.shape
    cout = wk[0].shape[1]
    wh, wl, wsc = wpairs(torch.cat(wk, 0))
    xh, xl = pairs16(x)
    pad = max(max(abs(dy), abs(dx)) for dy, dx in taps)
    xh, xl = (F.pad(v, (0, 0, pad, pad, pad, pad)) for v in (xh, xl))

    def slab(tap, c):
        dy, dx = taps[tap]
        cs = slice(16 * c, 16 * c + 16)
        a = [v[:, pad + dy:pad + dy + H, pad + dx:pad + dx + W, cs].reshape(-1, 16) for v in (xh, xl)]
        ws = slice(tap * cin + 16 * c, tap * cin + 16 * c + 16)
        return a[0], a[1], wh[ws], wl[ws]
    acc = emu_gemm([lambda t=t, c=c: slab(t, c) for t, c in order], n * H * W, cout, form, lh_first)
    return (acc / wsc).reshape(n, H, W, cout)


def main_generic(N, seed, wd, mel, video, ref, rms):
    inter = {}
    K.forward(wd, mel, video, intermediates=inter)
    T64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)

    def bn_act(y, name):   # y NHWC or [n, c]; BN + LeakyReLU in float64, stored as float32 (then as pairs by the reader)
        return f32(K.lrelu(K.bn(y, wd[name + "_bn"], torch.float64, channel_dim=y.dim() - 1)))

    out = {}
    for form in ("four", "three"):
        # v_conv6: 3x3 'same' on 4 x 4 x 512, k = tap * 512 + c (gemm.hip MODE 1), BN + LeakyReLU, 2x2 max pool
        v5 = f32(T64(inter["v_conv5"]))
        k6 = T64(np.asarray(wd["v_conv6"]["kernel"], np.float32))
        taps = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
        y = emu_gather(v5, taps, [k6[ky, kx] for ky in range(3) for kx in range(3)],
                       [(t, c) for t in range(9) for c in range(32)], form)
        y = bn_act(f32(y + T64(wd["v_conv6"]["bias"])), "v_conv6")
        y = F.max_pool2d(y.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).reshape(N, -1)
        aemb = inter["concat"].shape[1] - y.shape[1]
        x = torch.cat([f32(T64(inter["concat"][:, :aemb])), y], 1)
        x = bn_act(emu_dense(x, wd["enc_dense"]["kernel"], wd["enc_dense"]["bias"], form), "enc_dense")
        x = bn_act(emu_dense(x, wd["dec_dense1"]["kernel"], wd["dec_dense1"]["bias"], form), "dec_dense1")
        x = emu_dense(x, wd["dec_dense2"]["kernel"], wd["dec_dense2"]["bias"], form)
        x = bn_act(x.reshape(N, 5, -1, 128), "dec_dense2").permute(0, 3, 1, 2)
        for name, s_ in (("d_deconv1", (2, 1)), ("d_deconv2", (2, 1)), ("d_deconv3", (2, 2))):
            x = K.deconv_same(f32(x), wd[name]["kernel"], wd[name]["bias"], s_, torch.float64)
            x = f32(K.lrelu(K.bn(x, wd[name + "_bn"], torch.float64)))
        x = x.permute(0, 2, 3, 1)   # NHWC [N, 40, 10, 128]
        # d_deconv4: 4x4 stride 1, tap t = (ky, kx) reads (1 - ky, 1 - kx); K13 walks slab 16 c + t
        k4 = T64(np.asarray(wd["d_deconv4"]["kernel"], np.float32))   # (kh, kw, cout, cin)
        taps = [(1 - ky, 1 - kx) for ky in range(4) for kx in range(4)]
        y = emu_gather(x, taps, [k4[ky, kx].T for ky in range(4) for kx in range(4)],
                       [(t, c) for c in range(8) for t in range(16)], form, lh_first=True)
        x = bn_act(f32(y + T64(wd["d_deconv4"]["bias"])), "d_deconv4")
        # d_deconv5: 5x5 stride 2, phase (py, px): kernel rows ky with (py + 1 - ky) even read dy = (py + 1 - ky) / 2
        k5 = T64(np.asarray(wd["d_deconv5"]["kernel"], np.float32))
        n_, H, W, _ = x.shape
        y5 = torch.zeros(n_, 2 * H, 2 * W, k5.shape[2], dtype=torch.float64)
        for py in range(2):
            for px in range(2):
                kys = [ky for ky in range(5) if (py + 1 - ky) % 2 == 0]
                kxs = [kx for kx in range(5) if (px + 1 - kx) % 2 == 0]
                taps = [((py + 1 - ky) // 2, (px + 1 - kx) // 2) for ky in kys for kx in kxs]
                wk = [k5[ky, kx].T for ky in kys for kx in kxs]
                y5[:, py::2, px::2] = emu_gather(x, taps, wk, [(t, c) for t in range(len(taps)) for c in range(4)], form,
                                                 lh_first=True)
        x = bn_act(f32(y5 + T64(wd["d_deconv5"]["bias"])), "d_deconv5")
        got = (x @ T64(np.asarray(wd["d_deconv6"]["kernel"], np.float32))[0, 0].T + T64(wd["d_deconv6"]["bias"]))[..., 0].numpy()
        out[form] = float(np.sqrt(np.mean((got - ref) ** 2)))
        print(f"{form:6s} v_conv6 + dense + tail abs rms {out[form]:.3e}  rel {out[form] / rms:.2e}", flush=True)
    print(f"three - four {out['three'] - out['four']:+.3e}")


def main_groupings(N, seed, wd, mel, video, ref, rms):
    orig = K.conv_same
    v1 = make_conv("fp16x3", {"v_conv1"})
    out = {}
    for grouping in ("pair", "planar"):
        K.conv_same = make_grouped_conv(grouping, v1)
        try:
            got = K.forward(wd, mel, video)
        finally:
            K.conv_same = orig
        out[grouping] = float(np.sqrt(np.mean((got - ref) ** 2)))
        print(f"{grouping:8s} v2-v5 abs rms {out[grouping]:.3e}  rel {out[grouping] / rms:.2e}", flush=True)
    print(f"planar - pair {out['planar'] - out['pair']:+.3e}")


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 37
    torch.set_num_threads(8)
    model = KerasModel.init(seed=seed, randomize=True)
    k = model.tensors["d_deconv6/kernel"]
    model.tensors["d_deconv6/kernel"] = (k * 150.0).astype(np.float32)     # dB-scale output (test_gpu_forward.db_scale)
    model.tensors["d_deconv6/bias"] = np.full_like(model.tensors["d_deconv6/bias"], -40.0)
    rng = np.random.default_rng(seed + 100)
    x = synth_audio(rng, N, 3200)
    mel = np.stack([R.signal_to_spectrogram(x[i], 16000, 640, 160)[0][:, :20] for i in range(N)]).astype(np.float32)
    video = synth_video(rng, N)
    if len(sys.argv) > 3 and sys.argv[3] == "norm":
        m, s = R.video_normalizer_fit(video)
        video = R.video_normalize(video, m, s).astype(np.float32)
    wd = model.layer_dict()
    ref = K.forward(wd, mel, video)
    rms = float(np.sqrt(np.mean(ref ** 2)))
    layers_sets = {"v1-v5": {"v_conv1", "v_conv2", "v_conv3", "v_conv4", "v_conv5"},
                   "v1-v6": {"v_conv1", "v_conv2", "v_conv3", "v_conv4", "v_conv5", "v_conv6"}}
    orig = K.conv_same
    print(f"N={N} seed={seed} output rms {rms:.4g}")
    if len(sys.argv) > 3 and sys.argv[3] == "groupings":
        return main_groupings(N, seed, wd, mel, video, ref, rms)
    if len(sys.argv) > 3 and sys.argv[3] == "generic":
        return main_generic(N, seed, wd, mel, video, ref, rms)
    for sname in SCHEMES:
        for lname, ls in layers_sets.items():
            if sname == "fp32" and lname != "v1-v5":
                continue
            K.conv_same = make_conv(SCHEMES[sname] and sname, ls)
            try:
                got = K.forward(wd, mel, video)
            finally:
                K.conv_same = orig
            e = float(np.sqrt(np.mean((got - ref) ** 2)))
            print(f"{sname:12s} {lname:6s} abs rms {e:.3e}  rel {e / rms:.2e}", flush=True)


if __name__ == "__main__":
    main()
