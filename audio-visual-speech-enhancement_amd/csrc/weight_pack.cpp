// Host-only weight folding and packing (weight_pack.h).  Built by the same compiler as the kernels, so the host
// _Float16 conversions round as theirs.
#include "weight_pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace avse {

uint16_t f2h(float f) {   // the compiler's host _Float16 conversion
    const _Float16 h = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}
float h2f(uint16_t u) {
    _Float16 h;
    std::memcpy(&h, &u, 2);
    return (float)h;
}

uint16_t f2bf(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffff) ? 0x40 : 0));
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

SplitPair split_pair(float v) {
    const uint16_t h = f2h(v);
    return {h, f2h(v - h2f(h))};
}

std::vector<int> channel_exponents(const std::vector<float>& max_abs) {
    std::vector<int> ex(max_abs.size(), 0);
    for (size_t n = 0; n < max_abs.size(); ++n) {
        int e2 = 0;
        if (max_abs[n] > 0.f) (void)std::frexp(max_abs[n], &e2);   // max = f 2^e2, f in [0.5, 1)
        ex[n] = max_abs[n] > 0.f ? 15 - e2 : 0;
    }
    return ex;
}

void fold_bn(const LayerDef& L, const float* bias, const float* bn, std::vector<float>& scale, std::vector<float>& shift) {
    scale.assign(L.cout, 1.f);
    shift.assign(bias, bias + L.cout);
    if (!L.bn) return;
    const float* g = bn;
    const float* b = bn + L.bn_channels;
    const float* mu = bn + 2 * L.bn_channels;
    const float* var = bn + 3 * L.bn_channels;
    for (int n = 0; n < L.cout; ++n) {
        const int c = n % L.bn_channels;
        const double s = (double)g[c] / std::sqrt((double)var[c] + (double)kBnEps);
        scale[n] = (float)s;
        shift[n] = (float)(((double)bias[n] - (double)mu[c]) * s + (double)b[c]);
    }
}

// AVSE_F32_SPLIT activation exponents.  The split layers carry activations as f16 pairs, whose ~22 significant bits
// hold for |x| in [2^-3, 65504): below 2^-3 the lo piece is an f16 subnormal (absolute quantum 2^-24), from 65520 the
// hi piece overflows (the range guard then reports it).  A BatchNormalization layer's output per channel is
// gamma xhat + beta with xhat standardised by the moving statistics, so the layer's magnitude is ~ M = max_c (|beta_c| +
// |gamma_c|).  Layers with M in [2^-2, 2^8] keep exponent 0 (the common case: BN keeps activations O(1), and every
// stored value is then exactly the unscaled pair); any other layer stores the pairs of x 2^e with M 2^e in (4, 8], so a
// layer of tiny activations keeps its 22 bits and a layer of huge ones its headroom below 65504 (folded into the
// layer's own scale / shift and the next layer's scale, pack_layer).  The two concat halves (a_conv5, v_conv6) share
// one exponent, the smaller (enc_dense reads them as one K); d_deconv5 feeds the fp32 d_deconv6 dot (exponent 0).
void act_exponents(const NetPlan& P, const float* blob, int* e) {
    const float* p = blob;
    for (int i = 0; i < kNumLayers; ++i) {
        const LayerDef& L = P.L[i];
        p += (size_t)L.kh * L.kw * L.cin * L.cout + L.cout;
        e[i] = 0;
        if (!L.bn) continue;
        const float* g = p;
        const float* b = p + L.bn_channels;
        p += 4 * (size_t)L.bn_channels;
        double m = 0.0;
        for (int c = 0; c < L.bn_channels; ++c) m = std::max(m, std::fabs((double)b[c]) + std::fabs((double)g[c]));
        if (!(m > 0.0) || !std::isfinite(m) || (m >= 0.25 && m <= 256.0)) continue;
        int e2 = 0;
        (void)std::frexp(m, &e2);                      // m <= 2^e2
        e[i] = std::max(-24, std::min(24, 3 - e2));    // m 2^e in (4, 8]
    }
    e[4] = e[10] = std::min(e[4], e[10]);
    e[18] = e[19] = 0;
}

// the exponent of the activations layer i reads (act_exponents; the network inputs: 0)
int act_exp_in(const int* e, int i) {
    if (i == 0 || i == 5) return 0;
    if (i == 11) return e[4];
    return e[i - 1];
}

namespace {

// Element encoder of the tiled video convolutions' packings: one bf16 at o, or the split pair at o and o + lo_off.
struct HaloEnc {
    bool split;
    size_t lo_off;
    std::vector<uint16_t>& out;
    void operator()(size_t o, float v) const {
        if (!split) {
            out[o] = f2bf(v);
            return;
        }
        const SplitPair s = split_pair(v);
        out[o] = s.hi;
        out[o + lo_off] = s.lo;
    }
};

// The three layouts below take w(n, tap, c): output channel n's sign-folded (split: 2^e_n scaled) weight of Keras tap
// ky * kw + kx and input channel c.

// conv_stream.hip: [slice][Cout][32], slice = chunk * KS^2 + tap.  bf16: chunks of 32 channels (chunk = cg * 4 + cc of
// the kernel's 128-channel groups); split (S16): chunks of 16, row n = [Bh(16) | Bl(16)].
template <typename W>
std::vector<uint16_t> pack_stream(const LayerDef& L, bool split, W w) {
    const int ntap = L.kh * L.kw, cw = split ? 16 : 32, nsteps = (L.cin / cw) * ntap;
    std::vector<uint16_t> out((size_t)nsteps * L.cout * 32, 0);
    const HaloEnc enc{split, 16, out};
    for (int st = 0; st < nsteps; ++st)
        for (int n = 0; n < L.cout; ++n)
            for (int kk = 0; kk < cw; ++kk) enc(((size_t)st * L.cout + n) * 32 + kk, w(n, st % ntap, (st / ntap) * cw + kk));
    return out;
}

// conv_v1r.hip k_conv_v1r / k_conv_v1s: [kernel row ky][Cout][32], k = kx * 6 + frame (k = 30, 31 zero; frame 5 too
// with 5 frames); split: the image of the hi pieces, then the image of the lo pieces
template <typename W>
std::vector<uint16_t> pack_v1_rows(const LayerDef& L, bool split, W w) {
    const size_t img = (size_t)L.kh * L.cout * 32;
    std::vector<uint16_t> out(split ? 2 * img : img, 0);
    const HaloEnc enc{split, img, out};
    for (int ky = 0; ky < L.kh; ++ky)
        for (int n = 0; n < L.cout; ++n)
            for (int kx = 0; kx < L.kw; ++kx)
                for (int f = 0; f < L.cin; ++f) enc(((size_t)ky * L.cout + n) * 32 + kx * 6 + f, w(n, ky * L.kw + kx, f));
    return out;
}

// conv_v1r.hip k_conv_v1p (split, 5 x 5 taps x 5 frames): [piece h / l][K-slice s][Cout][32]; k-group g = 4 s + kg (8 k each):
//   s = 0..2, kg = ky (0..3), and s = 3, kg = s' (0..2) for ky = 4, of type s' / s:
//   0: kx 0, 1 x frames 0..3;  1: kx 2, 3 x frames 0..3;  2: kx 4 x frames 0..3, then kx 0..3 x frame 4;
//   s = 3, kg = 3: (ky 0..4, kx 4) x frame 4, three zeros
template <typename W>
std::vector<uint16_t> pack_v1p(const LayerDef& L, W w) {
    const size_t img = (size_t)4 * L.cout * 32;
    std::vector<uint16_t> out(2 * img, 0);
    const HaloEnc enc{true, img, out};
    auto wt = [&](int n, int ky, int kx, int f) { return w(n, ky * 5 + kx, f); };
    for (int g = 0; g < 16; ++g)
        for (int n = 0; n < L.cout; ++n)
            for (int j = 0; j < 8; ++j) {
                const int sl = g >> 2, kg = g & 3;
                const int t = sl < 3 ? sl : kg, ky = sl < 3 ? kg : 4;
                float v = 0.f;
                if (t == 0) v = wt(n, ky, j >> 2, j & 3);
                else if (t == 1) v = wt(n, ky, 2 + (j >> 2), j & 3);
                else if (t == 2) v = j < 4 ? wt(n, ky, 4, j) : wt(n, ky, j - 4, 4);
                else if (j < 5) v = wt(n, j, 4, 4);
                enc(((size_t)sl * L.cout + n) * 32 + kg * 8 + j, v);
            }
    return out;
}

// which tiled kernel a layer runs on (bf16 and split: the pooled video convs; Options::no_halo keeps the generic k_conv)
int halo_variant(const LayerDef& L, bool split, const Options& opt) {
    if (L.kind != CONV || !L.pool || L.hin < 8 || opt.no_halo) return HALO_NONE;
    if ((L.cin == 5 || L.cin == 6) && L.kh == 5)   // conv_v1r.hip: 5 (25 / 29.97 fps) or 6 frames (30)
        return split && L.cin == 5 && L.kw == 5 && L.cout == 128 && !opt.no_v1p ? HALO_V1P : HALO_V1;
    if (L.cin % 128) return HALO_NONE;
    if (L.kh == 5) return HALO_K5;
    return L.hin >= 16 ? HALO_K3_16 : HALO_K3_8;
}

}  // namespace

PackedLayer pack_layer(const LayerDef& L, const float* kernel, const float* bias, const float* bn, int dtype,
                       const Options& opt, int e_in, int e_out) {
    PackedLayer R;
    R.geom = layer_geom(L);
    const LayerGeom& G = R.geom;
    if (G.status != GEOM_OK) return R;
    const bool split = dtype == AVSE_F32_SPLIT;

    std::vector<float> scale;
    fold_bn(L, bias, bn, scale, R.shift);
    if (split && (e_in || e_out)) {
        // activation exponents (act_exponents): this layer reads pairs of x 2^e_in and stores pairs of y 2^e_out, so
        // y 2^e_out = LReLU(acc 2^-e_in scale 2^e_out + shift 2^e_out) — powers of two: exact, and they commute with
        // LeakyReLU and max pooling
        for (int n = 0; n < L.cout; ++n) {
            scale[n] = std::ldexp(scale[n], e_out - e_in);
            R.shift[n] = std::ldexp(R.shift[n], e_out);
        }
    }
    // split: output channel n's weights scaled by 2^ex[n] in every packing, the epilogue scale by 2^-ex[n] (exact)
    std::vector<int> ex(L.cout, 0);
    if (split) {
        std::vector<float> mx(L.cout, 0.f);
        for (int ky = 0; ky < L.kh; ++ky)
            for (int kx = 0; kx < L.kw; ++kx)
                for (int c = 0; c < L.cin; ++c)
                    for (int n = 0; n < L.cout; ++n) mx[n] = std::max(mx[n], std::fabs(kernel[kidx(L, ky, kx, c, n)]));
        ex = channel_exponents(mx);
    }
    R.scale = scale;
    for (int n = 0; n < L.cout; ++n) R.scale[n] = std::ldexp(scale[n], -ex[n]);

    // generic packing [phase][Cout][kpad]: the kernel read through the gather map (the dense layers, one tap and 2/3 of
    // all weights, directly: building their map costs as much as packing them)
    std::vector<float> packed((size_t)G.w_elems, 0.f);
    if (L.kind == DENSE) {
        for (int n = 0; n < L.cout; ++n)
            for (int c = 0; c < L.cin; ++c) packed[(size_t)n * G.ph[0].kpad + c] = kernel[kidx(L, 0, 0, c, n)];
    } else {
        const std::vector<int> map = gather_map(L, G);
        for (size_t i = 0; i < map.size(); ++i)
            if (map[i] >= 0) packed[i] = kernel[map[i]];
    }
    if (dtype == AVSE_BF16) {
        R.w16.resize(packed.size());
        for (size_t i = 0; i < packed.size(); ++i) R.w16[i] = f2bf(packed[i]);
    } else if (split) {
        // conv.hip k_conv<float, .., S16>: each 16-k slab row of [Cout][kpad] becomes [Bh(16) | Bl(16)] f16
        R.w16.resize(2 * packed.size());
        for (int p = 0; p < G.nphase; ++p)
            for (int n = 0; n < L.cout; ++n) {
                const size_t row = (size_t)G.ph[p].w_off + (size_t)n * G.ph[p].kpad;
                for (int k = 0; k < G.ph[p].kpad; ++k) {
                    const SplitPair s = split_pair(std::ldexp(packed[row + k], ex[n]));
                    const size_t dst = 2 * row + (size_t)(k / 16) * 32 + k % 16;
                    R.w16[dst] = s.hi;
                    R.w16[dst + 16] = s.lo;
                }
            }
    } else {
        R.w32 = std::move(packed);
    }
    if (L.kind == CONV && L.cin == 1) {   // a_conv1's own kernels read the single input channel's taps directly
        const int ntap = L.kh * L.kw;
        if (split) {   // f32 taps with the same per-channel power of two
            R.w_f32.resize((size_t)ntap * L.cout);
            for (int t = 0; t < ntap; ++t)
                for (int n = 0; n < L.cout; ++n) R.w_f32[(size_t)t * L.cout + n] = std::ldexp(kernel[(size_t)t * L.cout + n], ex[n]);
        } else if (dtype == AVSE_BF16 && ntap <= 32) {   // conv_aud.hip: a dense 32-deep K (25 real)
            R.w_dense.assign((size_t)L.cout * 32, 0);
            for (int n = 0; n < L.cout; ++n)
                for (int t = 0; t < ntap; ++t) R.w_dense[(size_t)n * 32 + t] = f2bf(kernel[(size_t)t * L.cout + n]);
        }
    }

    if (dtype == AVSE_F32) return R;
    R.halo = halo_variant(L, split, opt);
    if (R.halo == HALO_NONE) return R;
    // Sign fold: a channel whose folded BN scale is negative gets negated weights and |scale|, so every epilogue scale
    // is >= 0 and 2x2 max pooling commutes exactly with scale/shift (the kernels pool the raw accumulators, then apply
    // one FMA).  Negation and the power of two are exact.
    R.scale_h.resize(L.cout);
    for (int n = 0; n < L.cout; ++n) R.scale_h[n] = std::ldexp(std::fabs(scale[n]), -ex[n]);
    auto w = [&](int n, int tap, int c) {
        const float v = (scale[n] < 0.f ? -1.f : 1.f) * kernel[((size_t)tap * L.cin + c) * L.cout + n];
        return split ? std::ldexp(v, ex[n]) : v;
    };
    if (R.halo == HALO_V1P) R.w_halo = pack_v1p(L, w);
    else if (R.halo == HALO_V1) R.w_halo = pack_v1_rows(L, split, w);
    else R.w_halo = pack_stream(L, split, w);
    return R;
}

}  // namespace avse
