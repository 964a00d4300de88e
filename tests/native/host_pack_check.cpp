// Host-only check of the layer geometry, the weight packer and the spectrogram / ISTFT tables (csrc/layer_geom.h,
// weight_pack.cpp, spec_tables.cpp): no GPU, no file input.  Prints one 64-bit FNV-1a hash per produced buffer as a
// JSON object (tests/test_pack_host.py compares it with tests/golden/pack_hashes.json) and checks two properties
// itself: the geometry against a brute-force scatter definition of the (transposed) convolution, and every split
// pair against the weight it encodes.  Exit status 0: all checks passed.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../audio-visual-speech-enhancement_amd/csrc/spec_tables.h"
#include "../../audio-visual-speech-enhancement_amd/csrc/weight_pack.h"

using namespace avse;

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_failures <= 20) {                     \
                std::fprintf(stderr, "CHECK failed: ");   \
                std::fprintf(stderr, __VA_ARGS__);        \
                std::fprintf(stderr, "\n");               \
            }                                             \
        }                                                 \
    } while (0)

bool g_first = true;
template <typename T>
void emit(const std::string& name, const T* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n * sizeof(T); ++i) h = (h ^ b[i]) * 1099511628211ull;
    std::printf("%s\n  \"%s\": \"%016llx\"", g_first ? "{" : ",", name.c_str(), (unsigned long long)h);
    g_first = false;
}
template <typename T>
void emit(const std::string& name, const std::vector<T>& v) { emit(name, v.data(), v.size()); }

// fixed integer LCG (Numerical Recipes' constants): uniform in [-1, 1) from the top 24 bits
struct Lcg {
    uint32_t s;
    float next() {
        s = s * 1664525u + 1013904223u;
        return (float)((int32_t)(s >> 8) - (1 << 23)) / (float)(1 << 23);
    }
};

// A canonical blob (include/avse.h) with the cases the folding has to handle: negative BN gammas (every third
// channel), |gamma| + |beta| ~ 2^-6 in a_conv3 and ~ 2^12 in v_conv3 (activation exponents of either sign), and
// all-zero output channels (a_conv2 channel 5 on the generic kernel, v_conv2 channel 3 on a tiled one).
std::vector<float> make_blob(const NetPlan& P) {
    std::vector<float> blob;
    blob.reserve((size_t)blob_floats(P));
    Lcg r{12345u + (uint32_t)P.T * 97u + (uint32_t)P.F};
    for (int i = 0; i < kNumLayers; ++i) {
        const LayerDef& L = P.L[i];
        const float amp = 1.f / std::sqrt((float)(L.kh * L.kw * L.cin));
        const size_t k0 = blob.size();
        for (long long j = 0; j < (long long)L.kh * L.kw * L.cin * L.cout; ++j) blob.push_back(amp * r.next());
        const int zero_ch = i == 1 ? 5 : i == 6 ? 3 : -1;
        if (zero_ch >= 0)
            for (int ky = 0; ky < L.kh; ++ky)
                for (int kx = 0; kx < L.kw; ++kx)
                    for (int c = 0; c < L.cin; ++c) blob[k0 + (size_t)kidx(L, ky, kx, c, zero_ch)] = 0.f;
        for (int n = 0; n < L.cout; ++n) blob.push_back(0.1f * r.next());
        if (!L.bn) continue;
        const float mag = i == 2 ? std::ldexp(1.f, -7) : i == 7 ? std::ldexp(1.f, 11) : 1.f;
        for (int c = 0; c < L.bn_channels; ++c) blob.push_back(mag * (c % 3 == 1 ? -1.f : 1.f) * (1.f + 0.5f * r.next()));   // gamma
        for (int c = 0; c < L.bn_channels; ++c) blob.push_back(mag * 0.5f * r.next());                                   // beta
        for (int c = 0; c < L.bn_channels; ++c) blob.push_back(0.5f * r.next());                                         // mean
        for (int c = 0; c < L.bn_channels; ++c) blob.push_back(1.f + 0.5f * r.next());                                   // variance
    }
    return blob;
}

// ---- property 1: geometry against the scatter definition --------------------------------------------------------
// One (output pixel, input pixel, kernel tap) term of the layer as a key.  The plan's grids stay below 2^9 per axis.
uint64_t term(int oy, int ox, int iy, int ix, int ky, int kx) {
    return ((uint64_t)oy << 46) | ((uint64_t)ox << 37) | ((uint64_t)iy << 28) | ((uint64_t)ix << 19) | ((uint64_t)ky << 8) | (uint64_t)kx;
}

// TF semantics, written as loops over the definition.  CONV 'SAME' (DENSE: 1 x 1): out[o] += in[o s + k - pad_before]
// w[k]; conv2d_transpose 'SAME': every input pixel scatters in[i] w[k] to the full output at i s + k, of which the
// window [pad_before, pad_before + in s) is kept.
std::vector<uint64_t> brute_terms(const LayerDef& L, int* ho, int* wo) {
    std::vector<uint64_t> t;
    if (L.kind == DECONV) {
        *ho = L.hin * L.sh;
        *wo = L.win * L.sw;
        const int pt = std::max(L.kh - L.sh, 0) / 2, pl = std::max(L.kw - L.sw, 0) / 2;
        for (int iy = 0; iy < L.hin; ++iy)
            for (int ix = 0; ix < L.win; ++ix)
                for (int ky = 0; ky < L.kh; ++ky)
                    for (int kx = 0; kx < L.kw; ++kx) {
                        const int oy = iy * L.sh + ky - pt, ox = ix * L.sw + kx - pl;
                        if (oy >= 0 && oy < *ho && ox >= 0 && ox < *wo) t.push_back(term(oy, ox, iy, ix, ky, kx));
                    }
    } else {
        *ho = (L.hin + L.sh - 1) / L.sh;
        *wo = (L.win + L.sw - 1) / L.sw;
        const int pt = std::max((*ho - 1) * L.sh + L.kh - L.hin, 0) / 2, pl = std::max((*wo - 1) * L.sw + L.kw - L.win, 0) / 2;
        for (int oy = 0; oy < *ho; ++oy)
            for (int ox = 0; ox < *wo; ++ox)
                for (int ky = 0; ky < L.kh; ++ky)
                    for (int kx = 0; kx < L.kw; ++kx) {
                        const int iy = oy * L.sh + ky - pt, ix = ox * L.sw + kx - pl;
                        if (iy >= 0 && iy < L.hin && ix >= 0 && ix < L.win) t.push_back(term(oy, ox, iy, ix, ky, kx));
                    }
    }
    std::sort(t.begin(), t.end());
    return t;
}

// the terms k_conv computes from a phase set: grid point q of phase p writes pixel q os + (py, px) from the pixels
// q is + tap offset inside the [sh][sw] source; `dgrad`: written pixels are the layer's input
std::vector<uint64_t> geom_terms(const PhaseSet& g, int hq, int wq, int isy, int isx, int osy, int osx, int src_h, int src_w,
                                 int dst_h, int dst_w) {
    std::vector<uint64_t> t;
    for (int p = 0; p < g.nphase; ++p)
        for (int qy = 0; qy < hq; ++qy)
            for (int qx = 0; qx < wq; ++qx) {
                const int wy = qy * osy + g.ph[p].py, wx = qx * osx + g.ph[p].px;
                if (wy >= dst_h || wx >= dst_w) continue;
                for (int j = 0; j < g.ph[p].ntaps; ++j) {
                    const Tap d = g.taps[g.ph[p].tap_off + j];
                    const int ry = qy * isy + d.dy, rx = qx * isx + d.dx;
                    if (ry < 0 || ry >= src_h || rx < 0 || rx >= src_w) continue;
                    const int ky = g.kyx[p][j].first, kx = g.kyx[p][j].second;
                    t.push_back(g.dgrad ? term(ry, rx, wy, wx, ky, kx) : term(wy, wx, ry, rx, ky, kx));
                }
            }
    std::sort(t.begin(), t.end());
    return t;
}

void check_geometry(const NetPlan& P) {
    for (int i = 0; i < kNumLayers; ++i) {
        const LayerDef& L = P.L[i];
        int ho = 0, wo = 0;
        const std::vector<uint64_t> want = brute_terms(L, &ho, &wo);
        const LayerGeom f = layer_geom(L);
        CHECK(f.status == GEOM_OK, "%s: layer_geom status %d", L.name, (int)f.status);
        CHECK(f.hz == ho && f.wz == wo, "%s: output grid %d x %d, expected %d x %d", L.name, f.hz, f.wz, ho, wo);
        CHECK(f.ho == (L.pool ? ho / 2 : ho) && f.wo == (L.pool ? wo / 2 : wo), "%s: pooled grid", L.name);
        const bool dc = L.kind == DECONV;
        CHECK(geom_terms(f, f.hq, f.wq, dc ? 1 : L.sh, dc ? 1 : L.sw, dc ? L.sh : 1, dc ? L.sw : 1, L.hin, L.win, ho, wo) == want,
              "%s (T %d): layer_geom disagrees with the scatter definition", L.name, P.T);
        const DgradGeom d = dgrad_geom(L);
        CHECK(d.status == GEOM_OK, "%s: dgrad_geom status %d", L.name, (int)d.status);
        CHECK(geom_terms(d, d.hq, d.wq, d.sy, d.sx, d.oys, d.oxs, ho, wo, L.hin, L.win) == want,
              "%s (T %d): dgrad_geom disagrees with the transposed scatter definition", L.name, P.T);
        for (const PhaseSet* g : {(const PhaseSet*)&f, (const PhaseSet*)&d})
            for (int p = 0; p < g->nphase; ++p)
                CHECK(g->ph[p].kpad % 32 == 0 && g->ph[p].kpad >= g->ph[p].ntaps * g->cp && g->cp % 8 == 0 && g->cp >= g->red,
                      "%s: phase %d padding", L.name, p);
    }
}

// ---- property 2: hi + lo reproduces w 2^e to within one f16 ulp of lo --------------------------------------------
void check_pair(const char* what, const LayerDef& L, uint16_t hi, uint16_t lo, float w, int e) {
    static const std::vector<double> pow2 = [] {   // 2^(i - 64)
        std::vector<double> t(128);
        for (int i = 0; i < 128; ++i) t[i] = std::ldexp(1.0, i - 64);
        return t;
    }();
    const double want = (double)w * pow2[e + 64];                                 // exact: a power of two
    const double ulp = pow2[std::max((int)(lo >> 10 & 31), 1) - 25 + 64];         // f16: 2^(exponent field - 25), subnormals 2^-24
    CHECK(std::fabs((double)h2f(hi) + (double)h2f(lo) - want) <= ulp, "%s %s: pair (%04x, %04x) for %.9g x 2^%d", L.name, what, hi, lo, w, e);
}

void check_pairs(const LayerDef& L, const float* kernel, const float* bias, const float* bn, const PackedLayer& P) {
    std::vector<float> mx(L.cout, 0.f), scale, shift;
    for (int ky = 0; ky < L.kh; ++ky)
        for (int kx = 0; kx < L.kw; ++kx)
            for (int c = 0; c < L.cin; ++c)
                for (int n = 0; n < L.cout; ++n) mx[n] = std::max(mx[n], std::fabs(kernel[kidx(L, ky, kx, c, n)]));
    const std::vector<int> ex = channel_exponents(mx);
    for (int n = 0; n < L.cout; ++n) CHECK(mx[n] == 0.f ? ex[n] == 0 : (std::ldexp(mx[n], ex[n]) >= 16384.f && std::ldexp(mx[n], ex[n]) < 32768.f),
                                           "%s: channel %d exponent %d for max %g", L.name, n, ex[n], mx[n]);
    const std::vector<int> map = gather_map(L, P.geom);
    CHECK(P.w16.size() == 2 * map.size(), "%s: split packing size", L.name);
    for (int p = 0; p < P.geom.nphase; ++p)
        for (int n = 0; n < L.cout; ++n)
            for (int k = 0; k < P.geom.ph[p].kpad; ++k) {
                const size_t row = (size_t)P.geom.ph[p].w_off + (size_t)n * P.geom.ph[p].kpad;
                const size_t o = 2 * row + (size_t)(k / 16) * 32 + k % 16;
                check_pair("generic", L, P.w16[o], P.w16[o + 16], map[row + k] < 0 ? 0.f : kernel[map[row + k]], ex[n]);
            }
    if (P.halo == HALO_NONE) return;
    fold_bn(L, bias, bn, scale, shift);
    auto w = [&](int n, int tap, int c) { return (scale[n] < 0.f ? -1.f : 1.f) * kernel[((size_t)tap * L.cin + c) * L.cout + n]; };
    const int ntap = L.kh * L.kw;
    if (P.halo == HALO_V1 || P.halo == HALO_V1P) {
        // [piece][slice][Cout][32]: per output channel the pairs are those of its taps x frames, in the kernel's k order
        // (V1: k = kx * 6 + frame per kernel row; V1P: conv_v1r.hip's groups), and zeros
        const size_t img = P.w_halo.size() / 2;
        const int slices = (int)(img / ((size_t)L.cout * 32));
        for (int n = 0; n < L.cout; ++n) {
            std::vector<uint32_t> got, want;
            for (int s = 0; s < slices; ++s)
                for (int k = 0; k < 32; ++k) {
                    const size_t o = ((size_t)s * L.cout + n) * 32 + k;
                    got.push_back((uint32_t)P.w_halo[o] << 16 | P.w_halo[img + o]);
                    if (P.halo == HALO_V1 && k < L.kw * 6 && k % 6 < L.cin) check_pair("v1 rows", L, P.w_halo[o], P.w_halo[img + o], w(n, s * L.kw + k / 6, k % 6), ex[n]);
                }
            for (int t = 0; t < ntap; ++t)
                for (int c = 0; c < L.cin; ++c) {
                    const SplitPair sp = split_pair(std::ldexp(w(n, t, c), ex[n]));
                    check_pair("v1", L, sp.hi, sp.lo, w(n, t, c), ex[n]);
                    want.push_back((uint32_t)sp.hi << 16 | sp.lo);
                }
            want.resize(got.size(), 0u);
            std::sort(got.begin(), got.end());
            std::sort(want.begin(), want.end());
            CHECK(got == want, "%s: channel %d's packed pairs are not those of its weights", L.name, n);
        }
    } else {
        for (int st = 0; st < (L.cin / 16) * ntap; ++st)
            for (int n = 0; n < L.cout; ++n)
                for (int kk = 0; kk < 16; ++kk) {
                    const size_t o = ((size_t)st * L.cout + n) * 32 + kk;
                    check_pair("stream", L, P.w_halo[o], P.w_halo[o + 16], w(n, st % ntap, (st / ntap) * 16 + kk), ex[n]);
                }
    }
}

void pack_plan(int T, int F) {
    const NetPlan P = make_plan(T, F);
    const std::vector<float> blob = make_blob(P);
    CHECK((int64_t)blob.size() == blob_floats(P), "blob size");
    check_geometry(P);
    const char* dtn[3] = {"float32", "bfloat16", "float32_split"};
    for (int dtype : {AVSE_F32, AVSE_BF16, AVSE_F32_SPLIT}) {
        const std::string pre = "pack/T" + std::to_string(T) + "F" + std::to_string(F) + "/" + dtn[dtype] + "/";
        int e[kNumLayers] = {};
        if (dtype == AVSE_F32_SPLIT) {
            act_exponents(P, blob.data(), e);
            emit(pre + "act_exp", e, kNumLayers);
            CHECK(e[2] > 0 && e[7] < 0, "activation exponents: a_conv3 %d (expected > 0), v_conv3 %d (expected < 0)", e[2], e[7]);
        }
        const float* p = blob.data();
        for (int i = 0; i < kNumLayers - 1; ++i) {   // d_deconv6 is not packed
            const LayerDef& L = P.L[i];
            const float* kernel = p;
            p += (size_t)L.kh * L.kw * L.cin * L.cout;
            const float* bias = p;
            p += L.cout;
            const float* bn = L.bn ? p : nullptr;
            if (L.bn) p += 4 * (size_t)L.bn_channels;
            const PackedLayer R = pack_layer(L, kernel, bias, bn, dtype, Options(), act_exp_in(e, i), e[i]);
            CHECK(R.geom.status == GEOM_OK, "%s: pack_layer status", L.name);
            const std::string nm = pre + L.name + "/";
            const int g[7] = {R.geom.cin_pad, R.geom.hq, R.geom.wq, R.geom.ho, R.geom.wo, R.geom.nphase, R.halo};
            emit(nm + "geom", g, 7);
            for (int ph = 0; ph < R.geom.nphase; ++ph) {
                const long long v[6] = {R.geom.ph[ph].py, R.geom.ph[ph].px, R.geom.ph[ph].ntaps, R.geom.ph[ph].kpad,
                                        R.geom.ph[ph].w_off, R.geom.ph[ph].tap_off};
                emit(nm + "phase" + std::to_string(ph), v, 6);
            }
            emit(nm + "taps", R.geom.taps);
            if (dtype == AVSE_F32) emit(nm + "w", R.w32);
            else emit(nm + "w", R.w16);
            emit(nm + "scale", R.scale);
            emit(nm + "shift", R.shift);
            if (!R.scale_h.empty()) emit(nm + "scale_h", R.scale_h);
            if (!R.w_halo.empty()) emit(nm + "w_halo", R.w_halo);
            if (!R.w_dense.empty()) emit(nm + "w_dense", R.w_dense);
            if (!R.w_f32.empty()) emit(nm + "w_f32", R.w_f32);
            if (dtype == AVSE_F32_SPLIT) check_pairs(L, kernel, bias, bn, R);
        }
    }
}

void tables(int sr, int n_fft, int n_mels) {
    const std::string pre = "tables/" + std::to_string(sr) + "_" + std::to_string(n_fft) + "_" + std::to_string(n_mels) + "/";
    const double fmin = 0.0, fmax = 8000.0;
    const MelBands mb = mel_bands(sr, n_fft, n_mels, fmin, fmax);
    const int hdr[2] = {mb.n_bins, mb.max_width};
    emit(pre + "mel_dims", hdr, 2);
    emit(pre + "mel_start", mb.start);
    emit(pre + "mel_width", mb.width);
    emit(pre + "mel_weight", mb.weight);
    emit(pre + "mel_seg_nq", mb.seg_nq, 4);
    emit(pre + "mel_seg_nq4", mb.seg_nq4, 4);
    const DftTables fw = dft_tables(n_fft), inv = dft_tables(2 * (n_fft / 2));
    emit(pre + "stft_twiddle", fw.twiddle);
    emit(pre + "stft_window", fw.window);
    emit(pre + "istft_twiddle", inv.twiddle);
    emit(pre + "istft_window", inv.window);
    const IstftHostTables it = istft_tables(sr, n_fft, n_mels, fmin, fmax);
    emit(pre + "pinvT", it.pinvT);
    emit(pre + "bins", it.bins);
    emit(pre + "gram_inv", it.gram_inv);
    CHECK(it.pinvT.size() == (size_t)n_mels * mb.n_bins, "pinv size");
    // n_fft 640: the reference's bank (tridiagonal Gram matrix: the fused kernel's tables exist); 401: rank deficient
    CHECK(it.bins.empty() == (n_fft == 401) && it.gram_inv.empty() == it.bins.empty(), "n_fft %d: fused-path tables %zu / %zu",
          n_fft, it.bins.size(), it.gram_inv.size());
}

}  // namespace

int main() {
    pack_plan(4, 3);
    pack_plan(20, 5);
    pack_plan(24, 6);
    tables(16000, 640, 80);
    tables(16000, 401, 80);
    std::printf("\n}\n");
    if (g_failures) std::fprintf(stderr, "%d checks failed\n", g_failures);
    return g_failures ? 1 : 0;
}
