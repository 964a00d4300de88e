// avse_weights (include/avse.h): the folded / packed layers of weight_pack.cpp uploaded to the device, and the
// weights-only decisions of the forward (which fused kernels the layers' shapes allow).
#include <algorithm>
#include <cstring>

#include "ctx.h"
#include "weight_pack.h"

using namespace avse;

// the host-only tables' element types are uploaded as the HIP vector types the kernels read
static_assert(sizeof(Tap) == sizeof(int2) && offsetof(Tap, dy) == offsetof(int2, x) && offsetof(Tap, dx) == offsetof(int2, y),
              "Tap must be layout-compatible with int2");

avse_weights::~avse_weights() {
    delete f32_twin;
    (void)hipFree(vzero_emb.load());
}

namespace {

template <typename T, typename P>
int upload(avse_weights* W, const std::vector<T>& h, P** out) {
    Owned<char> b;
    if (b.alloc(sizeof(T) * (h.empty() ? 1 : h.size())) != hipSuccess) return fail(AVSE_ERR_OOM, "hipMalloc failed (weights)");
    if (!h.empty() && hipMemcpy(b, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail(AVSE_ERR_HIP, "hipMemcpy failed (weights)");
    *out = reinterpret_cast<P*>(b.p.get());
    W->allocs.push_back(std::move(b));
    return 0;
}

// Pack one layer on the host (weight_pack.cpp: geometry, folded scale / shift, every weight layout) and upload it.
int build_layer(avse_weights* W, int li, const float* kernel, const float* bias, const float* bn,
                const Options& opt, int e_in = 0, int e_out = 0) {
    const LayerDef& L = W->shape.plan.L[li];
    const PackedLayer P = pack_layer(L, kernel, bias, bn, W->dtype, opt, e_in, e_out);
    if (P.geom.status != GEOM_OK) return fail(AVSE_ERR_UNSUPPORTED, geom_message(P.geom.status));
    GpuLayer& G = W->layers[li];
    G.def = L;
    G.cin_pad = P.geom.cin_pad;
    G.hq = P.geom.hq; G.wq = P.geom.wq; G.ho = P.geom.ho; G.wo = P.geom.wo;
    G.nphase = P.geom.nphase;
    std::copy(P.geom.ph, P.geom.ph + MAX_PHASES, G.ph);
    G.halo = P.halo;
    const std::vector<Tap>& taps = P.geom.taps;
    std::memcpy(G.htaps, taps.data(), sizeof(Tap) * std::min(taps.size(), (size_t)(MAX_TAPS * MAX_PHASES)));
    // each non-empty buffer becomes one device allocation owned by W
    auto up = [&](const auto& h, auto** out) { return h.empty() ? 0 : upload(W, h, out); };
    int rc = 0;   // the generic weights are w32 or w16, never both
    (void)((rc = up(P.w32, &G.w)) || (rc = up(P.w16, &G.w)) || (rc = up(P.w_halo, &G.w_halo)) || (rc = up(P.w_dense, &G.w_dense)) ||
           (rc = up(P.w_f32, &G.w_f32)) || (rc = up(P.scale, &G.scale)) || (rc = up(P.shift, &G.shift)) ||
           (rc = up(P.scale_h, &G.scale_h)) || (rc = up(taps, &G.taps)));
    return rc;
}

// ---- the shapes the fused kernels are written for (network.py at the 200-ms segment); L: the plan's layers ----
// conv_aud.hip: a_conv1 .. a_conv5
bool aud_enc_shapes(const GpuLayer* L) {
    return L[0].def.cin == 1 && L[0].hq == 40 && L[0].wq == 10 && L[1].def.cin == 64 && L[1].def.cout == 64 &&
           L[1].def.kh == 4 && L[2].def.cout == 128 && L[2].hq == 20 && L[2].wq == 5 && L[3].hq == 10 && L[3].wq == 5 &&
           L[4].hq == 5 && L[4].wq == 5 && L[3].ph[0].kpad == 512 && L[4].ph[0].kpad == 512 && L[1].ph[0].kpad == 1024 &&
           L[2].ph[0].kpad == 1024;
}

// conv_dech.hip: d_deconv1 .. d_deconv3 with the network's shapes and sub-pixel tap grids
bool dec_head_shapes(const GpuLayer* L) {
    auto taps_ok = [](const GpuLayer& D, int np, int nt, bool wide) {
        if (D.nphase != np || D.def.cin != 128 || D.def.cout != 128) return false;
        for (int p = 0; p < np; ++p) {
            if (D.ph[p].ntaps != nt || D.ph[p].kpad != nt * 128 || D.ph[p].w_off != (long long)p * 128 * nt * 128) return false;
            for (int t = 0; t < nt; ++t) {
                const int2 d = D.htaps[D.ph[p].tap_off + t];
                const int dy = wide ? (p >> 1) - (t >> 1) : 0, dx = wide ? (p & 1) - (t & 1) : -t;
                if (d.x != dy || d.y != dx) return false;
            }
        }
        return true;
    };
    return L[14].hq == 5 && L[14].wq == 5 && L[15].hq == 10 && L[15].wq == 5 && L[16].hq == 20 && L[16].wq == 5 &&
           taps_ok(L[14], 2, 2, false) && taps_ok(L[15], 2, 2, false) && taps_ok(L[16], 4, 4, true);
}

// gemm.hip mode 1: v_conv6 as 3 x 3 'same' on 4 x 4 x 512 + 2 x 2 pool
bool v6_gemm_shape(const GpuLayer& G) {
    return G.def.hin == 4 && G.def.win == 4 && G.def.cin == 512 && G.def.kh == 3 && G.def.pool && G.ph[0].kpad == 9 * 512;
}

// conv.hip k_aconv1_split: a_conv1 on the vector ALUs from the audio input itself (split dtype: w_f32 is packed)
bool a1_valu_shape(const GpuLayer& G) {
    return G.w_f32 && G.def.cin == 1 && G.def.kind == CONV && G.def.cout == 64 && G.def.kh == 5 && G.def.kw == 5 &&
           G.def.sh == G.def.sw;
}

}  // namespace

extern "C" {

int64_t avse_weights_blob_floats(void) { return blob_floats(kPlan25); }

int64_t avse_weights_blob_floats_shape(int spec_frames, int video_frames) {
    if (!plan_valid(spec_frames, video_frames)) return -1;
    return blob_floats(make_plan(spec_frames, video_frames));
}

int avse_weights_load(avse_ctx* c, const float* blob, int64_t n_floats, int dtype, avse_weights** out) {
    return avse_weights_load_shape(c, blob, n_floats, dtype, kPlan25.T, kPlan25.F, out);
}

int avse_weights_shape(const avse_weights* w, int* spec_frames, int* video_frames) {
    if (!w || !spec_frames || !video_frames) return fail(AVSE_ERR_INVALID, "NULL argument");
    *spec_frames = w->shape.plan.T;
    *video_frames = w->shape.plan.F;
    return 0;
}

int avse_weights_load_shape(avse_ctx* c, const float* blob, int64_t n_floats, int dtype, int spec_frames,
                            int video_frames, avse_weights** out) {
    if (!c || !blob || !out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (!valid_dtype(dtype)) return fail(AVSE_ERR_INVALID, "bad compute dtype");
    if (!plan_valid(spec_frames, video_frames))
        return fail(AVSE_ERR_UNSUPPORTED, "network shape [80, " + std::to_string(spec_frames) + "] x [128, 128, " +
                                              std::to_string(video_frames) + "]: the decoder reproduces 80 x T only for "
                                              "T a multiple of 4; video frames must be 1..8");
    const NetPlan plan = make_plan(spec_frames, video_frames);
    if (n_floats != blob_floats(plan))
        return fail(AVSE_ERR_INVALID, "weight blob has " + std::to_string(n_floats) + " floats, expected " +
                                          std::to_string(blob_floats(plan)));
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    avse_weights* W = new avse_weights();
    static std::atomic<uint64_t> next_serial{1};
    W->serial = next_serial++;
    W->dtype = dtype;
    W->device = c->device;
    W->shape = arena_shape(plan);
    if (dtype == AVSE_F32_SPLIT) {
        if (!c->opt.no_act_scale) act_exponents(plan, blob, W->act_exp);
        W->blob.assign(blob, blob + n_floats);   // avse_forward_checked's exact-fp32 twin is built from it on demand
    }
    const float* p = blob;
    for (int i = 0; i < kNumLayers; ++i) {
        const LayerDef& L = plan.L[i];
        const float* kernel = p;
        p += (size_t)L.kh * L.kw * L.cin * L.cout;
        const float* bias = p;
        p += L.cout;
        const float* bn = nullptr;
        if (L.bn) {
            bn = p;
            p += 4 * (size_t)L.bn_channels;
        }
        if (i == kNumLayers - 1) {  // d_deconv6: 1x1, 64 -> 1
            std::vector<float> w64(kernel, kernel + 64);
            int rc = upload(W, w64, &W->d6_w);
            if (rc) { delete W; return rc; }
            W->d6_bias = bias[0];
            continue;
        }
        int rc = build_layer(W, i, kernel, bias, bn, c->opt, act_exp_in(W->act_exp, i), W->act_exp[i]);
        if (rc) { delete W; return rc; }
    }
    if (dtype == AVSE_F32_SPLIT) {
        // the split layers pass split-pair activations to each other: they must be a prefix v_conv1 .. of the video
        // encoder (a v_conv1 on the generic kernel makes every video layer generic; no_halo: all of them)
        bool prefix = true;
        for (int i = 5; i < 11; ++i) {
            if (W->layers[i].halo == HALO_NONE) prefix = false;
            if (!prefix) W->layers[i].halo = HALO_NONE;
        }
    }
    W->aud_enc_shapes = aud_enc_shapes(W->layers);
    W->dec_head_shapes = dec_head_shapes(W->layers);
    W->v6_gemm_shape = v6_gemm_shape(W->layers[10]);
    W->a1_valu_shape = a1_valu_shape(W->layers[0]);
    *out = W;
    return 0;
}

int avse_weights_act_exponents(const avse_weights* w, int* host_exp, int n) {
    if (!w || !host_exp || n < 0) return fail(AVSE_ERR_INVALID, "bad act_exponents args");
    for (int i = 0; i < n && i < kNumLayers; ++i) host_exp[i] = w->act_exp[i];
    return 0;
}

void avse_weights_destroy(avse_weights* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    delete w;
}

}  // extern "C"
