// The forward of libavse's C-ABI (include/avse.h): the layer plan of the reference's network.py executed as a sequence
// of HIP kernel launches on the caller's stream, its hipGraph replay cache, and the checked / profiled entry points.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "ctx.h"

using namespace avse;

namespace {

HaloArgs halo_args(const GpuLayer& G, const void* in, const void* video, int video_dtype, const float* vmean,
                   const float* vstd, void* out, long long out_clip_stride, int out_pix_stride, int out_c_off, int64_t N,
                   const Options& opt) {
    HaloArgs a;
    std::memset(&a, 0, sizeof(a));
    a.variant = G.halo;
    a.in = in;
    a.video = reinterpret_cast<const float*>(video);   // V1 loaders: float, or bytes when video_u8
    a.video_u8 = video_dtype == AVSE_VIDEO_U8;
    a.vmean = vmean;
    a.vstd = vstd;
    a.out = out;
    a.w = G.w_halo;
    a.mfma32 = opt.mfma32;
    a.no_planar = opt.no_planar;
    a.scale = G.scale_h;
    a.shift = G.shift;
    a.N = (int)N;
    a.Hc = G.def.hin;
    a.Wc = G.def.win;
    a.Ci = G.def.cin;
    a.Co = G.def.cout;
    a.out_clip_stride = out_clip_stride;
    a.out_pix_stride = out_pix_stride;
    a.out_c_off = out_c_off;
    return a;
}

// fused d_deconv4 -> d_deconv5 -> d_deconv6 (conv_dec.hip): window geometry from the layers' tap extents
DecTailArgs dec_tail_args(const GpuLayer& G4, const GpuLayer& G5, const avse_weights* W, const void* in, float* out,
                          int64_t N) {
    DecTailArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = reinterpret_cast<const bf16_t*>(in);
    a.out = out;
    a.N = (int)N;
    auto extents = [](const GpuLayer& G, int p, int& dy0, int& dy1, int& dx0, int& dx1) {
        dy0 = dx0 = 1 << 20;
        dy1 = dx1 = -(1 << 20);
        for (int t = 0; t < G.ph[p].ntaps; ++t) {
            const int2 d = G.htaps[G.ph[p].tap_off + t];
            dy0 = std::min(dy0, d.x); dy1 = std::max(dy1, d.x);
            dx0 = std::min(dx0, d.y); dx1 = std::max(dx1, d.y);
        }
    };
    a.w4 = reinterpret_cast<const bf16_t*>(G4.w);
    a.sc4 = G4.scale;
    a.sh4 = G4.shift;
    a.nt4 = G4.ph[0].ntaps;
    a.kpad4 = G4.ph[0].kpad;
    int dy0, dy1, dx0, dx1;
    extents(G4, 0, dy0, dy1, dx0, dx1);
    a.pt4 = -dy0; a.pl4 = -dx0; a.rows4 = G4.hq + dy1 - dy0; a.pitch4 = G4.wq + dx1 - dx0;
    // the kernel walks a phase's taps as a (dy0 - a, dx0 - b) grid with nx columns: check that layout
    bool grid_ok = true;
    auto tap_grid = [&](const GpuLayer& G, int p, int& dy, int& dx, int& nx) {
        const int2* t = G.htaps + G.ph[p].tap_off;
        const int nt = G.ph[p].ntaps;
        dy = t[0].x;
        dx = t[0].y;
        nx = 1;
        while (nx < nt && t[nx].x == dy) ++nx;
        for (int k = 0; k < nt; ++k)
            if (t[k].x != dy - k / nx || t[k].y != dx - k % nx) grid_ok = false;
    };
    tap_grid(G4, 0, a.dy4, a.dx4, a.nx4);
    a.w5 = reinterpret_cast<const bf16_t*>(G5.w);
    a.sc5 = G5.scale;
    a.sh5 = G5.shift;
    int ey0 = 1 << 20, ey1 = -(1 << 20), ex0 = 1 << 20, ex1 = -(1 << 20);
    for (int p = 0; p < 4 && p < G5.nphase; ++p) {
        a.nt5[p] = G5.ph[p].ntaps;
        a.kpad5[p] = G5.ph[p].kpad;
        a.woff5[p] = G5.ph[p].w_off;
        tap_grid(G5, p, a.dy5[p], a.dx5[p], a.nx5[p]);
        extents(G5, p, dy0, dy1, dx0, dx1);
        ey0 = std::min(ey0, dy0); ey1 = std::max(ey1, dy1);
        ex0 = std::min(ex0, dx0); ex1 = std::max(ex1, dx1);
    }
    a.pt5 = -ey0; a.pl5 = -ex0; a.rows5 = G5.hq + ey1 - ey0; a.pitch5 = G5.wq + ex1 - ex0;
    a.w6 = W->d6_w;
    a.b6 = W->d6_bias;
    // shapes the kernel is written for (network.py:125-133 at the 200-ms segment); anything else: k_conv
    const bool shape_ok = G4.def.kind == DECONV && G5.def.kind == DECONV && G4.hq == 40 && G4.wq == 10 &&
                          G4.def.cin == 128 && G4.def.cout == 64 && G4.nphase == 1 && G5.hq == 40 && G5.wq == 10 &&
                          G5.def.cin == 64 && G5.def.cout == 64 && G5.nphase == 4 && G5.def.sh == 2 && G5.def.sw == 2 &&
                          grid_ok;
    if (!shape_ok) a.N = 0;   // dec_tail_supported() refuses
    return a;
}

ConvArgs conv_args(const GpuLayer& G, const void* in, long long in_clip_stride, void* out, long long out_clip_stride,
                   int out_pix_stride, int out_c_off, int64_t N) {
    const LayerDef& L = G.def;
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = in;
    a.out = out;
    a.w = G.w;
    a.scale = G.scale;
    a.shift = G.shift;
    a.taps = G.taps;
    a.N = (int)N;
    a.Hi = L.hin;
    a.Wi = L.win;
    a.Ci = (L.kind == DENSE) ? L.cin : G.cin_pad;
    a.in_clip_stride = in_clip_stride;
    a.Hq = G.hq;
    a.Wq = G.wq;
    a.sy = (L.kind == CONV) ? L.sh : 1;
    a.sx = (L.kind == CONV) ? L.sw : 1;
    a.oys = (L.kind == DECONV) ? L.sh : 1;
    a.oxs = (L.kind == DECONV) ? L.sw : 1;
    a.Ho = G.ho;
    a.Wo = G.wo;
    a.Co = L.cout;
    a.out_clip_stride = out_clip_stride;
    a.out_pix_stride = out_pix_stride;
    a.out_c_off = out_c_off;
    a.pool = L.pool ? 1 : 0;
    a.act = 1;
    a.nphase = G.nphase;
    a.ksplit = 1;
    for (int p = 0; p < G.nphase; ++p) a.ph[p] = G.ph[p];
    return a;
}

// grows the forward scratch; never while `s` (nullable) is being captured into a graph: the caller must reserve first
int ensure_arena(avse_ctx* c, int64_t clips, int dtype, const ArenaShape& a, hipStream_t s) {
    // at least the N = 1 layout: a video == NULL forward runs a one-clip video encoder (and its split-K) in it
    const size_t need = std::max(arena_bytes(clips, dtype, c->opt, nullptr, a), arena_bytes(1, dtype, c->opt, nullptr, a));
    return grow(c->arena, need, s, "forward scratch", "call avse_ctx_reserve_weights(ctx, weights, max_clips) before the capture");
}

// One forward call: what its launches share.  Stages: avse_forward_profile's (include/avse.h AVSE_NUM_STAGES).
struct Run {
    avse_ctx* c;
    const avse_weights* W;
    const Options& opt;
    const NetPlan& P;
    hipStream_t s;          // the caller's stream
    hipEvent_t* ev;         // nullable: one event per stage boundary (profiling)
    const int dt;           // the weights' dtype
    const bool split;       // AVSE_F32_SPLIT: video convs on split-f16 operands, the rest fp32
    const int gdt;          // dtype of the generic kernels' buffers
    // launch_conv's arithmetic.  Split dtype: f16 split products; every generic layer writes its output as split pairs
    // (the next layer loads them as they are), except d_deconv5 (fused d_deconv6 -> float output, or fp32 unfused); the
    // layers fed by the fp32 preps (a_conv1, a generic v_conv1) split their fp32 input in the kernel
    const int cdt;
    const bool use_gemm;    // dense layers and v_conv6 on gemm.hip (bf16, and split pairs: k_gemm S16), not Options::no_gemm
    int stage = 0;

    Run(avse_ctx* c_, const avse_weights* W_, hipStream_t s_, hipEvent_t* ev_)
        : c(c_), W(W_), opt(c_->opt), P(W_->shape.plan), s(s_), ev(ev_), dt(W_->dtype), split(dt == AVSE_F32_SPLIT),
          gdt(dt == AVSE_BF16 ? AVSE_BF16 : AVSE_F32), cdt(split ? kConvSplit : gdt),
          use_gemm((dt == AVSE_BF16 || split) && !opt.no_gemm) {}

    const GpuLayer& L(int i) const { return W->layers[i]; }
    size_t es() const { return dt == AVSE_BF16 ? 2 : 4; }

    int mark() {
        if (ev) AVSE_HIP_CHECK(hipEventRecord(ev[stage], s));
        ++stage;
        return 0;
    }
    int mark(int n) {
        for (int k = 0; k < n; ++k)
            if (int rc = mark()) return rc;
        return 0;
    }

    // li: the layer's index in the plan (its range-guard bit); rflag: the range-guard word the kernels report into
    int pairs(ConvArgs& a, bool in_pairs, bool out_pairs, int li, unsigned* rflag) const {
        if (!split) return gdt;
        a.range_flag = rflag;
        a.range_bit = 1u << li;
        a.range_in_bit = li == 0 ? kRangeAudioIn : kRangeVideoIn;   // the fp32 input split on load (a_conv1, v_conv1)
        if (in_pairs) {
            a.Ci *= 2;
            a.in_clip_stride *= 2;
            for (int p = 0; p < a.nphase; ++p) {
                a.ph[p].kpad *= 2;
                a.ph[p].w_off *= 2;
            }
        }
        if (out_pairs) {
            a.out_s16 = 1;
            a.out_clip_stride *= 2;
            a.out_pix_stride *= 2;
            a.out_c_off *= 2;
        }
        return in_pairs ? kConvSplitPairs : kConvSplit;
    }

    // a generic layer launch: split-pair stride-1 gather layers on the windowed kernel (conv_win.hip) when it takes
    // their shape (option no_win: always k_conv)
    int conv(const ConvArgs& a, int dti, const GpuLayer& G, hipStream_t st) const {
        if (split && dti == kConvSplitPairs && !opt.no_win) {
            const int rw = launch_conv_win(a, G.htaps, st);
            if (rw != -1) return rw;
        }
        return launch_conv(a, split ? dti : cdt, st);
    }

    // v_conv6 or a dense layer (plan layer li) over n clips, split-K as split_plan says, the partials at part_off: the
    // split-K offset of the arena layout the launch's activations use (the N = 1 zero-video encoder has its own).  On
    // k_gemm; on k_conv + split-K reduce under Options::no_gemm, for AVSE_F32, for a v_conv6 of another shape, or when
    // a split launch has more tiles than k_gemm has split-K tickets (launch_gemm returns -1).
    int gemm_layer(int li, const void* in, long long lda, void* out, long long ldo, int out_pix_stride, int out_off,
                   int64_t n, size_t part_off, unsigned* rflag) const {
        const GpuLayer& G = L(li);
        const SplitPlan sp = split_plan(W->shape.split[li - kSplitFirst], n, dt, opt);
        float* partial = reinterpret_cast<float*>(c->arena + part_off);
        const int mode = li == kSplitFirst ? 1 : 0;   // v_conv6: 3 x 3 on 4 x 4 + pool
        if (use_gemm && (mode == 0 || W->v6_gemm_shape)) {
            GemmArgs g;
            std::memset(&g, 0, sizeof(g));
            g.a = reinterpret_cast<const bf16_t*>(in);
            g.w = reinterpret_cast<const bf16_t*>(G.w);
            g.out = reinterpret_cast<bf16_t*>(out);
            g.lda = split ? 2 * lda : lda;
            g.ldo = split ? 2 * ldo : ldo;
            g.out_off = split ? 2 * out_off : out_off;
            g.M = (int)(mode == 1 ? n * 16 : n); g.N = G.def.cout; g.kpad = G.ph[0].kpad;
            g.scale = G.scale; g.shift = G.shift; g.act = 1;
            g.ksplit = sp.gemm.ksplit; g.slabs_per_split = sp.gemm.slabs; g.partial = partial;
            g.counters = c->gemm_counters; g.counters_cap = kGemmCounters;
            g.split = split; g.four_products = opt.four_products;
            if (split) { g.range_flag = rflag; g.range_bit = 1u << li; }
            const int rc = launch_gemm(g, mode, s);
            if (rc != -1) return rc;
        }
        ConvArgs a = conv_args(G, in, lda, out, ldo, out_pix_stride, out_off, n);
        a.ksplit = sp.conv.ksplit; a.ksplit_slabs = sp.conv.slabs; a.partial = partial;
        const int dti = pairs(a, true, true, li, rflag);
        return launch_conv(a, split ? dti : cdt, s);
    }

    // video encoder (network.py:138-175) over n clips, activations at the arena offsets o, clip i's embedding at
    // element i * CAT + AEMB of cat (the concat rows, or packed rows: CAT 2048, AEMB 0), split-K partials at part_off;
    // record: its six launches are the v_conv1 .. v_conv6 stages
    int video_encoder(const void* vid, int vid_dt, const float* vm, const float* vs, int64_t n, const size_t* o,
                      void* cat, long long CAT, long long AEMB, size_t part_off, unsigned* rflag, bool record) {
        auto vb = [&](int b) { return (void*)(c->arena + o[b]); };
        const int v_in[6] = {B_VIN, B_V1, B_V2, B_V3, B_V4, B_V5};
        int rc;
        if (L(5).halo == HALO_NONE &&
            (rc = launch_video_prep(vid, vid_dt == AVSE_VIDEO_U8, vm, vs, vb(B_VIN), n, P.F, gdt, s)))
            return rc;
        for (int i = 0; i < 6; ++i) {
            const GpuLayer& G = L(5 + i);
            const long long in_cs = (long long)G.def.hin * G.def.win * (i == 0 ? G.cin_pad : G.def.cin);
            if (G.halo != HALO_NONE) {
                HaloArgs h = (i < 5) ? halo_args(G, vb(v_in[i]), vid, vid_dt, vm, vs, vb(v_in[i + 1]),
                                                 (long long)G.ho * G.wo * G.def.cout, G.def.cout, 0, n, opt)
                                     : halo_args(G, vb(v_in[i]), vid, vid_dt, vm, vs, cat, CAT, G.def.cout, AEMB, n, opt);
                if (split) {
                    // split-pair input (2 halves per channel) from the previous split layer; output split pairs for
                    // a next split layer, fp32 for a generic one (weights_load keeps the split layers a prefix)
                    // every consumer (the next split layer or the generic v_conv6) takes the pair layout
                    h.split = 1;
                    h.range_flag = rflag;
                    h.range_bit = 1u << (5 + i);
                    h.range_in_bit = kRangeVideoIn;
                    if (G.halo != HALO_V1 && G.halo != HALO_V1P) h.Ci = 2 * G.def.cin;
                    h.out_mode = OUT_S16;
                    h.out_clip_stride *= 2;
                    h.out_pix_stride *= 2;
                    h.out_c_off *= 2;
                }
                rc = G.halo == HALO_V1 || G.halo == HALO_V1P ? launch_conv_v1r(h, s) : launch_conv_stream(h, s);
            } else if (i == 5) {
                rc = gemm_layer(5 + i, vb(v_in[i]), in_cs, cat, CAT, G.def.cout, AEMB, n, part_off, rflag);   // concat[aemb:]
            } else {
                ConvArgs a = conv_args(G, vb(v_in[i]), in_cs, vb(v_in[i + 1]), (long long)G.ho * G.wo * G.def.cout, G.def.cout, 0, n);
                const int dti = pairs(a, i > 0, true, 5 + i, rflag);   // v_conv1 generic: fp32 video-prep input
                rc = launch_conv(a, split ? dti : cdt, s);
            }
            if (rc || (record && (rc = mark()))) return rc;
        }
        return 0;
    }

    // All-zero video: the embedding is one constant 2048-vector, computed once per weights object by an N = 1 video
    // encoder in the N = 1 arena layout, with its own range word (kept with the embedding), outside the profiled stages.
    int zero_video_embedding() {
        if (W->vzero_emb.load(std::memory_order_acquire)) return 0;
        std::lock_guard<std::mutex> lk(W->vzero_mu);
        if (W->vzero_emb.load(std::memory_order_relaxed)) return 0;
        if (int rc = not_capturing(s, "the all-zero-video embedding must be computed before graph capture")) return rc;
        if (!c->zero_video) {
            AVSE_HIP_CHECK(c->zero_video.alloc(sizeof(float) * 128 * 128 * 8));
            AVSE_HIP_CHECK(hipMemsetAsync(c->zero_video, 0, sizeof(float) * 128 * 128 * 8, s));
        }
        Owned<char> emb;
        AVSE_HIP_CHECK(emb.alloc(2048 * es()));
        size_t o1[B_COUNT + 1];
        arena_bytes(1, dt, opt, o1, W->shape);
        unsigned* flag = c->range + 2;
        if (split) AVSE_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(unsigned), s));
        if (int rc = video_encoder(c->zero_video, AVSE_VIDEO_F32, nullptr, nullptr, 1, o1, c->arena + o1[B_CAT], P.cat, P.aemb, o1[B_COUNT],
                                   flag, false))
            return rc;
        AVSE_HIP_CHECK(hipMemcpyAsync(emb, c->arena + o1[B_CAT] + P.aemb * es(), 2048 * es(), hipMemcpyDeviceToDevice, s));
        if (split) AVSE_HIP_CHECK(hipMemcpyAsync(c->range_host + 2, flag, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        // one-time: the embedding is complete before any stream can see the pointer
        AVSE_HIP_CHECK(hipStreamSynchronize(s));
        W->vzero_range = split ? c->range_host[2] : 0u;
        W->vzero_emb.store(emb.p.release(), std::memory_order_release);   // W owns it from here
        return 0;
    }
};

// A mixed forward (avse_forward_mixed): M of the N clips have video, 0 < M < N (mixed_resolve turns the other masks
// into the plain calls), and `video` holds those M packed in clip order.
struct Mixed {
    const uint8_t* present;   // HOST [N]
    int64_t M;
};

// What a mixed forward keeps behind the N-clip arena layout, whose offsets it leaves alone: room for [N][2048]
// embeddings, of which the video encoder writes the first M, packed (sized by N so that the offsets behind it do not
// depend on the mask), the row map [N] and the split-K partials of the encoder's M-clip launches (the
// N-clip workspace need not hold them: a plan splits short grids only).  Nothing else addresses this tail, so it is
// free whatever the side stream runs.  Returns the arena size.
struct MixedTail {
    size_t emb, map, ws;
};
size_t mixed_tail(int64_t N, int64_t M, int dtype, const Options& o, const ArenaShape& a, MixedTail* t) {
    const size_t es = dtype == AVSE_BF16 ? 2 : 4;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t off = std::max(arena_bytes(N, dtype, o, nullptr, a), arena_bytes(1, dtype, o, nullptr, a));
    t->emb = off;
    off += up((size_t)N * 2048 * es);
    t->map = off;
    off += up((size_t)N * sizeof(int));
    t->ws = off;
    return off + up(split_ws_bytes(M, dtype, o, a));
}

// The row map of a mixed forward, built in the next slot of the context's pinned ring and copied to `dev` on s: row i
// is clip i's row of the packed embeddings, -1 for a clip without video.  Waits only when MAP_SLOTS maps are in flight.
int upload_row_map(avse_ctx* c, const Mixed& mx, int64_t N, int* dev, hipStream_t s) {
    if ((size_t)N > c->map_cap) {   // the ring grows, never per call: every copy out of the old one has to be done
        for (int i = 0; i < avse_ctx::MAP_SLOTS; ++i) {
            if (c->map_used[i]) AVSE_HIP_CHECK(hipEventSynchronize(c->map_ev[i]));
            c->map_used[i] = false;
            if (!c->map_ev[i]) AVSE_HIP_CHECK(hipEventCreateWithFlags(&c->map_ev[i], hipEventDisableTiming));
        }
        const size_t cap = std::max<size_t>(1024, (size_t)N * 2);
        c->map_cap = 0;
        if (c->map_host.alloc(sizeof(int) * cap * avse_ctx::MAP_SLOTS) != hipSuccess)
            return fail(AVSE_ERR_OOM, "hipHostMalloc failed (mixed forward row map)");
        c->map_cap = cap;
    }
    const int i = c->map_slot;
    if (c->map_used[i]) AVSE_HIP_CHECK(hipEventSynchronize(c->map_ev[i]));
    int* host = c->map_host + (size_t)i * c->map_cap;
    int m = 0;
    for (int64_t k = 0; k < N; ++k) host[k] = mx.present[k] ? m++ : -1;
    AVSE_HIP_CHECK(hipMemcpyAsync(dev, host, sizeof(int) * (size_t)N, hipMemcpyHostToDevice, s));
    AVSE_HIP_CHECK(hipEventRecord(c->map_ev[i], s));
    c->map_used[i] = true;
    c->map_slot = (i + 1) % avse_ctx::MAP_SLOTS;
    return 0;
}

// rflag: the split dtype's range-guard word the kernels report into (avse_ctx::range)
// vdt: avse_video_dtype of `video`
// mx: nullable, a mixed forward (not capturable: its row map goes up from the host)
int forward_impl(avse_ctx* c, const avse_weights* W, const float* audio, const void* video, int vdt, const float* vmean,
                 const float* vstd, int64_t N, float* out, hipStream_t s, hipEvent_t* ev, unsigned* rflag,
                 const Mixed* mx = nullptr) {
    if (!c || !W || !audio || !out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (vdt != AVSE_VIDEO_F32 && vdt != AVSE_VIDEO_U8) return fail(AVSE_ERR_INVALID, "unknown video dtype");
    if (vdt == AVSE_VIDEO_U8 && ((uintptr_t)video & 3))
        return fail(AVSE_ERR_INVALID, "uint8 video must be 4-byte aligned (alignment of the base pointer)");
    if ((vmean == nullptr) != (vstd == nullptr)) return fail(AVSE_ERR_INVALID, "vnorm_mean and vnorm_std must both be set or both NULL");
    if (!video && vmean) return fail(AVSE_ERR_INVALID, "video == NULL (all-zero video) takes no normaliser");
    if (N < 0 || N > (int64_t)(1 << 30) / (128 * 128)) return fail(AVSE_ERR_INVALID, "bad N");
    if (N == 0) return 0;
    if (W->device != c->device) return fail(AVSE_ERR_INVALID, "weights and context are on different devices");
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    int rc = ensure_arena(c, N, W->dtype, W->shape, s);
    if (rc) return rc;
    MixedTail tail{};
    if (mx) {
        if (!video || mx->M <= 0 || mx->M >= N) return fail(AVSE_ERR_INVALID, "mixed forward: bad mask");
        if ((rc = not_capturing(s, "a mixed forward uploads its row map from the host: not inside a capture"))) return rc;
        const size_t need = mixed_tail(N, mx->M, W->dtype, c->opt, W->shape, &tail);
        if ((rc = grow(c->arena, need, s, "forward scratch"))) return rc;
    }
    c->last_shape = W->shape;
    Run r(c, W, s, ev);
    const Options& opt = r.opt;
    const NetPlan& P = r.P;
    const int dt = r.dt, gdt = r.gdt;
    const bool split = r.split;
    size_t off[B_COUNT + 1];
    arena_bytes(N, dt, opt, off, W->shape);
    const long long CAT = P.cat, AEMB = P.aemb, EMB = P.emb;
    auto buf = [&](int b) { return (void*)(c->arena + off[b]); };
    auto L = [&](int i) -> const GpuLayer& { return W->layers[i]; };
    if ((rc = r.mark(2))) return rc;   // video_prep stage: now the video encoder's first launch (k_conv path only); audio_prep
    // The all-zero-video embedding runs here, before the audio branch is launched: the per-layer audio branch runs on
    // the side stream and its N-clip buffers overlap the N = 1 layout (round 3: a race that broke video == NULL
    // forwards whenever the audio encoder was not the fused kernel, e.g. at 29.97 fps)
    if ((!video || mx) && (rc = r.zero_video_embedding())) return rc;
    int* row_of = reinterpret_cast<int*>(c->arena + tail.map);
    if (mx && (rc = upload_row_map(c, *mx, N, row_of, s))) return rc;
    // audio encoder (network.py:88-109): one fused kernel per clip (conv_aud.hip) when the layers have the network's
    // shapes (AVSE_NO_AUDENC=1: per-layer launches); profiled, its time shows as the audio_prep stage
    bool aud_fused = false;
    AudEncArgs aa;
    std::memset(&aa, 0, sizeof(aa));
    if (dt == AVSE_BF16) {
        aa.mel = audio;
        aa.out = reinterpret_cast<bf16_t*>(buf(B_CAT));
        aa.out_clip_stride = CAT;
        aa.N = (int)N;
        aa.w1 = (const bf16_t*)L(0).w_dense; aa.w2 = (const bf16_t*)L(1).w; aa.w3 = (const bf16_t*)L(2).w;
        aa.w4 = (const bf16_t*)L(3).w; aa.w5 = (const bf16_t*)L(4).w;
        for (int i = 0; i < 5; ++i) { aa.sc[i] = L(i).scale; aa.sh[i] = L(i).shift; }
        aud_fused = W->aud_enc_shapes && !opt.no_audenc && aud_enc_supported(aa);
    }

    // The per-layer audio branch (prep + a_conv1..5 -> concat[0:3200]) shares no buffer with the video encoder until
    // the fusion dense: it runs on the context's side stream, forked from and joined back into s, so its short,
    // latency-bound kernels overlap the video encoder (the profiling path keeps one stream for per-stage events;
    // AVSE_SERIAL=1 forces it).  The fork waits for everything enqueued on s before this call.
    // The fused audio encoder runs on the caller's stream: beside the persistent video convolutions its 152-KB
    // workgroups hold whole CUs they wait for (measured: concurrent 2.377 ms vs serial 2.304 ms per step), and the
    // fork / join events alone cost ~25 us of idle GPU per step (rocprof trace).  (The side-stream option for it was
    // removed in round 3, as was tile_alt, v_conv2 / v_conv4 tiles walked last-first: both measured no gain.)
    const bool concurrent = ev == nullptr && !opt.serial && !aud_fused;
    hipStream_t sa = s;
    if (concurrent) {
        if (!c->side) {
            if (opt.side_prio) {
                int least = 0, greatest = 0;
                AVSE_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
                AVSE_HIP_CHECK(hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, opt.side_prio == 1 ? least : greatest));
            } else {
                AVSE_HIP_CHECK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
            }
            AVSE_HIP_CHECK(hipEventCreateWithFlags(&c->fork, hipEventDisableTiming));
            AVSE_HIP_CHECK(hipEventCreateWithFlags(&c->join, hipEventDisableTiming));
        }
        AVSE_HIP_CHECK(hipEventRecord(c->fork, s));
        AVSE_HIP_CHECK(hipStreamWaitEvent(c->side, c->fork, 0));
        sa = c->side;
    }
    if (aud_fused && ((rc = launch_aud_enc(aa, s)) || (rc = r.mark(6)))) return rc;   // audio_prep (= the fused kernel), a_conv1..a_conv5
    // split: a_conv1 on the vector ALUs from the audio input itself (conv.hip k_aconv1_split; no audio_prep copy)
    const bool a1_valu = split && !aud_fused && !opt.no_a1valu && W->a1_valu_shape;
    if (a1_valu) {
        const GpuLayer& G = L(0);
        const int pt = std::max((G.ho - 1) * G.def.sh + G.def.kh - G.def.hin, 0) / 2;
        const int pl = std::max((G.wo - 1) * G.def.sw + G.def.kw - G.def.win, 0) / 2;
        if ((rc = r.mark()) ||
            (rc = launch_aconv1_split(audio, G.w_f32, G.scale, G.shift, buf(B_A1), N, G.def.hin, G.def.win, G.ho, G.wo,
                                      G.def.kh, G.def.kw, G.def.sh, pt, pl, G.def.cout, rflag, 1u, kRangeAudioIn, sa)) ||
            (rc = r.mark()))
            return rc;
    }
    if (!aud_fused && !a1_valu && ((rc = launch_audio_prep(audio, buf(B_AIN), N * kMels * P.T, gdt, sa)) || (rc = r.mark()))) return rc;
    const int a_in[5] = {B_AIN, B_A1, B_A2, B_A3, B_A4};
    for (int i = a1_valu ? 1 : 0; i < 5 && !aud_fused; ++i) {
        const GpuLayer& G = L(i);
        const long long in_cs = (long long)G.def.hin * G.def.win * (i == 0 ? G.cin_pad : G.def.cin);
        ConvArgs a = (i < 4) ? conv_args(G, buf(a_in[i]), in_cs, buf(a_in[i + 1]), (long long)G.ho * G.wo * G.def.cout, G.def.cout, 0, N)
                             : conv_args(G, buf(a_in[i]), in_cs, buf(B_CAT), CAT, G.def.cout, 0, N);   // Flatten -> concat[0:aemb]
        const int dti = r.pairs(a, i > 0, true, i, rflag);   // a_conv1: fp32 audio-prep input
        if ((rc = r.conv(a, dti, G, sa)) || (rc = r.mark())) return rc;
    }
    if (concurrent) AVSE_HIP_CHECK(hipEventRecord(c->join, sa));
    if (mx) {
        // the encoder over the M packed clips, in the N-clip layout's activation buffers, then every concat row from
        // its clip's packed embedding or the constant one
        const size_t es = r.es();
        char* emb = c->arena + tail.emb;
        if ((rc = r.video_encoder(video, vdt, vmean, vstd, mx->M, off, emb, 2048, 0, tail.ws, rflag, true))) return rc;
        if ((rc = launch_gather_rows(emb, W->vzero_emb.load(std::memory_order_acquire), row_of, (char*)buf(B_CAT) + AEMB * es,
                                     N, 2048 * es, 2048 * es, CAT * es, s)))
            return rc;
        if (split && W->vzero_range && rflag && (rc = launch_flag_or(rflag, W->vzero_range, s))) return rc;
    } else if (video) {
        if ((rc = r.video_encoder(video, vdt, vmean, vstd, N, off, buf(B_CAT), CAT, AEMB, off[B_COUNT], rflag, true))) return rc;
    } else {
        // all-zero video: broadcast the constant embedding computed above
        const size_t es = r.es();
        if ((rc = launch_broadcast_row(W->vzero_emb.load(std::memory_order_acquire), (char*)buf(B_CAT) + AEMB * es, N, 2048 * es, CAT * es, s))) return rc;
        // an embedding that left the pair range reports it in every forward that broadcasts it
        if (split && W->vzero_range && rflag && (rc = launch_flag_or(rflag, W->vzero_range, s))) return rc;
        if ((rc = r.mark(6))) return rc;   // v_conv1..v_conv6 stages (the broadcast shows as v_conv1)
    }
    if (concurrent) AVSE_HIP_CHECK(hipStreamWaitEvent(s, c->join, 0));
    // fusion + decoder dense (network.py:53-58, :66-78)
    const struct { int li, in, out; long long lda, ldo; } dense[3] = {
        {11, B_CAT, B_E1, CAT, EMB}, {12, B_E1, B_E2, EMB, EMB}, {13, B_E2, B_E3, EMB, AEMB}};
    for (const auto& d : dense)
        if ((rc = r.gemm_layer(d.li, buf(d.in), d.lda, buf(d.out), d.ldo, (int)d.ldo, 0, N, off[B_COUNT], rflag)) || (rc = r.mark()))
            return rc;
    // audio decoder (network.py:112-135)
    const int d_in[6] = {B_E3, B_D1, B_D2, B_D3, B_D4, B_D5};
    for (int i = 0; i < 5; ++i) {
        const GpuLayer& G = L(14 + i);
        const long long in_cs = (long long)G.def.hin * G.def.win * G.def.cin;
        if (i == 0 && dt == AVSE_BF16 && W->dec_head_shapes && !opt.no_dechead) {
            // d_deconv1 + d_deconv2 + d_deconv3 in one kernel, one workgroup per clip (conv_dech.hip)
            DecHeadArgs ha;
            std::memset(&ha, 0, sizeof(ha));
            ha.in = reinterpret_cast<const bf16_t*>(buf(B_E3));
            ha.in_clip_stride = AEMB;
            ha.out = reinterpret_cast<bf16_t*>(buf(B_D3));
            ha.out_clip_stride = 40 * 10 * 128;
            ha.N = (int)N;
            ha.w1 = (const bf16_t*)L(14).w; ha.w2 = (const bf16_t*)L(15).w; ha.w3 = (const bf16_t*)L(16).w;
            for (int k = 0; k < 3; ++k) { ha.sc[k] = L(14 + k).scale; ha.sh[k] = L(14 + k).shift; }
            if (dec_head_supported(ha)) {
                if ((rc = launch_dec_head(ha, s)) || (rc = r.mark(3))) return rc;
                i = 2;   // continue with d_deconv4
                continue;
            }
        }
        if (i == 3 && dt != AVSE_F32 && !opt.unfused_tail && !opt.no_dectail) {
            // d_deconv4 + d_deconv5 + d_deconv6 in one kernel: one workgroup per clip (conv_dec.hip, bf16), per half
            // clip on split pairs (conv_dects.hip)
            DecTailArgs da = dec_tail_args(L(17), L(18), W, buf(d_in[3]), out, N);
            if (split) {
                da.range_flag = rflag;
                da.range_bit = 1u << 17;
                da.four_products = opt.four_products;
            }
            if (split ? dec_tail_s16_supported(da) : dec_tail_supported(da)) {
                if ((rc = split ? launch_dec_tail_s16(da, s) : launch_dec_tail(da, s)) || (rc = r.mark(2))) return rc;   // d4, d5 stages
                break;
            }
        }
        if (i == 4 && !opt.unfused_tail) {
            // d_deconv5 with d_deconv6 (1x1, 64 -> 1, network.py:133) fused into its epilogue: the 64-channel
            // [N, 80, 20] activation is never written; orow addresses the float output pixel directly
            ConvArgs a = conv_args(G, buf(d_in[i]), in_cs, nullptr, (long long)G.ho * G.wo, 1, 0, N);
            a.fuse_w = W->d6_w;
            a.fuse_bias = W->d6_bias;
            a.fuse_out = out;
            const int dti = r.pairs(a, true, false, 14 + i, rflag);
            if ((rc = r.conv(a, dti, G, s)) || (rc = r.mark())) return rc;
            continue;
        }
        ConvArgs a = conv_args(G, buf(d_in[i]), in_cs, buf(d_in[i + 1]), (long long)G.ho * G.wo * G.def.cout, G.def.cout, 0, N);
        const int dti = r.pairs(a, true, i < 4 || !opt.unfused_tail, 14 + i, rflag);   // an unfused d_deconv5 feeds launch_out_conv fp32
        if ((rc = r.conv(a, dti, G, s)) || (rc = r.mark())) return rc;
    }
    if (opt.unfused_tail) {
        if ((rc = launch_out_conv(buf(B_D5), W->d6_w, W->d6_bias, out, N * kMels * P.T, gdt, s)) || (rc = r.mark())) return rc;
    } else if ((rc = r.mark())) {   // d_deconv6: fused into d_deconv5 above
        return rc;
    }
    return 0;
}

// avse_forward replays a hipGraph of the forward once the same arguments (weights, input / output pointers, N, the
// context's scratch arena and its Options) come a second time: the first call launches directly,
// the second captures and launches the graph, later ones replay it — the ~15 kernels then run without the per-kernel
// dispatch gaps of stream launches.  The graph bakes the pointers in; every argument set has its own entry (at most 8
// are kept).  Opt-in (AVSE_GRAPH=1): a torch graph of the whole bench step (spectrogram + forward) measured 2.20 ->
// 2.14 ms (tools/graph_probe.py), but replaying the forward alone inside the same step measured 2.234 vs 2.24-2.26 ms
// direct (bench.py A/B, same box), so direct launches stay the default.
int forward_dispatch(avse_ctx* c, const avse_weights* W, const float* audio, const void* video, int vdt,
                     const float* vmean, const float* vstd, int64_t N, float* out, void* stream, unsigned* rflag,
                     const Mixed* mx = nullptr) {
    if (!c || !W || N <= 0 || !c->opt.graph || mx)   // a mixed forward is never replayed: its mask is host data
        return forward_impl(c, W, audio, video, vdt, vmean, vstd, N, out, (hipStream_t)stream, nullptr, rflag, mx);
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    if (W->device != c->device) return fail(AVSE_ERR_INVALID, "weights and context are on different devices");
    int rc = ensure_arena(c, N, W->dtype, W->shape, (hipStream_t)stream);   // no allocation inside the capture
    if (rc) return rc;
    const void* key[10] = {(const void*)W->serial, audio, video, vmean, vstd, out, c->arena.p.get(), (const void*)c->arena.bytes,
                           rflag, (const void*)(uintptr_t)vdt};
    avse_ctx::Graph* hit = nullptr;
    for (auto& g : c->graphs)
        if (g.n == N && std::memcmp(&g.opt, &c->opt, sizeof(Options)) == 0 && std::memcmp(g.key, key, sizeof(key)) == 0)
            hit = &g;
    if (hit && hit->exec) {
        AVSE_HIP_CHECK(hipGraphLaunch(hit->exec, (hipStream_t)stream));
        return 0;
    }
    if (!hit) {   // first sighting of this argument set: launch directly (a one-off call pays no capture)
        if (c->graphs.size() >= 8) {
            if (c->graphs.front().exec) (void)hipGraphExecDestroy(c->graphs.front().exec);
            c->graphs.erase(c->graphs.begin());
        }
        avse_ctx::Graph g;
        std::memcpy(g.key, key, sizeof(key));
        g.n = N;
        g.opt = c->opt;
        g.exec = nullptr;
        c->graphs.push_back(g);
        return forward_impl(c, W, audio, video, vdt, vmean, vstd, N, out, (hipStream_t)stream, nullptr, rflag);
    }
    if (!c->cap) AVSE_HIP_CHECK(hipStreamCreateWithFlags(&c->cap, hipStreamNonBlocking));
    AVSE_HIP_CHECK(hipStreamBeginCapture(c->cap, hipStreamCaptureModeRelaxed));
    rc = forward_impl(c, W, audio, video, vdt, vmean, vstd, N, out, c->cap, nullptr, rflag);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(c->cap, &graph);
    if (rc || ce != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc ? rc : fail(AVSE_ERR_HIP, std::string("forward capture: ") + hipGetErrorString(ce));
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) return fail(AVSE_ERR_HIP, std::string("forward graph instantiate: ") + hipGetErrorString(ie));
    hit->exec = exec;
    AVSE_HIP_CHECK(hipGraphLaunch(exec, (hipStream_t)stream));
    return 0;
}

// The mask of a mixed call, before any GPU work: counts the clips with video and turns the masks that need no row map
// into the plain calls (all present: `video` is the whole batch; none: video == NULL, which takes no normaliser).
// *mixed: 0 < M < N, and mx describes it.
int mixed_resolve(const uint8_t* present, const void*& video, const float*& vmean, const float*& vstd, int64_t N,
                  Mixed* mx, bool* mixed) {
    *mixed = false;
    if (N < 0 || N > (int64_t)(1 << 30) / (128 * 128)) return fail(AVSE_ERR_INVALID, "bad N");
    if (!present) return fail(AVSE_ERR_INVALID, "present is NULL");
    if ((vmean == nullptr) != (vstd == nullptr)) return fail(AVSE_ERR_INVALID, "vnorm_mean and vnorm_std must both be set or both NULL");
    int64_t M = 0;
    for (int64_t i = 0; i < N; ++i) M += present[i] != 0;
    if (M > 0 && !video) return fail(AVSE_ERR_INVALID, "video == NULL but the mask has clips with video");
    if (M == 0) {
        video = nullptr;
        vmean = vstd = nullptr;
    }
    mx->present = present;
    mx->M = M;
    *mixed = M > 0 && M < N;
    return 0;
}

// avse_forward_checked_video, and avse_forward_mixed_checked with its mask resolved (mx, nullable)
int forward_checked(avse_ctx* c, const avse_weights* W, const float* audio, const void* video, int vdt, const float* vmean,
                    const float* vstd, int64_t N, float* out, void* stream, int mode, uint32_t* host_bits, const Mixed* mx) {
    if (host_bits) *host_bits = 0;
    if (!c || !W) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (mode != AVSE_RANGE_RECOMPUTE && mode != AVSE_RANGE_ERROR) return fail(AVSE_ERR_INVALID, "bad range mode");
    if (W->dtype != AVSE_F32_SPLIT || N <= 0) {
        if (int rc = forward_dispatch(c, W, audio, video, vdt, vmean, vstd, N, out, stream, c->range.p.get(), mx)) return rc;
        return avse::debug_poll(stream);
    }
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = not_capturing(s, "avse_forward_checked waits for its stream: capture avse_forward instead")) return rc;
    unsigned* flag = c->range + 1;
    AVSE_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(unsigned), s));
    // (option graph: the forward itself replays its hipGraph, so the launches after each wait are one graph launch)
    if (int rc = forward_dispatch(c, W, audio, video, vdt, vmean, vstd, N, out, stream, flag, mx)) return rc;
    AVSE_HIP_CHECK(hipMemcpyAsync(c->range_host + 1, flag, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    AVSE_HIP_CHECK(hipStreamSynchronize(s));
    const unsigned bits = c->range_host[1];
    if (host_bits) *host_bits = bits;
    if (!bits) return avse::debug_poll(stream);
    if (mode == AVSE_RANGE_ERROR)
        return fail(AVSE_ERR_RANGE, "AVSE_F32_SPLIT: an activation left the f16 pair range (range bits 0x" +
                                        [](unsigned b) { char t[16]; std::snprintf(t, sizeof(t), "%x", b); return std::string(t); }(bits) +
                                        "): the outputs are not float32-accurate");
    // recompute the batch on the exact-fp32 network (the same kernels as AVSE_F32 weights), built once from the blob
    const avse_weights* twin = nullptr;
    {
        std::lock_guard<std::mutex> lk(W->twin_mu);
        if (!W->f32_twin) {
            avse_weights* t = nullptr;
            if (int rc = avse_weights_load_shape(c, W->blob.data(), (int64_t)W->blob.size(), AVSE_F32, W->shape.plan.T,
                                                 W->shape.plan.F, &t))
                return rc;
            W->f32_twin = t;
        }
        twin = W->f32_twin;
    }
    if (int rc = forward_impl(c, twin, audio, video, vdt, vmean, vstd, N, out, s, nullptr, nullptr, mx)) return rc;
    return avse::debug_poll(stream);
}

}  // namespace

extern "C" {

int avse_ctx_reserve(avse_ctx* c, int64_t max_clips, int dtype) {
    if (!c || max_clips < 0 || !valid_dtype(dtype)) return fail(AVSE_ERR_INVALID, "bad reserve args");
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    return ensure_arena(c, max_clips, dtype, arena_shape(kPlan25), nullptr);   // the 25-fps network's scratch
}

int avse_ctx_reserve_weights(avse_ctx* c, const avse_weights* w, int64_t max_clips) {
    if (!c || !w || max_clips < 0) return fail(AVSE_ERR_INVALID, "bad reserve args");
    if (w->device != c->device) return fail(AVSE_ERR_INVALID, "weights and context are on different devices");
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    return ensure_arena(c, max_clips, w->dtype, w->shape, nullptr);   // the network shape these weights were built for
}

int avse_forward(avse_ctx* c, const avse_weights* W, const float* audio, const float* video, const float* vmean,
                 const float* vstd, int64_t N, float* out, void* stream) {
    return avse_forward_video(c, W, audio, video, AVSE_VIDEO_F32, vmean, vstd, N, out, stream);
}

int avse_forward_video(avse_ctx* c, const avse_weights* W, const float* audio, const void* video, int vdt,
                       const float* vmean, const float* vstd, int64_t N, float* out, void* stream) {
    if (int rc = forward_dispatch(c, W, audio, video, vdt, vmean, vstd, N, out, stream, c ? c->range.p.get() : nullptr))
        return rc;
    return avse::debug_poll(stream);
}

int avse_forward_mixed(avse_ctx* c, const avse_weights* W, const float* audio, const void* video, int vdt,
                       const float* vmean, const float* vstd, const uint8_t* present, int64_t N, float* out, void* stream) {
    Mixed mx{};
    bool mixed = false;
    if (int rc = mixed_resolve(present, video, vmean, vstd, N, &mx, &mixed)) return rc;
    if (int rc = forward_dispatch(c, W, audio, video, vdt, vmean, vstd, N, out, stream, c ? c->range.p.get() : nullptr,
                                  mixed ? &mx : nullptr))
        return rc;
    return avse::debug_poll(stream);
}

int avse_forward_mixed_checked(avse_ctx* c, const avse_weights* W, const float* audio, const void* video, int vdt,
                               const float* vmean, const float* vstd, const uint8_t* present, int64_t N, float* out,
                               void* stream, int mode, uint32_t* host_bits) {
    if (host_bits) *host_bits = 0;
    Mixed mx{};
    bool mixed = false;
    if (int rc = mixed_resolve(present, video, vmean, vstd, N, &mx, &mixed)) return rc;
    return forward_checked(c, W, audio, video, vdt, vmean, vstd, N, out, stream, mode, host_bits, mixed ? &mx : nullptr);
}

int avse_range_status(avse_ctx* c, void* stream, uint32_t* host_bits) {
    if (!c || !host_bits) return fail(AVSE_ERR_INVALID, "NULL argument");
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = not_capturing(s, "avse_range_status waits for its stream: not inside a capture")) return rc;
    AVSE_HIP_CHECK(hipMemcpyAsync(c->range_host, c->range, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    AVSE_HIP_CHECK(hipMemsetAsync(c->range, 0, sizeof(unsigned), s));
    AVSE_HIP_CHECK(hipStreamSynchronize(s));
    *host_bits = c->range_host[0];
    return 0;
}

int avse_range_snapshot(avse_ctx* c, void* stream, uint32_t* host_word) {
    if (!c || !host_word) return fail(AVSE_ERR_INVALID, "NULL argument");
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    AVSE_HIP_CHECK(hipMemcpyAsync(host_word, c->range, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    AVSE_HIP_CHECK(hipMemsetAsync(c->range, 0, sizeof(unsigned), s));
    return 0;
}

int avse_forward_checked(avse_ctx* c, const avse_weights* W, const float* audio, const float* video, const float* vmean,
                         const float* vstd, int64_t N, float* out, void* stream, int mode, uint32_t* host_bits) {
    return avse_forward_checked_video(c, W, audio, video, AVSE_VIDEO_F32, vmean, vstd, N, out, stream, mode, host_bits);
}

int avse_forward_checked_video(avse_ctx* c, const avse_weights* W, const float* audio, const void* video, int vdt,
                               const float* vmean, const float* vstd, int64_t N, float* out, void* stream, int mode,
                               uint32_t* host_bits) {
    return forward_checked(c, W, audio, video, vdt, vmean, vstd, N, out, stream, mode, host_bits, nullptr);
}

int avse_forward_profile(avse_ctx* c, const avse_weights* W, const float* audio, const float* video,
                         const float* vmean, const float* vstd, int64_t N, float* out, void* stream, float* host_ms) {
    return avse_forward_profile_video(c, W, audio, video, AVSE_VIDEO_F32, vmean, vstd, N, out, stream, host_ms);
}

int avse_forward_profile_video(avse_ctx* c, const avse_weights* W, const float* audio, const void* video, int vdt,
                               const float* vmean, const float* vstd, int64_t N, float* out, void* stream,
                               float* host_ms) {
    if (!host_ms) return fail(AVSE_ERR_INVALID, "host_ms is NULL");
    if (c) AVSE_HIP_CHECK(hipSetDevice(c->device));
    hipEvent_t ev[AVSE_NUM_STAGES + 1];
    for (int i = 0; i <= AVSE_NUM_STAGES; ++i) AVSE_HIP_CHECK(hipEventCreate(&ev[i]));
    int rc = forward_impl(c, W, audio, video, vdt, vmean, vstd, N, out, (hipStream_t)stream, ev, c ? c->range.p.get() : nullptr);
    if (!rc) {
        AVSE_HIP_CHECK(hipEventSynchronize(ev[AVSE_NUM_STAGES]));
        for (int i = 0; i < AVSE_NUM_STAGES; ++i) {
            float ms = 0.f;
            AVSE_HIP_CHECK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            host_ms[i] = ms;
        }
    }
    for (int i = 0; i <= AVSE_NUM_STAGES; ++i) (void)hipEventDestroy(ev[i]);
    return rc;
}

int avse_debug_scratch(avse_ctx* c, int64_t N, int dtype, void** base, int64_t* offsets) {
    if (!c || !base || !offsets || N <= 0) return fail(AVSE_ERR_INVALID, "bad debug_scratch args");
    size_t off[B_COUNT + 1];
    const size_t need = arena_bytes(N, dtype, c->opt, off, c->last_shape);
    if (!c->arena || need > c->arena.bytes) return fail(AVSE_ERR_INVALID, "no forward scratch of that size yet");
    *base = c->arena;
    for (int b = 0; b < B_COUNT; ++b) offsets[b] = (int64_t)off[b];
    return 0;
}

}  // extern "C"
