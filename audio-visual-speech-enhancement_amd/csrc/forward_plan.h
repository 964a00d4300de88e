// Host-only forward plan (no HIP header): the layout of the forward's scratch arena and split_plan, the one place that
// decides how v_conv6 and the dense layers split their reduction.  forward.hip's launches and arena_bytes both read it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/avse.h"
#include "layer_geom.h"
#include "options.h"

namespace avse {

// per-clip activation buffers of the forward scratch, in launch order
enum Buf { B_VIN, B_AIN, B_A1, B_A2, B_A3, B_A4, B_V1, B_V2, B_V3, B_V4, B_V5, B_CAT, B_E1, B_E2, B_E3,
           B_D1, B_D2, B_D3, B_D4, B_D5, B_COUNT };
inline size_t buf_elems(const NetPlan& p, int b) {
    const size_t T = p.T, w1 = (T + 1) / 2, w3 = p.W5;
    const size_t e[B_COUNT] = {128 * 128 * 8, 80 * T * 8, 40 * w1 * 64, 40 * w1 * 64, 20 * w3 * 128,
                               10 * w3 * 128, 64 * 64 * 128, 32 * 32 * 128, 16 * 16 * 256, 8 * 8 * 256,
                               4 * 4 * 512, (size_t)p.cat, (size_t)p.emb, (size_t)p.emb, (size_t)p.aemb,
                               10 * w3 * 128, 20 * w3 * 128, 40 * 2 * w3 * 128, 40 * 2 * w3 * 64, 80 * 4 * w3 * 64};
    return e[b];
}

// Split-K plan for a single-phase GEMM of M rows x Co columns x kpad on k_conv.
//  bf16: double the split while the grid stays <= ~1024 workgroups and every split keeps >= 16 k-slabs.
//  fp32 (AVSE_F32, and the generic layers of AVSE_F32_SPLIT): block-exact, as the training step's train_split —
//  every split is exactly one block of k_conv's blocked fp32 summation (kFp32Block 16-product slabs) and
//  k_splitk_reduce_tiles adds the splits in order, so each sum is the unsplit kernel's bit for bit.  Whether a launch
//  splits (short grids only) then changes no result: the fp32 forward of a clip is the same whatever batch it runs
//  in (the batched CLI predict reproduces the per-sample one exactly; tests/test_gpu_split.py).
//  AVSE_F32_SPLIT dense layers (one tap): groups of G blocks per split, G and the split count from K and Cout only
//  (never from M), so every batch size takes the same splits and the same ordered reduction — batch-invariant as
//  above, with G x fewer fp32 partials (enc_dense: 41 one-block splits moved 236 MB of partials per launch at B = 512;
//  11 four-block splits move 64 MB).  slabs_per_split (k_conv's ConvArgs::ksplit_slabs) = 8 G.
constexpr int64_t kSplitTileCap = 2048;   // fp32 tiles x splits per launch (128 x 128-float partials each)
inline int choose_ksplit(int64_t M, int Co, int kpad, int dtype, bool dense = false, int* slabs_per_split = nullptr) {
    const int BN = Co <= 64 ? 64 : 128;
    const int64_t tiles = ((M + 127) / 128) * ((Co + BN - 1) / BN);
    if (slabs_per_split) *slabs_per_split = 0;
    if (dtype == AVSE_F32_SPLIT && dense) {
        const int nblocks = (kpad / 16 + kFp32Block - 1) / kFp32Block, tiles_n = (Co + 127) / 128;
        const int G = std::max(1, (nblocks * tiles_n + 127) / 128);
        const int ks = (nblocks + G - 1) / G;
        if (ks < 2) return 1;
        if (slabs_per_split) *slabs_per_split = G * kFp32Block;
        return ks;
    }
    if (dtype != AVSE_BF16) {
        const int nslab = kpad / 16;
        const int ks = (nslab + kFp32Block - 1) / kFp32Block;
        if (tiles >= 256 || ks < 2 || (nslab + ks - 1) / ks != kFp32Block || tiles * ks > kSplitTileCap) return 1;
        return ks;
    }
    const int nslab = kpad / 32;
    int ks = 1;
    while (tiles * ks * 2 <= 1024 && nslab / (ks * 2) >= 16) ks *= 2;
    return ks;
}

// k_gemm (bf16) split-K factor: as many workgroups as fit one round on the 256 CUs (one 128-KB workgroup per CU: 264
// workgroups took two rounds), at least 8 slabs each
inline int gemm_ksplit(int M, int N, int kpad, int cap) {
    const int tiles = ((M + 127) / 128) * ((N + 127) / 128), nslab = kpad / 32;
    int ks = 256 / tiles;
    ks = ks > nslab / 8 ? nslab / 8 : ks;
    if (cap > 0 && cap < ks) ks = cap;   // A/B: cap the split (timing experiments, ksplit == 1 parity test)
    return ks < 1 ? 1 : ks;
}

// k_gemm's partials: [tiles][ksplit][128 x 128] fp32
inline size_t gemm_partial_bytes(int64_t M, int N, int ks) {
    return ks > 1 ? (size_t)((M + 127) / 128) * ((N + 127) / 128) * ks * 128 * 128 * 4 : 0;
}
inline size_t gemm_ws_bytes(int M, int N, int kpad, int cap) { return gemm_partial_bytes(M, N, gemm_ksplit(M, N, kpad, cap)); }

// AVSE_F32_SPLIT dense layers on k_gemm: splits of whole kFp32Block-slab blocks, the plan from K and N only (never M,
// so every batch takes the same splits and the same ordered reduction): as many splits as fill the 256 CUs at the
// bench batch's 4 row tiles
inline int gemm_s16_ksplit(int N, int kpad, int* slabs_per_split) {
    const int nblocks = (kpad / 16 + kFp32Block - 1) / kFp32Block, tiles_n = (N + 127) / 128;
    int ks = std::max(1, std::min(nblocks, 256 / (4 * tiles_n)));
    const int G = (nblocks + ks - 1) / ks;
    ks = (nblocks + G - 1) / G;
    if (slabs_per_split) *slabs_per_split = G * kFp32Block;
    return ks;
}

// One launch's split: factor, slabs per split (0: the kernel divides them evenly) and the partial sums it writes
struct KSplit {
    int ksplit = 1, slabs = 0;
    size_t bytes = 0;
};
// v_conv6 (rows: its 4 x 4 grid) or a dense layer (one tap) as the GEMM it is, kpad the packed reduction length
struct SplitLayer {
    int rows = 1, Co = 0, kpad = 0;
    bool dense = false;
};
struct SplitPlan {
    KSplit gemm;   // on k_gemm; ksplit 0: the dtype (AVSE_F32) has no k_gemm
    KSplit conv;   // on k_conv + k_splitk_reduce_tiles: Options::no_gemm, AVSE_F32, or a launch k_gemm declines
};

// The single source of both kernels' split of layer `l` at `clips` clips.
inline SplitPlan split_plan(const SplitLayer& l, int64_t clips, int dtype, const Options& o) {
    const int64_t M = clips * l.rows;
    SplitPlan p;
    p.gemm.ksplit = 0;
    p.conv.ksplit = choose_ksplit(M, l.Co, l.kpad, dtype, l.dense, &p.conv.slabs);
    // k_conv's partials cover whole 128 x BN tiles (MFMA-native order)
    const int bn = l.Co <= 64 ? 64 : 128;
    const size_t mp = (size_t)((M + 127) / 128) * 128, np = (size_t)((l.Co + bn - 1) / bn) * bn;
    if (p.conv.ksplit > 1) p.conv.bytes = (size_t)p.conv.ksplit * mp * np * 4;
    if (dtype == AVSE_BF16) {
        p.gemm.ksplit = gemm_ksplit((int)M, l.Co, l.kpad, o.gemm_ksplit_cap);
    } else if (dtype == AVSE_F32_SPLIT && l.dense) {
        p.gemm.ksplit = gemm_s16_ksplit(l.Co, l.kpad, &p.gemm.slabs);
    } else if (dtype == AVSE_F32_SPLIT) {   // v_conv6: k_conv's plan, one block per split or none
        p.gemm.ksplit = choose_ksplit(M, l.Co, l.kpad, dtype);
        p.gemm.slabs = p.gemm.ksplit > 1 ? kFp32Block : 0;
    }
    p.gemm.bytes = gemm_partial_bytes(M, l.Co, p.gemm.ksplit);
    return p;
}

// What the arena layout depends on besides batch, dtype and Options: the network shape and its split-K layers (v_conv6,
// enc_dense, dec_dense1, dec_dense2) with layer_geom's geometry, which is what pack_layer stores and the launches read.
constexpr int kSplitFirst = 10, kSplitLayers = 4;
struct ArenaShape {
    NetPlan plan;
    SplitLayer split[kSplitLayers];
};
inline ArenaShape arena_shape(const NetPlan& p) {
    ArenaShape a;
    a.plan = p;
    for (int i = 0; i < kSplitLayers; ++i) {
        const LayerGeom g = layer_geom(p.L[kSplitFirst + i]);
        a.split[i] = SplitLayer{g.hq * g.wq, p.L[kSplitFirst + i].cout, g.ph[0].kpad, g.ph[0].ntaps == 1};
    }
    return a;
}

// fp32 partial-sum workspace of the split-K layers at batch N: the most either kernel would write
inline size_t split_ws_bytes(int64_t N, int dtype, const Options& o, const ArenaShape& a) {
    size_t mx = 0;
    for (const SplitLayer& l : a.split) {
        const SplitPlan p = split_plan(l, N, dtype, o);
        mx = std::max({mx, p.conv.bytes, p.gemm.bytes});
    }
    return mx;
}

// Arena size for `clips` clips; offs (nullable) gets the B_COUNT buffer offsets and, at [B_COUNT], the workspace's.
inline size_t arena_bytes(int64_t clips, int dtype, const Options& o, size_t* offs, const ArenaShape& a) {
    const size_t es = dtype == AVSE_BF16 ? 2 : 4;
    size_t off = 0;
    for (int b = 0; b < B_COUNT; ++b) {
        if (offs) offs[b] = off;
        off += (buf_elems(a.plan, b) * es * (size_t)clips + 255) & ~(size_t)255;
    }
    if (offs) offs[B_COUNT] = off;   // split-K partials
    off += (split_ws_bytes(clips, dtype, o, a) + 255) & ~(size_t)255;
    return off;
}

}  // namespace avse
