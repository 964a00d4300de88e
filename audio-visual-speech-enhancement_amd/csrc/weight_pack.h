// Host-only weight folding and packing (no HIP header): from one layer's Keras kernel / bias / BatchNormalization
// parameters to every buffer the inference kernels read.  weights.hip uploads the result (build_layer).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/avse.h"
#include "layer_geom.h"
#include "options.h"

namespace avse {

uint16_t f2h(float f);    // f32 -> f16 bits, round to nearest even
float h2f(uint16_t u);
uint16_t f2bf(float f);   // f32 -> bf16 bits, round to nearest even

// AVSE_F32_SPLIT operand: hi = f16(v), lo = f16(v - hi)
struct SplitPair {
    uint16_t hi, lo;
};
SplitPair split_pair(float v);

// Per-channel power of two e with max|w| 2^e in [2^14, 2^15) (0 for an all-zero channel): hi = f16(w 2^e) stays below
// 2^15 and lo keeps full precision for every weight above 2^-10 of the channel's largest.
std::vector<int> channel_exponents(const std::vector<float>& max_abs);

// bias + BatchNormalization (moving statistics) as y = acc * scale + shift per output channel
void fold_bn(const LayerDef& L, const float* bias, const float* bn, std::vector<float>& scale, std::vector<float>& shift);

// AVSE_F32_SPLIT per-layer activation exponents from the canonical blob, and the exponent layer i reads
void act_exponents(const NetPlan& P, const float* blob, int* e);
int act_exp_in(const int* e, int i);

struct PackedLayer {
    LayerGeom geom;                 // geom.taps: the (dy, dx) table
    // generic k_conv weights [phase][Cout][kpad] (gather_map): f32 in w32, else 16-bit in w16 (bf16; split: each 16-k
    // slab row [Bh(16) | Bl(16)] f16, output channel n scaled by 2^e_n, which scale takes back)
    std::vector<float> w32;
    std::vector<uint16_t> w16;
    std::vector<float> scale, shift;
    int halo = HALO_NONE;           // tiled video conv variant; the three below only when it is one
    std::vector<uint16_t> w_halo;   // conv_stream.hip [slice][Cout][32] / conv_v1r.hip [kernel row][Cout][32] (pack_halo)
    std::vector<float> scale_h;     // |scale| for w_halo: channels with a negative BN scale have negated weights
    std::vector<uint16_t> w_dense;  // a_conv1 only (bf16): [Cout][32], k = ky * kw + kx, for conv_aud.hip
    std::vector<float> w_f32;       // a_conv1 only (split): [kh * kw][Cout] f32 x 2^e_n, for conv.hip k_aconv1_split
};

// e_in / e_out: the activation exponents the layer reads / stores (split dtype; else 0).  Reads Options::no_halo and
// Options::no_v1p.  geom.status != GEOM_OK: nothing else is filled.
PackedLayer pack_layer(const LayerDef& L, const float* kernel, const float* bias, const float* bn, int dtype,
                       const Options& opt, int e_in, int e_out);

}  // namespace avse
