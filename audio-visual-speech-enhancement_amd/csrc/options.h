// Host-only (no HIP header): the kernel-path switches of a context and the tiled video convolutions' variants, read
// by the launch code (avse_common.h) and by the host-only weight packer (weight_pack.h).
#pragma once

namespace avse {

// Kernel-path switches of one context.  Defaults are the production path; every field exists for an A/B
// experiment or a layer-by-layer parity test.  Initialised once from the AVSE_* environment at
// avse_ctx_create, changed with avse_ctx_set_option; launch code never reads the environment.
struct Options {
    int no_gemm = 0;          // AVSE_NO_GEMM: v_conv6 + dense layers on k_conv + split-K reduce (not k_gemm)
    int no_audenc = 0;        // AVSE_NO_AUDENC: audio encoder layer by layer (not k_aud_enc)
    int no_dechead = 0;       // AVSE_NO_DECHEAD: d_deconv1..3 layer by layer (not k_dec_head)
    int no_dectail = 0;       // AVSE_NO_DECTAIL: d_deconv4..6 layer by layer (not k_dec_tail)
    int unfused_tail = 0;     // AVSE_UNFUSED_TAIL: d_deconv6 as its own kernel (d_deconv5 activation materialised)
    int no_halo = 0;          // AVSE_NO_HALO: video convs on k_conv (read when weights are loaded)
    int mfma32 = 0;           // AVSE_MFMA32: 32x32x16 compute waves in the stream convolutions
    int serial = 0;           // AVSE_SERIAL: one stream for the whole forward
    int graph = 0;            // AVSE_GRAPH: avse_forward replays a hipGraph per argument set
    int gemm_ksplit_cap = 0;  // AVSE_GEMM_KSPLIT: cap k_gemm's split-K factor (0 = no cap)
    int dense_istft = 0;      // AVSE_DENSE_ISTFT: ISTFT through the dense pinv + scratch frames + k_ola (not fused)
    int no_act_scale = 0;     // AVSE_NO_ACT_SCALE: split weights loaded without per-layer activation exponents
    int no_win = 0;           // AVSE_NO_WIN: split stride-1 gather layers on k_conv, not the windowed conv_win.hip
    int no_v1p = 0;           // AVSE_NO_V1P: split 5-frame v_conv1 on k_conv_v1s (K 160), not k_conv_v1p (K 128; read at load)
    int no_a1valu = 0;        // AVSE_NO_A1VALU: split a_conv1 on k_conv after audio_prep, not k_aconv1_split
    int no_planar = 0;        // AVSE_NO_PLANAR: split stream convs on the slice-by-slice [Ah | Al] grouping with lane swaps
    int four_products = 0;    // AVSE_FOUR_PRODUCTS: split k_gemm and decoder tail slab by slab with all four products, not three-product planar slab pairs
    int side_prio = 0;       // AVSE_SIDE_PRIO: audio side stream priority (0 default, 1 least, 2 greatest; read when created)
};

// ---- tiled video convolutions: conv_v1r.hip (v_conv1), conv_stream.hip (v_conv2..v_conv5) ----
enum HaloVariant { HALO_NONE = -1, HALO_V1 = 0, HALO_K5 = 1, HALO_K3_16 = 2, HALO_K3_8 = 3, HALO_V1P = 4 };

}  // namespace avse
