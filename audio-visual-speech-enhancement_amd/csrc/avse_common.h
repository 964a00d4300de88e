// Shared device/host helpers for libavse (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "forward_plan.h"
#include "ragged_geom.h"

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct avse_ctx;

namespace avse {

void set_error(const std::string& msg);

// device index of a context (capi.hip; the training step, train.hip, allocates on the same device)
int ctx_device_index(const struct ::avse_ctx* c);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for `fn` on the CURRENT device, once per (kernel, device)
// (thread-safe; capi.hip).  Every launcher that needs more than 64 KB of dynamic LDS calls it first.
int ensure_lds_attr(const void* fn, int bytes);

#define AVSE_HIP_CHECK(expr)                                                                   \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            ::avse::set_error(std::string(#expr " failed: ") + hipGetErrorString(_e));         \
            return 2; /* AVSE_ERR_HIP */                                                       \
        }                                                                                      \
    } while (0)

// ---- checked build (make DEBUG=1 -> libavse_debug.so, -DAVSE_DEBUG) -----------------------
// Device-side protocol / bounds checks that a release build compiles out.  A failing check records the first hit
// (kernel, check code, block, thread, observed and expected value) in its translation unit's record with one vector
// compare-and-swap and the kernel carries on (no trap: a trapped wave can take the whole GPU down); the C-ABI entry
// points synchronise their stream after launching and turn a hit into AVSE_ERR_CHECK with the record in
// avse_last_error (debug_poll, capi.hip).
struct DebugHit {
    unsigned hit, kernel, code, block, thread;
    int value, expect;
};
enum DebugKernel : unsigned {
    DK_V1R = 1,      // k_conv_v1r: window-slot tags (the loader's window k in slot k % 3 when the compute waves read)
    DK_SPEC = 3,     // k_spec_seg / k_spec640: output and LDS index bounds
    DK_ISTFT = 4,    // k_istft_fused: frame range and output bounds
};
#ifdef AVSE_DEBUG
inline constexpr bool kDebugBuild = true;
__device__ __forceinline__ void debug_record(DebugHit* h, unsigned kern, unsigned code, int value, int expect) {
    if (atomicCAS(&h->hit, 0u, 1u) == 0u) {
        h->kernel = kern;
        h->code = code;
        h->block = blockIdx.x;
        h->thread = threadIdx.x;
        h->value = value;
        h->expect = expect;
        __threadfence();
    }
}
// one record per translation unit (no relocatable device code): AVSE_DEBUG_RECORD(name) defines it and the host
// reader `int name(DebugHit* out)` (copy + reset) that debug_poll calls
#define AVSE_DEBUG_RECORD(reader)                                                                    \
    static __device__ ::avse::DebugHit g_avse_dbg;                                                   \
    int reader(::avse::DebugHit* out) {                                                              \
        ::avse::DebugHit zero{};                                                                     \
        if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_avse_dbg), sizeof(zero)) != hipSuccess) return 2;   \
        return hipMemcpyToSymbol(HIP_SYMBOL(g_avse_dbg), &zero, sizeof(zero)) == hipSuccess ? 0 : 2; \
    }
#define AVSE_CHECK_DEV(cond, kern, code, value, expect)                                              \
    do {                                                                                             \
        if (!(cond)) ::avse::debug_record(&g_avse_dbg, (kern), (code), (int)(value), (int)(expect)); \
    } while (0)
#else
inline constexpr bool kDebugBuild = false;
#define AVSE_DEBUG_RECORD(reader)              \
    int reader(::avse::DebugHit* out) {          \
        *out = ::avse::DebugHit{};               \
        return 0;                                \
    }
#define AVSE_CHECK_DEV(cond, kern, code, value, expect) \
    do {                                                 \
    } while (0)
#endif
int debug_read_v1r(DebugHit* out);
int debug_read_stft(DebugHit* out);
int debug_read_istft(DebugHit* out);

// ---- STFT / mel front end ---------------------------------------------------------------
struct SpecArgs {
    const float* sig;
    int64_t n_utt;
    int64_t n_samples;
    int n_fft, hop, n_frames;
    int n_mels;
    float amin, top_db;
    float db_floor;           // 20*log10(amin) evaluated in double (bins <= amin)
    int pad_mode;
    int spf, n_slices;        // frames_per_slice (0 = plain [n_mels][T] layout)
    float* mel_db;
    float* stft_ri;           // nullable
    const float2* twiddle;    // [n_fft]  e^{-2 pi i k / n_fft}
    const float* window;      // [n_fft]  periodic Hann
    const int* mel_start;
    const int* mel_width;
    const float* mel_weight;
    int mel_max_width;
    int mel_seg_nq[4];        // MelTable::seg_nq
    int mel_seg_nq4[4];       // MelTable::seg_nq4
    unsigned int* umax;       // [n_utt] ordered-float max scratch (chunked mode)
};

int launch_spectrogram(const SpecArgs& a, hipStream_t s);

// Ragged batches (ragged_geom.h): the device copies of a RaggedGeom's rows, in the context's preprocess scratch.
struct RaggedDev {
    const RaggedUtt* utt;      // [n_utt]
    const RaggedItem* items;   // [n_items]
    int n_utt, n_items;
};
// frames per block of the kernel a ragged STFT of this shape runs in (k_spec640 / k_spec533); 0: no ragged kernel,
// the launcher walks the batch's equal-length runs through launch_spectrogram
int spectrogram_ragged_chunk(int n_fft, int hop, int n_mels, int mel_max_width);
// a.sig / a.mel_db / a.stft_ri are the packed buffers' bases, a.n_utt the batch; a.n_samples / n_frames / n_slices are
// ignored (per utterance in g).  One run: launch_spectrogram itself.  d may be empty where no ragged kernel runs.
int launch_spectrogram_ragged(const SpecArgs& a, const RaggedGeom& g, const RaggedDev& d, hipStream_t s);

struct IstftArgs {
    const float* mel_db;      // spf > 0: [n_utt][n_slices][n_mels][spf], else [n_utt][n_mels][T]
    int spf, n_slices;
    const float2* stft;       // mixture STFT [n_utt][nb][stft_frames] (phase source)
    int stft_frames;
    int64_t n_utt;
    int T;                    // frames reconstructed
    int nb;                   // bins = 1 + n_fft_analysis / 2
    int N;                    // inverse size = 2 (nb - 1)
    int hop;
    int n_mels;
    const float* pinvT;       // [n_mels][nb] pinv(mel)^T
    const float2* twiddle;    // [N] e^{-2 pi i k / N}
    const float* window;      // [N] periodic Hann
    float* frames;            // scratch [n_utt][T][N] (unfused path only)
    float* sig;               // [n_utt][hop (T - 1)]
    // fused n_fft 640 / hop 160 path: pinv(M) y = M^T (M M^T)^{-1} y with M M^T tridiagonal (adjacent Slaney
    // triangles overlap, nothing else does), so the 321 x 80 dense pinv becomes an 80 x 80 solve + a 2-tap expansion
    const float4* bins;       // [nb] (M[j0][k], M[j0+1][k], j0 as int bits, 0): the <= 2 filters covering bin k
    const float* gram_inv;    // [80][80] (M M^T)^{-1} (symmetric; the fused kernel's MFMA solve), null = Thomas
};

int launch_istft(const IstftArgs& a, hipStream_t s);

// output hops per block of k_istft_fused where it serves the shape (inverse size 640 / hop 160 / 80 bands, the
// tridiagonal tables present); 0: no ragged kernel, the launcher walks the runs through launch_istft
int istft_ragged_chunk(int N, int hop, int n_mels, bool fused_tables);
// the ragged twin (a.T / stft_frames / n_slices ignored): one run is launch_istft itself
int launch_istft_ragged(const IstftArgs& a, const RaggedGeom& g, const RaggedDev& d, hipStream_t s);

// ---- implicit-GEMM convolution ----------------------------------------------------------
struct ConvArgs {
    const void* in;      // T [N][Hi][Wi][Ci] (clip stride in_clip_stride)
    void* out;           // T
    const void* w;       // T packed
    const float* scale;  // [Cout]  folded BN scale (or 1)
    const float* shift;  // [Cout]  folded bias/BN shift
    const int2* taps;    // device (dy, dx) per tap, all phases
    int N;
    int Hi, Wi, Ci;
    long long in_clip_stride;
    int Hq, Wq;          // per-phase conv output grid
    int sy, sx;          // input step per grid step
    int oys, oxs;        // output step per grid step (deconv stride)
    int Ho, Wo, Co;      // output tensor (after pool)
    long long out_clip_stride;
    int out_pix_stride;
    int out_c_off;
    int pool;            // fused 2x2 max pool
    int act;             // 1 = LeakyReLU(0.3)
    int nphase;
    int ksplit;          // >1: split-K over blockIdx.z, fp32 partials + k_splitk_reduce (nphase == 1)
    int ksplit_slabs;    // > 0: K slabs (16-k units) per split, else ceil(slabs / ksplit)
    float* partial;      // [ksplit][M][Co] workspace
    // fused trailing 1x1 Cout -> 1 layer (d_deconv6, network.py:133): out_f[pixel] = bias + sum_c w[c] * y[c],
    // y = this layer's output rounded to T; the T output is not stored (Co == 64, ksplit == 1, no pool)
    const float* fuse_w;
    float fuse_bias;
    float* fuse_out;
    int out_s16;         // 1: the output in the split pair layout (strides and offset in halves), else T / fp32
    // AVSE_F32_SPLIT range guard (mfma_util.h pair_out_of_range): a stored pair value, or an fp32 input value split
    // on load, outside the f16 range ORs range_bit / range_in_bit into *range_flag (nullable)
    unsigned* range_flag;
    unsigned range_bit, range_in_bit;
    ConvPhase ph[MAX_PHASES];
};

// AVSE_F32_SPLIT range guard (mfma_util.h pair_out_of_range / range_report), the bits of its flag word: bit i = layer i
// of the plan (a_conv1 = 0 .. d_deconv5 = 18), the split network inputs below
constexpr unsigned kRangeAudioIn = 1u << 24, kRangeVideoIn = 1u << 25;
int launch_flag_or(unsigned* flag, unsigned bits, hipStream_t s);

// launch_conv dtype: 0 fp32 (exact-fp32 MFMA), 1 bf16, kConvSplit fp32 input with split-f16 products (the generic
// layers of AVSE_F32_SPLIT: weights packed [Cout][kpad] with each 16-k slab row [Bh(16) | Bl(16)] f16),
// kConvSplitPairs the same on an input already in the split pair layout (Ci, strides, kpad, w_off in halves)
constexpr int kConvSplit = 2, kConvSplitPairs = 3;
int launch_conv(const ConvArgs& a, int dtype, hipStream_t s);

// conv_win.hip: the split-pair layers whose every phase is a stride-1 gather over the input grid (the decoder's
// transposed convolutions, the stride-1 audio conv): k_conv's arithmetic with the A operand read from a per-tile input
// window staged once per 16-channel chunk in LDS (k_conv gathers every tap's im2col rows from global memory).
// htaps: host copy of a.taps.  Returns 0 when launched, -1 when the layer does not fit the kernel (the caller runs
// launch_conv), else an error status.
int launch_conv_win(const ConvArgs& a, const int2* htaps, hipStream_t s);

// fused decoder tail d_deconv4 -> d_deconv5 -> d_deconv6, one workgroup per clip (conv_dec.hip, bf16)
struct DecTailArgs {
    const bf16_t* in;        // d_deconv3 output [N][40][10][128]
    float* out;              // [N][80][20]
    int N;
    const bf16_t* w4;        // d_deconv4 packed [64][kpad4], k = tap * 128 + c
    const float* sc4;        // folded bias + BN
    const float* sh4;
    int nt4, kpad4;
    int pt4, pl4, rows4, pitch4;   // zero-padded input window: top / left pad, rows, pitch (pixels)
    int dy4, dx4, nx4;       // taps: t -> (dy4 - t / nx4, dx4 - t % nx4) (checked on the host)
    const bf16_t* w5;        // d_deconv5 packed, phase p at element w5 + woff5[p]: [64][kpad5[p]], k = tap * 64 + c
    const float* sc5;
    const float* sh5;
    int nt5[4], kpad5[4];
    int dy5[4], dx5[4], nx5[4];    // phase p's taps: t -> (dy5 - t / nx5, dx5 - t % nx5)
    long long woff5[4];
    int pt5, pl5, rows5, pitch5;   // zero-padded d_deconv4 output image
    const float* w6;         // d_deconv6 1x1 weights [64] + bias
    float b6;
    // split-f16 tail (conv_dects.hip, AVSE_F32_SPLIT): in = d_deconv3's split pairs [N][40][10][8 x (h(16) | l(16))],
    // w4 / w5 the layers' split packings ([Cout][2 kpad] halves, each 16-k slab row [Wh(16) | Wl(16)]); d_deconv4's
    // stored pairs report into the range guard
    unsigned* range_flag;
    unsigned range_bit;
    int four_products;       // split tail: 1 = slab by slab with all four products (Options::four_products), 0 = planar
                             // slab pairs with three
};
bool dec_tail_supported(const DecTailArgs& a);
bool dec_tail_s16_supported(const DecTailArgs& a);
int launch_dec_tail_s16(const DecTailArgs& a, hipStream_t s);

// fused audio encoder a_conv1 -> a_conv5, one workgroup per clip (conv_aud.hip, bf16)
struct AudEncArgs {
    const float* mel;        // [N][80][20] network input
    bf16_t* out;             // concat buffer: a_conv5's HWC flatten at [clip * out_clip_stride, + 3200)
    long long out_clip_stride;
    int N;
    const bf16_t* w1;        // a_conv1 dense [64][32], k = ky * 5 + kx (25 real)
    const bf16_t* w2;        // a_conv2 packed [64][1024], k = tap * 64 + c
    const bf16_t* w3;        // a_conv3 packed [128][1024]
    const bf16_t* w4;        // a_conv4 packed [128][512], k = tap * 128 + c
    const bf16_t* w5;        // a_conv5 packed [128][512]
    const float* sc[5];      // folded bias + BN per layer
    const float* sh[5];
};
bool aud_enc_supported(const AudEncArgs& a);

// fused decoder head d_deconv1 -> d_deconv3, one workgroup per clip (conv_dech.hip, bf16)
struct DecHeadArgs {
    const bf16_t* in;        // dec_dense2 output [N][3200] (= [5][5][128])
    long long in_clip_stride;
    bf16_t* out;             // d_deconv3 output [N][40][10][128]
    long long out_clip_stride;
    int N;
    const bf16_t* w1;        // packed per phase [phase][128][kpad], k = tap * 128 + c (kpad 256, 256, 512)
    const bf16_t* w2;
    const bf16_t* w3;
    const float* sc[3];
    const float* sh[3];
};
bool dec_head_supported(const DecHeadArgs& a);
int launch_dec_head(const DecHeadArgs& a, hipStream_t s);

// batched-clip GEMM (gemm.hip, bf16): mode 0 dense rows, mode 1 v_conv6 (3x3 'same' on 4 x 4 x 512 + 2x2 pool)
struct GemmArgs {
    const bf16_t* a;         // mode 0: [M][lda]; mode 1: input [M / 16][4][4][512], clip stride lda
    long long lda;
    const bf16_t* w;         // [N][kpad] (k = tap * 512 + c in mode 1)
    int M, N, kpad;
    const float* scale;      // folded bias + BN
    const float* shift;
    int act;
    bf16_t* out;             // mode 0: out[m * ldo + out_off + n]; mode 1: out[clip * ldo + out_off + q * N + n]
    long long ldo;
    int out_off;
    int ksplit;              // split-K over blockIdx.z, reduced by the last workgroup of each tile
    float* partial;          // [tiles][ksplit][128 x 128] fp32
    int* counters;           // [tiles], zero between launches
    int split;              // 1 = AVSE_F32_SPLIT (k_gemm S16): a / out in the split-pair layout (lda, ldo, out_off in
                             // halves), w packed [Wh(16) | Wl(16)] per 16 k, kpad in k
    int slabs_per_split;     // split: slabs per split (whole kFp32Block blocks; 0 = one split)
    unsigned* range_flag;    // split: range guard of the stored pairs
    unsigned range_bit;
    int counters_cap;        // ints in counters (layer_geom.h gemm_tickets_fit: launch_gemm returns -1 when a split
                             // launch has more tiles, and the caller runs the layer on k_conv)
    int four_products;       // split: 1 = slab by slab with all four products (Options::four_products), 0 = planar slab
                             // pairs with three
};
// (the split-K plans, gemm_ksplit and gemm_s16_ksplit among them: forward_plan.h)
int launch_gemm(const GemmArgs& g, int mode, hipStream_t s);   // 0 launched, -1 declined (counters_cap), else an error
int launch_aud_enc(const AudEncArgs& a, hipStream_t s);
int launch_dec_tail(const DecTailArgs& a, hipStream_t s);

// ---- tiled bf16 video convolutions: conv_v1r.hip (v_conv1), conv_stream.hip (v_conv2..v_conv5) ----
// output element format of the tiled video convolutions: bf16; split f16 pairs (per pixel and 16 channels,
// [h(16) | l(16)] with h = f16(x), l = f16(x - h): the next split layer's input); f32
enum HaloOut { OUT_BF16 = 0, OUT_S16 = 1, OUT_F32 = 2 };

struct HaloArgs {
    int variant;
    const void* in;          // bf16 [N][Hc][Wc][Ci]            (not V1)
    const float* video;      // f32  [N][Hc][Wc][5] raw video   (V1)
    const float* vmean;      // nullable [Hc][Wc]               (V1)
    const float* vstd;
    void* out;               // bf16, pooled [N][Hc/2][Wc/2][Co] at (clip stride, pixel stride, channel offset)
    const void* w;           // bf16 [step][Co][32] (V1: [5 kernel rows][Co][32], conv_v1r.hip)
    const float* scale;
    const float* shift;
    int N, Hc, Wc, Ci, Co;
    long long out_clip_stride;
    int out_pix_stride;
    int out_c_off;
    int mfma32;              // conv_stream.hip: 1 = v_mfma_f32_32x32x16_bf16 compute waves (A/B variant)
    int no_planar;           // conv_stream.hip, split: 1 = the [Ah | Al] x Bh grouping with v_permlane32_swap (A/B variant)
    int split;               // 1 = split-f16 operands (AVSE_F32_SPLIT): in is the split-pair layout, Ci counts halves
                             // (2 x channels), w holds [Bh | Bl] rows; out_mode OUT_S16 or OUT_F32
    int out_mode;            // HaloOut
    unsigned long long* prof;   // ablation harness only (ABL & 128): per-wave cycle counters, else unused
    unsigned* range_flag;    // split: range guard (ConvArgs::range_flag), nullable
    unsigned range_bit, range_in_bit;   // OUT_S16 stores / v_conv1's split of the (normalised) video input
    int video_u8;            // V1: `video` points at uint8 [N][Hc][Wc][Ci] (AVSE_VIDEO_U8), not f32
};

int launch_conv_stream(const HaloArgs& a, hipStream_t s);   // conv_stream.hip (non-V1 variants)
int launch_conv_v1r(const HaloArgs& a, hipStream_t s);      // conv_v1r.hip (v_conv1, kernel-row runs)
// video_u8: `video` is uint8 (AVSE_VIDEO_U8); converted exactly, then the float path's arithmetic
int launch_video_prep(const void* video, int video_u8, const float* mean, const float* stdv, void* out, int64_t N,
                      int F, int dtype, hipStream_t s);
int launch_audio_prep(const float* audio, void* out, int64_t npix, int dtype, hipStream_t s);
// split dtype a_conv1 (one input channel) on the vector ALUs straight from the audio input (conv.hip k_aconv1_split)
int launch_aconv1_split(const float* in, const float* w, const float* scale, const float* shift, void* out, int64_t N,
                        int H, int W, int Ho, int Wo, int KH, int KW, int S, int pt, int pl, int Co, unsigned* range_flag,
                        unsigned range_bit, unsigned range_in_bit, hipStream_t s);
int launch_out_conv(const void* in, const float* w64, float bias, float* out, int64_t npix, int dtype,
                    hipStream_t s);
int launch_broadcast_row(const void* src, void* dst, int64_t rows, int64_t row_bytes, int64_t stride_bytes,
                         hipStream_t s);
// dst row r = src row row_of[r] (device, [rows]), or `fill` where row_of[r] < 0 (conv.hip k_gather_rows)
int launch_gather_rows(const void* src, const void* fill, const int* row_of, void* dst, int64_t rows, int64_t row_bytes,
                       int64_t src_stride_bytes, int64_t dst_stride_bytes, hipStream_t s);
int launch_video_normalize(float* video, int64_t S, int H, int W, int F, const float* mean,
                           const float* stdv, hipStream_t s);
int launch_mse(const float* a, const float* b, int64_t n, float* loss, float* partial, hipStream_t s);

// ---- device-side preprocess (prep.hip) ---------------------------------------------------
// avse_mix_pairs: exact integer powers (64-bit integer atomics into `scratch`), the float64 gain of
// AudioMixer.snr_factor, then the mixture / speech / scaled-noise rows.  scratch: mix_pairs_scratch_bytes(U) bytes.
size_t mix_pairs_scratch_bytes(int64_t n_pairs);
int launch_mix_pairs(const int16_t* speech, const int64_t* speech_off, const int16_t* noise, const int64_t* noise_off,
                     const double* snr_lin, int64_t n_pairs, int64_t L, float* rows, double* mix64, double* factor,
                     void* scratch, hipStream_t s);
// avse_video_stats: per-pixel float64 moments about the pixel's first value, partials per chunk of slices in
// `scratch` (video_stats_scratch_bytes), combined in chunk order.  F <= kVideoStatsMaxF.
constexpr int kVideoStatsMaxF = 8;
size_t video_stats_scratch_bytes(int64_t S, int H, int W);
int launch_video_stats(const float* video, int64_t S, int H, int W, int F, float* mean, float* stdv, void* scratch,
                       hipStream_t s);
// uint8 video: exact 64-bit integer sums of x and x^2 per pixel and chunk (the same scratch size), combined in chunk
// order; mean and std are each rounded once to float32 from the exact integer moments
int launch_video_stats_u8(const uint8_t* video, int64_t S, int H, int W, int F, float* mean, float* stdv, void* scratch,
                          hipStream_t s);

// ---- evaluate stage (eval.hip) ------------------------------------------------------------
// avse_eval_pairs / avse_eval_pairs_ext: the device copies of the host tables (eval_tables.cpp) and the call's geometry, passed by value.
struct EvalDev {
    const double* taps;    // [2 H + 1] resampling filter for (up, down)
    const double* W;       // [256] STOI's frame window
    const double* twid;    // [256] (re, im): e^{-2 pi i k / 512}
    const double* segw;    // [win] the segmental SNR's window
    const int* bands;      // [15] (lo, hi) bin ranges
    int up, down, H;
    int win, skip;         // segmental-SNR frame and hop
    int stoi;              // 0: max(up, down) > 24 without AVSE_EVAL_ANY_RATE, slots 3 and 4 are NaN and 0 (5: NaN)
    int64_t cap;           // upper bound on off[n_pairs] - off[0] the scratch was sized for
    // avse_eval_pairs_ext
    const double* ptaps;   // [up][2 H / up + 1] the filter by phase (eval_tables.h resample_taps_by_phase); NULL when
                           // max(up, down) <= 24: k_eval_resample runs, from `taps`
    int ms;                // slots per metrics row: 5, or 6 with ESTOI in slot 5
};
size_t eval_pairs_scratch_bytes(int64_t n_pairs, const EvalDev& t);
int launch_eval_pairs(const float* ref, const float* deg, const int64_t* off, int64_t n_pairs, const EvalDev& t,
                      double* metrics, void* scratch, hipStream_t s);

}  // namespace avse
