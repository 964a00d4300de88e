// Private to the C-ABI's translation units (capi.hip: contexts, tables, audio / prep / eval entry points; weights.hip:
// avse_weights; forward.hip: the forward): the context, the weights object and the device buffers they own.
#pragma once
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/avse.h"
#include "avse_common.h"

namespace avse {

int fail(int code, const std::string& msg);   // sets avse_last_error's text and returns code (capi.hip)
// checked build: wait for the stream, then report the first device-side check that fired (capi.hip)
int debug_poll(void* stream);
inline bool valid_dtype(int dtype) { return dtype == AVSE_F32 || dtype == AVSE_BF16 || dtype == AVSE_F32_SPLIT; }

// One device (Host: pinned host) allocation, freed with its owner.  Move-only; converts to the pointer.
template <typename T, bool Host = false>
struct Owned {
    struct Free {
        void operator()(T* q) const { (void)(Host ? hipHostFree(q) : hipFree(q)); }
    };
    std::unique_ptr<T, Free> p;
    size_t bytes = 0;
    hipError_t alloc(size_t n) {   // the old allocation goes first; nothing is held when this fails
        p.reset();
        bytes = 0;
        T* q = nullptr;
        const hipError_t e = Host ? hipHostMalloc((void**)&q, n, hipHostMallocDefault) : hipMalloc((void**)&q, n);
        if (e == hipSuccess) { p.reset(q); bytes = n; }
        return e;
    }
    operator T*() const { return p.get(); }
};

// AVSE_ERR_INVALID with `msg` while `s` (nullable) is being captured into a graph: for what allocates or waits
inline int not_capturing(hipStream_t s, const std::string& msg) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (s) AVSE_HIP_CHECK(hipStreamIsCapturing(s, &cs));
    return cs == hipStreamCaptureStatusNone ? 0 : fail(AVSE_ERR_INVALID, msg);
}

// Grows the scratch `b` to `need` bytes (its contents are not kept), never inside a capture: `what` names the scratch
// in the error and `before` says what the caller has to do ahead of the capture instead.
template <typename T, bool Host>
int grow(Owned<T, Host>& b, size_t need, hipStream_t s, const char* what,
         const char* before = "run one call of this size before the capture") {
    if (need <= b.bytes) return 0;
    if (int rc = not_capturing(s, std::string("the ") + what + " would grow while the stream is being captured: " + before))
        return rc;
    if (b.alloc(need) != hipSuccess)
        return fail(AVSE_ERR_OOM, std::string(Host ? "hipHostMalloc" : "hipMalloc") + " failed (" + what + ")");
    return 0;
}

// device copy of the mel filterbank as one run of non-zero bins per band (spec_tables.h MelBands)
struct MelTable {
    int max_width = 0;         // max non-zero bins per band
    Owned<int> start, width;   // [n_mels]
    Owned<float> weight;       // [n_mels][max_width]
    int seg_nq[4] = {6, 6, 6, 6};   // k_spec640: 4-bin weight quads its mel pass j (bands 64 j / 3 ..) needs
    int seg_nq4[4] = {7, 7, 7, 7};  // k_spec_seg: the same from the band start rounded down to a multiple of 4 bins
};

struct SpecTables {
    int sr = -1, n_fft = -1, n_mels = -1;
    double fmin = 0, fmax = 0;
    Owned<float2> twiddle;
    Owned<float> window;
    MelTable mel;
};

struct IstftTables {
    int sr = -1, n_fft = -1, n_mels = -1;
    double fmin = 0, fmax = 0;
    Owned<float> pinvT;      // [n_mels][nb]
    Owned<float2> twiddle;   // [N]
    Owned<float> window;     // [N]
    Owned<float4> bins;      // [nb] the <= 2 adjacent filters covering each bin
    Owned<float> gram_inv;   // [n_mels][n_mels] (M M^T)^{-1} in float (n_mels == 80 only)
};

// device copies of the evaluate stage's tables (eval_tables.cpp), per sample rate and resampling path
struct EvalTables {
    int sr = -1;
    bool big = false;        // max(up, down) > 24 and built for AVSE_EVAL_ANY_RATE: ptaps in place of taps
    Owned<double> taps;      // [2 H + 1] (big: not allocated)
    Owned<double> ptaps;     // big only: [up][2 H / up + 1], the taps by phase
    Owned<double> W;         // [256]
    Owned<double> twid;      // [256] (re, im)
    Owned<double> segw;      // [win]
    Owned<int> bands;        // [15] (lo, hi)
    int up = 1, down = 1, H = 0, win = 0;
};

// device copy of one resampling ratio's taps by phase (resample.hip avse_resample_ragged)
struct ResampleTables {
    int up = 0, down = 0;
    Owned<double> ptaps;     // [up][2 H / up + 1]
};

// The tables of one geometry on the current device, kept when `t` already holds them (capi.hip): the context's own
// (replaced when a call names another geometry) and a streaming session's, which lives as long as the session.
int build_spec_tables(SpecTables& t, int sr, int n_fft, int n_mels, double fmin, double fmax);
int build_istft_tables(IstftTables& t, int sr, int n_fft, int n_mels, double fmin, double fmax);

struct GpuLayer {
    LayerDef def;
    int cin_pad = 0;
    int hq = 0, wq = 0, ho = 0, wo = 0;
    int nphase = 1;
    ConvPhase ph[MAX_PHASES];
    void* w = nullptr;
    float* scale = nullptr;
    float* shift = nullptr;
    int2* taps = nullptr;
    int halo = HALO_NONE;     // halo-tiled kernel variant (bf16 video convs)
    void* w_halo = nullptr;   // packing for conv_stream.hip / conv_v1r.hip (weight_pack.h)
    void* w_dense = nullptr;  // a_conv1 only (bf16): [Cout][32], k = ky * kw + kx, for conv_aud.hip
    float* w_f32 = nullptr;   // a_conv1 only (split): [kh * kw][Cout] f32 x 2^e_n, for conv.hip k_aconv1_split
    float* scale_h = nullptr; // |scale| for w_halo: channels with a negative BN scale have negated weights
    int2 htaps[MAX_TAPS * MAX_PHASES] = {};   // host copy of taps (conv_dec.hip's kernel arguments)
};

}  // namespace avse

struct avse_ctx {
    int device = 0;
    avse::Options opt;          // kernel-path switches (read from AVSE_* once, at creation)
    avse::SpecTables spec;
    avse::IstftTables istft;
    avse::EvalTables eval[4];   // the last four (sample rate, resampling path) of avse_eval_pairs*, replaced in turn
    int eval_next = 0;
    avse::ResampleTables resample[4];   // the last four ratios of avse_resample_ragged, replaced in turn
    int resample_next = 0;
    avse::Owned<float> frames;      // ISTFT frame scratch
    avse::Owned<unsigned> umax;     // spectrogram: one word per utterance
    avse::Owned<float> mse_partial;
    avse::Owned<float> zero_video;  // one all-zero [128][128][8] clip (video == NULL forwards, any F <= 8)
    avse::Owned<int> gemm_counters; // gemm.hip split-K tickets (zero between launches)
    // AVSE_F32_SPLIT range guard words (mfma_util.h pair_out_of_range): [0] sticky for avse_forward (read and cleared
    // by avse_range_status), [1] cleared and read by each avse_forward_checked, [2] the all-zero-video embedding
    avse::Owned<unsigned> range;
    avse::Owned<unsigned, true> range_host;   // pinned readback words
    avse::Owned<char> arena;    // forward scratch (forward_plan.h arena_bytes)
    avse::Owned<char> prep;     // avse_mix_pairs / avse_video_stats / avse_eval_pairs scratch, ragged tables
    // ragged STFT / ISTFT: the pinned host copy of the per-utterance rows and the item table (uploaded into `prep`),
    // and the event after which the last upload has read it
    avse::Owned<char, true> ragged_host;
    hipEvent_t ragged_done = nullptr;
    avse::ArenaShape last_shape = avse::arena_shape(avse::kPlan25);   // of the last forward (avse_debug_scratch's layout)
    // side stream for the audio branch of the forward (runs concurrently with the video encoder)
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    // avse_forward's replay cache: the whole forward captured once per argument set into a hipGraph
    struct Graph {
        const void* key[10];   // forward_dispatch: weights, pointers, arena, range word, video dtype
        int64_t n;
        avse::Options opt;
        hipGraphExec_t exec;
    };
    std::vector<Graph> graphs;
    hipStream_t cap = nullptr;   // capture stream
    // avse_forward_mixed's row maps go up from a pinned ring, one slot of map_cap ints per call in turn (as the
    // streaming session's staging ring); map_ev[i] is recorded once the copy out of slot i is queued
    static constexpr int MAP_SLOTS = 4;
    avse::Owned<int, true> map_host;
    size_t map_cap = 0;
    hipEvent_t map_ev[MAP_SLOTS] = {};
    bool map_used[MAP_SLOTS] = {};
    int map_slot = 0;
    ~avse_ctx();
};

struct avse_weights {
    int dtype = 0;
    int device = 0;
    uint64_t serial = 0;                // unique per created weights object (graph-cache key: addresses get reused)
    avse::ArenaShape shape = avse::arena_shape(avse::kPlan25);   // the network shape these weights were built for
    avse::GpuLayer layers[avse::kNumLayers - 1];  // all but d_deconv6
    float* d6_w = nullptr;
    float d6_bias = 0.f;
    // the fused kernels the layers' shapes allow (weights.hip, at load; Options and *_supported decide per launch)
    bool aud_enc_shapes = false;    // conv_aud.hip: a_conv1 .. a_conv5
    bool dec_head_shapes = false;   // conv_dech.hip: d_deconv1 .. d_deconv3
    bool v6_gemm_shape = false;     // gemm.hip mode 1: v_conv6
    bool a1_valu_shape = false;     // conv.hip k_aconv1_split: a_conv1 (split dtype)
    // avse_forward with video == NULL (all-zero video input, BASELINE configs[2]): the video encoder's output is
    // then the same 2048-vector for every clip — computed once on first use and broadcast into the concat rows.
    // Published only after its stream has finished (another stream / thread may read it right away), under a lock.
    mutable std::atomic<void*> vzero_emb{nullptr};
    mutable std::mutex vzero_mu;
    mutable unsigned vzero_range = 0;   // split: range-guard bits the embedding's computation raised (sticky per forward)
    // AVSE_F32_SPLIT: per-layer power-of-two activation exponents (act_exponents: layer i stores the pairs of
    // x 2^act_exp[i]), the canonical blob (host copy) and, built from it on the first range-guard hit, the same network
    // on exact-fp32 MFMA that avse_forward_checked recomputes such a batch on
    int act_exp[avse::kNumLayers] = {};
    std::vector<float> blob;
    mutable avse_weights* f32_twin = nullptr;
    mutable std::mutex twin_mu;
    std::vector<avse::Owned<char>> allocs;   // every device buffer the layers point into
    ~avse_weights();
};
