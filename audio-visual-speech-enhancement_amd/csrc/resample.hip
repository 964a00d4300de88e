// The streaming resampler (include/avse.h avse_resample_*, avse_resampler_*): one kernel for the
// per-stream push, the flush and the one-shot ragged call, driven by the host rows of resample_geom.h.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ctx.h"
#include "eval_tables.h"
#include "resample_geom.h"

namespace avse {
namespace {

struct ResampleArgs {
    const float* news;        // + the row's sample_off
    const float* hist;        // [2][B][T]: the copy a row names by hist_in
    float* hist_w;            // the same buffer, written at hist_out
    float* out;               // + the row's out_off
    const double* ptaps;      // [up][T] (eval_tables.h resample_taps_by_phase)
    int up, down, H, T, B;
};

// sample j of the row's stream, 0 outside [0, n_new)
__device__ __forceinline__ float resample_sample(const ResampleArgs& a, const ResampleRow& r, int b, int64_t j) {
    int64_t i = 0;
    switch (resample_source(r, a.T, j, &i)) {
        case RESAMPLE_HIST: return a.hist[((size_t)r.hist_in * a.B + b) * a.T + i];
        case RESAMPLE_NEW: return a.news[r.sample_off + i];
        default: return 0.f;
    }
}

// One block per 256 outputs of a stream, plus one per stream that received samples (its last block), which writes the
// stream's last T samples into the history copy the call does not read.  Output k = k0 + i: with
// c = H + k down = Bk up + phase, its taps are row `phase` of ptaps and meet the samples Bk - (T - 1) .. Bk in ascending
// order (a row whose first tap would pass 2H starts with a zero): T fmas in float64 from 0.0, one rounding to float32.
// A sample outside [0, n_new) is 0.f, which leaves the sum as it is, so the value is that of the definition's sum over
// the samples that exist.  The taps are read per lane from global memory: a lane walks its own row front to back (T
// consecutive doubles, 128-byte lines of 16 taps each used 16 times by the lane that fetched them), and the whole table
// (at most 105 KB) stays in L2; staging it in LDS would cost every block of 256 outputs the load of all up x T taps to
// use 256 x T of them.
__global__ __launch_bounds__(RESAMPLE_BLOCK) void k_resample(ResampleArgs a, const ResampleRow* __restrict__ rows,
                                                             int n_rows) {
    const int b = resample_row_of(rows, n_rows, (int)blockIdx.x);
    const ResampleRow r = rows[b];
    const int chunk = (int)blockIdx.x - r.blk0;
    const int nout_blocks = (r.n_out + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK;
    if (chunk >= nout_blocks) {   // the history block (r.fed)
        if (!r.fed) return;
        float* h = a.hist_w + ((size_t)r.hist_out * a.B + b) * a.T;
        for (int i = threadIdx.x; i < a.T; i += RESAMPLE_BLOCK) h[i] = resample_sample(a, r, b, r.n_new - a.T + i);
        return;
    }
    const int i = chunk * RESAMPLE_BLOCK + (int)threadIdx.x;
    if (i >= r.n_out) return;
    const int64_t k = r.k0 + i;
    if (a.H == 0) {   // equal rates: the sample's bits (a sum from +0.0 would turn -0.0 into +0.0)
        a.out[r.out_off + i] = resample_sample(a, r, b, k);
        return;
    }
    const int64_t c =(int64_t)a.H + k * a.down;
    const int64_t Bk = c / a.up;
    const int phase = (int)(c - Bk * a.up);
    const double* hp = a.ptaps + (size_t)phase * a.T;
    const int64_t j0 = Bk - (a.T - 1);
    double acc = 0.0;
    for (int q = 0; q < a.T; ++q) acc = fma(hp[q], (double)resample_sample(a, r, b, j0 + q), acc);
    a.out[r.out_off + i] = (float)acc;
}

int build_resample_taps(const ResampleCfg& g, Owned<double>& out) {
    const std::vector<double> rows = resample_taps_by_phase(resample_taps(g.up, g.down), g.up);
    if (out.alloc(sizeof(double) * rows.size()) != hipSuccess) return fail(AVSE_ERR_OOM, "hipMalloc failed (resampler taps)");
    AVSE_HIP_CHECK(hipMemcpy(out, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
    return 0;
}

int resample_cfg_checked(int sr_in, int sr_out, ResampleCfg* g) {
    const int st = resample_cfg(sr_in, sr_out, g);
    if (st == RESAMPLE_BAD_RATE) return fail(AVSE_ERR_INVALID, resample_message(st));
    if (st == RESAMPLE_RATIO)
        return fail(AVSE_ERR_UNSUPPORTED, "resampling " + std::to_string(sr_in) + " -> " + std::to_string(sr_out) + " is the ratio " +
                                              std::to_string(g->up) + " / " + std::to_string(g->down) + ": " + resample_message(st));
    return 0;
}

ResampleArgs resample_args(const ResampleCfg& g, const double* ptaps, const float* news, float* hist, float* out, int B) {
    ResampleArgs a;
    a.news = news; a.hist = hist; a.hist_w = hist; a.out = out; a.ptaps = ptaps;
    a.up = g.up; a.down = g.down; a.H = g.H; a.T = g.T; a.B = B;
    return a;
}

}  // namespace
}  // namespace avse

using namespace avse;

struct avse_resampler {
    avse_ctx* ctx = nullptr;
    int64_t B = 0;
    ResampleCfg g;
    Owned<double> ptaps;
    Owned<float> hist;        // [2][B][T]
    std::vector<ResampleState> st;
    std::vector<int64_t> emitted;
    // the rows of the call being decided, their device copy, and the pinned staging ring they go up from (one slot per
    // call in turn; `staged[i]` is recorded once the copy out of slot i is queued)
    static constexpr int SLOTS = 4;
    std::vector<ResampleRow> rows;
    size_t slot_bytes = 0;
    Owned<char, true> staging;
    Owned<char> tables;
    hipEvent_t staged[SLOTS] = {};
    bool staged_used[SLOTS] = {};
    int slot = 0;
    ~avse_resampler() {
        for (hipEvent_t e : staged)
            if (e) (void)hipEventDestroy(e);
    }
};

extern "C" {

int avse_resample_supported(int sr_in, int sr_out) {
    ResampleCfg g;
    return resample_cfg_checked(sr_in, sr_out, &g);
}

int avse_resample_counts(int sr_in, int sr_out, int64_t n_in, int flushed, int64_t* n_out) {
    if (!n_out) return fail(AVSE_ERR_INVALID, "NULL argument");
    ResampleCfg g;
    if (int rc = resample_cfg_checked(sr_in, sr_out, &g)) return rc;
    if (n_in < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    if (n_in > RESAMPLE_MAX_TOTAL) return fail(AVSE_ERR_INVALID, "counts too large");
    *n_out = resample_total(g, n_in, flushed != 0);
    return 0;
}

int avse_resample_ragged(avse_ctx* c, const float* sig, const int64_t* sig_off, const int64_t* n_samples, int64_t n_utt,
                         int sr_in, int sr_out, float* out, const int64_t* out_off, void* stream) {
    if (!c || !sig_off || !n_samples || !out_off) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n_utt < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    ResampleCfg g;
    if (int rc = resample_cfg_checked(sr_in, sr_out, &g)) return rc;
    if (n_utt == 0) return 0;
    if (n_utt > (1 << 24)) return fail(AVSE_ERR_INVALID, "batch too large");
    // every utterance a fresh stream that is fed and flushed at once; no history is read or written
    std::vector<ResampleRow> rows((size_t)n_utt);
    int64_t blocks = 0;
    for (int64_t u = 0; u < n_utt; ++u) {
        const int64_t n = n_samples[u];
        if (n < 0 || sig_off[u] < 0 || out_off[u] < 0) return fail(AVSE_ERR_INVALID, "utterance " + std::to_string(u) + ": negative counts");
        const int64_t n_out = n > RESAMPLE_MAX_TOTAL ? INT64_MAX : resample_total(g, n, true);
        if (n_out > INT32_MAX - RESAMPLE_BLOCK) return fail(AVSE_ERR_INVALID, "utterance " + std::to_string(u) + ": counts too large");
        ResampleRow& r = rows[(size_t)u];
        std::memset(&r, 0, sizeof(r));
        r.n_new = n;
        r.sample_off = sig_off[u];
        r.out_off = out_off[u];
        r.n_out = (int32_t)n_out;
        r.flush = 1;
        r.blk0 = (int32_t)blocks;
        blocks += resample_row_blocks(r);
        if (blocks > INT32_MAX) return fail(AVSE_ERR_INVALID, "batch too large");
    }
    if (blocks == 0) return 0;
    if (!sig || !out) return fail(AVSE_ERR_INVALID, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    // the taps of this ratio: the context keeps the last four
    ResampleTables* t = nullptr;
    for (ResampleTables& have : c->resample)
        if (have.up == g.up && have.down == g.down) t = &have;
    if (!t) {
        if (int rc = not_capturing(s, "the taps of this ratio would be built while the stream is being captured: run one "
                                      "call with this ratio before the capture"))
            return rc;
        t = &c->resample[c->resample_next];
        c->resample_next = (c->resample_next + 1) % 4;
        t->up = t->down = 0;
        if (int rc = build_resample_taps(g, t->ptaps)) return rc;
        t->up = g.up; t->down = g.down;
    }
    // the rows: through the pinned copy into the preprocess scratch, as a ragged spectrogram's tables go
    const size_t need = sizeof(ResampleRow) * rows.size();
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (s) AVSE_HIP_CHECK(hipStreamIsCapturing(s, &cs));
    const bool capturing = cs != hipStreamCaptureStatusNone;
    if (int rc = grow(c->prep, need, s, "preprocess scratch")) return rc;
    if (!capturing && c->ragged_done) AVSE_HIP_CHECK(hipEventSynchronize(c->ragged_done));   // the last upload has read it
    if (int rc = grow(c->ragged_host, need, s, "ragged tables")) return rc;
    if (!c->ragged_done) AVSE_HIP_CHECK(hipEventCreateWithFlags(&c->ragged_done, hipEventDisableTiming));
    std::memcpy(c->ragged_host, rows.data(), need);
    AVSE_HIP_CHECK(hipMemcpyAsync(c->prep, c->ragged_host, need, hipMemcpyHostToDevice, s));
    if (!capturing) AVSE_HIP_CHECK(hipEventRecord(c->ragged_done, s));
    hipLaunchKernelGGL(k_resample, dim3((unsigned)blocks), dim3(RESAMPLE_BLOCK), 0, s,
                       resample_args(g, t->ptaps, sig, nullptr, out, 0), reinterpret_cast<const ResampleRow*>(c->prep.p.get()),
                       (int)n_utt);
    AVSE_HIP_CHECK(hipGetLastError());
    return 0;
}

int avse_resampler_create(avse_ctx* c, int64_t n_streams, int sr_in, int sr_out, avse_resampler** out) {
    if (!c || !out) return fail(AVSE_ERR_INVALID, "NULL argument");
    ResampleCfg g;
    if (int rc = resample_cfg_checked(sr_in, sr_out, &g)) return rc;
    if (n_streams < 1) return fail(AVSE_ERR_INVALID, "n_streams must be positive");
    if (n_streams > 1024) return fail(AVSE_ERR_UNSUPPORTED, "at most 1024 streams");
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    std::unique_ptr<avse_resampler> r(new avse_resampler());
    r->ctx = c; r->B = n_streams; r->g = g;
    if (int rc = build_resample_taps(g, r->ptaps)) return rc;
    const size_t B = (size_t)n_streams;
    r->st.assign(B, ResampleState{0, 0, 0});
    r->emitted.assign(B, 0);
    r->rows.resize(B);
    r->slot_bytes = (sizeof(ResampleRow) * B + 255) & ~(size_t)255;
    if (r->hist.alloc(sizeof(float) * 2 * B * g.T) != hipSuccess || r->tables.alloc(r->slot_bytes) != hipSuccess)
        return fail(AVSE_ERR_OOM, "hipMalloc failed (resampler)");
    if (r->staging.alloc(r->slot_bytes * avse_resampler::SLOTS) != hipSuccess)
        return fail(AVSE_ERR_OOM, "hipHostMalloc failed (resampler)");
    for (hipEvent_t& e : r->staged) AVSE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    AVSE_HIP_CHECK(hipMemset(r->hist, 0, r->hist.bytes));
    AVSE_HIP_CHECK(hipStreamSynchronize(nullptr));
    *out = r.release();
    return 0;
}

int avse_resampler_push_each(avse_resampler* r, const float* samples, const int64_t* sample_off, const int64_t* n_new,
                             const uint8_t* flush, float* out, int64_t out_stride, int64_t* host_n_out, void* stream) {
    if (!r || !n_new || !host_n_out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (out_stride < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    const int B = (int)r->B;
    ResampleRow* rows = r->rows.data();
    const ResamplePlan p = resample_rows(r->g, r->st.data(), B, sample_off, n_new, flush, out != nullptr, out_stride, rows);
    if (p.status != RESAMPLE_OK)
        return fail(AVSE_ERR_INVALID, "stream " + std::to_string(p.bad) + ": " + resample_message(p.status));
    if (p.fed > 0 && (!samples || !sample_off)) return fail(AVSE_ERR_INVALID, "NULL argument");
    for (int b = 0; b < B; ++b) host_n_out[b] = rows[b].n_out;
    hipStream_t s = (hipStream_t)stream;
    if (p.blocks > 0) {
        if (int rc = not_capturing(s, "a resampler push cannot be captured into a graph")) return rc;
        AVSE_HIP_CHECK(hipSetDevice(r->ctx->device));
        // the next slot of the staging ring, once the copy that last left it has been read: the call's only wait
        const int i = r->slot;
        if (r->staged_used[i]) AVSE_HIP_CHECK(hipEventSynchronize(r->staged[i]));
        char* host = r->staging + (size_t)i * r->slot_bytes;
        const size_t bytes = sizeof(ResampleRow) * (size_t)B;
        std::memcpy(host, rows, bytes);
        AVSE_HIP_CHECK(hipMemcpyAsync(r->tables, host, bytes, hipMemcpyHostToDevice, s));
        AVSE_HIP_CHECK(hipEventRecord(r->staged[i], s));
        r->staged_used[i] = true;
        r->slot = (i + 1) % avse_resampler::SLOTS;
        // a launch that fails ran nothing: the copy the rows' streams read is untouched, and so the state stays
        hipLaunchKernelGGL(k_resample, dim3((unsigned)p.blocks), dim3(RESAMPLE_BLOCK), 0, s,
                           resample_args(r->g, r->ptaps, samples, r->hist, out, B),
                           reinterpret_cast<const ResampleRow*>(r->tables.p.get()), B);
        AVSE_HIP_CHECK(hipGetLastError());
    }
    resample_commit(rows, B, r->st.data());
    for (int b = 0; b < B; ++b) r->emitted[b] += rows[b].n_out;
    return 0;
}

int avse_resampler_reset_each(avse_resampler* r, const uint8_t* which, void* stream) {
    if (!r) return fail(AVSE_ERR_INVALID, "NULL argument");
    (void)stream;   // host counters only: a stream with n == 0 never reads its history, and work queued earlier has its rows
    for (int64_t b = 0; b < r->B; ++b)
        if (!which || which[b]) {
            r->st[b].n = 0;
            r->st[b].flushed = 0;   // the parity stays: either copy serves a fresh stream
            r->emitted[b] = 0;
        }
    return 0;
}

int avse_resampler_state(const avse_resampler* r, int64_t* n_in, int64_t* n_out, uint8_t* flushed) {
    if (!r) return fail(AVSE_ERR_INVALID, "NULL argument");
    for (int64_t b = 0; b < r->B; ++b) {
        if (n_in) n_in[b] = r->st[b].n;
        if (n_out) n_out[b] = r->emitted[b];
        if (flushed) flushed[b] = r->st[b].flushed;
    }
    return 0;
}

void avse_resampler_destroy(avse_resampler* r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->device);
    delete r;
}

}  // extern "C"
