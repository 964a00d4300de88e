// Host-only geometry of the streaming resampler (no HIP header; include/avse.h avse_resample_*, avse_resampler_*): the
// rule of which rate pairs are served, the counts of final outputs, and for one call the refusal decision and one row
// per stream.  ResampleRow is also the device-side layout (resample.hip uploads the rows and k_resample reads them).
// Nothing here allocates: the caller owns every array.
//
// The definition is scipy.signal.resample_poly(x, up, down) with its defaults (eval_tables.h resample_taps):
//   y[k] = sum_j h[H + k down - j up] x[j] over the j in [0, n) that keep the tap index in [0, 2H], H = 10 max(up, down),
// ceil(n up / down) outputs.  Output k reads inputs up to floor((H + k down) / up), so after n inputs
// F(n) = max(0, ceil((n up - H) / down)) outputs are final; with c = H + k down = Bk up + phase its taps are row `phase`
// of resample_taps_by_phase, met by the T = 2H / up + 1 samples j = Bk - (T - 1) .. Bk in ascending order.  For
// k >= F(n_old), Bk >= n_old: the oldest sample an output of this call reads is n_old - (T - 1), so the last T inputs
// are all the state a stream needs.  Equal rates: the one tap {1.0}, H = 0, T = 1, a copy.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>

namespace avse {

constexpr int RESAMPLE_MAX_RATIO = 640;    // max(up, down) served: the by-phase taps are at most 640 x 21 doubles
constexpr int RESAMPLE_BLOCK = 256;        // outputs per block (k_resample)
constexpr int64_t RESAMPLE_MAX_TOTAL = 1LL << 40;   // samples per stream: k down <= n up + H stays far inside int64

struct ResampleCfg {
    int up = 1, down = 1, H = 0, T = 1;
};

enum ResampleStatus {
    RESAMPLE_OK = 0,
    RESAMPLE_BAD_RATE,      // a rate <= 0
    RESAMPLE_RATIO,         // max(up, down) > RESAMPLE_MAX_RATIO after reduction
    RESAMPLE_BAD_COUNT,     // a negative n_new
    RESAMPLE_TOO_LARGE,     // totals past 2^40 samples
    RESAMPLE_AFTER_FLUSH,   // input or a second flush for a flushed stream
    RESAMPLE_OUT_SMALL,     // out NULL or out_stride below what the stream emits
};

inline const char* resample_message(int status) {
    switch (status) {
        case RESAMPLE_BAD_RATE: return "sample rates must be positive";
        case RESAMPLE_RATIO: return "max(up, down) above 640 after reduction";
        case RESAMPLE_BAD_COUNT: return "negative counts";
        case RESAMPLE_TOO_LARGE: return "counts too large";
        case RESAMPLE_AFTER_FLUSH: return "pushed or flushed after its flush: only a reset is legal";
        case RESAMPLE_OUT_SMALL: return "out is NULL or out_stride below what the call emits";
        default: return "ok";
    }
}

// up / down = (sr_out / g) / (sr_in / g); *cfg is written for RESAMPLE_OK and RESAMPLE_RATIO (the reduced ratio, for
// the message)
inline int resample_cfg(int64_t sr_in, int64_t sr_out, ResampleCfg* cfg) {
    if (sr_in <= 0 || sr_out <= 0 || sr_in > INT32_MAX || sr_out > INT32_MAX) return RESAMPLE_BAD_RATE;
    const int64_t g = std::gcd(sr_in, sr_out);
    ResampleCfg c;
    c.up = (int)(sr_out / g);
    c.down = (int)(sr_in / g);
    *cfg = c;
    if (std::max(c.up, c.down) > RESAMPLE_MAX_RATIO) return RESAMPLE_RATIO;
    c.H = c.up == c.down ? 0 : 10 * std::max(c.up, c.down);
    c.T = 2 * c.H / c.up + 1;
    *cfg = c;
    return RESAMPLE_OK;
}

// outputs that are final after n inputs: F(n), or ceil(n up / down) once flushed
inline int64_t resample_total(const ResampleCfg& g, int64_t n, bool flushed) {
    if (flushed) return (n * g.up + g.down - 1) / g.down;
    const int64_t a = n * g.up - g.H;
    return a <= 0 ? 0 : (a + g.down - 1) / g.down;
}

// What a resampler keeps per stream between calls.
struct ResampleState {
    int64_t n;           // samples received
    uint8_t flushed;
    uint8_t parity;      // which history copy holds the stream's last T samples
};

// One stream's part of one call.  The stream's history is hist[copy][stream][T]: entry i of the copy written by a call
// is sample n_new - T + i (0 where that is negative), so sample j < n_old sits at j - (n_old - T) of copy hist_in.
struct ResampleRow {
    int64_t n_old, n_new;   // samples received before / after this call
    int64_t k0;             // first output of this call
    int64_t sample_off;     // first float of this call's samples in `samples`
    int64_t out_off;        // first float of this call's outputs in `out`
    int32_t n_out;          // outputs of this call
    int32_t blk0;           // the stream's first block (exclusive prefix sum of the streams' blocks)
    int32_t hist_in, hist_out;   // the history copy read / the one holding the last T samples afterwards
    int32_t fed;            // samples arrived: the stream's last block writes copy hist_out
    int32_t flush;          // the stream is closed by this call
};
static_assert(sizeof(ResampleRow) == 64, "device row layout");

inline int64_t resample_row_blocks(const ResampleRow& r) {
    return ((int64_t)r.n_out + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK + (r.fed ? 1 : 0);
}

struct ResamplePlan {
    int status = RESAMPLE_OK;
    int64_t bad = -1;          // the first stream `status` refers to
    int64_t blocks = 0;        // the launch's grid
    int64_t max_n_out = 0;
    int64_t fed = 0;           // samples of all streams in this call
};

// The refusal decision and the rows of a call.  flush and sample_off may be NULL (no stream flushed; offsets 0, for a
// call without samples); have_out says whether the caller gave an `out`.  On a refusal `rows` holds nothing to rely on;
// `st` is never written (resample_commit does that once the launch is in).
inline ResamplePlan resample_rows(const ResampleCfg& g, const ResampleState* st, int64_t B, const int64_t* sample_off,
                                  const int64_t* n_new, const uint8_t* flush, bool have_out, int64_t out_stride,
                                  ResampleRow* rows) {
    ResamplePlan p;
    auto refuse = [&](int status, int64_t b) {
        p.status = status;
        p.bad = b;
        return p;
    };
    for (int64_t b = 0; b < B; ++b) {
        const ResampleState& s = st[b];
        const int64_t dn = n_new[b];
        const bool fl = flush && flush[b];
        if (dn < 0) return refuse(RESAMPLE_BAD_COUNT, b);
        if (dn > RESAMPLE_MAX_TOTAL - s.n) return refuse(RESAMPLE_TOO_LARGE, b);
        if (s.flushed && (dn > 0 || fl)) return refuse(RESAMPLE_AFTER_FLUSH, b);
        const int64_t n2 = s.n + dn;
        const int64_t k0 = resample_total(g, s.n, s.flushed), k1 = resample_total(g, n2, s.flushed || fl);
        const int64_t n_out = k1 - k0;
        if (n_out > INT32_MAX - RESAMPLE_BLOCK) return refuse(RESAMPLE_TOO_LARGE, b);
        if (n_out > 0 && (!have_out || out_stride < n_out)) return refuse(RESAMPLE_OUT_SMALL, b);
        ResampleRow& r = rows[b];
        r.n_old = s.n;
        r.n_new = n2;
        r.k0 = k0;
        r.sample_off = sample_off && dn > 0 ? sample_off[b] : 0;
        r.out_off = b * out_stride;
        r.n_out = (int32_t)n_out;
        r.hist_in = s.parity;
        r.hist_out = s.parity ^ (dn > 0 ? 1 : 0);
        r.fed = dn > 0 ? 1 : 0;
        r.flush = fl ? 1 : 0;
        if (p.blocks + resample_row_blocks(r) > INT32_MAX) return refuse(RESAMPLE_TOO_LARGE, b);
        r.blk0 = (int32_t)p.blocks;
        p.blocks += resample_row_blocks(r);
        p.max_n_out = std::max(p.max_n_out, n_out);
        p.fed += dn;
    }
    return p;
}

// The states after the call the rows describe.
inline void resample_commit(const ResampleRow* rows, int64_t B, ResampleState* st) {
    for (int64_t b = 0; b < B; ++b) {
        st[b].n = rows[b].n_new;
        st[b].flushed = st[b].flushed || rows[b].flush;
        st[b].parity = (uint8_t)rows[b].hist_out;
    }
}

// The row whose blocks hold block `blk` (0 <= blk < the plan's blocks): the last row with blk0 <= blk.  Rows without
// blocks share their blk0 with the next row that has some, so they are never the last.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int resample_row_of(const ResampleRow* rows, int B, int blk) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].blk0 <= blk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Where sample j of a stream is read from in a call: RESAMPLE_ZERO (outside [0, n_new): the definition's zeros), the
// history (index into copy hist_in) or the call's chunk (index from sample_off).
enum ResampleSrc { RESAMPLE_ZERO = 0, RESAMPLE_HIST, RESAMPLE_NEW };
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int resample_source(const ResampleRow& r, int T, int64_t j, int64_t* idx) {
    if (j < 0 || j >= r.n_new || j < r.n_old - T) return RESAMPLE_ZERO;   // the last: never asked for (k >= F(n_old))
    if (j < r.n_old) {
        *idx = j - (r.n_old - T);
        return RESAMPLE_HIST;
    }
    *idx = j - r.n_old;
    return RESAMPLE_NEW;
}

}  // namespace avse
