// Host-only geometry of the streaming frame retimer (no HIP header; include/avse.h avse_retime_*, avse_retimer_*): the
// rule of which rate pairs are served, the counts of final output frames and slices, and for one call the refusal
// decision and one row per stream.  RetimeRow is also the device-side layout (retime.hip uploads the rows and k_retime
// reads them).  Nothing here allocates: the caller owns every array.
//
// The definition: p / q = fps_in / fps_out, reduced.  Output frame j sits at input position j p / q: with c = j p,
// i0 = c div q, r = c mod q it is the blend ((q - r) A[i0] + r A[min(i0 + 1, n - 1)]) / q of two input frames (retime.hip
// states the rounding per dtype; r == 0 is A[i0]'s bits).  Output j reads inputs up to ceil(j p / q), so after n >= 1
// inputs G(n) = floor((n - 1) q / p) + 1 outputs are final (G(0) = 0); a flush brings the total to ceil(n q / p), the
// frames past G(n) clamping to the last input.  F consecutive outputs form slice k in the session's layout
// [128][128][F]; G div F slices are complete, and a flush drops the remainder.  For an output that becomes final in a
// call i0 >= n_old - 1, so the last input frame and the G mod F frames of the unfinished slice are all the state a
// stream needs.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>

namespace avse {

constexpr int64_t RETIME_MAX_RATIO = 65536;      // max(p, q) served: the uint8 blend 2 (a (q - r) + b r) + q fits 32 bits
constexpr int RETIME_BLOCK = 256;                // lanes per block (k_retime); a lane owns 16 bytes of a frame's row
constexpr int RETIME_PIXELS = 128 * 128;         // per frame
constexpr int64_t RETIME_MAX_TOTAL = 1LL << 40;  // frames per stream: j p and n q stay inside int64

struct RetimeCfg {
    int64_t p = 1, q = 1;   // fps_in / fps_out, reduced
    int F = 5;              // output frames per slice
    int tiles = 16;         // blocks per slice (and per history frame): RETIME_PIXELS / (RETIME_BLOCK * 16 / elem size)
};

enum RetimeStatus {
    RETIME_OK = 0,
    RETIME_BAD_RATE,       // a numerator or denominator <= 0 (or past 2^31 - 1)
    RETIME_RATIO,          // max(p, q) > RETIME_MAX_RATIO after reduction
    RETIME_BAD_COUNT,      // a negative n_new or frame offset
    RETIME_TOO_LARGE,      // totals past 2^40 frames
    RETIME_AFTER_FLUSH,    // input or a second flush for a flushed stream
    RETIME_OUT_SMALL,      // out NULL or fewer slices in it than the call completes
};

inline const char* retime_message(int status) {
    switch (status) {
        case RETIME_BAD_RATE: return "frame rates must be positive (numerators and denominators in 1 .. 2^31 - 1)";
        case RETIME_RATIO: return "max(p, q) above 65536 after reduction";
        case RETIME_BAD_COUNT: return "negative counts";
        case RETIME_TOO_LARGE: return "counts too large";
        case RETIME_AFTER_FLUSH: return "pushed or flushed after its flush: only a reset is legal";
        case RETIME_OUT_SMALL: return "out is NULL or holds fewer slices than the call completes";
        default: return "ok";
    }
}

// p / q = (in_num / in_den) / (out_num / out_den), reduced; *cfg is written for RETIME_OK and RETIME_RATIO (the reduced
// ratio, for the message).  F and tiles are the caller's to set.
inline int retime_cfg(int64_t in_num, int64_t in_den, int64_t out_num, int64_t out_den, RetimeCfg* cfg) {
    for (int64_t v : {in_num, in_den, out_num, out_den})
        if (v <= 0 || v > INT32_MAX) return RETIME_BAD_RATE;
    const int64_t a = in_num * out_den, b = in_den * out_num, g = std::gcd(a, b);
    RetimeCfg c = *cfg;
    c.p = a / g;
    c.q = b / g;
    *cfg = c;
    return std::max(c.p, c.q) > RETIME_MAX_RATIO ? RETIME_RATIO : RETIME_OK;
}

// output frames that are final after n inputs: G(n), or ceil(n q / p) once flushed (0 <= n <= RETIME_MAX_TOTAL)
inline int64_t retime_total(const RetimeCfg& g, int64_t n, bool flushed) {
    if (n <= 0) return 0;
    return flushed ? (n * g.q + g.p - 1) / g.p : (n - 1) * g.q / g.p + 1;
}

// slices a stream has handed out: a flush drops the unfinished one
inline int64_t retime_slices(const RetimeCfg& g, int64_t n, bool flushed) { return retime_total(g, n, flushed) / g.F; }

// What a retimer keeps per stream between calls.
struct RetimeState {
    int64_t n;           // frames received
    uint8_t flushed;
    uint8_t parity;      // which copy holds the stream's last input frame and the frames of its unfinished slice
};

// One stream's part of one call.  The stream's history is hist[copy][stream][128][128] (its last input frame) and
// pend[copy][stream][128][128][F] (the g_old mod F finished frames of slice g_old div F, frame innermost like a slice).
// The call's slots are the slices g_old div F .. : k_new complete ones, which go to `out`, then (unless the call
// flushes) the unfinished one when it holds any frame, which goes to copy hist_out of pend.
struct RetimeRow {
    int64_t n_old, n_new;   // frames received before / after this call
    int64_t g_old, g_new;   // output frames final before / after it (g_new: the flushed total when the call flushes)
    int64_t frame_off;      // first frame of this call's frames in `frames`
    int64_t out_slice;      // first slice of this call's slices in `out`
    int32_t k_new;          // slices completed by this call
    int32_t n_slots;        // slices the call's blocks write: k_new, plus the unfinished one
    int32_t blk0;           // the stream's first block (exclusive prefix sum of the streams' blocks)
    int32_t hist_in, hist_out;   // the copy read / the one that holds the state afterwards
    int32_t fed;            // frames arrived: the blocks of the stream's last slot write copy hist_out of hist
    int32_t flush;          // the stream is closed by this call
    int32_t pad;
};
static_assert(sizeof(RetimeRow) == 80, "device row layout");

// A row's blocks come in slots of `tiles` blocks: one slot per slice it writes; the last slot also copies the call's
// last frame into the history, and a call that feeds frames without touching a slice has one slot that does only that.
inline int64_t retime_row_slots(const RetimeRow& r) { return std::max<int64_t>(r.n_slots, r.fed ? 1 : 0); }
inline int64_t retime_row_blocks(const RetimeCfg& g, const RetimeRow& r) { return retime_row_slots(r) * g.tiles; }

struct RetimePlan {
    int status = RETIME_OK;
    int64_t bad = -1;          // the first stream `status` refers to
    int64_t blocks = 0;        // the launch's grid
    int64_t slices = 0;        // slices completed by all streams
    int64_t fed = 0;           // frames of all streams in this call
};

// One row from a stream's state and its part of the call; RETIME_OK or the refusal.  blk0 and out_slice are the
// caller's running sums.
inline int retime_row(const RetimeCfg& g, const RetimeState& s, int64_t dn, bool fl, int64_t frame_off, RetimeRow* row) {
    if (dn < 0 || (dn > 0 && frame_off < 0)) return RETIME_BAD_COUNT;
    if (dn > RETIME_MAX_TOTAL - s.n) return RETIME_TOO_LARGE;
    if (s.flushed && (dn > 0 || fl)) return RETIME_AFTER_FLUSH;
    RetimeRow r{};
    r.n_old = s.n;
    r.n_new = s.n + dn;
    r.g_old = retime_total(g, s.n, s.flushed);
    r.g_new = retime_total(g, r.n_new, s.flushed || fl);
    const int64_t s0 = r.g_old / g.F, k_new = r.g_new / g.F - s0;
    // the unfinished slice is rewritten into the other copy whenever frames arrived: the copies swap then
    const bool partial = !fl && !s.flushed && dn > 0 && r.g_new % g.F != 0;
    if (k_new + 1 > INT32_MAX / g.tiles - 1) return RETIME_TOO_LARGE;
    r.k_new = (int32_t)k_new;
    r.n_slots = (int32_t)k_new + (partial ? 1 : 0);
    r.frame_off = dn > 0 ? frame_off : 0;
    r.hist_in = s.parity;
    r.hist_out = s.parity ^ (dn > 0 ? 1 : 0);
    r.fed = dn > 0 ? 1 : 0;
    r.flush = fl ? 1 : 0;
    *row = r;
    return RETIME_OK;
}

// The refusal decision and the rows of a call.  flush and frame_off may be NULL (no stream flushed; offsets 0, for a
// call without frames); have_out says whether the caller gave an `out`, out_cap how many slices it holds.  The streams'
// slices are packed stream-major in `out`.  On a refusal `rows` holds nothing to rely on; `st` is never written
// (retime_commit does that once the launch is in).
inline RetimePlan retime_rows(const RetimeCfg& g, const RetimeState* st, int64_t B, const int64_t* frame_off,
                              const int64_t* n_new, const uint8_t* flush, bool have_out, int64_t out_cap,
                              RetimeRow* rows) {
    RetimePlan p;
    auto refuse = [&](int status, int64_t b) {
        p.status = status;
        p.bad = b;
        return p;
    };
    for (int64_t b = 0; b < B; ++b) {
        RetimeRow& r = rows[b];
        if (int rc = retime_row(g, st[b], n_new[b], flush && flush[b], frame_off ? frame_off[b] : 0, &r)) return refuse(rc, b);
        if (r.k_new > 0 && (!have_out || out_cap - p.slices < r.k_new)) return refuse(RETIME_OUT_SMALL, b);
        if (p.blocks + retime_row_blocks(g, r) > INT32_MAX) return refuse(RETIME_TOO_LARGE, b);
        r.out_slice = p.slices;
        r.blk0 = (int32_t)p.blocks;
        p.blocks += retime_row_blocks(g, r);
        p.slices += r.k_new;
        p.fed += n_new[b];
    }
    return p;
}

// The states after the call the rows describe.
inline void retime_commit(const RetimeRow* rows, int64_t B, RetimeState* st) {
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
inline int retime_row_of(const RetimeRow* rows, int B, int blk) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].blk0 <= blk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Where input frame i of a stream is read from in a call: the history (the one frame of copy hist_in, i == n_old - 1)
// or the call's frames (index from frame_off).  Only n_old - 1 <= i < n_new is ever asked for.
enum RetimeSrc { RETIME_NONE = 0, RETIME_HIST, RETIME_NEW };
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int retime_source(const RetimeRow& r, int64_t i, int64_t* idx) {
    if (i < r.n_old - 1 || i < 0 || i >= r.n_new) return RETIME_NONE;
    if (i < r.n_old) return RETIME_HIST;
    *idx = r.frame_off + (i - r.n_old);
    return RETIME_NEW;
}

// The two input frames and the weight of output j: i0 = j p div q, r = j p mod q, i1 = min(i0 + 1, n_new - 1).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void retime_taps(int64_t p, int64_t q, int64_t n_new, int64_t j, int64_t* i0, int64_t* i1, int32_t* r) {
    const int64_t c = j * p;
    *i0 = c / q;
    *r = (int32_t)(c - *i0 * q);
    *i1 = *i0 + 1 < n_new ? *i0 + 1 : n_new - 1;
}

}  // namespace avse
