// Host-only geometry of a sliding streaming session (K21, include/avse.h avse_slide_*; no HIP header): a session whose
// network windows start at every `stride`-th video frame instead of every slice.  The totals of one stream
// (slide_totals), the refusal decision of a call, one row per stream and one item table per kernel, block -> (stream,
// chunk).  SlideRow is also the device-side layout of the kernels that are new here (k_slide_route, k_slide_gather,
// k_slide_synth); the analysis and the overlap-add run the per-stream instances of K17's kernels and read a StreamRow
// (stream_geom.h) that slide_rows fills beside it.  Nothing here allocates: the caller owns every array.
//
// With N = n_fft, H = hop, spf frames and F video frames per window, q = spf / F and the stride s (1 <= s <= F), a
// stream that has received n samples and f video frames has
//   frames    = n < N/2 + 1 ? 0 : (n - N/2) / H + 1          (flushed: q f)
//   wa        = frames >= spf ? (frames - spf) / (q s) + 1 : 0      windows its samples complete
//   wv        = f >= F ? (f - F) / s + 1 : 0                          windows its video completes
//   windows   = min(wa, wv)
//   predicted = windows > 0 ? spf + q s (windows - 1) : 0            window 0 keeps spf columns, a later one its last q s
//   emitted   = max(0, H predicted - N/2)                             (flushed: predicted > 0 ? H (predicted - 1) : 0)
// With s = F these are stream_totals at v = f / F.
//
// Limits of a call, M = max_windows, all on the totals after the call (n2, f2, closed = flushed before or by the call):
//   windows(n2, f2) - windows(n, f) <= M          else SLIDE_TOO_MANY
//   wa(n2) - windows(n2, f2) <= M                 else SLIDE_SAMPLES_AHEAD   (samples at most M strides ahead of the video)
//   wv(f2) - windows(n2, f2) <= M                 else SLIDE_VIDEO_AHEAD     (video at most M strides ahead of the samples)
//   a flush needs n2 <= H q f2                    else SLIDE_FLUSH_SHORT     (after a flush wa == wv)
// Rings.  With w windows done before a call, the oldest frame any later window reads is q s w, and the limits give
// frames2 <= spf + q s (w2 + M) - 1 with w2 <= w + M: the live frames [q s w, frames2) of a call are fewer than
// spf + 2 q s M.  The frame-slotted rings (maxima, phases, time frames) have R = spf RS slots, and the slice-slotted
// mel ring RS = ceil((spf + 2 q s M) / spf) + 1 slots: a run of fewer than spf + 2 q s M frames touches at most that
// many slices, so live entries never share a slot.  Likewise the live video frames [s w, f2) of a call are fewer than
// F + 2 s M = RVf, the slots of the video frame ring.
#pragma once
#include <algorithm>
#include <cstdint>

#include "stream_geom.h"

namespace avse {

constexpr int SLIDE_GATHER_X = 4;      // blocks per gathered window (k_slide_gather)
constexpr int SLIDE_MAX_WINDOWS = 80;  // avse_slide_create's bound on max_windows

struct SlideCfg {
    int n_fft, hop, spf, F, stride;
    int64_t max_windows;
    int q() const { return spf / F; }
    int qs() const { return spf / F * stride; }
    int RS() const { return (int)((spf + 2 * (int64_t)qs() * max_windows + spf - 1) / spf + 1); }
    int R() const { return RS() * spf; }
    int RVf() const { return (int)(F + 2 * (int64_t)stride * max_windows); }
};

struct SlideCounts {
    int64_t frames, wa, wv, windows, predicted, emitted;
};
inline SlideCounts slide_totals(const SlideCfg& g, int64_t n, int64_t f, bool flushed) {
    SlideCounts c;
    const int64_t qs = g.qs();
    c.frames = flushed ? (int64_t)g.q() * f : (n < g.n_fft / 2 + 1 ? 0 : (n - g.n_fft / 2) / g.hop + 1);
    c.wa = c.frames >= g.spf ? (c.frames - g.spf) / qs + 1 : 0;
    c.wv = f >= g.F ? (f - g.F) / g.stride + 1 : 0;
    c.windows = std::min(c.wa, c.wv);
    c.predicted = c.windows > 0 ? g.spf + qs * (c.windows - 1) : 0;
    c.emitted = flushed ? (c.predicted > 0 ? (int64_t)g.hop * (c.predicted - 1) : 0)
                        : std::max<int64_t>(0, (int64_t)g.hop * c.predicted - g.n_fft / 2);
    return c;
}

// What the session keeps per stream between calls.
struct SlideState {
    int64_t n, f;        // samples and video frames received
    uint8_t flushed;
    uint8_t parity;      // which tail copy holds the stream's last samples
};

// One stream's part of one call, for the kernels that are new in K21 (the StreamRow beside it serves k_stream_spec and
// k_stream_ola).
struct SlideRow {
    int64_t w_old;       // windows through the network before this call
    int64_t f_old;       // video frames received before this call
    int64_t video_off;   // first frame of this call's video in the packed `video` (prefix sum of f_new)
    int64_t T0;          // frames inverted before this call (predicted, before)
    int64_t app0;        // first video frame this call appends to the frame ring: frames [app0, f_old + f_new)
    int32_t w_new;       // windows this call completes
    int32_t f_new;       // video frames this call brings
    int32_t clip0;       // the stream's first clip in the forward batch (exclusive prefix sum of w_new)
    int32_t nt;          // frames inverted by this call
    int32_t n_app;       // video frames appended
    int32_t pad;
};
static_assert(sizeof(SlideRow) == 64, "device row layout");

enum SlideStatus {
    SLIDE_OK = 0,
    SLIDE_BAD_COUNT,       // a negative n_new / f_new
    SLIDE_TOO_LARGE,       // totals past 2^40 samples / 2^30 frames
    SLIDE_AFTER_FLUSH,     // input or a second flush for a flushed stream
    SLIDE_FLUSH_SHORT,     // flush with n > H q f
    SLIDE_TOO_MANY,        // more than max_windows windows completed
    SLIDE_SAMPLES_AHEAD,   // the samples complete more than max_windows windows the video does not
    SLIDE_VIDEO_AHEAD,     // the video completes more than max_windows windows the samples do not
    SLIDE_OUT_SMALL,       // out NULL or out_stride below what the stream emits
    SLIDE_CAPACITY,        // the item tables sized at create would not hold the call (never, by slide_item_caps)
};

inline const char* slide_message(int status) {
    switch (status) {
        case SLIDE_BAD_COUNT: return "negative counts";
        case SLIDE_TOO_LARGE: return "counts too large";
        case SLIDE_AFTER_FLUSH: return "pushed or flushed after its flush: only a reset is legal";
        case SLIDE_FLUSH_SHORT: return "flush: more samples than the video frames cover (n > hop * q * f)";
        case SLIDE_TOO_MANY: return "the call would complete more than max_windows windows";
        case SLIDE_SAMPLES_AHEAD: return "the samples are more than max_windows strides ahead of the video";
        case SLIDE_VIDEO_AHEAD: return "the video is more than max_windows strides ahead of the samples";
        case SLIDE_OUT_SMALL: return "out is NULL or out_stride below what the call emits";
        case SLIDE_CAPACITY: return "the call passes the item tables sized at create";
        default: return "ok";
    }
}

struct SlideItemCounts {
    int64_t spec = 0, route = 0, gather = 0, synth = 0, ola = 0;
    int64_t total() const { return spec + route + gather + synth + ola; }
};

struct SlidePlan {
    int status = SLIDE_OK;
    int64_t bad = -1;          // the first stream `status` refers to
    int64_t clips = 0;         // sum of w_new: the forward's batch
    int64_t video_total = 0;   // sum of f_new
    int64_t max_n_out = 0;
    bool any = false;          // any stream has work
    SlideItemCounts items;
};

// The most items one stream can put into each table: a legal call analyses fewer than spf + (2 M + 1) q s frames (from
// the last frame of window w - 1 to frame spf + q s (w + 2 M) - 1), completes M windows, appends fewer than F + 2 s M
// video frames, inverts at most spf + q s (M - 1) frames and emits at most H of them plus N/2 - H samples (a flush).
inline SlideItemCounts slide_item_caps(const SlideCfg& g) {
    const int64_t M = g.max_windows, qs = g.qs();
    SlideItemCounts c;
    c.spec = (g.spf + (2 * M + 1) * qs + STREAM_SCHUNK - 1) / STREAM_SCHUNK + 1;
    c.route = 1;
    c.gather = SLIDE_GATHER_X * M + g.RVf();
    c.synth = (g.spf + qs * (M - 1) + STREAM_SYNTH_FPG - 1) / STREAM_SYNTH_FPG;
    c.ola = ((int64_t)g.hop * (g.spf + qs * (M - 1)) + g.n_fft / 2 + STREAM_OLA_BLOCK - 1) / STREAM_OLA_BLOCK;
    return c;
}

// item counts of one stream's rows
inline SlideItemCounts slide_row_items(const StreamRow& r, const SlideRow& x) {
    SlideItemCounts c;
    const bool fed = r.n_new > r.n_old;
    c.spec = (fed || r.nt > 0) ? r.nblk + (fed ? 1 : 0) : 0;
    c.route = x.w_new > 0 ? 1 : 0;
    c.gather = (int64_t)SLIDE_GATHER_X * x.w_new + x.n_app;
    c.synth = ((int64_t)x.nt + STREAM_SYNTH_FPG - 1) / STREAM_SYNTH_FPG;
    c.ola = ((int64_t)r.n_out + STREAM_OLA_BLOCK - 1) / STREAM_OLA_BLOCK;
    return c;
}

// The refusal decision and the rows of a call.  flush and sample_off may be NULL; have_out says whether the caller gave
// an `out`.  On a refusal the rows hold nothing to rely on; `st` is never written (slide_commit does that once the
// launches are in).  Of `rows` only the fields k_stream_spec and k_stream_ola read are meaningful.
inline SlidePlan slide_rows(const SlideCfg& g, const SlideState* st, int64_t B, const int64_t* sample_off,
                            const int64_t* n_new, const int64_t* f_new, const uint8_t* flush, bool have_out,
                            int64_t out_stride, StreamRow* rows, SlideRow* xrows) {
    SlidePlan p;
    const int64_t M = g.max_windows;
    const SlideItemCounts cap = slide_item_caps(g);
    auto refuse = [&](int status, int64_t b) {
        p.status = status;
        p.bad = b;
        return p;
    };
    for (int64_t b = 0; b < B; ++b) {
        const SlideState& s = st[b];
        const int64_t dn = n_new[b], df = f_new[b];
        const bool fl = flush && flush[b];
        if (dn < 0 || df < 0) return refuse(SLIDE_BAD_COUNT, b);
        if (dn > (1LL << 40) - s.n || df > (1LL << 30) - s.f) return refuse(SLIDE_TOO_LARGE, b);
        if (s.flushed && (dn > 0 || df > 0 || fl)) return refuse(SLIDE_AFTER_FLUSH, b);
        const SlideCounts c0 = slide_totals(g, s.n, s.f, s.flushed);
        const int64_t n2 = s.n + dn, f2 = s.f + df;
        const bool closed = s.flushed || fl;
        const int64_t Lf = (int64_t)g.hop * g.q() * f2;
        if (fl && n2 > Lf) return refuse(SLIDE_FLUSH_SHORT, b);
        const SlideCounts c1 = slide_totals(g, n2, f2, closed);
        const int64_t w_new = c1.windows - c0.windows, n_out = c1.emitted - c0.emitted;
        if (w_new > M) return refuse(SLIDE_TOO_MANY, b);
        if (c1.wa - c1.windows > M) return refuse(SLIDE_SAMPLES_AHEAD, b);
        if (c1.wv - c1.windows > M) return refuse(SLIDE_VIDEO_AHEAD, b);
        if (n_out > 0 && (!have_out || out_stride < n_out)) return refuse(SLIDE_OUT_SMALL, b);
        StreamRow& r = rows[b];
        r = StreamRow{};
        r.n_old = s.n;
        r.n_new = n2;
        r.Lf = fl ? Lf : -1;
        r.t0 = c0.frames;
        r.e_old = c0.emitted;
        r.T = c1.predicted;
        r.sample_off = sample_off && dn > 0 ? sample_off[b] : 0;
        const int64_t nt = c1.frames - c0.frames;
        r.nt = (int32_t)nt;
        r.nblk = (int32_t)((nt + STREAM_SCHUNK - 1) / STREAM_SCHUNK);
        r.n_out = (int32_t)n_out;
        r.tail_in = s.parity;
        r.tail_out = s.parity ^ (dn > 0 ? 1 : 0);
        r.flush = fl ? 1 : 0;
        SlideRow& x = xrows[b];
        x = SlideRow{};
        x.w_old = c0.windows;
        x.f_old = s.f;
        x.video_off = p.video_total;
        x.T0 = c0.predicted;
        x.w_new = (int32_t)w_new;
        x.f_new = (int32_t)df;
        x.clip0 = (int32_t)p.clips;
        x.nt = (int32_t)(c1.predicted - c0.predicted);
        // of the call's frames the ring takes those a later window reads: from frame s * windows on
        x.app0 = std::max<int64_t>(s.f, (int64_t)g.stride * c1.windows);
        x.n_app = (int32_t)std::max<int64_t>(0, f2 - x.app0);
        const SlideItemCounts c = slide_row_items(r, x);
        if (c.spec > cap.spec || c.route > cap.route || c.gather > cap.gather || c.synth > cap.synth || c.ola > cap.ola)
            return refuse(SLIDE_CAPACITY, b);
        p.items.spec += c.spec;
        p.items.route += c.route;
        p.items.gather += c.gather;
        p.items.synth += c.synth;
        p.items.ola += c.ola;
        p.clips += w_new;
        p.video_total += df;
        p.max_n_out = std::max(p.max_n_out, n_out);
        p.any = p.any || dn > 0 || df > 0 || fl;
    }
    return p;
}

// The item tables of the rows, stream-major; each array holds at least the plan's count for it.  A gather item's chunk
// is part chunk % SLIDE_GATHER_X of the stream's window w_old + chunk / SLIDE_GATHER_X, or (negative) -1 - i for the
// append of video frame app0 + i.
inline void slide_fill_items(const StreamRow* rows, const SlideRow* xrows, int64_t B, StreamItem* spec, StreamItem* route,
                             StreamItem* gather, StreamItem* synth, StreamItem* ola) {
    for (int64_t b = 0; b < B; ++b) {
        const SlideItemCounts c = slide_row_items(rows[b], xrows[b]);
        const int32_t sb = (int32_t)b;
        for (int32_t i = 0; i < c.spec; ++i) *spec++ = {sb, i};
        if (c.route) *route++ = {sb, STREAM_CLAMP};
        for (int32_t i = 0; i < SLIDE_GATHER_X * xrows[b].w_new; ++i) *gather++ = {sb, i};
        for (int32_t i = 0; i < xrows[b].n_app; ++i) *gather++ = {sb, -1 - i};
        for (int32_t i = 0; i < c.synth; ++i) *synth++ = {sb, i};
        for (int32_t i = 0; i < c.ola; ++i) *ola++ = {sb, i};
    }
}

// The states after the call the rows describe.
inline void slide_commit(const StreamRow* rows, const SlideRow* xrows, int64_t B, SlideState* st) {
    for (int64_t b = 0; b < B; ++b) {
        st[b].n = rows[b].n_new;
        st[b].f = xrows[b].f_old + xrows[b].f_new;
        st[b].flushed = st[b].flushed || rows[b].flush;
        st[b].parity = (uint8_t)rows[b].tail_out;
    }
}

}  // namespace avse
