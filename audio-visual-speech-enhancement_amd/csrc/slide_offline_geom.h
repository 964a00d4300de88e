// Host-only geometry of the offline sliding path (K22, include/avse.h avse_slide_windows / avse_slide_video_windows /
// avse_slide_keep; no HIP header): whole utterances through the windows of a flushed sliding session (slide_geom.h)
// in ragged batches.  The totals of an utterance are slide_totals' (one definition), here with their prefix sums over
// the batch, the refusals, one row per utterance and the block -> (utterance, chunk) item tables of slide_offline.hip.
// SlideOffRow / SlideOffVidRow are also the device-side rows.  Nothing here allocates: the caller owns every array.
//
// With spf frames and F video frames per slice, q = spf / F and the stride s (1 <= s <= F), an utterance of S slices
// (f = F S video frames, T >= q f frames of unclamped mel-dB) has
//   W = S > 0 ? (f - F) / s + 1 : 0         windows; window j is frames [q s j, q s j + spf), video frames [s j, s j + F)
//   P = W > 0 ? spf + q s (W - 1) : 0       kept columns: all spf of window 0, the last q s of each later window
// Video frame s j + i of an utterance is element i' = (s j + i) % F of its slice (s j + i) / F; kept column t comes from
// window j = t < spf ? 0 : (t - spf) / (q s) + 1, column t - q s j.
#pragma once
#include <cstdint>

#include "slide_geom.h"

namespace avse {

constexpr int SLIDE_OFF_SCAN = 256;    // frames per scan chunk of k_slide_off_scan (one block per utterance, a carry between chunks)
constexpr int SLIDE_OFF_WPB = 4;       // windows per block of k_slide_off_windows
constexpr int SLIDE_OFF_KEEP = 256;    // kept columns per block of k_slide_off_keep
constexpr int SLIDE_OFF_VX = 4;        // blocks per gathered video window (k_slide_off_video)

struct SlideOffCfg {
    int spf, F, stride;
    int q() const { return spf / F; }
    int qs() const { return spf / F * stride; }
};

enum SlideOffStatus {
    SLIDE_OFF_OK = 0,
    SLIDE_OFF_BAD_GEOM,      // spf < 1, F < 1 or spf % F != 0
    SLIDE_OFF_BAD_STRIDE,    // a stride outside 1 .. F
    SLIDE_OFF_BAD_COUNT,     // n_utt < 0, a negative S_u or T_u
    SLIDE_OFF_SHORT,         // T_u < q F S_u: the mel block does not hold the frames the windows read
    SLIDE_OFF_TOO_LARGE,     // an utterance or an item table past int32
    SLIDE_OFF_BAD_RANGE,     // a window range outside [0, sum W_u]
};

inline const char* slide_off_message(int status) {
    switch (status) {
        case SLIDE_OFF_BAD_GEOM: return "frames_per_slice must be a positive multiple of a positive video_frames";
        case SLIDE_OFF_BAD_STRIDE: return "the stride must be 1 .. video_frames";
        case SLIDE_OFF_BAD_COUNT: return "negative counts";
        case SLIDE_OFF_SHORT: return "n_frames is below the frames its slices' windows read (q * video_frames * n_slices)";
        case SLIDE_OFF_TOO_LARGE: return "batch too large (an utterance or an item table passes int32)";
        case SLIDE_OFF_BAD_RANGE: return "the window range lies outside the batch's windows";
        default: return "ok";
    }
}

// (W, P) of an utterance of S >= 0 slices: the flushed stream's totals
inline void slide_off_counts(const SlideOffCfg& g, int64_t S, int64_t* W, int64_t* P) {
    const SlideCfg c{2, 1, g.spf, g.F, g.stride, 1};
    const SlideCounts t = slide_totals(c, 0, (int64_t)g.F * S, true);
    *W = t.windows;
    *P = t.predicted;
}

struct SlideOffRow {     // one utterance
    int64_t t_off;       // frames before it in the batch: its mel block starts at float n_mels t_off, its prefix maxima at t_off
    int64_t w_off;       // windows before it: its first window of net_in / pred
    int64_t p_off;       // kept columns before it: its packed output starts at float n_mels p_off
    int64_t s_off;       // slices before it: its first video slice
    int32_t T, W, P, S;
    int32_t pad[4];
};
static_assert(sizeof(SlideOffRow) == 64, "device row layout");

struct SlideOffVidRow {  // one utterance's part of a window range
    int64_t s_off;       // its first video slice
    int64_t j0;          // its first window in the range, counted within the utterance
    int64_t out0;        // that window's index in the range's output
    int32_t n;           // windows of it in the range
    int32_t pad;
};
static_assert(sizeof(SlideOffVidRow) == 32, "device row layout");

struct SlideOffItems {
    int64_t scan = 0, windows = 0, keep = 0;
};

struct SlideOffPlan {
    int status = SLIDE_OFF_OK;
    int64_t bad = -1;                   // the utterance `status` refers to (-1: the call's own arguments)
    int64_t frames = 0, windows = 0, predicted = 0, slices = 0;      // sums over the batch
    SlideOffItems items;
};

inline int slide_off_check_cfg(const SlideOffCfg& g) {
    if (g.spf < 1 || g.F < 1 || g.spf % g.F) return SLIDE_OFF_BAD_GEOM;
    if (g.stride < 1 || g.stride > g.F) return SLIDE_OFF_BAD_STRIDE;
    return SLIDE_OFF_OK;
}

inline SlideOffItems slide_off_row_items(const SlideOffRow& r) {
    SlideOffItems c;
    c.scan = r.W > 0 ? 1 : 0;
    c.windows = ((int64_t)r.W + SLIDE_OFF_WPB - 1) / SLIDE_OFF_WPB;
    c.keep = ((int64_t)r.P + SLIDE_OFF_KEEP - 1) / SLIDE_OFF_KEEP;
    return c;
}

// The refusal decision, the totals and (rows != NULL) the rows of a batch.  n_frames == NULL: T_u = q F S_u (where only
// windows, kept columns and slices matter).  The prefix sums are the rows' *_off; the plan holds the sums.
inline SlideOffPlan slide_off_plan(const SlideOffCfg& g, const int64_t* n_slices, const int64_t* n_frames, int64_t n_utt,
                                   int n_mels, SlideOffRow* rows) {
    SlideOffPlan p;
    p.status = slide_off_check_cfg(g);
    if (p.status != SLIDE_OFF_OK) return p;
    if (n_utt < 0 || n_mels < 1) {
        p.status = SLIDE_OFF_BAD_COUNT;
        return p;
    }
    auto refuse = [&](int status, int64_t u) {
        p.status = status;
        p.bad = u;
        return p;
    };
    if (n_utt > INT32_MAX) return refuse(SLIDE_OFF_TOO_LARGE, -1);
    const int64_t per_slice = (int64_t)g.q() * g.F;
    for (int64_t u = 0; u < n_utt; ++u) {
        const int64_t S = n_slices[u];
        if (S < 0 || (n_frames && n_frames[u] < 0)) return refuse(SLIDE_OFF_BAD_COUNT, u);
        if (S > INT32_MAX / (per_slice * n_mels)) return refuse(SLIDE_OFF_TOO_LARGE, u);      // n_mels T and F S fit int32
        const int64_t T = n_frames ? n_frames[u] : per_slice * S;
        if (T < per_slice * S) return refuse(SLIDE_OFF_SHORT, u);
        if (T > INT32_MAX / n_mels) return refuse(SLIDE_OFF_TOO_LARGE, u);
        int64_t W, P;
        slide_off_counts(g, S, &W, &P);
        SlideOffRow r{};
        r.t_off = p.frames;
        r.w_off = p.windows;
        r.p_off = p.predicted;
        r.s_off = p.slices;
        r.T = (int32_t)T;
        r.W = (int32_t)W;
        r.P = (int32_t)P;
        r.S = (int32_t)S;
        const SlideOffItems c = slide_off_row_items(r);
        p.frames += T;
        p.windows += W;
        p.predicted += P;
        p.slices += S;
        p.items.scan += c.scan;
        p.items.windows += c.windows;
        p.items.keep += c.keep;
        // the window list is indexed in int32 by the video gather's items (SLIDE_OFF_VX per window)
        if (p.windows > INT32_MAX / SLIDE_OFF_VX || p.items.keep > INT32_MAX) return refuse(SLIDE_OFF_TOO_LARGE, u);
        if (rows) rows[u] = r;
    }
    return p;
}

// The item tables of the rows, utterance-major; each array (nullable) holds at least the plan's count for it.  A scan
// item is an utterance (chunk 0: the block walks its chunks itself, carrying the maximum); a windows item is windows
// [WPB chunk, WPB chunk + WPB) of the utterance; a keep item its kept columns [KEEP chunk, KEEP chunk + KEEP).
inline void slide_off_fill_items(const SlideOffRow* rows, int64_t n_utt, StreamItem* scan, StreamItem* windows,
                                 StreamItem* keep) {
    for (int64_t u = 0; u < n_utt; ++u) {
        const SlideOffItems c = slide_off_row_items(rows[u]);
        const int32_t ub = (int32_t)u;
        if (scan && c.scan) *scan++ = {ub, 0};
        if (windows)
            for (int32_t i = 0; i < c.windows; ++i) *windows++ = {ub, i};
        if (keep)
            for (int32_t i = 0; i < c.keep; ++i) *keep++ = {ub, i};
    }
}

struct SlideOffVidPlan {
    int status = SLIDE_OFF_OK;
    int64_t bad = -1;
    int64_t rows = 0;        // utterances with a window in the range
    int64_t items = 0;       // SLIDE_OFF_VX n
    int64_t slices = 0;      // slices of the whole batch
};

// The video gather of windows [w0, w0 + n) of the batch's concatenated window list: one row per utterance with a
// window in the range (vrows nullable: the counts alone; else room for min(n_utt, n) rows).
inline SlideOffVidPlan slide_off_video_plan(const SlideOffCfg& g, const int64_t* n_slices, int64_t n_utt, int64_t w0, int64_t n,
                                            SlideOffVidRow* vrows) {
    SlideOffVidPlan v;
    const SlideOffPlan p = slide_off_plan(g, n_slices, nullptr, n_utt, 1, nullptr);
    v.status = p.status;
    v.bad = p.bad;
    if (v.status != SLIDE_OFF_OK) return v;
    if (w0 < 0 || n < 0 || w0 > p.windows || n > p.windows - w0) {
        v.status = SLIDE_OFF_BAD_RANGE;
        return v;
    }
    v.slices = p.slices;
    v.items = (int64_t)SLIDE_OFF_VX * n;
    int64_t w_off = 0, s_off = 0;
    for (int64_t u = 0; u < n_utt && w_off < w0 + n; ++u) {
        int64_t W, P;
        slide_off_counts(g, n_slices[u], &W, &P);
        const int64_t a = std::max(w_off, w0), b = std::min(w_off + W, w0 + n);
        if (b > a) {
            if (vrows) {
                SlideOffVidRow r{};
                r.s_off = s_off;
                r.j0 = a - w_off;
                r.out0 = a - w0;
                r.n = (int32_t)(b - a);
                vrows[v.rows] = r;
            }
            ++v.rows;
        }
        w_off += W;
        s_off += n_slices[u];
    }
    return v;
}

// A video item is part chunk % VX of window j0 + chunk / VX of row b.
inline void slide_off_video_items(const SlideOffVidRow* vrows, int64_t n_rows, StreamItem* items) {
    for (int64_t b = 0; b < n_rows; ++b)
        for (int32_t i = 0; i < SLIDE_OFF_VX * vrows[b].n; ++i) *items++ = {(int32_t)b, i};
}

}  // namespace avse
