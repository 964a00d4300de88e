// Host-only geometry of a streaming session (no HIP header): the totals of one stream (stream_totals, shared by the
// lock-step and the per-stream calls), and for a per-stream push (include/avse.h avse_stream_push_each) the refusal
// decision, one row per stream and one item table per kernel, block -> (stream, chunk).  StreamRow / StreamItem are
// also the device-side layouts (stream.hip uploads them and the EACH instances of its kernels read them).  Nothing here
// allocates: the caller owns every array (the session sizes them at create from stream_item_caps).
#pragma once
#include <algorithm>
#include <cstdint>

namespace avse {

constexpr int STREAM_SCHUNK = 21;      // frames per analysis block (k_stream_spec)
constexpr int STREAM_ROUTE_X = 8;      // blocks per moved video slice (k_stream_route)
constexpr int STREAM_SYNTH_FPG = 3;    // frames per synthesis block (istft640::FPG)
constexpr int STREAM_OLA_BLOCK = 256;  // samples per overlap-add block
constexpr int STREAM_CLAMP = -1;       // chunk of a route item that is its stream's clamp block

struct StreamCfg {
    int n_fft, hop, spf;
    int64_t max_slices;
};

// the totals after n samples and v video slices
struct StreamCounts {
    int64_t frames, slices, emitted;
};
inline StreamCounts stream_totals(int n_fft, int hop, int spf, int64_t n, int64_t v, bool flushed) {
    StreamCounts c;
    if (flushed) {
        c.frames = spf * v;
        c.slices = v;
        c.emitted = v > 0 ? (int64_t)hop * (spf * v - 1) : 0;
        return c;
    }
    c.frames = n < n_fft / 2 + 1 ? 0 : (n - n_fft / 2) / hop + 1;   // frame 0 reads x[n_fft / 2] (left reflection)
    c.slices = std::min(c.frames / spf, v);
    c.emitted = std::max<int64_t>(0, (int64_t)spf * hop * c.slices - n_fft / 2);
    return c;
}

// What the session keeps per stream between calls.
struct StreamState {
    int64_t n, v;        // samples and video slices received
    uint8_t flushed;
    uint8_t parity;      // which tail copy holds the stream's last samples
};

// One stream's part of one call.  n_old / n_new are totals (before / after), v_new and k_new are this call's counts: the
// naming of the lock-step kernels' argument structs, whose per-call scalars these are.
struct StreamRow {
    int64_t n_old, n_new;   // samples received before / after this call
    int64_t Lf;             // flush: length of the closed signal; else -1
    int64_t t0;             // frames [t0, t0 + nt) are analysed
    int64_t k_old;          // slices through the network before this call
    int64_t v_old;          // video slices received before this call
    int64_t e_old;          // samples emitted before this call
    int64_t T;              // frames inverted once this call is done
    int64_t sample_off;     // first float of this call's samples in `samples` (the caller's sample_off)
    int64_t video_off;      // first slice of this call's video in the packed `video` (prefix sum of v_new)
    int32_t nt, nblk;       // frames analysed; analysis chunks (chunk nblk, when listed, writes the tail)
    int32_t k_new;          // slices this call completes
    int32_t v_new;          // video slices this call brings
    int32_t nv;             // video slices not yet consumed, this call's included
    int32_t n_out;          // samples this call emits
    int32_t clip0;          // the stream's first clip in the forward batch (exclusive prefix sum of k_new)
    int32_t tail_in, tail_out;   // the tail copy read / the one holding the last samples afterwards
    int32_t flush;          // the stream is closed by this call
};
static_assert(sizeof(StreamRow) == 120, "device row layout");

struct StreamItem {      // one block's work: chunk `chunk` of stream `b`
    int32_t b, chunk;
};

enum StreamStatus {
    STREAM_OK = 0,
    STREAM_BAD_COUNT,       // a negative n_new / v_new
    STREAM_TOO_LARGE,       // totals past 2^40 samples / 2^30 slices
    STREAM_AFTER_FLUSH,     // input or a second flush for a flushed stream
    STREAM_FLUSH_SHORT,     // flush with n > slice * v
    STREAM_TOO_MANY,        // more than max_slices slices completed
    STREAM_SAMPLES_AHEAD,   // more than max_slices slices of samples queued ahead of the video
    STREAM_VIDEO_AHEAD,     // more than max_slices video slices queued ahead of the samples
    STREAM_OUT_SMALL,       // out NULL or out_stride below what the stream emits
    STREAM_CAPACITY,        // the item tables sized at create would not hold the call (never, by stream_item_caps)
};

inline const char* stream_message(int status) {
    switch (status) {
        case STREAM_BAD_COUNT: return "negative counts";
        case STREAM_TOO_LARGE: return "counts too large";
        case STREAM_AFTER_FLUSH: return "pushed or flushed after its flush: only a reset is legal";
        case STREAM_FLUSH_SHORT: return "flush: more samples than the video slices cover (n > slice * v)";
        case STREAM_TOO_MANY: return "the call would complete more than max_slices slices";
        case STREAM_SAMPLES_AHEAD: return "more than max_slices slices of samples queued ahead of the video";
        case STREAM_VIDEO_AHEAD: return "more than max_slices video slices queued ahead of the samples";
        case STREAM_OUT_SMALL: return "out is NULL or out_stride below what the call emits";
        case STREAM_CAPACITY: return "the call passes the item tables sized at create";
        default: return "ok";
    }
}

struct StreamItemCounts {
    int64_t spec = 0, route = 0, synth = 0, ola = 0;
    int64_t total() const { return spec + route + synth + ola; }
};

struct StreamPlan {
    int status = STREAM_OK;
    int64_t bad = -1;          // the first stream `status` refers to
    int64_t clips = 0;         // sum of k_new: the forward's batch
    int64_t video_total = 0;   // sum of v_new
    int64_t max_n_out = 0;
    bool any = false;          // any stream has work
    StreamItemCounts items;
};

// The most items one stream can put into each table, for a session's max_slices: with M = max_slices, a legal call
// analyses at most spf (2 M + 1) frames of a stream (its frames and its video each within M slices of the other before
// and after, at most M slices completed), moves at most 2 M video slices, inverts M slices and emits at most
// spf hop M + n_fft / 2 - hop samples (a flush).
inline StreamItemCounts stream_item_caps(const StreamCfg& g) {
    const int64_t M = g.max_slices;
    StreamItemCounts c;
    c.spec = ((int64_t)g.spf * (2 * M + 1) + STREAM_SCHUNK - 1) / STREAM_SCHUNK + 1;
    c.route = STREAM_ROUTE_X * 2 * M + 1;
    c.synth = ((int64_t)g.spf * M + STREAM_SYNTH_FPG - 1) / STREAM_SYNTH_FPG;
    c.ola = ((int64_t)g.spf * g.hop * M + g.n_fft / 2 + STREAM_OLA_BLOCK - 1) / STREAM_OLA_BLOCK;
    return c;
}

// item counts of one row
inline StreamItemCounts stream_row_items(const StreamCfg& g, const StreamRow& r) {
    StreamItemCounts c;
    const bool fed = r.n_new > r.n_old;
    c.spec = (fed || r.nt > 0) ? r.nblk + (fed ? 1 : 0) : 0;
    // slices in flight kk = k - k_old in [0, nv): from the queue while k < v_old, to the network while kk < k_new; one
    // that is queued and stays queued does not move
    const int64_t stay_lo = r.k_new, stay_hi = std::max<int64_t>(r.k_new, r.v_old - r.k_old);
    c.route = STREAM_ROUTE_X * (r.nv - (stay_hi - stay_lo)) + (r.k_new > 0 ? 1 : 0);
    c.synth = ((int64_t)r.k_new * g.spf + STREAM_SYNTH_FPG - 1) / STREAM_SYNTH_FPG;
    c.ola = ((int64_t)r.n_out + STREAM_OLA_BLOCK - 1) / STREAM_OLA_BLOCK;
    return c;
}

// The refusal decision and the rows of a call.  flush and sample_off may be NULL (no stream flushed; offsets 0, for a
// call without samples); have_out says whether the caller gave an `out`.  On a refusal `rows` holds nothing to rely on;
// `st` is never written (stream_commit does that once the launches are in).
inline StreamPlan stream_rows(const StreamCfg& g, const StreamState* st, int64_t B, const int64_t* sample_off,
                              const int64_t* n_new, const int64_t* v_new, const uint8_t* flush, bool have_out,
                              int64_t out_stride, StreamRow* rows) {
    StreamPlan p;
    const int64_t slice = (int64_t)g.spf * g.hop, M = g.max_slices;
    const StreamItemCounts cap = stream_item_caps(g);
    auto refuse = [&](int status, int64_t b) {
        p.status = status;
        p.bad = b;
        return p;
    };
    for (int64_t b = 0; b < B; ++b) {
        const StreamState& s = st[b];
        const int64_t dn = n_new[b], dv = v_new[b];
        const bool fl = flush && flush[b];
        if (dn < 0 || dv < 0) return refuse(STREAM_BAD_COUNT, b);
        if (dn > (1LL << 40) - s.n || dv > (1LL << 30) - s.v) return refuse(STREAM_TOO_LARGE, b);
        if (s.flushed && (dn > 0 || dv > 0 || fl)) return refuse(STREAM_AFTER_FLUSH, b);
        const StreamCounts c0 = stream_totals(g.n_fft, g.hop, g.spf, s.n, s.v, s.flushed);
        const int64_t n2 = s.n + dn, v2 = s.v + dv;
        const bool closed = s.flushed || fl;
        if (fl && n2 > slice * v2) return refuse(STREAM_FLUSH_SHORT, b);
        const StreamCounts c1 = stream_totals(g.n_fft, g.hop, g.spf, n2, v2, closed);
        const int64_t k_new = c1.slices - c0.slices, n_out = c1.emitted - c0.emitted;
        if (k_new > M) return refuse(STREAM_TOO_MANY, b);
        if (n2 - slice * v2 > slice * M) return refuse(STREAM_SAMPLES_AHEAD, b);
        if (v2 - c1.frames / g.spf > M) return refuse(STREAM_VIDEO_AHEAD, b);
        if (n_out > 0 && (!have_out || out_stride < n_out)) return refuse(STREAM_OUT_SMALL, b);
        StreamRow& r = rows[b];
        r.n_old = s.n;
        r.n_new = n2;
        r.Lf = fl ? slice * v2 : -1;
        r.t0 = c0.frames;
        r.k_old = c0.slices;
        r.v_old = s.v;
        r.e_old = c0.emitted;
        r.T = c1.slices * g.spf;
        r.sample_off = sample_off && dn > 0 ? sample_off[b] : 0;
        r.video_off = p.video_total;
        const int64_t nt = c1.frames - c0.frames;
        r.nt = (int32_t)nt;
        r.nblk = (int32_t)((nt + STREAM_SCHUNK - 1) / STREAM_SCHUNK);
        r.k_new = (int32_t)k_new;
        r.v_new = (int32_t)dv;
        r.nv = (int32_t)(v2 - c0.slices);
        r.n_out = (int32_t)n_out;
        r.clip0 = (int32_t)p.clips;
        r.tail_in = s.parity;
        r.tail_out = s.parity ^ (dn > 0 ? 1 : 0);
        r.flush = fl ? 1 : 0;
        const StreamItemCounts c = stream_row_items(g, r);
        if (c.spec > cap.spec || c.route > cap.route || c.synth > cap.synth || c.ola > cap.ola)
            return refuse(STREAM_CAPACITY, b);
        p.items.spec += c.spec;
        p.items.route += c.route;
        p.items.synth += c.synth;
        p.items.ola += c.ola;
        p.clips += k_new;
        p.video_total += dv;
        p.max_n_out = std::max(p.max_n_out, n_out);
        p.any = p.any || dn > 0 || dv > 0 || fl;
    }
    return p;
}

// The item tables of the rows, stream-major; each array holds at least the plan's count for it.
inline void stream_fill_items(const StreamCfg& g, const StreamRow* rows, int64_t B, StreamItem* spec, StreamItem* route,
                              StreamItem* synth, StreamItem* ola) {
    for (int64_t b = 0; b < B; ++b) {
        const StreamRow& r = rows[b];
        const StreamItemCounts c = stream_row_items(g, r);
        const int32_t sb = (int32_t)b;
        for (int32_t i = 0; i < c.spec; ++i) *spec++ = {sb, i};   // chunks 0 .. nblk - 1, then the tail block (nblk)
        const int64_t stay_lo = r.k_new, stay_hi = std::max<int64_t>(r.k_new, r.v_old - r.k_old);
        for (int32_t kk = 0; kk < r.nv; ++kk) {
            if (kk >= stay_lo && kk < stay_hi) continue;
            for (int32_t part = 0; part < STREAM_ROUTE_X; ++part) *route++ = {sb, kk * STREAM_ROUTE_X + part};
        }
        if (r.k_new > 0) *route++ = {sb, STREAM_CLAMP};
        for (int32_t i = 0; i < c.synth; ++i) *synth++ = {sb, i};
        for (int32_t i = 0; i < c.ola; ++i) *ola++ = {sb, i};
    }
}

// The states after the call the rows describe.
inline void stream_commit(const StreamRow* rows, int64_t B, StreamState* st) {
    for (int64_t b = 0; b < B; ++b) {
        st[b].n = rows[b].n_new;
        st[b].v = rows[b].v_old + rows[b].v_new;
        st[b].flushed = st[b].flushed || rows[b].flush;
        st[b].parity = (uint8_t)rows[b].tail_out;
    }
}

}  // namespace avse
