// Stand-alone check of csrc/slide_geom.h (built with -fsanitize=address,undefined by tests/test_slide_host.py): random
// per-stream schedules, legal and illegal, are played through slide_rows / slide_fill_items / slide_commit, and every
// call is compared with a brute-force definition that counts frames, windows and kept columns one by one and keeps a
// model of every ring's slots: an entry that a window, the synthesis or the overlap-add reads must still be the one in
// its slot.  Prints "ok <n checks>" and exits 0, or the first mismatch and exits 1.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "slide_geom.h"

using namespace avse;

static long checks = 0;
static long seen_status[SLIDE_CAPACITY + 1] = {};
#define EXPECT(cond, ...)                          \
    do {                                           \
        ++checks;                                  \
        if (!(cond)) {                             \
            std::printf("FAILED %s: ", #cond);     \
            std::printf(__VA_ARGS__);              \
            std::printf("\n");                     \
            std::exit(1);                          \
        }                                          \
    } while (0)

// ---- the definition, by counting (include/avse.h, "low-latency streaming") ----
struct Totals {
    int64_t frames, wa, wv, windows, predicted, emitted;
};
static Totals brute(const SlideCfg& g, int64_t n, int64_t f, bool flushed) {
    const int N = g.n_fft, H = g.hop, q = g.spf / g.F, s = g.stride;
    Totals t{0, 0, 0, 0, 0, 0};
    if (flushed) t.frames = (int64_t)q * f;
    else
        while ((t.frames == 0 ? n >= N / 2 + 1 : n >= H * t.frames + N / 2)) ++t.frames;
    while ((int64_t)q * s * t.wa + g.spf <= t.frames) ++t.wa;     // window j needs frames [q s j, q s j + spf)
    while ((int64_t)s * t.wv + g.F <= f) ++t.wv;                  // and video frames [s j, s j + F)
    t.windows = t.wa < t.wv ? t.wa : t.wv;
    for (int64_t j = 0; j < t.windows; ++j) t.predicted += j == 0 ? g.spf : q * s;   // the kept columns, contiguous
    if (flushed) t.emitted = t.predicted > 0 ? H * (t.predicted - 1) : 0;
    else t.emitted = H * t.predicted - N / 2 > 0 ? H * t.predicted - N / 2 : 0;
    return t;
}

struct Call {
    std::vector<int64_t> dn, df, off;
    std::vector<uint8_t> fl;
};

static std::pair<int, int64_t> brute_refusal(const SlideCfg& g, const std::vector<SlideState>& st, const Call& c, bool have_out,
                                             int64_t out_stride) {
    const int64_t M = g.max_windows;
    for (size_t b = 0; b < st.size(); ++b) {
        const SlideState& s = st[b];
        if (c.dn[b] < 0 || c.df[b] < 0) return {SLIDE_BAD_COUNT, (int64_t)b};
        if (s.flushed && (c.dn[b] > 0 || c.df[b] > 0 || c.fl[b])) return {SLIDE_AFTER_FLUSH, (int64_t)b};
        const int64_t n2 = s.n + c.dn[b], f2 = s.f + c.df[b];
        if (c.fl[b] && n2 > (int64_t)g.hop * (g.spf / g.F) * f2) return {SLIDE_FLUSH_SHORT, (int64_t)b};
        const Totals t0 = brute(g, s.n, s.f, s.flushed), t1 = brute(g, n2, f2, s.flushed || c.fl[b]);
        if (t1.windows - t0.windows > M) return {SLIDE_TOO_MANY, (int64_t)b};
        if (t1.wa - t1.windows > M) return {SLIDE_SAMPLES_AHEAD, (int64_t)b};
        if (t1.wv - t1.windows > M) return {SLIDE_VIDEO_AHEAD, (int64_t)b};
        const int64_t n_out = t1.emitted - t0.emitted;
        if (n_out > 0 && (!have_out || out_stride < n_out)) return {SLIDE_OUT_SMALL, (int64_t)b};
    }
    return {SLIDE_OK, -1};
}

// what each ring slot of one stream holds (-1: nothing yet)
struct Rings {
    std::vector<int64_t> frame, slice, video, synth;   // analysed frame (maxima, phases); mel slice; video frame; time frame
    std::vector<int64_t> slice_lo, slice_hi;           // the frames [lo, hi) of the slot's slice that have been written
};

struct Session {
    SlideCfg g;
    std::vector<SlideState> st;
    std::vector<StreamRow> rows;
    std::vector<SlideRow> xrows;
    std::vector<StreamItem> items;
    std::vector<Rings> rings;
    SlideItemCounts cap;
    Session(const SlideCfg& cfg, int64_t B) : g(cfg), st(B, SlideState{0, 0, 0, 0}), rows(B), xrows(B), rings(B) {
        cap = slide_item_caps(g);
        items.resize((size_t)(cap.total() * B));
        for (Rings& r : rings) {
            r.frame.assign(g.R(), -1); r.synth.assign(g.R(), -1);
            r.slice.assign(g.RS(), -1); r.slice_lo.assign(g.RS(), 0); r.slice_hi.assign(g.RS(), 0);
            r.video.assign(g.RVf(), -1);
        }
    }
};

static void expect_items(const char* what, const StreamItem*& it, int b, int64_t n, int first, int step) {
    for (int64_t i = 0; i < n; ++i, ++it)
        EXPECT(it->b == b && it->chunk == first + step * (int)i, "%s: item %ld of stream %d is (%d, %d)", what, (long)i, b, it->b,
               it->chunk);
}

// plays one call; returns whether it was accepted
static bool play(Session& s, const Call& c, bool have_out, int64_t out_stride) {
    const SlideCfg& g = s.g;
    const int64_t B = (int64_t)s.st.size();
    const int q = g.spf / g.F, qs = q * g.stride, R = g.R(), RS = g.RS(), RVf = g.RVf();
    const std::vector<SlideState> before = s.st;
    const auto want = brute_refusal(g, s.st, c, have_out, out_stride);
    const SlidePlan p = slide_rows(g, s.st.data(), B, c.off.data(), c.dn.data(), c.df.data(), c.fl.data(), have_out, out_stride,
                                   s.rows.data(), s.xrows.data());
    EXPECT(p.status == want.first && p.bad == want.second, "status %d at stream %ld, want %d at %ld (%s)", p.status, (long)p.bad,
           want.first, (long)want.second, slide_message(want.first));
    for (int64_t b = 0; b < B; ++b)
        EXPECT(before[b].n == s.st[b].n && before[b].f == s.st[b].f && before[b].flushed == s.st[b].flushed &&
                   before[b].parity == s.st[b].parity, "slide_rows wrote the state");
    ++seen_status[p.status];
    if (p.status != SLIDE_OK) return false;

    int64_t clips = 0, video = 0;
    SlideItemCounts total;
    for (int64_t b = 0; b < B; ++b) {
        const SlideState& o = before[b];
        const StreamRow& r = s.rows[b];
        const SlideRow& x = s.xrows[b];
        const int64_t n2 = o.n + c.dn[b], f2 = o.f + c.df[b];
        const bool closed = o.flushed || c.fl[b];
        const Totals t0 = brute(g, o.n, o.f, o.flushed), t1 = brute(g, n2, f2, closed);
        EXPECT(r.n_old == o.n && r.n_new == n2 && r.t0 == t0.frames && r.nt == t1.frames - t0.frames, "stream %ld: analysis row", (long)b);
        EXPECT(r.Lf == (c.fl[b] ? (int64_t)g.hop * q * f2 : -1) && r.flush == (c.fl[b] ? 1 : 0), "stream %ld: flush row", (long)b);
        EXPECT(r.nblk == (r.nt + STREAM_SCHUNK - 1) / STREAM_SCHUNK, "stream %ld: nblk", (long)b);
        EXPECT(r.e_old == t0.emitted && r.n_out == t1.emitted - t0.emitted && r.T == t1.predicted, "stream %ld: ola row", (long)b);
        EXPECT(r.tail_in == o.parity && r.tail_out == (o.parity ^ (c.dn[b] > 0 ? 1 : 0)), "stream %ld: tail parity", (long)b);
        EXPECT(r.sample_off == (c.dn[b] > 0 ? c.off[b] : 0), "stream %ld: sample_off", (long)b);
        EXPECT(x.w_old == t0.windows && x.w_new == t1.windows - t0.windows && x.clip0 == clips, "stream %ld: windows", (long)b);
        EXPECT(x.f_old == o.f && x.f_new == c.df[b] && x.video_off == video, "stream %ld: video row", (long)b);
        EXPECT(x.T0 == t0.predicted && x.nt == t1.predicted - t0.predicted, "stream %ld: synthesis row", (long)b);
        clips += x.w_new;
        video += c.df[b];

        // ---- the rings: this call's writes, then every read of this call finds its entry ----
        Rings& ring = s.rings[b];
        for (int64_t t = t0.frames; t < t1.frames; ++t) {   // the analysis
            ring.frame[t % R] = t;
            const int64_t sl = t / g.spf, slot = sl % RS;
            if (ring.slice[slot] != sl) { ring.slice[slot] = sl; ring.slice_lo[slot] = t; }
            ring.slice_hi[slot] = t + 1;
        }
        EXPECT(x.app0 >= o.f && x.app0 + x.n_app == (x.n_app > 0 ? f2 : x.app0) && x.n_app >= 0, "stream %ld: append range", (long)b);
        EXPECT(x.app0 <= std::max<int64_t>(o.f, (int64_t)g.stride * t1.windows), "stream %ld: a frame a later window reads is not kept",
               (long)b);
        for (int64_t j = t0.windows; j < t1.windows; ++j)   // frames the windows take from the ring: before any append lands
            for (int64_t fr = g.stride * j; fr < g.stride * j + g.F; ++fr) {
                EXPECT(fr < f2, "stream %ld: window %ld reads video frame %ld of %ld", (long)b, (long)j, (long)fr, (long)f2);
                if (fr < o.f) EXPECT(ring.video[fr % RVf] == fr, "stream %ld: video frame %ld left the ring", (long)b, (long)fr);
            }
        for (int64_t fr = x.app0; fr < x.app0 + x.n_app; ++fr) {
            const int64_t old = ring.video[fr % RVf];   // the gather blocks of this call may still be reading
            EXPECT(old < g.stride * t0.windows, "stream %ld: appending frame %ld over live frame %ld", (long)b, (long)fr, (long)old);
            ring.video[fr % RVf] = fr;
        }
        for (int64_t j = t0.windows; j < t1.windows; ++j)
            for (int64_t t = (int64_t)qs * j; t < (int64_t)qs * j + g.spf; ++t) {
                const int64_t sl = t / g.spf, slot = sl % RS;
                EXPECT(ring.slice[slot] == sl && ring.slice_lo[slot] <= std::max(t, sl * g.spf) && t < ring.slice_hi[slot] &&
                           ring.slice_lo[slot] == sl * g.spf,
                       "stream %ld: mel frame %ld of window %ld left the ring", (long)b, (long)t, (long)j);
                EXPECT(ring.frame[t % R] == t || t < (j == 0 ? 0 : (int64_t)qs * j + g.spf - qs),
                       "stream %ld: the maximum of frame %ld left the ring", (long)b, (long)t);
            }
        for (int64_t t = t0.predicted; t < t1.predicted; ++t) {   // the synthesis: phases in, time frames out
            EXPECT(ring.frame[t % R] == t, "stream %ld: the phase of frame %ld left the ring", (long)b, (long)t);
            ring.synth[t % R] = t;
        }
        if (r.n_out > 0)
            for (int64_t t = std::max<int64_t>(0, t0.predicted - 3); t < t1.predicted; ++t)
                EXPECT(ring.synth[t % R] == t, "stream %ld: time frame %ld left the ring", (long)b, (long)t);

        const SlideItemCounts ic = slide_row_items(r, x);
        EXPECT(ic.spec <= s.cap.spec && ic.route <= s.cap.route && ic.gather <= s.cap.gather && ic.synth <= s.cap.synth &&
                   ic.ola <= s.cap.ola, "stream %ld: items past the caps", (long)b);
        EXPECT(ic.spec >= r.nblk && (ic.spec > r.nblk) == (c.dn[b] > 0), "stream %ld: analysis items", (long)b);
        EXPECT(ic.synth * STREAM_SYNTH_FPG >= x.nt && (ic.synth - 1) * STREAM_SYNTH_FPG < std::max(1, x.nt), "stream %ld: synth items", (long)b);
        EXPECT(ic.ola * STREAM_OLA_BLOCK >= r.n_out && (ic.ola - 1) * STREAM_OLA_BLOCK < std::max(1, r.n_out), "stream %ld: ola items", (long)b);
        total.spec += ic.spec; total.route += ic.route; total.gather += ic.gather; total.synth += ic.synth; total.ola += ic.ola;
    }
    EXPECT(p.clips == clips && p.video_total == video, "plan totals");
    EXPECT(p.items.spec == total.spec && p.items.route == total.route && p.items.gather == total.gather &&
               p.items.synth == total.synth && p.items.ola == total.ola, "plan item counts");
    EXPECT(clips <= B * g.max_windows, "more clips than the forward scratch holds");

    StreamItem* spec = s.items.data();
    StreamItem* route = spec + s.cap.spec * B;
    StreamItem* gather = route + s.cap.route * B;
    StreamItem* synth = gather + s.cap.gather * B;
    StreamItem* ola = synth + s.cap.synth * B;
    slide_fill_items(s.rows.data(), s.xrows.data(), B, spec, route, gather, synth, ola);
    const StreamItem *i0 = spec, *i1 = route, *i2 = gather, *i3 = synth, *i4 = ola;
    for (int64_t b = 0; b < B; ++b) {
        const SlideItemCounts ic = slide_row_items(s.rows[b], s.xrows[b]);
        expect_items("spec", i0, (int)b, ic.spec, 0, 1);
        expect_items("route", i1, (int)b, ic.route, STREAM_CLAMP, 0);
        expect_items("gather", i2, (int)b, (int64_t)SLIDE_GATHER_X * s.xrows[b].w_new, 0, 1);
        expect_items("append", i2, (int)b, s.xrows[b].n_app, -1, -1);
        expect_items("synth", i3, (int)b, ic.synth, 0, 1);
        expect_items("ola", i4, (int)b, ic.ola, 0, 1);
    }
    slide_commit(s.rows.data(), s.xrows.data(), B, s.st.data());
    for (int64_t b = 0; b < B; ++b)
        EXPECT(s.st[b].n == before[b].n + c.dn[b] && s.st[b].f == before[b].f + c.df[b] &&
                   s.st[b].flushed == (before[b].flushed || c.fl[b]), "commit");
    return true;
}

static void run(int spf, int F, int stride, int64_t M, unsigned seed) {
    const int n_fft = spf == 20 ? 640 : 800, hop = n_fft / 4, q = spf / F;
    const int64_t B = 3;
    std::mt19937 rng(seed);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    for (int rep = 0; rep < 6; ++rep) {
        Session s(SlideCfg{n_fft, hop, spf, F, stride, M}, B);
        long accepted = 0;
        for (int call = 0; call < 160; ++call) {
            Call c;
            c.dn.resize(B); c.df.resize(B); c.off.resize(B); c.fl.assign(B, 0);
            int64_t off = 0;
            for (int64_t b = 0; b < B; ++b) {
                if (s.st[b].flushed && pick(0, 9) != 0) continue;   // a closed stream mostly idles until its slot is reset
                const int mode = (int)pick(0, 19);
                const int64_t k = mode < 12 ? 1 : mode < 15 ? pick(0, M) * stride : mode < 19 ? pick(0, std::min<int64_t>(M * stride, 3))
                                                                                              : pick(0, 3 * M * stride + F);
                // mostly a tick of k video frames and their samples, with jitter; sometimes one input alone, far ahead
                c.df[b] = mode == 18 ? 0 : k;
                c.dn[b] = mode == 17 ? 0 : std::max<int64_t>(0, k * q * hop + (pick(0, 3) == 0 ? pick(-hop, hop) : 0));
                if (pick(0, 60) == 0) (pick(0, 1) ? c.dn[b] : c.df[b]) = -1;
                if (pick(0, 40) == 0) c.fl[b] = 1;
                c.off[b] = off;
                off += std::max<int64_t>(0, c.dn[b]);
            }
            const int om = (int)pick(0, 12);
            accepted += play(s, c, om != 0, om == 1 ? pick(0, 2 * hop) : (int64_t)1 << 30);
            for (int64_t b = 0; b < B; ++b)   // a caller leaves and its slot starts again
                if (pick(0, s.st[b].flushed ? 3 : 60) == 0) {
                    s.st[b] = SlideState{0, 0, 0, 0};
                    s.rings[b] = Session(s.g, 1).rings[0];
                }
        }
        EXPECT(accepted > 20, "only %ld calls of the schedule were legal (spf %d stride %d M %ld)", accepted, spf, stride, (long)M);
    }
}

int main() {
    // the closed forms against the counting definition
    for (int pair = 0; pair < 2; ++pair) {
        const int spf = pair ? 24 : 20, F = pair ? 6 : 5, n_fft = pair ? 800 : 640, hop = n_fft / 4;
        for (int stride = 1; stride <= F; ++stride) {
            const SlideCfg g{n_fft, hop, spf, F, stride, 4};
            for (int64_t f = 0; f <= 3 * F + 2; ++f)
                for (int64_t n = 0; n <= (int64_t)hop * (spf + 3 * spf / F * stride + 3); n += 37)
                    for (int fl = 0; fl < 2; ++fl) {
                        if (fl && n > (int64_t)hop * (spf / F) * f) continue;
                        const Totals t = brute(g, n, f, fl);
                        const SlideCounts c = slide_totals(g, n, f, fl);
                        EXPECT(c.frames == t.frames && c.wa == t.wa && c.wv == t.wv && c.windows == t.windows &&
                                   c.predicted == t.predicted && c.emitted == t.emitted,
                               "totals at spf %d stride %d n %ld f %ld flushed %d", spf, stride, (long)n, (long)f, fl);
                        if (stride == F && f % F == 0) {   // the existing session at v = f / F
                            const StreamCounts k = stream_totals(n_fft, hop, spf, n, f / F, fl);
                            EXPECT(k.frames == c.frames && k.slices == c.windows && k.emitted == c.emitted,
                                   "stride F differs from stream_totals at n %ld f %ld", (long)n, (long)f);
                        }
                    }
        }
    }
    unsigned seed = 1;
    for (int pair = 0; pair < 2; ++pair)
        for (int64_t M : {1, 3, 80})
            for (int sF = 0; sF < 2; ++sF) run(pair ? 24 : 20, pair ? 6 : 5, sF ? (pair ? 6 : 5) : 1, M, seed++);
    for (int st : {SLIDE_OK, SLIDE_BAD_COUNT, SLIDE_AFTER_FLUSH, SLIDE_FLUSH_SHORT, SLIDE_TOO_MANY, SLIDE_SAMPLES_AHEAD,
                   SLIDE_VIDEO_AHEAD, SLIDE_OUT_SMALL})
        EXPECT(seen_status[st] > 0, "the schedules never met status %d (%s)", st, slide_message(st));
    EXPECT(seen_status[SLIDE_CAPACITY] == 0, "a legal call passed the item caps");
    std::printf("ok %ld checks\n", checks);
    return 0;
}
