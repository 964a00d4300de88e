// Stand-alone check of csrc/stream_geom.h (built with -fsanitize=address,undefined by tests/test_stream_each_host.py):
// random per-stream schedules are played through stream_rows / stream_fill_items / stream_commit, and every call is
// compared with a brute-force definition that counts frames, slices and samples one by one.  Prints "ok <n checks>"
// and exits 0, or the first mismatch and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "stream_geom.h"

using namespace avse;

static long checks = 0;
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

constexpr int N = 640, H = 160;

// ---- the definition, by counting (include/avse.h avse_stream_push) ----
struct Totals {
    int64_t frames, slices, emitted;
};
static Totals brute(int spf, int64_t n, int64_t v, bool flushed) {
    Totals t{0, 0, 0};
    if (flushed) {   // the closed signal has slice * v samples: frames 0 .. spf v - 1, all slices, all but the last hop
        t.frames = (int64_t)spf * v;
        t.slices = v;
        t.emitted = v > 0 ? (int64_t)H * (spf * v - 1) : 0;
        return t;
    }
    // frame f reads samples up to H f + N/2 - 1 (frame 0: x[N/2] through the left reflection)
    while ((t.frames == 0 ? n >= N / 2 + 1 : n >= H * t.frames + N / 2)) ++t.frames;
    while ((t.slices + 1) * spf <= t.frames && t.slices + 1 <= v) ++t.slices;
    // sample i is final once every frame covering it (frames f with H f - N/2 <= i < H f + N/2) is inverted
    const int64_t inverted = t.slices * spf;
    t.emitted = inverted * H - N / 2 > 0 ? inverted * H - N / 2 : 0;
    return t;
}

struct Call {
    std::vector<int64_t> dn, dv, off;
    std::vector<uint8_t> fl;
};

// the first offending stream and why, in the order the header lists the checks
static std::pair<int, int64_t> brute_refusal(const StreamCfg& g, const std::vector<StreamState>& st, const Call& c,
                                             bool have_out, int64_t out_stride) {
    const int64_t slice = (int64_t)g.spf * H, M = g.max_slices;
    for (size_t b = 0; b < st.size(); ++b) {
        const StreamState& s = st[b];
        if (c.dn[b] < 0 || c.dv[b] < 0) return {STREAM_BAD_COUNT, (int64_t)b};
        if (s.flushed && (c.dn[b] > 0 || c.dv[b] > 0 || c.fl[b])) return {STREAM_AFTER_FLUSH, (int64_t)b};
        const int64_t n2 = s.n + c.dn[b], v2 = s.v + c.dv[b];
        if (c.fl[b] && n2 > slice * v2) return {STREAM_FLUSH_SHORT, (int64_t)b};
        const Totals t0 = brute(g.spf, s.n, s.v, s.flushed), t1 = brute(g.spf, n2, v2, s.flushed || c.fl[b]);
        if (t1.slices - t0.slices > M) return {STREAM_TOO_MANY, (int64_t)b};
        if (n2 - slice * v2 > slice * M) return {STREAM_SAMPLES_AHEAD, (int64_t)b};
        if (v2 - t1.frames / g.spf > M) return {STREAM_VIDEO_AHEAD, (int64_t)b};
        const int64_t n_out = t1.emitted - t0.emitted;
        if (n_out > 0 && (!have_out || out_stride < n_out)) return {STREAM_OUT_SMALL, (int64_t)b};
    }
    return {STREAM_OK, -1};
}

static bool same_state(const std::vector<StreamState>& a, const std::vector<StreamState>& b) {
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].n != b[i].n || a[i].v != b[i].v || a[i].flushed != b[i].flushed || a[i].parity != b[i].parity) return false;
    return true;
}

// every (stream, chunk) of `want` exactly once in items[0 .. n), nothing else, streams in increasing order
static void expect_table(const char* what, const StreamItem* items, int64_t n, const std::map<std::pair<int, int>, int>& want) {
    std::map<std::pair<int, int>, int> seen;
    for (int64_t i = 0; i < n; ++i) {
        ++seen[{items[i].b, items[i].chunk}];
        if (i > 0) EXPECT(items[i - 1].b <= items[i].b, "%s: item %ld is not stream-major", what, (long)i);
    }
    EXPECT(seen.size() == want.size() && (int64_t)want.size() == n, "%s: %zu distinct items of %ld, want %zu", what, seen.size(),
           (long)n, want.size());
    for (const auto& kv : want) EXPECT(seen.count(kv.first) && seen[kv.first] == 1, "%s: item (%d, %d)", what, kv.first.first,
                                       kv.first.second);
}

struct Session {
    StreamCfg g;
    std::vector<StreamState> st;
    std::vector<StreamRow> rows;
    std::vector<StreamItem> items;   // the four tables, one after the other, sized by stream_item_caps
    StreamItemCounts cap;
    Session(int spf, int64_t M, int64_t B) : g{N, H, spf, M}, st(B, StreamState{0, 0, 0, 0}), rows(B) {
        cap = stream_item_caps(g);
        items.resize((size_t)(cap.total() * B));
    }
};

// plays one call; returns whether it was accepted
static bool play(Session& s, const Call& c, bool have_out, int64_t out_stride) {
    const int64_t B = (int64_t)s.st.size();
    const std::vector<StreamState> before = s.st;
    const auto want = brute_refusal(s.g, s.st, c, have_out, out_stride);
    const StreamPlan p = stream_rows(s.g, s.st.data(), B, c.off.data(), c.dn.data(), c.dv.data(), c.fl.data(), have_out,
                                     out_stride, s.rows.data());
    EXPECT(p.status == want.first && p.bad == want.second, "status %d at stream %ld, want %d at %ld (%s)", p.status, (long)p.bad,
           want.first, (long)want.second, stream_message(want.first));
    EXPECT(same_state(before, s.st), "stream_rows wrote the state");
    if (p.status != STREAM_OK) return false;

    const int spf = s.g.spf;
    const int R = spf * (2 * (int)s.g.max_slices + 1), RS = R / spf, RV = 2 * (int)s.g.max_slices;
    std::map<std::pair<int, int>, int> w_spec, w_route, w_synth, w_ola;
    int64_t clips = 0, vids = 0, max_out = 0;
    bool any = false;
    for (int64_t b = 0; b < B; ++b) {
        const StreamState& o = before[b];
        const StreamRow& r = s.rows[b];
        const bool fl = c.fl[b] != 0;
        const int64_t n2 = o.n + c.dn[b], v2 = o.v + c.dv[b];
        const Totals t0 = brute(spf, o.n, o.v, o.flushed), t1 = brute(spf, n2, v2, o.flushed || fl);
        // the row: differences of the totals
        EXPECT(r.n_old == o.n && r.n_new == n2 && r.v_old == o.v && r.v_new == c.dv[b], "stream %ld: counters", (long)b);
        EXPECT(r.t0 == t0.frames && r.nt == t1.frames - t0.frames, "stream %ld: frames %ld + %d, want %ld + %ld", (long)b,
               (long)r.t0, r.nt, (long)t0.frames, (long)(t1.frames - t0.frames));
        EXPECT(r.k_old == t0.slices && r.k_new == t1.slices - t0.slices, "stream %ld: slices", (long)b);
        EXPECT(r.e_old == t0.emitted && r.n_out == t1.emitted - t0.emitted, "stream %ld: emitted", (long)b);
        EXPECT(r.T == t1.slices * spf && r.nv == v2 - t0.slices, "stream %ld: T / nv", (long)b);
        EXPECT(r.Lf == (fl ? (int64_t)spf * H * v2 : -1) && r.flush == (fl ? 1 : 0), "stream %ld: Lf", (long)b);
        EXPECT(r.clip0 == clips && r.video_off == vids, "stream %ld: clip0 %d / video_off %ld, want the prefix sums %ld / %ld",
               (long)b, r.clip0, (long)r.video_off, (long)clips, (long)vids);
        EXPECT(r.tail_in == o.parity && r.tail_out == (o.parity ^ (c.dn[b] > 0 ? 1 : 0)), "stream %ld: tail parity", (long)b);
        EXPECT(c.dn[b] == 0 || r.sample_off == c.off[b], "stream %ld: sample_off", (long)b);
        EXPECT(r.n_out <= out_stride || !have_out, "stream %ld: emits past out_stride", (long)b);
        clips += r.k_new;
        vids += r.v_new;
        max_out = r.n_out > max_out ? r.n_out : max_out;
        any = any || c.dn[b] > 0 || c.dv[b] > 0 || fl;
        // the work, item by item: every frame in one chunk, every moving slice in ROUTE_X parts, ..
        {
            int64_t covered = 0;
            for (int ch = 0; covered < r.nt; ++ch) {
                w_spec[{(int)b, ch}] = 1;
                covered += STREAM_SCHUNK;
            }
            EXPECT((int64_t)r.nblk * STREAM_SCHUNK >= r.nt && ((int64_t)r.nblk - 1) * STREAM_SCHUNK < r.nt, "stream %ld: nblk", (long)b);
            if (c.dn[b] > 0) w_spec[{(int)b, r.nblk}] = 1;   // the tail block
        }
        for (int64_t k = t0.slices; k < v2; ++k) {
            const bool from_queue = k < o.v, to_net = k < t1.slices;
            if (from_queue && !to_net) continue;             // queued and stays queued
            for (int part = 0; part < STREAM_ROUTE_X; ++part) w_route[{(int)b, (int)(k - t0.slices) * STREAM_ROUTE_X + part}] = 1;
        }
        if (t1.slices > t0.slices) w_route[{(int)b, STREAM_CLAMP}] = 1;
        for (int64_t f = 0; f < (t1.slices - t0.slices) * spf; f += STREAM_SYNTH_FPG) w_synth[{(int)b, (int)(f / STREAM_SYNTH_FPG)}] = 1;
        for (int64_t j = 0; j < t1.emitted - t0.emitted; j += STREAM_OLA_BLOCK) w_ola[{(int)b, (int)(j / STREAM_OLA_BLOCK)}] = 1;
        // live ring entries never share a slot: what the call reads and writes of each ring fits the ring
        EXPECT(t1.frames - t0.slices * spf <= R, "stream %ld: %ld live frames in a ring of %d", (long)b,
               (long)(t1.frames - t0.slices * spf), R);                                    // phase / max ring
        EXPECT((t1.frames + spf - 1) / spf - t0.slices <= RS, "stream %ld: mel ring", (long)b);
        EXPECT(v2 - t0.slices <= RV, "stream %ld: %ld video slices in a queue of %d", (long)b, (long)(v2 - t0.slices), RV);
        EXPECT((t1.slices - t0.slices) * spf + 3 <= R, "stream %ld: frame ring", (long)b);  // + the overlap-add tail
        {
            std::vector<char> used(R, 0);
            for (int64_t f = t0.slices * spf; f < t1.frames; ++f) {
                EXPECT(!used[f % R], "stream %ld: frames share slot %ld", (long)b, (long)(f % R));
                used[f % R] = 1;
            }
            std::vector<char> vused(RV, 0);
            for (int64_t k = t0.slices; k < v2; ++k) {
                EXPECT(!vused[k % RV], "stream %ld: video slices share slot %ld", (long)b, (long)(k % RV));
                vused[k % RV] = 1;
            }
        }
    }
    EXPECT(p.clips == clips && p.video_total == vids && p.max_n_out == max_out && p.any == any, "plan totals");
    EXPECT(p.items.spec == (int64_t)w_spec.size() && p.items.route == (int64_t)w_route.size() &&
               p.items.synth == (int64_t)w_synth.size() && p.items.ola == (int64_t)w_ola.size(),
           "item counts %ld %ld %ld %ld", (long)p.items.spec, (long)p.items.route, (long)p.items.synth, (long)p.items.ola);
    EXPECT(p.items.spec <= s.cap.spec * B && p.items.route <= s.cap.route * B && p.items.synth <= s.cap.synth * B &&
               p.items.ola <= s.cap.ola * B, "the tables sized at create hold the call");
    // fill with a guard word after each table: nothing is written past the counts
    std::vector<StreamItem> route(p.items.route + 1), synth(p.items.synth + 1), ola(p.items.ola + 1), specv(p.items.spec + 1);
    const StreamItem guard{-77, -77};
    specv.back() = route.back() = synth.back() = ola.back() = guard;
    stream_fill_items(s.g, s.rows.data(), B, specv.data(), route.data(), synth.data(), ola.data());
    for (const auto* t : {&specv, &route, &synth, &ola}) EXPECT(t->back().b == -77 && t->back().chunk == -77, "table overrun");
    expect_table("spec", specv.data(), p.items.spec, w_spec);
    expect_table("route", route.data(), p.items.route, w_route);
    expect_table("synth", synth.data(), p.items.synth, w_synth);
    expect_table("ola", ola.data(), p.items.ola, w_ola);
    stream_commit(s.rows.data(), B, s.st.data());
    for (int64_t b = 0; b < B; ++b) {
        const StreamState& o = before[b];
        EXPECT(s.st[b].n == o.n + c.dn[b] && s.st[b].v == o.v + c.dv[b] && s.st[b].flushed == (o.flushed || c.fl[b]),
               "stream %ld: committed state", (long)b);
    }
    return true;
}

static Call idle(int64_t B) {
    Call c;
    c.dn.assign(B, 0); c.dv.assign(B, 0); c.off.assign(B, 0); c.fl.assign(B, 0);
    return c;
}

int main() {
    std::mt19937_64 rng(17);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };

    // stream_totals against counting
    for (int spf : {20, 4})
        for (int64_t n = 0; n < 3 * spf * H + 700; n += (n < 700 ? 1 : 37))
            for (int64_t v = 0; v < 5; ++v)
                for (int f = 0; f < 2; ++f) {
                    if (f && n > (int64_t)spf * H * v) continue;
                    const StreamCounts c = stream_totals(N, H, spf, n, v, f != 0);
                    const Totals t = brute(spf, n, v, f != 0);
                    EXPECT(c.frames == t.frames && c.slices == t.slices && c.emitted == t.emitted, "totals(%ld, %ld, %d)", (long)n,
                           (long)v, f);
                }

    // random schedules: most calls legal, some over a limit; streams idle, flush, and are reset (a caller leaves)
    long accepted = 0, refused = 0;
    const int64_t Bs[] = {1, 3, 17, 64, 1024};
    for (int round = 0; round < 60; ++round) {
        const int64_t B = Bs[round % 5], M = pick(1, 16);
        const int spf = round % 7 == 6 ? 4 : 20;
        const int64_t slice = (int64_t)spf * H;
        Session s(spf, M, B);
        const int calls = B >= 1024 ? 6 : 40;
        for (int k = 0; k < calls; ++k) {
            Call c = idle(B);
            int64_t off = 0;
            for (int64_t b = 0; b < B; ++b) {
                const int mode = (int)pick(0, 9);
                if (mode < 3) continue;                                   // idle
                const StreamState& o = s.st[b];
                if (o.flushed) {                                          // a flushed stream: reset it, or (rarely) poke it
                    if (mode < 8) s.st[b] = StreamState{0, 0, 0, (uint8_t)0};
                    else c.dn[b] = 5;
                    continue;
                }
                const int64_t room = slice * (o.v + M) - o.n;             // samples until the ahead-of-video limit
                const int64_t sizes[] = {1, 7, 160, 321, 1000, slice, slice + 160, 3 * slice};
                c.dn[b] = mode == 9 ? room + pick(0, 2) : std::min<int64_t>(sizes[pick(0, 7)], room > 0 ? room : 0);
                c.dv[b] = pick(0, 5) == 0 ? pick(0, M + 1) : pick(0, 1);
                c.fl[b] = pick(0, 11) == 0;
                if (c.fl[b] && pick(0, 3)) {                              // usually a legal flush: enough video for the samples
                    const int64_t need = (o.n + c.dn[b] + slice - 1) / slice - o.v;
                    c.dv[b] = std::max<int64_t>(c.dv[b], need);
                }
                c.off[b] = off;
                off += c.dn[b] + pick(0, 3);
            }
            const bool have_out = pick(0, 19) != 0;
            const int64_t out_stride = pick(0, 9) == 0 ? pick(0, slice) : slice * M + N / 2;
            (play(s, c, have_out, out_stride) ? accepted : refused)++;
        }
    }
    EXPECT(accepted > 200 && refused > 200, "the schedules exercise both: %ld accepted, %ld refused", accepted, refused);

    // each refusal names the first offending stream, and the later streams do not matter
    {
        Session s(20, 2, 5);
        Call c = idle(5);
        c.dn = {3200, 3200, 3200, 3200, 3200};
        c.dv = {1, 1, 1, 1, 1};
        EXPECT(play(s, c, true, 6400 + 320), "a plain first push");
        const struct { int status; int64_t dn, dv; uint8_t fl; } bad[] = {
            {STREAM_BAD_COUNT, -1, 0, 0},       {STREAM_BAD_COUNT, 0, -1, 0},     {STREAM_TOO_MANY, 3 * 3200, 3, 0},
            {STREAM_SAMPLES_AHEAD, 2 * 3200 + 1, 0, 0}, {STREAM_VIDEO_AHEAD, 0, 3, 0}, {STREAM_FLUSH_SHORT, 1, 0, 1}};
        for (const auto& t : bad)
            for (int64_t at = 0; at < 5; ++at) {
                Call d = idle(5);
                d.dn[at] = t.dn; d.dv[at] = t.dv; d.fl[at] = t.fl;
                if (at + 1 < 5) d.dn[at + 1] = -9;   // a later offender is not the one named
                const StreamPlan p = stream_rows(s.g, s.st.data(), 5, d.off.data(), d.dn.data(), d.dv.data(), d.fl.data(), true,
                                                 1 << 20, s.rows.data());
                EXPECT(p.status == t.status && p.bad == at, "status %d at %ld, want %d at %ld", p.status, (long)p.bad, t.status, (long)at);
                EXPECT(!play(s, d, true, 1 << 20), "refused");
            }
        Call e = idle(5);
        e.dn[2] = 160;                                        // completes slice 0 of stream 2: 2880 samples
        EXPECT(!play(s, e, true, 2879) && !play(s, e, false, 1 << 20), "out too small / NULL");
        EXPECT(play(s, e, true, 2880), "out just large enough");
        Call f = idle(5);
        f.fl[3] = 1;
        EXPECT(play(s, f, true, 1 << 20), "flush of stream 3");
        Call h = idle(5);
        h.dv[3] = 1;
        const StreamPlan p = stream_rows(s.g, s.st.data(), 5, h.off.data(), h.dn.data(), h.dv.data(), h.fl.data(), true, 1 << 20,
                                         s.rows.data());
        EXPECT(p.status == STREAM_AFTER_FLUSH && p.bad == 3, "video for a flushed stream");
        h.dv[3] = 0; h.fl[3] = 1;
        EXPECT(!play(s, h, true, 1 << 20), "a second flush");
        EXPECT(play(s, idle(5), false, 0), "a call without work is legal, flushed streams included");
    }

    // one active stream among 1024: that stream's items, nobody else's
    for (int64_t M : {1, 4, 16}) {
        Session big(20, M, 1024), one(20, M, 1);
        const int64_t at = 700;
        for (int step = 0; step < 6; ++step) {
            Call c = idle(1024), c1 = idle(1);
            c1.dn[0] = c.dn[at] = step == 0 ? 321 : pick(1, 3200 * M);
            c1.dv[0] = c.dv[at] = step == 0 ? 0 : (c.dn[at] + 3199) / 3200;
            c1.fl[0] = c.fl[at] = step == 5;
            if (step == 5) c1.dv[0] = c.dv[at] = std::max<int64_t>(c.dv[at], (big.st[at].n + c.dn[at] + 3199) / 3200 - big.st[at].v);
            const StreamPlan p = stream_rows(big.g, big.st.data(), 1024, c.off.data(), c.dn.data(), c.dv.data(), c.fl.data(), true,
                                             1 << 20, big.rows.data());
            const StreamPlan q = stream_rows(one.g, one.st.data(), 1, c1.off.data(), c1.dn.data(), c1.dv.data(), c1.fl.data(), true,
                                             1 << 20, one.rows.data());
            EXPECT(p.status == q.status, "one of 1024: status %d / %d", p.status, q.status);
            if (p.status != STREAM_OK) continue;
            EXPECT(p.items.spec == q.items.spec && p.items.route == q.items.route && p.items.synth == q.items.synth &&
                       p.items.ola == q.items.ola && p.clips == q.clips, "one of 1024: the active stream's item counts");
            EXPECT(std::memcmp(&big.rows[at], &one.rows[0], sizeof(StreamRow)) == 0, "one of 1024: the same row");
            EXPECT(play(big, c, true, 1 << 20) && play(one, c1, true, 1 << 20), "accepted");
        }
    }
    std::printf("ok %ld checks (%ld calls accepted, %ld refused)\n", checks, accepted, refused);
    return 0;
}
