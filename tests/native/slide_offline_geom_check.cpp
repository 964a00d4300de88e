// Stand-alone check of csrc/slide_offline_geom.h (built with -fsanitize=address,undefined by
// tests/test_slide_offline_host.py): ragged batches over a sweep of (S, F in {5, 6}, stride 1 .. F, spf in {20, 24}),
// S = 0 and 1 included, are planned and compared with a brute-force restatement that counts windows, frames, video
// (slice, element) pairs and kept columns one by one: totals, prefix sums, the rows, every item table (each unit of work
// covered exactly once, nothing out of range), the video plan of every window range, and the refusals.  Every array
// is sized exactly, so a write past a table is the sanitizer's to report.  Prints "ok <n checks>" and exits 0, or the
// first mismatch and exits 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "slide_offline_geom.h"

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

// ---- the definition, by counting (include/avse.h, "offline sliding enhancement") ----
struct Brute {
    int64_t W = 0, P = 0;
    std::vector<std::pair<int64_t, int>> kept;      // kept column t -> (window, column of the window)
};
static Brute brute(int spf, int F, int s, int64_t S) {
    Brute b;
    const int q = spf / F;
    const int64_t f = (int64_t)F * S, frames = (int64_t)q * f;
    while (f >= F && (int64_t)s * b.W + F <= f && (int64_t)q * s * b.W + spf <= frames) ++b.W;
    for (int64_t j = 0; j < b.W; ++j)
        for (int c = j == 0 ? 0 : spf - q * s; c < spf; ++c) {
            // a kept column is the spectrogram frame it predicts: contiguous, each frame once
            EXPECT((int64_t)q * s * j + c == (int64_t)b.kept.size(), "kept columns are the frames 0 .. P - 1 in order");
            b.kept.push_back({j, c});
        }
    b.P = (int64_t)b.kept.size();
    return b;
}

static void check_batch(int spf, int F, int s, const std::vector<int64_t>& S, int n_mels) {
    const SlideOffCfg g{spf, F, s};
    const int q = spf / F;
    const int64_t U = (int64_t)S.size();
    std::vector<int64_t> T(S.size());
    for (size_t u = 0; u < S.size(); ++u) T[u] = (int64_t)q * F * S[u] + 1 + (u % 3 == 2 ? 5 : 0);      // the STFT's extra frame(s)
    const SlideOffPlan p0 = slide_off_plan(g, S.data(), T.data(), U, n_mels, nullptr);
    EXPECT(p0.status == SLIDE_OFF_OK, "plan refused: %d", p0.status);
    std::vector<SlideOffRow> rows(S.size());
    const SlideOffPlan p = slide_off_plan(g, S.data(), T.data(), U, n_mels, rows.data());
    EXPECT(p.windows == p0.windows && p.predicted == p0.predicted && p.items.keep == p0.items.keep, "the two passes agree");
    int64_t t_off = 0, w_off = 0, p_off = 0, s_off = 0;
    std::vector<Brute> bs;
    for (int64_t u = 0; u < U; ++u) {
        const Brute b = brute(spf, F, s, S[u]);
        const SlideOffRow& r = rows[u];
        EXPECT(r.W == b.W && r.P == b.P && r.S == S[u] && r.T == T[u], "u %lld: W %d / %lld, P %d / %lld", (long long)u, r.W,
               (long long)b.W, r.P, (long long)b.P);
        EXPECT(r.t_off == t_off && r.w_off == w_off && r.p_off == p_off && r.s_off == s_off, "prefix sums of u %lld", (long long)u);
        int64_t W2, P2;
        slide_off_counts(g, S[u], &W2, &P2);
        EXPECT(W2 == b.W && P2 == b.P, "slide_off_counts");
        // the closed forms of the issue
        EXPECT(b.W == (S[u] > 0 ? ((int64_t)F * S[u] - F) / s + 1 : 0) && b.P == (b.W > 0 ? spf + (int64_t)q * s * (b.W - 1) : 0),
               "closed forms");
        // every frame a window reads lies in the mel block, and the floor's frame too
        if (b.W > 0) EXPECT((int64_t)q * s * (b.W - 1) + spf <= T[u], "frames of the last window");
        // kept-column map of the kernel: j = t < spf ? 0 : (t - spf) / (q s) + 1, column t - q s j
        for (int64_t t = 0; t < b.P; ++t) {
            const int64_t j = t < spf ? 0 : (t - spf) / (q * s) + 1;
            EXPECT(j == b.kept[t].first && t - (int64_t)q * s * j == b.kept[t].second, "kept map at %lld", (long long)t);
        }
        // window -> (slice, element) pairs of the video: frame s j + i is element (s j + i) % F of slice (s j + i) / F
        for (int64_t j = 0; j < b.W; ++j) {
            const int64_t fr = (int64_t)s * j, k = fr / F;
            const int rot = (int)(fr - k * F);
            for (int i = 0; i < F; ++i) {
                const int64_t slice = i + rot < F ? k : k + 1;
                const int el = i + rot < F ? i + rot : i + rot - F;
                EXPECT(slice == (fr + i) / F && el == (fr + i) % F && slice < S[u], "video pair of window %lld frame %d", (long long)j, i);
            }
        }
        t_off += T[u]; w_off += b.W; p_off += b.P; s_off += S[u];
        bs.push_back(b);
    }
    EXPECT(p.frames == t_off && p.windows == w_off && p.predicted == p_off && p.slices == s_off, "totals");
    // item tables: exact sizes; every window and every kept column in exactly one item
    std::vector<StreamItem> scan((size_t)p.items.scan), wins((size_t)p.items.windows), keep((size_t)p.items.keep);
    slide_off_fill_items(rows.data(), U, scan.data(), wins.data(), keep.data());
    std::vector<int> seen_w((size_t)p.windows, 0), seen_p((size_t)p.predicted, 0), seen_u((size_t)U, 0);
    for (const StreamItem& it : scan) {
        EXPECT(it.b >= 0 && it.b < U && it.chunk == 0 && rows[it.b].W > 0, "scan item");
        ++seen_u[it.b];
    }
    for (int64_t u = 0; u < U; ++u) EXPECT(seen_u[u] == (rows[u].W > 0 ? 1 : 0), "one scan block per utterance with windows");
    for (const StreamItem& it : wins) {
        EXPECT(it.b >= 0 && it.b < U && it.chunk >= 0, "windows item");
        const SlideOffRow& r = rows[it.b];
        EXPECT(it.chunk * SLIDE_OFF_WPB < r.W, "no empty windows item");
        for (int j = it.chunk * SLIDE_OFF_WPB; j < r.W && j < (it.chunk + 1) * SLIDE_OFF_WPB; ++j) ++seen_w[r.w_off + j];
    }
    for (int v : seen_w) EXPECT(v == 1, "every window in one item");
    for (const StreamItem& it : keep) {
        EXPECT(it.b >= 0 && it.b < U && it.chunk >= 0, "keep item");
        const SlideOffRow& r = rows[it.b];
        EXPECT(it.chunk * SLIDE_OFF_KEEP < r.P, "no empty keep item");
        for (int t = it.chunk * SLIDE_OFF_KEEP; t < r.P && t < (it.chunk + 1) * SLIDE_OFF_KEEP; ++t) ++seen_p[r.p_off + t];
    }
    for (int v : seen_p) EXPECT(v == 1, "every kept column in one item");
    // nullable tables
    slide_off_fill_items(rows.data(), U, nullptr, nullptr, keep.data());
    slide_off_fill_items(rows.data(), U, scan.data(), wins.data(), nullptr);
    // the video plan of window ranges: every range for small batches, a few for the rest
    std::mt19937 rng((unsigned)(p.windows * 31 + s));
    const int64_t Wt = p.windows;
    auto check_range = [&](int64_t w0, int64_t n) {
        const SlideOffVidPlan c = slide_off_video_plan(g, S.data(), U, w0, n, nullptr);
        EXPECT(c.status == SLIDE_OFF_OK && c.items == SLIDE_OFF_VX * n && c.slices == s_off, "video plan counts");
        EXPECT(c.rows <= std::min<int64_t>(U, n), "rows fit min(n_utt, n)");
        std::vector<SlideOffVidRow> vr((size_t)c.rows);
        const SlideOffVidPlan v = slide_off_video_plan(g, S.data(), U, w0, n, vr.data());
        EXPECT(v.rows == c.rows, "video rows");
        std::vector<StreamItem> items((size_t)v.items);
        slide_off_video_items(vr.data(), v.rows, items.data());
        std::vector<int> parts((size_t)n, 0);
        size_t at = 0;
        for (int64_t b = 0; b < v.rows; ++b)
            for (int i = 0; i < SLIDE_OFF_VX * vr[b].n; ++i, ++at) EXPECT(items[at].b == b && items[at].chunk == i, "video item order");
        EXPECT(at == items.size(), "video item count");
        for (const StreamItem& it : items) {
            const SlideOffVidRow& r = vr[it.b];
            const int64_t kk = it.chunk / SLIDE_OFF_VX, out = r.out0 + kk, j = r.j0 + kk;
            EXPECT(out >= 0 && out < n, "output window in range");
            // the utterance of global window w0 + out, by counting
            int64_t u = 0, w = w0 + out, so = 0;
            while (w >= bs[u].W) { w -= bs[u].W; so += S[u]; ++u; }
            EXPECT(w == j && so == r.s_off, "window %lld of the range is window %lld of utterance %lld", (long long)out, (long long)w,
                   (long long)u);
            EXPECT(((int64_t)s * j + F - 1) / F < S[u], "its last frame lies in the utterance");
            parts[out] |= 1 << (it.chunk % SLIDE_OFF_VX);
        }
        for (int v2 : parts) EXPECT(v2 == (1 << SLIDE_OFF_VX) - 1, "every part of every window once");
    };
    if (Wt <= 40) {
        for (int64_t w0 = 0; w0 <= Wt; ++w0)
            for (int64_t n = 0; w0 + n <= Wt; ++n) check_range(w0, n);
    } else {
        check_range(0, Wt);
        for (int k = 0; k < 12; ++k) {
            const int64_t w0 = rng() % (Wt + 1);
            check_range(w0, rng() % (Wt - w0 + 1));
        }
        for (int64_t w0 = 0; w0 < Wt; w0 += 7) check_range(w0, std::min<int64_t>(7, Wt - w0));
    }
    EXPECT(slide_off_video_plan(g, S.data(), U, Wt, 1, nullptr).status == SLIDE_OFF_BAD_RANGE, "a window past the list");
    EXPECT(slide_off_video_plan(g, S.data(), U, -1, 1, nullptr).status == SLIDE_OFF_BAD_RANGE, "a negative w0");
    EXPECT(slide_off_video_plan(g, S.data(), U, 0, -1, nullptr).status == SLIDE_OFF_BAD_RANGE, "a negative n");
}

static void check_refusals() {
    const int64_t S[3] = {2, 0, 3}, T[3] = {41, 1, 61};
    auto st = [&](SlideOffCfg g, const int64_t* s, const int64_t* t, int64_t U, int64_t* bad = nullptr) {
        const SlideOffPlan p = slide_off_plan(g, s, t, U, 80, nullptr);
        if (bad) *bad = p.bad;
        return p.status;
    };
    EXPECT(st({20, 5, 1}, S, T, 3) == SLIDE_OFF_OK, "the legal batch");
    EXPECT(st({20, 5, 1}, S, T, 0) == SLIDE_OFF_OK, "an empty batch");
    EXPECT(st({20, 5, 0}, S, T, 3) == SLIDE_OFF_BAD_STRIDE && st({20, 5, 6}, S, T, 3) == SLIDE_OFF_BAD_STRIDE &&
           st({20, 5, -1}, S, T, 3) == SLIDE_OFF_BAD_STRIDE && st({24, 6, 7}, S, T, 3) == SLIDE_OFF_BAD_STRIDE, "stride outside 1 .. F");
    EXPECT(st({20, 6, 1}, S, T, 3) == SLIDE_OFF_BAD_GEOM && st({0, 5, 1}, S, T, 3) == SLIDE_OFF_BAD_GEOM &&
           st({20, 0, 1}, S, T, 3) == SLIDE_OFF_BAD_GEOM && st({-20, 5, 1}, S, T, 3) == SLIDE_OFF_BAD_GEOM, "spf %% F");
    EXPECT(st({20, 5, 1}, S, T, -1) == SLIDE_OFF_BAD_COUNT, "n_utt < 0");
    int64_t bad = -7;
    const int64_t Sn[3] = {2, -1, 3}, Tn[3] = {41, 1, -61}, Ts[3] = {41, 1, 59};
    EXPECT(st({20, 5, 1}, Sn, T, 3, &bad) == SLIDE_OFF_BAD_COUNT && bad == 1, "S_u < 0");
    EXPECT(st({20, 5, 1}, S, Tn, 3, &bad) == SLIDE_OFF_BAD_COUNT && bad == 2, "T_u < 0");
    EXPECT(st({20, 5, 1}, S, Ts, 3, &bad) == SLIDE_OFF_SHORT && bad == 2, "T_u < q F S_u");
    EXPECT(st({20, 5, 1}, S, nullptr, 3) == SLIDE_OFF_OK, "n_frames NULL: T_u = q F S_u");
    // totals past the int32 limits: one utterance whose mel block passes 2^31 floats; a batch whose windows do
    const int64_t Sbig[1] = {(int64_t)1 << 21}, Sw[4] = {1 << 20, 1 << 20, 1 << 20, 1 << 20};
    EXPECT(st({20, 5, 1}, Sbig, nullptr, 1, &bad) == SLIDE_OFF_TOO_LARGE && bad == 0, "n_mels T past int32");
    const int64_t Sww[2] = {100000000, 100000000};      // 5e8 - 4 windows each: the second passes (2^31 - 1) / SLIDE_OFF_VX
    const SlideOffPlan pw = slide_off_plan({20, 5, 1}, Sww, nullptr, 2, 1, nullptr);
    EXPECT(pw.status == SLIDE_OFF_TOO_LARGE && pw.bad == 1, "VX x the windows of the batch past int32: %d", pw.status);
    EXPECT(slide_off_plan({20, 5, 1}, Sww, nullptr, 1, 1, nullptr).status == SLIDE_OFF_OK, "one of them alone fits");
    const SlideOffPlan ok = slide_off_plan({20, 5, 5}, Sw, nullptr, 4, 1, nullptr);
    EXPECT(ok.status == SLIDE_OFF_OK && ok.windows == 4 * ((int64_t)1 << 20) && ok.predicted == 20 * ok.windows, "stride F: a window per slice");
    EXPECT(slide_off_video_plan({5, 5, 0}, S, 3, 0, 0, nullptr).status == SLIDE_OFF_BAD_STRIDE, "the video plan checks the stride");
    EXPECT(slide_off_video_plan({5, 5, 1}, Sn, 3, 0, 0, nullptr).status == SLIDE_OFF_BAD_COUNT, "and the counts");
    for (int s2 = SLIDE_OFF_OK; s2 <= SLIDE_OFF_BAD_RANGE; ++s2) EXPECT(slide_off_message(s2)[0] != 0, "a message per status");
}

int main() {
    check_refusals();
    std::mt19937 rng(22);
    for (int F : {5, 6})
        for (int spf : {20, 24}) {
            if (spf % F) {
                const int64_t S1[1] = {1};
                EXPECT(slide_off_plan({spf, F, 1}, S1, nullptr, 1, 80, nullptr).status == SLIDE_OFF_BAD_GEOM, "spf %d F %d", spf, F);
                continue;
            }
            for (int s = 1; s <= F; ++s) {
                for (int64_t S = 0; S <= 16; ++S) check_batch(spf, F, s, {S}, 80);       // single utterances, S = 0 and 1 included
                check_batch(spf, F, s, {4, 2, 1}, 80);                                   // the GPU tests' batch
                check_batch(spf, F, s, {0, 1, 0, 3, 0}, 80);                             // empty utterances between others
                check_batch(spf, F, s, {14}, 80);                                        // 281 frames: two scan chunks
                check_batch(spf, F, s, {70, 1, 129}, 7);                                 // more kept columns than one keep block
                for (int k = 0; k < 6; ++k) {
                    std::vector<int64_t> S((size_t)(1 + rng() % 6));
                    for (auto& x : S) x = rng() % 9;
                    check_batch(spf, F, s, S, 80);
                }
            }
        }
    std::printf("ok %ld\n", checks);
    return 0;
}
