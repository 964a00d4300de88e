// Stand-alone check of csrc/retime_geom.h (built with AddressSanitizer / UndefinedBehaviorSanitizer by
// tests/test_retime_host.py): random per-stream schedules run through retime_rows / retime_commit and a host copy of
// k_retime's per-block work with one pixel per frame, on arrays of exactly the sizes the library allocates, against the
// definition evaluated on each stream's whole sequence of frames.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "retime_geom.h"

using namespace avse;

static long long g_checks = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        ++g_checks;                                                               \
        if (!(cond)) {                                                            \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            return 1;                                                             \
        }                                                                         \
    } while (0)

// the uint8 definition on one pixel
static int blend(int a, int b, int64_t q, int64_t r) { return r == 0 ? a : (int)((2 * (a * (q - r) + b * r) + q) / (2 * q)); }

static int define(const RetimeCfg& g, const std::vector<int>& x, int64_t j) {
    const int64_t c = j * g.p, i0 = c / g.q, r = c % g.q, n = (int64_t)x.size();
    return blend(x[(size_t)i0], x[(size_t)std::min(i0 + 1, n - 1)], g.q, r);
}

struct Device {   // what the retimer owns on the device, one pixel per frame
    std::vector<int> hist;   // [2][B]
    std::vector<int> pend;   // [2][B][F]
};

// k_retime's grid on the host; `reverse` runs the blocks backwards (the order must not matter: a call reads one copy
// and writes the other)
static int run_blocks(const RetimeCfg& g, Device& d, const std::vector<RetimeRow>& rows, int64_t blocks,
                      const std::vector<int>& news, std::vector<int>& out, int64_t cap, bool reverse) {
    const int B = (int)rows.size(), F = g.F;
    for (int64_t n = 0; n < blocks; ++n) {
        const int blk = (int)(reverse ? blocks - 1 - n : n);
        const int b = retime_row_of(rows.data(), B, blk);
        const RetimeRow& r = rows[(size_t)b];
        CHECK(blk >= r.blk0 && blk < r.blk0 + retime_row_blocks(g, r));
        const int local = blk - r.blk0, slot = local / g.tiles, tile = local % g.tiles;
        CHECK(slot < retime_row_slots(r));
        if (tile != 0) continue;   // the tiles differ in their pixels only
        const bool hist_job = r.fed && slot == retime_row_slots(r) - 1;
        CHECK(hist_job || slot < r.n_slots);
        auto frame = [&](int64_t i, bool* bad) {
            int64_t idx = -1;
            switch (retime_source(r, i, &idx)) {
                case RETIME_HIST: return d.hist[(size_t)r.hist_in * B + b];
                case RETIME_NEW:
                    if (idx < 0 || idx >= (int64_t)news.size()) { *bad = true; return 0; }
                    return news[(size_t)idx];
                default: *bad = true; return 0;
            }
        };
        bool bad = false;
        if (hist_job) {   // the last slot: the call's last frame into the other copy
            CHECK(r.hist_out != r.hist_in);
            d.hist[(size_t)r.hist_out * B + b] = frame(r.n_new - 1, &bad);
            CHECK(!bad);
        }
        if (slot >= r.n_slots) continue;
        const int64_t j0 = (r.g_old / F + slot) * F;
        const int n_pend = slot == 0 ? (int)(r.g_old - j0) : 0;
        const int n_valid = (int)std::min<int64_t>(F, r.g_new - j0);
        CHECK(n_pend >= 0 && n_pend < F && n_valid > 0 && n_pend <= n_valid);
        std::vector<int> w((size_t)F, -1);
        for (int f = 0; f < n_pend; ++f) w[(size_t)f] = d.pend[((size_t)r.hist_in * B + b) * F + f];
        for (int f = n_pend; f < n_valid; ++f) {
            int64_t i0, i1;
            int32_t rr;
            retime_taps(g.p, g.q, r.n_new, j0 + f, &i0, &i1, &rr);
            CHECK(i0 >= r.n_old - 1 && i0 < r.n_new && i1 >= i0 && i1 < r.n_new && rr >= 0 && rr < g.q);
            if (!r.flush && rr) CHECK(i1 == i0 + 1);   // a final frame never clamps
            const int a = frame(i0, &bad), c = rr ? frame(i1, &bad) : a;
            w[(size_t)f] = blend(a, c, g.q, rr);
        }
        CHECK(!bad);
        const bool complete = slot < r.k_new;
        CHECK(complete == (n_valid == F) || r.flush);
        if (complete) {
            CHECK(n_valid == F && r.out_slice + slot < cap);
            for (int f = 0; f < F; ++f) out[(size_t)(r.out_slice + slot) * F + f] = w[(size_t)f];
        } else {
            CHECK(!r.flush && r.fed && slot == r.n_slots - 1 && r.hist_out != r.hist_in);
            for (int f = 0; f < F; ++f) d.pend[((size_t)r.hist_out * B + b) * F + f] = w[(size_t)f];
        }
    }
    return 0;
}

static int brute_counts(const RetimeCfg& g) {
    // G(n): the outputs j with ceil(j p / q) <= n - 1; flushed: those with j p < n q
    for (int64_t n = 0; n <= 300; ++n) {
        int64_t k = 0, kf = 0;
        while (n > 0 && (k * g.p + g.q - 1) / g.q <= n - 1) ++k;
        while (kf * g.p < n * g.q) ++kf;
        CHECK(retime_total(g, n, false) == k);
        CHECK(retime_total(g, n, true) == kf);
        CHECK(k <= kf);
        CHECK(retime_slices(g, n, true) == kf / g.F);
        // the clamped frames all sit on the last input
        for (int64_t j = k; j < kf; ++j) CHECK(j * g.p / g.q == n - 1 && j * g.p % g.q > 0);
    }
    return 0;
}

static int schedule(int64_t in_num, int64_t in_den, int64_t out_num, int64_t out_den, int F, int tiles, uint32_t seed) {
    RetimeCfg g;
    CHECK(retime_cfg(in_num, in_den, out_num, out_den, &g) == RETIME_OK);
    g.F = F;
    g.tiles = tiles;
    if (brute_counts(g)) return 1;
    std::mt19937 rng(seed);
    const int B = 1 + (int)(rng() % 4);
    Device d;
    d.hist.assign((size_t)2 * B, -1000000);   // stale state must never be read
    d.pend.assign((size_t)2 * B * F, -1000000);
    std::vector<RetimeState> st((size_t)B, RetimeState{0, 0, 0});
    std::vector<std::vector<int>> x((size_t)B), y((size_t)B);
    std::vector<RetimeRow> rows((size_t)B);
    const int calls = 14;
    for (int call = 0; call <= calls; ++call) {
        std::vector<int64_t> n_new((size_t)B), off((size_t)B);
        std::vector<uint8_t> flush((size_t)B);
        std::vector<int> news;
        for (int b = 0; b < B; ++b) {
            const int64_t pick[] = {0, 1, 1, 2, F - 1, F, F + 1, 3 * F + 2, 37, 0};
            int64_t dn = pick[rng() % 10];
            const bool last = call == calls;
            bool fl = last || rng() % 11 == 0;
            if (st[(size_t)b].flushed) { dn = 0; fl = false; }
            if (last) dn = 0;
            n_new[(size_t)b] = dn;
            flush[(size_t)b] = fl;
            off[(size_t)b] = (int64_t)news.size();
            for (int64_t i = 0; i < dn; ++i) {
                news.push_back((int)(rng() % 256));
                x[(size_t)b].push_back(news.back());
            }
        }
        // the slices the call will complete, and an `out` of exactly that many
        int64_t cap = 0;
        std::vector<int64_t> want_k((size_t)B);
        for (int b = 0; b < B; ++b) {
            const RetimeState& s = st[(size_t)b];
            want_k[(size_t)b] = retime_slices(g, s.n + n_new[(size_t)b], s.flushed || flush[(size_t)b]) - retime_slices(g, s.n, s.flushed);
            cap += want_k[(size_t)b];
        }
        const std::vector<RetimeState> before = st;
        // refusals: each leaves the states as they were
        if (cap > 0) {
            RetimePlan p = retime_rows(g, st.data(), B, off.data(), n_new.data(), flush.data(), true, cap - 1, rows.data());
            CHECK(p.status == RETIME_OUT_SMALL && p.bad >= 0 && p.bad < B && want_k[(size_t)p.bad] > 0);
            p = retime_rows(g, st.data(), B, off.data(), n_new.data(), flush.data(), false, cap, rows.data());
            CHECK(p.status == RETIME_OUT_SMALL);
        }
        {
            std::vector<int64_t> neg = n_new;
            neg[(size_t)(B - 1)] = -1;
            RetimePlan p = retime_rows(g, st.data(), B, off.data(), neg.data(), flush.data(), true, cap, rows.data());
            CHECK(p.status == RETIME_BAD_COUNT && p.bad == B - 1);
            std::vector<int64_t> big = n_new;
            big[0] = RETIME_MAX_TOTAL + 1 - st[0].n;
            if (!st[0].flushed) {
                p = retime_rows(g, st.data(), B, off.data(), big.data(), flush.data(), true, cap, rows.data());
                CHECK(p.status == RETIME_TOO_LARGE && p.bad == 0);
            }
            for (int b = 0; b < B; ++b)
                if (st[(size_t)b].flushed) {
                    std::vector<int64_t> more = n_new;
                    more[(size_t)b] = 1;
                    p = retime_rows(g, st.data(), B, off.data(), more.data(), nullptr, true, cap + 8, rows.data());
                    CHECK(p.status == RETIME_AFTER_FLUSH && p.bad <= b);
                    std::vector<uint8_t> again((size_t)B, 0);
                    again[(size_t)b] = 1;
                    p = retime_rows(g, st.data(), B, off.data(), n_new.data(), again.data(), true, cap + 8, rows.data());
                    CHECK(p.status == RETIME_AFTER_FLUSH);
                }
        }
        CHECK(std::memcmp(before.data(), st.data(), sizeof(RetimeState) * (size_t)B) == 0);
        const RetimePlan p = retime_rows(g, st.data(), B, off.data(), n_new.data(), flush.data(), true, cap, rows.data());
        CHECK(p.status == RETIME_OK && p.slices == cap);
        int64_t blocks = 0, first = 0;
        for (int b = 0; b < B; ++b) {
            const RetimeRow& r = rows[(size_t)b];
            CHECK(r.blk0 == blocks && r.out_slice == first && r.k_new == want_k[(size_t)b]);
            blocks += retime_row_blocks(g, r);
            first += r.k_new;
            if (n_new[(size_t)b] == 0 && !flush[(size_t)b]) CHECK(retime_row_blocks(g, r) == 0);   // idle: no blocks
        }
        CHECK(blocks == p.blocks);
        std::vector<int> out((size_t)(cap * F), -1);
        if (run_blocks(g, d, rows, blocks, news, out, cap, (call & 1) != 0)) return 1;
        retime_commit(rows.data(), B, st.data());
        for (int b = 0; b < B; ++b) {
            const RetimeRow& r = rows[(size_t)b];
            CHECK((int64_t)y[(size_t)b].size() == r.g_old / F * F);
            for (int64_t i = 0; i < (int64_t)r.k_new * F; ++i) y[(size_t)b].push_back(out[(size_t)(r.out_slice * F + i)]);
            CHECK(st[(size_t)b].n == (int64_t)x[(size_t)b].size());
            if (r.fed) CHECK(d.hist[(size_t)r.hist_out * B + b] == x[(size_t)b].back());
        }
    }
    for (int b = 0; b < B; ++b) {
        const int64_t n = (int64_t)x[(size_t)b].size();
        CHECK(st[(size_t)b].flushed);
        const int64_t total = n == 0 ? 0 : (n * g.q + g.p - 1) / g.p;
        CHECK((int64_t)y[(size_t)b].size() == total / F * F);   // all calls plus the flush; the remainder dropped
        for (int64_t j = 0; j < (int64_t)y[(size_t)b].size(); ++j) CHECK(y[(size_t)b][(size_t)j] == define(g, x[(size_t)b], j));
    }
    return 0;
}

int main() {
    RetimeCfg g;
    CHECK(retime_cfg(0, 1, 25, 1, &g) == RETIME_BAD_RATE);
    CHECK(retime_cfg(30, 1, 25, -1, &g) == RETIME_BAD_RATE);
    CHECK(retime_cfg(30, 0, 25, 1, &g) == RETIME_BAD_RATE);
    CHECK(retime_cfg(65537, 1, 1, 1, &g) == RETIME_RATIO && g.p == 65537 && g.q == 1);
    CHECK(retime_cfg(65536, 1, 1, 1, &g) == RETIME_OK && g.p == 65536 && g.q == 1);
    CHECK(retime_cfg(30, 1, 25, 1, &g) == RETIME_OK && g.p == 6 && g.q == 5);
    CHECK(retime_cfg(30000, 1001, 25, 1, &g) == RETIME_OK && g.p == 1200 && g.q == 1001);
    CHECK(retime_cfg(2997, 100, 25, 1, &g) == RETIME_OK && g.p == 2997 && g.q == 2500);
    CHECK(retime_cfg(25, 1, 25, 1, &g) == RETIME_OK && g.p == 1 && g.q == 1);
    const int64_t pairs[][4] = {{30, 1, 25, 1}, {30000, 1001, 25, 1}, {2997, 100, 25, 1}, {15, 1, 25, 1}, {60, 1, 25, 1},
                                {24, 1, 25, 1}, {25, 1, 30, 1}, {5, 1, 4, 1}, {2, 1, 1, 1}, {25, 1, 25, 1}, {1, 1, 7, 1}};
    uint32_t seed = 1;
    for (const auto& p : pairs)
        for (int rep = 0; rep < 4; ++rep)
            if (schedule(p[0], p[1], p[2], p[3], rep & 1 ? 6 : 5, rep & 2 ? 4 : 16, seed++)) return 1;
    std::printf("ok %lld\n", g_checks);
    return 0;
}
