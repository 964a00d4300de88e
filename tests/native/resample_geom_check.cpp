// Stand-alone check of csrc/resample_geom.h (built with AddressSanitizer / UndefinedBehaviorSanitizer by
// tests/test_resample_host.py): random per-stream schedules run through resample_rows / resample_commit and a host
// copy of the kernel's per-block work, on arrays of exactly the sizes the library allocates, against the definition
// evaluated on each stream's whole signal.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "eval_tables.h"
#include "resample_geom.h"

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

// the definition: y[k] = sum_j h[H + k down - j up] x[j], ascending j, over the whole signal
static float define(const ResampleCfg& g, const std::vector<double>& h, const std::vector<float>& x, int64_t k) {
    if (g.H == 0) return x[(size_t)k];
    double acc = 0.0;
    // only the j near (k down) / up can keep the tap index in range: the others are skipped without being visited
    const int64_t mid = k * g.down / g.up, reach = 2 * (int64_t)g.H / g.up + 2;
    for (int64_t j = std::max<int64_t>(0, mid - reach); j < std::min<int64_t>((int64_t)x.size(), mid + reach + 1); ++j) {
        const int64_t i = (int64_t)g.H + k * g.down - j * g.up;
        if (i < 0 || i > 2 * (int64_t)g.H) continue;
        acc = std::fma(h[(size_t)i], (double)x[(size_t)j], acc);
    }
    return (float)acc;
}

struct Device {   // what the resampler owns on the device
    std::vector<float> hist;      // [2][B][T]
    std::vector<double> ptaps;    // [up][T]
};

// sample j of row r's stream; every index is range-checked by the vectors' sizes under ASan through data() + i
static float sample(const ResampleCfg& g, const Device& d, const ResampleRow& r, int B, int b, const std::vector<float>& news,
                    int64_t j, bool* bad) {
    int64_t i = 0;
    switch (resample_source(r, g.T, j, &i)) {
        case RESAMPLE_HIST:
            if (i < 0 || i >= g.T) { *bad = true; return 0.f; }
            return d.hist[((size_t)r.hist_in * B + b) * g.T + (size_t)i];
        case RESAMPLE_NEW:
            if (r.sample_off + i < 0 || r.sample_off + i >= (int64_t)news.size()) { *bad = true; return 0.f; }
            return news[(size_t)(r.sample_off + i)];
        default: return 0.f;
    }
}

// k_resample's grid on the host: outputs first, then the history blocks (the order must not matter: they touch
// different copies), `reverse` runs the blocks backwards to show it
static int run_blocks(const ResampleCfg& g, Device& d, const std::vector<ResampleRow>& rows, int64_t blocks,
                      const std::vector<float>& news, std::vector<float>& out, int64_t out_stride, bool reverse) {
    const int B = (int)rows.size();
    bool bad = false;
    for (int64_t n = 0; n < blocks; ++n) {
        const int blk = (int)(reverse ? blocks - 1 - n : n);
        const int b = resample_row_of(rows.data(), B, blk);
        const ResampleRow& r = rows[(size_t)b];
        CHECK(blk >= r.blk0 && blk < r.blk0 + resample_row_blocks(r));
        const int chunk = blk - r.blk0;
        const int nout_blocks = (r.n_out + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK;
        if (chunk >= nout_blocks) {
            CHECK(r.fed && r.hist_out != r.hist_in);
            for (int i = 0; i < g.T; ++i)
                d.hist[((size_t)r.hist_out * B + b) * g.T + i] = sample(g, d, r, B, b, news, r.n_new - g.T + i, &bad);
            continue;
        }
        for (int t = 0; t < RESAMPLE_BLOCK; ++t) {
            const int i = chunk * RESAMPLE_BLOCK + t;
            if (i >= r.n_out) break;
            const int64_t k = r.k0 + i;
            CHECK(r.out_off == (int64_t)b * out_stride && i < out_stride);
            float y;
            if (g.H == 0) {
                y = sample(g, d, r, B, b, news, k, &bad);
            } else {
                const int64_t c = (int64_t)g.H + k * g.down, Bk = c / g.up;
                const int phase = (int)(c - Bk * g.up);
                double acc = 0.0;
                for (int q = 0; q < g.T; ++q) {
                    const int64_t j = Bk - (g.T - 1) + q;
                    // the guard of resample_source never fires for a sample the sum needs
                    if (j >= 0 && j < r.n_old) CHECK(j >= r.n_old - g.T);
                    if (!r.flush) CHECK(j < r.n_new);
                    acc = std::fma(d.ptaps[(size_t)phase * g.T + q], (double)sample(g, d, r, B, b, news, j, &bad), acc);
                }
                y = (float)acc;
            }
            out[(size_t)(r.out_off + i)] = y;
        }
    }
    CHECK(!bad);
    return 0;
}

static int brute_counts(const ResampleCfg& g) {
    // F(n): the outputs k with floor((H + k down) / up) < n
    for (int64_t n = 0; n <= 700; ++n) {
        int64_t k = 0;
        while (((int64_t)g.H + k * g.down) / g.up < n) ++k;
        if (g.H == 0) k = n;
        CHECK(resample_total(g, n, false) == k);
        CHECK(resample_total(g, n, true) == (n * g.up + g.down - 1) / g.down);
        CHECK(resample_total(g, n, false) <= resample_total(g, n, true));
    }
    return 0;
}

static int schedule(int sr_in, int sr_out, uint32_t seed) {
    ResampleCfg g;
    CHECK(resample_cfg(sr_in, sr_out, &g) == RESAMPLE_OK);
    if (brute_counts(g)) return 1;
    std::mt19937 rng(seed);
    const int B = 1 + (int)(rng() % 4);
    const std::vector<double> h = resample_taps(g.up, g.down);
    Device d;
    d.ptaps = resample_taps_by_phase(h, g.up);
    CHECK((int)d.ptaps.size() == g.up * g.T && (int)h.size() == 2 * g.H + 1);
    d.hist.assign((size_t)2 * B * g.T, 1e30f);   // a stale history must never be read
    std::vector<ResampleState> st((size_t)B, ResampleState{0, 0, 0});
    std::vector<std::vector<float>> x((size_t)B), y((size_t)B);
    std::vector<ResampleRow> rows((size_t)B);
    std::uniform_real_distribution<float> val(-30000.f, 30000.f);
    const int calls = 12;
    for (int call = 0; call <= calls; ++call) {
        std::vector<int64_t> n_new((size_t)B), off((size_t)B);
        std::vector<uint8_t> flush((size_t)B);
        std::vector<float> news;
        for (int b = 0; b < B; ++b) {
            // chunks shorter than, equal to and longer than T, single samples, idle calls
            const int64_t pick[] = {0, 1, g.T - 1, g.T, g.T + 1, 3 * g.T + 7, 997, 0};
            int64_t dn = pick[rng() % 8];
            const bool last = call == calls;
            bool fl = last || rng() % 9 == 0;
            if (st[(size_t)b].flushed) { dn = 0; fl = false; }
            if (last) dn = 0;
            n_new[(size_t)b] = dn;
            flush[(size_t)b] = fl;
            off[(size_t)b] = (int64_t)news.size();
            for (int64_t i = 0; i < dn; ++i) {
                news.push_back(std::round(val(rng)));
                x[(size_t)b].push_back(news.back());
            }
        }
        // the counts the call will give, and a stride of exactly the largest
        int64_t stride = 0;
        for (int b = 0; b < B; ++b) {
            const ResampleState& s = st[(size_t)b];
            stride = std::max(stride, resample_total(g, s.n + n_new[(size_t)b], s.flushed || flush[(size_t)b]) -
                                          resample_total(g, s.n, s.flushed));
        }
        const std::vector<ResampleState> before = st;
        // refusals: each leaves the states as they were
        if (stride > 0) {
            ResamplePlan p = resample_rows(g, st.data(), B, off.data(), n_new.data(), flush.data(), true, stride - 1, rows.data());
            CHECK(p.status == RESAMPLE_OUT_SMALL && p.bad >= 0 && p.bad < B);
            p = resample_rows(g, st.data(), B, off.data(), n_new.data(), flush.data(), false, stride, rows.data());
            CHECK(p.status == RESAMPLE_OUT_SMALL);
        }
        {
            std::vector<int64_t> neg = n_new;
            neg[(size_t)(B - 1)] = -1;
            ResamplePlan p = resample_rows(g, st.data(), B, off.data(), neg.data(), flush.data(), true, stride, rows.data());
            CHECK(p.status == RESAMPLE_BAD_COUNT && p.bad == B - 1);
            for (int b = 0; b < B; ++b)
                if (st[(size_t)b].flushed) {
                    std::vector<int64_t> more = n_new;
                    more[(size_t)b] = 1;
                    p = resample_rows(g, st.data(), B, off.data(), more.data(), nullptr, true, stride + 1, rows.data());
                    CHECK(p.status == RESAMPLE_AFTER_FLUSH && p.bad <= b);
                    std::vector<uint8_t> again((size_t)B, 0);
                    again[(size_t)b] = 1;
                    p = resample_rows(g, st.data(), B, off.data(), n_new.data(), again.data(), true, stride + 1, rows.data());
                    CHECK(p.status == RESAMPLE_AFTER_FLUSH);
                }
        }
        CHECK(std::memcmp(before.data(), st.data(), sizeof(ResampleState) * (size_t)B) == 0);
        const ResamplePlan p = resample_rows(g, st.data(), B, off.data(), n_new.data(), flush.data(), true, stride, rows.data());
        CHECK(p.status == RESAMPLE_OK && p.max_n_out == stride);
        int64_t blocks = 0;
        for (int b = 0; b < B; ++b) {
            CHECK(rows[(size_t)b].blk0 == blocks);
            blocks += resample_row_blocks(rows[(size_t)b]);
            if (n_new[(size_t)b] == 0 && !flush[(size_t)b]) CHECK(resample_row_blocks(rows[(size_t)b]) == 0);   // idle: no blocks
        }
        CHECK(blocks == p.blocks);
        std::vector<float> out((size_t)(B * stride), -1.f);
        if (run_blocks(g, d, rows, blocks, news, out, stride, (call & 1) != 0)) return 1;
        resample_commit(rows.data(), B, st.data());
        for (int b = 0; b < B; ++b) {
            const ResampleRow& r = rows[(size_t)b];
            CHECK((int64_t)y[(size_t)b].size() == r.k0);
            for (int i = 0; i < r.n_out; ++i) y[(size_t)b].push_back(out[(size_t)(r.out_off + i)]);
            CHECK(st[(size_t)b].n == (int64_t)x[(size_t)b].size());
            // the history copy the call wrote: the last T samples, zeros before the signal's start
            if (r.fed)
                for (int i = 0; i < g.T; ++i) {
                    const int64_t j = r.n_new - g.T + i;
                    const float want = j < 0 ? 0.f : x[(size_t)b][(size_t)j];
                    const float have = d.hist[((size_t)r.hist_out * B + b) * g.T + i];
                    CHECK(std::memcmp(&want, &have, 4) == 0);
                }
        }
    }
    for (int b = 0; b < B; ++b) {
        const int64_t n = (int64_t)x[(size_t)b].size();
        CHECK(st[(size_t)b].flushed);
        CHECK((int64_t)y[(size_t)b].size() == (n * g.up + g.down - 1) / g.down);   // all calls plus the flush
        for (int64_t k = 0; k < (int64_t)y[(size_t)b].size(); ++k) {
            const float want = define(g, h, x[(size_t)b], k);
            CHECK(std::memcmp(&want, &y[(size_t)b][(size_t)k], 4) == 0);
        }
    }
    return 0;
}

int main() {
    ResampleCfg g;
    CHECK(resample_cfg(0, 16000, &g) == RESAMPLE_BAD_RATE);
    CHECK(resample_cfg(16000, -1, &g) == RESAMPLE_BAD_RATE);
    CHECK(resample_cfg(16001, 16000, &g) == RESAMPLE_RATIO && g.up == 16000 && g.down == 16001);
    CHECK(resample_cfg(16000, 16000, &g) == RESAMPLE_OK && g.up == 1 && g.down == 1 && g.H == 0 && g.T == 1);
    CHECK(resample_cfg(44100, 16000, &g) == RESAMPLE_OK && g.up == 160 && g.down == 441 && g.T == 56);
    CHECK(resample_cfg(16000, 44100, &g) == RESAMPLE_OK && g.T == 21);
    CHECK(resample_cfg(11025, 16000, &g) == RESAMPLE_OK && g.up == 640 && g.T == 21);
    CHECK(resample_cfg(16000, 11025, &g) == RESAMPLE_OK && g.T == 30);
    CHECK(resample_cfg(44100, 24000, &g) == RESAMPLE_OK && g.up == 80 && g.T == 37);
    const int pairs[][2] = {{44100, 16000}, {16000, 44100}, {11025, 16000}, {16000, 11025}, {44100, 24000}, {8000, 16000},
                            {96000, 16000}, {16000, 16000}, {22050, 16000}, {48000, 44100}};
    uint32_t seed = 1;
    for (const auto& p : pairs)
        for (int rep = 0; rep < 3; ++rep)
            if (schedule(p[0], p[1], seed++)) return 1;
    std::printf("ok %lld\n", g_checks);
    return 0;
}
