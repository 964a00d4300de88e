// Stand-alone check of csrc/ragged_geom.h (built with -fsanitize=address,undefined by tests/test_ragged_host.py):
// for a few length lists every table is compared with a brute-force definition that loops over utterance, frame and
// slice and counts.  Prints "ok <n checks>" and exits 0, or the first mismatch and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ragged_geom.h"

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

// centred frames by counting: frame t covers padded samples [t hop, t hop + n_fft) of L + 2 (n_fft / 2)
static int64_t frames_by_counting(int64_t L, int n_fft, int hop) {
    const int64_t padded = L + 2 * (n_fft / 2);
    int64_t t = 0;
    while (t * hop + n_fft <= padded) ++t;
    return t;
}

static void check_spec(const std::vector<int64_t>& lens, const std::vector<int64_t>& off, int n_fft, int hop, int spf,
                       int n_mels, int chunk) {
    const int64_t U = (int64_t)lens.size();
    const RaggedGeom g = ragged_spec_geom(off.data(), lens.data(), U, n_fft, hop, spf, n_mels, true, chunk);
    EXPECT(g.status == RAGGED_OK, "status %d", g.status);
    EXPECT((int64_t)g.utt.size() == U && (int64_t)g.n_chunks.size() == U, "sizes");
    const int64_t nb = n_fft / 2 + 1;
    std::vector<int64_t> owner;          // owner[i]: the utterance that writes mel element i
    std::vector<RaggedItem> items;
    int64_t mel = 0, stft = 0;
    std::vector<RaggedRun> runs;
    for (int64_t u = 0; u < U; ++u) {
        const int64_t T = frames_by_counting(lens[u], n_fft, hop);
        int64_t S = 0;
        if (spf > 0)
            while ((S + 1) * spf <= T) ++S;
        EXPECT(g.utt[u].T == T && g.utt[u].L == lens[u] && g.utt[u].in_off == off[u], "utt %lld T %d want %lld",
               (long long)u, g.utt[u].T, (long long)T);
        EXPECT(g.utt[u].S == S, "utt %lld S %d want %lld", (long long)u, g.utt[u].S, (long long)S);
        EXPECT(g.utt[u].mel_off == mel && g.utt[u].out_off == stft, "utt %lld offsets", (long long)u);
        EXPECT(g.utt[u].first_item == (int64_t)items.size(), "utt %lld first_item", (long long)u);
        int last_chunk = -1;
        for (int64_t t = 0; t < T; ++t) {
            const int c = (int)(t / chunk);
            if (c != last_chunk) items.push_back({(int32_t)u, c});
            last_chunk = c;
            for (int m = 0; m < n_mels; ++m)
                if (spf == 0 || t / spf < S) {
                    owner.push_back(u);
                    ++mel;
                }
            stft += nb;
        }
        EXPECT(g.n_chunks[u] == last_chunk + 1, "utt %lld chunks", (long long)u);
        if (u == 0 || lens[u] != lens[u - 1] || off[u] != off[u - 1] + lens[u - 1]) runs.push_back({u, 1});
        else ++runs.back().count;
    }
    EXPECT(g.mel_total == mel && g.out_total == stft, "totals %lld %lld", (long long)g.mel_total, (long long)mel);
    EXPECT(g.items.size() == items.size(), "items %zu want %zu", g.items.size(), items.size());
    for (size_t i = 0; i < items.size(); ++i)
        EXPECT(g.items[i].u == items[i].u && g.items[i].chunk == items[i].chunk, "item %zu", i);
    EXPECT(g.runs.size() == runs.size(), "runs %zu want %zu", g.runs.size(), runs.size());
    for (size_t i = 0; i < runs.size(); ++i)
        EXPECT(g.runs[i].first == runs[i].first && g.runs[i].count == runs[i].count, "run %zu", i);
    for (int64_t i = 0; i < mel; ++i)
        EXPECT(ragged_mel_utt(g.utt.data(), U, i) == owner[i], "element %lld owner", (long long)i);
}

static void check_istft(const std::vector<int64_t>& nf, const std::vector<int64_t>& sf, int spf, int nb, int hop,
                        int n_mels, int chunk) {
    const int64_t U = (int64_t)nf.size();
    const RaggedGeom g = ragged_istft_geom(nf.data(), sf.data(), U, spf, nb, hop, n_mels, chunk);
    EXPECT(g.status == RAGGED_OK, "status %d", g.status);
    int64_t mel = 0, stft = 0, out = 0;
    std::vector<RaggedItem> items;
    std::vector<RaggedRun> runs;
    for (int64_t u = 0; u < U; ++u) {
        EXPECT(g.utt[u].T == nf[u] && g.utt[u].L == sf[u], "utt %lld", (long long)u);
        EXPECT(g.utt[u].mel_off == mel && g.utt[u].in_off == stft && g.utt[u].out_off == out, "utt %lld offsets",
               (long long)u);
        EXPECT(g.utt[u].first_item == (int64_t)items.size(), "utt %lld first_item", (long long)u);
        int64_t S = 0;
        if (spf > 0)
            while ((S + 1) * spf <= nf[u]) ++S;
        EXPECT(g.utt[u].S == S, "utt %lld S", (long long)u);
        for (int64_t t = 0; t < nf[u]; ++t) mel += n_mels;
        for (int64_t t = 0; t < sf[u]; ++t) stft += nb;
        int last_chunk = -1;
        for (int64_t h = 0; h + 1 < nf[u]; ++h) {      // output hop h: samples [h hop, (h + 1) hop)
            const int c = (int)(h / chunk);
            if (c != last_chunk) items.push_back({(int32_t)u, c});
            last_chunk = c;
            out += hop;
        }
        EXPECT(g.n_chunks[u] == last_chunk + 1, "utt %lld chunks", (long long)u);
        if (u == 0 || nf[u] != nf[u - 1] || sf[u] != sf[u - 1]) runs.push_back({u, 1});
        else ++runs.back().count;
    }
    EXPECT(g.mel_total == mel && g.in_total == stft && g.out_total == out, "totals");
    EXPECT(g.items.size() == items.size(), "items %zu want %zu", g.items.size(), items.size());
    for (size_t i = 0; i < items.size(); ++i)
        EXPECT(g.items[i].u == items[i].u && g.items[i].chunk == items[i].chunk, "item %zu", i);
    EXPECT(g.runs.size() == runs.size(), "runs");
    for (size_t i = 0; i < runs.size(); ++i)
        EXPECT(g.runs[i].first == runs[i].first && g.runs[i].count == runs[i].count, "run %zu", i);
}

static std::vector<int64_t> packed(const std::vector<int64_t>& lens) {
    std::vector<int64_t> off(lens.size());
    int64_t o = 0;
    for (size_t u = 0; u < lens.size(); ++u) {
        off[u] = o;
        o += lens[u];
    }
    return off;
}
static std::vector<int64_t> rows(const std::vector<int64_t>& lens, int64_t stride) {
    std::vector<int64_t> off(lens.size());
    for (size_t u = 0; u < lens.size(); ++u) off[u] = (int64_t)u * stride;
    return off;
}

int main() {
    // 640 / 160: one chunk, under a chunk (zero slices at spf 20), one frame into a second chunk, three chunks, odd
    const std::vector<int64_t> a = {3200, 400, 3360, 6721, 4799, 16000, 3200};
    for (int spf : {0, 20}) {
        check_spec(a, packed(a), 640, 160, spf, 80, 21);
        check_spec(a, rows(a, 16000), 640, 160, spf, 80, 21);
    }
    // a one-frame utterance (reflect needs L > n_fft / 2: 4 samples at n_fft 6), zero slices, n_utt = 1, equal lengths
    const std::vector<int64_t> tiny = {4, 5, 9, 4, 4};
    check_spec(tiny, packed(tiny), 6, 5, 2, 3, 2);        // T = 1, 2, 2, 1, 1
    check_spec(tiny, packed(tiny), 6, 5, 0, 3, 1);
    check_spec({3200}, {7}, 640, 160, 20, 80, 21);
    const std::vector<int64_t> eq(7, 3200);
    check_spec(eq, packed(eq), 640, 160, 20, 80, 21);     // one run
    check_spec(eq, rows(eq, 4000), 640, 160, 20, 80, 21); // strided rows: seven runs of one
    const std::vector<int64_t> b = {3192, 3325, 8000, 1000, 3193, 3326};
    check_spec(b, packed(b), 533, 133, 24, 80, 25);
    check_spec(b, packed(b), 533, 133, 0, 17, 25);
    const std::vector<int64_t> c = {3000, 3000, 4200, 3000};
    check_spec(c, packed(c), 600, 150, 0, 80, 1 << 30);

    check_istft({20, 31, 32, 40, 100, 1}, {21, 32, 33, 41, 101, 2}, 0, 321, 160, 80, 30);
    check_istft({20, 40, 100, 0, 20, 20}, {21, 41, 101, 3, 21, 21}, 20, 321, 160, 80, 30);
    check_istft({24, 48, 24}, {25, 49, 25}, 24, 267, 133, 80, 1 << 30);
    check_istft({61}, {61}, 0, 321, 160, 80, 30);
    check_istft({2, 2, 2}, {2, 2, 2}, 1, 4, 1, 2, 1);

    // refusals
    {
        const int64_t off[2] = {0, 100}, neg[2] = {100, -1}, zero[2] = {100, 0}, shortl[2] = {321, 320}, big[2] = {100, 1LL << 31};
        EXPECT(ragged_spec_geom(off, neg, 2, 640, 160, 0, 80, false, 21).status == RAGGED_BAD_COUNT, "negative");
        EXPECT(ragged_spec_geom(off, zero, 2, 640, 160, 0, 80, false, 21).status == RAGGED_BAD_COUNT, "zero");
        const RaggedGeom r = ragged_spec_geom(off, shortl, 2, 640, 160, 0, 80, true, 21);
        EXPECT(r.status == RAGGED_REFLECT_SHORT && r.bad_utt == 1, "reflect");
        EXPECT(ragged_spec_geom(off, shortl, 2, 640, 160, 0, 80, false, 21).status == RAGGED_OK, "constant pad");
        EXPECT(ragged_spec_geom(off, big, 2, 640, 160, 0, 80, false, 21).status == RAGGED_TOO_LARGE, "2^31 samples");
        const int64_t nf[2] = {20, 30}, sf[2] = {21, 31}, sf_short[2] = {21, 29}, nneg[2] = {20, -1};
        EXPECT(ragged_istft_geom(nf, sf, 2, 20, 321, 160, 80, 30).status == RAGGED_NOT_SLICED, "slices");
        EXPECT(ragged_istft_geom(nf, sf_short, 2, 0, 321, 160, 80, 30).status == RAGGED_PAST_STFT, "past stft");
        EXPECT(ragged_istft_geom(nneg, sf, 2, 0, 321, 160, 80, 30).status == RAGGED_BAD_COUNT, "negative frames");
        const int64_t huge[1] = {1LL << 40};
        EXPECT(ragged_istft_geom(huge, huge, 1, 0, 321, 160, 80, 30).status == RAGGED_TOO_LARGE, "huge");
        // items past int32: 2^12 utterances of 2^20 one-hop chunks each
        std::vector<int64_t> many(1 << 12, (1LL << 20) + 1);
        EXPECT(ragged_istft_geom(many.data(), many.data(), (int64_t)many.size(), 0, 2, 1, 1, 1).status == RAGGED_TOO_LARGE,
               "items past int32");
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
