// Host-only check of k_gemm's split-K ticket bound (csrc/layer_geom.h gemm_tickets_fit, kGemmCounters): a launch the
// bound accepts indexes no ticket past the array (tile = blockIdx.y * gridDim.x + blockIdx.x, gemm.hip), the bound
// turns exactly where the tile count passes the array, and unsplit launches (which take no ticket) always fit.
#include <cstdio>

#include "../../audio-visual-speech-enhancement_amd/csrc/layer_geom.h"

using namespace avse;

static int fails = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            ++fails;                                                     \
        }                                                                \
    } while (0)

int main() {
    // the dense layers of the three shipped audio geometries (T = 20, 24 at W5 = 5, 6; T = 64: W5 = 16)
    for (int T : {20, 24, 64}) {
        const NetPlan p = make_plan(T, 5);
        for (int N : {p.emb, p.aemb}) {
            const long long tn = (N + 127) / 128;
            const long long rows_fit = kGemmCounters / tn;   // row tiles that still fit
            long long first_bad = -1;
            for (long long M = 1; M <= (rows_fit + 2) * 128; M += (M % 128 == 0 || M % 128 == 127) ? 1 : 63) {
                const bool fit = gemm_tickets_fit(M, N, 2, kGemmCounters);
                const long long last_tile = (tn - 1) * ((M + 127) / 128) + (M + 127) / 128 - 1;
                EXPECT(fit == (last_tile < kGemmCounters));
                if (!fit && first_bad < 0) first_bad = M;
                EXPECT(gemm_tickets_fit(M, N, 1, kGemmCounters));   // no split: no ticket
                EXPECT(gemm_tickets_fit(M, N, 1, 0));
            }
            EXPECT(first_bad == rows_fit * 128 + 1);
            std::printf("T=%d N=%d: %lld column tiles, first batch declined %lld\n", T, N, tn, first_bad);
        }
    }
    // dec_dense2 at the 25-fps plan: 25 column tiles, 327 row tiles fit
    EXPECT(gemm_tickets_fit(327 * 128, 3200, 3, kGemmCounters));
    EXPECT(!gemm_tickets_fit(327 * 128 + 1, 3200, 3, kGemmCounters));
    EXPECT(!gemm_tickets_fit(1LL << 40, 3200, 3, kGemmCounters));   // no int overflow
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
