// Host-only check of the forward plan (csrc/forward_plan.h): prints, for every recorded combination of network shape,
// dtype, gemm_ksplit_cap and batch, the arena size and offsets and the split-K plans of layers 10-13 (one row of
// integers each; tests/test_forward_plan_host.py compares them with tests/golden/forward_plan.json), and asserts on
// every row that the arena is well formed, that the workspace holds the partials of the plan each layer can take, and
// that a k_gemm split plan is one launch_gemm accepts.
#include <cstdio>

#include "../../audio-visual-speech-enhancement_amd/csrc/forward_plan.h"

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
    const int plans[5][2] = {{20, 5}, {24, 5}, {24, 6}, {4, 1}, {64, 8}};
    const int dtypes[3] = {AVSE_F32, AVSE_BF16, AVSE_F32_SPLIT};
    const long long Ns[11] = {1, 2, 3, 37, 127, 128, 129, 512, 4096, 41856, 41857};
    for (const auto& pl : plans) {
        EXPECT(plan_valid(pl[0], pl[1]));
        const ArenaShape shape = arena_shape(make_plan(pl[0], pl[1]));
        for (int dt : dtypes)
            for (int cap : {0, 1})
                for (long long N : Ns) {
                    Options o;
                    o.gemm_ksplit_cap = cap;
                    size_t off[B_COUNT + 1];
                    const size_t total = arena_bytes(N, dt, o, off, shape);
                    EXPECT(total == arena_bytes(N, dt, o, nullptr, shape));
                    std::printf("%d %d %d %d %lld %zu", pl[0], pl[1], dt, cap, N, total);
                    for (int b = 0; b <= B_COUNT; ++b) {
                        std::printf(" %zu", off[b]);
                        EXPECT(off[b] % 256 == 0);
                        EXPECT(b == 0 ? off[b] == 0 : off[b] > off[b - 1]);
                    }
                    EXPECT(total % 256 == 0 && total >= off[B_COUNT]);
                    const size_t ws = total - off[B_COUNT];
                    for (const SplitLayer& l : shape.split) {
                        const SplitPlan p = split_plan(l, N, dt, o);
                        std::printf(" %d %d %d %d", p.conv.ksplit, p.conv.slabs, p.gemm.ksplit, p.gemm.slabs);
                        const long long M = N * l.rows;
                        // the layer runs on k_gemm when the dtype has one and its tickets fit, else on k_conv
                        // (Options::no_gemm takes k_conv whenever: its partials fit as well)
                        const bool on_gemm = p.gemm.ksplit > 0 && gemm_tickets_fit(M, l.Co, p.gemm.ksplit, kGemmCounters);
                        EXPECT(ws >= (on_gemm ? p.gemm.bytes : p.conv.bytes));
                        EXPECT(ws >= p.conv.bytes);
                        EXPECT((p.conv.bytes > 0) == (p.conv.ksplit > 1) && (p.gemm.bytes > 0) == (p.gemm.ksplit > 1));
                        EXPECT(p.conv.ksplit >= 1 && (dt == AVSE_F32 ? p.gemm.ksplit == 0 : p.gemm.ksplit >= 1));
                        if (dt == AVSE_F32_SPLIT && p.gemm.ksplit > 1) {   // launch_gemm's conditions on a split plan
                            const int nslab = l.kpad / 16;
                            EXPECT(p.gemm.slabs > 0 && p.gemm.slabs % kFp32Block == 0);
                            EXPECT((nslab + p.gemm.slabs - 1) / p.gemm.slabs == p.gemm.ksplit);
                        }
                        if (dt != AVSE_BF16 && p.conv.ksplit > 1) {   // k_conv: whole fp32 blocks that cover the slabs
                            const int nslab = l.kpad / 16, slabs = p.conv.slabs ? p.conv.slabs : kFp32Block;
                            EXPECT(slabs % kFp32Block == 0 && (nslab + slabs - 1) / slabs == p.conv.ksplit);
                        }
                    }
                    std::printf("\n");
                }
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
