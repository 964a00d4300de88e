// Stand-alone check of the large-ratio resampling tables (csrc/eval_tables.cpp resample_taps_by_phase), built with
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_eval_ext_host.py.  For each (up, down) it builds the
// taps and their by-phase copy and walks the copy with k_eval_resample_big's index arithmetic (eval.hip) for outputs at
// the start, in the middle and at the end of a signal: every table read goes through the heap block the sanitizer
// guards, and each output must equal, bit for bit, the header's sum over h[H + k down - j up] in ascending j.
// Prints one JSON object: per ratio the geometry, the worst difference, the table's zeros and sampled taps; for
// (100, 441) the whole table.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../audio-visual-speech-enhancement_amd/csrc/eval_tables.h"

static double sample(int64_t j) { return (double)((j * 2654435761LL) % 2001 - 1000); }   // fixed integers in [-1000, 1000]

int main() {
    using namespace avse;
    const int ratios[6][2] = {{100, 441}, {200, 441}, {400, 441}, {10000, 16001}, {10000, 47999}, {10000, 8001}};
    std::printf("{\n");
    for (int r = 0; r < 6; ++r) {
        const int up = ratios[r][0], down = ratios[r][1];
        const std::vector<double> h = resample_taps(up, down);
        const std::vector<double> rows = resample_taps_by_phase(h, up);
        const int64_t H = ((int64_t)h.size() - 1) / 2;
        const int T = (int)(2 * H / up) + 1;
        const int64_t n = 20000;                                   // input samples
        const int64_t n10 = (n * up + down - 1) / down;
        double worst = 0.0;
        int64_t checked = 0;
        for (int64_t k = 0; k < n10; k += (k < 300 || k + 300 >= n10) ? 1 : 37) {
            // the kernel's walk
            const int64_t c = H + k * down;
            const int64_t B = c / up;
            const int phase = (int)(c - B * up);
            const double* hp = rows.data() + (size_t)phase * T;
            double a = 0.0;
            for (int q = 0; q < T; ++q) {
                const int64_t j = B - (T - 1) + q;
                a += hp[q] * (j >= 0 && j < n ? sample(j) : 0.0);
            }
            // the definition
            double b = 0.0;
            for (int64_t j = 0; j < n; ++j) {
                const int64_t i = H + k * down - j * up;
                if (i >= 0 && i <= 2 * H) b += h[(size_t)i] * sample(j);
            }
            const double d = a > b ? a - b : b - a;
            if (d > worst) worst = d;
            ++checked;
        }
        size_t zeros = 0;
        for (double v : rows) zeros += v == 0.0;
        std::printf("\"%d_%d\": {\"H\": %lld, \"T\": %d, \"rows\": %zu, \"zeros\": %zu, \"checked\": %lld, \"worst\": %.17g,\n",
                    up, down, (long long)H, T, rows.size(), zeros, (long long)checked, worst);
        std::printf("  \"taps_every_1009\": [");
        for (size_t i = 0; i < h.size(); i += 1009) std::printf("%s%.17g", i ? ", " : "", h[i]);
        std::printf("]");
        if (r == 0) {
            std::printf(",\n  \"table\": [");
            for (size_t i = 0; i < rows.size(); ++i) std::printf("%s%.17g", i ? ", " : "", rows[i]);
            std::printf("],\n  \"taps\": [");
            for (size_t i = 0; i < h.size(); ++i) std::printf("%s%.17g", i ? ", " : "", h[i]);
            std::printf("]");
        }
        std::printf("}%s\n", r < 5 ? "," : "");
    }
    std::printf("}\n");
    return 0;
}
