// Host-only tables of the evaluate stage (eval_tables.h).
#include "eval_tables.h"

#include <cmath>
#include <numeric>

namespace avse {

void eval_ratio(int sr, int* up, int* down) {
    const int g = std::gcd(kStoiFs, sr);
    *up = kStoiFs / g;
    *down = sr / g;
}

double bessel_i0(double x) {
    // sum_k ((x / 2)^2)^k / (k!)^2: every term positive, so the sum loses nothing to cancellation
    const double q = x * x / 4.0;
    double term = 1.0, total = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        total += term;
        if (term < total * 1e-17) break;
    }
    return total;
}

std::vector<double> resample_taps(int up, int down) {
    if (up == down) return {1.0};
    const int mx = up > down ? up : down;
    const int H = 10 * mx;
    const double fc = 1.0 / (double)mx;
    std::vector<double> h(2 * H + 1);
    const double i0b = bessel_i0(5.0);
    double sum = 0.0;
    for (int i = 0; i <= 2 * H; ++i) {
        const double t = (double)(i - H);
        const double a = M_PI * fc * t;
        const double sinc = i == H ? 1.0 : std::sin(a) / a;
        const double r = t / (double)H;
        const double arg = 1.0 - r * r;
        h[i] = fc * sinc * bessel_i0(5.0 * std::sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
        sum += h[i];
    }
    for (double& v : h) v = v / sum * (double)up;
    return h;
}

std::vector<double> resample_taps_by_phase(const std::vector<double>& h, int up) {
    const size_t last = h.size() - 1;            // 2H
    const size_t T = last / (size_t)up + 1;
    std::vector<double> rows((size_t)up * T);
    for (size_t phase = 0; phase < (size_t)up; ++phase)
        for (size_t q = 0; q < T; ++q) {
            const size_t i = phase + (size_t)up * (T - 1 - q);
            rows[phase * T + q] = i <= last ? h[i] : 0.0;
        }
    return rows;
}

std::vector<double> hann_inner(int n) {
    std::vector<double> w(n > 0 ? n : 0);
    for (int i = 0; i < n; ++i) w[i] = 0.5 * (1.0 - std::cos(2.0 * M_PI * (double)(i + 1) / (double)(n + 1)));
    return w;
}

std::vector<int> stoi_bands() {
    std::vector<int> b(2 * kStoiBands);
    const double df = (double)kStoiFs / (double)kStoiFft;
    for (int j = 0; j < kStoiBands; ++j) {
        const double cf = 150.0 * std::pow(2.0, (double)j / 3.0);
        const double edge[2] = {cf * std::pow(2.0, -1.0 / 6.0), cf * std::pow(2.0, 1.0 / 6.0)};
        for (int e = 0; e < 2; ++e) {
            int best = 0;
            double bd = -1.0;
            for (int k = 0; k <= kStoiFft / 2; ++k) {   // the first nearest bin, as numpy's argmin
                const double d = ((double)k * df - edge[e]) * ((double)k * df - edge[e]);
                if (bd < 0.0 || d < bd) { bd = d; best = k; }
            }
            b[2 * j + e] = best;
        }
    }
    return b;
}

std::vector<double> stoi_twiddle() {
    std::vector<double> t(kStoiFft);
    for (int k = 0; k < kStoiFft / 2; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)kStoiFft;
        t[2 * k] = std::cos(a);
        t[2 * k + 1] = std::sin(a);
    }
    return t;
}

int seg_snr_window(int sr) { return (3 * sr + 50) / 100; }   // round(0.03 sr), halves up, in integers

}  // namespace avse
