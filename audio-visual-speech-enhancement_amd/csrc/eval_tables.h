// Host-only tables of the evaluate stage (avse_eval_pairs, include/avse.h; no HIP header): double precision
// throughout.  capi.hip caches them per sample rate and uploads them (ensure_eval_tables).
#pragma once
#include <vector>

namespace avse {

constexpr int kStoiFs = 10000;       // STOI's sample rate
constexpr int kStoiFrame = 256;      // frame length, hop kStoiFrame / 2
constexpr int kStoiFft = 512;
constexpr int kStoiBands = 15;       // third-octave bands from 150 Hz
constexpr int kStoiSegment = 30;     // frames per intermediate-intelligibility segment
constexpr int kEvalMaxRatio = 24;    // max(up, down) up to which the taps fit in LDS; above it STOI needs AVSE_EVAL_ANY_RATE

// up / down = (10000 / g) / (sr / g), g = gcd(10000, sr)
void eval_ratio(int sr, int* up, int* down);

// Modified Bessel function of the first kind, order 0 (power series; x >= 0)
double bessel_i0(double x);

// scipy.signal.resample_poly's default filter: h[i] = up fc sinc(fc (i - H)) I0(5 sqrt(1 - ((i - H) / H)^2)) / I0(5),
// i = 0 .. 2H, H = 10 max(up, down), fc = 1 / max(up, down), normalised so that sum(h) / up == 1.
// up == down: the single tap {1.0} (a copy).
std::vector<double> resample_taps(int up, int down);

// The taps h[0 .. 2H] (resample_taps, up != down) by phase: [up][T], T = 2H / up + 1.  Row `phase` holds the taps
// h[phase + i up] in DESCENDING i: entry q is h[phase + (T - 1 - q) up], or 0 where that index passes 2H (entry 0 of
// the rows with phase > 2H mod up).  An output whose tap indices are congruent to `phase` reads its row front to back
// while its input samples ascend (eval.hip k_eval_resample_big).
std::vector<double> resample_taps_by_phase(const std::vector<double>& h, int up);

// W[i] = 0.5 (1 - cos(2 pi (i + 1) / (n + 1))), i < n: STOI's frame window (n = 256) and the segmental SNR's
std::vector<double> hann_inner(int n);

// [2 kStoiBands]: lo_j, hi_j, the half-open bin range of band j — the bins nearest to 150 2^(j/3) 2^(-+1/6) Hz on the
// grid of 10000 / 512 Hz
std::vector<int> stoi_bands();

// e^{-2 pi i k / 512}, k < 256, as (re, im) pairs
std::vector<double> stoi_twiddle();

// round(0.03 sr): the segmental SNR's frame length (the hop is a quarter of it, as an integer)
int seg_snr_window(int sr);

}  // namespace avse
