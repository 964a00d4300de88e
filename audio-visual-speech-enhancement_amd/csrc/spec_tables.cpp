// Host-only librosa-equivalent tables (spec_tables.h).
#include "spec_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace avse {

namespace {
double hz_to_mel(double f) {  // Slaney (htk=False)
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
    const double logstep = std::log(6.4) / 27.0;
    if (f >= min_log_hz) return min_log_mel + std::log(f / min_log_hz) / logstep;
    return f / f_sp;
}
double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
    const double logstep = std::log(6.4) / 27.0;
    if (m >= min_log_mel) return min_log_hz * std::exp(logstep * (m - min_log_mel));
    return f_sp * m;
}
}  // namespace

// librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=False, norm=1) -> [n_mels][n_bins] (double)
std::vector<double> mel_filterbank(int sr, int n_fft, int n_mels, double fmin, double fmax) {
    const int nb = 1 + n_fft / 2;
    std::vector<double> w((size_t)n_mels * nb, 0.0);
    std::vector<double> fftf(nb), melf(n_mels + 2);
    for (int k = 0; k < nb; ++k) fftf[k] = (nb == 1) ? 0.0 : (double)k * ((double)sr / 2) / (double)(nb - 1);
    const double lo = hz_to_mel(fmin), hi = hz_to_mel(fmax);
    for (int i = 0; i < n_mels + 2; ++i) melf[i] = mel_to_hz(lo + (hi - lo) * (double)i / (double)(n_mels + 1));
    for (int i = 0; i < n_mels; ++i) {
        const double d0 = melf[i + 1] - melf[i], d1 = melf[i + 2] - melf[i + 1];
        const double enorm = 2.0 / (melf[i + 2] - melf[i]);
        for (int k = 0; k < nb; ++k) {
            const double lower = -(melf[i] - fftf[k]) / d0;
            const double upper = (melf[i + 2] - fftf[k]) / d1;
            double v = std::fmin(lower, upper);
            if (v < 0) v = 0;
            w[(size_t)i * nb + k] = v * enorm;
        }
    }
    return w;
}

DftTables dft_tables(int n) {
    DftTables t;
    t.twiddle.resize(n);
    t.window.resize(n);
    for (int k = 0; k < n; ++k) {
        const double ang = -2.0 * M_PI * (double)k / (double)n;
        t.twiddle[k] = Cplx{(float)std::cos(ang), (float)std::sin(ang)};
        t.window[k] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)k / (double)n));
    }
    return t;
}

MelBands mel_bands(int sr, int n_fft, int n_mels, double fmin, double fmax) {
    MelBands t;
    const int nb = 1 + n_fft / 2;
    std::vector<double> fb = mel_filterbank(sr, n_fft, n_mels, fmin, fmax);
    std::vector<int> st(n_mels), wd(n_mels);
    int maxw = 1;
    for (int m = 0; m < n_mels; ++m) {
        int lo = -1, hi = -1;
        for (int k = 0; k < nb; ++k)
            if (fb[(size_t)m * nb + k] > 0) { if (lo < 0) lo = k; hi = k; }
        // bands start at an even bin (a leading zero weight when the first non-zero bin is odd): the STFT kernels
        // read a band's magnitudes as 8-B pairs (half the LDS instructions and bank-conflict cycles of 4-B reads)
        lo = lo < 0 ? -1 : (lo & ~1);
        st[m] = lo < 0 ? 0 : lo;
        wd[m] = lo < 0 ? 0 : hi - lo + 1;
        if (wd[m] > maxw) maxw = wd[m];
    }
    if (maxw <= 24) maxw = 24;   // rows padded to the STFT kernel's compile-time band width (16-B staging copies)
    std::vector<float> wt((size_t)n_mels * maxw, 0.f);
    for (int m = 0; m < n_mels; ++m)
        for (int j = 0; j < wd[m]; ++j) wt[(size_t)m * maxw + j] = (float)fb[(size_t)m * nb + st[m] + j];
    // k_spec_seg's mel pass j covers items 64 j .. 64 j + 63 = bands (item / 3): the widest of those bands (aligned
    // start) in 4-bin quads; the rows stay padded to maxw, so a pass reads only the quads its bands can use
    for (int j = 0; j < 4; ++j) {
        int w = 0;
        for (int it = 64 * j; it < 64 * j + 64 && it / 3 < n_mels; ++it) w = std::max(w, wd[it / 3]);
        t.seg_nq[j] = std::min((w + 3) / 4, maxw / 4);
        // k_spec_seg reads 16-B quads from 4-aligned band starts (st & ~3: a further 0 or 2 leading zero weights)
        int w4 = 0;
        for (int it = 64 * j; it < 64 * j + 64 && it / 3 < n_mels; ++it) w4 = std::max(w4, (st[it / 3] & 3) + wd[it / 3]);
        t.seg_nq4[j] = std::min((w4 + 3) / 4, (maxw + 4) / 4);
    }
    t.n_bins = nb;
    t.max_width = maxw;
    t.start = st;
    t.width = wd;
    t.weight = wt;
    return t;
}

// pinv(mel) as np.linalg.pinv computes it (data_processor.py:112): from the singular value decomposition, dropping
// the singular values at or below 1e-15 of the largest.  The reference's own banks are full row rank (cond ~4.5), for
// which this is M^T (M M^T)^{-1}; a bank with more bands than the bins can tell apart is not (n_fft 401 with 80 bands:
// an FFT bin lands on a band edge and leaves singular values of 3e-6 and 2e-20 of the largest), and there the
// Gram-matrix inverse this replaced followed the dropped direction (waveform 7e-4 from the oracle's).
// One-sided Jacobi (Hestenes) on the rows of M, in double: plane rotations J make the rows of A = J M mutually
// orthogonal, so sigma_i = |a_i|, M = J^T diag(sigma) (a_i / sigma_i) and pinv(M)[k][m] = sum_i a_i[k] J[i][m] /
// sigma_i^2 over the kept i.  Small singular values come out to high relative accuracy.
IstftHostTables istft_tables(int sr, int n_fft, int n_mels, double fmin, double fmax) {
    IstftHostTables t;
    const int nb = 1 + n_fft / 2;
    const std::vector<double> M = mel_filterbank(sr, n_fft, n_mels, fmin, fmax);
    std::vector<double> A(M), J((size_t)n_mels * n_mels, 0.0);
    for (int i = 0; i < n_mels; ++i) J[(size_t)i * n_mels + i] = 1.0;
    // 5-8 sweeps for a full-rank bank; the rounding noise of a zero direction keeps rotating until the cap
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n_mels - 1; ++p)
            for (int q = p + 1; q < n_mels; ++q) {
                double* ap = &A[(size_t)p * nb];
                double* aq = &A[(size_t)q * nb];
                double alpha = 0, beta = 0, gamma = 0;
                for (int k = 0; k < nb; ++k) {
                    alpha += ap[k] * ap[k];
                    beta += aq[k] * aq[k];
                    gamma += ap[k] * aq[k];
                }
                if (std::fabs(gamma) <= 1e-15 * std::sqrt(alpha * beta)) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double az = std::fabs(zeta);   // (zeta^2 overflows past 1e154: tan = 1 / (2 zeta) there)
                const double tn = az > 1e100 ? 0.5 / zeta : (zeta >= 0 ? 1.0 : -1.0) / (az + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + tn * tn), sn = cs * tn;
                for (int k = 0; k < nb; ++k) {
                    const double x = ap[k], y = aq[k];
                    ap[k] = cs * x - sn * y;
                    aq[k] = sn * x + cs * y;
                }
                double* jp = &J[(size_t)p * n_mels];
                double* jq = &J[(size_t)q * n_mels];
                for (int m = 0; m < n_mels; ++m) {
                    const double x = jp[m], y = jq[m];
                    jp[m] = cs * x - sn * y;
                    jq[m] = sn * x + cs * y;
                }
            }
        if (!rotated) break;
    }
    std::vector<double> sig2(n_mels);
    double smax2 = 0;
    for (int i = 0; i < n_mels; ++i) {
        double a2 = 0;
        for (int k = 0; k < nb; ++k) a2 += A[(size_t)i * nb + k] * A[(size_t)i * nb + k];
        sig2[i] = a2;
        smax2 = std::max(smax2, a2);
    }
    // pinv[k][m] = sum_i a_i[k] J[i][m] / sigma_i^2 over sigma_i > 1e-15 sigma_max; stored transposed [m][k]
    std::vector<float> pinvT((size_t)n_mels * nb);
    for (int m = 0; m < n_mels; ++m)
        for (int k = 0; k < nb; ++k) {
            double sum = 0;
            for (int i = 0; i < n_mels; ++i)
                if (sig2[i] > 1e-30 * smax2) sum += A[(size_t)i * nb + k] * J[(size_t)i * n_mels + m] / sig2[i];
            pinvT[(size_t)m * nb + k] = (float)sum;
        }
    t.pinvT = pinvT;
    // Tridiagonal form for the fused kernel: every bin covered by at most two filters j0, j0 + 1 => M M^T
    // has no entry beyond the first off-diagonals, and pinv(M) a = M^T y with (M M^T) y = a (Thomas, no
    // pivoting: the Gram matrix is symmetric positive definite).
    {
        // (only for a well-conditioned bank, cond < 1e6: the Gram solve squares the condition number)
        bool ok = *std::min_element(sig2.begin(), sig2.end()) > 1e-12 * smax2;
        std::vector<MelBin> bins(nb);
        for (int k = 0; k < nb && ok; ++k) {
            int j0 = -1, cnt = 0;
            for (int j = 0; j < n_mels; ++j)
                if (M[(size_t)j * nb + k] != 0.0) {
                    if (j0 < 0) j0 = j;
                    else if (j != j0 + 1) ok = false;
                    ++cnt;
                }
            if (cnt > 2) ok = false;
            const float w0 = j0 >= 0 ? (float)M[(size_t)j0 * nb + k] : 0.f;
            const float w1 = (j0 >= 0 && j0 + 1 < n_mels) ? (float)M[(size_t)(j0 + 1) * nb + k] : 0.f;
            bins[k] = MelBin{w0, w1, j0, 0.f};
        }
        if (ok) {
            auto gram = [&](int i, int j) {
                double acc = 0;
                for (int k = 0; k < nb; ++k) acc += M[(size_t)i * nb + k] * M[(size_t)j * nb + k];
                return acc;
            };
            // M M^T must be tridiagonal (adjacent Slaney triangles overlap, nothing else does) and its LU pivots
            // non-zero: the checks that make M^T (M M^T)^{-1} = pinv(M) computable from the band-local pieces
            double cprev = 0;
            for (int i = 0; i < n_mels && ok; ++i) {
                for (int j = 0; j < i - 1 && ok; ++j)
                    if (gram(i, j) != 0.0) ok = false;
                const double ai = i > 0 ? gram(i, i - 1) : 0.0, bi = gram(i, i);
                const double ci = i + 1 < n_mels ? gram(i, i + 1) : 0.0;
                const double piv = bi - ai * cprev;
                if (!(std::fabs(piv) > 1e-300)) { ok = false; break; }
                cprev = ci / piv;
            }
            if (ok) {
                t.bins = bins;
                if (n_mels == 80) {
                    // (M M^T)^{-1} by Gauss-Jordan in double (the Gram matrix is symmetric positive definite, cond ~20):
                    // the fused kernel solves all frames of a chunk at once as a [frames x 80] x [80 x 80] fp32 MFMA
                    // product (round 2: one Thomas recurrence per frame and lane)
                    const int n = n_mels;
                    std::vector<double> g((size_t)n * n), inv((size_t)n * n, 0.0);
                    for (int i = 0; i < n; ++i) {
                        inv[(size_t)i * n + i] = 1.0;
                        for (int j = std::max(0, i - 1); j <= std::min(n - 1, i + 1); ++j) g[(size_t)i * n + j] = gram(i, j);
                    }
                    for (int c = 0; c < n && ok; ++c) {
                        const double piv = g[(size_t)c * n + c];
                        if (!(std::fabs(piv) > 1e-300)) { ok = false; break; }
                        for (int j = 0; j < n; ++j) { g[(size_t)c * n + j] /= piv; inv[(size_t)c * n + j] /= piv; }
                        for (int r = 0; r < n; ++r) {
                            if (r == c) continue;
                            const double f = g[(size_t)r * n + c];
                            if (f == 0.0) continue;
                            for (int j = 0; j < n; ++j) {
                                g[(size_t)r * n + j] -= f * g[(size_t)c * n + j];
                                inv[(size_t)r * n + j] -= f * inv[(size_t)c * n + j];
                            }
                        }
                    }
                    if (ok) t.gram_inv.assign(inv.begin(), inv.end());
                }
            }
        }
    }
    return t;
}

}  // namespace avse
