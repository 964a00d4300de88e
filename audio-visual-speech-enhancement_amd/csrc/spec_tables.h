// Host-only librosa-equivalent tables (no HIP header): double precision, rounded to float once.  capi.hip caches
// them per (sr, n_fft, n_mels, fmin, fmax) and uploads them (ensure_spec_tables, ensure_istft_tables).
#pragma once
#include <vector>

namespace avse {

// librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=False, norm=1) -> [n_mels][1 + n_fft / 2]
std::vector<double> mel_filterbank(int sr, int n_fft, int n_mels, double fmin, double fmax);

struct Cplx {   // the layout of HIP's float2
    float re, im;
};
// e^{-2 pi i k / n} and the periodic Hann window, k < n
struct DftTables {
    std::vector<Cplx> twiddle;
    std::vector<float> window;
};
DftTables dft_tables(int n);

// The filterbank as one run of non-zero bins per band (MelTable, ctx.h).
struct MelBands {
    int n_bins = 0, max_width = 0;
    std::vector<int> start, width;   // [n_mels]
    std::vector<float> weight;       // [n_mels][max_width]
    int seg_nq[4] = {}, seg_nq4[4] = {};
};
MelBands mel_bands(int sr, int n_fft, int n_mels, double fmin, double fmax);

struct MelBin {   // the layout of HIP's float4: the <= 2 adjacent filters j0, j0 + 1 covering a bin
    float w0, w1;
    int j0;
    float zero;
};
struct IstftHostTables {
    std::vector<float> pinvT;      // [n_mels][nb] pinv(mel)^T
    std::vector<MelBin> bins;      // [nb]; empty unless the bank is well conditioned with a tridiagonal Gram matrix
    std::vector<float> gram_inv;   // [n_mels][n_mels] (M M^T)^{-1}; only with bins and n_mels == 80
};
IstftHostTables istft_tables(int sr, int n_fft, int n_mels, double fmin, double fmax);

}  // namespace avse
