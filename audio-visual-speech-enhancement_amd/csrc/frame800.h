// Per-frame arithmetic of the 800-point streaming kernels (30-fps video: n_fft 800 at 24 kHz, 1600 at 48 kHz), beside
// frame640.h / frame_poly.h.  A frame of N = 800 P samples (P = 1, 2) whose spectrum is band-limited to bins 0 .. 266
// (the 30-Hz bins up to 7980 Hz: all the Slaney bank and its pseudo-inverse touch at these rates) is P interleaved
// 800-point frames and a twiddle combine.  With xw the windowed frame, W_N = e^{-2 pi i / N}, F_r = DFT800(xw[r::P]):
//
//   analysis   X[k] = sum_{r < P} W_N^{r k} F_r[k],  k <= 266
//   synthesis  irfft(Z, N)[P m + r] = (1 / P) irfft800(Y_r)[m],  Y_r[k] = Z[k] W_N^{-r k},  Z zero above bin 266
//              (bin 266 lies below the 800-point Nyquist bin 400: no Nyquist term, unlike the 640-point form)
//
// A real 800-point frame is the packed 400-point complex transform of z[n] = x[2n] + i x[2n+1], and 400 = 20 x 20:
// n = n1 + 20 n2, k = k2 + 20 k1, both steps the 20-point butterfly of fft_common.h (pk_dft20 / dft20).
//
//   spec800   the analysis side: lanes (frame, n1 < 20), three frames per wave (60 of 64 lanes); step 1 (window,
//             20-point DFT over n2, twiddle W400^{n1 k2}), step 2 (20-point DFT over n1), the untangling of the pairs
//             (k, 400 - k), k <= 200, and step 3 of a phase into register accumulators.  |X|, the band dots, dB and
//             the frame maximum are spec640's (pk_abs, band_dot_nq, mel_to_db)
//   istft800  the synthesis side: one block's <= 3 frames, as istft640::synth_frames (the sources and the sink passed
//             in); the overlap-add is istft640::ola_sample
//
// LDS frame slot: 20 rows of 21 float2 (row k2 at 21 k2), ZS = 420.  Against the bank model (ds_write_b64: groups of 16
// contiguous lanes, bank = dword mod 32; ds_read_b64: groups of 32 lanes, bank = dword mod 64): the stores of steps 1
// and 2 write f ZS + const + n (n the lane's 0 .. 19): a 16-lane group holds parts of at most two frames, and
// 2 ZS = 8 (mod 32) dwords puts the second frame's run behind the first's, so no two lanes of a group share a bank;
// the step-2 loads read f ZS + 21 k2 + n: 42 k2 (mod 64) are 20 distinct even banks, and the frames' offsets 2 ZS = 8,
// 4 ZS = 16 (mod 64) interleave them without a collision in either 32-lane group.  What remains: the step-3 reads
// zf[400 - k] (descending, an odd offset against zf[k]: 2-way where a 32-lane group straddles two frames) and the
// magnitude stores mf[400 - k] (ds_write_b32 beside mf[k] of the next item: 2-way at the straddles).
#pragma once
#include "frame640.h"

namespace avse {
namespace spec800 {

using spec640::FPG;   // frames per wave
using spec640::MW;
constexpr int ZS = 420;          // float2 slots per frame in LDS (20 rows x 21)
constexpr int RS = 21;           // row stride
constexpr int M = 400;           // the packed transform's length
constexpr int KH = 200;          // untangling pairs (k, M - k), k <= KH
constexpr int KTOP = 266;        // last bin the bank and its pseudo-inverse touch
constexpr int IT3 = (FPG * (KH + 1) + 63) / 64;   // step-3 items (frame, k <= 200) per lane: 10

// lane (f1, n1) of step 1, phase r: z_r[j] = (x[s0 + P 2j + r], x[s0 + P (2j + 1) + r]), j = n1 + 20 n2,
// from a frame that lies whole in one buffer (p = its sample s0) ...
template <int P>
__device__ __forceinline__ void load_phase(float2 (&x)[20], const float* __restrict__ p, int n1, int r) {
    p += 2 * P * n1 + r;
#pragma unroll
    for (int n2 = 0; n2 < 20; ++n2) x[n2] = make_float2(p[40 * P * n2], p[40 * P * n2 + P]);
}
// ... or sample by sample (sample(i): sample i of the padded signal)
template <int P, class Sample>
__device__ __forceinline__ void load_phase(float2 (&x)[20], Sample sample, long long s0, int n1, int r) {
#pragma unroll
    for (int n2 = 0; n2 < 20; ++n2) {
        const long long i = s0 + 2 * P * (n1 + 20 * n2) + r;
        x[n2] = make_float2(sample(i), sample(i + P));
    }
}

// the window of phase r as the pairs window_frame reads: pair j = (w[P 2j + r], w[P (2j + 1) + r]), j < 400
template <int P>
__device__ __forceinline__ float2 window_pair(const float* __restrict__ window, int r, int j) {
    return make_float2(window[2 * P * j + r], window[2 * P * j + P + r]);
}

// ---- step 1, lane (frame, n1): the Hann window on the loaded pairs, then the 20-point DFT over n2 and the twiddle
// W400^{n1 k2} = W800^{2 n1 k2} (2 n1 k2 <= 722) into the frame's LDS rows zf[k2 * 21 + n1] ----
__device__ __forceinline__ void window_frame(v2f (&v)[20], const float2 (&x)[20], const float2* winl, int n1) {
#pragma unroll
    for (int n2 = 0; n2 < 20; ++n2) {
        const float2 w = winl[n1 + 20 * n2];
        v[n2] = v2f{x[n2].x, x[n2].y} * v2f{w.x, w.y};
    }
}
__device__ __forceinline__ void dft20_store(v2f (&v)[20], const float2* twl, float2* zframe, int n1) {
    pk_dft20(v);
    // v[5c + d] = Y[c + 4d]
    v2f* zf = reinterpret_cast<v2f*>(zframe);
    const v2f* twv = reinterpret_cast<const v2f*>(twl);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            const int k2 = c + 4 * d;
            v2f y = v[5 * c + d];
            if (k2) y = pk_cmul_t(y, twv[2 * n1 * k2]);
            zf[k2 * RS + n1] = y;
        }
}
// ---- step 2, lane (frame, k2): the 20-point DFT over n1 -> Z[k2 + 20 k1].  Every lane's row is read before any lane
// stores (the caller synchronises between the two halves): the stores land in other lanes' rows ----
__device__ __forceinline__ void row_load(v2f (&w)[20], const v2f* zf, int k2) {
#pragma unroll
    for (int n = 0; n < 20; ++n) w[n] = zf[k2 * RS + n];
}
__device__ __forceinline__ void row_store(v2f (&w)[20], v2f* zf, int k2) {
    pk_dft20(w);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int d = 0; d < 5; ++d) zf[k2 + 20 * (c + 4 * d)] = w[5 * c + d];
}

// real-FFT untangling of the packed 400-point transform Z of one frame, as spec640::pk_untangle:
// X = X[k], Y = conj X[400 - k] from Z[k], Z[400 - k]; U = -i W800^k / 2 (a float2 table, k <= 200)
__device__ __forceinline__ void pk_untangle(const v2f* __restrict__ zf, int k, const v2f* __restrict__ ut, v2f& X, v2f& Y) {
    const v2f zk = zf[k], zm = zf[k == 0 ? 0 : M - k];
    const v2f S = pk_add_conj(zk, zm);
    const v2f WO = pk_cmul_t(pk_sub_conj(zk, zm), ut[k]);
    X = __builtin_elementwise_fma(v2f(0.5f), S, WO);
    Y = __builtin_elementwise_fma(v2f(0.5f), S, -WO);
}

// Step 3 of phase r for this lane's items (f, k <= 200) of the wave's ng frames: F_r[k] and F_r[400 - k] from the
// untangling of the frame's packed transform in zw, times W_N^{r k} and W_N^{r (400 - k)}, into ax (X[k]) and ay
// (X[400 - k]).  twN: W_N^j, j <= 400 (P - 1).
template <int P>
__device__ __forceinline__ void accumulate(v2f (&ax)[IT3], v2f (&ay)[IT3], const float2* zw, const v2f* ut2,
                                           const float2* __restrict__ twN, int r, int ng, int lane) {
#pragma unroll
    for (int j = 0; j < IT3; ++j) {
        const int it = lane + 64 * j;
        if (it >= ng * (KH + 1)) break;
        const int f = it / (KH + 1), k = it - (KH + 1) * f;
        v2f X, Y;
        pk_untangle(reinterpret_cast<const v2f*>(zw + f * ZS), k, ut2, X, Y);
        const v2f Xm = v2f{Y.x, -Y.y};   // F_r[400 - k] = conj(Y)
        if (r == 0) {
            ax[j] = X;
            ay[j] = Xm;
        } else {
            const float2 wk = twN[r * k], wm = twN[r * (M - k)];
            ax[j] += pk_cmul_t(X, v2f{wk.x, wk.y});
            ay[j] += pk_cmul_t(Xm, v2f{wm.x, wm.y});
        }
    }
}

}  // namespace spec800

namespace istft800 {

using istft640::FPG;
constexpr int ZS = spec800::ZS;
constexpr int RS = spec800::RS;
constexpr int M = spec800::M;
constexpr int NB = spec800::KTOP + 1;   // bins 0 .. 266

// istft640::synth_frames for frames of N = 800 P samples: a.twiddle is W_N^k and a.window the window, both [N];
// a.pinvT has a.nb = N / 2 + 1 columns of which 0 .. 266 are read; stft(k, f), k <= 266; frame(f) is where the frame's
// N windowed samples go.  Amplitudes, the pinv product and the unit phase once per frame; then per phase r the fold of
// Y_r into the 400-point complex sequence, the in-register inverse (conj(DFT(conj Z)) / 400), 1 / P, phase r of the
// window, and the store to samples P m + r.
template <int P, class MelDb, class Stft, class Frame>
__device__ __forceinline__ void synth_frames(const IstftArgs& a, int ng, MelDb mel_db, Stft stft, Frame frame) {
    __shared__ float amp[FPG][80];
    __shared__ float2 xb[FPG][M + 4];             // X[k], k <= 400: zero above bin 266
    __shared__ float2 zbuf[FPG * ZS];
    __shared__ float2 tw[800];                    // W800^k = W_N^{P k}
    const int lane = threadIdx.x;
    const float2* __restrict__ twN = a.twiddle;   // W_N^k

    for (int i = lane; i < 800; i += 64) tw[i] = twN[P * i];
    for (int it = lane; it < ng * a.n_mels; it += 64) {
        const int f = it / a.n_mels, m = it - f * a.n_mels;
        amp[f][m] = sqrtf(exp10f(0.1f * mel_db(m, f)));
    }
    __syncthreads();
    for (int it = lane; it < ng * (M + 1); it += 64) {
        const int f = it / (M + 1), k = it - f * (M + 1);
        float2 x = make_float2(0.f, 0.f);
        if (k < NB) {
            x = istft640::spectrum_bin(a.pinvT, a.n_mels, a.nb, amp[f], k, stft(k, f));
            if (k == 0) x.y = 0.f;                    // irfft ignores the DC imaginary part
        }
        xb[f][k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < P; ++r) {
        // fold Y_r into Z'[k] = conj(E[k] + i O[k]), k in [0,400), as istft640 does with X:
        //   E = (Y[k] + conj Y[400-k]) / 2,  O = (Y[k] - conj Y[400-k]) W800^{-k} / 2
        // (r (400 - k) <= 400 (P - 1): inside the table; bins above 266 are zero whatever their twiddle)
        for (int it = lane; it < ng * M; it += 64) {
            const int f = it / M, k = it - f * M;
            float2 xk = xb[f][k], xm = xb[f][M - k];
            if (r) {
                xk = cmul(xk, cconj(twN[r * k]));
                xm = cmul(xm, cconj(twN[r * (M - k)]));
            }
            xm = cconj(xm);
            const float2 E = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y + xm.y));
            const float2 O = cmul(make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y - xm.y)), cconj(tw[k]));
            const float2 Z = make_float2(E.x - O.y, E.y + O.x);   // E + i O
            zbuf[f * ZS + k] = cconj(Z);
        }
        __syncthreads();
        // forward 400-point DFT of Z': lane = (f, n1) in step 1 (20-point over n2 of z[n1 + 20 n2]) and (f, k2) in
        // step 2 (20-point over n1); lanes 60 .. 63 idle
        const int f = lane / 20, n1 = lane - 20 * (lane / 20);
        const bool act = f < ng;
        float2 v[20];
        if (act) {
#pragma unroll
            for (int n2 = 0; n2 < 20; ++n2) v[n2] = zbuf[f * ZS + n1 + 20 * n2];
        }
        __syncthreads();
        if (act) {
            dft20<40>(v, tw);
            float2* zf = zbuf + f * ZS;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int d = 0; d < 5; ++d) {
                    const int k2 = c + 4 * d;
                    float2 y = v[5 * c + d];
                    if (k2) y = cmul(y, tw[2 * n1 * k2]);
                    zf[k2 * RS + n1] = y;
                }
        }
        __syncthreads();
        if (act) {
            const int k2 = n1;
            const float2* zf = zbuf + f * ZS;
#pragma unroll
            for (int n = 0; n < 20; ++n) v[n] = zf[k2 * RS + n];
            dft20<40>(v, tw);
            float* fr = frame(f) + r;
            const float* __restrict__ win = a.window + r;
            const float s = 1.0f / (400.0f * P);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int d = 0; d < 5; ++d) {
                    const int n = k2 + 20 * (c + 4 * d);       // z[n] = conj(out[n]) / 400
                    const float2 o = v[5 * c + d];
                    fr[2 * P * n] = o.x * s * win[2 * P * n];
                    fr[2 * P * n + P] = -o.y * s * win[2 * P * n + P];
                }
        }
        __syncthreads();   // the next phase's fold overwrites the rows step 2 read
    }
}

}  // namespace istft800
}  // namespace avse
