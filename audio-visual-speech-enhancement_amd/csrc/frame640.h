// Per-frame arithmetic of the 640-point audio kernels, shared by the whole-utterance kernels (stft.hip k_spec640 /
// k_spec_seg, istft.hip k_istft640 / k_ola) and the streaming session (stream.hip): a frame computed as an utterance
// arrives goes through the same instructions, in the same order, as the frame of the finished utterance.
//
//   spec640   the analysis side: centre-padding index, the frame load, step 1 (window, 20-point DFTs, W320 twiddles)
//             and step 2 (16-point DFTs) of the 16 x 20 split, the real-FFT untangling, |X|, the Slaney band dots, dB,
//             and the order-preserving float <-> uint map of the top_db maximum
//   istft640  the synthesis side: one block's <= 3 frames from mel-dB and the mixture's STFT to windowed time frames
//             (k_istft640's body, its sources and its sink passed in), and one output sample's overlap-add (k_ola's)
#pragma once
#include "fft_common.h"
#include "mfma_util.h"   // lds_barrier, wave_lds_sync

namespace avse {
namespace spec640 {

constexpr int FPG = 3;          // frames per pass (per wave)
constexpr int ZS = 340;         // float2 slots per frame in LDS (20 rows x 17, padded)
constexpr int MW = 24;          // padded Slaney band width of the LDS table (host-checked)

__device__ __forceinline__ unsigned int f2ord(float f) {
    unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned int u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// index of sample i after centre padding: reflect (librosa's 2017 default) or zero (then `keep` is false)
__device__ __forceinline__ int padded_index(int i, int L, int pad_mode, bool& keep) {
    keep = pad_mode == 0 || (i >= 0 && i < L);
    if (pad_mode == 0) {
        const int j = abs(i);
        return min(j, 2 * (L - 1) - j);
    }
    return min(max(i, 0), L - 1);
}

// |X| by the hardware v_sqrt_f32 (1 ulp; sqrtf's correctly rounded sequence is ~12 instructions, 16 per lane per
// chunk, and the magnitudes only feed the mel sums, dB tolerance 1e-3) of the packed square
__device__ __forceinline__ float pk_abs(v2f x) {
    const v2f x2 = x * x;
    return __builtin_amdgcn_sqrtf(x2.x + x2.y);
}

// Slaney band dot of NQ weight quads against the band's magnitudes (k_spec_seg step 4, k_spec640): loads first,
// then the FMAs (same summation order as the quad loop it replaced)
template <int NQ>
__device__ __forceinline__ float band_dot(const float4* wm, const v2f* mf) {
    float4 w[NQ];
    v2f x[2 * NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        w[q] = wm[q];
        x[2 * q] = mf[2 * q];
        x[2 * q + 1] = mf[2 * q + 1];
    }
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        acc = fmaf(x[2 * q].x, w[q].x, acc);
        acc = fmaf(x[2 * q].y, w[q].y, acc);
        acc = fmaf(x[2 * q + 1].x, w[q].z, acc);
        acc = fmaf(x[2 * q + 1].y, w[q].w, acc);
    }
    return acc;
}
// the band dot over the nq quads a mel pass needs (MelTable::seg_nq): straight-line loads per quad count (k_spec_seg
// step 4).  The quads past a band's own are x * 0 added to the sum: the same value for every nq that covers the band.
__device__ __forceinline__ float band_dot_nq(const float4* wm, const v2f* mf2, int nq) {
    switch (nq) {
        case 1: return band_dot<1>(wm, mf2);
        case 2: return band_dot<2>(wm, mf2);
        case 3: return band_dot<3>(wm, mf2);
        case 4: return band_dot<4>(wm, mf2);
        case 5: return band_dot<5>(wm, mf2);
        default: return band_dot<MW / 4>(wm, mf2);
    }
}
// amplitude_to_db of one mel value: 20 log10(acc) via v_log_f32, the exact floor value for acc <= amin
__device__ __forceinline__ float mel_to_db(float acc, float amin, float db_floor) {
    return acc > amin ? 6.0205999132796239f * __log2f(acc) : db_floor;
}

// real-FFT untangling of the packed 320-point transform Z of one frame (z[n] = x[2n] + i x[2n+1]):
// packed form: X = X[k], Y = conj X[320 - k] from Z[k], Z[320 - k]; U = -i W640^k / 2 (a float2 table):
// E = (Zk + conj Zm) / 2, W^k O = U (Zk - conj Zm), X = E + W^k O, Y = E - W^k O
__device__ __forceinline__ void pk_untangle(const v2f* __restrict__ zf, int k, const v2f* __restrict__ ut, v2f& X, v2f& Y) {
    const v2f zk = zf[k], zm = zf[k == 0 ? 0 : 320 - k];
    const v2f S = pk_add_conj(zk, zm);
    const v2f WO = pk_cmul_t(pk_sub_conj(zk, zm), ut[k]);
    X = __builtin_elementwise_fma(v2f(0.5f), S, WO);
    Y = __builtin_elementwise_fma(v2f(0.5f), S, -WO);
}

// lane (f1, n1) of step 1 loads z[n1 + 16 n2] = (x[s0 + 2(n1 + 16 n2)], x[s0 + 2(n1 + 16 n2) + 1]), n2 < 20
// RG (ragged batches): an utterance may start at any element of the packed buffer, so a base that is not 8-byte
// aligned loads the pair as two dwords (the same values)
template <bool RG = false>
__device__ __forceinline__ void load_frame(float2 (&x)[20], const float* __restrict__ s, int L, int s0, int n1,
                                           int pad_mode) {
    if (RG && s0 >= 0 && s0 + 640 <= L && (reinterpret_cast<uintptr_t>(s) & 7)) {
        const float* p = s + s0 + 2 * n1;
#pragma unroll
        for (int n2 = 0; n2 < 20; ++n2) x[n2] = make_float2(p[32 * n2], p[32 * n2 + 1]);
    } else if (s0 >= 0 && s0 + 640 <= L) {
        const float2* p = reinterpret_cast<const float2*>(s + s0) + n1;
#pragma unroll
        for (int n2 = 0; n2 < 20; ++n2) x[n2] = p[16 * n2];
    } else {   // edge frame: branch-free per-sample index arithmetic
#pragma unroll
        for (int n2 = 0; n2 < 20; ++n2) {
            const int i = s0 + 2 * (n1 + 16 * n2);
            bool k0, k1;
            const int j0 = padded_index(i, L, pad_mode, k0), j1 = padded_index(i + 1, L, pad_mode, k1);
            const float v0 = s[j0], v1 = s[j1];
            x[n2] = make_float2(k0 ? v0 : 0.f, k1 ? v1 : 0.f);
        }
    }
}

// ---- step 1, lane (frame, n1): the Hann window on the loaded pairs, then the 20-point DFT over n2 and the twiddle
// W320^{n1 k2} = W640^{2 n1 k2} (2 n1 k2 <= 570) into the frame's LDS rows zf[k2 * 17 + n1] (packed fp32, pk_*) ----
__device__ __forceinline__ void window_frame(v2f (&v)[20], const float2 (&x)[20], const float2* winl, int n1) {
#pragma unroll
    for (int n2 = 0; n2 < 20; ++n2) {
        const float2 w = winl[n1 + 16 * n2];
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
            zf[k2 * 17 + n1] = y;
        }
}
// ---- step 2, lane (frame, k2): the 16-point DFT over n1 -> Z[k2 + 20 k1].  Every lane's row is read before any lane
// stores (the caller synchronises between the two halves): the stores land in other lanes' rows ----
__device__ __forceinline__ void dft16_load(v2f (&w)[16], const v2f* zf, int k2) {
#pragma unroll
    for (int n = 0; n < 16; ++n) w[n] = zf[k2 * 17 + n];
}
__device__ __forceinline__ void dft16_store(v2f (&w)[16], v2f* zf, int k2) {
    pk_dft16(w);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int d = 0; d < 4; ++d) zf[k2 + 20 * (c + 4 * d)] = w[4 * c + d];
}

}  // namespace spec640

namespace istft640 {

constexpr int FPG = 3;          // frames per 64-lane block
// frame slot stride in float2: >= 340 (the 20 x 17 layout of the DFT steps); 353 makes 2 ZS = 2 (mod 32) dwords, so
// the step-3 stores of 16 consecutive frames at one bin (ds_write_b64 lane groups) hit distinct bank pairs (340: 4-way)
constexpr int ZS = 353;

// D / |D| (librosa.magphase; 1 where D == 0) as D * rsq(|D|^2): one v_rsq_f32 and two multiplies instead of a
// square root and two IEEE divisions (~10 instructions each; 16 per lane per chunk in k_istft_fused)
__device__ __forceinline__ float2 unit_phase(float2 d) {
    const float r2 = d.x * d.x + d.y * d.y;
    const float s = __builtin_amdgcn_rsqf(r2);
    return r2 > 0.f ? make_float2(d.x * s, d.y * s) : make_float2(1.f, 0.f);
}

// X[k] = (pinv(mel) @ amp)[k] * d / |d| for one frame's bin k of nb, d the mixture's STFT value there
__device__ __forceinline__ float2 spectrum_bin(const float* __restrict__ pinvT, int n_mels, int nb, const float* amp,
                                               int k, float2 d) {
    float acc = 0.f;
    for (int m = 0; m < n_mels; ++m) acc = fmaf(pinvT[m * nb + k], amp[m], acc);
    const float2 ph = unit_phase(d);
    return make_float2(acc * ph.x, acc * ph.y);
}

// One 64-lane block's ng <= FPG frames: mel_db(m, f) is frame f's predicted mel-dB in band m, stft(k, f) the mixture's
// STFT in bin k, frame(f) where its 640 windowed samples go.  db_to_amplitude -> pinv(mel) -> x unit phase -> the fold
// into the 320-point complex sequence -> the in-register 20 x 16 DFTs (IDFT(Z) = conj(DFT(conj Z)) / 320) -> window.
template <class MelDb, class Stft, class Frame>
__device__ __forceinline__ void synth_frames(const IstftArgs& a, int ng, MelDb mel_db, Stft stft, Frame frame) {
    __shared__ float amp[FPG][80];
    __shared__ float2 xb[FPG][324];
    __shared__ float2 zbuf[FPG * ZS];
    const int lane = threadIdx.x;
    const float2* __restrict__ tw = a.twiddle;   // W640^k

    // db_to_amplitude: (10^(0.1 S))^0.5
    for (int it = lane; it < ng * a.n_mels; it += 64) {
        const int f = it / a.n_mels, m = it - f * a.n_mels;
        amp[f][m] = sqrtf(exp10f(0.1f * mel_db(m, f)));
    }
    __syncthreads();
    for (int it = lane; it < ng * 321; it += 64) {
        const int f = it / 321, k = it - f * 321;
        float2 x = spectrum_bin(a.pinvT, a.n_mels, a.nb, amp[f], k, stft(k, f));
        if (k == 0 || k == 320) x.y = 0.f;            // irfft ignores the DC / Nyquist imaginary parts
        xb[f][k] = x;
    }
    __syncthreads();
    // fold into Z'[k] = conj(E[k] + i O[k]), k in [0,320):
    //   E = (X[k] + conj X[320-k]) / 2,  O = (X[k] - conj X[320-k]) W640^{-k} / 2
    for (int it = lane; it < ng * 320; it += 64) {
        const int f = it / 320, k = it - f * 320;
        const float2 xk = xb[f][k], xm = cconj(xb[f][320 - k]);
        const float2 E = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y + xm.y));
        const float2 O = cmul(make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y - xm.y)), cconj(tw[k]));
        const float2 Z = make_float2(E.x - O.y, E.y + O.x);   // E + i O
        zbuf[f * ZS + k] = cconj(Z);
    }
    __syncthreads();
    // forward 320-point DFT of Z' (step 1: 20-point over n2 of z[n1 + 16 n2], lane = (f, n1))
    {
        const int f = lane >> 4, n1 = lane & 15;
        float2 v[20];
        const bool act = f < ng;
        if (act) {
#pragma unroll
            for (int n2 = 0; n2 < 20; ++n2) v[n2] = zbuf[f * ZS + n1 + 16 * n2];
        }
        __syncthreads();
        if (act) {
            dft20(v, tw);
            float2* zf = zbuf + f * ZS;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int d = 0; d < 5; ++d) {
                    const int k2 = c + 4 * d;
                    float2 y = v[5 * c + d];
                    if (k2) y = cmul(y, tw[(2 * n1 * k2) % 640]);
                    zf[k2 * 17 + n1] = y;
                }
        }
    }
    __syncthreads();
    // step 2: 16-point DFT over n1, lane = (f, k2); write the time samples
    {
        const int f = lane / 20, k2 = lane - 20 * (lane / 20);
        if (f < ng) {
            float2 v[16];
            const float2* zf = zbuf + f * ZS;
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) v[n1] = zf[k2 * 17 + n1];
            dft16(v, tw);
            float* fr = frame(f);
            const float s = 1.0f / 320.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int n = k2 + 20 * (c + 4 * d);       // z[n] = conj(out[n]) / 320
                    const float2 o = v[4 * c + d];
                    fr[2 * n] = o.x * s * a.window[2 * n];
                    fr[2 * n + 1] = -o.y * s * a.window[2 * n + 1];
                }
        }
    }
}

// Output sample at position p of the untrimmed signal of T frames: the frames that cover it (t * hop <= p <=
// t * hop + N - 1) summed in increasing frame order (librosa's order), over the window sum-square of those frames where
// it exceeds float32 tiny.  sample(t, o) is sample o of windowed frame t.
template <class FrameSample>
__device__ __forceinline__ float ola_sample(long long p, long long T, int N, int hop, const float* __restrict__ window,
                                            FrameSample sample) {
    const long long tlo = (p - N + 1 <= 0) ? 0 : (p - N + 1 + hop - 1) / hop;
    const long long thi = min(T - 1, p / hop);
    float y = 0.f, wss = 0.f;
    for (long long t = tlo; t <= thi; ++t) {
        const int o = (int)(p - t * hop);
        y += sample(t, o);
        const float w = window[o];
        wss += w * w;
    }
    if (wss > 1.17549435e-38f) y /= wss;
    return y;
}

}  // namespace istft640
}  // namespace avse
