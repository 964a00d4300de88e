// Device-side preprocess (include/avse.h avse_mix_pairs, avse_video_stats): the SNR mixing of the reference's
// preprocess_audio_pair (data_processor.py:119-139) for a ragged group of int16 (speech, noise) pairs, and the
// VideoNormalizer fit of data_processor.py:203-206 (mean / population std over slices and frames).
// Both are memory bound; every store is a vector store, the only atomics are 64-bit integer vector atomics.
#include <algorithm>

#include "avse_common.h"

// numpy rounds the noise gain's product and the mixture's sum separately, so nothing here may contract to an FMA: the
// Makefile builds this file with -ffp-contract=off (the pragma alone does not reach the header-defined __dmul_rn /
// __dadd_rn, whose product and sum the backend then fuses after inlining), and the pragma keeps that true for any other
// build line
#pragma clang fp contract(off)

namespace avse {
namespace {

constexpr int kThreads = 256;
typedef short short8 __attribute__((ext_vector_type(8)));
typedef short short4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

// ---- pair mixing ------------------------------------------------------------------------------
// Scratch words of pair u (avse_ctx prep scratch): acc[4 u + 0] sum of speech^2, + 1 sum of noise^2 over
// [0, min(n_n, n_s)), + 2 sum of noise^2 over [0, n_s mod n_n) (n_n <= n_s), then gain[u] (double) behind the words.

// This block's share (part of nparts) of the exact sum of x[0, n)^2.  Loads are 16-byte vectors over the aligned
// 8-sample groups of the buffer; the groups cut by the segment's ends (a segment may start at any element) go sample
// by sample.
__device__ __forceinline__ u64 sumsq_share(const int16_t* x, int64_t n, int part, int nparts) {
    if (n <= 0) return 0;
    const int m = (int)(((uintptr_t)x & 15) >> 1);   // samples between the previous 16-byte boundary and x
    const int64_t ngroups = (n + m + 7) >> 3;
    u64 acc = 0;
    for (int64_t g = (int64_t)part * kThreads + threadIdx.x; g < ngroups; g += (int64_t)nparts * kThreads) {
        const int64_t e0 = g * 8 - m;                // the group's first sample, relative to x
        if (e0 >= 0 && e0 + 8 <= n) {
            const short8 v = *reinterpret_cast<const short8*>(x + e0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int a = v[k];
                acc += (u64)(unsigned)(a * a);       // <= 2^30
            }
        } else {
            for (int k = 0; k < 8; ++k) {
                const int64_t e = e0 + k;
                if (e >= 0 && e < n) {
                    const int a = x[e];
                    acc += (u64)(unsigned)(a * a);
                }
            }
        }
    }
    return acc;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// Phase 1: exact integer powers.  grid (parts, pairs).  The noise looped cyclically to n_s samples has the power
// (n_s / n_n) * sum(noise^2) + sum(noise[0, n_s mod n_n)^2), so no sample is read through a wrapped index here.
__global__ __launch_bounds__(kThreads) void k_mix_power(const int16_t* __restrict__ speech, const int64_t* __restrict__ so,
                                                        const int16_t* __restrict__ noise, const int64_t* __restrict__ no,
                                                        u64* __restrict__ acc) {
    __shared__ u64 red[kThreads / 64][3];
    const int64_t u = blockIdx.y;
    const int64_t n_s = so[u + 1] - so[u], n_n = no[u + 1] - no[u];
    if (n_s <= 0) return;   // block-uniform (refused by the binding; the mix kernel writes silence)
    const int16_t* sp = speech + so[u];
    const int16_t* nz = noise + no[u];
    const int64_t head = n_n < n_s ? (n_n > 0 ? n_n : 0) : n_s;
    const int64_t rem = (n_n > 0 && n_n <= n_s) ? n_s % n_n : 0;   // once per thread, not per sample
    u64 a[3];
    a[0] = sumsq_share(sp, n_s, blockIdx.x, gridDim.x);
    a[1] = sumsq_share(nz, head, blockIdx.x, gridDim.x);
    a[2] = sumsq_share(nz, rem, blockIdx.x, gridDim.x);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const u64 w = wave_sum(a[k]);
        if (lane == 0) red[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        u64 t = 0;
        for (int w = 0; w < kThreads / 64; ++w) t += red[w][threadIdx.x];
        if (t) atomicAdd(&acc[4 * u + threadIdx.x], t);   // integer: any arrival order gives the same word
    }
}

// The gain of AudioMixer.snr_factor, operation for operation: s = S / n_s, n = N / n_s, 0.0 when n == 0, else
// sqrt(s / (n * snr_lin)), each step correctly rounded.  One thread per pair.
__global__ __launch_bounds__(kThreads) void k_mix_gain(const int64_t* __restrict__ so, const int64_t* __restrict__ no,
                                                       const double* __restrict__ snr_lin, const u64* __restrict__ acc,
                                                       int64_t U, double* __restrict__ gain, double* __restrict__ factor) {
    const int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (u >= U) return;
    const int64_t n_s = so[u + 1] - so[u], n_n = no[u + 1] - no[u];
    double f = 0.0;
    if (n_s > 0 && n_n > 0) {
        const u64 S = acc[4 * u], F = acc[4 * u + 1], P = acc[4 * u + 2];
        const u64 N = n_n <= n_s ? (u64)(n_s / n_n) * F + P : F;
        if (N != 0) {
            const double s = __ddiv_rn((double)S, (double)n_s);
            const double n = __ddiv_rn((double)N, (double)n_s);
            f = __dsqrt_rn(__ddiv_rn(s, n * (snr_lin ? snr_lin[u] : 1.0)));
        }
    }
    gain[u] = f;
    if (factor) factor[u] = f;
}

// Phase 2: four consecutive output samples per thread.  grid (ceil(L / 1024), pairs).  VEC: L % 4 == 0 and 16-byte
// aligned outputs (16-byte stores); the 2-byte inputs load as one 8-byte vector where the segment's alignment and ends
// allow, else sample by sample with the noise index wrapped as it advances.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_mix(const int16_t* __restrict__ speech, const int64_t* __restrict__ so,
                                                  const int16_t* __restrict__ noise, const int64_t* __restrict__ no,
                                                  const double* __restrict__ gain, int64_t U, int64_t L,
                                                  float* __restrict__ rows, double* __restrict__ mix64) {
    const int64_t i0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (i0 >= L) return;
    const int64_t u = blockIdx.y;
    int64_t n_s = so[u + 1] - so[u], n_n = no[u + 1] - no[u];
    if (n_s < 0) n_s = 0;
    if (n_n < 0) n_n = 0;
    const int16_t* sp = speech + so[u];
    const int16_t* nz = noise + no[u];
    const double f = gain[u];
    double sv[4], nv[4];
    const bool inside = i0 + 4 <= n_s;
    if (inside && (((uintptr_t)(sp + i0)) & 7) == 0) {
        const short4 v = *reinterpret_cast<const short4*>(sp + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) sv[k] = (double)v[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) sv[k] = i0 + k < n_s ? (double)sp[i0 + k] : 0.0;
    }
    // i0 < L < 2^31 (checked by the launcher), and the remainder is taken only when n_n <= i0: 32-bit operands
    int64_t j = (n_n == 0 || i0 < n_n) ? i0 : (int64_t)((uint32_t)i0 % (uint32_t)n_n);
    if (inside && j + 4 <= n_n && (((uintptr_t)(nz + j)) & 7) == 0) {
        const short4 v = *reinterpret_cast<const short4*>(nz + j);
#pragma unroll
        for (int k = 0; k < 4; ++k) nv[k] = (double)v[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nv[k] = 0.0;
            if (n_n > 0 && i0 + k < n_s) {
                nv[k] = (double)nz[j];
                if (++j == n_n) j = 0;
            }
        }
    }
    double mx[4];
    float r0[4], r1[4], r2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool live = i0 + k < n_s;            // beyond the speech: the zero padding of pad_with_zeros
        const double ns = live ? nv[k] * f : 0.0;  // two roundings: product, then sum (no FMA, see the top of the file)
        mx[k] = live ? sv[k] + ns : 0.0;
        r0[k] = (float)mx[k];
        r1[k] = (float)sv[k];
        r2[k] = (float)ns;
    }
    float* o0 = rows + ((int64_t)0 * U + u) * L + i0;
    float* o1 = rows + ((int64_t)1 * U + u) * L + i0;
    float* o2 = rows + ((int64_t)2 * U + u) * L + i0;
    double* om = mix64 ? mix64 + u * L + i0 : nullptr;
    if (VEC) {   // L % 4 == 0: the four samples are inside the row
        *reinterpret_cast<float4*>(o0) = make_float4(r0[0], r0[1], r0[2], r0[3]);
        *reinterpret_cast<float4*>(o1) = make_float4(r1[0], r1[1], r1[2], r1[3]);
        *reinterpret_cast<float4*>(o2) = make_float4(r2[0], r2[1], r2[2], r2[3]);
        if (om) {
            *reinterpret_cast<double2*>(om) = make_double2(mx[0], mx[1]);
            *reinterpret_cast<double2*>(om + 2) = make_double2(mx[2], mx[3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < L) {
                o0[k] = r0[k];
                o1[k] = r1[k];
                o2[k] = r2[k];
                if (om) om[k] = mx[k];
            }
    }
}

// ---- video moments ----------------------------------------------------------------------------
constexpr int kPix = 256;   // pixels per workgroup (one per thread)

// One thread's registers' worth of a slice's [256 F] span: element (or 16-byte unit) t + 256 k of the span.
template <bool VEC>
struct SliceRegs;
template <>
struct SliceRegs<true> {
    float4 r[kVideoStatsMaxF / 4];
    __device__ __forceinline__ void load(const float* src, int t, int n_tile) {
#pragma unroll
        for (int k = 0; k < kVideoStatsMaxF / 4; ++k) {
            const int i = t + k * kThreads;
            r[k] = i * 4 < n_tile ? reinterpret_cast<const float4*>(src)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __device__ __forceinline__ void stage(float* dst, int t, int n_tile) const {
#pragma unroll
        for (int k = 0; k < kVideoStatsMaxF / 4; ++k) {
            const int i = t + k * kThreads;
            if (i * 4 < n_tile) reinterpret_cast<float4*>(dst)[i] = r[k];
        }
    }
};
template <>
struct SliceRegs<false> {
    float r[kVideoStatsMaxF];
    __device__ __forceinline__ void load(const float* src, int t, int n_tile) {
#pragma unroll
        for (int k = 0; k < kVideoStatsMaxF; ++k) {
            const int i = t + k * kThreads;
            r[k] = i < n_tile ? src[i] : 0.f;
        }
    }
    __device__ __forceinline__ void stage(float* dst, int t, int n_tile) const {
#pragma unroll
        for (int k = 0; k < kVideoStatsMaxF; ++k) {
            const int i = t + k * kThreads;
            if (i < n_tile) dst[i] = r[k];
        }
    }
};

// grid (ceil(HW / 256), chunks of chunk_len slices).  A workgroup streams its pixels' contiguous [256 F] span of each
// slice (16-byte loads when VEC: H W F % 4 == 0 and an aligned base), regroups it through LDS (a pixel's F values are
// not 16-byte units) and keeps per-pixel float64 sums of d and d^2, d = x - pivot, pivot = video[0, h, w, 0]: the
// subtraction is exact in float64, and a constant pixel sums exact zeros.  The next slice's loads are issued before
// the current one is summed; the two LDS buffers alternate, so one barrier per slice is enough.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_video_moments(const float* __restrict__ video, int64_t S, int HW, int F,
                                                            int chunk_len, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float buf[2][kPix * kVideoStatsMaxF];
    const int t = threadIdx.x;
    const int64_t P = (int64_t)HW * F;
    const int64_t tile0 = (int64_t)blockIdx.x * kPix * F;
    const int n_tile = (int)(P - tile0 < (int64_t)kPix * F ? P - tile0 : (int64_t)kPix * F);
    const int pix = blockIdx.x * kPix + t;
    const bool live = pix < HW;
    const int64_t s0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t s1 = s0 + chunk_len < S ? s0 + chunk_len : S;
    const double pivot = live ? (double)video[(int64_t)pix * F] : 0.0;
    SliceRegs<VEC> regs;
    double sd = 0.0, sd2 = 0.0;
    int b = 0;
    if (s0 < s1) regs.load(video + s0 * P + tile0, t, n_tile);
    for (int64_t s = s0; s < s1; ++s) {
        regs.stage(buf[b], t, n_tile);
        if (s + 1 < s1) regs.load(video + (s + 1) * P + tile0, t, n_tile);
        __syncthreads();
        if (live) {
#pragma unroll
            for (int f = 0; f < kVideoStatsMaxF; ++f)
                if (f < F) {
                    const double d = (double)buf[b][t * F + f] - pivot;
                    sd += d;
                    sd2 += d * d;
                }
        }
        b ^= 1;
    }
    if (live) {
        partial[((int64_t)blockIdx.y * 2 + 0) * HW + pix] = sd;
        partial[((int64_t)blockIdx.y * 2 + 1) * HW + pix] = sd2;
    }
}

// Combines the chunks' partial sums in chunk order (no floating-point atomics: bitwise reproducible), then
// mean = pivot + E[d], var = max(0, E[d^2] - E[d]^2), each rounded once to float32.
__global__ __launch_bounds__(kThreads) void k_video_moments_finish(const float* __restrict__ video,
                                                                   const double* __restrict__ partial, int n_chunks,
                                                                   int64_t S, int HW, int F, float* __restrict__ mean,
                                                                   float* __restrict__ stdv) {
    const int pix = blockIdx.x * kThreads + threadIdx.x;
    if (pix >= HW) return;
    double sd = 0.0, sd2 = 0.0;
    for (int c = 0; c < n_chunks; ++c) {
        sd += partial[((int64_t)c * 2 + 0) * HW + pix];
        sd2 += partial[((int64_t)c * 2 + 1) * HW + pix];
    }
    const double n = (double)(S * F);
    const double ed = sd / n, ed2 = sd2 / n;
    double var = ed2 - ed * ed;
    if (var < 0.0) var = 0.0;   // a NaN stays a NaN
    mean[pix] = (float)((double)video[(int64_t)pix * F] + ed);
    stdv[pix] = (float)__dsqrt_rn(var);
}

// uint8 video: grid as k_video_moments, one pixel per thread.  Sums of bytes and of their squares are exact in 64-bit
// integers (255^2 S F < 2^64 for any video that fits in memory), so there is no pivot and no staging: a thread reads its
// pixel's F consecutive bytes of each slice (a wave reads one contiguous 64 F-byte run) and the partials are integers.
__global__ __launch_bounds__(kThreads) void k_video_moments_u8(const uint8_t* __restrict__ video, int64_t S, int HW, int F,
                                                               int chunk_len, u64* __restrict__ partial) {
    const int pix = blockIdx.x * kPix + threadIdx.x;
    if (pix >= HW) return;
    const int64_t P = (int64_t)HW * F;
    const int64_t s0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t s1 = s0 + chunk_len < S ? s0 + chunk_len : S;
    const uint8_t* src = video + s0 * P + (int64_t)pix * F;
    u64 sx = 0, sx2 = 0;
    for (int64_t s = s0; s < s1; ++s, src += P) {
        unsigned a = 0, a2 = 0;   // one slice: at most 8 x 255^2
#pragma unroll
        for (int f = 0; f < kVideoStatsMaxF; ++f)
            if (f < F) {
                const unsigned x = src[f];
                a += x;
                a2 += x * x;
            }
        sx += a;
        sx2 += a2;
    }
    partial[((int64_t)blockIdx.y * 2 + 0) * HW + pix] = sx;
    partial[((int64_t)blockIdx.y * 2 + 1) * HW + pix] = sx2;
}

// mean = Sx / n and var = (n Sx2 - Sx^2) / n^2 from the exact integer moments (the numerator in 128 bits), each rounded
// once to float64 by the division and once more to float32
__global__ __launch_bounds__(kThreads) void k_video_moments_u8_finish(const u64* __restrict__ partial, int n_chunks,
                                                                      int64_t S, int HW, int F, float* __restrict__ mean,
                                                                      float* __restrict__ stdv) {
    const int pix = blockIdx.x * kThreads + threadIdx.x;
    if (pix >= HW) return;
    u64 sx = 0, sx2 = 0;
    for (int c = 0; c < n_chunks; ++c) {
        sx += partial[((int64_t)c * 2 + 0) * HW + pix];
        sx2 += partial[((int64_t)c * 2 + 1) * HW + pix];
    }
    const u64 n = (u64)S * (u64)F;
    const unsigned __int128 num = (unsigned __int128)n * sx2 - (unsigned __int128)sx * sx;   // >= 0 (Cauchy-Schwarz)
    const double numd = (double)(u64)(num >> 64) * 18446744073709551616.0 + (double)(u64)num;
    mean[pix] = (float)__ddiv_rn((double)sx, (double)n);
    stdv[pix] = (float)__dsqrt_rn(__ddiv_rn(numd, (double)n * (double)n));
}

}  // namespace

size_t mix_pairs_scratch_bytes(int64_t n_pairs) { return (size_t)n_pairs * (4 * sizeof(u64) + sizeof(double)); }

int launch_mix_pairs(const int16_t* speech, const int64_t* speech_off, const int16_t* noise, const int64_t* noise_off,
                     const double* snr_lin, int64_t U, int64_t L, float* rows, double* mix64, double* factor,
                     void* scratch, hipStream_t s) {
    u64* acc = reinterpret_cast<u64*>(scratch);
    double* gain = reinterpret_cast<double*>(acc + 4 * U);
    AVSE_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(u64) * 4 * U, s));
    // workgroups per pair in the power pass: enough to fill the device for a small group, one for a large one
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(32, 2048 / U));
    const bool vec = L % 4 == 0 && ((uintptr_t)rows & 15) == 0 && ((uintptr_t)mix64 & 15) == 0;
    const unsigned gx = (unsigned)((L + 4 * kThreads - 1) / (4 * kThreads));
    for (int64_t u0 = 0; u0 < U; u0 += 65535) {   // grid.y limit
        const unsigned nu = (unsigned)std::min<int64_t>(65535, U - u0);
        hipLaunchKernelGGL(k_mix_power, dim3(parts, nu), dim3(kThreads), 0, s, speech, speech_off + u0, noise,
                           noise_off + u0, acc + 4 * u0);
        AVSE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_mix_gain, dim3((unsigned)((U + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, speech_off,
                       noise_off, snr_lin, acc, U, gain, factor);
    AVSE_HIP_CHECK(hipGetLastError());
    for (int64_t u0 = 0; u0 < U; u0 += 65535) {
        const unsigned nu = (unsigned)std::min<int64_t>(65535, U - u0);
        // the row planes are U rows apart: pass the plane-0 row of pair u0 and the whole group's U
        if (vec)
            hipLaunchKernelGGL(k_mix<true>, dim3(gx, nu), dim3(kThreads), 0, s, speech, speech_off + u0, noise,
                               noise_off + u0, gain + u0, U, L, rows + u0 * L, mix64 ? mix64 + u0 * L : nullptr);
        else
            hipLaunchKernelGGL(k_mix<false>, dim3(gx, nu), dim3(kThreads), 0, s, speech, speech_off + u0, noise,
                               noise_off + u0, gain + u0, U, L, rows + u0 * L, mix64 ? mix64 + u0 * L : nullptr);
        AVSE_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

void video_stats_plan(int64_t S, int* n_chunks, int* chunk_len) {
    // up to 32 chunks of at least 16 slices: 64 pixel tiles x 32 chunks fill the device for the 128 x 128 crops
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(32, (S + 15) / 16));
    const int64_t len = (S + want - 1) / want;
    *chunk_len = (int)std::min<int64_t>(len, INT32_MAX);
    *n_chunks = (int)((S + len - 1) / len);
}

size_t video_stats_scratch_bytes(int64_t S, int H, int W) {
    int nc, cl;
    video_stats_plan(S, &nc, &cl);
    return sizeof(double) * 2 * (size_t)nc * H * W;
}

int launch_video_stats(const float* video, int64_t S, int H, int W, int F, float* mean, float* stdv, void* scratch,
                       hipStream_t s) {
    int nc, cl;
    video_stats_plan(S, &nc, &cl);
    const int HW = H * W;
    double* partial = reinterpret_cast<double*>(scratch);
    const dim3 grid((unsigned)((HW + kPix - 1) / kPix), (unsigned)nc);
    const bool vec = ((int64_t)HW * F) % 4 == 0 && ((uintptr_t)video & 15) == 0;
    if (vec) hipLaunchKernelGGL(k_video_moments<true>, grid, dim3(kThreads), 0, s, video, S, HW, F, cl, partial);
    else hipLaunchKernelGGL(k_video_moments<false>, grid, dim3(kThreads), 0, s, video, S, HW, F, cl, partial);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_video_moments_finish, dim3((unsigned)((HW + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                       video, partial, nc, S, HW, F, mean, stdv);
    AVSE_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_video_stats_u8(const uint8_t* video, int64_t S, int H, int W, int F, float* mean, float* stdv, void* scratch,
                          hipStream_t s) {
    int nc, cl;
    video_stats_plan(S, &nc, &cl);
    const int HW = H * W;
    u64* partial = reinterpret_cast<u64*>(scratch);   // video_stats_scratch_bytes: 2 x 8 bytes per chunk and pixel
    static_assert(sizeof(u64) == sizeof(double), "scratch size");
    hipLaunchKernelGGL(k_video_moments_u8, dim3((unsigned)((HW + kPix - 1) / kPix), (unsigned)nc), dim3(kThreads), 0, s,
                       video, S, HW, F, cl, partial);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_video_moments_u8_finish, dim3((unsigned)((HW + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                       (const u64*)partial, nc, S, HW, F, mean, stdv);
    AVSE_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace avse
