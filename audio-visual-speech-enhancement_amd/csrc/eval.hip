// The evaluate stage (include/avse.h avse_eval_pairs, avse_eval_pairs_ext): SNR, scale-invariant SDR, segmental SNR,
// STOI and (the _ext entry point's sixth slot) ESTOI for a ragged group of (clean, degraded) float32 pairs.  Everything
// is float64 arithmetic; every reduction has an order that depends on the pair's own length only (never on its place in
// the batch or on its address), so a pair's numbers are the same bits alone and inside any batch.  No floating-point
// atomics; every store is a vector store.
#include <algorithm>

#include "avse_common.h"

// products and sums round separately, as the numpy reference does (tests/eval_ref.py); the Makefile passes
// -ffp-contract=off as well, which also reaches header-defined helpers after inlining (see prep.hip)
#pragma clang fp contract(off)

namespace avse {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kParts = 16;                     // partial sums per pair: fixed, so the order never depends on the batch
constexpr int64_t kMaxPair = (int64_t)1 << 24;
constexpr double kEps = 2.220446049250313e-16; // 2^-52

struct Pair {
    int64_t o, n;          // element offset relative to off[0], samples
    int64_t n10, F;        // resampled length, STOI frames
    int64_t s10, fs, ss;   // region starts: resampled samples, STOI frames, segmental-SNR frames
    int64_t Fs;            // segmental-SNR frames
};

// Geometry of pair u.  A pair outside [0, 2^24] samples, or offsets that leave [off[0], off[0] + cap], count as empty:
// every scratch index below is bounded by cap whatever the offsets hold.
__device__ __forceinline__ Pair pair_geom(const int64_t* __restrict__ off, int64_t U, int64_t u, const EvalDev& t) {
    Pair p;
    const int64_t base = off[0];
    p.o = off[u] - base;
    p.n = off[u + 1] - off[u];
    const int64_t total = off[U] - base;
    if (total < 0 || total > t.cap || p.o < 0 || p.n < 0 || p.n > kMaxPair || p.o + p.n > t.cap) {
        p.o = 0;
        p.n = 0;
    }
    p.n10 = (p.n * t.up + t.down - 1) / t.down;
    p.F = p.n10 > 256 ? (p.n10 - 256 + 127) / 128 : 0;   // starts 0, 128, .. while i < n10 - 256
    p.s10 = p.o * t.up / t.down + u;
    p.fs = p.s10 / 128;
    p.ss = p.o / t.skip;
    p.Fs = p.n >= t.win ? (p.n - t.win) / t.skip + 1 : 0;
    return p;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// four consecutive samples from x + e (e + 4 <= n checked by the caller): one 16-byte load where the address allows
__device__ __forceinline__ void load4(const float* x, int64_t e, double v[4]) {
    if ((((uintptr_t)(x + e)) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(x + e);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = x[e + k];
    }
}

// ---- sums ---------------------------------------------------------------------------------------
// grid (pairs, kParts).  Thread t of part q takes the 4-sample groups (q 256 + t) + 4096 i of the pair, counted from
// the pair's own first sample.  PASS 0: sum s^2, sum s y, sum (s - y)^2.  PASS 1: sum (alpha s - y)^2 with
// alpha = (sum s y) / (sum s^2) from pass 0.
template <int PASS>
__global__ __launch_bounds__(kThreads) void k_eval_sums(const float* __restrict__ ref, const float* __restrict__ deg,
                                                        const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                        const double* __restrict__ sums, double* __restrict__ partial) {
    __shared__ double red[kWaves][3];
    const int64_t u = blockIdx.x;
    const Pair p = pair_geom(off, U, u, t);
    const float* s = ref + off[u];
    const float* y = deg + off[u];
    const double alpha = PASS ? sums[4 * u + 1] / sums[4 * u + 0] : 0.0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const int64_t ngroups = (p.n + 3) >> 2;
    for (int64_t g = (int64_t)blockIdx.y * kThreads + threadIdx.x; g < ngroups; g += (int64_t)kParts * kThreads) {
        const int64_t e = g * 4;
        double sv[4] = {0.0, 0.0, 0.0, 0.0}, yv[4] = {0.0, 0.0, 0.0, 0.0};
        int cnt = 4;
        if (e + 4 <= p.n) {
            load4(s, e, sv);
            load4(y, e, yv);
        } else {
            cnt = (int)(p.n - e);
            for (int k = 0; k < cnt; ++k) {
                sv[k] = s[e + k];
                yv[k] = y[e + k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) {
                if (PASS == 0) {
                    const double d = sv[k] - yv[k];
                    a0 += sv[k] * sv[k];
                    a1 += sv[k] * yv[k];
                    a2 += d * d;
                } else {
                    const double r = alpha * sv[k] - yv[k];
                    a0 += r * r;
                }
            }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    a0 = wave_sum(a0);
    if (PASS == 0) {
        a1 = wave_sum(a1);
        a2 = wave_sum(a2);
    }
    if (lane == 0) {
        red[wave][0] = a0;
        red[wave][1] = a1;
        red[wave][2] = a2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = 0.0;
        for (int w = 0; w < kWaves; ++w) v += red[w][threadIdx.x];
        partial[(u * kParts + blockIdx.y) * 3 + threadIdx.x] = v;
    }
}

// One thread per pair: the parts in part order.  PASS 0 leaves the three sums for pass 1; PASS 1 writes SNR and SI-SDR
// (and the whole row of an empty pair, and the STOI slots when STOI is not computed for this rate).
template <int PASS>
__global__ __launch_bounds__(kThreads) void k_eval_sums_finish(const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                               const double* __restrict__ partial,
                                                               double* __restrict__ sums, double* __restrict__ metrics) {
    const int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (u >= U) return;
    double v[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < kParts; ++q)
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] += partial[(u * kParts + q) * 3 + k];
    if (PASS == 0) {
        sums[4 * u + 0] = v[0];
        sums[4 * u + 1] = v[1];
        sums[4 * u + 2] = v[2];
        return;
    }
    const Pair p = pair_geom(off, U, u, t);
    double* m = metrics + u * t.ms;
    if (p.n == 0) {
        for (int k = 0; k < t.ms; ++k) m[k] = quiet_nan();
        return;
    }
    const double s2 = sums[4 * u + 0], sy = sums[4 * u + 1], d2 = sums[4 * u + 2];
    const double alpha = sy / s2;
    m[0] = 10.0 * log10(s2 / d2);
    m[1] = 10.0 * log10(alpha * alpha * s2 / v[0]);
    if (!t.stoi) {
        m[3] = quiet_nan();
        m[4] = 0.0;
        if (t.ms > 5) m[5] = quiet_nan();
    }
}

// ---- segmental SNR ------------------------------------------------------------------------------
// grid (pairs, G): one wave per frame; lane l takes samples l, l + 64, .. of the frame.
__global__ __launch_bounds__(kThreads) void k_eval_seg(const float* __restrict__ ref, const float* __restrict__ deg,
                                                       const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                       double* __restrict__ segv) {
    const int64_t u = blockIdx.x;
    const Pair p = pair_geom(off, U, u, t);
    const float* s = ref + off[u];
    const float* y = deg + off[u];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t f = (int64_t)blockIdx.y * kWaves + wave; f < p.Fs; f += (int64_t)gridDim.y * kWaves) {
        const int64_t i0 = f * t.skip;
        double a = 0.0, b = 0.0;
        for (int i = lane; i < t.win; i += 64) {
            const double w = t.segw[i];
            const double sv = s[i0 + i], yv = y[i0 + i];
            const double ws = w * sv, wd = w * (sv - yv);
            a += ws * ws;
            b += wd * wd;
        }
        a = wave_sum(a);
        b = wave_sum(b);
        if (lane == 0) {
            double v = 10.0 * log10(a / (b + kEps) + kEps);
            v = v < -10.0 ? -10.0 : (v > 35.0 ? 35.0 : v);
            segv[p.ss + f] = v;
        }
    }
}

// The mean of cnt values in a fixed order: thread t sums the contiguous run [t c, (t + 1) c), c = ceil(cnt / 256), in
// index order, and thread 0 adds the 256 run sums in run order.  NaN for cnt == 0.  One workgroup per pair.
// MODE 0: the segmental-SNR frame values -> slot 2.  MODE 1: STOI's d(j, m) -> slot 3.  MODE 2: ESTOI's d_m -> slot 5.
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_eval_mean(const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                        const double* __restrict__ vals, const int* __restrict__ kept,
                                                        double* __restrict__ metrics) {
    __shared__ double run[kThreads];
    const int64_t u = blockIdx.x;
    const Pair p = pair_geom(off, U, u, t);
    int64_t base, cnt;
    if (MODE == 0) {
        base = p.ss;
        cnt = p.Fs;
    } else {
        const int64_t M = (int64_t)kept[u] - 1;
        base = MODE == 1 ? 15 * p.fs : p.fs;
        cnt = M >= 30 ? (MODE == 1 ? 15 : 1) * (M - 29) : 0;
    }
    const int64_t c = (cnt + kThreads - 1) / kThreads;
    double a = 0.0;
    for (int64_t i = threadIdx.x * c; i < (threadIdx.x + 1) * c && i < cnt; ++i) a += vals[base + i];
    run[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < kThreads; ++i) tot += run[i];
        metrics[u * t.ms + (MODE == 0 ? 2 : MODE == 1 ? 3 : 5)] = (cnt > 0 && p.n > 0) ? tot / (double)cnt : quiet_nan();
    }
}

// ---- STOI: polyphase resampler ------------------------------------------------------------------
// ceil(a / b), b > 0, any sign of a
__device__ __forceinline__ int64_t ceil_div(int64_t a, int64_t b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }

// Input samples one tile of 256 outputs reads: the first output's first sample to the last output's last one
__host__ __device__ inline int resample_span(int up, int down, int H) { return 255 * down / up + 2 * H / up + 3; }

// grid (pairs, G): a workgroup takes tiles of 256 consecutive outputs of both signals, one output per thread.
// y10[k] = sum_j h[H + k down - j up] x[j] over the j that keep the tap index in [0, 2H] and j in [0, n), in ascending
// j: only the taps that meet a sample (2H / up + 1 of the 2H + 1).  The taps sit in LDS behind `up` zeros and the
// tile's input span is staged in LDS with zeros outside [0, n), so the tap loop has a fixed trip count and no bounds.
// Dynamic LDS: (up + 2H + 1) doubles, then 2 x resample_span floats.
__global__ __launch_bounds__(kThreads) void k_eval_resample(const float* __restrict__ ref, const float* __restrict__ deg,
                                                            const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                            double* __restrict__ x10, double* __restrict__ y10) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int ntap = 2 * t.H + 1, T = 2 * t.H / t.up + 1, span = resample_span(t.up, t.down, t.H);
    double* h = lds;                                          // h[up + i] = taps[i]
    float* xs = reinterpret_cast<float*>(lds + t.up + ntap);
    float* ys = xs + span;
    for (int i = threadIdx.x; i < t.up + ntap; i += kThreads) h[i] = i < t.up ? 0.0 : t.taps[i - t.up];
    const int64_t u = blockIdx.x;
    const Pair p = pair_geom(off, U, u, t);
    const float* s = ref + off[u];
    const float* y = deg + off[u];
    for (int64_t k0 = (int64_t)blockIdx.y * kThreads; k0 < p.n10; k0 += (int64_t)gridDim.y * kThreads) {
        const int64_t jlo = ceil_div(k0 * t.down - t.H, t.up);   // the tile's first input sample (may be negative)
        __syncthreads();                                         // the previous tile's reads; the taps
        for (int i = threadIdx.x; i < span; i += kThreads) {
            const int64_t j = jlo + i;
            const bool in = j >= 0 && j < p.n;
            xs[i] = in ? s[j] : 0.f;
            ys[i] = in ? y[j] : 0.f;
        }
        __syncthreads();
        const int64_t k = k0 + threadIdx.x;
        if (k < p.n10) {
            const int64_t c = k * t.down;
            const int64_t j0 = ceil_div(c - t.H, t.up);
            const int i0 = (int)(j0 - jlo);                      // 0 <= i0, i0 + T <= span
            const double* hp = h + t.up + (int)(t.H + c - j0 * t.up);   // tap of sample j0, in (2H - up, 2H]
            double ax = 0.0, ay = 0.0;
            for (int q = 0; q < T; ++q) {                        // the last tap index is above -up: the zeros in front
                const double w = hp[-q * t.up];
                ax += w * (double)xs[i0 + q];
                ay += w * (double)ys[i0 + q];
            }
            x10[p.s10 + k] = ax;
            y10[p.s10 + k] = ay;
        }
    }
}

// The same sum for max(up, down) > 24 (avse_eval_pairs_ext with AVSE_EVAL_ANY_RATE), where the 2H + 1 taps do not fit
// in LDS: the same tiles and the same staged span (clean and degraded interleaved), the taps read from global memory.
// With H + k down = B up + phase (0 <= phase < up) the tap of sample j is h[phase + (B - j) up], so output k walks row
// `phase` of t.ptaps, which holds that row's T = 2H / up + 1 taps in ascending j from j = B - (T - 1): a contiguous run
// per thread, the same terms in the same ascending-j order as above.  A row whose first tap would lie past 2H starts
// with a zero (eval_tables.h resample_taps_by_phase), so the loop has a fixed trip count and no bounds; the table
// (up T doubles: 71 KB at 100 / 441, up to 7.7 MB for a rate coprime to 10000) stays in L2.
// Ranges: k down <= 2^24 up = 1.7e11 and H + k down fit int64; phase T + q < up T <= 970,000 fits int.
// Dynamic LDS: resample_span float2.
__global__ __launch_bounds__(kThreads) void k_eval_resample_big(const float* __restrict__ ref,
                                                                const float* __restrict__ deg,
                                                                const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                                double* __restrict__ x10, double* __restrict__ y10) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int T = 2 * t.H / t.up + 1, span = resample_span(t.up, t.down, t.H);
    float2* xy = reinterpret_cast<float2*>(lds);
    const int64_t u = blockIdx.x;
    const Pair p = pair_geom(off, U, u, t);
    const float* s = ref + off[u];
    const float* y = deg + off[u];
    for (int64_t k0 = (int64_t)blockIdx.y * kThreads; k0 < p.n10; k0 += (int64_t)gridDim.y * kThreads) {
        const int64_t jlo = (t.H + k0 * t.down) / t.up - (T - 1);   // the tile's first input sample (may be negative)
        __syncthreads();                                             // the previous tile's reads
        for (int i = threadIdx.x; i < span; i += kThreads) {
            const int64_t j = jlo + i;
            const bool in = j >= 0 && j < p.n;
            xy[i] = make_float2(in ? s[j] : 0.f, in ? y[j] : 0.f);
        }
        __syncthreads();
        const int64_t k = k0 + threadIdx.x;
        if (k < p.n10) {
            const int64_t c = t.H + k * t.down;
            const int64_t B = c / t.up;
            const int phase = (int)(c - B * t.up);
            const int i0 = (int)(B - (T - 1) - jlo);                 // 0 <= i0, i0 + T <= 255 down / up + 1 + T < span
            const double* hp = t.ptaps + phase * T;
            double ax = 0.0, ay = 0.0;
            for (int q = 0; q < T; ++q) {
                const double w = hp[q];
                const float2 v = xy[i0 + q];
                ax += w * (double)v.x;
                ay += w * (double)v.y;
            }
            x10[p.s10 + k] = ax;
            y10[p.s10 + k] = ay;
        }
    }
}

// ---- STOI: frame energies of the clean signal ---------------------------------------------------
// grid (pairs, G): one wave per frame, e = 20 log10(||W x_f|| + eps).
__global__ __launch_bounds__(kThreads) void k_eval_energy(const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                          const double* __restrict__ x10, double* __restrict__ en) {
    const int64_t u = blockIdx.x;
    const Pair p = pair_geom(off, U, u, t);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t f = (int64_t)blockIdx.y * kWaves + wave; f < p.F; f += (int64_t)gridDim.y * kWaves) {
        const double* x = x10 + p.s10 + f * 128;
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double v = t.W[lane + 64 * k] * x[lane + 64 * k];
            a += v * v;
        }
        a = wave_sum(a);
        if (lane == 0) en[p.fs + f] = 20.0 * log10(sqrt(a) + kEps);
    }
}

// One workgroup per pair: the maximum energy, the mask e > max - 40, and its exclusive scan into the list of kept
// frames (ascending).  K goes to kept[u] and to slot 4.
__global__ __launch_bounds__(kThreads) void k_eval_mask(const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                        const double* __restrict__ en, int* __restrict__ idx,
                                                        int* __restrict__ kept, double* __restrict__ metrics) {
    __shared__ double wmax[kWaves];
    __shared__ int wcnt[kWaves];
    const int64_t u = blockIdx.x;
    const Pair p = pair_geom(off, U, u, t);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double* e = en + p.fs;
    double mx = -HUGE_VAL;
    for (int64_t f = threadIdx.x; f < p.F; f += kThreads) mx = fmax(mx, e[f]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    mx = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
    const double thr = mx - 40.0;
    int K = 0;
    for (int64_t f0 = 0; f0 < p.F; f0 += kThreads) {
        const int64_t f = f0 + threadIdx.x;
        const bool keep = f < p.F && e[f] > thr;
        const unsigned long long b = __ballot(keep);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();   // wcnt of the previous tile has been read
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        int pos = K + before;
        for (int w = 0; w < wave; ++w) pos += wcnt[w];
        if (keep) idx[p.fs + pos] = (int)f;
        K += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
    if (threadIdx.x == 0) {
        kept[u] = K;
        metrics[u * t.ms + 4] = p.n > 0 ? (double)K : quiet_nan();
    }
}

// ---- STOI: band spectra -------------------------------------------------------------------------
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 mul_mi(double2 a) { return make_double2(a.y, -a.x); }   // a * (-i)

// In-place 8-point DFT, natural order in and out: v[k] = sum_n v[n] e^{-2 pi i n k / 8}.  HALF: v[4..7] are zero.
template <bool HALF>
__device__ __forceinline__ void dft8(double2 v[8]) {
    const double r = 0.70710678118654752440;
    double2 a0, a1, a2, a3, a4, a5, a6, a7;
    if (HALF) {
        a0 = v[0]; a1 = v[0]; a2 = v[2]; a3 = mul_mi(v[2]);
        a4 = v[1]; a5 = v[1]; a6 = v[3]; a7 = mul_mi(v[3]);
    } else {
        a0 = cadd(v[0], v[4]); a1 = csub(v[0], v[4]); a2 = cadd(v[2], v[6]); a3 = mul_mi(csub(v[2], v[6]));
        a4 = cadd(v[1], v[5]); a5 = csub(v[1], v[5]); a6 = cadd(v[3], v[7]); a7 = mul_mi(csub(v[3], v[7]));
    }
    const double2 e0 = cadd(a0, a2), e2 = csub(a0, a2), e1 = cadd(a1, a3), e3 = csub(a1, a3);   // DFT4 of the even inputs
    const double2 o0 = cadd(a4, a6), o2 = csub(a4, a6), o1 = cadd(a5, a7), o3 = csub(a5, a7);   // and of the odd ones
    const double2 w1 = cmul(o1, make_double2(r, -r)), w2 = mul_mi(o2), w3 = cmul(o3, make_double2(-r, -r));
    v[0] = cadd(e0, o0); v[4] = csub(e0, o0);
    v[1] = cadd(e1, w1); v[5] = csub(e1, w1);
    v[2] = cadd(e2, w2); v[6] = csub(e2, w2);
    v[3] = cadd(e3, w3); v[7] = csub(e3, w3);
}

// e^{-2 pi i e / 512}, 0 <= e < 512, from the table's first half
__device__ __forceinline__ double2 twid512(const double* __restrict__ tw, int e) {
    const int r = e & 255;
    const double2 w = make_double2(tw[2 * r], tw[2 * r + 1]);
    return (e & 256) ? make_double2(-w.x, -w.y) : w;
}

constexpr int kFftRow = 72;   // LDS row pitch of the 8 x 64 exchanges, in double2: rows 128 bytes apart modulo 256

// grid (pairs, G): one wave per output frame m < M = K - 1, four frames per workgroup step.  The 256 samples of frame m
// of the overlap-added signal come from the kept source frames m - 1, m, m + 1 (never materialised).  Clean and
// degraded go through one 512-point complex FFT as real and imaginary part and are separated by the conjugate
// symmetry.  The FFT is 8 x 8 x 8: each lane holds 8 points in registers for an 8-point DFT, with two exchanges through
// LDS between the three passes (n = 64 n1 + 8 a + b, k = k1 + 8 c + 64 d); the first pass sees the zero padding
// (n1 >= 4).  The barriers are workgroup-wide and every wave runs every step, so the trip count is uniform.
__global__ __launch_bounds__(kThreads) void k_eval_bands(const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                         const double* __restrict__ x10, const double* __restrict__ y10,
                                                         const int* __restrict__ idx, const int* __restrict__ kept,
                                                         double* __restrict__ XB, double* __restrict__ YB) {
    __shared__ double2 zbuf[kWaves][8 * kFftRow];
    __shared__ double W[256];
    const int64_t u = blockIdx.x;
    const Pair p = pair_geom(off, U, u, t);
    const int64_t M = (int64_t)kept[u] - 1;
    if (M < 30) return;   // block-uniform: STOI is NaN, nothing reads the bands
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int hi3 = lane >> 3, lo3 = lane & 7;
    W[tid] = t.W[tid];
    double2 t1[8], t2[8];   // pass-1 twiddles e^{-2 pi i lane k1 / 512}, pass-2 twiddles e^{-2 pi i b c / 64}
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        t1[k] = twid512(t.twid, lane * k);
        t2[k] = twid512(t.twid, 8 * lo3 * k);
    }
    // band sums: lanes 2 q and 2 q + 1 take the two halves of (signal, band) q = signal * 15 + band
    const int q = lane >> 1, sig = q / 15, band = q % 15;
    int blo = 0, bhi = 0;
    if (lane < 60) {
        const int lo = t.bands[2 * band], hi = t.bands[2 * band + 1], mid = (lo + hi + 1) >> 1;
        blo = (lane & 1) ? mid : lo;
        bhi = (lane & 1) ? hi : mid;
    }
    double2* z = zbuf[wave];
    const double* x = x10 + p.s10;
    const double* y = y10 + p.s10;
    const int* src = idx + p.fs;
    __syncthreads();
    for (int64_t m0 = (int64_t)blockIdx.y * kWaves; m0 < M; m0 += (int64_t)gridDim.y * kWaves) {
        const int64_t m = m0 + wave;
        const bool live = m < M;
        double2 v[8];
#pragma unroll
        for (int n1 = 0; n1 < 4; ++n1) {
            const int i = lane + 64 * n1;   // sample of the frame
            double ox = 0.0, oy = 0.0;
            if (live) {
                if (n1 < 2) {               // source frames m - 1 (its second half) and m (its first half), in order
                    if (m >= 1) {
                        const int64_t a = (int64_t)src[m - 1] * 128 + i + 128;
                        ox = W[i + 128] * x[a];
                        oy = W[i + 128] * y[a];
                    }
                    const int64_t b = (int64_t)src[m] * 128 + i;
                    ox += W[i] * x[b];
                    oy += W[i] * y[b];
                } else {                    // source frames m (its second half) and m + 1 (its first half)
                    const int64_t a = (int64_t)src[m] * 128 + i;
                    const int64_t b = (int64_t)src[m + 1] * 128 + i - 128;
                    ox = W[i] * x[a] + W[i - 128] * x[b];
                    oy = W[i] * y[a] + W[i - 128] * y[b];
                }
            }
            v[n1] = make_double2(W[i] * ox, W[i] * oy);
        }
#pragma unroll
        for (int k = 4; k < 8; ++k) v[k] = make_double2(0.0, 0.0);
        // pass 1: over n1 -> k1 (lane = n2), then the twiddle e^{-2 pi i n2 k1 / 512}
        dft8<true>(v);
#pragma unroll
        for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], t1[k]);
#pragma unroll
        for (int k = 0; k < 8; ++k) z[k * kFftRow + lane] = v[k];
        __syncthreads();
        // pass 2: lane = (k1, b) takes n2 = 8 a + b over a -> c, then e^{-2 pi i b c / 64}
#pragma unroll
        for (int a = 0; a < 8; ++a) v[a] = z[hi3 * kFftRow + 8 * a + lo3];
        dft8<false>(v);
#pragma unroll
        for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], t2[k]);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 8; ++c) z[hi3 * kFftRow + lo3 * 9 + c] = v[c];
        __syncthreads();
        // pass 3: lane = (k1, c) over b -> d; bin k1 + 8 c + 64 d
#pragma unroll
        for (int b = 0; b < 8; ++b) v[b] = z[hi3 * kFftRow + b * 9 + lo3];
        dft8<false>(v);
        __syncthreads();
#pragma unroll
        for (int d = 0; d < 8; ++d) z[hi3 + 8 * lo3 + 64 * d] = v[d];
        __syncthreads();
        // |X|^2 and |Y|^2 of bins 7 .. 218: X = (Z[k] + conj(Z[N - k])) / 2, Y = (Z[k] - conj(Z[N - k])) / (2 i)
        double2 pw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 7 + lane + 64 * i;
            pw[i] = make_double2(0.0, 0.0);
            if (k < 219) {
                const double2 a = z[k], b = z[512 - k];
                const double xr = 0.5 * (a.x + b.x), xi = 0.5 * (a.y - b.y);
                const double yr = 0.5 * (a.y + b.y), yi = -0.5 * (a.x - b.x);
                pw[i] = make_double2(xr * xr + xi * xi, yr * yr + yi * yi);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 7 + lane + 64 * i;
            if (k < 219) z[k] = pw[i];
        }
        __syncthreads();
        // a band's bins in bin order, as two runs: the first half, the second half, then first + second
        double acc = 0.0;
        for (int k = blo; k < bhi; ++k) acc += sig == 0 ? z[k].x : z[k].y;
        const double other = __shfl_xor(acc, 1, 64);
        if (live && lane < 60 && !(lane & 1))
            (sig == 0 ? XB : YB)[15 * p.fs + (int64_t)band * M + m] = sqrt(acc + other);
        __syncthreads();
    }
}

// ---- STOI: segment correlations -----------------------------------------------------------------
// grid (pairs, G): one (segment, band) per thread and step; the 30 frames ending at m = 30 + segment.
__global__ __launch_bounds__(kThreads) void k_eval_corr(const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                        const double* __restrict__ XB, const double* __restrict__ YB,
                                                        const int* __restrict__ kept, double* __restrict__ d) {
    const int64_t u = blockIdx.x;
    const Pair p = pair_geom(off, U, u, t);
    const int64_t M = (int64_t)kept[u] - 1;
    if (M < 30) return;
    const int64_t items = 15 * (M - 29);
    const double clip = 1.0 + 5.623413251903491;   // 1 + 10^(15 / 20)
    for (int64_t it = (int64_t)blockIdx.y * kThreads + threadIdx.x; it < items; it += (int64_t)gridDim.y * kThreads) {
        const int64_t seg = it / 15;
        const int j = (int)(it % 15);
        const double* X = XB + 15 * p.fs + (int64_t)j * M + seg;
        const double* Y = YB + 15 * p.fs + (int64_t)j * M + seg;
        double xs[30], ys[30];
        double sx2 = 0.0, sy2 = 0.0;
#pragma unroll
        for (int k = 0; k < 30; ++k) {
            xs[k] = X[k];
            ys[k] = Y[k];
            sx2 += xs[k] * xs[k];
            sy2 += ys[k] * ys[k];
        }
        const double a = sqrt(sx2 / (sy2 + kEps));
        double mx = 0.0, my = 0.0;
#pragma unroll
        for (int k = 0; k < 30; ++k) {
            ys[k] = fmin(a * ys[k], xs[k] * clip);
            mx += xs[k];
            my += ys[k];
        }
        mx /= 30.0;
        my /= 30.0;
        double cxy = 0.0, cxx = 0.0, cyy = 0.0;
#pragma unroll
        for (int k = 0; k < 30; ++k) {
            const double dx = xs[k] - mx, dy = ys[k] - my;
            cxy += dx * dy;
            cxx += dx * dx;
            cyy += dy * dy;
        }
        d[15 * p.fs + it] = cxy / (sqrt(cxx) * sqrt(cyy) + kEps);
    }
}

// ---- ESTOI: segment correlations ----------------------------------------------------------------
constexpr int kSegPitch = 31;   // LDS row pitch of a 15 x 30 tile, in doubles: odd, so rows and columns both spread over the banks

// grid (pairs, G): one wave per segment (the 30 frames ending at m = 30 + segment), four segments per workgroup step.
// The 15 x 30 tiles of X and Y go to LDS.  1: lanes 0 .. 29 take one (signal, band) row each: the mean over its 30
// frames in frame order, the row minus the mean, the norm of that from the squares in frame order, the row over
// (norm + eps), back to LDS.  2: lanes 0 .. 29 take one frame each, the column of X and of Y in registers: the same
// over the 15 bands in band order, then the column's sum of x y in band order.  Lane 0 adds the 30 column sums in
// frame order and stores the sum over 30.  The barriers are workgroup-wide and every wave runs every step.
__global__ __launch_bounds__(kThreads) void k_eval_ecorr(const int64_t* __restrict__ off, int64_t U, EvalDev t,
                                                         const double* __restrict__ XB, const double* __restrict__ YB,
                                                         const int* __restrict__ kept, double* __restrict__ de) {
    __shared__ double tile[kWaves][2][15 * kSegPitch];
    __shared__ double colsum[kWaves][32];
    const int64_t u = blockIdx.x;
    const Pair p = pair_geom(off, U, u, t);
    const int64_t M = (int64_t)kept[u] - 1;
    if (M < 30) return;   // block-uniform: ESTOI is NaN
    const int64_t nseg = M - 29;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double* X = XB + 15 * p.fs;
    const double* Y = YB + 15 * p.fs;
    for (int64_t s0 = (int64_t)blockIdx.y * kWaves; s0 < nseg; s0 += (int64_t)gridDim.y * kWaves) {
        const int64_t seg = s0 + wave;
        const bool live = seg < nseg;
        __syncthreads();   // the previous step's reads
        for (int i = lane; i < 2 * 15 * 30; i += 64) {
            const int sig = i / 450, r = i - 450 * sig, j = r / 30, k = r - 30 * j;
            tile[wave][sig][j * kSegPitch + k] = live ? (sig ? Y : X)[(int64_t)j * M + seg + k] : 0.0;
        }
        __syncthreads();
        if (lane < 30) {
            double* row = tile[wave][lane / 15] + (lane % 15) * kSegPitch;
            double v[30];
            double mean = 0.0, sq = 0.0;
#pragma unroll
            for (int k = 0; k < 30; ++k) {
                v[k] = row[k];
                mean += v[k];
            }
            mean /= 30.0;
#pragma unroll
            for (int k = 0; k < 30; ++k) {
                v[k] -= mean;
                sq += v[k] * v[k];
            }
            const double den = sqrt(sq) + kEps;
#pragma unroll
            for (int k = 0; k < 30; ++k) row[k] = v[k] / den;
        }
        __syncthreads();
        if (lane < 30) {
            double xc[15], yc[15];
            double mx = 0.0, my = 0.0, qx = 0.0, qy = 0.0, dot = 0.0;
#pragma unroll
            for (int j = 0; j < 15; ++j) {
                xc[j] = tile[wave][0][j * kSegPitch + lane];
                yc[j] = tile[wave][1][j * kSegPitch + lane];
                mx += xc[j];
                my += yc[j];
            }
            mx /= 15.0;
            my /= 15.0;
#pragma unroll
            for (int j = 0; j < 15; ++j) {
                xc[j] -= mx;
                yc[j] -= my;
                qx += xc[j] * xc[j];
                qy += yc[j] * yc[j];
            }
            const double dx = sqrt(qx) + kEps, dy = sqrt(qy) + kEps;
#pragma unroll
            for (int j = 0; j < 15; ++j) dot += (xc[j] / dx) * (yc[j] / dy);
            colsum[wave][lane] = dot;
        }
        __syncthreads();
        if (lane == 0 && live) {
            double tot = 0.0;
            for (int k = 0; k < 30; ++k) tot += colsum[wave][k];
            de[p.fs + seg] = tot / 30.0;
        }
    }
}

struct Layout {
    size_t partial, sums, kept, segv, x10, y10, en, idx, xb, yb, d, de, total;
};

// estoi: the ESTOI values behind everything else, so the other offsets (and the total without it) do not move
Layout eval_layout(int64_t U, int64_t cap, int up, int down, int skip, bool stoi, bool estoi) {
    Layout L;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += (bytes + 255) & ~(size_t)255;
        return at;
    };
    L.partial = take(sizeof(double) * 3 * kParts * (size_t)U);
    L.sums = take(sizeof(double) * 4 * (size_t)U);
    L.kept = take(sizeof(int) * (size_t)U);
    L.segv = take(sizeof(double) * (size_t)(cap / skip + 1));
    const size_t cap10 = stoi ? (size_t)(cap * up / down + U + 1) : 0;
    const size_t capf = stoi ? cap10 / 128 + 1 : 0;
    L.x10 = take(sizeof(double) * cap10);
    L.y10 = take(sizeof(double) * cap10);
    L.en = take(sizeof(double) * capf);
    L.idx = take(sizeof(int) * capf);
    L.xb = take(sizeof(double) * 15 * capf);
    L.yb = take(sizeof(double) * 15 * capf);
    L.d = take(sizeof(double) * 15 * capf);
    L.de = take(sizeof(double) * (estoi ? capf : 0));
    L.total = o;
    return L;
}

}  // namespace

size_t eval_pairs_scratch_bytes(int64_t n_pairs, const EvalDev& t) {
    return eval_layout(n_pairs, t.cap, t.up, t.down, t.skip, t.stoi != 0, t.stoi != 0 && t.ms > 5).total;
}

int launch_eval_pairs(const float* ref, const float* deg, const int64_t* off, int64_t U, const EvalDev& t,
                      double* metrics, void* scratch, hipStream_t s) {
    const Layout L = eval_layout(U, t.cap, t.up, t.down, t.skip, t.stoi != 0, t.stoi != 0 && t.ms > 5);
    char* base = reinterpret_cast<char*>(scratch);
    double* partial = reinterpret_cast<double*>(base + L.partial);
    double* sums = reinterpret_cast<double*>(base + L.sums);
    int* kept = reinterpret_cast<int*>(base + L.kept);
    double* segv = reinterpret_cast<double*>(base + L.segv);
    double* x10 = reinterpret_cast<double*>(base + L.x10);
    double* y10 = reinterpret_cast<double*>(base + L.y10);
    double* en = reinterpret_cast<double*>(base + L.en);
    int* idx = reinterpret_cast<int*>(base + L.idx);
    double* xb = reinterpret_cast<double*>(base + L.xb);
    double* yb = reinterpret_cast<double*>(base + L.yb);
    double* d = reinterpret_cast<double*>(base + L.d);
    // workgroups per pair of the kernels whose work items are independent (any value gives the same bits)
    const unsigned G = (unsigned)std::max<int64_t>(4, std::min<int64_t>(256, 8192 / U));
    const unsigned gu = (unsigned)U;
    const dim3 per_pair(gu), blk(kThreads), wide(gu, G), fin((unsigned)((U + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(k_eval_sums<0>, dim3(gu, kParts), blk, 0, s, ref, deg, off, U, t, (const double*)sums, partial);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_sums_finish<0>, fin, blk, 0, s, off, U, t, (const double*)partial, sums, metrics);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_sums<1>, dim3(gu, kParts), blk, 0, s, ref, deg, off, U, t, (const double*)sums, partial);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_sums_finish<1>, fin, blk, 0, s, off, U, t, (const double*)partial, sums, metrics);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_seg, wide, blk, 0, s, ref, deg, off, U, t, segv);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_mean<0>, per_pair, blk, 0, s, off, U, t, (const double*)segv, (const int*)kept, metrics);
    AVSE_HIP_CHECK(hipGetLastError());
    if (!t.stoi) return 0;
    const int span = resample_span(t.up, t.down, t.H);
    if (t.ptaps) {
        hipLaunchKernelGGL(k_eval_resample_big, wide, blk, sizeof(float2) * (size_t)span, s, ref, deg, off, U, t, x10, y10);
    } else {
        const size_t res_lds = sizeof(double) * (size_t)(t.up + 2 * t.H + 1) + 2 * sizeof(float) * (size_t)span;
        hipLaunchKernelGGL(k_eval_resample, wide, blk, res_lds, s, ref, deg, off, U, t, x10, y10);
    }
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_energy, wide, blk, 0, s, off, U, t, (const double*)x10, en);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_mask, per_pair, blk, 0, s, off, U, t, (const double*)en, idx, kept, metrics);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_bands, wide, blk, 0, s, off, U, t, (const double*)x10, (const double*)y10,
                       (const int*)idx, (const int*)kept, xb, yb);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_corr, wide, blk, 0, s, off, U, t, (const double*)xb, (const double*)yb,
                       (const int*)kept, d);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_mean<1>, per_pair, blk, 0, s, off, U, t, (const double*)d, (const int*)kept, metrics);
    AVSE_HIP_CHECK(hipGetLastError());
    if (t.ms <= 5) return 0;
    double* de = reinterpret_cast<double*>(base + L.de);
    hipLaunchKernelGGL(k_eval_ecorr, wide, blk, 0, s, off, U, t, (const double*)xb, (const double*)yb,
                       (const int*)kept, de);
    AVSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_mean<2>, per_pair, blk, 0, s, off, U, t, (const double*)de, (const int*)kept, metrics);
    AVSE_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace avse
