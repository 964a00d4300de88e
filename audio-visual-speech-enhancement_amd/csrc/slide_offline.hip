// The offline sliding path (include/avse.h avse_slide_windows / avse_slide_video_windows / avse_slide_keep; DESIGN.md
// §3 K22): whole utterances through the windows of a flushed sliding session in ragged batches.  Three data movers
// between the existing ragged STFT, forward and ragged ISTFT, driven by the host rows and item tables of
// slide_offline_geom.h (uploaded into the context's preprocess scratch as a ragged spectrogram's tables go):
//   k_slide_off_scan     per utterance, the inclusive prefix maximum along time of the unclamped mel-dB's column maxima
//   k_slide_off_windows  window j of an utterance = max(x, prefixmax[q s j + spf - 1] - top_db), the causal floor
//   k_slide_off_video    windows [w0, w0 + n) of the video: [128][128][F] clips that start at every s-th frame of the slices
//   k_slide_off_keep     the kept columns of the predicted windows, packed [n_mels][P_u] per utterance
// Nothing here rounds: the kernels move values and take maxima, which are exact in any order.
#include <cmath>
#include <cstring>
#include <string>

#include "ctx.h"
#include "slide_offline_geom.h"

namespace avse {
namespace {

// ---- causal clamp ------------------------------------------------------------------------------------------------
// One block per utterance with windows.  Thread i of chunk c takes frame t = 256 c + i: the maximum of its n_mels
// values (row-major [n_mels][T]: a wave reads 64 consecutive floats per row), then an inclusive scan over the block
// (xor-free shuffles up within a wave, the waves' totals through LDS) on top of the carry of the chunks before.
// fmaxf drops a NaN where torch's max() would propagate it: "the bits of the torch composition" holds for NaN-free
// mel-dB, which is all the STFT writes (20 log10 of a value clamped at amin > 0).
__global__ __launch_bounds__(SLIDE_OFF_SCAN) void k_slide_off_scan(const float* __restrict__ mel, float* __restrict__ pmax,
                                                                    int n_mels, const SlideOffRow* __restrict__ rows,
                                                                    const StreamItem* __restrict__ items) {
    __shared__ float wave_max[SLIDE_OFF_SCAN / 64];
    const SlideOffRow& r = rows[items[blockIdx.x].b];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* x = mel + r.t_off * n_mels;
    float carry = -INFINITY;
    for (int t0 = 0; t0 < r.T; t0 += SLIDE_OFF_SCAN) {
        const int t = t0 + tid;
        float v = -INFINITY;
        if (t < r.T)
            for (int m = 0; m < n_mels; ++m) v = fmaxf(v, x[(long long)m * r.T + t]);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(v, o);
            if (lane >= o) v = fmaxf(v, up);
        }
        if (lane == 63) wave_max[wv] = v;
        __syncthreads();
        float before = carry;
        for (int k = 0; k < wv; ++k) before = fmaxf(before, wave_max[k]);
        v = fmaxf(v, before);
        if (t < r.T) pmax[r.t_off + t] = v;
#pragma unroll
        for (int k = 0; k < SLIDE_OFF_SCAN / 64; ++k) carry = fmaxf(carry, wave_max[k]);
        __syncthreads();   // wave_max is rewritten by the next chunk
    }
}

// Windows [WPB chunk, ..) of utterance item.b.  A thread takes four consecutive columns of a row (spf % 4 == 0: one
// 16-byte store; the source row starts at any float, so its loads are scalar) or, otherwise, one value at a time.
__global__ __launch_bounds__(256) void k_slide_off_windows(const float* __restrict__ mel, const float* __restrict__ pmax,
                                                           float* __restrict__ net_in, int n_mels, int spf, int qs, float top_db,
                                                           const SlideOffRow* __restrict__ rows,
                                                           const StreamItem* __restrict__ items) {
    const StreamItem it = items[blockIdx.x];
    const SlideOffRow& r = rows[it.b];
    const float* x = mel + r.t_off * n_mels;
    const int j_end = min(r.W, (it.chunk + 1) * SLIDE_OFF_WPB);
    const int per = n_mels * spf;
    for (int j = it.chunk * SLIDE_OFF_WPB; j < j_end; ++j) {
        const int t0 = qs * j;
        const float floor_db = top_db >= 0.f ? pmax[r.t_off + t0 + spf - 1] - top_db : -INFINITY;
        float* dst = net_in + (r.w_off + j) * (long long)per;
        if ((spf & 3) == 0) {
            for (int i = threadIdx.x * 4; i < per; i += 256 * 4) {
                const int m = i / spf, c = i - m * spf;
                const float* src = x + (long long)m * r.T + t0 + c;
                float4 v;
                v.x = fmaxf(src[0], floor_db);
                v.y = fmaxf(src[1], floor_db);
                v.z = fmaxf(src[2], floor_db);
                v.w = fmaxf(src[3], floor_db);
                *reinterpret_cast<float4*>(dst + i) = v;
            }
        } else {
            for (int i = threadIdx.x; i < per; i += 256) {
                const int m = i / spf, c = i - m * spf;
                dst[i] = fmaxf(x[(long long)m * r.T + t0 + c], floor_db);
            }
        }
    }
}

// ---- kept columns ------------------------------------------------------------------------------------------------
// Columns [KEEP chunk, ..) of utterance item.b's packed [n_mels][P].  With vec4 (spf and q multiples of 4: every run of
// kept columns starts at a multiple of 4 on both sides, and so does every row) a thread moves four columns as one
// 16-byte vector; otherwise one column.  Threads run along the columns, so the stores of a row are contiguous.
template <bool VEC4>
__global__ __launch_bounds__(256) void k_slide_off_keep(const float* __restrict__ pred, float* __restrict__ out, int n_mels,
                                                        int spf, int qs, const SlideOffRow* __restrict__ rows,
                                                        const StreamItem* __restrict__ items) {
    constexpr int V = VEC4 ? 4 : 1;
    const StreamItem it = items[blockIdx.x];
    const SlideOffRow& r = rows[it.b];
    const int c0 = it.chunk * SLIDE_OFF_KEEP, c1 = min(r.P, c0 + SLIDE_OFF_KEEP);
    const int ncol = (c1 - c0) / V;
    float* dst = out + r.p_off * n_mels;
    for (int i = threadIdx.x; i < ncol * n_mels; i += 256) {
        const int m = i / ncol, t = c0 + (i - m * ncol) * V;
        const int j = t < spf ? 0 : (t - spf) / qs + 1;
        const float* src = pred + ((r.w_off + j) * (long long)n_mels + m) * spf + (t - qs * j);
        float* d = dst + (long long)m * r.P + t;
        if constexpr (VEC4) *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(src);
        else *d = *src;
    }
}

// ---- video windows -----------------------------------------------------------------------------------------------
// Part chunk % VX of window j = j0 + chunk / VX of row item.b.  The window's frames s j .. s j + F - 1 start at element
// R = s j % F of slice k = s j / F: pixel p of the window is elements [R, F) of pixel p of slice k, then elements [0, R)
// of pixel p of slice k + 1.  A thread takes G = 16 / sizeof(T) pixels: their F 16-byte vectors of slice k, with R > 0
// the F vectors of slice k + 1 too, rotates the elements in registers (R is a template argument, so every index is a
// constant) and stores F whole vectors.  The last window of an utterance ends inside its last slice, so slice k + 1 is
// read only where it exists.
template <class T, int F, int R>
__device__ __forceinline__ void video_window_part(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                                  uint4* __restrict__ dst, int g_begin, int g_end) {
    constexpr int G = 16 / (int)sizeof(T);
    for (int g = g_begin + threadIdx.x; g < g_end; g += 256) {
        union { uint4 v[F]; T e[G * F]; } lo, hi, o;
#pragma unroll
        for (int i = 0; i < F; ++i) lo.v[i] = a[(long long)g * F + i];
        if constexpr (R > 0) {
#pragma unroll
            for (int i = 0; i < F; ++i) hi.v[i] = b[(long long)g * F + i];
        }
#pragma unroll
        for (int p = 0; p < G; ++p)
#pragma unroll
            for (int i = 0; i < F; ++i) {
                if constexpr (R > 0) o.e[p * F + i] = i + R < F ? lo.e[p * F + i + R] : hi.e[p * F + i + R - F];
                else o.e[p * F + i] = lo.e[p * F + i];
            }
#pragma unroll
        for (int i = 0; i < F; ++i) dst[(long long)g * F + i] = o.v[i];
    }
}

template <class T, int F>
__global__ __launch_bounds__(256) void k_slide_off_video(const char* __restrict__ video, char* __restrict__ out, int stride,
                                                         const SlideOffVidRow* __restrict__ rows,
                                                         const StreamItem* __restrict__ items) {
    constexpr int G = 16 / (int)sizeof(T);
    constexpr long long SB = 128LL * 128 * F * sizeof(T);      // bytes of a slice, and of a window
    constexpr int NG = 128 * 128 / G;                            // pixel groups per window
    const StreamItem it = items[blockIdx.x];
    const SlideOffVidRow& r = rows[it.b];
    const int kk = it.chunk / SLIDE_OFF_VX, part = it.chunk - SLIDE_OFF_VX * kk;
    const long long fr = (long long)stride * (r.j0 + kk);
    const long long k = fr / F;
    const int rot = (int)(fr - k * F);
    const uint4* a = reinterpret_cast<const uint4*>(video + (r.s_off + k) * SB);
    const uint4* b = reinterpret_cast<const uint4*>(video + (r.s_off + k + 1) * SB);
    uint4* dst = reinterpret_cast<uint4*>(out + (r.out0 + kk) * SB);
    const int g0 = part * (NG / SLIDE_OFF_VX), g1 = g0 + NG / SLIDE_OFF_VX;
    switch (rot) {      // uniform over the block
        case 0: video_window_part<T, F, 0>(a, b, dst, g0, g1); break;
        case 1: video_window_part<T, F, 1>(a, b, dst, g0, g1); break;
        case 2: video_window_part<T, F, 2>(a, b, dst, g0, g1); break;
        case 3: video_window_part<T, F, 3>(a, b, dst, g0, g1); break;
        case 4: video_window_part<T, F, 4>(a, b, dst, g0, g1); break;
        default:
            if constexpr (F > 5) video_window_part<T, F, 5>(a, b, dst, g0, g1);
            break;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------
// Room for `need` bytes of tables in the pinned copy and in the preprocess scratch (plus `extra` bytes of device
// scratch behind them): the rule of a ragged spectrogram's tables (capi.hip upload_ragged).  The caller fills
// c->ragged_host and calls tables_up.
int tables_room(avse_ctx* c, size_t need, size_t extra, hipStream_t s, bool* capturing) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (s) AVSE_HIP_CHECK(hipStreamIsCapturing(s, &cs));
    *capturing = cs != hipStreamCaptureStatusNone;
    if (int rc = grow(c->prep, need + extra, s, "preprocess scratch")) return rc;
    if (!*capturing && c->ragged_done) AVSE_HIP_CHECK(hipEventSynchronize(c->ragged_done));   // the last upload has read it
    if (int rc = grow(c->ragged_host, need, s, "ragged tables")) return rc;
    if (!c->ragged_done) AVSE_HIP_CHECK(hipEventCreateWithFlags(&c->ragged_done, hipEventDisableTiming));
    return 0;
}

int tables_up(avse_ctx* c, size_t need, hipStream_t s, bool capturing) {
    AVSE_HIP_CHECK(hipMemcpyAsync(c->prep, c->ragged_host, need, hipMemcpyHostToDevice, s));
    if (!capturing) AVSE_HIP_CHECK(hipEventRecord(c->ragged_done, s));
    return 0;
}

int refuse(int status, int64_t bad) {
    return fail(AVSE_ERR_INVALID, std::string(slide_off_message(status)) + (bad >= 0 ? " (utterance " + std::to_string(bad) + ")" : ""));
}

constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

template <class T>
void launch_video(int F, unsigned blocks, hipStream_t s, const void* video, void* out, int stride, const SlideOffVidRow* rows,
                  const StreamItem* items) {
    if (F == 5)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_slide_off_video<T, 5>), dim3(blocks), dim3(256), 0, s, (const char*)video, (char*)out,
                           stride, rows, items);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_slide_off_video<T, 6>), dim3(blocks), dim3(256), 0, s, (const char*)video, (char*)out,
                           stride, rows, items);
}

}  // namespace
}  // namespace avse

using namespace avse;

extern "C" {

int avse_slide_windows(avse_ctx* c, const float* mel_db, const int64_t* n_frames, const int64_t* n_slices, int64_t n_utt,
                       int frames_per_slice, int video_frames, int stride, int n_mels, float top_db, float* net_in,
                       void* stream) {
    if (!c || !mel_db || !n_frames || !n_slices || !net_in) return fail(AVSE_ERR_INVALID, "NULL argument");
    const SlideOffCfg g{frames_per_slice, video_frames, stride};
    const SlideOffPlan p0 = slide_off_plan(g, n_slices, n_frames, n_utt, n_mels, nullptr);
    if (p0.status != SLIDE_OFF_OK) return refuse(p0.status, p0.bad);
    if ((uintptr_t)net_in % 16) return fail(AVSE_ERR_INVALID, "net_in must be 16-byte aligned");
    if (p0.windows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    const size_t rb = sizeof(SlideOffRow) * (size_t)n_utt, sb = sizeof(StreamItem) * (size_t)p0.items.scan,
                 wb = sizeof(StreamItem) * (size_t)p0.items.windows;
    const size_t need = align16(rb + sb + wb);
    bool capturing = false;
    if (int rc = tables_room(c, need, sizeof(float) * (size_t)p0.frames, s, &capturing)) return rc;
    SlideOffRow* rows = reinterpret_cast<SlideOffRow*>(c->ragged_host.p.get());
    slide_off_plan(g, n_slices, n_frames, n_utt, n_mels, rows);
    slide_off_fill_items(rows, n_utt, reinterpret_cast<StreamItem*>(c->ragged_host + rb),
                         reinterpret_cast<StreamItem*>(c->ragged_host + rb + sb), nullptr);
    if (int rc = tables_up(c, need, s, capturing)) return rc;
    const SlideOffRow* drows = reinterpret_cast<const SlideOffRow*>(c->prep.p.get());
    const StreamItem* scan = reinterpret_cast<const StreamItem*>(c->prep + rb);
    const StreamItem* wins = reinterpret_cast<const StreamItem*>(c->prep + rb + sb);
    float* pmax = reinterpret_cast<float*>(c->prep + need);
    if (top_db >= 0.f) {
        hipLaunchKernelGGL(k_slide_off_scan, dim3((unsigned)p0.items.scan), dim3(SLIDE_OFF_SCAN), 0, s, mel_db, pmax, n_mels, drows,
                           scan);
        AVSE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_slide_off_windows, dim3((unsigned)p0.items.windows), dim3(256), 0, s, mel_db, (const float*)pmax, net_in,
                       n_mels, g.spf, g.qs(), top_db, drows, wins);
    AVSE_HIP_CHECK(hipGetLastError());
    return debug_poll(stream);
}

int avse_slide_video_windows(avse_ctx* c, const void* video, int video_dtype, const int64_t* n_slices, int64_t n_utt,
                             int video_frames, int stride, int64_t w0, int64_t n, void* out, void* stream) {
    if (!c || !video || !n_slices || !out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (video_dtype != AVSE_VIDEO_F32 && video_dtype != AVSE_VIDEO_U8) return fail(AVSE_ERR_INVALID, "bad video dtype");
    const SlideOffCfg g{video_frames, video_frames, stride};      // q = 1: the video has no use for spf
    const SlideOffVidPlan v0 = slide_off_video_plan(g, n_slices, n_utt, w0, n, nullptr);
    if (v0.status != SLIDE_OFF_OK) return refuse(v0.status, v0.bad);
    if (video_frames != 5 && video_frames != 6) return fail(AVSE_ERR_UNSUPPORTED, "video windows are built for 5 and 6 video frames per slice");
    if ((uintptr_t)video % 16 || (uintptr_t)out % 16) return fail(AVSE_ERR_INVALID, "video and out must be 16-byte aligned");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    const size_t rb = sizeof(SlideOffVidRow) * (size_t)v0.rows, ib = sizeof(StreamItem) * (size_t)v0.items;
    bool capturing = false;
    if (int rc = tables_room(c, rb + ib, 0, s, &capturing)) return rc;
    SlideOffVidRow* rows = reinterpret_cast<SlideOffVidRow*>(c->ragged_host.p.get());
    slide_off_video_plan(g, n_slices, n_utt, w0, n, rows);
    slide_off_video_items(rows, v0.rows, reinterpret_cast<StreamItem*>(c->ragged_host + rb));
    if (int rc = tables_up(c, rb + ib, s, capturing)) return rc;
    const SlideOffVidRow* drows = reinterpret_cast<const SlideOffVidRow*>(c->prep.p.get());
    const StreamItem* items = reinterpret_cast<const StreamItem*>(c->prep + rb);
    if (video_dtype == AVSE_VIDEO_U8) launch_video<uint8_t>(video_frames, (unsigned)v0.items, s, video, out, stride, drows, items);
    else launch_video<float>(video_frames, (unsigned)v0.items, s, video, out, stride, drows, items);
    AVSE_HIP_CHECK(hipGetLastError());
    return debug_poll(stream);
}

int avse_slide_keep(avse_ctx* c, const float* pred_db, const int64_t* n_slices, int64_t n_utt, int frames_per_slice,
                    int video_frames, int stride, int n_mels, float* mel_db, void* stream) {
    if (!c || !pred_db || !n_slices || !mel_db) return fail(AVSE_ERR_INVALID, "NULL argument");
    const SlideOffCfg g{frames_per_slice, video_frames, stride};
    const SlideOffPlan p0 = slide_off_plan(g, n_slices, nullptr, n_utt, n_mels, nullptr);
    if (p0.status != SLIDE_OFF_OK) return refuse(p0.status, p0.bad);
    if ((uintptr_t)pred_db % 16 || (uintptr_t)mel_db % 16) return fail(AVSE_ERR_INVALID, "pred_db and mel_db must be 16-byte aligned");
    if (p0.predicted == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    const size_t rb = sizeof(SlideOffRow) * (size_t)n_utt, kb = sizeof(StreamItem) * (size_t)p0.items.keep;
    bool capturing = false;
    if (int rc = tables_room(c, rb + kb, 0, s, &capturing)) return rc;
    SlideOffRow* rows = reinterpret_cast<SlideOffRow*>(c->ragged_host.p.get());
    slide_off_plan(g, n_slices, nullptr, n_utt, n_mels, rows);
    slide_off_fill_items(rows, n_utt, nullptr, nullptr, reinterpret_cast<StreamItem*>(c->ragged_host + rb));
    if (int rc = tables_up(c, rb + kb, s, capturing)) return rc;
    const SlideOffRow* drows = reinterpret_cast<const SlideOffRow*>(c->prep.p.get());
    const StreamItem* items = reinterpret_cast<const StreamItem*>(c->prep + rb);
    const bool vec4 = g.spf % 4 == 0 && g.q() % 4 == 0;
    if (vec4)
        hipLaunchKernelGGL(k_slide_off_keep<true>, dim3((unsigned)p0.items.keep), dim3(256), 0, s, pred_db, mel_db, n_mels, g.spf,
                           g.qs(), drows, items);
    else
        hipLaunchKernelGGL(k_slide_off_keep<false>, dim3((unsigned)p0.items.keep), dim3(256), 0, s, pred_db, mel_db, n_mels, g.spf,
                           g.qs(), drows, items);
    AVSE_HIP_CHECK(hipGetLastError());
    return debug_poll(stream);
}

}  // extern "C"
