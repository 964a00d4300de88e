// The streaming frame retimer (include/avse.h avse_retime_*, avse_retimer_*): one kernel for the
// per-stream push, the flush and the one-shot ragged call, driven by the host rows of retime_geom.h.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ctx.h"
#include "retime_geom.h"

namespace avse {
namespace {

struct RetimeArgs {
    const char* frames;     // packed [n][128][128] of the call, stream-major; a row's frames start at its frame_off
    const char* hist;       // [2][B][128][128]: the copy a row names by hist_in
    char* hist_w;           // the same buffer, written at hist_out
    const char* pend;       // [2][B][128][128][F]
    char* pend_w;
    char* out;              // packed [slices][128][128][F]; a row's slices start at its out_slice
    int64_t p, q;
    int B;
    int wide;               // `frames` and `out` are both 16-byte aligned (host only: picks the kernel's WIDE form)
};

// 16 bytes per lane: one access where the pointers are 16-byte aligned (WIDE), else four 4-byte ones
template <bool WIDE>
__device__ __forceinline__ uint4 load16(const char* src) {
    if constexpr (WIDE) return *reinterpret_cast<const uint4*>(src);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(src);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <bool WIDE>
__device__ __forceinline__ void store16(char* dst, uint4 v) {
    if constexpr (WIDE) {
        *reinterpret_cast<uint4*>(dst) = v;
    } else {
        uint32_t* w = reinterpret_cast<uint32_t*>(dst);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
}

__device__ __forceinline__ uint32_t word_of(const uint4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// float32: float32((double(q - r) a + double(r) b) / double(q)): both products are exact in float64 (q, r < 2^17), so
// the value has one rounding at the add, one at the divide and one to float32 (the file is built with
// -ffp-contract=off).
__device__ __forceinline__ uint32_t blend_f32(uint32_t a, uint32_t b, int32_t q, int32_t r) {
    const double x = (double)(q - r) * (double)__uint_as_float(a), y = (double)r * (double)__uint_as_float(b);
    return __float_as_uint((float)((x + y) / (double)q));
}
// uint8: (2 (a (q - r) + b r) + q) div (2 q), round-half-up in integers.  The numerator n is below 2^26 and the
// quotient below 256, so trunc(float(n) * rcp), rcp = float(1 / 2q), is within one of it (the two float roundings
// move the product by less than 1e-4): one step either way makes it exact, with no integer division.
__device__ __forceinline__ uint32_t blend_u8(uint32_t a, uint32_t b, int32_t q, int32_t r, float rcp) {
    const uint32_t n = 2u * (a * (uint32_t)(q - r) + b * (uint32_t)r) + (uint32_t)q, d = 2u * (uint32_t)q;
    uint32_t t = (uint32_t)((float)n * rcp);
    int32_t rem = (int32_t)(n - t * d);
    if (rem < 0) { --t; rem += (int32_t)d; }
    if (rem >= (int32_t)d) ++t;
    return t;
}

// where input frame i of the row's stream starts (n_old - 1 <= i < n_new: retime_geom.h retime_source; any other i, which
// only a value that is thrown away asks for, reads the history's frame: always there when a stream has state)
template <typename T>
__device__ __forceinline__ const char* retime_frame(const RetimeArgs& a, const RetimeRow& r, int b, int64_t i) {
    constexpr size_t FRAME = sizeof(T) * RETIME_PIXELS;
    int64_t idx = 0;
    return retime_source(r, i, &idx) == RETIME_NEW ? a.frames + (size_t)idx * FRAME
                                                   : a.hist + ((size_t)r.hist_in * a.B + b) * FRAME;
}

// A block owns 16 bytes per lane of one frame-sized tile: 256 x 4 float32 pixels (8 rows of a frame, 16 tiles per
// frame) or 256 x 16 uint8 pixels (32 rows, 4 tiles).  A row's blocks are its slots of `tiles` blocks each: one slot
// per slice the call writes (the k_new complete ones into `out`, then the unfinished one into copy hist_out of pend);
// when frames arrived, the blocks of the last slot also copy the call's last frame into copy hist_out of hist (a call
// that feeds frames and touches no slice has one slot for that alone).  The call reads copy hist_in only, so one launch
// needs no barrier between streams or slots.
// A lane assembles its pixels' F output values in registers, frame innermost as the slice has them: 16 F contiguous
// bytes per lane in either dtype (4 px x F x 4 bytes, or 16 px x F x 1 byte), which go out as F 16-byte stores; the
// lanes of a wave cover 64 x 16 F contiguous bytes between them.  The frames of the slice that were final before this
// call come from copy hist_in of pend, in the same layout (F 16-byte loads).  All loads of a block (2 F frame pieces,
// the pending slice, the history's frame) are issued before the first value is used: the kernel is bound by the
// latency of its few loads per lane, not by arithmetic, so they must be in flight together.
template <typename T, int F, bool WIDE>
__global__ __launch_bounds__(RETIME_BLOCK) void k_retime(RetimeArgs a, const RetimeRow* __restrict__ rows, int n_rows) {
    constexpr int PPL = 16 / (int)sizeof(T);                  // pixels per lane
    constexpr int TILES = RETIME_PIXELS / (RETIME_BLOCK * PPL);
    constexpr size_t FRAME = sizeof(T) * RETIME_PIXELS, SLICE = FRAME * F;
    const int b = retime_row_of(rows, n_rows, (int)blockIdx.x);
    const RetimeRow r = rows[b];
    const int local = (int)blockIdx.x - r.blk0;
    const int slot = local / TILES, tile = local - slot * TILES;
    const size_t pix0 = ((size_t)tile * RETIME_BLOCK + threadIdx.x) * PPL, at = pix0 * sizeof(T);
    const int slots = r.n_slots > r.fed ? r.n_slots : r.fed;
    const bool keep_last = r.fed && slot == slots - 1;
    uint4 last = make_uint4(0, 0, 0, 0);
    if (keep_last) last = load16<WIDE>(retime_frame<T>(a, r, b, r.n_new - 1) + at);
    if (slot < r.n_slots) {
        const int64_t j0 = (r.g_old / F + slot) * F;              // the slice's first output frame
        const int n_pend = slot == 0 ? (int)(r.g_old - j0) : 0;   // its frames that were final before this call
        const int64_t left = r.g_new - j0;
        const int n_valid = left < F ? (int)left : F;             // below F: the unfinished slice
        int32_t rr[F];
        uint4 va[F], vb[F];
#pragma unroll
        for (int f = 0; f < F; ++f) {
            // a frame this block does not compute (pending, or not final yet) loads what a neighbour loads anyway
            const int fc = f < n_pend ? n_pend : f >= n_valid ? n_valid - 1 : f;
            int64_t i0, i1;
            retime_taps(a.p, a.q, r.n_new, j0 + fc, &i0, &i1, &rr[f]);
            va[f] = load16<WIDE>(retime_frame<T>(a, r, b, i0) + at);
            vb[f] = load16<WIDE>(retime_frame<T>(a, r, b, rr[f] ? i1 : i0) + at);
        }
        uint32_t w[4 * F];
        if (n_pend > 0) {
            const char* src = a.pend + ((size_t)r.hist_in * a.B + b) * SLICE + pix0 * F * sizeof(T);
#pragma unroll
            for (int i = 0; i < F; ++i) {
                const uint4 v = load16<true>(src + 16 * i);
                w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4 * F; ++i) w[i] = 0;
        }
        const float rcp = 1.0f / (float)(2 * a.q);
#pragma unroll
        for (int f = 0; f < F; ++f) {
            if (f < n_pend || f >= n_valid) continue;
#pragma unroll
            for (int px = 0; px < PPL; ++px) {
                const int o = px * F + f;   // the value's place among the lane's PPL x F
                if constexpr (sizeof(T) == 4) {
                    const uint32_t x = word_of(va[f], px), y = word_of(vb[f], px);
                    w[o] = rr[f] ? blend_f32(x, y, (int32_t)a.q, rr[f]) : x;   // r == 0: A[i0]'s bits
                } else {
                    const int sh = (px & 3) * 8, so = (o & 3) * 8;
                    const uint32_t x = (word_of(va[f], px >> 2) >> sh) & 0xffu, y = (word_of(vb[f], px >> 2) >> sh) & 0xffu;
                    const uint32_t v = rr[f] ? blend_u8(x, y, (int32_t)a.q, rr[f], rcp) : x;
                    w[o >> 2] = (w[o >> 2] & ~(0xffu << so)) | (v << so);
                }
            }
        }
        if (slot < r.k_new) {
            char* dst = a.out + ((size_t)r.out_slice + slot) * SLICE + pix0 * F * sizeof(T);
#pragma unroll
            for (int i = 0; i < F; ++i) store16<WIDE>(dst + 16 * i, make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]));
        } else {
            char* dst = a.pend_w + ((size_t)r.hist_out * a.B + b) * SLICE + pix0 * F * sizeof(T);
#pragma unroll
            for (int i = 0; i < F; ++i) store16<true>(dst + 16 * i, make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]));
        }
    }
    if (keep_last) store16<true>(a.hist_w + ((size_t)r.hist_out * a.B + b) * FRAME + at, last);
}

int retime_cfg_checked(int64_t in_num, int64_t in_den, int64_t out_num, int64_t out_den, RetimeCfg* g) {
    const int st = retime_cfg(in_num, in_den, out_num, out_den, g);
    if (st == RETIME_BAD_RATE) return fail(AVSE_ERR_INVALID, retime_message(st));
    if (st == RETIME_RATIO)
        return fail(AVSE_ERR_UNSUPPORTED, "retiming " + std::to_string(in_num) + "/" + std::to_string(in_den) + " -> " +
                                              std::to_string(out_num) + "/" + std::to_string(out_den) + " fps is the ratio " +
                                              std::to_string(g->p) + " / " + std::to_string(g->q) + ": " + retime_message(st));
    return 0;
}

int retime_shape_checked(int frames_per_slice, int video_dtype, RetimeCfg* g) {
    if (frames_per_slice != 5 && frames_per_slice != 6) return fail(AVSE_ERR_UNSUPPORTED, "frames_per_slice must be 5 or 6");
    if (video_dtype != AVSE_VIDEO_F32 && video_dtype != AVSE_VIDEO_U8) return fail(AVSE_ERR_INVALID, "unknown video dtype");
    g->F = frames_per_slice;
    g->tiles = RETIME_PIXELS / (RETIME_BLOCK * (video_dtype == AVSE_VIDEO_U8 ? 16 : 4));
    return 0;
}

void retime_launch(const RetimeCfg& g, int video_dtype, int64_t blocks, const RetimeArgs& a, const RetimeRow* rows, int n_rows,
                   hipStream_t s) {
    const dim3 grid((unsigned)blocks), block(RETIME_BLOCK);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, s, a, rows, n_rows); };
    const bool u8 = video_dtype == AVSE_VIDEO_U8, wide = a.wide != 0;
    if (u8 && g.F == 5) wide ? go(k_retime<uint8_t, 5, true>) : go(k_retime<uint8_t, 5, false>);
    else if (u8) wide ? go(k_retime<uint8_t, 6, true>) : go(k_retime<uint8_t, 6, false>);
    else if (g.F == 5) wide ? go(k_retime<float, 5, true>) : go(k_retime<float, 5, false>);
    else wide ? go(k_retime<float, 6, true>) : go(k_retime<float, 6, false>);
}

RetimeArgs retime_args(const RetimeCfg& g, const void* frames, char* hist, char* pend, void* out, int B) {
    RetimeArgs a;
    a.frames = (const char*)frames; a.hist = hist; a.hist_w = hist; a.pend = pend; a.pend_w = pend; a.out = (char*)out;
    a.p = g.p; a.q = g.q; a.B = B;
    a.wide = (uintptr_t)frames % 16 == 0 && (uintptr_t)out % 16 == 0;
    return a;
}

}  // namespace
}  // namespace avse

using namespace avse;

struct avse_retimer {
    avse_ctx* ctx = nullptr;
    int64_t B = 0;
    RetimeCfg g;
    int video_dtype = AVSE_VIDEO_F32;
    Owned<char> hist;         // [2][B][128][128]
    Owned<char> pend;         // [2][B][128][128][F]
    std::vector<RetimeState> st;
    std::vector<int64_t> emitted;   // slices handed out
    // the rows of the call being decided, their device copy, and the pinned staging ring they go up from (one slot per
    // call in turn; `staged[i]` is recorded once the copy out of slot i is queued)
    static constexpr int SLOTS = 4;
    std::vector<RetimeRow> rows;
    size_t slot_bytes = 0;
    Owned<char, true> staging;
    Owned<char> tables;
    hipEvent_t staged[SLOTS] = {};
    bool staged_used[SLOTS] = {};
    int slot = 0;
    ~avse_retimer() {
        for (hipEvent_t e : staged)
            if (e) (void)hipEventDestroy(e);
    }
};

extern "C" {

int avse_retime_supported(int64_t in_num, int64_t in_den, int64_t out_num, int64_t out_den) {
    RetimeCfg g;
    return retime_cfg_checked(in_num, in_den, out_num, out_den, &g);
}

int avse_retime_counts(int64_t in_num, int64_t in_den, int64_t out_num, int64_t out_den, int frames_per_slice,
                       int64_t n_frames, int flushed, int64_t* out_frames, int64_t* out_slices) {
    if (!out_frames && !out_slices) return fail(AVSE_ERR_INVALID, "NULL argument");
    RetimeCfg g;
    if (int rc = retime_cfg_checked(in_num, in_den, out_num, out_den, &g)) return rc;
    if (int rc = retime_shape_checked(frames_per_slice, AVSE_VIDEO_F32, &g)) return rc;
    if (n_frames < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    if (n_frames > RETIME_MAX_TOTAL) return fail(AVSE_ERR_INVALID, "counts too large");
    if (out_frames) *out_frames = retime_total(g, n_frames, flushed != 0);
    if (out_slices) *out_slices = retime_slices(g, n_frames, flushed != 0);
    return 0;
}

int avse_retime_ragged(avse_ctx* c, const void* frames, const int64_t* frame_off, const int64_t* n_frames, int64_t n_utt,
                       int video_dtype, int64_t in_num, int64_t in_den, int64_t out_num, int64_t out_den,
                       int frames_per_slice, void* out, int64_t out_slices_cap, int64_t* host_k, void* stream) {
    if (!c || !frame_off || !n_frames || !host_k) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n_utt < 0 || out_slices_cap < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    RetimeCfg g;
    if (int rc = retime_cfg_checked(in_num, in_den, out_num, out_den, &g)) return rc;
    if (int rc = retime_shape_checked(frames_per_slice, video_dtype, &g)) return rc;
    if (n_utt == 0) return 0;
    if (n_utt > (1 << 24)) return fail(AVSE_ERR_INVALID, "batch too large");
    if ((uintptr_t)frames % 4 || (uintptr_t)out % 4) return fail(AVSE_ERR_INVALID, "frames and out must be 4-byte aligned");
    // every utterance a fresh stream that is fed and flushed at once; no history is read or written
    std::vector<RetimeRow> rows((size_t)n_utt);
    int64_t blocks = 0, slices = 0;
    for (int64_t u = 0; u < n_utt; ++u) {
        RetimeRow& r = rows[(size_t)u];
        const int st = retime_row(g, RetimeState{0, 0, 0}, n_frames[u], true, frame_off[u], &r);
        if (st != RETIME_OK) return fail(AVSE_ERR_INVALID, "utterance " + std::to_string(u) + ": " + retime_message(st));
        if (r.k_new > 0 && (!out || out_slices_cap - slices < r.k_new))
            return fail(AVSE_ERR_INVALID, "utterance " + std::to_string(u) + ": " + retime_message(RETIME_OUT_SMALL));
        r.fed = 0;
        r.hist_out = r.hist_in;
        // the launch below has no state (hist and pend are NULL): a fresh, flushed row has only complete slices, none
        // of them with pending frames, so k_retime asks for no frame outside the call's own and touches neither copy
        if (r.n_slots != r.k_new || r.g_old != 0 || r.n_old != 0)
            return fail(AVSE_ERR_INVALID, "utterance " + std::to_string(u) + ": internal: a one-shot row with state");
        r.out_slice = slices;
        r.blk0 = (int32_t)blocks;
        blocks += retime_row_blocks(g, r);
        slices += r.k_new;
        if (blocks > INT32_MAX) return fail(AVSE_ERR_INVALID, "batch too large");
    }
    if (blocks > 0 && !frames) return fail(AVSE_ERR_INVALID, "NULL argument");
    // host_k is written once nothing can fail any more: a call that returns an error leaves it as it was
    auto counts_out = [&] { for (int64_t u = 0; u < n_utt; ++u) host_k[u] = rows[(size_t)u].k_new; };
    if (blocks == 0) {
        counts_out();
        return 0;
    }
    hipStream_t s = (hipStream_t)stream;
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    // the rows: through the pinned copy into the preprocess scratch, as a ragged spectrogram's tables go
    const size_t need = sizeof(RetimeRow) * rows.size();
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (s) AVSE_HIP_CHECK(hipStreamIsCapturing(s, &cs));
    const bool capturing = cs != hipStreamCaptureStatusNone;
    if (int rc = grow(c->prep, need, s, "preprocess scratch")) return rc;
    if (!capturing && c->ragged_done) AVSE_HIP_CHECK(hipEventSynchronize(c->ragged_done));   // the last upload has read it
    if (int rc = grow(c->ragged_host, need, s, "ragged tables")) return rc;
    if (!c->ragged_done) AVSE_HIP_CHECK(hipEventCreateWithFlags(&c->ragged_done, hipEventDisableTiming));
    std::memcpy(c->ragged_host, rows.data(), need);
    AVSE_HIP_CHECK(hipMemcpyAsync(c->prep, c->ragged_host, need, hipMemcpyHostToDevice, s));
    if (!capturing) AVSE_HIP_CHECK(hipEventRecord(c->ragged_done, s));
    retime_launch(g, video_dtype, blocks, retime_args(g, frames, nullptr, nullptr, out, 0),
                  reinterpret_cast<const RetimeRow*>(c->prep.p.get()), (int)n_utt, s);
    AVSE_HIP_CHECK(hipGetLastError());
    counts_out();
    return 0;
}

int avse_retimer_create(avse_ctx* c, int64_t n_streams, int64_t in_num, int64_t in_den, int64_t out_num, int64_t out_den,
                        int frames_per_slice, int video_dtype, avse_retimer** out) {
    if (!c || !out) return fail(AVSE_ERR_INVALID, "NULL argument");
    RetimeCfg g;
    if (int rc = retime_cfg_checked(in_num, in_den, out_num, out_den, &g)) return rc;
    if (int rc = retime_shape_checked(frames_per_slice, video_dtype, &g)) return rc;
    if (n_streams < 1) return fail(AVSE_ERR_INVALID, "n_streams must be positive");
    if (n_streams > 1024) return fail(AVSE_ERR_UNSUPPORTED, "at most 1024 streams");
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    std::unique_ptr<avse_retimer> r(new avse_retimer());
    r->ctx = c; r->B = n_streams; r->g = g; r->video_dtype = video_dtype;
    const size_t B = (size_t)n_streams;
    const size_t frame = (video_dtype == AVSE_VIDEO_U8 ? 1 : 4) * (size_t)RETIME_PIXELS;
    r->st.assign(B, RetimeState{0, 0, 0});
    r->emitted.assign(B, 0);
    r->rows.resize(B);
    r->slot_bytes = (sizeof(RetimeRow) * B + 255) & ~(size_t)255;
    if (r->hist.alloc(2 * B * frame) != hipSuccess || r->pend.alloc(2 * B * frame * g.F) != hipSuccess ||
        r->tables.alloc(r->slot_bytes) != hipSuccess)
        return fail(AVSE_ERR_OOM, "hipMalloc failed (retimer)");
    if (r->staging.alloc(r->slot_bytes * avse_retimer::SLOTS) != hipSuccess)
        return fail(AVSE_ERR_OOM, "hipHostMalloc failed (retimer)");
    for (hipEvent_t& e : r->staged) AVSE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    AVSE_HIP_CHECK(hipMemset(r->hist, 0, r->hist.bytes));
    AVSE_HIP_CHECK(hipMemset(r->pend, 0, r->pend.bytes));
    AVSE_HIP_CHECK(hipStreamSynchronize(nullptr));
    *out = r.release();
    return 0;
}

int avse_retimer_push_each(avse_retimer* r, const void* frames, const int64_t* frame_off, const int64_t* n_new,
                           const uint8_t* flush, void* out, int64_t out_slices_cap, int64_t* host_k_new, void* stream) {
    if (!r || !n_new || !host_k_new) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (out_slices_cap < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    if ((uintptr_t)frames % 4 || (uintptr_t)out % 4) return fail(AVSE_ERR_INVALID, "frames and out must be 4-byte aligned");
    const int B = (int)r->B;
    RetimeRow* rows = r->rows.data();
    const RetimePlan p = retime_rows(r->g, r->st.data(), B, frame_off, n_new, flush, out != nullptr, out_slices_cap, rows);
    if (p.status != RETIME_OK)
        return fail(AVSE_ERR_INVALID, "stream " + std::to_string(p.bad) + ": " + retime_message(p.status));
    if (p.fed > 0 && (!frames || !frame_off)) return fail(AVSE_ERR_INVALID, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    if (p.blocks > 0) {
        if (int rc = not_capturing(s, "a retimer push cannot be captured into a graph")) return rc;
        AVSE_HIP_CHECK(hipSetDevice(r->ctx->device));
        // the next slot of the staging ring, once the copy that last left it has been read: the call's only wait
        const int i = r->slot;
        if (r->staged_used[i]) AVSE_HIP_CHECK(hipEventSynchronize(r->staged[i]));
        char* host = r->staging + (size_t)i * r->slot_bytes;
        const size_t bytes = sizeof(RetimeRow) * (size_t)B;
        std::memcpy(host, rows, bytes);
        AVSE_HIP_CHECK(hipMemcpyAsync(r->tables, host, bytes, hipMemcpyHostToDevice, s));
        AVSE_HIP_CHECK(hipEventRecord(r->staged[i], s));
        r->staged_used[i] = true;
        r->slot = (i + 1) % avse_retimer::SLOTS;
        // a launch that fails ran nothing: the copies the rows' streams read are untouched, and so the state stays
        retime_launch(r->g, r->video_dtype, p.blocks, retime_args(r->g, frames, r->hist, r->pend, out, B),
                      reinterpret_cast<const RetimeRow*>(r->tables.p.get()), B, s);
        AVSE_HIP_CHECK(hipGetLastError());
    }
    for (int b = 0; b < B; ++b) host_k_new[b] = rows[b].k_new;
    retime_commit(rows, B, r->st.data());
    for (int b = 0; b < B; ++b) r->emitted[b] += rows[b].k_new;
    return 0;
}

int avse_retimer_reset_each(avse_retimer* r, const uint8_t* which, void* stream) {
    if (!r) return fail(AVSE_ERR_INVALID, "NULL argument");
    (void)stream;   // host counters only: a stream with n == 0 reads neither copy, and work queued earlier has its rows
    for (int64_t b = 0; b < r->B; ++b)
        if (!which || which[b]) {
            r->st[b].n = 0;
            r->st[b].flushed = 0;   // the parity stays: either copy serves a fresh stream
            r->emitted[b] = 0;
        }
    return 0;
}

int avse_retimer_state(const avse_retimer* r, int64_t* n_in, int64_t* n_slices, uint8_t* flushed) {
    if (!r) return fail(AVSE_ERR_INVALID, "NULL argument");
    for (int64_t b = 0; b < r->B; ++b) {
        if (n_in) n_in[b] = r->st[b].n;
        if (n_slices) n_slices[b] = r->emitted[b];
        if (flushed) flushed[b] = r->st[b].flushed;
    }
    return 0;
}

void avse_retimer_destroy(avse_retimer* r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->device);
    delete r;
}

}  // extern "C"
