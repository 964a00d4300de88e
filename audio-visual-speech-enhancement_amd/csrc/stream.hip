// K17: streaming enhancement.  A session carries B lock-step streams through STFT -> mel-dB -> network -> ISTFT in
// pushes of any size (include/avse.h avse_stream_*): what the offline path (K1 -> forward -> K6) computes for the
// finished utterance, produced as the utterance arrives.
//
// Replaces the per-sample predict path of the reference as it would run incrementally (speech_enhancer.py:70-85;
// preprocess_audio_signal, data_processor.py:35-57; reconstruct_speech_signal, :60-74; signal_to_spectrogram and
// reconstruct_signal_from_spectrogram, :77-116).
//
// State of a session (all on the device, sized at create; the counters that address it live on the host and are
// functions of the call arguments alone, so no call reads anything back):
//   tail        [2][B][640]           the last 640 samples of each stream; the analysis kernel reads one copy and writes
//                                     the other (the copies swap per push: no block reads what another block writes)
//   mel ring    [B][RS][80][spf]      unclamped mel-dB of slice k in slot k % RS; a partial slice simply waits there
//   max ring    [B][R]                each frame's maximum over its 80 bands (plain stores), slot t % R
//   phase ring  [B][R][321] complex   the mixture's STFT of frame t, kept until its slice has been inverted
//   run max     [B]                   maximum of the unclamped mel-dB of every frame of every slice completed so far
//   video queue [B][RV] slices        video that arrived ahead of its samples, slot k % RV
//   frame ring  [B][R][640]           windowed time frames of inverted frames; the last three are the overlap-add tail
// R = spf (2 max_slices + 1), RS = R / spf, RV = 2 max_slices: a push may complete max_slices slices and leave
// max_slices queued (avse_stream_push refuses more), so live entries never share a slot.
//
// Launches of a push (around the forward): k_stream_spec, k_stream_route, [forward], k_stream_synth, k_stream_ola.
//   k_stream_spec   the frames that became computable: the 640-point frame arithmetic of k_spec640 (frame640.h: the same
//                   functions) -> complex frame to the phase ring, unclamped mel-dB to the mel ring, the frame's
//                   maximum to the max ring; one more block per stream writes the new sample tail
//   k_stream_route  the causal top_db clamp of the slices that completed (prefix maximum over run max and the slices'
//                   frame maxima, in slice order: an ordered reduction, no atomics) into the network's input, and the
//                   video slices to where they go (queue or new -> network input; new -> queue).  Two kernels, not
//                   one: a slice's floor needs the maxima of all its frames, which other blocks of k_stream_spec write.
//   k_stream_synth  k_istft640's body (frame640.h synth_frames) on the predicted frames and the ring's phases
//   k_stream_ola    k_ola's sample (frame640.h ola_sample) over the frame ring for the samples that became final
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "ctx.h"
#include "frame640.h"

#ifdef AVSE_NO_WPE   // A/B: no occupancy cap (as stft.hip)
#define AVSE_WPE4
#else
#define AVSE_WPE4 __attribute__((amdgpu_waves_per_eu(4)))
#endif

namespace avse {
namespace {

using namespace spec640;

constexpr int SCHUNK = 21;               // frames per analysis block
constexpr int SWAVES = SCHUNK / FPG;     // 7 waves, 3 frames each
constexpr int TAIL = 640;                // carried samples per stream (n_fft)
constexpr int NMEL = 80;

struct SpecStreamArgs {
    const float* tail_in;     // [B][TAIL]: sample n_old - TAIL + j of each stream
    float* tail_out;          // [B][TAIL]: sample n_new - TAIL + j
    const float* news;        // [B][news_stride]: samples n_old .. n_new - 1
    long long news_stride;
    long long n_old, n_new;   // samples received before / after this call
    long long Lf;             // flush: length of the closed signal (zeros from n_new on, reflected at Lf); else -1
    long long t0;             // frames [t0, t0 + nt) are computed
    int nt, nblk;             // nblk = blocks of SCHUNK frames; block nblk (when launched) writes the tail
    int spf, R, RS;
    const float2* twiddle;
    const float* window;
    const int* mel_start;
    const float* mel_weight;  // [80][MW]
    int nq[4];
    float amin, db_floor;
    float* mel_ring;
    float2* phase_ring;
    float* fmax_ring;
};

// sample i (0 <= i < n_new) of stream b: from this call's samples or from the carried tail
__device__ __forceinline__ float stream_sample(const SpecStreamArgs& a, int b, long long i) {
    if (i >= a.n_old) return a.news[b * a.news_stride + (i - a.n_old)];
    const long long j = i - (a.n_old - TAIL);
    return a.tail_in[b * (long long)TAIL + (j > 0 ? j : 0)];
}
// sample i of the centre-padded signal: x[-i] = x[i]; a flush closes the signal at Lf (zeros from n_new, reflected)
__device__ __forceinline__ float frame_sample(const SpecStreamArgs& a, int b, long long i) {
    if (i < 0) i = -i;
    if (a.Lf >= 0 && i >= a.Lf) i = 2 * (a.Lf - 1) - i;
    if (i >= a.n_new) return 0.f;
    return stream_sample(a, b, i);
}

__global__ __launch_bounds__(64 * SWAVES) AVSE_WPE4 void k_stream_spec(SpecStreamArgs a) {
    __shared__ float2 zbuf[SWAVES * FPG * ZS];
    __shared__ float2 twl[640];
    __shared__ v2f ut2[161];       // U = -i W640^k / 2 (untangling)
    __shared__ float2 winl[320];
    __shared__ float4 melw4[NMEL * MW / 4];
    __shared__ int mel_st[NMEL];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    if ((int)blockIdx.x == a.nblk) {   // the new tail: the last TAIL samples received (zeros before sample 0)
        for (int j = tid; j < TAIL; j += 64 * SWAVES) {
            const long long i = a.n_new - TAIL + j;
            a.tail_out[b * (long long)TAIL + j] = i < 0 ? 0.f : stream_sample(a, b, i);
        }
        return;
    }
    for (int i = tid; i < 640; i += 64 * SWAVES) twl[i] = a.twiddle[i];
    for (int k = tid; k < 161; k += 64 * SWAVES) {
        const float2 w = a.twiddle[k];
        ut2[k] = v2f{0.5f * w.y, -0.5f * w.x};
    }
    for (int i = tid; i < 320; i += 64 * SWAVES) winl[i] = reinterpret_cast<const float2*>(a.window)[i];
    for (int i = tid; i < NMEL * MW / 4; i += 64 * SWAVES) melw4[i] = reinterpret_cast<const float4*>(a.mel_weight)[i];
    for (int i = tid; i < NMEL; i += 64 * SWAVES) mel_st[i] = a.mel_start[i];

    const int g = FPG * wave;                                  // this wave's first frame in the block
    const int nf = min(SCHUNK, a.nt - SCHUNK * (int)blockIdx.x);
    const int ng = max(0, min(FPG, nf - g));
    const long long tw0 = a.t0 + SCHUNK * (long long)blockIdx.x + g;   // the wave's first frame
    const int f1 = lane >> 4, n1 = lane & 15;
    float2 x[20];
#pragma unroll
    for (int n2 = 0; n2 < 20; ++n2) x[n2] = make_float2(0.f, 0.f);
    if (f1 < ng) {
        const long long s0 = (tw0 + f1) * 160 - 320;
        if (s0 >= a.n_old && s0 + 640 <= a.n_new && (a.Lf < 0 || s0 + 640 <= a.Lf)) {   // all in this call's samples
            const float* p = a.news + b * a.news_stride + (s0 - a.n_old) + 2 * n1;
#pragma unroll
            for (int n2 = 0; n2 < 20; ++n2) x[n2] = make_float2(p[32 * n2], p[32 * n2 + 1]);
        } else {
#pragma unroll
            for (int n2 = 0; n2 < 20; ++n2) {
                const long long i = s0 + 2 * (n1 + 16 * n2);
                x[n2] = make_float2(frame_sample(a, b, i), frame_sample(a, b, i + 1));
            }
        }
    }
    __syncthreads();
    float2* zw = zbuf + wave * FPG * ZS;
    // ---- steps 1 and 2: the 16 x 20 split of k_spec640, wave-local (each wave owns its three frames) ----
    v2f v[20];
    window_frame(v, x, winl, n1);
    if (f1 < ng) dft20_store(v, twl, zw + f1 * ZS, n1);
    wave_lds_sync();
    {
        const int f = lane / 20, k2 = lane - 20 * (lane / 20);
        const bool act = f < ng;
        v2f w[16];
        v2f* zf = reinterpret_cast<v2f*>(zw + min(f, FPG - 1) * ZS);
        if (act) dft16_load(w, zf, k2);
        wave_lds_sync();
        if (act) dft16_store(w, zf, k2);
    }
    wave_lds_sync();
    // ---- step 3: untangling -> the complex frame into the phase ring, its magnitudes into LDS; item = (f, k) ----
    {
        constexpr int IT3 = (FPG * 161 + 63) / 64;   // 8
        float mk[IT3], mm[IT3];
#pragma unroll
        for (int j = 0; j < IT3; ++j) {
            const int it = lane + 64 * j;
            if (it >= ng * 161) break;
            const int f = it / 161, k = it - 161 * f;
            v2f X, Y;
            pk_untangle(reinterpret_cast<const v2f*>(zw + f * ZS), k, ut2, X, Y);
            mk[j] = pk_abs(X);
            mm[j] = pk_abs(Y);
            float2* o = a.phase_ring + ((long long)b * a.R + (int)((tw0 + f) % a.R)) * 321;
            o[k] = make_float2(X.x, X.y);
            if (k != 160) o[320 - k] = make_float2(Y.x, -Y.y);   // X[320 - k] = conj(Y)
        }
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < IT3; ++j) {
            const int it = lane + 64 * j;
            if (it >= ng * 161) break;
            const int f = it / 161, k = it - 161 * f;
            float* mf = reinterpret_cast<float*>(zw + f * ZS);
            mf[k] = mk[j];
            mf[320 - k] = mm[j];
        }
        for (int it = lane; it < FPG * MW; it += 64) {   // bins [321, 321 + MW) are read by the padded band dots
            const int f = it / MW, j = it - MW * f;
            reinterpret_cast<float*>(zw + f * ZS)[321 + j] = 0.f;
        }
        wave_lds_sync();
    }
    // ---- step 4: Slaney mel + dB, item = (m, f) as k_spec640; unclamped, into the frame's slice slot ----
    float fm0 = -INFINITY, fm1 = -INFINITY, fm2 = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int it = lane + 64 * jj;
        if (it >= FPG * NMEL) break;
        const int m = __umul24(it, 43691) >> 17, f = it - 3 * m;   // m = it / 3 (it < 240)
        if (f >= ng) continue;
        const float* mf = reinterpret_cast<const float*>(zw + f * ZS) + mel_st[m];
        const float acc = band_dot_nq(melw4 + m * (MW / 4), reinterpret_cast<const v2f*>(mf), a.nq[jj]);
        const float db = mel_to_db(acc, a.amin, a.db_floor);
        const long long t = tw0 + f, sl = t / a.spf;
        a.mel_ring[(((long long)b * a.RS + (int)(sl % a.RS)) * NMEL + m) * a.spf + (int)(t - sl * a.spf)] = db;
        fm0 = f == 0 ? fmaxf(fm0, db) : fm0;
        fm1 = f == 1 ? fmaxf(fm1, db) : fm1;
        fm2 = f == 2 ? fmaxf(fm2, db) : fm2;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        fm0 = fmaxf(fm0, __shfl_xor(fm0, o));
        fm1 = fmaxf(fm1, __shfl_xor(fm1, o));
        fm2 = fmaxf(fm2, __shfl_xor(fm2, o));
    }
    if (lane < ng) a.fmax_ring[(long long)b * a.R + (int)((tw0 + lane) % a.R)] = lane == 0 ? fm0 : lane == 1 ? fm1 : fm2;
}

struct RouteArgs {
    // the causal clamp of slices [k_old, k_old + k_new)
    const float* mel_ring;
    const float* fmax_ring;
    float* run_max;           // [B]
    float* net_in;            // [B][k_new][80][spf]
    float* mel_out;           // nullable: the same values for the caller
    long long k_old;
    int k_new, spf, R, RS;
    float top_db;
    // video slices [k_old, k_old + nv): from the queue (k < v_old) or this call's video, to the network input
    // (k < k_old + k_new) or the queue
    const char* vnew;         // [B][v_new] slices
    char* vq;                 // [B][RV] slices
    char* vstage;             // [B][k_new] slices
    long long vbytes, v_old, v_new;
    int nv, RV, B, vec16;
};
constexpr int ROUTE_X = 8;    // blocks per video slice
constexpr int MAX_SLICES_CAP = 16;   // avse_stream_create's bound on max_slices

// grid: ROUTE_X blocks per (stream, video slice in flight), then one clamp block per stream when slices completed
__global__ __launch_bounds__(256) void k_stream_route(RouteArgs a) {
    __shared__ float slice_max[MAX_SLICES_CAP];
    const int tid = threadIdx.x;
    const int n_video = ROUTE_X * a.B * a.nv;
    if ((int)blockIdx.x < n_video) {
        const int y = blockIdx.x / ROUTE_X, part = blockIdx.x - ROUTE_X * y;
        const int b = y / a.nv;
        const long long k = a.k_old + (y - b * a.nv);
        const bool from_q = k < a.v_old, to_net = k < a.k_old + a.k_new;
        if (from_q && !to_net) return;   // stays queued
        const char* src = from_q ? a.vq + ((long long)b * a.RV + (int)(k % a.RV)) * a.vbytes
                                 : a.vnew + ((long long)b * a.v_new + (k - a.v_old)) * a.vbytes;
        char* dst = to_net ? a.vstage + ((long long)b * a.k_new + (k - a.k_old)) * a.vbytes
                           : a.vq + ((long long)b * a.RV + (int)(k % a.RV)) * a.vbytes;
        if (a.vec16) {
            const long long n = a.vbytes / 16;
            const uint4* s4 = reinterpret_cast<const uint4*>(src);
            uint4* d4 = reinterpret_cast<uint4*>(dst);
            for (long long i = part * 256LL + tid; i < n; i += ROUTE_X * 256LL) d4[i] = s4[i];
        } else {
            const long long n = a.vbytes / 4;
            const unsigned* s1 = reinterpret_cast<const unsigned*>(src);
            unsigned* d1 = reinterpret_cast<unsigned*>(dst);
            for (long long i = part * 256LL + tid; i < n; i += ROUTE_X * 256LL) d1[i] = s1[i];
        }
        return;
    }
    // one block per stream: the floor of slice k is (the maximum over every frame up to its last) - top_db.  Wave w
    // takes the maxima of slices w, w + 4, ..: a lane per frame, then the wave's maximum (a maximum has no order)
    const int b = blockIdx.x - n_video;
    for (int kk = tid >> 6; kk < a.k_new; kk += 4) {
        const long long t0 = (a.k_old + kk) * a.spf;
        float m = -INFINITY;
        for (int tt = tid & 63; tt < a.spf; tt += 64) m = fmaxf(m, a.fmax_ring[(long long)b * a.R + (int)((t0 + tt) % a.R)]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) slice_max[kk] = m;
    }
    float cur = a.run_max[b];
    __syncthreads();   // the slices' maxima are there, and every thread has read the old running maximum
    const int per = NMEL * a.spf;
    for (int kk = 0; kk < a.k_new; ++kk) {   // the prefix maximum, in slice order
        cur = fmaxf(cur, slice_max[kk]);
        const float floor_db = a.top_db >= 0.f ? cur - a.top_db : -INFINITY;
        const float* src = a.mel_ring + ((long long)b * a.RS + (int)((a.k_old + kk) % a.RS)) * per;
        const long long d0 = ((long long)b * a.k_new + kk) * per;
        for (int i = tid; i < per; i += 256) {
            const float v = fmaxf(src[i], floor_db);
            a.net_in[d0 + i] = v;
            if (a.mel_out) a.mel_out[d0 + i] = v;
        }
    }
    if (tid == 0) a.run_max[b] = cur;
}

struct SynthArgs {
    const float2* phase_ring;
    float* frame_ring;
    long long T0;             // first frame inverted by this call
    int nt, R;
};

__global__ __launch_bounds__(64) void k_stream_synth(IstftArgs a, SynthArgs s) {
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * istft640::FPG;
    istft640::synth_frames(
        a, min(istft640::FPG, s.nt - t0),
        [&](int m, int f) {
            const int t = t0 + f, sl = t / a.spf;
            return a.mel_db[(((long long)b * a.n_slices + sl) * a.n_mels + m) * (long long)a.spf + (t - sl * a.spf)];
        },
        [&](int k, int f) { return s.phase_ring[((long long)b * s.R + (int)((s.T0 + t0 + f) % s.R)) * 321 + k]; },
        [&](int f) { return s.frame_ring + ((long long)b * s.R + (int)((s.T0 + t0 + f) % s.R)) * 640; });
}

struct OlaArgs {
    const float* frame_ring;
    const float* window;
    float* out;               // [B][out_stride]
    long long out_stride, e_old, T;   // samples emitted before; frames inverted so far
    int n_out, R;
};

__global__ __launch_bounds__(256) void k_stream_ola(OlaArgs a) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n_out) return;
    const long long p = a.e_old + j + 320;   // position in the untrimmed signal
    a.out[b * a.out_stride + j] = istft640::ola_sample(p, a.T, 640, 160, a.window, [&](long long t, int o) {
        return a.frame_ring[((long long)b * a.R + (int)(t % a.R)) * 640 + o];
    });
}

// the host totals after n samples and v video slices
struct Counts {
    int64_t frames, slices, emitted;
};
Counts stream_totals(int n_fft, int hop, int spf, int64_t n, int64_t v, bool flushed) {
    Counts c;
    if (flushed) {
        c.frames = spf * v;
        c.slices = v;
        c.emitted = v > 0 ? (int64_t)hop * (spf * v - 1) : 0;
        return c;
    }
    c.frames = n < n_fft / 2 + 1 ? 0 : (n - n_fft / 2) / hop + 1;   // frame 0 reads x[n_fft / 2] (left reflection)
    c.slices = std::min(c.frames / spf, v);
    c.emitted = std::max<int64_t>(0, (int64_t)spf * hop * c.slices - n_fft / 2);
    return c;
}

}  // namespace
}  // namespace avse

using namespace avse;

struct avse_stream {
    avse_ctx* ctx = nullptr;
    const avse_weights* w = nullptr;
    int64_t B = 0, max_slices = 0;
    int sr = 0, n_fft = 0, hop = 0, spf = 0, n_mels = 0, vdt = 0, F = 0;
    float amin = 0, top_db = 0, db_floor = 0;
    int R = 0, RS = 0, RV = 0;
    size_t vbytes = 0;
    SpecTables spec;
    IstftTables ist;
    Owned<float> tail, mel_ring, fmax_ring, run_max, net_in, pred, frame_ring;
    Owned<float2> phase_ring;
    Owned<char> vq, vstage;
    // host counters
    int64_t n = 0, v = 0;
    int parity = 0;           // which tail copy holds the last samples
    bool flushed = false, broken = false;
};

namespace {

int stream_init_state(avse_stream* s, hipStream_t st) {
    AVSE_HIP_CHECK(hipMemsetAsync(s->tail, 0, s->tail.bytes, st));
    AVSE_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)s->run_max.p.get(), (int)0xff800000u, (size_t)s->B, st));   // -inf
    s->n = s->v = 0;
    s->parity = 0;
    s->flushed = s->broken = false;
    return 0;
}

// The work of a push (n_new samples, v_new video slices) or of a flush (the remaining frames of the closed signal).
int stream_step(avse_stream* s, bool flush, const float* samples, int64_t n_new, int64_t sample_stride, const void* video,
                int64_t v_new, const float* vmean, const float* vstd, float* out, int64_t out_stride, int64_t* host_n_out,
                float* mel_db, float* pred_db, void* stream) {
    const Counts c0 = stream_totals(s->n_fft, s->hop, s->spf, s->n, s->v, false);
    const int64_t n2 = s->n + n_new, v2 = s->v + v_new;
    const Counts c1 = stream_totals(s->n_fft, s->hop, s->spf, n2, v2, flush);
    const int64_t slice = (int64_t)s->spf * s->hop;
    if (flush && n2 > slice * v2) return fail(AVSE_ERR_INVALID, "flush: more samples than the video slices cover (n > slice * v)");
    const int64_t k_new = c1.slices - c0.slices, n_out = c1.emitted - c0.emitted;
    if (k_new > s->max_slices) return fail(AVSE_ERR_INVALID, "the call would complete more than max_slices slices");
    if (n2 - slice * v2 > slice * s->max_slices)
        return fail(AVSE_ERR_INVALID, "more than max_slices slices of samples queued ahead of the video");
    if (v2 - c1.frames / s->spf > s->max_slices)
        return fail(AVSE_ERR_INVALID, "more than max_slices video slices queued ahead of the samples");
    if (n_out > 0 && (!out || out_stride < n_out)) return fail(AVSE_ERR_INVALID, "out is NULL or out_stride below what the call emits");
    *host_n_out = n_out;
    if (n_new == 0 && v_new == 0 && !flush) return 0;
    hipStream_t st = (hipStream_t)stream;
    AVSE_HIP_CHECK(hipSetDevice(s->ctx->device));
    const int B = (int)s->B;
    // from here on a failure leaves the device state half updated: the session is broken until reset
    auto run = [&]() -> int {
        const int64_t nt = c1.frames - c0.frames;
        if (n_new > 0 || nt > 0) {
            SpecStreamArgs a;
            std::memset(&a, 0, sizeof(a));
            a.tail_in = s->tail + (size_t)s->parity * B * TAIL;
            a.tail_out = s->tail + (size_t)(s->parity ^ 1) * B * TAIL;
            a.news = samples; a.news_stride = sample_stride;
            a.n_old = s->n; a.n_new = n2;
            a.Lf = flush ? slice * v2 : -1;
            a.t0 = c0.frames; a.nt = (int)nt; a.nblk = (int)((nt + SCHUNK - 1) / SCHUNK);
            a.spf = s->spf; a.R = s->R; a.RS = s->RS;
            a.twiddle = s->spec.twiddle; a.window = s->spec.window;
            a.mel_start = s->spec.mel.start; a.mel_weight = s->spec.mel.weight;
            std::memcpy(a.nq, s->spec.mel.seg_nq, sizeof(a.nq));
            a.amin = s->amin; a.db_floor = s->db_floor;
            a.mel_ring = s->mel_ring; a.phase_ring = s->phase_ring; a.fmax_ring = s->fmax_ring;
            const int tail_blk = n_new > 0 ? 1 : 0;
            hipLaunchKernelGGL(k_stream_spec, dim3(a.nblk + tail_blk, B), dim3(64 * SWAVES), 0, st, a);
            AVSE_HIP_CHECK(hipGetLastError());
            if (tail_blk) s->parity ^= 1;
        }
        const int64_t nv = v2 - c0.slices;   // video slices not yet consumed, this call's included
        if (k_new > 0 || v_new > 0) {
            RouteArgs r;
            std::memset(&r, 0, sizeof(r));
            r.mel_ring = s->mel_ring; r.fmax_ring = s->fmax_ring; r.run_max = s->run_max;
            r.net_in = s->net_in; r.mel_out = mel_db;
            r.k_old = c0.slices; r.k_new = (int)k_new; r.spf = s->spf; r.R = s->R; r.RS = s->RS; r.top_db = s->top_db;
            r.vnew = reinterpret_cast<const char*>(video); r.vq = s->vq; r.vstage = s->vstage;
            r.vbytes = (long long)s->vbytes; r.v_old = s->v; r.v_new = v_new;
            r.nv = (int)nv; r.RV = s->RV; r.B = B;
            r.vec16 = (reinterpret_cast<uintptr_t>(video) & 15) == 0;
            hipLaunchKernelGGL(k_stream_route, dim3((unsigned)(ROUTE_X * B * nv + (k_new > 0 ? B : 0))), dim3(256), 0, st, r);
            AVSE_HIP_CHECK(hipGetLastError());
        }
        if (k_new > 0) {
            if (int rc = avse_forward_video(s->ctx, s->w, s->net_in, s->vstage, s->vdt, vmean, vstd, B * k_new, s->pred, stream))
                return rc;
            if (pred_db)
                AVSE_HIP_CHECK(hipMemcpyAsync(pred_db, s->pred, sizeof(float) * (size_t)B * k_new * NMEL * s->spf,
                                              hipMemcpyDeviceToDevice, st));
            IstftArgs ia;
            std::memset(&ia, 0, sizeof(ia));
            ia.mel_db = s->pred; ia.spf = s->spf; ia.n_slices = (int)k_new;
            ia.n_utt = B; ia.T = (int)(k_new * s->spf); ia.nb = 321; ia.N = 640; ia.hop = s->hop; ia.n_mels = s->n_mels;
            ia.pinvT = s->ist.pinvT; ia.twiddle = s->ist.twiddle; ia.window = s->ist.window;
            SynthArgs sa;
            sa.phase_ring = s->phase_ring; sa.frame_ring = s->frame_ring;
            sa.T0 = c0.slices * s->spf; sa.nt = ia.T; sa.R = s->R;
            hipLaunchKernelGGL(k_stream_synth, dim3((ia.T + istft640::FPG - 1) / istft640::FPG, B), dim3(64), 0, st, ia, sa);
            AVSE_HIP_CHECK(hipGetLastError());
        }
        if (n_out > 0) {
            OlaArgs o;
            o.frame_ring = s->frame_ring; o.window = s->ist.window; o.out = out; o.out_stride = out_stride;
            o.e_old = c0.emitted; o.T = c1.slices * s->spf; o.n_out = (int)n_out; o.R = s->R;
            hipLaunchKernelGGL(k_stream_ola, dim3((unsigned)((n_out + 255) / 256), B), dim3(256), 0, st, o);
            AVSE_HIP_CHECK(hipGetLastError());
        }
        return 0;
    };
    if (int rc = run()) {
        s->broken = true;
        return rc;
    }
    s->n = n2;
    s->v = v2;
    if (flush) s->flushed = true;
    return debug_poll(stream);
}

}  // namespace

extern "C" {

int avse_stream_create(avse_ctx* c, const avse_weights* w, int64_t n_streams, int sr, int n_fft, int hop,
                       int frames_per_slice, int n_mels, float fmin, float fmax, float amin, float top_db, int video_dtype,
                       int64_t max_slices, avse_stream** out) {
    if (!c || !w || !out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n_streams < 1 || max_slices < 1 || sr <= 0 || n_fft < 2 || hop <= 0 || frames_per_slice < 1 || n_mels < 1 || !(amin > 0.f))
        return fail(AVSE_ERR_INVALID, "bad stream geometry");
    if (video_dtype != AVSE_VIDEO_F32 && video_dtype != AVSE_VIDEO_U8) return fail(AVSE_ERR_INVALID, "unknown video dtype");
    // a geometry streams when slices do not drift against the samples: n_fft even and four hops long (the slice is
    // then frames_per_slice * hop samples by construction); of those, the 640-point kernels are built
    if (n_fft % 2 || n_fft != 4 * hop)
        return fail(AVSE_ERR_UNSUPPORTED, "streaming needs an even n_fft == 4 * hop (25 fps at 16 kHz: 640 / 160)");
    if (n_fft != 640 || n_mels != NMEL) return fail(AVSE_ERR_UNSUPPORTED, "streaming is built for n_fft 640, hop 160, 80 bands");
    if (n_streams > 1024 || max_slices > MAX_SLICES_CAP)
        return fail(AVSE_ERR_UNSUPPORTED, "at most 1024 streams and max_slices 16");
    if (w->device != c->device) return fail(AVSE_ERR_INVALID, "weights and context are on different devices");
    int wt = 0, wf = 0;
    if (int rc = avse_weights_shape(w, &wt, &wf)) return rc;
    if (wt != frames_per_slice)
        return fail(AVSE_ERR_INVALID, "the weights were loaded for slices of " + std::to_string(wt) + " frames, not " +
                                          std::to_string(frames_per_slice));
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    std::unique_ptr<avse_stream> s(new avse_stream());
    s->ctx = c; s->w = w; s->B = n_streams; s->max_slices = max_slices;
    s->sr = sr; s->n_fft = n_fft; s->hop = hop; s->spf = frames_per_slice; s->n_mels = n_mels; s->vdt = video_dtype; s->F = wf;
    s->amin = amin; s->top_db = top_db;
    s->db_floor = (float)(20.0 * std::log10((double)amin));
    if (int rc = build_spec_tables(s->spec, sr, n_fft, n_mels, fmin, fmax)) return rc;
    if (s->spec.mel.max_width != MW)
        return fail(AVSE_ERR_UNSUPPORTED, "streaming needs a Slaney bank whose bands fit 24 bins (sr 16000, fmin 0, fmax 8000)");
    if (int rc = build_istft_tables(s->ist, sr, n_fft, n_mels, fmin, fmax)) return rc;
    s->RS = 2 * (int)max_slices + 1;
    s->R = s->RS * s->spf;
    s->RV = 2 * (int)max_slices;
    s->vbytes = (size_t)128 * 128 * wf * (video_dtype == AVSE_VIDEO_U8 ? 1 : 4);
    const size_t B = (size_t)n_streams, clips = B * (size_t)max_slices, per = (size_t)NMEL * s->spf;
    if (s->tail.alloc(sizeof(float) * 2 * B * TAIL) != hipSuccess ||
        s->mel_ring.alloc(sizeof(float) * B * s->RS * per) != hipSuccess ||
        s->fmax_ring.alloc(sizeof(float) * B * s->R) != hipSuccess ||
        s->run_max.alloc(sizeof(float) * B) != hipSuccess ||
        s->net_in.alloc(sizeof(float) * clips * per) != hipSuccess ||
        s->pred.alloc(sizeof(float) * clips * per) != hipSuccess ||
        s->frame_ring.alloc(sizeof(float) * B * s->R * 640) != hipSuccess ||
        s->phase_ring.alloc(sizeof(float2) * B * s->R * 321) != hipSuccess ||
        s->vq.alloc(B * s->RV * s->vbytes) != hipSuccess || s->vstage.alloc(clips * s->vbytes) != hipSuccess)
        return fail(AVSE_ERR_OOM, "hipMalloc failed (stream session)");
    // a slot read before its first write holds zeros, never stale memory
    AVSE_HIP_CHECK(hipMemset(s->frame_ring, 0, s->frame_ring.bytes));
    AVSE_HIP_CHECK(hipMemset(s->phase_ring, 0, s->phase_ring.bytes));
    AVSE_HIP_CHECK(hipMemset(s->mel_ring, 0, s->mel_ring.bytes));
    AVSE_HIP_CHECK(hipMemset(s->fmax_ring, 0, s->fmax_ring.bytes));
    if (int rc = avse_ctx_reserve_weights(c, w, (int64_t)clips)) return rc;   // pushes never grow the forward scratch
    if (int rc = stream_init_state(s.get(), nullptr)) return rc;
    AVSE_HIP_CHECK(hipStreamSynchronize(nullptr));
    *out = s.release();
    return 0;
}

int avse_stream_counts(const avse_stream* s, int64_t n_samples, int64_t n_video_slices, int flushed, int64_t* frames,
                       int64_t* slices, int64_t* emitted) {
    if (n_samples < 0 || n_video_slices < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    const int n_fft = s ? s->n_fft : 640, hop = s ? s->hop : 160, spf = s ? s->spf : 20;
    if (flushed && n_samples > (int64_t)spf * hop * n_video_slices)
        return fail(AVSE_ERR_INVALID, "a flush needs n <= slice * v");
    const Counts c = stream_totals(n_fft, hop, spf, n_samples, n_video_slices, flushed != 0);
    if (frames) *frames = c.frames;
    if (slices) *slices = c.slices;
    if (emitted) *emitted = c.emitted;
    return 0;
}

int avse_stream_push(avse_stream* s, const float* samples, int64_t n_new, int64_t sample_stride, const void* video,
                     int64_t v_new, const float* vmean, const float* vstd, float* out, int64_t out_stride,
                     int64_t* host_n_out, float* mel_db, float* pred_db, void* stream) {
    if (!s || !host_n_out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n_new < 0 || v_new < 0 || out_stride < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    if ((n_new > 0 && !samples) || (v_new > 0 && !video)) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n_new > 0 && sample_stride < n_new) return fail(AVSE_ERR_INVALID, "sample_stride below n_new");
    if ((vmean == nullptr) != (vstd == nullptr)) return fail(AVSE_ERR_INVALID, "vnorm_mean and vnorm_std must both be given");
    if (s->broken) return fail(AVSE_ERR_INVALID, "the session is broken by an earlier failure: avse_stream_reset it");
    if (s->flushed) return fail(AVSE_ERR_INVALID, "push after flush: only avse_stream_reset is legal");
    if (v_new > 0 && (reinterpret_cast<uintptr_t>(video) & 3)) return fail(AVSE_ERR_INVALID, "video must be 4-byte aligned");
    if (n_new > (1LL << 40) - s->n || v_new > (1LL << 30) - s->v) return fail(AVSE_ERR_INVALID, "counts too large");
    return stream_step(s, false, samples, n_new, sample_stride, video, v_new, vmean, vstd, out, out_stride, host_n_out, mel_db,
                       pred_db, stream);
}

int avse_stream_flush(avse_stream* s, const float* vmean, const float* vstd, float* out, int64_t out_stride,
                      int64_t* host_n_out, float* mel_db, float* pred_db, void* stream) {
    if (!s || !host_n_out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (out_stride < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    if ((vmean == nullptr) != (vstd == nullptr)) return fail(AVSE_ERR_INVALID, "vnorm_mean and vnorm_std must both be given");
    if (s->broken) return fail(AVSE_ERR_INVALID, "the session is broken by an earlier failure: avse_stream_reset it");
    if (s->flushed) return fail(AVSE_ERR_INVALID, "flush after flush: only avse_stream_reset is legal");
    return stream_step(s, true, nullptr, 0, 0, nullptr, 0, vmean, vstd, out, out_stride, host_n_out, mel_db, pred_db, stream);
}

int avse_stream_reset(avse_stream* s, void* stream) {
    if (!s) return fail(AVSE_ERR_INVALID, "NULL argument");
    AVSE_HIP_CHECK(hipSetDevice(s->ctx->device));
    return stream_init_state(s, (hipStream_t)stream);
}

void avse_stream_destroy(avse_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    delete s;
}

}  // extern "C"
