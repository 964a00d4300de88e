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
//   tail        [2][B][N]             the last N = n_fft samples of each stream (640; 1280 / 1920 at 32 / 48 kHz); the
//                                     analysis kernel reads one copy and writes the other (the copies swap per push:
//                                     no block reads what another block writes)
//   mel ring    [B][RS][80][spf]      unclamped mel-dB of slice k in slot k % RS; a partial slice simply waits there
//   max ring    [B][R]                each frame's maximum over its 80 bands (plain stores), slot t % R
//   phase ring  [B][R][321] complex   the mixture's STFT of frame t, kept until its slice has been inverted
//   run max     [B]                   maximum of the unclamped mel-dB of every frame of every slice completed so far
//   video queue [B][RV] slices        video that arrived ahead of its samples, slot k % RV
//   frame ring  [B][R][N]             windowed time frames of inverted frames; the last three are the overlap-add tail
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
//
// Each launch is one kernel template, k_stream_spec<BASE, P, EACH>, k_stream_route<EACH>, k_stream_synth<BASE, P, EACH>,
// k_stream_ola<BASE, P, EACH> (and k_stream_reset<BASE, P> for avse_stream_reset_each), with its body written once in
// the kernel:
//   EACH  Streams need not move together (avse_stream_push_each): the session keeps its counters per stream,
//         stream_geom.h turns a call's per-stream counts into one row per stream and one item table per kernel (block ->
//         stream, chunk), and the EACH instances take the row's counters in place of the call's scalars (`if constexpr
//         (EACH)` at the top of each kernel; the lock-step instances ignore `rows` and `items`).  The forward runs once
//         on the slices all streams completed.  The lock-step calls run the lock-step instances while every stream's
//         counters are equal.
//   P     n_fft = 640 P: 1 at 16 kHz; at 32 and 48 kHz (P = 2, 3) the analysis and the synthesis compute each frame as P
//         interleaved 640-point frames (frame_poly.h).  N, the hop and N / 2 are compile-time everywhere;
//         k_stream_route and the forward do not depend on P.
//   BASE  the frame arithmetic, n_fft = BASE P: 640 (frame640.h, frame_poly.h: 25-fps video at 16 / 32 / 48 kHz, P = 1,
//         2, 3) or 800 (frame800.h: 30-fps video at 24 / 48 kHz, P = 1, 2; bins 0 .. 266 of a 20 x 20 split).  The
//         rings, the mel tables, k_stream_route, the forward and the host geometry do not depend on it.
// A kernel template, not a function taking the argument struct: the by-value kernel argument never leaves the kernel,
// so each of its fields is still loaded where it is used ("Independent streams").
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>

#include "ctx.h"
#include "frame640.h"
#include "frame800.h"
#include "frame_poly.h"
#include "spec_tables.h"
#include "slide_geom.h"
#include "stream_geom.h"

#ifdef AVSE_NO_WPE   // A/B: no occupancy cap (as stft.hip)
#define AVSE_SPEC_WPE(BASE, P)
#else   // the 16 kHz analysis is capped at 4 waves per SIMD's registers; the P-phase and the 800-point instances are not
        // (1: no cap)
#define AVSE_SPEC_WPE(BASE, P) __attribute__((amdgpu_waves_per_eu((BASE) == 640 && (P) == 1 ? 4 : 1)))
#endif

namespace avse {
namespace {

using namespace spec640;

constexpr int SCHUNK = 21;               // frames per analysis block
constexpr int SWAVES = SCHUNK / FPG;     // 7 waves, 3 frames each
constexpr int NMEL = 80;

struct SpecStreamArgs {
    const float* tail_in;     // [B][N]: sample n_old - N + j of each stream
    float* tail_out;          // [B][N]: sample n_new - N + j
    const float* news;        // [B][news_stride]: samples n_old .. n_new - 1
    long long news_stride;
    long long n_old, n_new;   // samples received before / after this call
    long long Lf;             // flush: length of the closed signal (zeros from n_new on, reflected at Lf); else -1
    long long t0;             // frames [t0, t0 + nt) are computed
    int nt, nblk;             // nblk = blocks of SCHUNK frames; block nblk (when launched) writes the tail
    int spf, R, RS;
    const float2* twiddle;    // W_N^k [N]
    const float* window;      // [N]
    const int* mel_start;
    const float* mel_weight;  // [80][MW]
    int nq[4];
    float amin, db_floor;
    float* mel_ring;
    float2* phase_ring;
    float* fmax_ring;
};

// sample i (0 <= i < n_new) of stream b: from this call's samples or from the carried tail of N samples
template <int N>
__device__ __forceinline__ float stream_sample(const SpecStreamArgs& a, int b, long long i) {
    if (i >= a.n_old) return a.news[b * a.news_stride + (i - a.n_old)];
    const long long j = i - (a.n_old - N);
    return a.tail_in[b * (long long)N + (j > 0 ? j : 0)];
}
// sample i of the centre-padded signal: x[-i] = x[i]; a flush closes the signal at Lf (zeros from n_new, reflected)
template <int N>
__device__ __forceinline__ float frame_sample(const SpecStreamArgs& a, int b, long long i) {
    if (i < 0) i = -i;
    if (a.Lf >= 0 && i >= a.Lf) i = 2 * (a.Lf - 1) - i;
    if (i >= a.n_new) return 0.f;
    return stream_sample<N>(a, b, i);
}

// One analysis block: chunk blk of SCHUNK frames of stream b, or (blk == a.nblk) the stream's new tail.  Lock-step:
// grid [blocks, B].  EACH (avse_stream_push_each): block -> item -> (stream, chunk) -> its row (stream_geom.h),
// all wave-uniform; the row's counters take the place of the lock-step call's scalars in `a`; on entry a.tail_in /
// tail_out are tail copies 0 / 1 and a.news the caller's `samples` (row stride 0: the row's sample_off addresses the
// stream).
// P == 1 is the packed real FFT of k_spec640.  P > 1 (32 / 48 kHz, frame_poly.h): a.twiddle is W_N^k and a.window the
// Hann window, both [N], and a frame starts at sample P (160 t - 320); the phases run one after another through the
// wave's three LDS frame slots (LDS is the P == 1 size plus the P - 1 further window phases), X[k] and X[320 - k] of
// the lane's step-3 items accumulate in registers, and the magnitudes follow the last phase.  The rings, the mel tables
// and everything after step 3 are the same (the band-limited bins 0 .. 320 are the same 25-Hz bins).
//
// BASE == 800 (30-fps video, frame800.h): N = 800 P, a frame starts at sample P (200 t - 400), lanes (frame, n1 < 20) run
// the 20 x 20 split (lanes 60 .. 63 idle in steps 1 and 2), step 3 takes the pairs (k, 400 - k), k <= 200, into the
// accumulators for P = 1 too, and only bins 0 .. 266 (the 30-Hz bins under 8 kHz) reach the phase ring and the mel step.
template <int BASE, int P, bool EACH>
__global__ __launch_bounds__(64 * SWAVES) AVSE_SPEC_WPE(BASE, P) void k_stream_spec(SpecStreamArgs a, const StreamRow* __restrict__ rows,
                                                                                    const StreamItem* __restrict__ items) {
    static_assert(BASE == 640 || BASE == 800, "the frame arithmetic of frame640.h or frame800.h");
    constexpr int N = BASE * P;
    constexpr int ZS = BASE == 640 ? spec640::ZS : spec800::ZS;      // LDS slot of a frame
    constexpr int KPAD = BASE == 640 ? 321 : spec800::KTOP + 1;      // first bin past the band-limited spectrum
    int b;
    unsigned blk;
    if constexpr (EACH) {
        const StreamItem it = items[blockIdx.x];
        const StreamRow& r = rows[it.b];
        const float* t0 = a.tail_in;
        float* t1 = a.tail_out;
        a.tail_in = r.tail_in ? t1 : t0;
        a.tail_out = r.tail_in ? const_cast<float*>(t0) : t1;   // the other copy (written only when the stream was fed)
        a.news += r.sample_off;
        a.n_old = r.n_old; a.n_new = r.n_new;
        a.Lf = r.Lf;
        a.t0 = r.t0; a.nt = r.nt; a.nblk = r.nblk;
        b = it.b;
        blk = it.chunk;
    } else {
        b = blockIdx.y;
        blk = blockIdx.x;
    }
    __shared__ float2 zbuf[SWAVES * FPG * ZS];
    __shared__ float2 twl[BASE];       // W640^k = W_N^{P k} (W800^k)
    __shared__ v2f ut2[BASE / 4 + 1];  // U = -i W640^k / 2 (untangling)
    __shared__ float2 winl[P * (BASE / 2)];   // phase r of the window as the pairs window_frame reads
    __shared__ float4 melw4[NMEL * MW / 4];
    __shared__ int mel_st[NMEL];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blk == a.nblk) {   // the new tail: the last N samples received (zeros before sample 0)
        for (int j = tid; j < N; j += 64 * SWAVES) {
            const long long i = a.n_new - N + j;
            a.tail_out[b * (long long)N + j] = i < 0 ? 0.f : stream_sample<N>(a, b, i);
        }
        return;
    }
    for (int i = tid; i < BASE; i += 64 * SWAVES) twl[i] = a.twiddle[P * i];
    for (int k = tid; k < BASE / 4 + 1; k += 64 * SWAVES) {
        const float2 w = a.twiddle[P * k];
        ut2[k] = v2f{0.5f * w.y, -0.5f * w.x};
    }
    for (int i = tid; i < P * (BASE / 2); i += 64 * SWAVES) {
        if constexpr (P == 1) winl[i] = reinterpret_cast<const float2*>(a.window)[i];
        else winl[i] = spec_poly::window_pair<P>(a.window, i / (BASE / 2), i % (BASE / 2));
    }
    for (int i = tid; i < NMEL * MW / 4; i += 64 * SWAVES) melw4[i] = reinterpret_cast<const float4*>(a.mel_weight)[i];
    for (int i = tid; i < NMEL; i += 64 * SWAVES) mel_st[i] = a.mel_start[i];
    if constexpr (P != 1 || BASE != 640) __syncthreads();   // (the 16 kHz instance loads its samples first)

    const int g = FPG * wave;                                  // this wave's first frame in the block
    const int nf = min(SCHUNK, a.nt - SCHUNK * (int)blk);
    const int ng = max(0, min(FPG, nf - g));
    const long long tw0 = a.t0 + SCHUNK * (long long)blk + g;   // the wave's first frame
    const int f1 = lane >> 4, n1 = lane & 15;
    float2* zw;
    // ---- steps 1 to 3: the complex frame into the phase ring, its magnitudes into LDS ----
    if constexpr (BASE == 800) {
        const int f8 = lane / 20, n8 = lane - 20 * (lane / 20);   // (frame, n1) in step 1, (frame, k2) in step 2
        const bool act = f8 < ng;                                   // (lanes 60 .. 63: f8 == 3 == FPG, never active)
        const long long s0 = ((tw0 + f8) * 200 - 400) * P;
        const bool whole = s0 >= a.n_old && s0 + N <= a.n_new && (a.Lf < 0 || s0 + N <= a.Lf);   // all in this call's samples
        zw = zbuf + wave * FPG * ZS;
        v2f ax[spec800::IT3], ay[spec800::IT3];
#pragma unroll
        for (int r = 0; r < P; ++r) {
            float2 x[20];
#pragma unroll
            for (int n2 = 0; n2 < 20; ++n2) x[n2] = make_float2(0.f, 0.f);
            if (act) {
                if (whole)
                    spec800::load_phase<P>(x, a.news + b * a.news_stride + (s0 - a.n_old), n8, r);
                else
                    spec800::load_phase<P>(x, [&](long long i) { return frame_sample<N>(a, b, i); }, s0, n8, r);
            }
            // steps 1 and 2 of the 20 x 20 split on the phase's 800 samples, wave-local
            v2f v[20];
            spec800::window_frame(v, x, winl + r * 400, n8);
            if (act) spec800::dft20_store(v, twl, zw + f8 * ZS, n8);
            wave_lds_sync();
            {
                v2f* zf = reinterpret_cast<v2f*>(zw + min(f8, FPG - 1) * ZS);
                if (act) spec800::row_load(v, zf, n8);
                wave_lds_sync();
                if (act) spec800::row_store(v, zf, n8);
            }
            wave_lds_sync();
            // step 3 of the phase: W_N^{r k} F_r[k] into the accumulators
            spec800::accumulate<P>(ax, ay, zw, ut2, a.twiddle, r, ng, lane);
            wave_lds_sync();   // the next phase (or the magnitudes below) overwrites the slots
        }
#pragma unroll
        for (int j = 0; j < spec800::IT3; ++j) {   // item = (f, k <= 200): bins k and 400 - k, the latter up to bin 266
            const int it = lane + 64 * j;
            if (it >= ng * 201) break;
            const int f = it / 201, k = it - 201 * f;
            float2* o = a.phase_ring + ((long long)b * a.R + (int)((tw0 + f) % a.R)) * 321;
            float* mf = reinterpret_cast<float*>(zw + f * ZS);
            o[k] = make_float2(ax[j].x, ax[j].y);
            mf[k] = pk_abs(ax[j]);
            if (k != 200 && 400 - k < KPAD) {
                o[400 - k] = make_float2(ay[j].x, ay[j].y);
                mf[400 - k] = pk_abs(ay[j]);
            }
        }
    } else if constexpr (P == 1) {
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
                    x[n2] = make_float2(frame_sample<N>(a, b, i), frame_sample<N>(a, b, i + 1));
                }
            }
        }
        __syncthreads();
        zw = zbuf + wave * FPG * ZS;
        // steps 1 and 2: the 16 x 20 split of k_spec640, wave-local (each wave owns its three frames)
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
        // step 3: untangling; item = (f, k)
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
    } else {
        const long long s0 = ((tw0 + f1) * 160 - 320) * P;
        const bool whole = s0 >= a.n_old && s0 + N <= a.n_new && (a.Lf < 0 || s0 + N <= a.Lf);   // all in this call's samples
        zw = zbuf + wave * FPG * ZS;
        v2f ax[spec_poly::IT3], ay[spec_poly::IT3];
#pragma unroll
        for (int r = 0; r < P; ++r) {
            float2 x[20];
#pragma unroll
            for (int n2 = 0; n2 < 20; ++n2) x[n2] = make_float2(0.f, 0.f);
            if (f1 < ng) {
                if (whole)
                    spec_poly::load_phase<P>(x, a.news + b * a.news_stride + (s0 - a.n_old), n1, r);
                else
                    spec_poly::load_phase<P>(x, [&](long long i) { return frame_sample<N>(a, b, i); }, s0, n1, r);
            }
            // steps 1 and 2 of the 16 x 20 split on the phase's 640 samples, wave-local
            v2f v[20];
            window_frame(v, x, winl + r * 320, n1);
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
            // step 3 of the phase: W_N^{r k} F_r[k] into the accumulators
            spec_poly::accumulate<P>(ax, ay, zw, ut2, a.twiddle, r, ng, lane);
            wave_lds_sync();   // the next phase (or the magnitudes below) overwrites the slots
        }
#pragma unroll
        for (int j = 0; j < spec_poly::IT3; ++j) {   // item = (f, k)
            const int it = lane + 64 * j;
            if (it >= ng * 161) break;
            const int f = it / 161, k = it - 161 * f;
            float2* o = a.phase_ring + ((long long)b * a.R + (int)((tw0 + f) % a.R)) * 321;
            o[k] = make_float2(ax[j].x, ax[j].y);
            if (k != 160) o[320 - k] = make_float2(ay[j].x, ay[j].y);
            float* mf = reinterpret_cast<float*>(zw + f * ZS);
            mf[k] = pk_abs(ax[j]);
            mf[320 - k] = pk_abs(ay[j]);
        }
    }
    for (int it = lane; it < FPG * MW; it += 64) {   // bins [321, 321 + MW) are read by the padded band dots
        const int f = it / MW, j = it - MW * f;
        reinterpret_cast<float*>(zw + f * ZS)[KPAD + j] = 0.f;
    }
    wave_lds_sync();
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

// part `part` of ROUTE_X of one video slice's copy (scalars, not RouteArgs: see the header)
__device__ __forceinline__ void route_copy(const char* src, char* dst, long long vbytes, int vec16, int part, int tid) {
    if (vec16) {
        const long long n = vbytes / 16;
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (long long i = part * 256LL + tid; i < n; i += ROUTE_X * 256LL) d4[i] = s4[i];
    } else {
        const long long n = vbytes / 4;
        const unsigned* s1 = reinterpret_cast<const unsigned*>(src);
        unsigned* d1 = reinterpret_cast<unsigned*>(dst);
        for (long long i = part * 256LL + tid; i < n; i += ROUTE_X * 256LL) d1[i] = s1[i];
    }
}

// Lock-step grid: ROUTE_X blocks per (stream, video slice in flight), then one clamp block per stream when slices
// completed.  EACH: an item is part chunk % ROUTE_X of the move of the stream's slice k_old + chunk / ROUTE_X (only
// slices that move are listed), or (chunk == STREAM_CLAMP) its clamp block; a.vnew is the packed video of the call, and
// the network input, mel_out and vstage are compacted: the stream's slices are clips clip0 .. clip0 + k_new - 1.
template <bool EACH>
__global__ __launch_bounds__(256) void k_stream_route(RouteArgs a, const StreamRow* __restrict__ rows,
                                                      const StreamItem* __restrict__ items) {
    __shared__ float slice_max[MAX_SLICES_CAP];
    const int tid = threadIdx.x;
    // The block's item, row and (lock-step) video block count stand here, at function scope, with a dummy for the form
    // that has none, and not inside the `if constexpr` braces below: a brace scope that declares locals, returns early
    // and is also left normally compiles to a cleanup switch, and with it to another control flow than these kernels
    // had as two functions (2,291 instruction lines of the lock-step instance moved).
    const StreamItem it = EACH ? items[blockIdx.x] : StreamItem{0, 0};
    const StreamRow* r = EACH ? rows + it.b : nullptr;
    const int n_video = EACH ? 0 : ROUTE_X * a.B * a.nv;   // lock-step: the grid's video blocks come first
    if constexpr (EACH) {
        if (it.chunk != STREAM_CLAMP) {
            const int b = it.b;
            const int kk = it.chunk / ROUTE_X, part = it.chunk - ROUTE_X * kk;
            const long long k = r->k_old + kk;
            const bool from_q = k < r->v_old, to_net = kk < r->k_new;
            const char* src = from_q ? a.vq + ((long long)b * a.RV + (int)(k % a.RV)) * a.vbytes
                                     : a.vnew + (r->video_off + (k - r->v_old)) * a.vbytes;
            char* dst = to_net ? a.vstage + ((long long)r->clip0 + kk) * a.vbytes
                               : a.vq + ((long long)b * a.RV + (int)(k % a.RV)) * a.vbytes;
            route_copy(src, dst, a.vbytes, a.vec16, part, tid);
            return;
        }
    } else {
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
            route_copy(src, dst, a.vbytes, a.vec16, part, tid);
            return;
        }
    }
    // the clamp block of stream b: its slices [k_old, k_old + k_new) are clips clip0 .. of the network's input, each
    // of the three read where it is used (the row's fields are reloaded there, as the call's scalars are; copies made
    // here, or accessor lambdas capturing `a`, compile to other code)
    const int b = EACH ? it.b : blockIdx.x - n_video;
    // the floor of slice k is (the maximum over every frame up to its last) - top_db.  Wave w takes the maxima of
    // slices w, w + 4, ..: a lane per frame, then the wave's maximum (a maximum has no order)
    for (int kk = tid >> 6; kk < (EACH ? r->k_new : a.k_new); kk += 4) {
        const long long t0 = ((EACH ? r->k_old : a.k_old) + kk) * a.spf;
        float m = -INFINITY;
        for (int tt = tid & 63; tt < a.spf; tt += 64) m = fmaxf(m, a.fmax_ring[(long long)b * a.R + (int)((t0 + tt) % a.R)]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) slice_max[kk] = m;
    }
    float cur = a.run_max[b];
    __syncthreads();   // the slices' maxima are there, and every thread has read the old running maximum
    const int per = NMEL * a.spf;
    for (int kk = 0; kk < (EACH ? r->k_new : a.k_new); ++kk) {   // the prefix maximum, in slice order
        cur = fmaxf(cur, slice_max[kk]);
        const float floor_db = a.top_db >= 0.f ? cur - a.top_db : -INFINITY;
        const float* src = a.mel_ring + ((long long)b * a.RS + (int)(((EACH ? r->k_old : a.k_old) + kk) % a.RS)) * per;
        const long long d0 = ((EACH ? r->clip0 : (long long)b * a.k_new) + kk) * per;
        for (int i = tid; i < per; i += 256) {
            const float v = fmaxf(src[i], floor_db);
            a.net_in[d0 + i] = v;
            if (a.mel_out) a.mel_out[d0 + i] = v;
        }
    }
    if (tid == 0) a.run_max[b] = cur;
}

// One video slice's move in a call with slices that have no video (avse_stream_push_each_mixed): from the call's packed
// video (src_q 0: slice src of it) or the queue (src_q 1: slot src of [B][RV]) to the compacted network input (dst_q 0:
// clip dst of the clips with video) or the queue (dst_q 1).  The host lists only slices that have video and move.
struct StreamMove {
    int32_t src_q, src, dst_q, dst;
};
static_assert(sizeof(StreamMove) == 2 * sizeof(StreamItem), "a move takes two item slots of the route table");

// ROUTE_X blocks per listed move
__global__ __launch_bounds__(256) void k_stream_move(const char* __restrict__ vnew, char* vq, char* vstage, long long vbytes,
                                                     int vec16, const StreamMove* __restrict__ moves) {
    const StreamMove m = moves[blockIdx.x / ROUTE_X];
    const int part = blockIdx.x % ROUTE_X;
    const char* src = (m.src_q ? (const char*)vq : vnew) + (long long)m.src * vbytes;
    char* dst = (m.dst_q ? vq : vstage) + (long long)m.dst * vbytes;
    route_copy(src, dst, vbytes, vec16, part, threadIdx.x);
}

struct SynthArgs {
    const float2* phase_ring;
    float* frame_ring;
    long long T0;             // first frame inverted by this call
    int nt, R;
};

// One group of FPG frames from t0 of stream b's s.nt predicted frames, into the frame ring's slots of 640 P samples;
// clip(sl) is the clip of a.mel_db that holds the stream's slice sl of this call.  (Its callers are distinct instances,
// Clip being a lambda type: one LDS allocation of synth_frames per kernel.)  P > 1: a.N = 640 P, frame_poly.h.
// BASE == 800: a.N = 800 P, frame800.h (P = 1 and 2 alike); the ring's rows stay 321 wide, bins 0 .. 266 are read.
template <int BASE, int P, class Clip>
__device__ __forceinline__ void synth_group(const IstftArgs& a, const SynthArgs& s, const int b, const int t0, Clip clip) {
    const int ng = min(istft640::FPG, s.nt - t0);
    auto mel_db = [&](int m, int f) {
        const int t = t0 + f, sl = t / a.spf;
        return a.mel_db[(clip(sl) * a.n_mels + m) * (long long)a.spf + (t - sl * a.spf)];
    };
    auto stft = [&](int k, int f) { return s.phase_ring[((long long)b * s.R + (int)((s.T0 + t0 + f) % s.R)) * 321 + k]; };
    auto frame = [&](int f) { return s.frame_ring + ((long long)b * s.R + (int)((s.T0 + t0 + f) % s.R)) * (BASE * P); };
    if constexpr (BASE == 800) istft800::synth_frames<P>(a, ng, mel_db, stft, frame);
    else if constexpr (P == 1) istft640::synth_frames(a, ng, mel_db, stft, frame);
    else istft_poly::synth_frames<P>(a, ng, mel_db, stft, frame);
}

// Lock-step: grid [groups, B].  EACH: item (stream, group); the stream inverts its k_new slices from frame spf k_old on.
template <int BASE, int P, bool EACH>
__global__ __launch_bounds__(64) void k_stream_synth(IstftArgs a, SynthArgs s, const StreamRow* __restrict__ rows,
                                                     const StreamItem* __restrict__ items) {
    if constexpr (EACH) {
        const StreamItem it = items[blockIdx.x];
        const StreamRow& r = rows[it.b];
        s.T0 = r.k_old * a.spf;
        s.nt = r.k_new * a.spf;
        synth_group<BASE, P>(a, s, it.b, it.chunk * istft640::FPG, [&](int sl) { return (long long)r.clip0 + sl; });
    } else {
        const int b = blockIdx.y;
        const int t0 = blockIdx.x * istft640::FPG;
        synth_group<BASE, P>(a, s, b, t0, [&](int sl) { return (long long)b * a.n_slices + sl; });
    }
}

struct OlaArgs {
    const float* frame_ring;
    const float* window;
    float* out;               // [B][out_stride]
    long long out_stride, e_old, T;   // samples emitted before; frames inverted so far
    int n_out, R;
};

// Output sample j of this call of each stream.  Lock-step: grid [blocks of 256 samples, B].  EACH: item (stream, block).
template <int BASE, int P, bool EACH>
__global__ __launch_bounds__(256) void k_stream_ola(OlaArgs a, const StreamRow* __restrict__ rows,
                                                    const StreamItem* __restrict__ items) {
    constexpr int N = BASE * P, hop = BASE / 4 * P;
    int b, j;
    if constexpr (EACH) {
        const StreamItem it = items[blockIdx.x];
        const StreamRow& r = rows[it.b];
        a.e_old = r.e_old; a.T = r.T; a.n_out = r.n_out;
        b = it.b;
        j = it.chunk * STREAM_OLA_BLOCK + threadIdx.x;
    } else {
        b = blockIdx.y;
        j = blockIdx.x * 256 + threadIdx.x;
    }
    if (j >= a.n_out) return;
    const long long p = a.e_old + j + N / 2;   // position in the untrimmed signal
    a.out[b * a.out_stride + j] = istft640::ola_sample(p, a.T, N, hop, a.window, [&](long long t, int o) {
        return a.frame_ring[((long long)b * a.R + (int)(t % a.R)) * N + o];
    });
}

// The streams ids[0 .. gridDim.x) go back to the state after create: both tail copies zero, running maximum -inf.
template <int BASE, int P>
__global__ __launch_bounds__(256) void k_stream_reset(float* tail, float* run_max, const int* __restrict__ ids, int B) {
    constexpr int N = BASE * P;
    const int b = ids[blockIdx.x];
    for (int j = threadIdx.x; j < 2 * N; j += 256) {
        const int copy = j / N;
        tail[((long long)copy * B + b) * N + (j - copy * N)] = 0.f;
    }
    if (threadIdx.x == 0) run_max[b] = -INFINITY;
}

// ---- K21: the sliding session (avse_slide_*, slide_geom.h).  Network windows start at every `stride`-th video frame;
// the analysis and the overlap-add are k_stream_spec<BASE, P, true> and k_stream_ola<BASE, P, true> on rows that
// slide_geom.h fills, the three kernels below take the place of k_stream_route and k_stream_synth. ----
struct SlideRouteArgs {
    const float* mel_ring;    // [B][RS][80][spf], slice-slotted as k_stream_spec fills it
    const float* fmax_ring;   // [B][R]
    float* run_max;           // [B]: maximum over every frame up to the last window's last
    float* net_in;            // [clips][80][spf]
    float* mel_out;           // nullable: the same values for the caller
    int spf, qs, R, RS;
    float top_db;
};

// The clamp block of one stream (item.b): windows [w_old, w_old + w_new) become clips clip0 .. of the network's input.
// Window j reads frames [qs j, qs j + spf), up to two slots of the mel ring, and adds frames [qs j + spf - qs,
// qs j + spf) (window 0: all spf) to the running maximum: the prefix maximum in window order, no atomics.
__global__ __launch_bounds__(256) void k_slide_route(SlideRouteArgs a, const SlideRow* __restrict__ rows,
                                                     const StreamItem* __restrict__ items) {
    __shared__ float win_max[SLIDE_MAX_WINDOWS];
    const int tid = threadIdx.x;
    const int b = items[blockIdx.x].b;
    const SlideRow& r = rows[b];
    for (int kk = tid >> 6; kk < r.w_new; kk += 4) {
        const long long j = r.w_old + kk;
        const long long t_hi = (long long)a.qs * j + a.spf, t_lo = j == 0 ? 0 : t_hi - a.qs;
        float m = -INFINITY;
        for (long long t = t_lo + (tid & 63); t < t_hi; t += 64) m = fmaxf(m, a.fmax_ring[(long long)b * a.R + (int)(t % a.R)]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) win_max[kk] = m;
    }
    float cur = a.run_max[b];
    __syncthreads();   // the windows' maxima are there, and every thread has read the old running maximum
    const int per = NMEL * a.spf;
    for (int kk = 0; kk < r.w_new; ++kk) {
        cur = fmaxf(cur, win_max[kk]);
        const float floor_db = a.top_db >= 0.f ? cur - a.top_db : -INFINITY;
        const long long t0 = (long long)a.qs * (r.w_old + kk);
        const long long d0 = ((long long)r.clip0 + kk) * per;
        for (int i = tid; i < per; i += 256) {
            const int m = i / a.spf, c = i - m * a.spf;
            const long long t = t0 + c, sl = t / a.spf;
            const float x = a.mel_ring[(((long long)b * a.RS + (int)(sl % a.RS)) * NMEL + m) * a.spf + (int)(t - sl * a.spf)];
            const float v = fmaxf(x, floor_db);
            a.net_in[d0 + i] = v;
            if (a.mel_out) a.mel_out[d0 + i] = v;
        }
    }
    if (tid == 0) a.run_max[b] = cur;
}

struct SlideGatherArgs {
    const char* vnew;         // the call's packed video: [sum f_new] frames of [128][128]
    char* vring;              // [B][RVf] frames, frame f of a stream in slot f % RVf
    char* vstage;             // [clips][128][128][F]
    int stride, RVf, vec16;   // vec16: vnew is 16-byte aligned
};

// 16 bytes of a frame: from the ring (aligned), or from the caller's buffer as four dwords when that is only 4-byte
// aligned
__device__ __forceinline__ uint4 load16(const char* p, bool aligned) {
    if (aligned) return *reinterpret_cast<const uint4*>(p);
    const unsigned* q = reinterpret_cast<const unsigned*>(p);
    return make_uint4(q[0], q[1], q[2], q[3]);
}

// The video of a call.  A window item (chunk >= 0) is part chunk % SLIDE_GATHER_X of the transpose of window
// w_old + chunk / SLIDE_GATHER_X: its F frames [128][128], each from the ring (received in an earlier call) or from
// the call's buffer, into the clip's [128][128][F].  A thread takes 16 bytes of consecutive pixels from each frame
// (coalesced rows) and writes the F 16-byte vectors that hold those pixels' F values.  An append item (chunk < 0)
// copies frame app0 + (-1 - chunk) of the call into its ring slot; the windows of this call never read that slot (they
// take the frame from the call's buffer), and it shares no slot with a frame they do read (slide_geom.h, RVf).
template <class T, int F>
__global__ __launch_bounds__(256) void k_slide_gather(SlideGatherArgs a, const SlideRow* __restrict__ rows,
                                                      const StreamItem* __restrict__ items) {
    constexpr int G = 16 / (int)sizeof(T);              // pixels per 16-byte vector
    constexpr long long FB = 128 * 128 * sizeof(T);      // bytes of a frame
    constexpr int NG = 128 * 128 / G;                    // vectors per frame
    const StreamItem it = items[blockIdx.x];
    const SlideRow& r = rows[it.b];
    const int tid = threadIdx.x;
    if (it.chunk < 0) {
        const long long fr = r.app0 + (-1 - it.chunk);
        const char* src = a.vnew + (r.video_off + (fr - r.f_old)) * FB;
        char* dst = a.vring + ((long long)it.b * a.RVf + (int)(fr % a.RVf)) * FB;
        for (int g = tid; g < NG; g += 256) reinterpret_cast<uint4*>(dst)[g] = load16(src + 16LL * g, a.vec16 != 0);
        return;
    }
    const int kk = it.chunk / SLIDE_GATHER_X, part = it.chunk - SLIDE_GATHER_X * kk;
    const char* src[F];
    bool aligned[F];
#pragma unroll
    for (int i = 0; i < F; ++i) {
        const long long fr = (long long)a.stride * (r.w_old + kk) + i;
        const bool ring = fr < r.f_old;
        src[i] = ring ? a.vring + ((long long)it.b * a.RVf + (int)(fr % a.RVf)) * FB
                      : a.vnew + (r.video_off + (fr - r.f_old)) * FB;
        aligned[i] = ring || a.vec16 != 0;
    }
    uint4* dst = reinterpret_cast<uint4*>(a.vstage + ((long long)r.clip0 + kk) * (F * FB));
    for (int g = part * (NG / SLIDE_GATHER_X) + tid; g < (part + 1) * (NG / SLIDE_GATHER_X); g += 256) {
        union { uint4 v; T e[G]; } in[F];
        union { uint4 v[F]; T e[G * F]; } o;
#pragma unroll
        for (int i = 0; i < F; ++i) in[i].v = load16(src[i] + 16LL * g, aligned[i]);
#pragma unroll
        for (int p = 0; p < G; ++p)
#pragma unroll
            for (int i = 0; i < F; ++i) o.e[p * F + i] = in[i].e[p];
#pragma unroll
        for (int i = 0; i < F; ++i) dst[(long long)g * F + i] = o.v[i];
    }
}

// One group of FPG frames of a stream's newly predicted frames [T0, T0 + nt).  The accessor maps an emitted frame t to
// (window, column): every column of window 0 (t < spf), then the last qs columns of each later window,
// j = (t - spf) / qs + 1, column t - qs j; window j of the call is clip clip0 + j - w_old.
template <int BASE, int P>
__global__ __launch_bounds__(64) void k_slide_synth(IstftArgs a, SynthArgs s, int qs, const SlideRow* __restrict__ rows,
                                                    const StreamItem* __restrict__ items) {
    const StreamItem it = items[blockIdx.x];
    const SlideRow& r = rows[it.b];
    const int b = it.b, t0 = it.chunk * istft640::FPG;
    const int ng = min(istft640::FPG, r.nt - t0);
    auto mel_db = [&](int m, int f) {
        const long long t = r.T0 + t0 + f;
        const long long j = t < a.spf ? 0 : (t - a.spf) / qs + 1;
        return a.mel_db[(((long long)r.clip0 + (j - r.w_old)) * a.n_mels + m) * (long long)a.spf + (int)(t - qs * j)];
    };
    auto stft = [&](int k, int f) { return s.phase_ring[((long long)b * s.R + (int)((r.T0 + t0 + f) % s.R)) * 321 + k]; };
    auto frame = [&](int f) { return s.frame_ring + ((long long)b * s.R + (int)((r.T0 + t0 + f) % s.R)) * (BASE * P); };
    if constexpr (BASE == 800) istft800::synth_frames<P>(a, ng, mel_db, stft, frame);
    else if constexpr (P == 1) istft640::synth_frames(a, ng, mel_db, stft, frame);
    else istft_poly::synth_frames<P>(a, ng, mel_db, stft, frame);
}

// the frame arithmetic a geometry runs on: n_fft = base * P.  0: none is built (avse_stream_supported's rule:
// 640 P at 16 / 32 / 48 kHz for 25-fps video, 800 P at 24 / 48 kHz for 30-fps video; a frame length belongs to its rate)
int stream_base(int sr, int n_fft) {
    if (n_fft == 640 || (n_fft == 1280 && sr == 32000) || (n_fft == 1920 && sr == 48000)) return 640;
    if ((n_fft == 800 && sr == 24000) || (n_fft == 1600 && sr == 48000)) return 800;
    return 0;
}

// ---- host: f(integral_constant<int, BASE>, integral_constant<int, P>) for the session's n_fft = BASE * P, the
// kernels' template arguments ----
template <class F>
void with_phases(int base, int P, F f) {
    using B640 = std::integral_constant<int, 640>;
    using B800 = std::integral_constant<int, 800>;
    if (base == 800) {
        if (P == 1) f(B800{}, std::integral_constant<int, 1>{});
        else f(B800{}, std::integral_constant<int, 2>{});
    } else if (P == 1) f(B640{}, std::integral_constant<int, 1>{});
    else if (P == 2) f(B640{}, std::integral_constant<int, 2>{});
    else f(B640{}, std::integral_constant<int, 3>{});
}

using Counts = StreamCounts;   // the host totals (stream_geom.h stream_totals)
static_assert(SCHUNK == STREAM_SCHUNK && ROUTE_X == STREAM_ROUTE_X && istft640::FPG == STREAM_SYNTH_FPG,
              "stream_geom.h chunks the kernels' work");

}  // namespace
}  // namespace avse

using namespace avse;

struct avse_stream {
    avse_ctx* ctx = nullptr;
    const avse_weights* w = nullptr;
    int64_t B = 0, max_slices = 0;
    int sr = 0, n_fft = 0, hop = 0, spf = 0, n_mels = 0, vdt = 0, F = 0;
    int base = 640;           // the frame arithmetic: 640 (frame640.h / frame_poly.h) or 800 (frame800.h)
    int P = 1;                // n_fft / base: the phases of a frame
    float amin = 0, top_db = 0, db_floor = 0;
    int R = 0, RS = 0, RV = 0;
    size_t vbytes = 0;
    SpecTables spec;
    IstftTables ist;
    Owned<float> tail, mel_ring, fmax_ring, run_max, net_in, pred, frame_ring;
    Owned<float2> phase_ring;
    Owned<char> vq, vstage;
    // host counters, per stream; while `uniform` (every stream's are equal) st[0] speaks for all, and the lock-step
    // calls run the lock-step kernels
    std::vector<StreamState> st;
    bool uniform = true;
    bool broken = false;
    // per-stream calls: the rows of the call being decided, and the pinned staging ring their tables go up from (one
    // slot per call in turn; `staged[i]` is recorded once the copy out of slot i is queued)
    static constexpr int SLOTS = 4;
    std::vector<StreamRow> rows;
    std::vector<int64_t> arg_n, arg_v, arg_off;   // a lock-step call's arguments, per stream
    std::vector<uint8_t> arg_flush;
    StreamItemCounts cap;     // items per table, all streams
    size_t slot_bytes = 0;
    Owned<char, true> staging;
    Owned<char> tables;       // device copy of the current call's tables
    hipEvent_t staged[SLOTS] = {};
    bool staged_used[SLOTS] = {};
    int slot = 0;
    // slices without video (avse_stream_push_each_mixed): host state.  vflag[b][k % RV] says whether queued video slice
    // k of stream b has video; every slot outside a stream's queue [slices done, v) holds 1, so the calls that know no
    // blank slice never write it.  blank_live counts the queued blank slices of all streams: while it is not 0 every
    // call takes the per-stream path that reads the flags.
    std::vector<uint8_t> vflag, clip_present;
    std::vector<int64_t> n_blank;
    std::vector<StreamItem> route_tmp;
    int64_t blank_live = 0;
    ~avse_stream() {
        for (hipEvent_t e : staged)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// every stream to one state: create / reset, and after a lock-step step
void stream_set_all(avse_stream* s, const StreamState& t) {
    std::fill(s->st.begin(), s->st.end(), t);
    s->uniform = true;
}

int stream_init_state(avse_stream* s, hipStream_t st) {
    AVSE_HIP_CHECK(hipMemsetAsync(s->tail, 0, s->tail.bytes, st));
    AVSE_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)s->run_max.p.get(), (int)0xff800000u, (size_t)s->B, st));   // -inf
    s->broken = false;
    stream_set_all(s, StreamState{0, 0, 0, 0});
    std::fill(s->vflag.begin(), s->vflag.end(), (uint8_t)1);
    std::fill(s->n_blank.begin(), s->n_blank.end(), (int64_t)0);
    s->blank_live = 0;
    return 0;
}

// after a per-stream step: are the streams in lock step again?
void stream_refresh_uniform(avse_stream* s) {
    const StreamState a = s->st[0];
    bool u = true;
    for (const StreamState& t : s->st) u = u && t.n == a.n && t.v == a.v && t.flushed == a.flushed && t.parity == a.parity;
    s->uniform = u;
}

// ---- the kernels' argument structs with the session's constants; a step sets the per-call fields ----
SpecStreamArgs spec_args(const avse_stream* s, const float* samples, int64_t sample_stride) {
    SpecStreamArgs a;
    std::memset(&a, 0, sizeof(a));
    a.news = samples; a.news_stride = sample_stride;
    a.spf = s->spf; a.R = s->R; a.RS = s->RS;
    a.twiddle = s->spec.twiddle; a.window = s->spec.window;
    a.mel_start = s->spec.mel.start; a.mel_weight = s->spec.mel.weight;
    std::memcpy(a.nq, s->spec.mel.seg_nq, sizeof(a.nq));
    a.amin = s->amin; a.db_floor = s->db_floor;
    a.mel_ring = s->mel_ring; a.phase_ring = s->phase_ring; a.fmax_ring = s->fmax_ring;
    return a;
}
RouteArgs route_args(const avse_stream* s, const void* video, float* mel_db) {
    RouteArgs r;
    std::memset(&r, 0, sizeof(r));
    r.mel_ring = s->mel_ring; r.fmax_ring = s->fmax_ring; r.run_max = s->run_max;
    r.net_in = s->net_in; r.mel_out = mel_db;
    r.spf = s->spf; r.R = s->R; r.RS = s->RS; r.top_db = s->top_db;
    r.vnew = reinterpret_cast<const char*>(video); r.vq = s->vq; r.vstage = s->vstage;
    r.vbytes = (long long)s->vbytes;
    r.RV = s->RV; r.B = (int)s->B;
    r.vec16 = (reinterpret_cast<uintptr_t>(video) & 15) == 0;
    return r;
}
IstftArgs istft_args(const avse_stream* s) {
    IstftArgs ia;
    std::memset(&ia, 0, sizeof(ia));
    ia.mel_db = s->pred; ia.spf = s->spf;
    ia.n_utt = (int)s->B; ia.nb = s->n_fft / 2 + 1; ia.N = s->n_fft; ia.hop = s->hop; ia.n_mels = s->n_mels;
    ia.pinvT = s->ist.pinvT; ia.twiddle = s->ist.twiddle; ia.window = s->ist.window;
    return ia;
}
SynthArgs synth_args(const avse_stream* s, int64_t T0, int nt) {
    SynthArgs sa;
    sa.phase_ring = s->phase_ring; sa.frame_ring = s->frame_ring;
    sa.T0 = T0; sa.nt = nt; sa.R = s->R;
    return sa;
}
OlaArgs ola_args(const avse_stream* s, float* out, int64_t out_stride, int64_t e_old, int64_t T, int n_out) {
    OlaArgs o;
    o.frame_ring = s->frame_ring; o.window = s->ist.window; o.out = out; o.out_stride = out_stride;
    o.e_old = e_old; o.T = T; o.n_out = n_out; o.R = s->R;
    return o;
}

// The next slot of the pinned staging ring, once the copy that last left it has been read: the only wait of a
// per-stream call, and only when SLOTS calls are still in flight.
int stream_stage_acquire(avse_stream* s, char** host) {
    const int i = s->slot;
    if (s->staged_used[i]) AVSE_HIP_CHECK(hipEventSynchronize(s->staged[i]));
    *host = s->staging + (size_t)i * s->slot_bytes;
    return 0;
}
int stream_stage_upload(avse_stream* s, size_t bytes, hipStream_t st) {
    const int i = s->slot;
    AVSE_HIP_CHECK(hipMemcpyAsync(s->tables, s->staging + (size_t)i * s->slot_bytes, bytes, hipMemcpyHostToDevice, st));
    AVSE_HIP_CHECK(hipEventRecord(s->staged[i], st));
    s->staged_used[i] = true;
    s->slot = (i + 1) % avse_stream::SLOTS;
    return 0;
}

// The work of a per-stream push: stream b receives n_new[b] samples and v_new[b] video slices and is closed when
// flush && flush[b].  host_n_out / host_k_new: per stream, nullable; host_max_out: nullable, the largest n_out.
int stream_step_each(avse_stream* s, const float* samples, const int64_t* sample_off, const int64_t* n_new, const void* video,
                     const int64_t* v_new, const uint8_t* flush, const float* vmean, const float* vstd, float* out,
                     int64_t out_stride, int64_t* host_n_out, int64_t* host_max_out, float* mel_db, float* pred_db,
                     int64_t* host_k_new, void* stream, const uint8_t* v_present = nullptr, uint8_t* host_k_present = nullptr) {
    const StreamCfg g{s->n_fft, s->hop, s->spf, s->max_slices};
    const int B = (int)s->B;
    StreamRow* rows = s->rows.data();
    const StreamPlan p = stream_rows(g, s->st.data(), B, sample_off, n_new, v_new, flush, out != nullptr, out_stride, rows);
    if (p.status != STREAM_OK)
        return fail(AVSE_ERR_INVALID, "stream " + std::to_string(p.bad) + ": " + stream_message(p.status));
    int64_t fed = 0;
    for (int b = 0; b < B; ++b) fed += rows[b].n_new - rows[b].n_old;
    // v_present (nullable: all present): which of the call's video slices have video; `video` holds only those.  A
    // call is `mixed` when it brings a blank slice or one is still queued: its video moves are listed one by one
    int64_t present_total = p.video_total;
    if (v_present) {
        present_total = 0;
        for (int64_t i = 0; i < p.video_total; ++i) present_total += v_present[i] != 0;
    }
    const bool mixed = present_total != p.video_total || s->blank_live > 0;
    if (fed > 0 && (!samples || !sample_off)) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (present_total > 0 && !video) {
        if (!v_present) return fail(AVSE_ERR_INVALID, "NULL argument");
        int64_t i = 0;   // the first slice that has video, and its stream
        while (!v_present[i]) ++i;
        int b = 0;
        while (i >= rows[b].video_off + rows[b].v_new) ++b;
        return fail(AVSE_ERR_INVALID, "stream " + std::to_string(b) + ": video is NULL but a slice is marked present");
    }
    if (present_total > 0 && (reinterpret_cast<uintptr_t>(video) & 3)) return fail(AVSE_ERR_INVALID, "video must be 4-byte aligned");
    const int RV = s->RV;
    // has video slice k of stream b video?  queued ones by their flag, this call's by v_present
    auto has_video = [&](int b, int64_t k) -> bool {
        if (k < rows[b].v_old) return s->vflag[(size_t)b * RV + (size_t)(k % RV)] != 0;
        return !v_present || v_present[rows[b].video_off + (k - rows[b].v_old)] != 0;
    };
    if (host_k_present) {
        uint8_t* kp = host_k_present;
        for (int b = 0; b < B; ++b)
            for (int kk = 0; kk < rows[b].k_new; ++kk) *kp++ = has_video(b, rows[b].k_old + kk);
    }
    hipStream_t st = (hipStream_t)stream;
    if (p.any) {
        if (int rc = not_capturing(st, "a per-stream push cannot be captured into a graph")) return rc;
    }
    for (int b = 0; b < B; ++b) {
        if (host_n_out) host_n_out[b] = rows[b].n_out;
        if (host_k_new) host_k_new[b] = rows[b].k_new;
    }
    if (host_max_out) *host_max_out = p.max_n_out;
    if (!p.any) return 0;
    AVSE_HIP_CHECK(hipSetDevice(s->ctx->device));
    // the tables: rows, then the four item tables, in one copy
    char* host = nullptr;
    if (int rc = stream_stage_acquire(s, &host)) return rc;
    const size_t row_bytes = sizeof(StreamRow) * (size_t)B;
    std::memcpy(host, rows, row_bytes);
    StreamItem* h_spec = reinterpret_cast<StreamItem*>(host + row_bytes);
    StreamItem* h_route = h_spec + p.items.spec;
    // mixed: the route table holds the clamp items of the streams that complete slices, then the moves of the slices
    // that have video (two item slots each: never more than the ROUTE_X items per moving slice it replaces)
    int64_t n_clamp = 0, n_moves = 0, n_present_clips = 0;
    int64_t route_units = p.items.route;
    if (mixed) {
        for (int b = 0; b < B; ++b) n_clamp += rows[b].k_new > 0;
        StreamItem* clamp = h_route;
        StreamMove* moves = reinterpret_cast<StreamMove*>(h_route + n_clamp);
        int64_t packed = 0;   // slices with video of this call's `video` seen so far (stream-major, as they are packed)
        for (int b = 0; b < B; ++b) {
            const StreamRow& r = rows[b];
            if (r.k_new > 0) *clamp++ = {(int32_t)b, STREAM_CLAMP};
            for (int kk = 0; kk < r.nv; ++kk) {
                const int64_t k = r.k_old + kk;
                const bool from_q = k < r.v_old, to_net = kk < r.k_new;
                if (from_q && !to_net) continue;   // stays queued
                const bool has = has_video(b, k);
                if (to_net) s->clip_present[(size_t)r.clip0 + kk] = has;
                const int32_t qslot = (int32_t)((int64_t)b * RV + k % RV);
                if (has) {
                    moves[n_moves++] = StreamMove{from_q ? 1 : 0, from_q ? qslot : (int32_t)packed, to_net ? 0 : 1,
                                                  to_net ? (int32_t)n_present_clips : qslot};
                    if (!from_q) ++packed;
                    if (to_net) ++n_present_clips;
                }
            }
        }
        route_units = n_clamp + 2 * n_moves;
    }
    StreamItem* h_synth = h_route + route_units;
    StreamItem* h_ola = h_synth + p.items.synth;
    stream_fill_items(g, rows, B, h_spec, mixed ? s->route_tmp.data() : h_route, h_synth, h_ola);
    const size_t n_items = (size_t)(p.items.spec + route_units + p.items.synth + p.items.ola);
    if (int rc = stream_stage_upload(s, row_bytes + sizeof(StreamItem) * n_items, st)) return rc;
    const StreamRow* d_rows = reinterpret_cast<const StreamRow*>(s->tables.p.get());
    const StreamItem* d_spec = reinterpret_cast<const StreamItem*>(s->tables + row_bytes);
    const StreamItem* d_route = d_spec + p.items.spec;
    const StreamItem* d_synth = d_route + route_units;
    const StreamItem* d_ola = d_synth + p.items.synth;
    // from here on a failure leaves the device state half updated: the session is broken until reset
    auto run = [&]() -> int {
        if (p.items.spec > 0) {
            SpecStreamArgs a = spec_args(s, samples, 0);  // row stride 0: + the row's sample_off
            a.tail_in = s->tail;                          // copies 0 / 1: the kernel picks by the row's parity
            a.tail_out = s->tail + (size_t)B * s->n_fft;
            with_phases(s->base, s->P, [&](auto BASE, auto P) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_spec<BASE, P, true>), dim3((unsigned)p.items.spec), dim3(64 * SWAVES), 0, st,
                                   a, d_rows, d_spec);
            });
            AVSE_HIP_CHECK(hipGetLastError());
        }
        if (mixed) {
            const RouteArgs ra = route_args(s, video, mel_db);
            if (n_moves > 0) {
                hipLaunchKernelGGL(k_stream_move, dim3((unsigned)(ROUTE_X * n_moves)), dim3(256), 0, st, ra.vnew, ra.vq, ra.vstage,
                                   ra.vbytes, ra.vec16, reinterpret_cast<const StreamMove*>(d_route + n_clamp));
                AVSE_HIP_CHECK(hipGetLastError());
            }
            if (n_clamp > 0) {   // the clamp blocks alone: the same kernel, no video item listed
                hipLaunchKernelGGL(k_stream_route<true>, dim3((unsigned)n_clamp), dim3(256), 0, st, ra, d_rows, d_route);
                AVSE_HIP_CHECK(hipGetLastError());
            }
        } else if (p.items.route > 0) {
            hipLaunchKernelGGL(k_stream_route<true>, dim3((unsigned)p.items.route), dim3(256), 0, st,
                               route_args(s, video, mel_db), d_rows, d_route);
            AVSE_HIP_CHECK(hipGetLastError());
        }
        if (p.clips > 0) {
            // mixed: vstage holds the clips with video, compacted, and the forward takes the clips' mask
            if (int rc = mixed ? avse_forward_mixed(s->ctx, s->w, s->net_in, s->vstage, s->vdt, vmean, vstd,
                                                    s->clip_present.data(), p.clips, s->pred, stream)
                               : avse_forward_video(s->ctx, s->w, s->net_in, s->vstage, s->vdt, vmean, vstd, p.clips, s->pred,
                                                    stream))
                return rc;
            if (pred_db)
                AVSE_HIP_CHECK(hipMemcpyAsync(pred_db, s->pred, sizeof(float) * (size_t)p.clips * NMEL * s->spf,
                                              hipMemcpyDeviceToDevice, st));
            with_phases(s->base, s->P, [&](auto BASE, auto P) {   // T0, nt: the rows'
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_synth<BASE, P, true>), dim3((unsigned)p.items.synth), dim3(64), 0, st,
                                   istft_args(s), synth_args(s, 0, 0), d_rows, d_synth);
            });
            AVSE_HIP_CHECK(hipGetLastError());
        }
        if (p.items.ola > 0) {
            with_phases(s->base, s->P, [&](auto BASE, auto P) {   // e_old, T, n_out: the rows'
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_ola<BASE, P, true>), dim3((unsigned)p.items.ola), dim3(256), 0, st,
                                   ola_args(s, out, out_stride, 0, 0, 0), d_rows, d_ola);
            });
            AVSE_HIP_CHECK(hipGetLastError());
        }
        return 0;
    };
    if (int rc = run()) {
        s->broken = true;
        return rc;
    }
    if (mixed) {
        // the flags after the call: a slice that went through the network frees its slot (1 again), one that is queued
        // now keeps what the call said of it
        for (int b = 0; b < B; ++b) {
            const StreamRow& r = rows[b];
            for (int64_t k = r.v_old; k < r.v_old + r.v_new; ++k) {   // before the slots below change
                const bool has = has_video(b, k);
                s->n_blank[b] += !has;
                if (!has && k >= r.k_old + r.k_new) {
                    s->vflag[(size_t)b * RV + (size_t)(k % RV)] = 0;
                    ++s->blank_live;
                }
            }
            for (int64_t k = r.k_old; k < std::min<int64_t>(r.k_old + r.k_new, r.v_old); ++k) {
                uint8_t& f = s->vflag[(size_t)b * RV + (size_t)(k % RV)];
                s->blank_live -= !f;
                f = 1;
            }
        }
    }
    stream_commit(rows, B, s->st.data());
    stream_refresh_uniform(s);
    return debug_poll(stream);
}

// a lock-step call on streams that are not in lock step: the per-stream step with the same counts for every stream
int stream_step_spread(avse_stream* s, bool flush, const float* samples, int64_t n_new, int64_t sample_stride,
                       const void* video, int64_t v_new, const float* vmean, const float* vstd, float* out,
                       int64_t out_stride, int64_t* host_n_out, float* mel_db, float* pred_db, void* stream) {
    bool open = false;
    for (int64_t b = 0; b < s->B; ++b) {
        s->arg_n[b] = n_new;
        s->arg_v[b] = v_new;
        s->arg_off[b] = b * sample_stride;
        s->arg_flush[b] = flush && !s->st[b].flushed;
        open = open || !s->st[b].flushed;
    }
    if (flush && !open) return fail(AVSE_ERR_INVALID, "flush after flush: only avse_stream_reset is legal");
    return stream_step_each(s, samples, s->arg_off.data(), s->arg_n.data(), video, s->arg_v.data(), s->arg_flush.data(), vmean,
                            vstd, out, out_stride, nullptr, host_n_out, mel_db, pred_db, nullptr, stream);
}

// The work of a push (n_new samples, v_new video slices) or of a flush (the remaining frames of the closed signal).
int stream_step(avse_stream* s, bool flush, const float* samples, int64_t n_new, int64_t sample_stride, const void* video,
                int64_t v_new, const float* vmean, const float* vstd, float* out, int64_t out_stride, int64_t* host_n_out,
                float* mel_db, float* pred_db, void* stream) {
    const StreamState cur = s->st[0];   // every stream's: the caller saw `uniform`
    const Counts c0 = stream_totals(s->n_fft, s->hop, s->spf, cur.n, cur.v, false);
    const int64_t n2 = cur.n + n_new, v2 = cur.v + v_new;
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
    const int tail_blk = n_new > 0 ? 1 : 0;   // the tail copies swap when samples arrive
    const StreamRow* no_rows = nullptr;       // the lock-step kernels read the call's scalars
    const StreamItem* no_items = nullptr;
    // from here on a failure leaves the device state half updated: the session is broken until reset
    auto run = [&]() -> int {
        const int64_t nt = c1.frames - c0.frames;
        if (n_new > 0 || nt > 0) {
            SpecStreamArgs a = spec_args(s, samples, sample_stride);
            a.tail_in = s->tail + (size_t)cur.parity * B * s->n_fft;
            a.tail_out = s->tail + (size_t)(cur.parity ^ 1) * B * s->n_fft;
            a.n_old = cur.n; a.n_new = n2;
            a.Lf = flush ? slice * v2 : -1;
            a.t0 = c0.frames; a.nt = (int)nt; a.nblk = (int)((nt + SCHUNK - 1) / SCHUNK);
            with_phases(s->base, s->P, [&](auto BASE, auto P) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_spec<BASE, P, false>), dim3(a.nblk + tail_blk, B), dim3(64 * SWAVES), 0, st,
                                   a, no_rows, no_items);
            });
            AVSE_HIP_CHECK(hipGetLastError());
        }
        const int64_t nv = v2 - c0.slices;   // video slices not yet consumed, this call's included
        if (k_new > 0 || v_new > 0) {
            RouteArgs r = route_args(s, video, mel_db);
            r.k_old = c0.slices; r.k_new = (int)k_new;
            r.v_old = cur.v; r.v_new = v_new;
            r.nv = (int)nv;
            hipLaunchKernelGGL(k_stream_route<false>, dim3((unsigned)(ROUTE_X * B * nv + (k_new > 0 ? B : 0))), dim3(256), 0, st,
                               r, no_rows, no_items);
            AVSE_HIP_CHECK(hipGetLastError());
        }
        if (k_new > 0) {
            if (int rc = avse_forward_video(s->ctx, s->w, s->net_in, s->vstage, s->vdt, vmean, vstd, B * k_new, s->pred, stream))
                return rc;
            if (pred_db)
                AVSE_HIP_CHECK(hipMemcpyAsync(pred_db, s->pred, sizeof(float) * (size_t)B * k_new * NMEL * s->spf,
                                              hipMemcpyDeviceToDevice, st));
            IstftArgs ia = istft_args(s);
            ia.n_slices = (int)k_new;
            ia.T = (int)(k_new * s->spf);
            with_phases(s->base, s->P, [&](auto BASE, auto P) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_synth<BASE, P, false>), dim3((ia.T + istft640::FPG - 1) / istft640::FPG, B),
                                   dim3(64), 0, st, ia, synth_args(s, c0.slices * s->spf, ia.T), no_rows, no_items);
            });
            AVSE_HIP_CHECK(hipGetLastError());
        }
        if (n_out > 0) {
            with_phases(s->base, s->P, [&](auto BASE, auto P) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_ola<BASE, P, false>), dim3((unsigned)((n_out + 255) / 256), B), dim3(256), 0,
                                   st, ola_args(s, out, out_stride, c0.emitted, c1.slices * s->spf, (int)n_out), no_rows, no_items);
            });
            AVSE_HIP_CHECK(hipGetLastError());
        }
        return 0;
    };
    if (int rc = run()) {
        s->broken = true;
        return rc;
    }
    stream_set_all(s, StreamState{n2, v2, (uint8_t)flush, (uint8_t)(cur.parity ^ tail_blk)});
    return debug_poll(stream);
}

}  // namespace

extern "C" {

int avse_stream_supported(int sr, int n_fft, int hop, int frames_per_slice, int n_mels, float fmin, float fmax) {
    if (sr <= 0 || n_fft < 2 || hop <= 0 || frames_per_slice < 1 || n_mels < 1) return fail(AVSE_ERR_INVALID, "bad stream geometry");
    // a geometry streams when slices do not drift against the samples: n_fft even and four hops long (the slice is
    // then frames_per_slice * hop samples by construction); of those, the 640-point kernels are built, their P-phase
    // forms for 2 x 640 at 32 kHz and 3 x 640 at 48 kHz, and the 800-point kernels of 30-fps video at 24 kHz and, in
    // two phases, at 48 kHz
    if (n_fft % 2 || n_fft != 4 * hop)
        return fail(AVSE_ERR_UNSUPPORTED, "streaming needs an even n_fft == 4 * hop (25 fps at 16, 32 or 48 kHz: 640 / 160, "
                                          "1280 / 320, 1920 / 480; 30 fps at 24 or 48 kHz: 800 / 200, 1600 / 400)");
    const int base = stream_base(sr, n_fft);
    if (!base || n_mels != NMEL)
        return fail(AVSE_ERR_UNSUPPORTED, "streaming is built for 25 fps at 16, 32 and 48 kHz (n_fft 640 / hop 160, 1280 / 320 at "
                                          "sr 32000, 1920 / 480 at sr 48000), for 30 fps at 24 and 48 kHz (800 / 200 at sr 24000, "
                                          "1600 / 400 at sr 48000), and 80 bands");
    // the bank the kernels will read (build_spec_tables makes the same one): every band within the 24-bin table, and
    // nothing above the last bin of the frame arithmetic: 320 of the 640-point one (always so at n_fft 640), 266 of the
    // 800-point one (the 30-Hz bins under 8 kHz)
    const int top = base == 640 ? 320 : spec800::KTOP;
    const MelBands mb = mel_bands(sr, n_fft, n_mels, fmin, fmax);
    bool low = true;
    for (int m = 0; m < n_mels; ++m) low = low && mb.start[m] + mb.width[m] - 1 <= top;
    if (mb.max_width != MW || !low)
        return fail(AVSE_ERR_UNSUPPORTED, base == 640
                        ? "streaming needs a Slaney bank whose bands fit 24 bins and lie in bins 0 .. 320 "
                          "(fmin 0, fmax 8000 at sr 16000, 32000 or 48000)"
                        : "streaming needs a Slaney bank whose bands fit 24 bins and lie in bins 0 .. 266 "
                          "(fmin 0, fmax 8000 at sr 24000 or 48000 with 30-fps video)");
    return 0;
}

int avse_stream_create(avse_ctx* c, const avse_weights* w, int64_t n_streams, int sr, int n_fft, int hop,
                       int frames_per_slice, int n_mels, float fmin, float fmax, float amin, float top_db, int video_dtype,
                       int64_t max_slices, avse_stream** out) {
    if (!c || !w || !out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n_streams < 1 || max_slices < 1 || sr <= 0 || n_fft < 2 || hop <= 0 || frames_per_slice < 1 || n_mels < 1 || !(amin > 0.f))
        return fail(AVSE_ERR_INVALID, "bad stream geometry");
    if (video_dtype != AVSE_VIDEO_F32 && video_dtype != AVSE_VIDEO_U8) return fail(AVSE_ERR_INVALID, "unknown video dtype");
    if (int rc = avse_stream_supported(sr, n_fft, hop, frames_per_slice, n_mels, fmin, fmax)) return rc;
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
    s->base = stream_base(sr, n_fft);
    s->P = n_fft / s->base;
    if (int rc = build_spec_tables(s->spec, sr, n_fft, n_mels, fmin, fmax)) return rc;
    if (s->spec.mel.max_width != MW) return fail(AVSE_ERR_UNSUPPORTED, "the mel tables differ from the bank avse_stream_supported saw");
    if (int rc = build_istft_tables(s->ist, sr, n_fft, n_mels, fmin, fmax)) return rc;
    s->RS = 2 * (int)max_slices + 1;
    s->R = s->RS * s->spf;
    s->RV = 2 * (int)max_slices;
    s->vbytes = (size_t)128 * 128 * wf * (video_dtype == AVSE_VIDEO_U8 ? 1 : 4);
    const size_t B = (size_t)n_streams, clips = B * (size_t)max_slices, per = (size_t)NMEL * s->spf;
    if (s->tail.alloc(sizeof(float) * 2 * B * n_fft) != hipSuccess ||
        s->mel_ring.alloc(sizeof(float) * B * s->RS * per) != hipSuccess ||
        s->fmax_ring.alloc(sizeof(float) * B * s->R) != hipSuccess ||
        s->run_max.alloc(sizeof(float) * B) != hipSuccess ||
        s->net_in.alloc(sizeof(float) * clips * per) != hipSuccess ||
        s->pred.alloc(sizeof(float) * clips * per) != hipSuccess ||
        s->frame_ring.alloc(sizeof(float) * B * s->R * n_fft) != hipSuccess ||
        s->phase_ring.alloc(sizeof(float2) * B * s->R * 321) != hipSuccess ||
        s->vq.alloc(B * s->RV * s->vbytes) != hipSuccess || s->vstage.alloc(clips * s->vbytes) != hipSuccess)
        return fail(AVSE_ERR_OOM, "hipMalloc failed (stream session)");
    // per-stream calls: host rows, and the worst-case tables of one call (stream_geom.h stream_item_caps) on the device
    // and in each slot of the pinned staging ring, so that no push allocates
    s->st.assign(B, StreamState{0, 0, 0, 0});
    s->rows.resize(B);
    s->arg_n.resize(B); s->arg_v.resize(B); s->arg_off.resize(B); s->arg_flush.resize(B);
    s->vflag.assign(B * s->RV, 1); s->clip_present.assign(clips, 1); s->n_blank.assign(B, 0);
    const StreamItemCounts per_stream = stream_item_caps(StreamCfg{n_fft, hop, frames_per_slice, max_slices});
    s->cap.spec = per_stream.spec * n_streams; s->cap.route = per_stream.route * n_streams;
    s->cap.synth = per_stream.synth * n_streams; s->cap.ola = per_stream.ola * n_streams;
    s->route_tmp.resize((size_t)s->cap.route);
    s->slot_bytes = (sizeof(StreamRow) * B + sizeof(StreamItem) * (size_t)s->cap.total() + 255) & ~(size_t)255;
    if (s->tables.alloc(s->slot_bytes) != hipSuccess) return fail(AVSE_ERR_OOM, "hipMalloc failed (stream session)");
    if (s->staging.alloc(s->slot_bytes * avse_stream::SLOTS) != hipSuccess)
        return fail(AVSE_ERR_OOM, "hipHostMalloc failed (stream session)");
    for (hipEvent_t& e : s->staged) AVSE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
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
    if (!s->uniform || s->blank_live > 0)   // queued blank slices: the per-stream path reads their flags
        return stream_step_spread(s, false, samples, n_new, sample_stride, video, v_new, vmean, vstd, out, out_stride,
                                  host_n_out, mel_db, pred_db, stream);
    if (s->st[0].flushed) return fail(AVSE_ERR_INVALID, "push after flush: only avse_stream_reset is legal");
    if (v_new > 0 && (reinterpret_cast<uintptr_t>(video) & 3)) return fail(AVSE_ERR_INVALID, "video must be 4-byte aligned");
    if (n_new > (1LL << 40) - s->st[0].n || v_new > (1LL << 30) - s->st[0].v) return fail(AVSE_ERR_INVALID, "counts too large");
    return stream_step(s, false, samples, n_new, sample_stride, video, v_new, vmean, vstd, out, out_stride, host_n_out, mel_db,
                       pred_db, stream);
}

int avse_stream_flush(avse_stream* s, const float* vmean, const float* vstd, float* out, int64_t out_stride,
                      int64_t* host_n_out, float* mel_db, float* pred_db, void* stream) {
    if (!s || !host_n_out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (out_stride < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    if ((vmean == nullptr) != (vstd == nullptr)) return fail(AVSE_ERR_INVALID, "vnorm_mean and vnorm_std must both be given");
    if (s->broken) return fail(AVSE_ERR_INVALID, "the session is broken by an earlier failure: avse_stream_reset it");
    if (!s->uniform || s->blank_live > 0)
        return stream_step_spread(s, true, nullptr, 0, 0, nullptr, 0, vmean, vstd, out, out_stride, host_n_out, mel_db, pred_db,
                                  stream);
    if (s->st[0].flushed) return fail(AVSE_ERR_INVALID, "flush after flush: only avse_stream_reset is legal");
    return stream_step(s, true, nullptr, 0, 0, nullptr, 0, vmean, vstd, out, out_stride, host_n_out, mel_db, pred_db, stream);
}

int avse_stream_push_each(avse_stream* s, const float* samples, const int64_t* sample_off, const int64_t* n_new,
                          const void* video, const int64_t* v_new, const uint8_t* flush, const float* vmean,
                          const float* vstd, float* out, int64_t out_stride, int64_t* host_n_out, float* mel_db,
                          float* pred_db, int64_t* host_k_new, void* stream) {
    if (!s || !n_new || !v_new || !host_n_out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (out_stride < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    if ((vmean == nullptr) != (vstd == nullptr)) return fail(AVSE_ERR_INVALID, "vnorm_mean and vnorm_std must both be given");
    if (s->broken) return fail(AVSE_ERR_INVALID, "the session is broken by an earlier failure: avse_stream_reset it");
    return stream_step_each(s, samples, sample_off, n_new, video, v_new, flush, vmean, vstd, out, out_stride, host_n_out,
                            nullptr, mel_db, pred_db, host_k_new, stream);
}

int avse_stream_push_each_mixed(avse_stream* s, const float* samples, const int64_t* sample_off, const int64_t* n_new,
                                const void* video, const int64_t* v_new, const uint8_t* v_present, const uint8_t* flush,
                                const float* vmean, const float* vstd, float* out, int64_t out_stride, int64_t* host_n_out,
                                float* mel_db, float* pred_db, int64_t* host_k_new, uint8_t* host_k_present, void* stream) {
    if (!s || !n_new || !v_new || !host_n_out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (out_stride < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    if ((vmean == nullptr) != (vstd == nullptr)) return fail(AVSE_ERR_INVALID, "vnorm_mean and vnorm_std must both be given");
    if (s->broken) return fail(AVSE_ERR_INVALID, "the session is broken by an earlier failure: avse_stream_reset it");
    return stream_step_each(s, samples, sample_off, n_new, video, v_new, flush, vmean, vstd, out, out_stride, host_n_out,
                            nullptr, mel_db, pred_db, host_k_new, stream, v_present, host_k_present);
}

int avse_stream_blank(const avse_stream* s, int64_t* n_blank) {
    if (!s || !n_blank) return fail(AVSE_ERR_INVALID, "NULL argument");
    for (int64_t b = 0; b < s->B; ++b) n_blank[b] = s->n_blank[b];
    return 0;
}

int avse_stream_reset(avse_stream* s, void* stream) {
    if (!s) return fail(AVSE_ERR_INVALID, "NULL argument");
    AVSE_HIP_CHECK(hipSetDevice(s->ctx->device));
    return stream_init_state(s, (hipStream_t)stream);
}

int avse_stream_reset_each(avse_stream* s, const uint8_t* which, void* stream) {
    if (!s || !which) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (s->broken) return fail(AVSE_ERR_INVALID, "the session is broken by an earlier failure: avse_stream_reset it");
    const int B = (int)s->B;
    int n = 0;
    for (int b = 0; b < B; ++b) n += which[b] != 0;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = not_capturing(st, "a per-stream reset cannot be captured into a graph")) return rc;
    AVSE_HIP_CHECK(hipSetDevice(s->ctx->device));
    char* host = nullptr;
    if (int rc = stream_stage_acquire(s, &host)) return rc;
    int* ids = reinterpret_cast<int*>(host);
    n = 0;
    for (int b = 0; b < B; ++b)
        if (which[b]) ids[n++] = b;
    if (int rc = stream_stage_upload(s, sizeof(int) * (size_t)n, st)) return rc;
    const int* ids_d = reinterpret_cast<const int*>(s->tables.p.get());
    with_phases(s->base, s->P, [&](auto BASE, auto P) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_reset<BASE, P>), dim3((unsigned)n), dim3(256), 0, st, s->tail.p.get(), s->run_max.p.get(), ids_d, B);
    });
    AVSE_HIP_CHECK(hipGetLastError());   // nothing ran: the session is as it was
    for (int b = 0; b < B; ++b)
        if (which[b]) {
            s->st[b] = StreamState{0, 0, 0, 0};
            for (int i = 0; i < s->RV; ++i) {   // its queued blank flags go with it
                uint8_t& f = s->vflag[(size_t)b * s->RV + i];
                s->blank_live -= !f;
                f = 1;
            }
            s->n_blank[b] = 0;
        }
    stream_refresh_uniform(s);
    return debug_poll(stream);
}

int avse_stream_state(const avse_stream* s, int64_t* n_samples, int64_t* n_video, uint8_t* flushed) {
    if (!s) return fail(AVSE_ERR_INVALID, "NULL argument");
    for (int64_t b = 0; b < s->B; ++b) {
        if (n_samples) n_samples[b] = s->st[b].n;
        if (n_video) n_video[b] = s->st[b].v;
        if (flushed) flushed[b] = s->st[b].flushed;
    }
    return 0;
}

void avse_stream_destroy(avse_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    delete s;
}

}  // extern "C"

// ---- K21: the sliding session ----
struct avse_slide {
    avse_stream core;         // K17's rings, tables and staging ring, sized by slide_geom.h's bounds; its video queue,
                              // host counters and blank flags stay empty
    SlideCfg g{};
    size_t fbytes = 0;        // bytes of a video frame
    Owned<char> vring;        // [B][RVf] frames
    std::vector<SlideState> st;
    std::vector<SlideRow> xrows;
    SlideItemCounts cap;      // items per table, all streams
};

namespace {

int slide_init_state(avse_slide* s, hipStream_t st) {
    if (int rc = stream_init_state(&s->core, st)) return rc;
    std::fill(s->st.begin(), s->st.end(), SlideState{0, 0, 0, 0});
    return 0;
}

template <class T>
void launch_gather(int F, unsigned blocks, hipStream_t st, const SlideGatherArgs& a, const SlideRow* rows, const StreamItem* items) {
    if (F == 5) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_slide_gather<T, 5>), dim3(blocks), dim3(256), 0, st, a, rows, items);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_slide_gather<T, 6>), dim3(blocks), dim3(256), 0, st, a, rows, items);
}

int slide_counts(const SlideCfg& g, int64_t n, int64_t f, int flushed, int64_t* frames, int64_t* windows, int64_t* predicted,
                 int64_t* emitted) {
    if (n < 0 || f < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    if (g.n_fft < 2 || g.hop < 1 || g.F < 1 || g.spf < 1 || g.spf % g.F) return fail(AVSE_ERR_INVALID, "bad slide geometry");
    if (g.stride < 1 || g.stride > g.F) return fail(AVSE_ERR_INVALID, "the stride must be 1 .. video_frames");
    if (flushed && n > (int64_t)g.hop * g.q() * f) return fail(AVSE_ERR_INVALID, "a flush needs n <= hop * q * f");
    const SlideCounts c = slide_totals(g, n, f, flushed != 0);
    if (frames) *frames = c.frames;
    if (windows) *windows = c.windows;
    if (predicted) *predicted = c.predicted;
    if (emitted) *emitted = c.emitted;
    return 0;
}

}  // namespace

extern "C" {

int avse_slide_supported(int sr, int n_fft, int hop, int frames_per_slice, int video_frames, int stride, int n_mels, float fmin,
                         float fmax) {
    if (video_frames < 1) return fail(AVSE_ERR_INVALID, "bad stream geometry");
    if (int rc = avse_stream_supported(sr, n_fft, hop, frames_per_slice, n_mels, fmin, fmax)) return rc;
    if (stride < 1 || stride > video_frames) return fail(AVSE_ERR_INVALID, "the stride must be 1 .. video_frames");
    if (frames_per_slice % video_frames)
        return fail(AVSE_ERR_UNSUPPORTED, "a sliding session needs frames_per_slice % video_frames == 0");
    if (video_frames != 5 && video_frames != 6)
        return fail(AVSE_ERR_UNSUPPORTED, "the sliding session's video gather is built for 5 and 6 video frames per window");
    return 0;
}

int avse_slide_create(avse_ctx* c, const avse_weights* w, int64_t n_streams, int sr, int n_fft, int hop, int frames_per_slice,
                      int stride, int n_mels, float fmin, float fmax, float amin, float top_db, int video_dtype,
                      int64_t max_windows, avse_slide** out) {
    if (!c || !w || !out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n_streams < 1 || max_windows < 1 || sr <= 0 || n_fft < 2 || hop <= 0 || frames_per_slice < 1 || n_mels < 1 || !(amin > 0.f))
        return fail(AVSE_ERR_INVALID, "bad stream geometry");
    if (video_dtype != AVSE_VIDEO_F32 && video_dtype != AVSE_VIDEO_U8) return fail(AVSE_ERR_INVALID, "unknown video dtype");
    if (stride < 1) return fail(AVSE_ERR_INVALID, "the stride must be 1 .. video_frames");
    // what does not depend on the weights first, so that a geometry no kernel serves is refused before they are read
    if (int rc = avse_stream_supported(sr, n_fft, hop, frames_per_slice, n_mels, fmin, fmax)) return rc;
    int wt = 0, wf = 0;
    if (int rc = avse_weights_shape(w, &wt, &wf)) return rc;
    if (int rc = avse_slide_supported(sr, n_fft, hop, frames_per_slice, wf, stride, n_mels, fmin, fmax)) return rc;
    if (n_streams > 1024 || max_windows > SLIDE_MAX_WINDOWS)
        return fail(AVSE_ERR_UNSUPPORTED, "at most 1024 streams and max_windows 80");
    if (w->device != c->device) return fail(AVSE_ERR_INVALID, "weights and context are on different devices");
    if (wt != frames_per_slice)
        return fail(AVSE_ERR_INVALID, "the weights were loaded for slices of " + std::to_string(wt) + " frames, not " +
                                          std::to_string(frames_per_slice));
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    std::unique_ptr<avse_slide> sl(new avse_slide());
    sl->g = SlideCfg{n_fft, hop, frames_per_slice, wf, stride, max_windows};
    avse_stream* s = &sl->core;
    s->ctx = c; s->w = w; s->B = n_streams; s->max_slices = max_windows;
    s->sr = sr; s->n_fft = n_fft; s->hop = hop; s->spf = frames_per_slice; s->n_mels = n_mels; s->vdt = video_dtype; s->F = wf;
    s->amin = amin; s->top_db = top_db;
    s->db_floor = (float)(20.0 * std::log10((double)amin));
    s->base = stream_base(sr, n_fft);
    s->P = n_fft / s->base;
    if (int rc = build_spec_tables(s->spec, sr, n_fft, n_mels, fmin, fmax)) return rc;
    if (s->spec.mel.max_width != MW) return fail(AVSE_ERR_UNSUPPORTED, "the mel tables differ from the bank avse_stream_supported saw");
    if (int rc = build_istft_tables(s->ist, sr, n_fft, n_mels, fmin, fmax)) return rc;
    s->RS = sl->g.RS();
    s->R = sl->g.R();
    sl->fbytes = (size_t)128 * 128 * (video_dtype == AVSE_VIDEO_U8 ? 1 : 4);
    s->vbytes = sl->fbytes * wf;
    const size_t B = (size_t)n_streams, clips = B * (size_t)max_windows, per = (size_t)NMEL * s->spf;
    if (s->tail.alloc(sizeof(float) * 2 * B * n_fft) != hipSuccess ||
        s->mel_ring.alloc(sizeof(float) * B * s->RS * per) != hipSuccess ||
        s->fmax_ring.alloc(sizeof(float) * B * s->R) != hipSuccess ||
        s->run_max.alloc(sizeof(float) * B) != hipSuccess ||
        s->net_in.alloc(sizeof(float) * clips * per) != hipSuccess ||
        s->pred.alloc(sizeof(float) * clips * per) != hipSuccess ||
        s->frame_ring.alloc(sizeof(float) * B * s->R * n_fft) != hipSuccess ||
        s->phase_ring.alloc(sizeof(float2) * B * s->R * 321) != hipSuccess ||
        sl->vring.alloc(B * sl->g.RVf() * sl->fbytes) != hipSuccess || s->vstage.alloc(clips * s->vbytes) != hipSuccess)
        return fail(AVSE_ERR_OOM, "hipMalloc failed (slide session)");
    sl->st.assign(B, SlideState{0, 0, 0, 0});
    s->rows.resize(B);
    sl->xrows.resize(B);
    const SlideItemCounts per_stream = slide_item_caps(sl->g);
    sl->cap.spec = per_stream.spec * n_streams; sl->cap.route = per_stream.route * n_streams;
    sl->cap.gather = per_stream.gather * n_streams; sl->cap.synth = per_stream.synth * n_streams;
    sl->cap.ola = per_stream.ola * n_streams;
    s->slot_bytes = ((sizeof(StreamRow) + sizeof(SlideRow)) * B + sizeof(StreamItem) * (size_t)sl->cap.total() + 255) & ~(size_t)255;
    if (s->tables.alloc(s->slot_bytes) != hipSuccess) return fail(AVSE_ERR_OOM, "hipMalloc failed (slide session)");
    if (s->staging.alloc(s->slot_bytes * avse_stream::SLOTS) != hipSuccess)
        return fail(AVSE_ERR_OOM, "hipHostMalloc failed (slide session)");
    for (hipEvent_t& e : s->staged) AVSE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    // a slot read before its first write holds zeros, never stale memory
    AVSE_HIP_CHECK(hipMemset(s->frame_ring, 0, s->frame_ring.bytes));
    AVSE_HIP_CHECK(hipMemset(s->phase_ring, 0, s->phase_ring.bytes));
    AVSE_HIP_CHECK(hipMemset(s->mel_ring, 0, s->mel_ring.bytes));
    AVSE_HIP_CHECK(hipMemset(s->fmax_ring, 0, s->fmax_ring.bytes));
    AVSE_HIP_CHECK(hipMemset(sl->vring, 0, sl->vring.bytes));
    if (int rc = avse_ctx_reserve_weights(c, w, (int64_t)clips)) return rc;   // pushes never grow the forward scratch
    if (int rc = slide_init_state(sl.get(), nullptr)) return rc;
    AVSE_HIP_CHECK(hipStreamSynchronize(nullptr));
    *out = sl.release();
    return 0;
}

int avse_slide_counts_geom(int n_fft, int hop, int frames_per_slice, int video_frames, int stride, int64_t n_samples,
                           int64_t n_video_frames, int flushed, int64_t* frames, int64_t* windows, int64_t* predicted,
                           int64_t* emitted) {
    return slide_counts(SlideCfg{n_fft, hop, frames_per_slice, video_frames, stride, 1}, n_samples, n_video_frames, flushed, frames,
                        windows, predicted, emitted);
}

int avse_slide_counts(const avse_slide* s, int stride, int64_t n_samples, int64_t n_video_frames, int flushed, int64_t* frames,
                      int64_t* windows, int64_t* predicted, int64_t* emitted) {
    SlideCfg g = s ? s->g : SlideCfg{640, 160, 20, 5, 1, 1};
    g.stride = stride;
    return slide_counts(g, n_samples, n_video_frames, flushed, frames, windows, predicted, emitted);
}

int avse_slide_push_each(avse_slide* sl, const float* samples, const int64_t* sample_off, const int64_t* n_new, const void* video,
                         const int64_t* f_new, const uint8_t* flush, const float* vmean, const float* vstd, float* out,
                         int64_t out_stride, int64_t* host_n_out, float* mel_db, float* pred_db, int64_t* host_w_new,
                         void* stream) {
    if (!sl || !n_new || !f_new || !host_n_out) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (out_stride < 0) return fail(AVSE_ERR_INVALID, "negative counts");
    if ((vmean == nullptr) != (vstd == nullptr)) return fail(AVSE_ERR_INVALID, "vnorm_mean and vnorm_std must both be given");
    avse_stream* s = &sl->core;
    if (s->broken) return fail(AVSE_ERR_INVALID, "the session is broken by an earlier failure: avse_slide_reset it");
    const SlideCfg& g = sl->g;
    const int B = (int)s->B;
    StreamRow* rows = s->rows.data();
    SlideRow* xrows = sl->xrows.data();
    const SlidePlan p = slide_rows(g, sl->st.data(), B, sample_off, n_new, f_new, flush, out != nullptr, out_stride, rows, xrows);
    if (p.status != SLIDE_OK)
        return fail(AVSE_ERR_INVALID, "stream " + std::to_string(p.bad) + ": " + slide_message(p.status));
    int64_t fed = 0;
    for (int b = 0; b < B; ++b) fed += rows[b].n_new - rows[b].n_old;
    if ((fed > 0 && (!samples || !sample_off)) || (p.video_total > 0 && !video)) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (p.video_total > 0 && (reinterpret_cast<uintptr_t>(video) & 3)) return fail(AVSE_ERR_INVALID, "video must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (p.any) {
        if (int rc = not_capturing(st, "a sliding push cannot be captured into a graph")) return rc;
    }
    for (int b = 0; b < B; ++b) {
        host_n_out[b] = rows[b].n_out;
        if (host_w_new) host_w_new[b] = xrows[b].w_new;
    }
    if (!p.any) return 0;
    AVSE_HIP_CHECK(hipSetDevice(s->ctx->device));
    // the tables: both rows of every stream, then the five item tables, in one copy
    char* host = nullptr;
    if (int rc = stream_stage_acquire(s, &host)) return rc;
    const size_t row_bytes = sizeof(StreamRow) * (size_t)B, xrow_bytes = sizeof(SlideRow) * (size_t)B;
    std::memcpy(host, rows, row_bytes);
    std::memcpy(host + row_bytes, xrows, xrow_bytes);
    StreamItem* h_spec = reinterpret_cast<StreamItem*>(host + row_bytes + xrow_bytes);
    StreamItem* h_route = h_spec + p.items.spec;
    StreamItem* h_gather = h_route + p.items.route;
    StreamItem* h_synth = h_gather + p.items.gather;
    StreamItem* h_ola = h_synth + p.items.synth;
    slide_fill_items(rows, xrows, B, h_spec, h_route, h_gather, h_synth, h_ola);
    if (int rc = stream_stage_upload(s, row_bytes + xrow_bytes + sizeof(StreamItem) * (size_t)p.items.total(), st)) return rc;
    const StreamRow* d_rows = reinterpret_cast<const StreamRow*>(s->tables.p.get());
    const SlideRow* d_xrows = reinterpret_cast<const SlideRow*>(s->tables + row_bytes);
    const StreamItem* d_spec = reinterpret_cast<const StreamItem*>(s->tables + row_bytes + xrow_bytes);
    const StreamItem* d_route = d_spec + p.items.spec;
    const StreamItem* d_gather = d_route + p.items.route;
    const StreamItem* d_synth = d_gather + p.items.gather;
    const StreamItem* d_ola = d_synth + p.items.synth;
    // from here on a failure leaves the device state half updated: the session is broken until reset
    auto run = [&]() -> int {
        if (p.items.spec > 0) {
            SpecStreamArgs a = spec_args(s, samples, 0);  // row stride 0: + the row's sample_off
            a.tail_in = s->tail;                          // copies 0 / 1: the kernel picks by the row's parity
            a.tail_out = s->tail + (size_t)B * s->n_fft;
            with_phases(s->base, s->P, [&](auto BASE, auto P) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_spec<BASE, P, true>), dim3((unsigned)p.items.spec), dim3(64 * SWAVES), 0, st,
                                   a, d_rows, d_spec);
            });
            AVSE_HIP_CHECK(hipGetLastError());
        }
        if (p.items.gather > 0) {
            SlideGatherArgs ga;
            ga.vnew = reinterpret_cast<const char*>(video); ga.vring = sl->vring; ga.vstage = s->vstage;
            ga.stride = g.stride; ga.RVf = g.RVf();
            ga.vec16 = (reinterpret_cast<uintptr_t>(video) & 15) == 0;
            if (s->vdt == AVSE_VIDEO_U8) launch_gather<uint8_t>(g.F, (unsigned)p.items.gather, st, ga, d_xrows, d_gather);
            else launch_gather<float>(g.F, (unsigned)p.items.gather, st, ga, d_xrows, d_gather);
            AVSE_HIP_CHECK(hipGetLastError());
        }
        if (p.clips > 0) {
            SlideRouteArgs ra;
            ra.mel_ring = s->mel_ring; ra.fmax_ring = s->fmax_ring; ra.run_max = s->run_max;
            ra.net_in = s->net_in; ra.mel_out = mel_db;
            ra.spf = s->spf; ra.qs = g.qs(); ra.R = s->R; ra.RS = s->RS; ra.top_db = s->top_db;
            hipLaunchKernelGGL(k_slide_route, dim3((unsigned)p.items.route), dim3(256), 0, st, ra, d_xrows, d_route);
            AVSE_HIP_CHECK(hipGetLastError());
            if (int rc = avse_forward_video(s->ctx, s->w, s->net_in, s->vstage, s->vdt, vmean, vstd, p.clips, s->pred, stream))
                return rc;
            if (pred_db)
                AVSE_HIP_CHECK(hipMemcpyAsync(pred_db, s->pred, sizeof(float) * (size_t)p.clips * NMEL * s->spf,
                                              hipMemcpyDeviceToDevice, st));
            with_phases(s->base, s->P, [&](auto BASE, auto P) {   // T0, nt: the rows'
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_slide_synth<BASE, P>), dim3((unsigned)p.items.synth), dim3(64), 0, st,
                                   istft_args(s), synth_args(s, 0, 0), g.qs(), d_xrows, d_synth);
            });
            AVSE_HIP_CHECK(hipGetLastError());
        }
        if (p.items.ola > 0) {
            with_phases(s->base, s->P, [&](auto BASE, auto P) {   // e_old, T, n_out: the rows'
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_ola<BASE, P, true>), dim3((unsigned)p.items.ola), dim3(256), 0, st,
                                   ola_args(s, out, out_stride, 0, 0, 0), d_rows, d_ola);
            });
            AVSE_HIP_CHECK(hipGetLastError());
        }
        return 0;
    };
    if (int rc = run()) {
        s->broken = true;
        return rc;
    }
    slide_commit(rows, xrows, B, sl->st.data());
    return debug_poll(stream);
}

int avse_slide_reset(avse_slide* sl, void* stream) {
    if (!sl) return fail(AVSE_ERR_INVALID, "NULL argument");
    AVSE_HIP_CHECK(hipSetDevice(sl->core.ctx->device));
    return slide_init_state(sl, (hipStream_t)stream);
}

int avse_slide_reset_each(avse_slide* sl, const uint8_t* which, void* stream) {
    if (!sl || !which) return fail(AVSE_ERR_INVALID, "NULL argument");
    avse_stream* s = &sl->core;
    if (s->broken) return fail(AVSE_ERR_INVALID, "the session is broken by an earlier failure: avse_slide_reset it");
    const int B = (int)s->B;
    int n = 0;
    for (int b = 0; b < B; ++b) n += which[b] != 0;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = not_capturing(st, "a per-stream reset cannot be captured into a graph")) return rc;
    AVSE_HIP_CHECK(hipSetDevice(s->ctx->device));
    char* host = nullptr;
    if (int rc = stream_stage_acquire(s, &host)) return rc;
    int* ids = reinterpret_cast<int*>(host);
    n = 0;
    for (int b = 0; b < B; ++b)
        if (which[b]) ids[n++] = b;
    if (int rc = stream_stage_upload(s, sizeof(int) * (size_t)n, st)) return rc;
    const int* ids_d = reinterpret_cast<const int*>(s->tables.p.get());
    with_phases(s->base, s->P, [&](auto BASE, auto P) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_reset<BASE, P>), dim3((unsigned)n), dim3(256), 0, st, s->tail.p.get(), s->run_max.p.get(), ids_d, B);
    });
    AVSE_HIP_CHECK(hipGetLastError());   // nothing ran: the session is as it was
    for (int b = 0; b < B; ++b)
        if (which[b]) sl->st[b] = SlideState{0, 0, 0, 0};
    return debug_poll(stream);
}

int avse_slide_state(const avse_slide* sl, int64_t* n_samples, int64_t* n_video_frames, uint8_t* flushed) {
    if (!sl) return fail(AVSE_ERR_INVALID, "NULL argument");
    for (int64_t b = 0; b < sl->core.B; ++b) {
        if (n_samples) n_samples[b] = sl->st[b].n;
        if (n_video_frames) n_video_frames[b] = sl->st[b].f;
        if (flushed) flushed[b] = sl->st[b].flushed;
    }
    return 0;
}

void avse_slide_destroy(avse_slide* sl) {
    if (!sl) return;
    (void)hipSetDevice(sl->core.ctx->device);
    delete sl;
}

}  // extern "C"
