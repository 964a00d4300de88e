// Host-only geometry of ragged STFT / ISTFT batches (no HIP header): from the callers' per-utterance length arrays,
// the frame / slice / chunk counts, the int64 offsets of every packed buffer (include/avse.h
// avse_spectrogram_ragged / avse_istft_ragged), the flat item table item -> (utterance, chunk) a ragged kernel's
// blocks index, the element-range -> utterance map of the top_db clamp pass, and the maximal runs of consecutive
// equal-length utterances the launchers hand to the equal-length kernels.  RaggedUtt / RaggedItem are also the
// device-side rows (capi.hip uploads them into the context's preprocess scratch; stft.hip / istft.hip read them).
#pragma once
#include <cstdint>
#include <vector>

namespace avse {

// One utterance of a ragged batch.  The STFT and the ISTFT share the row: `in` is what the kernel reads besides the
// mel block, `out` what it writes besides it.
struct RaggedUtt {
    int64_t in_off;      // STFT: first sample in `sig` (the caller's sig_off);  ISTFT: first complex element of its STFT
    int64_t mel_off;     // first float of its mel block ([n_mels][T], or [S][n_mels][spf])
    int64_t out_off;     // STFT: first complex element of its STFT block;        ISTFT: first output sample
    int32_t L;           // STFT: n_samples;                                      ISTFT: stft_frames
    int32_t T;           // frames (STFT: centred frame count; ISTFT: frames reconstructed)
    int32_t S;           // slices (T / spf; 0 when spf == 0)
    int32_t first_item;  // index of its chunk 0 in the item table
};
static_assert(sizeof(RaggedUtt) == 40, "device row layout");

struct RaggedItem {      // one block's work: chunk `chunk` of utterance `u`
    int32_t u, chunk;
};

struct RaggedRun {       // utterances [first, first + count): one length, and laid out as an equal-length batch
    int64_t first, count;
};

enum RaggedStatus {
    RAGGED_OK = 0,
    RAGGED_BAD_COUNT,        // a negative (STFT: non-positive) length
    RAGGED_REFLECT_SHORT,    // reflect padding on an utterance of at most n_fft / 2 samples
    RAGGED_NOT_SLICED,       // n_frames[u] is no multiple of frames_per_slice
    RAGGED_PAST_STFT,        // n_frames[u] > stft_frames[u]
    RAGGED_TOO_LARGE,        // an utterance or the item table past int32
};

inline const char* ragged_message(int status) {
    switch (status) {
        case RAGGED_BAD_COUNT: return "a length is negative (n_samples must be positive, n_frames / stft_frames >= 0)";
        case RAGGED_REFLECT_SHORT: return "reflect padding needs n_samples > n_fft/2 for every utterance";
        case RAGGED_NOT_SLICED: return "every n_frames must be a multiple of frames_per_slice";
        case RAGGED_PAST_STFT: return "n_frames must not exceed stft_frames for any utterance";
        case RAGGED_TOO_LARGE: return "ragged batch too large (an utterance or the item table passes int32)";
        default: return "ok";
    }
}

struct RaggedGeom {
    int status = RAGGED_OK;
    int64_t bad_utt = -1;                 // the utterance `status` refers to
    std::vector<RaggedUtt> utt;           // [n_utt]
    std::vector<RaggedItem> items;        // [sum of chunk counts], utterance-major
    std::vector<int32_t> n_chunks;        // [n_utt]
    std::vector<RaggedRun> runs;
    int64_t mel_total = 0;                // floats of the packed mel buffer
    int64_t in_total = 0;                 // ISTFT: complex elements of the packed STFT (STFT: unused, the caller's offsets)
    int64_t out_total = 0;                // STFT: complex elements of the packed STFT; ISTFT: output samples
};

// centred frame count of librosa.stft (the equal-length avse_spectrogram's formula)
inline int64_t ragged_frames(int64_t n_samples, int n_fft, int hop) {
    return 1 + (n_samples + 2 * (n_fft / 2) - n_fft) / hop;
}

// The clamp pass's map: the utterance whose mel block holds element i (0 <= i < mel_total): the last u with
// mel_off[u] <= i.  Utterances without mel (zero slices) share their successor's offset and are never the last.
// (k_spec_clamp_ragged runs the same search on the device rows.)
inline int64_t ragged_mel_utt(const RaggedUtt* utt, int64_t n_utt, int64_t i) {
    int64_t lo = 0, hi = n_utt - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (utt[mid].mel_off <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

namespace ragged_detail {
inline bool finish(RaggedGeom& g, int chunk_rule_istft, int chunk) {
    int64_t items = 0;
    const int64_t n = (int64_t)g.utt.size();
    g.n_chunks.resize(n);
    for (int64_t u = 0; u < n; ++u) {
        const int64_t T = g.utt[u].T;
        const int64_t span = chunk_rule_istft ? T - 1 : T;        // the ISTFT chunks its hop * (T - 1) output hops
        const int64_t nc = span > 0 ? (span + chunk - 1) / chunk : 0;
        if (items + nc > INT32_MAX) {
            g.status = RAGGED_TOO_LARGE;
            g.bad_utt = u;
            return false;
        }
        g.utt[u].first_item = (int32_t)items;
        g.n_chunks[u] = (int32_t)nc;
        items += nc;
    }
    g.items.reserve(items);
    for (int64_t u = 0; u < n; ++u)
        for (int32_t c = 0; c < g.n_chunks[u]; ++c) g.items.push_back({(int32_t)u, c});
    return true;
}
inline RaggedGeom fail(RaggedGeom& g, int status, int64_t u) {
    g.status = status;
    g.bad_utt = u;
    return g;
}
}  // namespace ragged_detail

// STFT: utterance u is n_samples[u] samples from sig + sig_off[u].  spf = frames_per_slice (0: the [n_mels][T]
// layout), chunk = frames per block of the kernel that will run (any positive value where only the offsets matter).
// A run continues while the next utterance has the same length and starts where an equal-length batch would put it.
inline RaggedGeom ragged_spec_geom(const int64_t* sig_off, const int64_t* n_samples, int64_t n_utt, int n_fft, int hop,
                                   int spf, int n_mels, bool reflect, int chunk) {
    RaggedGeom g;
    g.utt.resize(n_utt > 0 ? n_utt : 0);
    const int64_t nb = n_fft / 2 + 1;
    for (int64_t u = 0; u < n_utt; ++u) {
        const int64_t L = n_samples[u];
        if (L <= 0) return ragged_detail::fail(g, RAGGED_BAD_COUNT, u);
        if (reflect && L <= n_fft / 2) return ragged_detail::fail(g, RAGGED_REFLECT_SHORT, u);
        if (L > INT32_MAX - 2 * (int64_t)n_fft) return ragged_detail::fail(g, RAGGED_TOO_LARGE, u);
        const int64_t T = ragged_frames(L, n_fft, hop);
        const int64_t S = spf > 0 ? T / spf : 0;
        RaggedUtt& r = g.utt[u];
        r.in_off = sig_off[u];
        r.mel_off = g.mel_total;
        r.out_off = g.out_total;
        r.L = (int32_t)L;
        r.T = (int32_t)T;
        r.S = (int32_t)S;
        r.first_item = 0;
        g.mel_total += spf > 0 ? S * n_mels * spf : (int64_t)n_mels * T;
        g.out_total += nb * T;
        if (u > 0 && n_samples[u - 1] == L && sig_off[u] == sig_off[u - 1] + L) ++g.runs.back().count;
        else g.runs.push_back({u, 1});
    }
    ragged_detail::finish(g, 0, chunk);
    return g;
}

// ISTFT: utterance u reconstructs n_frames[u] frames against a mixture STFT of stft_frames[u] frames; nb bins.
// Its output is hop * (n_frames[u] - 1) samples, nothing below two frames; chunk = output hops per block.
inline RaggedGeom ragged_istft_geom(const int64_t* n_frames, const int64_t* stft_frames, int64_t n_utt, int spf, int nb,
                                    int hop, int n_mels, int chunk) {
    RaggedGeom g;
    g.utt.resize(n_utt > 0 ? n_utt : 0);
    for (int64_t u = 0; u < n_utt; ++u) {
        const int64_t T = n_frames[u], F = stft_frames[u];
        if (T < 0 || F < 0) return ragged_detail::fail(g, RAGGED_BAD_COUNT, u);
        if (spf > 0 && T % spf) return ragged_detail::fail(g, RAGGED_NOT_SLICED, u);
        if (T > F) return ragged_detail::fail(g, RAGGED_PAST_STFT, u);
        // 32-bit byte offsets into one utterance's STFT and mel block (the fused kernel's buffer resources)
        if ((int64_t)nb * F * 8 >= 0x7fffff00LL || (int64_t)n_mels * T * 4 >= 0x7fffff00LL)
            return ragged_detail::fail(g, RAGGED_TOO_LARGE, u);
        RaggedUtt& r = g.utt[u];
        r.in_off = g.in_total;
        r.mel_off = g.mel_total;
        r.out_off = g.out_total;
        r.L = (int32_t)F;
        r.T = (int32_t)T;
        r.S = (int32_t)(spf > 0 ? T / spf : 0);
        r.first_item = 0;
        g.in_total += (int64_t)nb * F;
        g.mel_total += (int64_t)n_mels * T;          // [n_mels][T], or [T / spf][n_mels][spf]: the same count
        g.out_total += T >= 2 ? (int64_t)hop * (T - 1) : 0;
        if (u > 0 && n_frames[u - 1] == T && stft_frames[u - 1] == F) ++g.runs.back().count;
        else g.runs.push_back({u, 1});
    }
    ragged_detail::finish(g, 1, chunk);
    return g;
}

}  // namespace avse
