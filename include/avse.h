/*
 * avse.h — C-ABI of libavse.so, the MI355X-native (gfx950) hot path of
 * melspectrum007/audio-visual-speech-enhancement.
 *
 * The reference has no FFI layer: its hot path is the Python API below, whose arithmetic is
 * delegated to librosa / numpy / Keras.  Each entry point names the reference interface it
 * replaces (file:line into /root/reference).  The build's Python package
 * (audio-visual-speech-enhancement_amd/) binds these symbols with ctypes; INTEGRATION.md shows
 * the binding a maintainer of the reference would add.
 *
 * Conventions
 *  - Every data pointer is a DEVICE pointer into caller-owned memory, unless the parameter name
 *    starts with host_.
 *  - Calls are asynchronous and ordered on `stream` (a hipStream_t passed as void*; NULL = the
 *    legacy default stream).  No call synchronises the device.
 *  - Every call returns an int status (AVSE_OK = 0).  avse_last_error() returns a thread-local
 *    message for the last failing call on this thread.
 *  - A context belongs to one device; it is not thread-safe (lock externally).
 *  - Buffers are row-major, C-contiguous, float32 unless stated.
 */
#ifndef AVSE_H
#define AVSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: compute dtype AVSE_F32_SPLIT, avse_ctx_reserve_weights; option names tile_alt / aud_side removed (round 3);
 *    status AVSE_ERR_CHECK (checked build)
 * 3: AVSE_F32_SPLIT range guard (avse_forward_checked, avse_range_status, status AVSE_ERR_RANGE), per-layer activation
 *    exponents (avse_weights_act_exponents, option no_act_scale); later additions under the same version (new symbols
 *    only, nothing existing changed): avse_mix_pairs, avse_video_stats, avse_eval_pairs,
 *    avse_eval_pairs_sized, avse_eval_pairs_ext, avse_stream_create, avse_stream_counts, avse_stream_push,
 *    avse_stream_flush, avse_stream_reset, avse_stream_destroy, avse_stream_push_each, avse_stream_reset_each,
 *    avse_stream_state, avse_stream_supported, avse_resample_supported, avse_resample_counts, avse_resample_ragged,
 *    avse_resampler_create, avse_resampler_push_each, avse_resampler_reset_each, avse_resampler_state,
 *    avse_resampler_destroy, avse_retime_supported, avse_retime_counts, avse_retime_ragged, avse_retimer_create,
 *    avse_retimer_push_each, avse_retimer_reset_each, avse_retimer_state, avse_retimer_destroy, avse_forward_mixed,
 *    avse_forward_mixed_checked, avse_stream_push_each_mixed, avse_stream_blank, avse_slide_supported,
 *    avse_slide_create, avse_slide_counts, avse_slide_counts_geom, avse_slide_push_each, avse_slide_reset_each,
 *    avse_slide_reset, avse_slide_state, avse_slide_destroy, avse_slide_windows, avse_slide_video_windows,
 *    avse_slide_keep (K22's three entry points too stay under version 3, as every addition before them: they are new
 *    symbols, nothing existing changed, and the host tests of each earlier addition pin avse_abi_version() == 3; a
 *    binding that needs them asks for the symbols) */
#define AVSE_ABI_VERSION 3

enum avse_status {
    AVSE_OK = 0,
    AVSE_ERR_INVALID = 1,      /* bad argument / shape                                  */
    AVSE_ERR_HIP = 2,          /* HIP runtime error (message in avse_last_error)       */
    AVSE_ERR_UNSUPPORTED = 3,  /* configuration outside what the kernels implement      */
    AVSE_ERR_OOM = 4,          /* device allocation failed                             */
    AVSE_ERR_CHECK = 5,        /* checked build only: a device-side protocol / bounds check fired */
    AVSE_ERR_RANGE = 6         /* avse_forward_checked(AVSE_RANGE_ERROR): a split-f16 activation left the f16 range */
};

/* Compute dtypes of avse_weights_load (inputs, outputs and accumulation are float32 in all three):
 *   AVSE_F32        every layer on exact-fp32 MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain)
 *   AVSE_BF16       activations and weights rounded to bf16 (the fast path; ~2e-3 relative output error)
 *   AVSE_F32_SPLIT  float32 accuracy on the 16-bit matrix cores: every layer carries each fp32 operand as an f16 pair
 *                   x = h + l (h = f16(x), l = f16(x - h); weights scaled per output channel by a power of two) and
 *                   forms the products with v_mfma_f32_16x16x32_f16, each MFMA rounding its 32 exact products once
 *                   into the fp32 accumulator (a K = 3200 dot product: more accurate than exact-fp32 MFMA,
 *                   tools/split_probe.hip): h h, l h, h l in the video convolutions v_conv1..v_conv5, in k_gemm's
 *                   layers (v_conv6, the dense layers) and in the fused decoder tail (l l, 2^-22 of |a b|, dropped;
 *                   option four_products keeps it in the latter two), all four in the remaining layers.  Activations pass between layers as the pairs
 *                   (about 22 significant bits; the float32 network inputs are split on load, the decoder's last
 *                   output is float32): whole-network error measured 1.3x AVSE_F32's (6.8e-5 vs
 *                   5.1e-5 absolute RMS on dB-scale outputs, tests/test_gpu_split.py), inside the north star's 1e-4.
 *                   Range: a pair holds |x| < 65520 (f16 overflow) at ~22 bits from 2^-3 up.  Each layer stores the
 *                   pairs of x 2^e_L with a power-of-two exponent e_L from its BatchNormalization parameters (0 for
 *                   layers whose |beta| + |gamma| lies in [2^-2, 2^8]; avse_weights_act_exponents), and every kernel
 *                   that stores a pair (or splits an fp32 input) reports a value outside the range into a range guard:
 *                   avse_forward_checked recomputes such a batch on the exact-fp32 kernels (or fails with
 *                   AVSE_ERR_RANGE); after plain avse_forward calls avse_range_status tells whether any did. */
enum avse_dtype { AVSE_F32 = 0, AVSE_BF16 = 1, AVSE_F32_SPLIT = 2 };
enum avse_pad_mode { AVSE_PAD_REFLECT = 0, AVSE_PAD_CONSTANT = 1 };
/* Element type of a video argument of the avse_*_video entry points: float32, or the mouth crops' own 8-bit grayscale
 * values [N][128][128][F] uint8 (a quarter of the bytes to store and upload).  float(uint8) is exact and every kernel
 * converts on load, so a uint8 call returns the bits of the float32 call on the same pixel values.  A uint8 video
 * pointer must be 4-byte aligned (the loaders read whole dwords; every clip of H W F bytes is then aligned too):
 * AVSE_ERR_INVALID otherwise. */
enum avse_video_dtype { AVSE_VIDEO_F32 = 0, AVSE_VIDEO_U8 = 1 };

typedef struct avse_ctx avse_ctx;
typedef struct avse_weights avse_weights;

/* ---- library / context ----------------------------------------------------------------- */

int avse_abi_version(void);
const char* avse_last_error(void);

/* One context per device: owns the DFT twiddle / window / mel tables and the forward scratch. */
int avse_ctx_create(int device, avse_ctx** out);
void avse_ctx_destroy(avse_ctx* ctx);

/* Kernel-path switches of a context, by name (A/B experiments and layer-by-layer parity tests; the
 * defaults are the production path).  Each is initialised at avse_ctx_create from an AVSE_*
 * environment variable and never re-read afterwards:
 *   no_gemm (AVSE_NO_GEMM)           v_conv6 + dense layers on k_conv + split-K reduce, not k_gemm
 *   no_audenc (AVSE_NO_AUDENC)       audio encoder layer by layer, not the fused k_aud_enc
 *   no_dechead / no_dectail          decoder head (d_deconv1..3) / tail (d_deconv4..6) layer by layer
 *   unfused_tail (AVSE_UNFUSED_TAIL) d_deconv6 as its own kernel (d_deconv5 activation materialised)
 *   no_halo (AVSE_NO_HALO)           video convs on k_conv (applies to weights loaded afterwards)
 *   mfma32 (AVSE_MFMA32)             32x32x16 compute waves in the stream convolutions
 *   serial (AVSE_SERIAL)             the per-layer audio branch on the caller's stream (not the side stream)
 *   graph (AVSE_GRAPH)               avse_forward replays a hipGraph per argument set
 *   gemm_ksplit_cap (AVSE_GEMM_KSPLIT) cap on k_gemm's split-K factor (0 = none)
 *   dense_istft (AVSE_DENSE_ISTFT)   avse_istft through the dense pinv + frame scratch + overlap-add pass
 *   no_act_scale (AVSE_NO_ACT_SCALE) AVSE_F32_SPLIT weights loaded afterwards keep every activation exponent 0
 *   no_win (AVSE_NO_WIN)             AVSE_F32_SPLIT stride-1 gather layers (decoder phases, a_conv2) on the generic
 *                                    k_conv instead of the windowed kernel
 *   no_v1p (AVSE_NO_V1P)             AVSE_F32_SPLIT 5-frame v_conv1 on k_conv_v1s (K 160) instead of k_conv_v1p
 *                                    (K 128; applies to weights loaded afterwards)
 *   no_a1valu (AVSE_NO_A1VALU)       AVSE_F32_SPLIT a_conv1 on audio_prep + k_conv instead of k_aconv1_split
 *   no_planar (AVSE_NO_PLANAR)       AVSE_F32_SPLIT stream convolutions on the slice-by-slice [Ah | Al] grouping with
 *                                    lane swaps instead of the planar slice-pair grouping
 *   four_products (AVSE_FOUR_PRODUCTS) AVSE_F32_SPLIT k_gemm (v_conv6, the dense layers) and the fused decoder tail slab
 *                                    by slab with all four products of (Ah + Al)(Wh + Wl) instead of three-product
 *                                    planar slab pairs
 *   side_prio (AVSE_SIDE_PRIO)       audio side stream priority: 0 default, 1 least, 2 greatest (set before the
 *                                    context's first concurrent forward)
 * Unknown names return AVSE_ERR_INVALID. */
int avse_ctx_set_option(avse_ctx* ctx, const char* name, int value);
int avse_ctx_get_option(avse_ctx* ctx, const char* name, int* value);

/* Pre-size the forward scratch for up to max_clips clips of the 25-fps network so that later avse_forward calls
 * never allocate (required before capturing avse_forward into a hipGraph). */
int avse_ctx_reserve(avse_ctx* ctx, int64_t max_clips, int compute_dtype);
/* The same for the network shape and compute dtype `weights` were loaded for (avse_weights_load_shape: e.g. the
 * 29.97 / 30-fps networks need a larger scratch).  avse_forward fails with AVSE_ERR_INVALID, instead of growing the
 * scratch, while its stream is being captured. */
int avse_ctx_reserve_weights(avse_ctx* ctx, const avse_weights* weights, int64_t max_clips);

/* ---- audio front end ------------------------------------------------------------------- */

/* Replaces signal_to_spectrogram(audio_signal, n_fft, hop_length, mel=True, db=True)
 * (data_processor.py:77-96): librosa.core.stft (:79, periodic Hann, centred, pad_mode) ->
 * magphase (:80) -> librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) (Slaney) np.dot (:83-91)
 * -> librosa.amplitude_to_db(ref=1, amin, top_db) (:94), the top_db clamp taken over each
 * utterance's WHOLE [n_mels, T] array, and — when frames_per_slice > 0 — the slicing of
 * preprocess_audio_signal (data_processor.py:49-57) fused into the store.
 *
 *   sig      [n_utt][n_samples]                  channel-0 samples (already padded/truncated)
 *   T        = 1 + n_samples / hop               (centred frames)
 *   mel_db   frames_per_slice == 0: [n_utt][n_mels][T]
 *            frames_per_slice  > 0: [n_utt][n_slices][n_mels][frames_per_slice],
 *                                   n_slices = T / frames_per_slice (trailing frames dropped
 *                                   from the output but still inside the top_db max)
 *   stft_ri  nullable; [n_utt][n_fft/2+1][T][2]  complex STFT (re, im), librosa layout
 *
 * n_fft == 640 runs the mixed-radix (16 x 20) FFT kernel; other n_fft <= 2048 (e.g. 533 at
 * 29.97 fps, data_processor.py:44) run a direct-DFT kernel. */
int avse_spectrogram(avse_ctx* ctx, const float* sig, int64_t n_utt, int64_t n_samples,
                     int sr, int n_fft, int hop, int n_mels, float fmin, float fmax,
                     float amin, float top_db, int pad_mode, int frames_per_slice,
                     float* mel_db, float* stft_ri, void* stream);

/* Replaces reconstruct_signal_from_spectrogram (data_processor.py:99-116) as called by
 * reconstruct_speech_signal (:60-74): db_to_amplitude (:101) -> np.dot(pinv(mel), .) (:112) ->
 * x exp(i angle D) of the mixture STFT -> librosa.istft(hop_length=hop) (:114: periodic Hann,
 * window-sum-square normalisation, n_fft/2 trimmed at both ends).
 *   mel_db   frames_per_slice > 0: [n_utt][n_frames/frames_per_slice][n_mels][frames_per_slice]
 *            (the network's [N][80][20] output of consecutive slices = np.concatenate(..., axis=1))
 *            frames_per_slice == 0: [n_utt][n_mels][n_frames]
 *   stft_ri  [n_utt][n_fft/2+1][stft_frames][2] complex STFT of the mixture (avse_spectrogram's
 *            stft_ri output); the first n_frames frames are used (min(T_pred, T_phase), :68-70)
 *   sig      [n_utt][hop * (n_frames - 1)]
 * n_fft is the ANALYSIS size (int(sr / fps)); the inverse size is 2 * (n_fft/2), like librosa. */
int avse_istft(avse_ctx* ctx, const float* mel_db, const float* stft_ri, int64_t n_utt, int n_frames,
               int stft_frames, int frames_per_slice, int sr, int n_fft, int hop, int n_mels,
               float fmin, float fmax, float* sig, void* stream);

/* avse_spectrogram for a RAGGED batch: n_utt utterances of n_utt lengths in one call.  Replaces the same
 * signal_to_spectrogram / preprocess_audio_signal code (data_processor.py:49-57, 77-96) as it runs once per
 * utterance: every utterance has its own reflect / zero padding, its own trailing frames and its own top_db
 * floor (the maximum over its own WHOLE [n_mels, T_u] array), exactly as if it were passed to avse_spectrogram
 * alone — the results are the same bits.
 *
 *   sig_off    HOST [n_utt] int64   element offset of utterance u's first sample from `sig`; any offset, odd ones
 *                                   included: tightly packed utterances and the rows of a [n_utt][stride] buffer
 *                                   (avse_mix_pairs' rows) are both expressible
 *   n_samples  HOST [n_utt] int64   its length; T_u = the centred frame count of avse_spectrogram for that length
 *                                   (1 + n_samples[u] / hop for an even n_fft)
 *   mel_db     frames_per_slice == 0: per utterance [n_mels][T_u], concatenated in utterance order
 *              frames_per_slice  > 0: [sum_u S_u][n_mels][frames_per_slice], S_u = T_u / frames_per_slice; an
 *                                   utterance's slices are consecutive, so the buffer is avse_forward's audio input
 *                                   as it stands.  S_u == 0 is legal: that utterance writes no mel (its complex STFT
 *                                   is still written) and takes part in no other utterance's top_db
 *   stft_ri    nullable; per utterance [n_fft/2+1][T_u][2], concatenated
 *
 * A batch whose lengths are all equal has exactly avse_spectrogram's layout; where its utterances also start
 * n_samples apart, the call IS avse_spectrogram's launch.  Otherwise n_fft 640 and 533 run ragged instantiations of
 * their kernels (one block per (utterance, chunk of frames) from an item table built on the host), followed by the
 * per-utterance clamp pass; other n_fft walk the maximal runs of consecutive equal-length, evenly spaced utterances
 * through the equal-length kernels.  The item table is uploaded into context scratch, which grows outside a stream
 * capture only (like avse_mix_pairs' scratch); a captured call reads the table from context-owned host memory when
 * the graph runs, so replay it before the next ragged call on this context.
 *
 * Refused with AVSE_ERR_INVALID before any GPU work: a NULL ctx / sig / sig_off / n_samples / mel_db, n_utt < 0, an
 * n_samples[u] < 1, reflect padding on an utterance of at most n_fft/2 samples, a negative frames_per_slice, and a
 * batch too large (an utterance of 2^31 samples or more, or more than 2^31 - 1 (utterance, chunk) items). */
int avse_spectrogram_ragged(avse_ctx* ctx, const float* sig, const int64_t* sig_off, const int64_t* n_samples,
                            int64_t n_utt, int sr, int n_fft, int hop, int n_mels, float fmin, float fmax,
                            float amin, float top_db, int pad_mode, int frames_per_slice, float* mel_db,
                            float* stft_ri /* nullable */, void* stream);

/* avse_istft for a RAGGED batch: replaces reconstruct_signal_from_spectrogram / reconstruct_speech_signal
 * (data_processor.py:60-74, 99-116) as they run once per utterance.  Every utterance has its own last frame, and so
 * its own window-sum edges; utterance u's samples are the bits avse_istft gives for it alone.
 *
 *   n_frames     HOST [n_utt] int64  frames reconstructed for utterance u (the first n_frames[u] of its STFT)
 *   stft_frames  HOST [n_utt] int64  frames its mixture STFT holds
 *   mel_db   frames_per_slice > 0: [sum_u n_frames[u] / frames_per_slice][n_mels][frames_per_slice] (avse_forward's
 *            output for the concatenated slices, as it stands); == 0: per utterance [n_mels][n_frames[u]], concatenated
 *   stft_ri  per utterance [n_fft/2+1][stft_frames[u]][2], concatenated (avse_spectrogram_ragged's stft_ri)
 *   sig      per utterance hop * (n_frames[u] - 1) samples, concatenated; nothing for n_frames[u] < 2
 *
 * Equal lengths: avse_istft's layout and its launch.  Otherwise n_fft 640 / hop 160 / 80 bands run the ragged
 * instantiation of the fused kernel (its prefetch reads the next item's utterance through buffer resources bounded
 * by that utterance's own blocks); every other shape walks the runs of equal (n_frames, stft_frames) through the
 * equal-length kernels.  Scratch and stream capture: as avse_spectrogram_ragged.
 *
 * Refused with AVSE_ERR_INVALID before any GPU work: a NULL ctx / mel_db / stft_ri / n_frames / stft_frames / sig,
 * n_utt < 0, a negative n_frames[u] or stft_frames[u], an n_frames[u] that is no multiple of a positive
 * frames_per_slice, n_frames[u] > stft_frames[u], a negative frames_per_slice, and a batch too large (an utterance
 * whose STFT or mel block passes 2 GiB, or more than 2^31 - 1 items). */
int avse_istft_ragged(avse_ctx* ctx, const float* mel_db, const float* stft_ri, const int64_t* n_frames,
                      const int64_t* stft_frames, int64_t n_utt, int frames_per_slice, int sr, int n_fft, int hop,
                      int n_mels, float fmin, float fmax, float* sig, void* stream);

/* ---- network --------------------------------------------------------------------------- */

/* Number of float32 values in a canonical weight blob (see avse_weights_load): the 25-fps network
 * (build((80, 20), (128, 128, 5))). */
int64_t avse_weights_blob_floats(void);

/* The same for the network SpeechEnhancementNetwork.build((80, spec_frames), (128, 128, video_frames)) builds
 * (network.py:17-40; data_processor.py:44-52: spec_frames = int(slice samples / hop) = 20 at 25 fps, 24 at
 * 29.97 / 30 fps; video_frames = int(0.2 * fps) = 5 at 25 / 29.97 fps, 6 at 30 fps).  The shapes set the audio
 * embedding (5 x ceil(spec_frames / 4) x 128), the concat width (+ 2048) and the dense widths (concat / 4,
 * network.py:55).  -1 for shapes the kernels do not implement (spec_frames not a multiple of 4 — the decoder
 * would not reproduce 80 x spec_frames — or video_frames outside 1..8). */
int64_t avse_weights_blob_floats_shape(int spec_frames, int video_frames);

/* Replaces SpeechEnhancementNetwork.load (network.py:222-226) for the build's own weight format.
 * host_blob: the Keras-layout tensors of network.py's layers in creation order (float32):
 *   for each conv / dense / transposed-conv layer: kernel, bias
 *     conv (kh, kw, cin, cout); transposed conv (kh, kw, cout, cin); dense (in, out)
 *   followed, when the layer has a BatchNormalization, by gamma, beta, moving_mean,
 *   moving_variance.
 *   order: a_conv1..5, v_conv1..6, enc_dense, dec_dense1, dec_dense2, d_deconv1..6
 *   (d_deconv6 has no BatchNormalization).
 * BN (eps 1e-3) is folded into per-channel scale/shift; kernels are repacked for the implicit
 * GEMM and uploaded in compute_dtype (avse_dtype).  Synchronous. */
int avse_weights_load(avse_ctx* ctx, const float* host_blob, int64_t n_floats, int compute_dtype,
                      avse_weights** out);
/* avse_weights_load for the network of build((80, spec_frames), (128, 128, video_frames)); the weights remember
 * the shape, and avse_forward then takes audio [N][80][spec_frames] and video [N][128][128][video_frames].
 * The fused per-clip kernels cover the 25-fps shape (and v_conv1's 5-frame kernel every 5-frame shape); other
 * shapes run the generic implicit-GEMM path.  AVSE_ERR_UNSUPPORTED as avse_weights_blob_floats_shape's -1. */
int avse_weights_load_shape(avse_ctx* ctx, const float* host_blob, int64_t n_floats, int compute_dtype,
                            int spec_frames, int video_frames, avse_weights** out);
/* The shape the weights were loaded for. */
int avse_weights_shape(const avse_weights* w, int* spec_frames, int* video_frames);
void avse_weights_destroy(avse_weights* w);

/* Replaces SpeechEnhancementNetwork.predict's Model.predict (network.py:208-212) and the
 * VideoNormalizer.normalize it is preceded by (data_processor.py:208-212,
 * speech_enhancer.py:74), fused:
 *   audio      [N][80][20]        mixed mel-dB spectrograms (the expand_dims(-1) is implicit);
 *                                 [N][80][T] for weights loaded with avse_weights_load_shape(T, F)
 *   video      [N][128][128][5]   mouth crops ([N][128][128][F]), NOT normalised; NULL = an all-zero video input (the audio
 *                                 branch alone, BASELINE configs[2]: the video encoder's output is then one
 *                                 constant vector, computed once per weights object and broadcast;
 *                                 vnorm_* must be NULL)
 *   vnorm_mean [128][128]         nullable: VideoNormalizer mean image (applied in-kernel)
 *   vnorm_std  [128][128]         nullable: VideoNormalizer std image
 *   out        [N][80][20]        predicted speech mel-dB spectrograms (float32; [N][80][T])
 * Computes in the weights' compute dtype, accumulating in float32. */
int avse_forward(avse_ctx* ctx, const avse_weights* w, const float* audio, const float* video,
                 const float* vnorm_mean, const float* vnorm_std, int64_t N, float* out,
                 void* stream);

/* avse_forward (replaces the same reference calls) with the video in video_dtype (avse_video_dtype): video
 * [N][128][128][F] float32 or uint8, NULL as avse_forward for either dtype.  AVSE_VIDEO_F32 is avse_forward itself. */
int avse_forward_video(avse_ctx* ctx, const avse_weights* w, const float* audio, const void* video, int video_dtype,
                       const float* vnorm_mean, const float* vnorm_std, int64_t N, float* out, void* stream);

/* avse_forward for AVSE_F32_SPLIT weights with the range guard read back: waits for `stream` after the forward (not
 * capturable) and, when a stored activation or a split input left the f16 pair range (|x| >= 65520 or NaN; bit i of
 * *host_bits = plan layer i, a_conv1 = 0 .. d_deconv5 = 18; bit 24 the audio input, bit 25 the video input):
 *   mode AVSE_RANGE_RECOMPUTE  recomputes the whole batch on the exact-fp32 kernels (the AVSE_F32 path of the same
 *                              network, built once per weights object from the blob they were loaded from) into `out`
 *                              and returns AVSE_OK — the outputs are then the AVSE_F32 forward's;
 *   mode AVSE_RANGE_ERROR      returns AVSE_ERR_RANGE (outputs not float32-accurate).
 * host_bits (nullable) receives the bits (0: every pair was in range).  Other dtypes: avse_forward, *host_bits = 0. */
enum avse_range_mode { AVSE_RANGE_RECOMPUTE = 0, AVSE_RANGE_ERROR = 1 };
int avse_forward_checked(avse_ctx* ctx, const avse_weights* w, const float* audio, const float* video,
                         const float* vnorm_mean, const float* vnorm_std, int64_t N, float* out, void* stream,
                         int mode, uint32_t* host_bits);

/* avse_forward_checked (the checked form of the reference's Model.predict, network.py:208-212) with the video in
 * video_dtype; the exact-fp32 recompute reads the same uint8 input, and bit 25 reports what the float32 call reports
 * for the same pixel values. */
int avse_forward_checked_video(avse_ctx* ctx, const avse_weights* w, const float* audio, const void* video,
                               int video_dtype, const float* vnorm_mean, const float* vnorm_std, int64_t N, float* out,
                               void* stream, int mode, uint32_t* host_bits);

/* avse_forward_video for a batch in which some clips have no video (camera off, mouth lost, packets late):
 *   present    HOST [N]           non-zero: the clip has video
 *   video      [M][128][128][F]   PACKED: only the M = count(present) clips with video, in clip order, in video_dtype;
 *                                 may be NULL when M == 0
 *   vnorm_*                       apply to the clips with video; allowed (and unused) when M == 0
 * A clip without video is the all-zero NORMALISED input, i.e. the video == NULL input of avse_forward (with a
 * normaliser: the mean image): its embedding is the constant vector of the weights object.  The video encoder runs
 * over the M packed clips only and one kernel fills every concat row from its clip's embedding or the constant one.
 * With AVSE_F32 and AVSE_F32_SPLIT weights, whose forwards are batch-invariant, out[i] has the bits of the call the
 * clip would have had alone: avse_forward_video(video) where present, avse_forward_video(NULL) where not.  The network
 * was not trained with missing video: the quality of its audio-only estimate is unmeasured.
 * M == N enqueues exactly avse_forward_video's launches, M == 0 exactly those of video == NULL.  Otherwise the call is
 * asynchronous but NOT capturable (the row map goes up from pinned host memory), and option graph does not replay it.
 * avse_ctx_reserve / avse_ctx_reserve_weights size the scratch of the plain calls only: the first mixed call of a given
 * (N, M) may still grow it once (for the packed embeddings, the row map and the M-clip split-K partials).
 * AVSE_ERR_INVALID before any GPU work: present == NULL, video == NULL with M > 0, and avse_forward_video's rules. */
int avse_forward_mixed(avse_ctx* ctx, const avse_weights* w, const float* audio, const void* video, int video_dtype,
                       const float* vnorm_mean, const float* vnorm_std, const uint8_t* present, int64_t N, float* out,
                       void* stream);

/* avse_forward_checked_video with avse_forward_mixed's `present` and packed video; the exact-fp32 recompute takes the
 * same mask and video, and the constant embedding's range bits count whenever a clip without video is in the batch. */
int avse_forward_mixed_checked(avse_ctx* ctx, const avse_weights* w, const float* audio, const void* video,
                               int video_dtype, const float* vnorm_mean, const float* vnorm_std, const uint8_t* present,
                               int64_t N, float* out, void* stream, int mode, uint32_t* host_bits);

/* Range-guard bits (as avse_forward_checked's) raised by the AVSE_F32_SPLIT forwards of plain avse_forward /
 * avse_forward_profile calls on this context since the last avse_range_status; waits for `stream` (the stream those
 * forwards ran on) and clears them. */
int avse_range_status(avse_ctx* ctx, void* stream, uint32_t* host_bits);

/* Stream-ordered, non-blocking form of avse_range_status for pipelines (verify batch k while batch k + 1 runs): enqueues
 * on `stream` a copy of the guard bits raised so far into *host_word (pinned host memory, e.g. hipHostMalloc; valid
 * once the stream has reached this point: record an event after the call and wait for it) and a reset of the guard, so
 * the bits of the forwards enqueued between two snapshots land in the later one.
 *
 * Contract of the three guard readers: the guard words belong to the context.  Unchecked forwards of one context on
 * several streams (or threads) OR into the same word, and avse_forward_checked uses one word per context, so per-batch
 * attribution holds only while ONE stream at a time drives the context; concurrent pipelines each create their own
 * context (they may share the read-only avse_weights). */
int avse_range_snapshot(avse_ctx* ctx, void* stream, uint32_t* host_word);

/* AVSE_F32_SPLIT: the activation exponent e_L of each plan layer (host_exp[0..n), n <= 20; layer L stores the pairs of
 * x 2^e_L); 0 for every layer of the other dtypes. */
int avse_weights_act_exponents(const avse_weights* w, int* host_exp, int n);

/* Stages of the forward pass, in launch order (avse_forward_profile). */
#define AVSE_NUM_STAGES 22
/*  0 video prep (normalise + cast)   1 audio prep      2-6 a_conv1..a_conv5
 *  7-12 v_conv1..v_conv6              13 enc_dense  14 dec_dense1  15 dec_dense2
 *  16-20 d_deconv1..d_deconv5         21 d_deconv6 (1x1 -> float32 output)            */

/* avse_forward with a HIP event recorded between consecutive kernel launches; synchronises the
 * stream and writes each stage's elapsed milliseconds to host_ms[AVSE_NUM_STAGES]. */
int avse_forward_profile(avse_ctx* ctx, const avse_weights* w, const float* audio, const float* video,
                         const float* vnorm_mean, const float* vnorm_std, int64_t N, float* out,
                         void* stream, float* host_ms);

/* avse_forward_profile (the reference's Model.predict, network.py:208-212, timed per stage) with the video in
 * video_dtype. */
int avse_forward_profile_video(avse_ctx* ctx, const avse_weights* w, const float* audio, const void* video,
                               int video_dtype, const float* vnorm_mean, const float* vnorm_std, int64_t N, float* out,
                               void* stream, float* host_ms);

/* ---- streaming enhancement ---------------------------------------------------------------- */

/* A session enhances n_streams lock-step streams (e.g. the participants of one call) as their audio and video arrive.
 * The calls below replace the per-sample predict path of the reference as it would run incrementally
 * (speech_enhancer.py:70-85: preprocess_audio_signal, data_processor.py:35-57 -> VideoNormalizer.normalize + Model.predict
 * -> reconstruct_speech_signal, data_processor.py:60-74, over signal_to_spectrogram / reconstruct_signal_from_spectrogram,
 * :77-116), which needs the whole utterance: the reflect padding of both ends, the top_db floor from the utterance's
 * maximum, the window sum of the finished signal.  A session carries the sample tail, the running floor, the mixture
 * phase of frames awaiting their prediction and the overlap-add tail between calls instead.
 *
 * Geometry and dB parameters are avse_spectrogram's / avse_istft's, video_dtype avse_forward_video's; a slice is
 * frames_per_slice * hop samples, and `weights` must have been loaded for frames_per_slice spectrogram frames
 * (AVSE_ERR_INVALID otherwise).  A geometry streams when its slices do not drift against the samples: n_fft even and
 * n_fft == 4 * hop, else AVSE_ERR_UNSUPPORTED (29.97 fps at every rate, and 30 fps at 16 kHz: n_fft 533, and
 * 24 x 133 = 3192 samples per 3200-sample slice; int(48000 / 29.97) = 1601 is odd).  Built: the reference's 25-fps
 * geometries (n_fft = sr / 25, data_processor.py:44) at 16, 32 and 48 kHz, i.e. n_fft 640 / hop 160, n_fft 1280 / hop 320
 * at sr 32000 and n_fft 1920 / hop 480 at sr 48000, with 80 bands and a Slaney bank whose bands fit 24 bins and lie in
 * bins 0 .. 320 (fmin 0, fmax 8000: at every one of these rates the bins are 25 Hz apart and the bank is the 16 kHz
 * bank, so the longer frames are computed as 2 or 3 interleaved 640-point frames); and its 30-fps geometries
 * (n_fft = sr / 30) at 24 and 48 kHz, i.e. n_fft 800 / hop 200 at sr 24000 and n_fft 1600 / hop 400 at sr 48000, with
 * 80 bands and a bank that lies in bins 0 .. 266 (fmin 0, fmax 8000: the bins are 30 Hz apart at both rates and the
 * banks are equal, so the 1600-sample frame is two interleaved 800-point frames); a frame length belongs to its rate
 * (800 / 200 at 16 kHz is refused).  Any frames_per_slice the weights have (20 at 25 fps, 24 at 30 fps, where the
 * weights are those of the [80, 24] x 6-frame network), up to 1024 streams and max_slices 16.  Other geometries that
 * pass the condition are AVSE_ERR_UNSUPPORTED too (44.1 kHz: n_fft 1764; fmax 24000 at 48 kHz);
 * avse_stream_supported is the rule.
 * max_slices: the most slices one call may complete, and the most either input may run ahead of the other.  All device
 * state and scratch is sized from n_streams and max_slices here (the forward scratch through
 * avse_ctx_reserve_weights(ctx, weights, n_streams * max_slices)); create synchronises, a push or a flush allocates
 * nothing and never synchronises, and the host reads nothing back: the session's counters are functions of the call
 * arguments alone (avse_stream_counts).  `weights` and `ctx` must outlive the session.
 * Sessions of one context are independent of each other (each owns its tables and state) and follow the context's
 * one-stream-at-a-time rule.  With AVSE_F32_SPLIT weights the pushes run the unchecked forward: the range-guard bits
 * accumulate in the context, and avse_range_status / avse_range_snapshot read them as for avse_forward. */
typedef struct avse_stream avse_stream;
/* Host-only, no GPU work: 0 when avse_stream_create serves this geometry and bank, else the status it would return for
 * them (AVSE_ERR_INVALID: non-positive values; AVSE_ERR_UNSUPPORTED: see above) with the reason in avse_last_error.
 * avse_stream_create calls it; the limits on n_streams / max_slices and the weights' shape are checked there. */
int avse_stream_supported(int sr, int n_fft, int hop, int frames_per_slice, int n_mels, float fmin, float fmax);
int avse_stream_create(avse_ctx* ctx, const avse_weights* weights, int64_t n_streams, int sr, int n_fft, int hop,
                       int frames_per_slice, int n_mels, float fmin, float fmax, float amin, float top_db,
                       int video_dtype, int64_t max_slices, avse_stream** out);

/* Host-only: the totals of a stream that has received n_samples samples and n_video_slices video slices (flushed != 0:
 * after its flush, which needs n_samples <= slice * n_video_slices): frames analysed, slices through the network,
 * samples emitted.  Any of the three outputs may be NULL.  A NULL session means the 640 / 160 / 20 geometry. */
int avse_stream_counts(const avse_stream* s, int64_t n_samples, int64_t n_video_slices, int flushed, int64_t* frames,
                       int64_t* slices, int64_t* emitted);

/* Feeds every stream n_new samples and v_new video slices (either may be 0; both 0 is a no-op) and appends to `out`
 * the samples that became final.  With N = n_fft, H = hop, spf = frames_per_slice, after n samples and v slices in total:
 *  - frame t is the offline frame t (window x[H t - N/2, H t + N/2), left reflection x[-i] = x[i]); it is computed as
 *    soon as every sample it reads has arrived (n >= H t + N/2; n >= N/2 + 1 for t = 0), never again, and its complex
 *    STFT is kept until its slice has been inverted;
 *  - slice k is frames [spf k, spf k + spf); it runs through the network once its frames and its video slice are both
 *    there: k_done = min(frames_done / spf, v);
 *  - the network sees slice k clamped from below at (the maximum of the unclamped mel-dB of frames 0 .. spf k + spf - 1
 *    of that stream) - top_db: the causal form of amplitude_to_db's whole-array maximum (data_processor.py:94); amin as
 *    offline, top_db < 0 disables the clamp.  It depends on nothing after the slice, so not on how the input was cut
 *    into calls; a stream on which the floor never binds (unclamped range below top_db) gives, in exact arithmetic,
 *    the offline result;
 *  - output sample i is final once every frame covering it is inverted; it is y[i] of librosa.istft over the frames so
 *    far (frames added in increasing order, each sample over the window sum-square of the frames that cover it), so a
 *    stream has emitted max(0, spf H k_done - N/2) samples: N/2 + H samples (30 ms at every built rate: 480 at 16 kHz)
 *    of latency beyond the slice.
 *   samples   [n_streams][n_new] at row stride sample_stride (>= n_new); NULL when n_new == 0
 *   video     [n_streams][v_new][128][128][F] in the session's video_dtype (4-byte aligned); NULL when v_new == 0
 *   vnorm_*   nullable, as avse_forward
 *   out       [n_streams][out_stride]: row b receives *host_n_out new samples of stream b; NULL only when nothing is emitted.
 *             A push emits at most spf H max_slices samples in the session's H (3200 max_slices at 16 kHz, 6400 at 32,
 *             9600 at 48), so an out_stride of that many always serves
 *   host_n_out  HOST: the samples appended per stream (the same for all)
 *   mel_db    nullable [n_streams][slices completed by this call][n_mels][spf]: what the network saw
 *   pred_db   nullable, same shape: what it predicted
 * Refused with AVSE_ERR_INVALID before any GPU work, the session left exactly as it was: NULL arguments where not
 * nullable, negative counts, sample_stride < n_new, a call that would complete more than max_slices slices or leave more
 * than max_slices slices' worth of samples or of video queued ahead of the other input, out_stride below what the call
 * emits, a push after a flush.  A failure after launches have begun marks the session broken: every later call is
 * AVSE_ERR_INVALID until avse_stream_reset. */
int avse_stream_push(avse_stream* s, const float* samples, int64_t n_new, int64_t sample_stride, const void* video,
                     int64_t v_new, const float* vnorm_mean, const float* vnorm_std, float* out, int64_t out_stride,
                     int64_t* host_n_out, float* mel_db /* nullable */, float* pred_db /* nullable */, void* stream);

/* Closes every stream as the offline call on fit_length(x, slice * v): needs n <= slice * v (AVSE_ERR_INVALID
 * otherwise); missing samples are zeros, as in preprocess_audio_signal (data_processor.py:39-42), the remaining frames
 * take the right reflection of that signal, the remaining slices run, and the rest of the slice * v - hop samples is
 * emitted (frames 0 .. spf v - 1: the offline call drops frame spf v the same way).  Arguments as avse_stream_push.
 * A flush emits at most spf H max_slices + N/2 - H samples in the session's N and H (3200 max_slices + 160 at 16 kHz,
 * 9600 max_slices + 480 at 48: max_slices pending slices plus the tail the pushes held back), more than any push: size
 * `out` for it.
 * After a flush only avse_stream_reset is legal. */
int avse_stream_flush(avse_stream* s, const float* vnorm_mean, const float* vnorm_std, float* out, int64_t out_stride,
                      int64_t* host_n_out, float* mel_db /* nullable */, float* pred_db /* nullable */, void* stream);

/* Back to the state after create (no samples, no video, not flushed, not broken), ordered on `stream`: every stream. */
int avse_stream_reset(avse_stream* s, void* stream);
void avse_stream_destroy(avse_stream* s);

/* ---- independent streams of one session ----
 * The streams of a session need not move together (callers of a service: packets of different sizes, video late by
 * different amounts, joining and hanging up at different times).  The session keeps its counters per stream (samples,
 * video slices, flushed), and every statement in avse_stream_push's comment holds for each stream with that stream's own
 * totals (n_b, v_b): frame t as soon as its samples are there, slice k at min(frames / spf, v), the causal floor over the
 * stream's own frames, emitted = max(0, spf H k_done - N/2), the flush rule n <= slice * v.  The network runs once per
 * call on the slices all streams completed together, and is batch-invariant, so each stream's output is, bit for bit,
 * that of a session of its own fed the same way.
 *
 * Per-stream form of avse_stream_push / avse_stream_flush: stream b receives n_new[b] samples and v_new[b] video
 * slices (either or both may be 0: an idle stream costs no blocks), and is closed as by avse_stream_flush when
 * flush && flush[b].
 *   samples     stream b's n_new[b] samples start at samples + sample_off[b] (floats; as avse_spectrogram_ragged's
 *               sig_off); both NULL only when every n_new is 0
 *   video       packed, stream-major: v_new[0] slices of stream 0, then v_new[1] of stream 1, ..; 4-byte aligned
 *   out         [n_streams][out_stride]: row b receives host_n_out[b] samples
 *   host_n_out  HOST [n_streams]: the samples appended per stream
 *   mel_db, pred_db   nullable, packed [sum of host_k_new][n_mels][spf], stream-major
 *   host_k_new  HOST [n_streams], nullable: the slices each stream completed in this call
 * Refused with AVSE_ERR_INVALID before any GPU work, the session left exactly as it was, with a message that names the
 * first offending stream ("stream 3: ..."), when any stream would complete more than max_slices slices, leave more than
 * max_slices slices of either input queued ahead of the other, be pushed (or flushed again) after its flush, be flushed
 * with n > slice * v, or emit more than out_stride; negative counts and NULL where not nullable as avse_stream_push.
 * A failure after launches have begun marks the session broken, as there.
 * The call allocates nothing: its per-stream rows and block tables (sized at create for the worst case) go up in one
 * copy from a ring of four pinned staging slots, and the call waits on the host only when the slot it is about to
 * overwrite has not been read yet, i.e. when four per-stream calls are still queued; otherwise it does not synchronise.
 * Not capturable into a graph.
 *
 * The lock-step calls keep their meaning: while every stream has the same counters they run exactly what they ran
 * before.  Once the counters differ, avse_stream_push is avse_stream_push_each with the same n_new / v_new for every
 * stream (samples and video as laid out for avse_stream_push), avse_stream_flush flushes every stream not yet flushed,
 * and both write the LARGEST per-stream count to *host_n_out (row b of `out` receives stream b's own count, which
 * avse_stream_state and avse_stream_counts give) and lay mel_db / pred_db out packed as above. */
int avse_stream_push_each(avse_stream* s,
        const float* samples, const int64_t* sample_off /* HOST [B] */, const int64_t* n_new /* HOST [B] */,
        const void* video, const int64_t* v_new /* HOST [B] */, const uint8_t* flush /* HOST [B], nullable */,
        const float* vnorm_mean, const float* vnorm_std,
        float* out, int64_t out_stride, int64_t* host_n_out /* HOST [B] */,
        float* mel_db /* nullable */, float* pred_db /* nullable */, int64_t* host_k_new /* HOST [B], nullable */,
        void* stream);
/* Streams with which[b] != 0 go back to the state after create (a caller left, the slot is free for the next one):
 * counters 0, not flushed, sample tail zero, running maximum -inf.  Ordered on `stream`; the other streams are
 * untouched.  Uses a staging slot as avse_stream_push_each does.  A broken session needs avse_stream_reset. */
int avse_stream_reset_each(avse_stream* s, const uint8_t* which /* HOST [B] */, void* stream);
/* HOST: per-stream totals (samples, video slices, flushed) of the session, [n_streams] each; any output nullable. */
int avse_stream_state(const avse_stream* s, int64_t* n_samples, int64_t* n_video, uint8_t* flushed);

/* avse_stream_push_each for streams whose video may be missing (camera off, mouth lost, packets late), so that such a
 * stream goes on emitting:
 *   v_present       HOST [sum v_new], stream-major, nullable (NULL: every slice has video): non-zero, the slice has video
 *   video           only the slices that have video, packed stream-major; may be NULL when there are none
 *   host_k_present  HOST [sum host_k_new], nullable: which of the slices this call completed had video
 * A slice without video ("blank") carries no bytes and counts as a video slice everywhere: in v, in the slices done,
 * in the flush rule n <= slice * v, in the max_slices queue limits and in avse_stream_counts.  It is predicted from the
 * all-zero normalised video, the input of avse_forward(video == NULL) (avse_forward_mixed says why that is exact); the
 * network was not trained with missing video, and the quality of its audio-only estimate is unmeasured.  Which queued
 * slices are blank is host state of the session, cleared by avse_stream_reset and avse_stream_reset_each.  While a blank
 * slice is queued every call of the session, the lock-step ones included, lists its video moves one by one (k_stream_move)
 * and runs avse_forward_mixed on the compacted clips; a session that never received a blank slice enqueues what
 * avse_stream_push_each enqueues, which is this call with v_present == NULL.  AVSE_ERR_INVALID with "stream b: ..."
 * and the session as it was: video == NULL while a slice is marked present, and every refusal of avse_stream_push_each
 * (a blank slice past the queue limit among them). */
int avse_stream_push_each_mixed(avse_stream* s,
        const float* samples, const int64_t* sample_off /* HOST [B] */, const int64_t* n_new /* HOST [B] */,
        const void* video, const int64_t* v_new /* HOST [B] */, const uint8_t* v_present /* HOST [sum v_new], nullable */,
        const uint8_t* flush /* HOST [B], nullable */, const float* vnorm_mean, const float* vnorm_std,
        float* out, int64_t out_stride, int64_t* host_n_out /* HOST [B] */,
        float* mel_db /* nullable */, float* pred_db /* nullable */, int64_t* host_k_new /* HOST [B], nullable */,
        uint8_t* host_k_present /* HOST [sum host_k_new], nullable */, void* stream);
/* HOST: blank slices received per stream since its last reset. */
int avse_stream_blank(const avse_stream* s, int64_t* n_blank /* HOST [B] */);

/* ---- low-latency streaming: sliding windows at a stride of `stride` video frames ----
 * A sliding session is a streaming session whose network windows start at every `stride`-th video frame, not at every
 * slice, so that beyond the first window a sample waits for one stride of video plus the synthesis tail
 * (q s H + N/2 + H samples: 70 ms at 16 kHz, 25 fps, stride 1) instead of a whole slice (230 ms).  It costs F / stride
 * times the forwards.  N = n_fft, H = hop, spf = frames_per_slice, F = the weights' video frames per slice,
 * q = spf / F, s = stride.  A stream that has received n samples and f video FRAMES (each one [128][128] crop; video does
 * not arrive as slices here) has
 *   frames    as avse_stream_push: frame t, same window and left reflection, arrives once n >= H t + N/2
 *   windows   = min(wa, wv), wa = frames >= spf ? (frames - spf) / (q s) + 1 : 0, wv = f >= F ? (f - F) / s + 1 : 0;
 *               window j is video frames [s j, s j + F) and spectrogram frames [q s j, q s j + spf)
 *   input     of window j: the unclamped mel-dB of its spf frames, clamped from below at (the maximum of the unclamped
 *               mel-dB of the stream's frames 0 .. q s j + spf - 1) - top_db (top_db < 0: no clamp): the causal floor
 *               of avse_stream_push at the window's last frame, independent of how the input was cut; its F video
 *               frames as [128][128][F], frame innermost, the normaliser fused as in avse_forward_video
 *   kept      window 0 contributes all spf predicted columns, window j > 0 its last q s (frames [q s j + spf - q s,
 *               q s j + spf)); predicted = windows > 0 ? spf + q s (windows - 1) : 0.  Keeping the newest columns is
 *               the choice latency asks for; whether centre columns would sound better has not been measured
 *   emitted   = max(0, H predicted - N/2): the mixture phase of the same frame, frames added in increasing order, each
 *               sample divided by the window sum-square of the frames covering it, as avse_stream_push
 *   flush     closes the stream as the signal zero-padded (or of length) H q f, right reflection there, frames = q f:
 *               it needs n <= H q f; the remaining windows run, emitted = predicted > 0 ? H (predicted - 1) : 0; video
 *               frames past the last full stride are dropped
 * With s = F all of this is avse_stream_push_each fed the same frames stacked into slices (v = f / F), bit for bit.
 * Host-only: avse_stream_supported's rule plus 1 <= stride <= video_frames (else AVSE_ERR_INVALID),
 * frames_per_slice % video_frames == 0 and video_frames 5 or 6 (else AVSE_ERR_UNSUPPORTED). */
typedef struct avse_slide avse_slide;
int avse_slide_supported(int sr, int n_fft, int hop, int frames_per_slice, int video_frames, int stride, int n_mels,
                         float fmin, float fmax);
/* All state and scratch is sized here (the forward's through avse_ctx_reserve_weights(ctx, weights, n_streams *
 * max_windows)); create synchronises, later calls allocate nothing.  max_windows M, 1 .. 80: the most windows one call
 * may complete per stream, and how far (in windows) either input may run ahead of the other.  video_frames is the
 * weights'. */
int avse_slide_create(avse_ctx* ctx, const avse_weights* weights, int64_t n_streams, int sr, int n_fft, int hop,
                      int frames_per_slice, int stride, int n_mels, float fmin, float fmax, float amin, float top_db,
                      int video_dtype, int64_t max_windows, avse_slide** out);
/* HOST: the totals above.  s == NULL is n_fft 640, hop 160, 20 frames and 5 video frames per slice; avse_slide_counts_geom
 * takes the geometry itself.  Outputs nullable.  AVSE_ERR_INVALID: negative counts, a stride outside 1 .. video_frames,
 * flushed with n > H q f. */
int avse_slide_counts(const avse_slide* s, int stride, int64_t n_samples, int64_t n_video_frames, int flushed,
                      int64_t* frames, int64_t* windows, int64_t* predicted, int64_t* emitted);
int avse_slide_counts_geom(int n_fft, int hop, int frames_per_slice, int video_frames, int stride, int64_t n_samples,
                           int64_t n_video_frames, int flushed, int64_t* frames, int64_t* windows, int64_t* predicted,
                           int64_t* emitted);
/* The only push.  Stream b receives n_new[b] samples (from samples + sample_off[b]) and f_new[b] video frames (packed
 * stream-major in `video`, [sum f_new][128][128] in the session's video dtype, 4-byte aligned) and is closed when flush
 * && flush[b]; lock-step use is the same counts for every stream.  out [B][out_stride] receives host_n_out[b] samples
 * per stream; mel_db / pred_db (nullable) receive, packed [sum host_w_new][n_mels][spf], the whole window the network
 * saw and predicted for every window the call completed, not only the kept columns.
 * Refused with AVSE_ERR_INVALID and "stream b: ..." naming the first offending stream, before any GPU work and with
 * the session exactly as it was: negative or too large counts; input or a flush after the stream's flush; a flush with
 * n > H q f; more than max_windows windows completed by the call; after the call, the samples completing more than
 * max_windows windows that the video does not (wa - windows > M), or the video more than the samples
 * (wv - windows > M); out NULL or out_stride below what a stream emits.  A failure after the launches have begun
 * marks the session broken (AVSE_ERR_INVALID until avse_slide_reset).  Asynchronous on `stream`; never synchronises
 * apart from the staging-slot wait of avse_stream_push_each; not capturable into a graph.  With AVSE_F32_SPLIT weights
 * the forward is the unchecked one and the guard bits accumulate in the context. */
int avse_slide_push_each(avse_slide* s, const float* samples, const int64_t* sample_off /* HOST [B] */,
                         const int64_t* n_new /* HOST [B] */, const void* video_frames,
                         const int64_t* f_new /* HOST [B] */, const uint8_t* flush /* HOST [B], nullable */,
                         const float* vnorm_mean, const float* vnorm_std, float* out, int64_t out_stride,
                         int64_t* host_n_out /* HOST [B] */, float* mel_db /* nullable */, float* pred_db /* nullable */,
                         int64_t* host_w_new /* HOST [B], nullable */, void* stream);
/* The streams with which[b] != 0 (all of them: avse_slide_reset, which also mends a broken session) go back to the
 * state after create, ordered on `stream`. */
int avse_slide_reset_each(avse_slide* s, const uint8_t* which /* HOST [B] */, void* stream);
int avse_slide_reset(avse_slide* s, void* stream);
/* HOST: per stream, samples and video frames received and whether it is flushed.  Outputs nullable. */
int avse_slide_state(const avse_slide* s, int64_t* n_samples, int64_t* n_video_frames, uint8_t* flushed);
void avse_slide_destroy(avse_slide* s);

/* ---- offline sliding enhancement: whole utterances through the windows of a flushed sliding session ----
 * What a sliding session computes for a stream that is fed and flushed, for a RAGGED batch of whole utterances at batch
 * throughput: avse_spectrogram_ragged(top_db < 0, frames_per_slice 0) -> avse_slide_windows -> avse_forward* over chunks of
 * windows, each chunk's video from avse_slide_video_windows -> avse_slide_keep -> avse_istft_ragged(frames_per_slice 0).
 * The three calls here move values and take maxima; they round nothing.  spf = frames_per_slice, F = video_frames,
 * q = spf / F, s = stride.  Utterance u has S_u = n_slices[u] slices, f = F S_u video frames, and
 *   W_u = S_u > 0 ? (f - F) / s + 1 : 0       windows: avse_slide_counts_geom(.., n_samples 0, f, flushed 1)'s
 *   P_u = W_u > 0 ? spf + q s (W_u - 1) : 0   predicted columns, likewise
 * The windows of all utterances, in utterance order, are "the window list" (sum W_u entries).  S_u == 0 is legal and
 * yields nothing.  Every count array is HOST [n_utt] int64.  All three calls are asynchronous on `stream`; their tables go
 * through context scratch, which grows outside a stream capture only, as avse_spectrogram_ragged's (and a captured call is
 * replayed before the next ragged or sliding call on the context).
 * Refused with AVSE_ERR_INVALID before any GPU work: a NULL pointer argument, n_utt < 0, a negative count, spf or F below
 * 1 or spf % F != 0, a stride outside 1 .. F, an n_frames[u] below q F S_u, a window range outside the window list, a
 * device pointer that is not 16-byte aligned, and a batch too large (n_mels times an utterance's frames, the windows of
 * the batch times 4, or an item table past 2^31 - 1).
 *
 * avse_slide_windows: the network's audio input.
 *   mel_db    per utterance [n_mels][n_frames[u]] UNCLAMPED mel-dB, concatenated: what avse_spectrogram_ragged writes
 *             with top_db < 0 and frames_per_slice 0 (n_frames[u] = q F S_u + 1 for a signal of hop q F S_u samples)
 *   net_in    [sum W_u][n_mels][spf]: window j of utterance u is its frames [q s j, q s j + spf), clamped from below at
 *             (the maximum of its frames 0 .. q s j + spf - 1) - top_db: the causal floor of avse_slide_push_each
 *             (top_db < 0: no clamp).  One block per utterance forms the prefix maximum of the frames' maxima along
 *             time in chunks of 256 frames with a carry; maxima are exact, so the bits do not depend on that shape. */
int avse_slide_windows(avse_ctx* ctx, const float* mel_db, const int64_t* n_frames, const int64_t* n_slices,
                       int64_t n_utt, int frames_per_slice, int video_frames, int stride, int n_mels, float top_db,
                       float* net_in, void* stream);
/* avse_slide_video_windows: the network's video input for windows [w0, w0 + n) of the window list, so that a forward over
 * a chunk of windows stages that chunk's video only.
 *   video     [sum S_u][128][128][F] slices, float32 or uint8 (avse_video_dtype), the utterances' slices consecutive
 *   out       [n][128][128][F] in the same dtype: out[w][y][x][i] = video[slice (s j + i) / F of the utterance][y][x]
 *             [(s j + i) % F], j the window's index within its utterance
 * F 5 and 6 are built (else AVSE_ERR_UNSUPPORTED); whole 16-byte vectors in and out for both dtypes. */
int avse_slide_video_windows(avse_ctx* ctx, const void* video, int video_dtype, const int64_t* n_slices, int64_t n_utt,
                             int video_frames, int stride, int64_t w0, int64_t n, void* out, void* stream);
/* avse_slide_keep: the kept columns of the predicted windows.
 *   pred_db   [sum W_u][n_mels][spf]: the forward's output for the window list
 *   mel_db    per utterance [n_mels][P_u], concatenated (avse_istft_ragged's frames_per_slice 0 layout, n_frames = P_u):
 *             all spf columns of window 0, then the last q s columns of each later window */
int avse_slide_keep(avse_ctx* ctx, const float* pred_db, const int64_t* n_slices, int64_t n_utt, int frames_per_slice,
                    int video_frames, int stride, int n_mels, float* mel_db, void* stream);

/* ---- resampling: any sample rate around a session ----
 * y = scipy.signal.resample_poly(x, up, down) with its defaults, up / down = (sr_out / g) / (sr_in / g),
 * g = gcd(sr_in, sr_out): the filter h of avse_eval_pairs' step 1, H = 10 max(up, down),
 *   y[k] = sum_j h[H + k down - j up] x[j] over the j in [0, n) that keep the tap index in [0, 2H],
 * ceil(n up / down) outputs for n inputs.  Equal rates are a copy of the bits.  Taps and accumulator are float64, one
 * fma per tap in ascending j (2H / up + 1 of them), the sum rounded once to float32: the value of output k is a function
 * of k and the stream's samples alone, whatever the cuts, the batch or the other streams.
 * Output k reads inputs up to floor((H + k down) / up), so after n inputs F(n) = max(0, ceil((n up - H) / down))
 * outputs are final; a flush brings the total to ceil(n up / down), with zeros past the end as the one-shot call has
 * them.  The next output needs at most the last T = 2H / up + 1 inputs (56 at 44100 -> 16000, 21 at 16000 -> 44100).
 *
 * HOST only: 0 when the pair is served, else AVSE_ERR_INVALID (a rate <= 0) or AVSE_ERR_UNSUPPORTED (max(up, down) > 640
 * after reduction, e.g. 16001 -> 16000; the reduced ratio is in avse_last_error).  8, 11.025, 12, 16, 22.05, 24, 32,
 * 44.1, 48, 88.2 and 96 kHz against 16 and 24 kHz are served in both directions. */
int avse_resample_supported(int sr_in, int sr_out);
/* HOST only: *n_out = F(n_in), or ceil(n_in up / down) when flushed.  n_in in 0 .. 2^40. */
int avse_resample_counts(int sr_in, int sr_out, int64_t n_in, int flushed, int64_t* n_out);
/* One-shot, ragged: utterance u's n_samples[u] samples at sig + sig_off[u] -> its ceil(n_samples[u] up / down) outputs
 * at out + out_off[u] (offsets in floats, HOST arrays, as avse_spectrogram_ragged takes sig_off; n_samples[u] == 0 is
 * legal and writes nothing).  The streaming kernel on a fresh state with every utterance flushed, in one launch.  The
 * rows go up through context scratch, which grows outside a stream capture only; the taps of a ratio are built at the
 * first call with it (the context keeps the last four).  Asynchronous on `stream`. */
int avse_resample_ragged(avse_ctx* ctx, const float* sig, const int64_t* sig_off, const int64_t* n_samples,
                         int64_t n_utt, int sr_in, int sr_out, float* out, const int64_t* out_off, void* stream);

typedef struct avse_resampler avse_resampler;
/* n_streams (1 .. 1024) independent streams at one rate pair.  State per stream: two copies of its last T samples
 * (a call reads one and writes the other, so one launch serves outputs and history) and the host counters. */
int avse_resampler_create(avse_ctx* ctx, int64_t n_streams, int sr_in, int sr_out, avse_resampler** out);
/* Stream b receives n_new[b] samples at samples + sample_off[b] and is closed when flush && flush[b]; row b of
 * out [n_streams][out_stride] receives the host_n_out[b] outputs that became final (the layout avse_stream_push_each
 * reads through sample_off and writes as out).  One launch for all streams, an idle stream costs no blocks.
 * Refused with AVSE_ERR_INVALID before any GPU work, the state unchanged, naming the first offending stream: a negative
 * count, a stream pushed (or flushed again) after its flush, more outputs than out_stride.
 * The call allocates nothing and does not synchronise: the rows go up from a ring of four pinned slots, and the host
 * waits only when four calls are still queued.  Not capturable into a graph. */
int avse_resampler_push_each(avse_resampler* r, const float* samples, const int64_t* sample_off /* HOST [B] */,
                             const int64_t* n_new /* HOST [B] */, const uint8_t* flush /* HOST [B], nullable */,
                             float* out, int64_t out_stride, int64_t* host_n_out /* HOST [B] */, void* stream);
/* Streams with which[b] != 0 (NULL: all) go back to the state after create.  Host counters only: a fresh stream never
 * reads its history. */
int avse_resampler_reset_each(avse_resampler* r, const uint8_t* which /* HOST [B], nullable */, void* stream);
/* HOST: per-stream totals (inputs received, outputs emitted, flushed), [n_streams] each; any output nullable. */
int avse_resampler_state(const avse_resampler* r, int64_t* n_in, int64_t* n_out, uint8_t* flushed);
void avse_resampler_destroy(avse_resampler* r);

/* ---- retiming: any video frame rate in front of a session ----
 * A rate is a rational num / den (30 fps: 30 / 1; NTSC: 30000 / 1001); p / q = fps_in / fps_out, reduced.  Output frame j
 * sits at input position j p / q: with c = j p, i0 = c div q, r = c mod q, a = A[i0], b = A[min(i0 + 1, n - 1)], per
 * pixel
 *   float32  float32((double(q - r) a + double(r) b) / double(q)): both products exact in float64, one rounding at the
 *            add, one at the divide, one to float32; r == 0 gives a's bits
 *   uint8    (2 (a (q - r) + b r) + q) div (2 q) in integers: round-half-up, exact
 * so an output frame is a function of j and the stream's frames alone, whatever the cuts, the batch or the other
 * streams.  Linear interpolation only.  Output j reads inputs up to ceil(j p / q), so after n >= 1 inputs
 * G(n) = floor((n - 1) q / p) + 1 outputs are final (G(0) = 0); a flush brings the total to ceil(n q / p), the frames
 * past G(n) being copies of the last input.  frames_per_slice (F: 5 or 6) consecutive outputs form one slice
 * [128][128][F], frame innermost: the layout of avse_stream_push_each's `video`.  G div F slices are complete; a flush
 * drops the remainder of ceil(n q / p) over F, as preprocess_video_sample does (data_processor.py:24-30).  Equal rates
 * regroup the bits into slices.
 *
 * HOST only: 0 when the pair is served, else AVSE_ERR_INVALID (a numerator or denominator outside 1 .. 2^31 - 1) or
 * AVSE_ERR_UNSUPPORTED (max(p, q) > 65536 after reduction; the reduced ratio is in avse_last_error).  30, 30000/1001, 24,
 * 15, 60 and 2997/100 fps against 25 and 30 fps are served in both directions. */
int avse_retime_supported(int64_t in_num, int64_t in_den, int64_t out_num, int64_t out_den);
/* HOST only: *out_frames = G(n_frames), or ceil(n_frames q / p) when flushed; *out_slices = that div frames_per_slice.
 * Either output may be NULL, not both.  n_frames in 0 .. 2^40. */
int avse_retime_counts(int64_t in_num, int64_t in_den, int64_t out_num, int64_t out_den, int frames_per_slice,
                       int64_t n_frames, int flushed, int64_t* out_frames, int64_t* out_slices);
/* One-shot, ragged: utterance u's n_frames[u] frames [128][128] (video_dtype, 4-byte aligned) start at frame
 * frame_off[u] of `frames`; its host_k[u] = ceil(n_frames[u] q / p) div frames_per_slice slices are written to `out`
 * packed utterance-major (out_slices_cap: the slices `out` holds; HOST arrays; n_frames[u] == 0 is legal and writes
 * nothing; host_k is written only by a call that returns 0).  The streaming kernel on a fresh state with every utterance
 * flushed, in one launch.  The rows go up through context scratch, which grows outside a stream capture only.
 * Asynchronous on `stream`. */
int avse_retime_ragged(avse_ctx* ctx, const void* frames, const int64_t* frame_off, const int64_t* n_frames,
                       int64_t n_utt, int video_dtype, int64_t in_num, int64_t in_den, int64_t out_num, int64_t out_den,
                       int frames_per_slice, void* out, int64_t out_slices_cap, int64_t* host_k, void* stream);

typedef struct avse_retimer avse_retimer;
/* n_streams (1 .. 1024) independent streams at one rate pair, slice length and dtype.  State per stream: two copies of
 * its last input frame and of the finished frames of its unfinished slice (a call reads one copy and writes the other,
 * so one launch serves slices and state), 2 x (1 + F) frames in all, and the host counters. */
int avse_retimer_create(avse_ctx* ctx, int64_t n_streams, int64_t in_num, int64_t in_den, int64_t out_num,
                        int64_t out_den, int frames_per_slice, int video_dtype, avse_retimer** out);
/* Stream b receives n_new[b] frames starting at frame frame_off[b] of `frames` (packed [n][128][128] in the retimer's
 * dtype, 4-byte aligned) and is closed when flush && flush[b]; the host_k_new[b] slices it completed are appended to
 * `out` stream-major: exactly avse_stream_push_each's packed `video`, so `out` and host_k_new feed a session with no
 * copy.  out_slices_cap: the slices `out` holds.  One launch for all streams, an idle stream costs no blocks.
 * Refused with AVSE_ERR_INVALID before any GPU work, the state unchanged, naming the first offending stream: a negative
 * count, totals past 2^40 frames, a stream pushed (or flushed again) after its flush, `out` NULL or holding fewer slices
 * than the call completes.
 * The call allocates nothing and does not synchronise: the rows go up from a ring of four pinned slots, and the host
 * waits only when four calls are still queued.  Not capturable into a graph. */
int avse_retimer_push_each(avse_retimer* r, const void* frames, const int64_t* frame_off /* HOST [B] */,
                           const int64_t* n_new /* HOST [B] */, const uint8_t* flush /* HOST [B], nullable */,
                           void* out, int64_t out_slices_cap, int64_t* host_k_new /* HOST [B] */, void* stream);
/* Streams with which[b] != 0 (NULL: all) go back to the state after create.  Host counters only: a fresh stream reads
 * neither copy of its state. */
int avse_retimer_reset_each(avse_retimer* r, const uint8_t* which /* HOST [B], nullable */, void* stream);
/* HOST: per-stream totals (frames received, slices handed out, flushed), [n_streams] each; any output nullable. */
int avse_retimer_state(const avse_retimer* r, int64_t* n_in, int64_t* n_slices, uint8_t* flushed);
void avse_retimer_destroy(avse_retimer* r);

/* VideoNormalizer.normalize (data_processor.py:208-212), in place on device (float32 only: uint8 video takes the
 * normaliser fused into the forward, vnorm_mean / vnorm_std):
 *   video[s, :, :, f] = (video[s, :, :, f] - mean) / std   for video [S][H][W][F]. */
int avse_video_normalize(avse_ctx* ctx, float* video, int64_t S, int H, int W, int F,
                         const float* mean, const float* std, void* stream);

/* ---- device-side preprocess ------------------------------------------------------------- */

/* Replaces the arithmetic of preprocess_audio_pair (data_processor.py:119-139) between reading the wav files and
 * the three signal_to_spectrogram calls, for a ragged group of pairs: the noise looped cyclically to the speech's
 * length (:124-128), AudioMixer.snr_factor and amplify_by_factor (:130-131), AudioMixer.mix (:133), and the pad /
 * truncate to the slice geometry of preprocess_audio_signal (:39-42).
 *   speech      int16 samples of n_pairs utterances, concatenated (channel 0)
 *   speech_off  [n_pairs + 1] int64 element offsets into speech (device array); utterance u is
 *               speech[speech_off[u] .. speech_off[u + 1]), n_s samples, at any element offset
 *   noise, noise_off  the same for the noises (n_n samples; n_n == 0 is silence)
 *   snr_lin     nullable (= 1.0, 0 dB); [n_pairs] float64, 10.0 ** (snr_db / 10.0) as the caller computed it
 *   L           common output length (signal_length of the slice geometry), 0 < L < 2^31
 *   rows        [3][n_pairs][L] float32: mixture, speech, scaled noise, each the round-to-nearest float32 of the
 *               float64 value; zeros from sample n_s on.  With L % 4 == 0 every row is 16-byte aligned when rows is,
 *               and avse_spectrogram takes the buffer as [3 n_pairs][L]
 *   mix64       nullable; [n_pairs][L] float64, the mixed signal itself
 *   factor      nullable; [n_pairs] float64, the noise gain
 * Numerics: the powers are exact 64-bit integer sums (deterministic; equal to numpy's float64 means while a sum stays
 * below 2^53, i.e. for n_s < 2^23 samples); factor = sqrt((S / n_s) / ((N / n_s) * snr_lin)) in float64 with every
 * operation correctly rounded, 0.0 when N == 0; noise * factor and speech + that are two separately rounded float64
 * operations (no FMA).  factor, mix64 and rows therefore equal the numpy path's bit for bit.
 * n_s == 0 is not meaningful (numpy: a mean over nothing): the caller, who built the offsets, refuses it; such a pair's
 * outputs here are zeros.  Scratch comes from the context and grows outside a stream capture only. */
int avse_mix_pairs(avse_ctx* ctx, const int16_t* speech, const int64_t* speech_off, const int16_t* noise,
                   const int64_t* noise_off, const double* snr_lin, int64_t n_pairs, int64_t L, float* rows,
                   double* mix64, double* factor, void* stream);

/* Replaces VideoNormalizer.__init__ (data_processor.py:203-206): np.mean / np.std over axes (0, 3) of
 * video [S][H][W][F] (float32, F <= 8) -> mean [H][W], std [H][W] (float32; population std).
 * One streaming read.  Per pixel, float64 sums of d and d^2 with d = x - video[0][h][w][0] (exact in float64: a
 * constant pixel gives std == 0 exactly), per chunk of slices, combined in chunk order — no floating-point atomics,
 * so two calls on one input agree bit for bit; mean = pivot + E[d], std = sqrt(max(0, E[d^2] - E[d]^2)), each rounded
 * once to float32 (within 1 float32 ulp of numpy's float64 result rounded to float32).  Scratch as avse_mix_pairs. */
int avse_video_stats(avse_ctx* ctx, const float* video, int64_t S, int H, int W, int F, float* mean, float* std,
                     void* stream);

/* avse_video_stats (replaces VideoNormalizer.__init__, data_processor.py:203-206) with the video in video_dtype.
 * AVSE_VIDEO_U8: per pixel the sums of the bytes and of their squares in 64-bit integers (exact for any S), per chunk
 * of slices, combined in chunk order; mean = Sx / n and std = sqrt((n Sx2 - Sx^2) / n^2), the numerator exact in 128
 * bits, each rounded once to float64 and once to float32 (within 1 float32 ulp of numpy's float64 result rounded to
 * float32); two calls agree bit for bit. */
int avse_video_stats_video(avse_ctx* ctx, const void* video, int video_dtype, int64_t S, int H, int W, int F,
                           float* mean, float* std, void* stream);

/* SpeechEnhancementNetwork.evaluate's loss (network.py:214-220, Keras mean_squared_error over
 * every element): *loss = mean((pred - target)^2) over n values; loss is a device float. */
int avse_mse(avse_ctx* ctx, const float* pred, const float* target, int64_t n, float* loss,
             void* stream);

/* ---- training (SpeechEnhancementNetwork.train, network.py:177-206) ---------------------- */

/* One Keras fit step of the model compiled at network.py:35-36 (Adam(lr) on mean_squared_error), in float32:
 * BatchNormalization on batch statistics (biased variance, eps 1e-3) with moving-average updates (momentum 0.99; the
 * moving variance takes the BIASED batch variance as Keras 2.0.x does — Keras >= 2.1.3 applies an n / (n - 1)
 * correction there; the reference pins only keras >= 2.0.4 (README), so which one it trained with is unpinned),
 * LeakyReLU(0.3), MaxPooling2D(2, 2), Dropout(dropout_rate) after each video pooling (the reference uses 0.25),
 * MSE over every element, Keras-2.0 Adam (beta1 0.9, beta2 0.999, epsilon 1e-8, bias-corrected step size).
 * Parameters, gradients and Adam moments are kept in the canonical blob layout of avse_weights_load. */
typedef struct avse_trainer avse_trainer;
enum avse_train_buffer { AVSE_TRAIN_PARAMS = 0, AVSE_TRAIN_GRADS = 1, AVSE_TRAIN_ADAM_M = 2, AVSE_TRAIN_ADAM_V = 3,
                         /* test aid: the first n_floats of the dz scratch (as large as the largest pre-pool layer
                          * output of a max_batch batch) */
                         AVSE_TRAIN_DEBUG_DZ = 4 };
/* AVSE_TRAIN_DEBUG_STOP | (layer << 8): test aid, end the backward pass right after layer's BN backward (its
 * dL/dz is then readable with AVSE_TRAIN_DEBUG_DZ; gradients of earlier layers are not computed).  d_deconv6 has no
 * BatchNormalization: its dz, dL/dy with the output's 8-channel stride, is copied to the dz scratch */
/* AVSE_TRAIN_DEBUG_GIN | (layer << 8): test aid, end the backward pass after layer's input gradient, copied to the
 * dz scratch */
/* AVSE_TRAIN_DEBUG_GHAT | (layer << 8): test aid, end the backward pass right after layer's activation backward
 * (LeakyReLU slope, pool routing, dropout), before its BN backward: dL/d(BN output) is then in the dz scratch at the
 * full pre-pool resolution, [N][hq][wq][C] */
enum avse_train_flags { AVSE_TRAIN_GRADS_ONLY = 1, AVSE_TRAIN_DEBUG_STOP = 2, AVSE_TRAIN_DEBUG_GIN = 4,
                        AVSE_TRAIN_DEBUG_GHAT = 8 };

/* host_blob: initial parameters (avse_weights_load layout); max_batch: largest N passed to avse_trainer_step,
 * 1..1023 (activation tensors stay below 2^31 elements). */
int avse_trainer_create(avse_ctx* ctx, const float* host_blob, int64_t n_floats, int64_t max_batch,
                        avse_trainer** out);
/* avse_trainer_create for the network of build((80, spec_frames), (128, 128, video_frames)) (see
 * avse_weights_blob_floats_shape); avse_trainer_step then takes audio / target [N][80][spec_frames] and video
 * [N][128][128][video_frames]. */
int avse_trainer_create_shape(avse_ctx* ctx, const float* host_blob, int64_t n_floats, int64_t max_batch,
                              int spec_frames, int video_frames, avse_trainer** out);
void avse_trainer_destroy(avse_trainer* t);

/* audio [N][80][20] mixed mel-dB, video [N][128][128][5] raw mouth crops (normalised in-kernel when vnorm_* are
 * given), target [N][80][20] speech mel-dB.  loss: nullable device float (the batch MSE before the update).
 * flags AVSE_TRAIN_GRADS_ONLY: forward (moving statistics updated) + backward, no Adam update.
 * The dropout mask of element e of video layer l is hash(dropout_seed, l, e) >= dropout_rate (train.hip). */
int avse_trainer_step(avse_trainer* t, const float* audio, const float* video, const float* target,
                      const float* vnorm_mean, const float* vnorm_std, int64_t N, float lr, float dropout_rate,
                      uint32_t dropout_seed, int flags, float* loss, void* stream);

/* avse_trainer_step (one Model.fit step of network.py:177-206, with the VideoNormalizer.normalize of
 * speech_enhancer.py:52-53 fused) with the video in video_dtype: a uint8 set is trained on with vnorm_* given, since it
 * cannot be normalised in place. */
int avse_trainer_step_video(avse_trainer* t, const float* audio, const void* video, int video_dtype,
                            const float* target, const float* vnorm_mean, const float* vnorm_std, int64_t N, float lr,
                            float dropout_rate, uint32_t dropout_seed, int flags, float* loss, void* stream);

/* Copy one of the trainer's blobs (avse_train_buffer) to the host; synchronises the device.  n_floats is the blob
 * size, except for AVSE_TRAIN_DEBUG_DZ (any count up to the size of the dz scratch). */
int avse_trainer_read(avse_trainer* t, int what, float* host_blob, int64_t n_floats);
/* Adam iterations applied so far (Keras `optimizer.iterations`). */
int avse_trainer_iterations(avse_trainer* t, int64_t* iterations);

/* ---- diagnostics ----------------------------------------------------------------------- */

/* Build flags of the loaded library: bit 0 = checked build (make DEBUG=1 -> libavse_debug.so, -DAVSE_DEBUG).  A checked
 * build runs device-side protocol and bounds checks (v_conv1 window-slot tags, STFT sample staging and output bounds,
 * ISTFT chunk frame ranges); avse_spectrogram / avse_istft / avse_forward then synchronise their stream and return
 * AVSE_ERR_CHECK with the first failing check (kernel, check, block, thread, value, expected) in avse_last_error. */
int avse_build_flags(void);

/* ---- evaluate ---------------------------------------------------------------------------- */

enum avse_eval_metric { AVSE_EVAL_SNR = 0, AVSE_EVAL_SI_SDR = 1, AVSE_EVAL_SEG_SNR = 2,
                        AVSE_EVAL_STOI = 3, AVSE_EVAL_STOI_KEPT = 4,
                        AVSE_EVAL_ESTOI = 5 /* avse_eval_pairs_ext only */ };
#define AVSE_EVAL_NMETRICS 5
/* Replaces speech_enhancement_evaluator.py:34-64 (the per-sample measure; PESQ itself stays an external binary).
 * Four open measures of a (clean, degraded) pair, for a ragged group of pairs in one call.
 *   ref, deg   float32 samples of n_pairs utterances, concatenated; pair u is [off[u], off[u + 1]) in BOTH buffers
 *              (the caller has cut each pair to a common length), at any element offset
 *   off        [n_pairs + 1] int64 element offsets (device array), ascending
 *   sr         sample rate of every pair, 8000 .. 48000
 *   metrics    [n_pairs][AVSE_EVAL_NMETRICS] float64
 * Returns AVSE_ERR_INVALID for a NULL argument, n_pairs < 1, sr outside 8000 .. 48000, or a pair of more than 2^24
 * samples.  The offsets are read on the device only: the caller, who built them, checks the pair lengths on the host
 * (the Python binding does), and this entry point trusts them as avse_mix_pairs does.  What the device does with
 * offsets that break the contract is bounded all the same: a pair longer than 2^24 samples, a descending offset, or
 * offsets that pass the end of the allocations holding ref / deg, is treated as a pair of 0 samples.
 * A pair of 0 samples gives NaN in every slot.
 *
 * All arithmetic is float64 on s = ref, y = deg (n samples), eps = 2^-52.
 *  SNR      10 log10(sum s^2 / sum (s - y)^2).
 *  SI-SDR   alpha = sum s y / sum s^2;  10 log10(alpha^2 sum s^2 / sum (alpha s - y)^2).  No mean is removed.
 *           Two passes (the sums, then the residual with alpha): deg == ref gives alpha == 1.0 and a residual of
 *           exactly 0, so SNR and SI-SDR are both +inf; sum s^2 == 0 gives NaN in both.
 *  Segmental SNR   win = round(0.03 sr) (halves up), skip = win / 4 as an integer, w[i] = 0.5 (1 - cos(2 pi (i + 1) /
 *           (win + 1))); frames start at i = 0, skip, .. while i + win <= n; per frame
 *           v = 10 log10(sum (w s)^2 / (sum (w (s - y))^2 + eps) + eps) clamped to [-10, 35]; the result is the mean
 *           over the frames, NaN without frames.
 *  STOI     (Taal et al. 2011; fs = 10 kHz, 256-sample frames, hop 128, 512-point FFT, 15 third-octave bands from
 *           150 Hz, 30-frame segments, beta = -15 dB, 40 dB dynamic range)
 *    1. Resample both signals by up / down = (10000 / g) / (sr / g), g = gcd(10000, sr), as
 *       scipy.signal.resample_poly(x, up, down) does with its defaults: H = 10 max(up, down), fc = 1 / max(up, down),
 *       h[i] = up fc sinc(fc (i - H)) I0(5 sqrt(1 - ((i - H) / H)^2)) / I0(5), i = 0 .. 2H, normalised so that
 *       sum(h) / up == 1; n10 = ceil(n up / down) outputs, y10[k] = sum_j h[H + k down - j up] x[j] over the j that keep
 *       the tap index in [0, 2H].  up == down is a copy.  (This is scipy's filter, not the MATLAB / pystoi one: values
 *       may differ from those tools in the low decimals.)  STOI is computed when max(up, down) <= 24; otherwise slots
 *       3 and 4 are NaN and 0 and the other metrics are still computed (avse_eval_pairs_ext with AVSE_EVAL_ANY_RATE
 *       computes STOI at every rate).
 *    2. Silent-frame removal: W[i] = 0.5 (1 - cos(2 pi (i + 1) / 257)), i < 256; frames start at i = 0, 128, .. while
 *       i < n10 - 256 (strict); e_i = 20 log10(||W x_i|| + eps) from the clean signal; a frame is kept when
 *       e_i > max(e) - 40.  K, the number of kept frames, is slot AVSE_EVAL_STOI_KEPT.  The kept windowed frames of
 *       both signals (the clean signal's mask) are overlap-added at hop 128 in order: (K - 1) 128 + 256 samples.
 *    3. Band spectra: the overlap-added signals are framed again by the same rule (M = K - 1 frames), windowed by W,
 *       zero-padded to 512; X[j][m], Y[j][m] = sqrt(sum of |rfft|^2 over the bins [lo_j, hi_j)), the bins nearest to
 *       150 2^(j/3) 2^(-+1/6) Hz on the grid of 10000 / 512 Hz: (7,9) (9,11) (11,14) (14,17) (17,22) (22,27) (27,34)
 *       (34,43) (43,55) (55,69) (69,87) (87,109) (109,138) (138,174) (174,219).
 *    4. For m = 30 .. M and each band j, over the 30 frames ending at m: a = sqrt(sum X^2 / (sum Y^2 + eps)),
 *       Y' = min(a Y, X (1 + 10^(15/20))), d = sum (X - mean X)(Y' - mean Y') / (||X - mean X|| ||Y' - mean Y'|| + eps).
 *       STOI = the mean of d over all j and m; NaN when M < 30 (no frames at all included).
 *    5. ESTOI (Jensen & Taal 2016; avse_eval_pairs_ext only, slot AVSE_EVAL_ESTOI): the same X, Y of step 3, no
 *       clipping and no factor a.  For m = 30 .. M, x = X[:, m-30:m] and y = Y[:, m-30:m] (15 bands x 30 frames) are
 *       each normalised twice: per band, minus the mean over its 30 frames, then over (its Euclidean norm + eps); then
 *       per frame, minus the mean over the 15 bands, then over (that column's norm + eps).
 *       d_m = (1/30) sum_{j,k} x y; ESTOI = the mean of d_m over m = 30 .. M, NaN when M < 30.  (pystoi adds
 *       eps-scaled random noise before each normalisation where this adds eps to the denominators: the value here is
 *       deterministic and may differ from pystoi's in the low decimals.)
 * Determinism: no floating-point atomics; every sum has an order fixed by the pair's own length (16 partial sums per
 * pair combined in part order; frame and segment values stored, then summed in index order by contiguous runs), so two
 * calls agree bit for bit and a pair's five numbers are the same bits alone and inside any batch, at any offset.
 * The call is asynchronous on `stream` and does not synchronise.  Scratch comes from the context and grows outside a
 * stream capture only.  The pair lengths are not known on the host, so this entry point sizes the scratch (up to about
 * 25 bytes per sample) for the most samples the allocations holding ref / deg have room for behind the two pointers
 * (hipMemGetAddressRange; pointers outside such allocations are refused): under a caching allocator that can be far
 * more than the data.  A caller who knows off[n_pairs] - off[0] uses avse_eval_pairs_sized, which sizes the scratch for
 * exactly that and takes any device pointer.  The tables of a sample rate are built and uploaded at the first call with
 * that rate, outside a capture; the context keeps the last four rates, and a call that builds tables (a new rate, or a
 * fifth one replacing the oldest) allocates, copies and frees, which synchronises the device. */
int avse_eval_pairs(avse_ctx* ctx, const float* ref, const float* deg, const int64_t* off,
                    int64_t n_pairs, int sr, double* metrics, void* stream);
/* avse_eval_pairs with total_samples = off[n_pairs] - off[0] as the caller, who built the offsets, knows it
 * (1 .. n_pairs * 2^24; 0 = unknown, which is avse_eval_pairs).  The scratch is sized for that many samples; offsets
 * that pass it make their pairs empty (NaN rows), nothing is written out of bounds. */
int avse_eval_pairs_sized(avse_ctx* ctx, const float* ref, const float* deg, const int64_t* off, int64_t n_pairs,
                          int64_t total_samples, int sr, double* metrics, void* stream);

#define AVSE_EVAL_NMETRICS_EXT 6   /* slots 0 .. 4 as avse_eval_pairs, slot 5 = AVSE_EVAL_ESTOI */
enum avse_eval_flags { AVSE_EVAL_ANY_RATE = 1 };
/* avse_eval_pairs_sized with a sixth slot per pair, ESTOI (step 5 above), and STOI at every rate on request.
 *   metrics    [n_pairs][AVSE_EVAL_NMETRICS_EXT] float64
 *   flags      0 or AVSE_EVAL_ANY_RATE; any other bit is AVSE_ERR_INVALID
 * Arguments, refusals, the scratch rule (total_samples, 0 = unknown), asynchrony and capture rules are those of
 * avse_eval_pairs_sized.
 * flags == 0: slots 0 .. 4 are the bits avse_eval_pairs_sized writes (the same kernels in the same order); ESTOI is NaN
 *   wherever STOI is NaN, the rates with max(up, down) > 24 included.
 * AVSE_EVAL_ANY_RATE: STOI, K and ESTOI are computed for every sr in 8000 .. 48000.  Rates with max(up, down) <= 24
 *   give the same bits as without the flag.  The larger ratios (44100: 100 / 441; a rate coprime to 10000: up = 10000)
 *   use step 1's formula and filter unchanged, H = 10 max(up, down) up to 479,990, each output summed in ascending j
 *   over its 2H / up + 1 taps; the filter is kept by phase on the device, up to 7.7 MB per rate.  At such a ratio a
 *   scratch bound (total_samples, or the room behind ref / deg) above 2^40 samples is AVSE_ERR_OOM.
 * ESTOI's sums: a band's mean and norm over its 30 frames in frame order; a frame's mean, norm and sum of x y over the
 * 15 bands in band order; d_m from the 30 frame sums in frame order; the mean of d_m as STOI's mean of d.  A pair's six
 * numbers are the same bits alone and inside any batch, at any offset, with or without the flag where both compute them.
 * The context's four table sets are per (rate, large-ratio filter): an AVSE_EVAL_ANY_RATE call and a default call at
 * 44100 use two of them. */
int avse_eval_pairs_ext(avse_ctx* ctx, const float* ref, const float* deg, const int64_t* off, int64_t n_pairs,
                        int64_t total_samples, int sr, int flags, double* metrics, void* stream);

/* Number of forward scratch buffers reported by avse_debug_scratch. */
#define AVSE_DEBUG_NBUF 20

/* Layout of the forward scratch for batch N in compute_dtype, valid after an avse_forward call
 * with that N: *base = device base pointer, offsets[i] = byte offset of buffer i, in launch order:
 *   0 video-in [N][128][128][8]  1 audio-in [N][80][20][8]  2-5 a_conv1..a_conv4
 *   6-10 v_conv1..v_conv5 (pooled)  11 concat [N][5248]  12 enc_dense  13 dec_dense1
 *   14 dec_dense2 [N][5][5][128]  15-19 d_deconv1..d_deconv5          (all NHWC, compute dtype)
 * Test / debugging aid only. */
int avse_debug_scratch(avse_ctx* ctx, int64_t N, int compute_dtype, void** base, int64_t* offsets);

#ifdef __cplusplus
}
#endif
#endif /* AVSE_H */
