"""End-to-end enhancement of whole utterances on one GPU (BASELINE configs[4]): STFT -> fusion CNN -> ISTFT.

The reference's predict loop (speech_enhancer.py:61-88) handles one sample at a time: `preprocess_audio_signal`
(data_processor.py:35-57) slices the mixture's mel-dB spectrogram, the network predicts the speech slices
(network.py:208-212, with VideoNormalizer.normalize before it), and `reconstruct_speech_signal`
(data_processor.py:60-74) re-analyses the mixture for its phase and inverts the predicted mel-dB.  Here a batch of
equal-length utterances runs through the same three steps on device tensors:

  K1  avse_spectrogram  [U, L] -> mel-dB slices [U, S, 80, spf] + the complex STFT [U, 321, T] (kept for the phase,
                        so the mixture is analysed once, not twice as in the reference)
  fwd avse_forward      [U*S, 80, spf] x [U*S, 128, 128, frames] -> [U*S, 80, spf], in chunks of <= `chunk` clips
                        (the normaliser fused into v_conv1)
  K6  avse_istft        predicted slices + mixture phase -> [U, hop * (S*spf - 1)]

Utterances of mixed lengths run through the ragged forms of K1 / K6 (Enhancer.enhance_ragged: one
avse_spectrogram_ragged, the forward over the concatenated clips, one avse_istft_ragged).

Every utterance is independent (top_db is per utterance), so a multi-GPU run shards utterances
(parallel.sharded_enhance) with no collective before the final gather.
"""
import numpy as np
import torch

from . import _lib, data_processor, ops


NoVideo = ops.NoVideo      # k video slices without video, as an entry of StreamEnhancer's `video` arguments


def _has_blank(video):
    """does a push_each `video` argument hold a NoVideo entry?"""
    for v in ([] if video is None else video):
        if isinstance(v, NoVideo) or (isinstance(v, (list, tuple)) and any(isinstance(p, NoVideo) for p in v)):
            return True
    return False


class Enhancer:
    """Batched predict path for one device: `enhancer(signals, video, vmean, vstd)` -> enhanced signals."""

    def __init__(self, weights, video_frame_rate=25.0, sample_rate=16000, slice_duration_ms=200, chunk=1024, stride=None):
        """stride (None, or 1 .. the video frames per slice): with a stride the object computes what a flushed
        SlidingStreamEnhancer of that stride does, at batch throughput: network windows at every
        stride-th video frame, each clamped at its causal floor, window 0's columns and the newest q * stride of every
        later window kept.  Its outputs are hop * (predicted - 1) samples per utterance, predicted =
        spf + q stride ((F (S - 1)) // stride): shorter than the slice path's where the stride does not divide
        F (S - 1).  `chunk` then counts windows, and video_present is refused (a partly blank window has no rule yet)."""
        self.weights = weights
        self.fps = float(video_frame_rate)
        self.sr = int(sample_rate)
        self.slice_ms = slice_duration_ms
        self.chunk = int(chunk)
        self.range_bits = 0
        self.stride = None if stride is None else int(stride)
        if self.stride is not None:
            F = int(round(self.fps * float(slice_duration_ms) / 1000))      # video frames per slice of this geometry
            if not 1 <= self.stride <= F:
                raise ValueError(f"stride must be 1 .. {F} (the video frames per slice), got {stride}")
            if self.chunk < 1:
                raise ValueError("chunk must be positive")
        self.staged_video_bytes = 0      # stride: bytes of the largest chunk of video windows the last call staged

    def geometry(self, n_video_slices):
        return data_processor.frame_geometry(self.sr, self.slice_ms, n_video_slices, self.fps)

    @staticmethod
    def _present(video_present, counts):
        """video_present of __call__ ([U, S] bool) / enhance_ragged (one sequence per utterance) as one host bool
        array over the concatenated clips; None stays None."""
        if video_present is None:
            return None
        if isinstance(video_present, torch.Tensor):
            video_present = video_present.cpu().numpy()
        rows = [np.asarray(r, dtype=bool).reshape(-1) for r in video_present]
        if [r.shape[0] for r in rows] != [int(c) for c in counts]:
            raise ValueError(f"video_present has {[r.shape[0] for r in rows]} entries per utterance, the video has "
                             f"{[int(c) for c in counts]} slices")
        return np.concatenate(rows)

    @staticmethod
    def _chunk_video(frames, present, a, b):
        """The video arguments of ops.forward for clips a..b: the rows with video gathered on the device (the rows
        without are never read), or the whole chunk when every clip has video."""
        if present is None or present[a:b].all():
            return frames[a:b], None
        idx = torch.from_numpy(np.flatnonzero(present[a:b])).to(frames.device)
        return (frames[a:b].index_select(0, idx) if idx.numel() else None), present[a:b]

    def __call__(self, signals, video, vmean=None, vstd=None, timings=None, video_present=None):
        """signals [U, L] float32 (int16-scale samples, padded / truncated to S slices like
        preprocess_audio_signal), video [U, S, 128, 128, frames] float32 or uint8 raw mouth crops; vmean / vstd the
        VideoNormalizer images.  Returns [U, hop * (S * spf - 1)] float32 enhanced speech.
        `timings`, when a dict, receives the stages' HIP-event milliseconds (adds synchronisation).
        video_present: [U, S] bool (host), False where a slice has no video (ops.forward's video_present: the slice is
        predicted from the all-zero normalised video; the network was not trained for that, and the quality of its
        audio-only estimate is unmeasured).  video keeps its full shape; the contents of such slices are never read."""
        if self.stride is not None and video_present is not None:
            raise ValueError("video_present is not built with a stride: a partly blank window has no rule")
        if signals.dim() != 2 or video.dim() != 5 or video.shape[0] != signals.shape[0]:
            raise ValueError("signals must be [U, L] and video [U, S, H, W, frames] with the same U")
        U, S = video.shape[0], video.shape[1]
        if self.stride is not None:      # [U, hop * (predicted - 1)]: the rows of enhance_ragged's packed buffer
            outs = self._slide(list(signals), list(video), vmean, vstd, timings,
                               frames=video.contiguous().view((U * S,) + tuple(video.shape[2:])))
            return torch.stack(outs)
        g = self.geometry(S)
        if g["n_slices"] != S:
            raise ValueError(f"{S} video slices but the audio geometry gives {g['n_slices']} spectrogram slices")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timings is not None else None
        if ev:
            ev[0].record()
        L = g["signal_length"]
        if signals.shape[1] != L:
            signals = torch.nn.functional.pad(signals, (0, max(0, L - signals.shape[1])))[:, :L].contiguous()
        spf = g["spectrogram_samples_per_slice"]
        if spf != self.weights.T or video.shape[-1] != self.weights.F:
            raise ValueError(f"{self.fps} fps gives [80, {spf}] slices with {video.shape[-1]} video frames; the weights "
                             f"are for [80, {self.weights.T}] x {self.weights.F} frames (build the network for this rate)")
        mel, stft = ops.spectrogram(signals, sample_rate=self.sr, n_fft=g["n_fft"], hop_length=g["hop_length"],
                                    n_mels=data_processor.N_MELS, fmin=data_processor.MEL_FMIN,
                                    fmax=data_processor.MEL_FMAX, frames_per_slice=spf, return_stft=True)
        if ev:
            ev[1].record()
        n = U * S
        present = self._present(video_present, [S] * U)
        clips = mel.view(n, data_processor.N_MELS, spf)
        frames = video.reshape((n,) + tuple(video.shape[2:]))
        pred = torch.empty_like(clips)
        # float32_split: each chunk's range guard is verified one chunk later (ops.RangePipeline), so the chunks'
        # forwards queue back to back; a flagged chunk is recomputed on the exact-fp32 kernels
        split = self.weights.dtype == _lib.AVSE_F32_SPLIT
        pipe = ops.RangePipeline(self.weights.ctx) if split else None
        if split:
            self.weights.ctx.set_aside_range()   # earlier forwards' bits stay readable by range_status()

        def chunk(a, b, checked):
            v, m = self._chunk_video(frames, present, a, b)
            ops.forward(self.weights, clips[a:b], v, vmean, vstd, out=pred[a:b], checked=checked, video_present=m)

        for a in range(0, n, self.chunk):
            b = min(n, a + self.chunk)
            chunk(a, b, False)
            if split:
                pipe.submit(lambda a=a, b=b: chunk(a, b, True))
        if ev:
            ev[2].record()
        def istft():
            return ops.istft(pred.view(U, S, data_processor.N_MELS, spf), stft, sample_rate=self.sr, n_fft=g["n_fft"],
                             hop_length=g["hop_length"], n_mels=data_processor.N_MELS, fmin=data_processor.MEL_FMIN,
                             fmax=data_processor.MEL_FMAX)
        out = istft()
        self.range_bits = 0
        if split:
            self.range_bits = pipe.drain()
            if pipe.recomputed:      # a chunk was redone after the ISTFT had been queued: redo the ISTFT after it
                out = istft()
        if ev:
            ev[3].record()
            ev[3].synchronize()
            timings.update(stft_ms=ev[0].elapsed_time(ev[1]), forward_ms=ev[1].elapsed_time(ev[2]),
                           istft_ms=ev[2].elapsed_time(ev[3]))
        return out

    def _slide(self, signals, videos, vmean, vstd, timings, return_spectrograms=False, frames=None):
        """The strided path of __call__ / enhance_ragged for signals[u] [L_u] and videos[u]
        [S_u, 128, 128, F]: one unclamped ragged STFT, the causal clamp and window gather (ops.slide_windows), forwards
        over chunks of <= `chunk` windows (which may span utterances) with each chunk's video windows gathered into one
        staging buffer (ops.slide_video_windows), the kept columns (ops.slide_keep), one ragged ISTFT.  -> a list of
        [hop * (predicted_u - 1)] views of one buffer; with return_spectrograms (out, net_in, pred, W)."""
        if len(signals) != len(videos) or not signals:
            raise ValueError("signals and videos must be non-empty lists of one length")
        geo = [self.geometry(int(v.shape[0])) for v in videos]
        g0 = geo[0]
        spf, F = g0["spectrogram_samples_per_slice"], self.weights.F
        fixed = []
        for u, (s, v, g) in enumerate(zip(signals, videos, geo)):
            if s.dim() != 1 or v.dim() != 4:
                raise ValueError(f"signals[{u}] must be [L] and videos[{u}] [S, H, W, frames]")
            if v.shape[0] < 1 or g["n_slices"] != v.shape[0]:
                raise ValueError(f"{v.shape[0]} video slices but the audio geometry gives {g['n_slices']} spectrogram slices")
            if spf != self.weights.T or v.shape[-1] != F:
                raise ValueError(f"{self.fps} fps gives [80, {spf}] slices with {v.shape[-1]} video frames; the weights "
                                 f"are for [80, {self.weights.T}] x {self.weights.F} frames (build the network for this rate)")
            L = g["signal_length"]
            if s.shape[0] != L:
                s = torch.nn.functional.pad(s, (0, max(0, L - s.shape[0])))[:L]
            fixed.append(s.contiguous())
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)] if timings is not None else None

        def mark(i):
            if ev:
                ev[i].record()
        mark(0)
        kw = dict(sample_rate=self.sr, n_fft=g0["n_fft"], hop_length=g0["hop_length"], n_mels=data_processor.N_MELS,
                  fmin=data_processor.MEL_FMIN, fmax=data_processor.MEL_FMAX)
        un, T, _, stft, sviews = ops.spectrogram_ragged(fixed, top_db=None, frames_per_slice=0, return_stft=True, **kw)
        mark(1)
        slices = np.array([int(v.shape[0]) for v in videos], dtype=np.int64)
        clips = ops.slide_windows(un, T, slices, frames_per_slice=spf, video_frames=F, stride=self.stride,
                                  n_mels=data_processor.N_MELS)
        mark(2)
        n = clips.shape[0]
        if frames is None:      # (__call__ hands over its batch as it stands)
            frames = torch.cat(videos) if len(videos) > 1 else videos[0].contiguous()
        pred = torch.empty_like(clips)
        stage = torch.empty((min(n, self.chunk),) + tuple(frames.shape[1:]), dtype=frames.dtype, device=frames.device)
        self.staged_video_bytes = stage.numel() * stage.element_size()
        split = self.weights.dtype == _lib.AVSE_F32_SPLIT
        pipe = ops.RangePipeline(self.weights.ctx) if split else None
        if split:
            self.weights.ctx.set_aside_range()

        def chunk(a, b, checked):      # the staging buffer is reused in stream order; a recompute gathers its chunk again
            v = ops.slide_video_windows(frames, slices, stride=self.stride, w0=a, n=b - a, out=stage)
            ops.forward(self.weights, clips[a:b], v, vmean, vstd, out=pred[a:b], checked=checked)

        for a in range(0, n, self.chunk):
            b = min(n, a + self.chunk)
            chunk(a, b, False)
            if split:
                pipe.submit(lambda a=a, b=b: chunk(a, b, True))
        mark(3)

        def istft():
            kept, P = ops.slide_keep(pred, slices, video_frames=F, stride=self.stride)
            mark(4)
            return ops.istft_ragged(kept, P, stft, [sh[1] for sh in sviews.shapes], **kw)
        out = istft()
        self.range_bits = 0
        if split:
            self.range_bits = pipe.drain()
            if pipe.recomputed:      # a chunk was redone after the ISTFT had been queued: redo the ISTFT after it
                out = istft()
        if ev:
            ev[5].record()
            ev[5].synchronize()
            timings.update(stft_ms=ev[0].elapsed_time(ev[1]), forward_ms=ev[2].elapsed_time(ev[3]),
                           istft_ms=ev[4].elapsed_time(ev[5]), windows_ms=ev[1].elapsed_time(ev[2]),
                           keep_ms=ev[3].elapsed_time(ev[4]))
        if return_spectrograms:
            return out, clips, pred, ops.slide_window_counts(slices, spf, F, self.stride)[0]
        return out

    def enhance_ragged(self, signals, videos, vmean=None, vstd=None, video_present=None, return_spectrograms=False):
        """With a stride: the same arguments -> a list of [hop * (predicted_u - 1)] tensors (views of one buffer), each
        the bits of that utterance alone; return_spectrograms (stride only) -> (that list, the windows' inputs
        [sum W_u, 80, spf], their predictions, W_u).  Without a stride:
        __call__ for utterances of mixed lengths: signals[u] is [L_u] float32, videos[u] [S_u, 128, 128, frames]
        (float32 or uint8, one dtype for all).  One ragged STFT, the forward over the concatenated clips of all
        utterances (in chunks of <= `chunk`, which may span utterances), one ragged ISTFT.  Each signal is padded /
        truncated to its own S_u slices first, as __call__ does for the batch.  Returns a list of [hop * (S_u * spf - 1)]
        tensors (views of one buffer), each the bits __call__ gives for that utterance alone.
        video_present: one bool sequence [S_u] per utterance, as __call__'s."""
        if self.stride is not None:
            if video_present is not None:
                raise ValueError("video_present is not built with a stride: a partly blank window has no rule")
            return self._slide(list(signals), list(videos), vmean, vstd, None, return_spectrograms=return_spectrograms)
        if return_spectrograms:
            raise ValueError("return_spectrograms is for an Enhancer with a stride")
        signals, videos = list(signals), list(videos)
        if len(signals) != len(videos) or not signals:
            raise ValueError("signals and videos must be non-empty lists of one length")
        geo = [self.geometry(int(v.shape[0])) for v in videos]
        g0 = geo[0]
        spf = g0["spectrogram_samples_per_slice"]
        fixed = []
        for u, (s, v, g) in enumerate(zip(signals, videos, geo)):
            if s.dim() != 1 or v.dim() != 4:
                raise ValueError(f"signals[{u}] must be [L] and videos[{u}] [S, H, W, frames]")
            if g["n_slices"] != v.shape[0]:
                raise ValueError(f"{v.shape[0]} video slices but the audio geometry gives {g['n_slices']} spectrogram slices")
            if spf != self.weights.T or v.shape[-1] != self.weights.F:
                raise ValueError(f"{self.fps} fps gives [80, {spf}] slices with {v.shape[-1]} video frames; the weights "
                                 f"are for [80, {self.weights.T}] x {self.weights.F} frames (build the network for this rate)")
            L = g["signal_length"]
            if s.shape[0] != L:
                s = torch.nn.functional.pad(s, (0, max(0, L - s.shape[0])))[:L]
            fixed.append(s.contiguous())
        kw = dict(sample_rate=self.sr, n_fft=g0["n_fft"], hop_length=g0["hop_length"], n_mels=data_processor.N_MELS,
                  fmin=data_processor.MEL_FMIN, fmax=data_processor.MEL_FMAX)
        clips, counts, _, stft, sviews = ops.spectrogram_ragged(fixed, frames_per_slice=spf, return_stft=True, **kw)
        if [int(c) for c in counts] != [int(v.shape[0]) for v in videos]:
            raise ValueError("the spectrogram's slice counts differ from the videos'")
        n = clips.shape[0]
        present = self._present(video_present, counts)
        frames = torch.cat(videos) if len(videos) > 1 else videos[0]
        pred = torch.empty_like(clips)
        split = self.weights.dtype == _lib.AVSE_F32_SPLIT
        pipe = ops.RangePipeline(self.weights.ctx) if split else None
        if split:
            self.weights.ctx.set_aside_range()

        def chunk(a, b, checked):
            v, m = self._chunk_video(frames, present, a, b)
            ops.forward(self.weights, clips[a:b], v, vmean, vstd, out=pred[a:b], checked=checked, video_present=m)

        for a in range(0, n, self.chunk):
            b = min(n, a + self.chunk)
            chunk(a, b, False)
            if split:
                pipe.submit(lambda a=a, b=b: chunk(a, b, True))

        def istft():
            return ops.istft_ragged(pred, counts, stft, [sh[1] for sh in sviews.shapes], **kw)
        out = istft()
        self.range_bits = 0
        if split:
            self.range_bits = pipe.drain()
            if pipe.recomputed:      # a chunk was redone after the ISTFT had been queued: redo the ISTFT after it
                out = istft()
        return out


class StreamEnhancer:
    """Enhancement of audio as it arrives: `n_streams` streams pushed in chunks of any size, in lock
    step (push / flush: e.g. the participants of one call) or each at its own pace (push_each / open / close: the
    callers of a service).

    The reference's predict loop needs the whole utterance (the reflect padding of both ends, the top_db floor from
    the utterance's maximum, the window sum of the finished signal).  A session carries the sample tail, the running
    floor, the mixture phase of frames awaiting their prediction and the overlap-add tail between pushes instead;
    include/avse.h avse_stream_push states what each push computes.  Where the unclamped mel-dB range of a stream stays
    below top_db the concatenated output is the offline Enhancer's, for all slice * S - hop samples (3200 S - 160 at
    16 kHz).

    Only geometries whose slices do not drift against the samples stream, and of those 25 fps at sample_rate 16000,
    32000 or 48000 (n_fft = rate / 25; the same weights) and 30 fps at sample_rate 24000 or 48000 (n_fft = rate / 30,
    weights of the [80, 24] x 6-frame network); ops.stream_supported is the rule.  29.97 fps, 30 fps at 16 kHz (n_fft
    533) and 44.1 kHz raise _lib.AvseError at construction.

    Any other rate goes through `input_rate=R`: push, flush, push_each and close then take and return
    samples at R, while the session runs at `sample_rate` (16000 by default; 24000 or 48000 with 30-fps weights).  Per
    call a stateful device resampler (ops.resampler_create, R -> sample_rate) feeds the session and a second one
    (sample_rate -> R) takes the session's output rows in place; nothing leaves the device.  Each resampler is
    scipy.signal.resample_poly with its defaults in float64, and its output does not depend on the cuts, so a stream's
    concatenated output is, bit for bit, ops.resample(R -> sample_rate) -> a plain StreamEnhancer -> ops.resample(back).
    The network then sees the feature scale it was trained on (a native 44.1 kHz frame would sit 8.81 dB above it), and
    nothing is lost: the mel bank ends at 8 kHz at every rate.  R samples in give F(n) = max(0, ceil((n up - H) / down))
    session samples, H = 10 max(up, down); a flush flushes the first resampler in the call that flushes the session and
    then the second.  The session's limits (max_slices, a flush needs n <= slice * v) apply to the resampled counts and
    are checked on the host before the first launch, so a refused call leaves all three objects as they were.
    input_rate=None (or equal to sample_rate) is the object described above, with no resampler built.

    A camera at any other frame rate goes through `input_fps=R`: `video_frame_rate` stays the rate of
    the weights and the session, and the `video` arguments become mouth crops at R fps: push takes frames
    [B, n, 128, 128], push_each and close take [n_b, 128, 128] per stream (float32 or uint8, the session's dtype).  Per
    call a stateful device retimer (ops.retimer_create, R -> video_frame_rate; linear interpolation between the two
    nearest frames, include/avse.h states the rounding) turns them into the session's slices, which go on to the session
    with no copy; its output does not depend on the cuts, so a stream's concatenated result is, bit for bit,
    ops.retime(all its frames) -> the same StreamEnhancer without input_fps, fed those slices.  R is an int, a
    fractions.Fraction, a (num, den) pair or a float (ops.frame_rate: 29.97 is 2997/100, 30000 / 1001 is NTSC).  n frames
    in give G(n) = floor((n - 1) q / p) + 1 output frames, p / q = R / video_frame_rate, of which every F make a slice; a
    flush flushes the retimer first (the last frame is repeated up to ceil(n q / p) frames, what does not fill a slice is
    dropped), then the rest of the chain.  Alone or together with input_rate; the session's limits are checked on the
    host before the first launch either way.  input_fps=None (or equal to video_frame_rate) builds no retimer.  Whether
    the 25-fps network prefers blended or repeated frames has not been measured."""

    def __init__(self, weights, n_streams, video_frame_rate=25.0, sample_rate=16000, slice_duration_ms=200, max_slices=4,
                 video_dtype=torch.float32, input_rate=None, input_fps=None):
        self.weights = weights
        g = data_processor.frame_geometry(int(sample_rate), slice_duration_ms, 1, float(video_frame_rate))
        self.geometry = g
        spf = g["spectrogram_samples_per_slice"]
        if spf != weights.T:
            raise ValueError(f"{video_frame_rate} fps gives [80, {spf}] slices; the weights are for [80, {weights.T}]")
        self.session = ops.stream_create(weights, n_streams, sample_rate=int(sample_rate), n_fft=g["n_fft"],
                                         hop_length=g["hop_length"], frames_per_slice=spf, n_mels=data_processor.N_MELS,
                                         fmin=data_processor.MEL_FMIN, fmax=data_processor.MEL_FMAX,
                                         video_dtype=video_dtype, max_slices=max_slices)
        self._busy = set()      # slots handed out by open()
        self._blank_seen = False   # a NoVideo entry was given: counts then has blank_slices
        self.sample_rate = int(sample_rate)
        self.input_rate = None if input_rate is None or int(input_rate) == int(sample_rate) else int(input_rate)
        self.resampler_in = self.resampler_out = None
        if self.input_rate is not None:
            dev = torch.device("cuda", weights.ctx.device_index)
            self.resampler_in = ops.resampler_create(n_streams, self.input_rate, self.sample_rate, dev)
            self.resampler_out = ops.resampler_create(n_streams, self.sample_rate, self.input_rate, dev)
        self.input_fps = self.retimer = None
        if input_fps is not None and ops.frame_rate(input_fps) != ops.frame_rate(video_frame_rate):
            self.input_fps = ops.frame_rate(input_fps)
            self.retimer = ops.retimer_create(n_streams, self.input_fps, video_frame_rate, weights.F, video_dtype,
                                              torch.device("cuda", weights.ctx.device_index))

    def push(self, samples, video=None, vmean=None, vstd=None, return_spectrograms=False):
        """samples [B, n] float32 (int16-scale), video [B, v, 128, 128, F] float32 or uint8 (the session's dtype) or
        None -> the [B, n_out] newly final samples; with return_spectrograms also the [B, k, 80, spf] slices the
        network saw and predicted for the k slices this push completed.  With input_rate the samples in and out are at
        that rate (and the results come back per stream, as lists, once the streams are out of step).  With input_fps
        video is [B, n, 128, 128]: n frames at that rate.
        video=NoVideo(k): k slices without video for every stream (camera off, mouth lost, packets late).  They count
        as video slices and are predicted from the all-zero normalised video, so the streams go on emitting; the
        network was not trained with missing video, and the quality of its audio-only estimate is unmeasured.
        last_video_present then says which completed slices had video.  Not with input_fps (see push_each)."""
        if isinstance(video, NoVideo):
            B = self.session.n_streams
            if samples is not None and (samples.dim() != 2 or samples.shape[0] != B):
                raise ValueError(f"samples must be [{B}, n]")
            res = self.push_each(None if samples is None else list(samples), [video] * B, None, vmean, vstd,
                                 return_spectrograms)
            parts = res if return_spectrograms else (res,)
            if any(len({tuple(t.shape) for t in p}) > 1 for p in parts):
                return res      # the streams are out of step: per-stream lists, as push gives then
            stacked = tuple(torch.stack(list(p)) for p in parts)
            return stacked if return_spectrograms else stacked[0]
        if self.input_rate is not None or self.retimer is not None:
            return self._anyrate_lockstep(samples, video, False, vmean, vstd, return_spectrograms)
        return ops.stream_push(self.session, samples, video, vmean, vstd, return_spectrograms)

    def flush(self, vmean=None, vstd=None, return_spectrograms=False):
        """Close the streams as the offline call on the signal zero-padded to the video's length; returns the rest."""
        if self.input_rate is not None or self.retimer is not None:
            return self._anyrate_lockstep(None, None, True, vmean, vstd, return_spectrograms)
        return ops.stream_flush(self.session, vmean, vstd, return_spectrograms)

    def reset(self):
        ops.stream_reset(self.session)
        if self.input_rate is not None:
            ops.resampler_reset_each(self.resampler_in)
            ops.resampler_reset_each(self.resampler_out)
        if self.retimer is not None:
            ops.retimer_reset_each(self.retimer)
        self._busy = set()

    # ---- input_rate / input_fps: retimer -> resampler in -> session -> resampler out, one call of each per push ----
    def _label(self):
        return ", ".join([f"input_rate={self.input_rate}"] * (self.input_rate is not None) +
                         [f"input_fps={self.input_fps}"] * (self.retimer is not None))

    def _anyrate_check(self, n_mid, v_new, flush):
        """The session's refusals (stream_geom.h stream_rows) for a call with these per-stream counts (samples at the
        session's rate, video slices), from the host totals, before anything is launched: the retimer and the first
        resampler cannot be taken back once they have run."""
        s, g = self.session, self.geometry
        spf = g["spectrogram_samples_per_slice"]
        slice_, M = spf * g["hop_length"], s.max_slices
        for b in range(s.n_streams):
            dn, dv, fl = n_mid[b], v_new[b], flush[b]
            if s.fl[b] and (dn > 0 or dv > 0 or fl):
                why = "pushed or flushed after its flush: only a reset is legal"
            else:
                n2, v2 = s.ns[b] + dn, s.vs[b] + dv
                if fl and n2 > slice_ * v2:
                    why = "flush: more samples than the video slices cover (n > slice * v)"
                else:
                    _, k0, _ = ops.stream_counts(s.ns[b], s.vs[b], s.fl[b], s)
                    f1, k1, _ = ops.stream_counts(n2, v2, s.fl[b] or fl, s)
                    if k1 - k0 > M:
                        why = "the call would complete more than max_slices slices"
                    elif n2 - slice_ * v2 > slice_ * M:
                        why = "more than max_slices slices of samples queued ahead of the video"
                    elif v2 - f1 // spf > M:
                        why = "more than max_slices video slices queued ahead of the samples"
                    else:
                        continue
            raise _lib.AvseError(f"StreamEnhancer({self._label()}): stream {b}: {why} (counts at "
                                 f"{self.sample_rate} Hz; nothing was launched)")

    def _anyrate_step(self, packed, off, n_new, vpacked, v_new, flush, vmean, vstd, return_spectrograms, f_off=None,
                      present=None):
        """One call of the chain on packed arguments -> (out [B, max count] at input_rate, counts, mel, pred, slices).
        With input_fps vpacked holds frames, v_new counts them and f_off is each stream's first frame in vpacked."""
        rin, rout, s, rt = self.resampler_in, self.resampler_out, self.session, self.retimer
        B = s.n_streams
        for b in range(B):
            if (rin is not None and rin.fl[b] and (n_new[b] > 0 or flush[b])) or \
                    (rt is not None and rt.fl[b] and (v_new[b] > 0 or flush[b])):
                raise _lib.AvseError(f"StreamEnhancer({self._label()}): stream {b}: pushed or flushed after "
                                     "its flush: only a reset is legal")
        n_mid = rin.expect(n_new, flush) if rin is not None else list(n_new)
        k_vid = rt.expect(v_new, flush) if rt is not None else list(v_new)
        self._anyrate_check(n_mid, k_vid, flush)
        if rt is not None:
            vpacked, v_new = ops._retimer_push_packed(rt, vpacked, f_off, v_new, flush)
            vpacked = vpacked if sum(v_new) else None
        if rin is None:
            out, mel, pred, ks, es = ops._stream_push_packed(s, packed, off, n_new, vpacked, v_new, flush, vmean, vstd,
                                                             return_spectrograms, present=present)
            return out, es, mel, pred, ks
        mid, n_mid = ops._resampler_push_packed(rin, packed, off, n_new, flush)
        stride = int(mid.shape[1])
        enh, mel, pred, ks, es = ops._stream_push_packed(s, mid, [b * stride for b in range(B)], n_mid, vpacked, v_new,
                                                         flush, vmean, vstd, return_spectrograms, present=present)
        stride = int(enh.shape[1])
        out, n_ret = ops._resampler_push_packed(rout, enh, [b * stride for b in range(B)], es, flush)
        return out, n_ret, mel, pred, ks

    def _anyrate_lockstep(self, samples, video, flush, vmean, vstd, return_spectrograms):
        w, s = self.weights, self.session
        B = s.n_streams
        n = v = 0
        if samples is not None:
            ops._dev_f32(samples, "samples")
            if samples.dim() != 2 or samples.shape[0] != B:
                raise ValueError(f"samples must be [{B}, n]")
            n = int(samples.shape[1])
        if video is not None and self.retimer is not None:
            if ops._dev_frames(video, "video", 4) != s.video_dtype:
                raise TypeError(f"video is {video.dtype}, the session was created for the other video dtype")
            if video.shape[0] != B:
                raise ValueError(f"video must be [{B}, n, 128, 128] (frames at input_fps)")
            v = int(video.shape[1])
        elif video is not None:
            if ops._dev_video(video, "video", (128, 128, w.F)) != s.video_dtype:
                raise TypeError(f"video is {video.dtype}, the session was created for the other video dtype")
            if video.dim() != 5 or video.shape[0] != B:
                raise ValueError(f"video must be [{B}, v, 128, 128, {w.F}]")
            v = int(video.shape[1])
        todo = [flush and not f for f in s.fl]
        if flush and not any(todo):
            raise _lib.AvseError("flush after flush: only reset is legal")
        out, n_ret, mel, pred, ks = self._anyrate_step(samples if n else None, [b * n for b in range(B)], [n] * B,
                                                       video.reshape((B * v,) + tuple(video.shape[2:])) if v else None,
                                                       [v] * B, todo, vmean, vstd, return_spectrograms,
                                                       f_off=[b * v for b in range(B)])
        if len(set(n_ret)) > 1 or len(set(ks)) > 1:
            return ops._stream_split(out, mel, pred, ks, n_ret, return_spectrograms)
        out = out[:, :n_ret[0]]
        if not return_spectrograms:
            return out
        shape = (B, ks[0], 80, s.spf)
        return out, mel.view(shape), pred.view(shape)

    def _anyrate_each(self, samples, video, flush, vmean, vstd, return_spectrograms):
        f_off = present = None
        if self.retimer is not None:
            B = self.session.n_streams
            frames = [None] * B if video is None else list(video)
            if len(frames) != B:
                raise ValueError(f"samples, video and flush must have one entry per stream ({B})")
            packed, off, n_new, _, _, flush = ops._stream_pack_each(self.session, samples, None, flush, vmean, vstd)
            vpacked, f_off, v_new = ops._retimer_pack(self.retimer, frames)
        else:
            packed, off, n_new, vpacked, v_new, flush = ops._stream_pack_each(self.session, samples, video, flush, vmean,
                                                                              vstd)
            present = self.session._v_present
        out, n_ret, mel, pred, ks = self._anyrate_step(packed, off, n_new, vpacked, v_new, flush, vmean, vstd,
                                                       return_spectrograms, f_off=f_off, present=present)
        return ops._stream_split(out, mel, pred, ks, n_ret, return_spectrograms)

    # ---- independent streams: the slots of one session serve callers that never move together ----
    def push_each(self, samples=None, video=None, flush=None, vmean=None, vstd=None, return_spectrograms=False):
        """Every stream by its own amount (ops.stream_push_each): samples / video are lists with one tensor (1-D float32;
        [v, 128, 128, F]) or None per stream, flush a list of bools -> per-stream lists of what push returns.  A stream
        without input costs nothing; each stream's output is, bit for bit, that of a session of its own.  With
        input_rate the samples in and out are at that rate; with input_fps video[b] is [n_b, 128, 128], frames at that
        rate.
        An entry of video may also be NoVideo(k), k slices without video, or a list of tensors and NoVideo in arrival
        order (ops.stream_push_each); input_rate composes unchanged.  NoVideo together with input_fps raises ValueError:
        a gap in a retimed stream needs a rule for the slice the gap cuts, which is not built."""
        blank = _has_blank(video)
        if self.retimer is not None and blank:
            raise ValueError("NoVideo with input_fps: a gap in a retimed stream needs a rule for the slice the gap cuts "
                             "(not built); feed such a stream at the weights' frame rate")
        self._blank_seen = self._blank_seen or blank
        if self.input_rate is not None or self.retimer is not None:
            return self._anyrate_each(samples, video, flush, vmean, vstd, return_spectrograms)
        return ops.stream_push_each(self.session, samples, video, flush, vmean, vstd, return_spectrograms)

    def reset_streams(self, ids):
        """The listed streams back to the state after construction; the others keep streaming."""
        ops.stream_reset_each(self.session, ids)
        if self.input_rate is not None:
            ops.resampler_reset_each(self.resampler_in, ids)
            ops.resampler_reset_each(self.resampler_out, ids)
        if self.retimer is not None:
            ops.retimer_reset_each(self.retimer, ids)

    def open(self):
        """-> a free slot (the lowest stream no caller holds) for a caller that joins; close() gives it back."""
        for b in range(self.session.n_streams):
            if b not in self._busy:
                self._busy.add(b)
                return b
        raise RuntimeError(f"all {self.session.n_streams} streams of the session are in use")

    def close(self, slot, vmean=None, vstd=None, samples=None, video=None):
        """A caller hangs up: flushes the slot, resets it and frees it -> its last samples (1-D).  samples / video: the
        slot's last input (video as an entry of push_each: a tensor, NoVideo(k) or a list of both), fed in the same
        call."""
        B = self.session.n_streams
        flush = [b == slot for b in range(B)]
        each = lambda x: None if x is None else [x if b == slot else None for b in range(B)]
        last = self.push_each(each(samples), each(video), flush, vmean=vmean, vstd=vstd)[slot]
        self.reset_streams([slot])
        self._busy.discard(slot)
        return last

    @property
    def last_video_present(self):
        """Per stream, which of the slices the last per-stream call completed had video (a list of bools each)."""
        return [list(k) for k in self.session.k_present]

    @property
    def counts(self):
        """Host totals: dict(samples, video_slices, frames, slices, emitted) while the streams are in step, else the
        same keys with one list entry per stream.  Once the enhancer has been given a NoVideo entry, blank_slices
        counts the slices without video received (video_slices includes them).  With input_rate the keys above count at the session's rate, and
        `received` / `returned` count the samples taken and given back at input_rate.  With input_fps `video_frames`
        counts the frames received at that rate (video_slices: the slices the retimer has handed to the session)."""
        s = self.session
        if s.in_step:
            f, k, e = ops.stream_counts(s.n, s.v, s.flushed, s)
            c = dict(samples=s.n, video_slices=s.v, frames=f, slices=k, emitted=e)
            if self._blank_seen:
                blank = ops.stream_blank(s)
                c.update(blank_slices=blank[0] if len(set(blank)) == 1 else blank)
            if self.input_rate is not None:
                c.update(received=self.resampler_in.ns[0], returned=self.resampler_out.outs[0])
            if self.retimer is not None:
                rt = self.retimer
                c.update(video_frames=rt.ns[0] if len(set(rt.ns)) == 1 else list(rt.ns))
            return c
        rows = [ops.stream_counts(n, v, fl, s) for n, v, fl in zip(s.ns, s.vs, s.fl)]
        c = dict(samples=list(s.ns), video_slices=list(s.vs), frames=[r[0] for r in rows],
                 slices=[r[1] for r in rows], emitted=[r[2] for r in rows])
        if self._blank_seen:
            c.update(blank_slices=ops.stream_blank(s))
        if self.input_rate is not None:
            c.update(received=list(self.resampler_in.ns), returned=list(self.resampler_out.outs))
        if self.retimer is not None:
            c.update(video_frames=list(self.retimer.ns))
        return c

    @property
    def range_bits(self):
        """float32_split: the range-guard bits the pushes' forwards raised since the last read (waits for the stream;
        Context.range_status); 0 for the other dtypes."""
        if self.weights.dtype != _lib.AVSE_F32_SPLIT:
            return 0
        return self.weights.ctx.range_status()


class SlidingStreamEnhancer:
    """Low-latency streaming: a StreamEnhancer whose network windows start at every `stride`-th video
    frame instead of every slice.  Video arrives as frames ([128, 128] mouth crops), not as slices.  The network runs on
    the most recent 200-ms window each time `stride` new video frames and their samples are there; window 0 contributes
    all its predicted columns, every later window its newest q * stride (q = spectrogram frames per video frame).
    Beyond the first window a sample therefore waits for q * stride * hop + n_fft / 2 + hop samples (70 ms at 16 kHz,
    25 fps, stride 1) instead of a whole slice plus the tail (230 ms), for F / stride times the forwards.  Keeping the
    newest columns is the choice latency asks for; whether centre columns would sound better has not been measured.

    Each window's input is clamped at the causal floor of StreamEnhancer evaluated at the window's last frame, so the
    output does not depend on how the input was cut.  stride = F is, bit for bit, a StreamEnhancer fed the same frames
    stacked into slices.  max_windows: the most windows one call may complete per stream, and how many windows either
    input may run ahead of the other.  Geometries as StreamEnhancer (ops.slide_supported is the rule).

    input_rate, input_fps and NoVideo are not built around a sliding session (ValueError): the resampler composes
    unchanged and the retimer with one frame per slice, but a blank frame needs a rule for windows that are partly
    blank."""

    def __init__(self, weights, n_streams, stride=1, video_frame_rate=25.0, sample_rate=16000, slice_duration_ms=200,
                 max_windows=8, video_dtype=torch.float32, input_rate=None, input_fps=None):
        if input_rate is not None or input_fps is not None:
            raise ValueError("SlidingStreamEnhancer: input_rate / input_fps are not built around a sliding session; "
                             "resample or retime before it")
        self.weights = weights
        g = data_processor.frame_geometry(int(sample_rate), slice_duration_ms, 1, float(video_frame_rate))
        self.geometry = g
        spf = g["spectrogram_samples_per_slice"]
        if spf != weights.T:
            raise ValueError(f"{video_frame_rate} fps gives [80, {spf}] slices; the weights are for [80, {weights.T}]")
        self.stride = int(stride)
        self.sample_rate = int(sample_rate)
        self.session = ops.slide_create(weights, n_streams, stride=self.stride, sample_rate=int(sample_rate),
                                        n_fft=g["n_fft"], hop_length=g["hop_length"], frames_per_slice=spf,
                                        n_mels=data_processor.N_MELS, fmin=data_processor.MEL_FMIN,
                                        fmax=data_processor.MEL_FMAX, video_dtype=video_dtype, max_windows=max_windows)
        self._busy = set()      # slots handed out by open()

    @property
    def latency_samples(self):
        """Samples a sample waits beyond the first window: q * stride * hop + n_fft / 2 + hop."""
        g = self.geometry
        q = g["spectrogram_samples_per_slice"] // self.weights.F
        return q * self.stride * g["hop_length"] + g["n_fft"] // 2 + g["hop_length"]

    def _lockstep(self, samples, video, flush, vmean, vstd, return_spectrograms):
        s = self.session
        B = s.n_streams
        if isinstance(video, NoVideo):
            raise ValueError("SlidingStreamEnhancer: NoVideo needs a rule for windows that are partly blank (not built)")
        if samples is not None and (samples.dim() != 2 or samples.shape[0] != B):
            raise ValueError(f"samples must be [{B}, n]")
        if video is not None and (video.dim() != 4 or video.shape[0] != B):
            raise ValueError(f"video must be [{B}, k, 128, 128] (video frames)")
        todo = [flush and not f for f in s.fl]
        if flush and not any(todo):
            raise _lib.AvseError("flush after flush: only reset is legal")
        res = ops.slide_push_each(s, None if samples is None else list(samples), None if video is None else list(video),
                                  todo, vmean, vstd, return_spectrograms)
        parts = res if return_spectrograms else (res,)
        if any(len({tuple(t.shape) for t in p}) > 1 for p in parts):
            return res      # the streams are out of step: per-stream lists
        stacked = tuple(torch.stack(list(p)) for p in parts)
        return stacked if return_spectrograms else stacked[0]

    def push(self, samples, video=None, vmean=None, vstd=None, return_spectrograms=False):
        """samples [B, n] float32 (int16-scale) or None, video [B, k, 128, 128] float32 or uint8 (the session's dtype):
        k video frames, or None -> the [B, n_out] newly final samples; with return_spectrograms also the [B, w, 80, spf]
        whole windows the network saw and predicted for the w windows this push completed.  Per-stream lists once the
        streams are out of step, as StreamEnhancer.push."""
        return self._lockstep(samples, video, False, vmean, vstd, return_spectrograms)

    def flush(self, vmean=None, vstd=None, return_spectrograms=False):
        """Close the streams as the signal zero-padded to hop * q * (video frames received); returns the rest.  Video
        frames past the last full stride are dropped."""
        return self._lockstep(None, None, True, vmean, vstd, return_spectrograms)

    def push_each(self, samples=None, video=None, flush=None, vmean=None, vstd=None, return_spectrograms=False):
        """Every stream by its own amount (ops.slide_push_each): samples / video are lists with one tensor (1-D float32;
        [k, 128, 128] video frames) or None per stream, flush a list of bools -> per-stream lists of what push returns.
        Each stream's output is, bit for bit, that of a session of its own."""
        if _has_blank(video):
            raise ValueError("SlidingStreamEnhancer: NoVideo needs a rule for windows that are partly blank (not built)")
        return ops.slide_push_each(self.session, samples, video, flush, vmean, vstd, return_spectrograms)

    def reset(self):
        ops.slide_reset_each(self.session)
        self._busy = set()

    def reset_streams(self, ids):
        """The listed streams back to the state after construction; the others keep streaming."""
        ops.slide_reset_each(self.session, ids)

    def open(self):
        """-> a free slot (the lowest stream no caller holds) for a caller that joins; close() gives it back."""
        for b in range(self.session.n_streams):
            if b not in self._busy:
                self._busy.add(b)
                return b
        raise RuntimeError(f"all {self.session.n_streams} streams of the session are in use")

    def close(self, slot, vmean=None, vstd=None, samples=None, video=None, return_spectrograms=False):
        """A caller hangs up: flushes the slot, resets it and frees it -> its last samples (1-D); with
        return_spectrograms also the [w, 80, spf] windows the flush completed, as seen and as predicted.  samples /
        video: the slot's last input, fed in the same call."""
        B = self.session.n_streams
        flush = [b == slot for b in range(B)]
        each = lambda x: None if x is None else [x if b == slot else None for b in range(B)]
        res = self.push_each(each(samples), each(video), flush, vmean, vstd, return_spectrograms)
        self.reset_streams([slot])
        self._busy.discard(slot)
        return tuple(r[slot] for r in res) if return_spectrograms else res[slot]

    @property
    def counts(self):
        """Host totals: dict(samples, video_frames, frames, windows, predicted, emitted) while the streams are in step,
        else the same keys with one list entry per stream."""
        s = self.session
        rows = [ops.slide_counts(n, f, fl, session=s) for n, f, fl in zip(s.ns, s.fs, s.fl)]
        c = dict(samples=list(s.ns), video_frames=list(s.fs), frames=[r[0] for r in rows], windows=[r[1] for r in rows],
                 predicted=[r[2] for r in rows], emitted=[r[3] for r in rows])
        return {k: v[0] for k, v in c.items()} if s.in_step else c

    @property
    def range_bits(self):
        """float32_split: the range-guard bits the pushes' forwards raised since the last read (waits for the stream;
        Context.range_status); 0 for the other dtypes."""
        if self.weights.dtype != _lib.AVSE_F32_SPLIT:
            return 0
        return self.weights.ctx.range_status()
