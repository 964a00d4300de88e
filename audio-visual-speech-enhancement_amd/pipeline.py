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
import torch

from . import _lib, data_processor, ops


class Enhancer:
    """Batched predict path for one device: `enhancer(signals, video, vmean, vstd)` -> enhanced signals."""

    def __init__(self, weights, video_frame_rate=25.0, sample_rate=16000, slice_duration_ms=200, chunk=1024):
        self.weights = weights
        self.fps = float(video_frame_rate)
        self.sr = int(sample_rate)
        self.slice_ms = slice_duration_ms
        self.chunk = int(chunk)
        self.range_bits = 0

    def geometry(self, n_video_slices):
        return data_processor.frame_geometry(self.sr, self.slice_ms, n_video_slices, self.fps)

    def __call__(self, signals, video, vmean=None, vstd=None, timings=None):
        """signals [U, L] float32 (int16-scale samples, padded / truncated to S slices like
        preprocess_audio_signal), video [U, S, 128, 128, frames] float32 or uint8 raw mouth crops; vmean / vstd the
        VideoNormalizer images.  Returns [U, hop * (S * spf - 1)] float32 enhanced speech.
        `timings`, when a dict, receives the stages' HIP-event milliseconds (adds synchronisation)."""
        if signals.dim() != 2 or video.dim() != 5 or video.shape[0] != signals.shape[0]:
            raise ValueError("signals must be [U, L] and video [U, S, H, W, frames] with the same U")
        U, S = video.shape[0], video.shape[1]
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
            ops.forward(self.weights, clips[a:b], frames[a:b], vmean, vstd, out=pred[a:b], checked=checked)

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

    def enhance_ragged(self, signals, videos, vmean=None, vstd=None):
        """__call__ for utterances of mixed lengths: signals[u] is [L_u] float32, videos[u] [S_u, 128, 128, frames]
        (float32 or uint8, one dtype for all).  One ragged STFT, the forward over the concatenated clips of all
        utterances (in chunks of <= `chunk`, which may span utterances), one ragged ISTFT.  Each signal is padded /
        truncated to its own S_u slices first, as __call__ does for the batch.  Returns a list of [hop * (S_u * spf - 1)]
        tensors (views of one buffer), each the bits __call__ gives for that utterance alone."""
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
        frames = torch.cat(videos) if len(videos) > 1 else videos[0]
        pred = torch.empty_like(clips)
        split = self.weights.dtype == _lib.AVSE_F32_SPLIT
        pipe = ops.RangePipeline(self.weights.ctx) if split else None
        if split:
            self.weights.ctx.set_aside_range()

        def chunk(a, b, checked):
            ops.forward(self.weights, clips[a:b], frames[a:b], vmean, vstd, out=pred[a:b], checked=checked)

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
    533) and 44.1 kHz raise _lib.AvseError at construction."""

    def __init__(self, weights, n_streams, video_frame_rate=25.0, sample_rate=16000, slice_duration_ms=200, max_slices=4,
                 video_dtype=torch.float32):
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

    def push(self, samples, video=None, vmean=None, vstd=None, return_spectrograms=False):
        """samples [B, n] float32 (int16-scale), video [B, v, 128, 128, F] float32 or uint8 (the session's dtype) or
        None -> the [B, n_out] newly final samples; with return_spectrograms also the [B, k, 80, spf] slices the
        network saw and predicted for the k slices this push completed."""
        return ops.stream_push(self.session, samples, video, vmean, vstd, return_spectrograms)

    def flush(self, vmean=None, vstd=None, return_spectrograms=False):
        """Close the streams as the offline call on the signal zero-padded to the video's length; returns the rest."""
        return ops.stream_flush(self.session, vmean, vstd, return_spectrograms)

    def reset(self):
        ops.stream_reset(self.session)
        self._busy = set()

    # ---- independent streams: the slots of one session serve callers that never move together ----
    def push_each(self, samples=None, video=None, flush=None, vmean=None, vstd=None, return_spectrograms=False):
        """Every stream by its own amount (ops.stream_push_each): samples / video are lists with one tensor (1-D float32;
        [v, 128, 128, F]) or None per stream, flush a list of bools -> per-stream lists of what push returns.  A stream
        without input costs nothing; each stream's output is, bit for bit, that of a session of its own."""
        return ops.stream_push_each(self.session, samples, video, flush, vmean, vstd, return_spectrograms)

    def reset_streams(self, ids):
        """The listed streams back to the state after construction; the others keep streaming."""
        ops.stream_reset_each(self.session, ids)

    def open(self):
        """-> a free slot (the lowest stream no caller holds) for a caller that joins; close() gives it back."""
        for b in range(self.session.n_streams):
            if b not in self._busy:
                self._busy.add(b)
                return b
        raise RuntimeError(f"all {self.session.n_streams} streams of the session are in use")

    def close(self, slot, vmean=None, vstd=None):
        """A caller hangs up: flushes the slot, resets it and frees it -> its last samples (1-D)."""
        flush = [b == slot for b in range(self.session.n_streams)]
        last = self.push_each(flush=flush, vmean=vmean, vstd=vstd)[slot]
        self.reset_streams([slot])
        self._busy.discard(slot)
        return last

    @property
    def counts(self):
        """Host totals: dict(samples, video_slices, frames, slices, emitted) while the streams are in step, else the
        same keys with one list entry per stream."""
        s = self.session
        if s.in_step:
            f, k, e = ops.stream_counts(s.n, s.v, s.flushed, s)
            return dict(samples=s.n, video_slices=s.v, frames=f, slices=k, emitted=e)
        rows = [ops.stream_counts(n, v, fl, s) for n, v, fl in zip(s.ns, s.vs, s.fl)]
        return dict(samples=list(s.ns), video_slices=list(s.vs), frames=[r[0] for r in rows],
                    slices=[r[1] for r in rows], emitted=[r[2] for r in rows])

    @property
    def range_bits(self):
        """float32_split: the range-guard bits the pushes' forwards raised since the last read (waits for the stream;
        Context.range_status); 0 for the other dtypes."""
        if self.weights.dtype != _lib.AVSE_F32_SPLIT:
            return 0
        return self.weights.ctx.range_status()
