"""Device-level entry points: torch (ROCm) tensors in, torch tensors out, arithmetic in libavse.

Every function here is a thin shape/dtype check around one C-ABI call (include/avse.h) launched
on torch's current HIP stream.  Nothing computes on the CPU.
"""
import ctypes
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from .model import KerasModel, blob_floats

DTYPES = {"float32": _lib.AVSE_F32, "fp32": _lib.AVSE_F32, "bfloat16": _lib.AVSE_BF16, "bf16": _lib.AVSE_BF16,
          # float32 accuracy from split-f16 matrix-core products (include/avse.h AVSE_F32_SPLIT)
          "float32_split": _lib.AVSE_F32_SPLIT, "fp32_split": _lib.AVSE_F32_SPLIT}


def _dev_f32(t, name, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a ROCm device tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape[-len(shape):]) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [..., {shape}]")
    return t


def _dev_video(t, name, shape=None):
    """A video argument: a float32 or uint8 device tensor, checked like _dev_f32 -> its avse_video_dtype.  uint8 crops
    (include/avse.h AVSE_VIDEO_U8) are converted in the kernels, exactly, so they give the float32 call's bits."""
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8):
        _dev_f32(t, name, shape)
        return _lib.AVSE_VIDEO_F32
    if not t.is_cuda:
        raise TypeError(f"{name} must be a ROCm device tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape[-len(shape):]) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [..., {shape}]")
    return _lib.AVSE_VIDEO_U8


def _check_video(rc, what, video):
    """_lib.check for the avse_*_video calls: the library's refusal of a uint8 video that is not 4-byte aligned (the
    one argument error the checks above leave to it) is the caller's ValueError, like the other shape errors."""
    if rc == 1 and video is not None and video.dtype == torch.uint8 and video.data_ptr() % 4:
        raise ValueError(f"{what}: {_lib.load().avse_last_error().decode(errors='replace')}")
    _lib.check(rc, what)


def video_to_device(x, device=None):
    """to_device for video: uint8 crops (numpy or tensor) stay uint8, everything else becomes float32."""
    if (x.dtype == torch.uint8) if isinstance(x, torch.Tensor) else (np.asarray(x).dtype == np.uint8):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        return t.to(dev).contiguous()
    return to_device(x, device)


def n_frames(n_samples, hop, n_fft):
    """Centred STFT frame count (librosa.stft, center=True): 1 + (L + 2*(n_fft//2) - n_fft) // hop."""
    return 1 + (n_samples + 2 * (n_fft // 2) - n_fft) // hop


def spectrogram(sig, sample_rate=16000, n_fft=640, hop_length=160, n_mels=80, fmin=0.0, fmax=8000.0,
                amin=1e-5, top_db=80.0, pad_mode="reflect", frames_per_slice=0, return_stft=False, out=None):
    """K1: STFT -> mel -> dB for a batch of utterances.

    sig [U, L] float32 device tensor.  Returns mel_db [U, n_mels, T] (frames_per_slice == 0) or
    [U, n_slices, n_mels, frames_per_slice] (into `out` when given); with return_stft also the complex64 STFT
    [U, 1+n_fft//2, T].
    """
    _dev_f32(sig, "sig")
    if sig.dim() != 2:
        raise ValueError("sig must be [n_utterances, n_samples]")
    U, L = sig.shape
    T = n_frames(L, hop_length, n_fft)
    shape = (U, T // frames_per_slice, n_mels, frames_per_slice) if frames_per_slice else (U, n_mels, T)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=sig.device)
    else:
        _dev_f32(out, "out")
        if tuple(out.shape) != shape or out.device != sig.device:
            raise ValueError(f"out must be {shape} on {sig.device}")
    stft = torch.empty((U, 1 + n_fft // 2, T, 2), dtype=torch.float32, device=sig.device) if return_stft else None
    pm = {"reflect": _lib.AVSE_PAD_REFLECT, "constant": _lib.AVSE_PAD_CONSTANT}[pad_mode]
    if U == 0:   # empty batch: empty outputs (the C-ABI takes no NULL buffers, even for zero utterances)
        return (out, torch.view_as_complex(stft)) if return_stft else out
    ctx = _lib.context(sig.device)
    with torch.cuda.device(sig.device):
        _lib.check(_lib.load().avse_spectrogram(
            ctx.handle, _lib.ptr(sig), U, L, int(sample_rate), int(n_fft), int(hop_length), int(n_mels),
            float(fmin), float(fmax), float(amin), float(-1.0 if top_db is None else top_db), pm,
            int(frames_per_slice), _lib.ptr(out), _lib.ptr(stft), _lib.stream_handle(sig.device)), "avse_spectrogram")
    if return_stft:
        return out, torch.view_as_complex(stft)
    return out


def istft(mel_db, stft, sample_rate=16000, n_fft=640, hop_length=160, n_mels=80, fmin=0.0, fmax=8000.0,
          n_frames=None):
    """K6: speech mel-dB + mixture STFT -> time signal (reconstruct_signal_from_spectrogram).

    mel_db: [U, n_slices, n_mels, spf] (network output of consecutive slices) or [U, n_mels, T];
    stft: complex64 [U, n_fft//2+1, T_stft] (or its float32 [..., 2] view) from spectrogram(return_stft=True).
    Uses the first n_frames = min(T_pred, T_stft) frames (data_processor.py:68-70).
    Returns [U, hop * (n_frames - 1)] float32."""
    _dev_f32(mel_db, "mel_db")
    if stft.dtype == torch.complex64:
        stft = torch.view_as_real(stft)
    _dev_f32(stft, "stft")
    if mel_db.dim() == 4:
        U, ns, nm, spf = mel_db.shape
        T_pred = ns * spf
    else:
        U, nm, T_pred = mel_db.shape
        spf = 0
    if nm != n_mels or stft.shape[0] != U or stft.shape[1] != n_fft // 2 + 1:
        raise ValueError("mel_db / stft shapes do not match")
    T_stft = stft.shape[2]
    T = min(T_pred, T_stft) if n_frames is None else n_frames
    if T != T_pred:
        # min() cut the prediction: use the [U, n_mels, T] layout of the concatenated, trimmed slices
        if spf:
            mel_db = mel_db.permute(0, 2, 1, 3).reshape(U, nm, T_pred)
        mel_db = mel_db[:, :, :T].contiguous()
        spf = 0
    out = torch.empty((U, hop_length * (T - 1)), dtype=torch.float32, device=mel_db.device)
    if U == 0:
        return out
    ctx = _lib.context(mel_db.device)
    with torch.cuda.device(mel_db.device):
        _lib.check(_lib.load().avse_istft(ctx.handle, _lib.ptr(mel_db), _lib.ptr(stft), U, int(T), int(T_stft), int(spf),
                                          int(sample_rate), int(n_fft), int(hop_length), int(n_mels), float(fmin),
                                          float(fmax), _lib.ptr(out), _lib.stream_handle(mel_db.device)), "avse_istft")
    return out


def _ragged_signals(sigs):
    """spectrogram_ragged's signal argument -> (1-D float32 device buffer, int64 offsets [U], int64 lengths [U]):
    a list of 1-D float32 device tensors (packed here, tightly), or a (buffer, offsets, lengths) triple whose offsets
    and lengths are integer sequences (any offsets: packed utterances, or the rows of a [U, stride] buffer)."""
    if isinstance(sigs, tuple) and len(sigs) == 3 and isinstance(sigs[0], torch.Tensor) and \
            not (isinstance(sigs[1], torch.Tensor) and sigs[1].is_floating_point()):
        buf, off, lens = sigs
        _dev_f32(buf, "sigs[0]")
        off, lens = (np.ascontiguousarray(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x), dtype=np.int64)
                     for x in (off, lens))
        if off.ndim != 1 or off.shape != lens.shape:
            raise ValueError("offsets and lengths must be 1-D and of one size")
        if off.size and (off.min() < 0 or lens.min() < 0 or (off + lens).max() > buf.numel()):
            raise ValueError("an utterance lies outside the buffer")
        return buf.view(-1), off, lens
    sigs = list(sigs)
    for k, t in enumerate(sigs):
        _dev_f32(t, f"sigs[{k}]")
        if t.dim() != 1:
            raise ValueError(f"sigs[{k}] must be 1-D, got shape {tuple(t.shape)}")
    lens = np.array([t.numel() for t in sigs], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(sigs) else np.zeros(0, np.int64)
    if not sigs:
        raise ValueError("spectrogram_ragged needs at least one utterance")
    return torch.cat(sigs), off, lens


class RaggedViews:
    """The per-utterance views of a packed buffer as a read-only sequence: view u is built when it is asked for (a
    Tensor.view per utterance up front costs more host time than the launch it follows at small sizes).
    `shapes[u]` is view u's shape without building it."""

    def __init__(self, packed, sizes, shapes):
        self.packed, self.shapes = packed, shapes
        self._ends = np.cumsum(sizes)
        self._sizes = sizes

    def __len__(self):
        return len(self.shapes)

    def __getitem__(self, u):
        if isinstance(u, slice):
            return [self[k] for k in range(*u.indices(len(self)))]
        u = range(len(self))[u]
        e = int(self._ends[u])
        return self.packed[e - int(self._sizes[u]):e].view(self.shapes[u])

    def __iter__(self):
        return (self[u] for u in range(len(self)))


def spectrogram_ragged(sigs, sample_rate=16000, n_fft=640, hop_length=160, n_mels=80, fmin=0.0, fmax=8000.0,
                       amin=1e-5, top_db=80.0, pad_mode="reflect", frames_per_slice=0, return_stft=False):
    """K1 for utterances of mixed lengths in one avse_spectrogram_ragged call: each utterance's result is the bits
    spectrogram() gives for it alone (its own padding, trailing frames and top_db floor).

    sigs: a list of 1-D float32 device tensors, or (buffer, offsets, lengths).  Returns (mel, counts, views):
    (views: a RaggedViews sequence, each view built on access)
    frames_per_slice == 0: mel is the 1-D packed buffer, counts the frames T_u, views[u] its [n_mels, T_u] block;
    frames_per_slice  > 0: mel is [sum S_u, n_mels, frames_per_slice] (forward()'s input as it stands), counts the
    slices S_u = T_u // frames_per_slice (0 is legal: an empty view), views[u] = mel[its slices].
    With return_stft also (stft, stft_views): the packed 1-D complex64 STFT and the [1 + n_fft // 2, T_u] blocks."""
    buf, off, lens = _ragged_signals(sigs)
    U = int(lens.size)
    dev = buf.device
    spf = int(frames_per_slice)
    if spf < 0:
        raise ValueError("frames_per_slice < 0")
    nb = 1 + n_fft // 2
    T = n_frames(lens, hop_length, n_fft)             # (numpy, per utterance)
    counts = T // spf if spf else T
    sizes = counts * (n_mels * spf) if spf else T * n_mels
    total, stotal = int(sizes.sum()), int(T.sum()) * nb
    packed = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    mel = packed[:total]
    stft = torch.empty((max(stotal, 1), 2), dtype=torch.float32, device=dev) if return_stft else None
    pm = {"reflect": _lib.AVSE_PAD_REFLECT, "constant": _lib.AVSE_PAD_CONSTANT}[pad_mode]
    if U:
        ctx = _lib.context(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().avse_spectrogram_ragged(
                ctx.handle, _lib.ptr(buf), off.ctypes.data, lens.ctypes.data, U, int(sample_rate), int(n_fft),
                int(hop_length), int(n_mels), float(fmin), float(fmax), float(amin),
                float(-1.0 if top_db is None else top_db), pm, spf, _lib.ptr(packed), _lib.ptr(stft),
                _lib.stream_handle(dev)), "avse_spectrogram_ragged")
    Tl = T.tolist()
    if spf:
        views = RaggedViews(mel, sizes, [(c, n_mels, spf) for c in counts.tolist()])
        mel = mel.view(-1, n_mels, spf)
    else:
        views = RaggedViews(mel, sizes, [(n_mels, t) for t in Tl])
    if not return_stft:
        return mel, counts, views
    cstft = torch.view_as_complex(stft)[:stotal]
    return mel, counts, views, cstft, RaggedViews(cstft, T * nb, [(nb, t) for t in Tl])


def istft_ragged(mel_packed, counts, stft_packed, stft_frames, sample_rate=16000, n_fft=640, hop_length=160, n_mels=80,
                 fmin=0.0, fmax=8000.0):
    """K6 for utterances of mixed lengths in one avse_istft_ragged call: utterance u's signal is the bits istft() gives
    for it alone.

    mel_packed: [sum S_u, n_mels, spf] (forward()'s output for the concatenated slices; counts = the slices S_u, so
    n_frames_u = S_u * spf) or the 1-D packed [n_mels, T_u] blocks (counts = the frames T_u).  stft_packed: the packed
    complex64 STFT of spectrogram_ragged (or its float32 [..., 2] view), stft_frames its frames per utterance; every
    n_frames_u <= stft_frames[u].  Returns a list of views of one packed output, hop * (n_frames_u - 1) samples each
    (none for n_frames_u < 2)."""
    _dev_f32(mel_packed, "mel_packed")
    if stft_packed.dtype == torch.complex64:
        stft_packed = torch.view_as_real(stft_packed)
    _dev_f32(stft_packed, "stft_packed")
    counts = np.ascontiguousarray(np.asarray(counts), dtype=np.int64)
    sf = np.ascontiguousarray(np.asarray(stft_frames), dtype=np.int64)
    if counts.ndim != 1 or counts.shape != sf.shape:
        raise ValueError("counts and stft_frames must be 1-D and of one size")
    if mel_packed.dim() == 3:
        if mel_packed.shape[1] != n_mels:
            raise ValueError("mel_packed / n_mels do not match")
        spf = int(mel_packed.shape[2])
        nf = counts * spf
    elif mel_packed.dim() == 1:
        spf = 0
        nf = counts.copy()
    else:
        raise ValueError("mel_packed must be [slices, n_mels, spf] or the 1-D packed [n_mels, T] blocks")
    nb = 1 + n_fft // 2
    U = int(counts.size)
    if U and (counts.min() < 0 or sf.min() < 0):
        raise ValueError("negative counts")
    if int(nf.sum()) * n_mels != mel_packed.numel() or int(sf.sum()) * nb * 2 != stft_packed.numel():
        raise ValueError("counts / stft_frames do not add up to the packed buffers")
    sizes = np.where(nf >= 2, hop_length * (nf - 1), 0)
    dev = mel_packed.device
    total = int(sizes.sum())
    packed = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    if U and mel_packed.numel() and stft_packed.numel():
        ctx = _lib.context(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().avse_istft_ragged(
                ctx.handle, _lib.ptr(mel_packed), _lib.ptr(stft_packed), nf.ctypes.data, sf.ctypes.data, U, spf,
                int(sample_rate), int(n_fft), int(hop_length), int(n_mels), float(fmin), float(fmax),
                _lib.ptr(packed), _lib.stream_handle(dev)), "avse_istft_ragged")
    return list(packed[:total].split(sizes.tolist()))


def act_exponent(model, layer):
    """The AVSE_F32_SPLIT activation exponent rule of csrc/weight_pack.cpp act_exponents for one layer: with M =
    max_c (|beta_c| + |gamma_c|) of its BatchNormalization, 0 for M in [2^-2, 2^8], else 3 - ceil-exponent(M) (M 2^e in
    (4, 8]), clamped to [-24, 24]."""
    g = np.abs(np.asarray(model.tensors[layer + "_bn/gamma"], np.float64))
    b = np.abs(np.asarray(model.tensors[layer + "_bn/beta"], np.float64))
    m = float(np.max(b + g))
    if not m > 0.0 or not np.isfinite(m) or 0.25 <= m <= 256.0:
        return 0
    return int(max(-24, min(24, 3 - np.frexp(m)[1])))


def _warn_concat_exponents(model):
    """a_conv5 and v_conv6 write the two halves of one concat row that enc_dense reads as one K, so they share one
    exponent, the smaller (weight_pack.cpp act_exponents).  When the halves' own rules disagree, the half that wanted the larger
    exponent is stored with fewer than the pairs' ~22 bits (its lo pieces run into the f16 subnormals): flag it at load
    time — the range guard reports overflow and NaN, not this precision loss."""
    ea, ev = act_exponent(model, "a_conv5"), act_exponent(model, "v_conv6")
    if ea != ev:
        import warnings
        warnings.warn(f"float32_split: the concat halves want activation exponents {ea} (a_conv5) and {ev} (v_conv6); "
                      f"both are stored at {min(ea, ev)}, so the {'audio' if ea > ev else 'video'} half's activations "
                      f"lose precision (BatchNormalization parameters outside [2^-2, 2^8]); use dtype float32 for exact "
                      "fp32 if that matters", RuntimeWarning, stacklevel=3)


class DeviceWeights:
    """avse_weights: BN-folded, GEMM-packed weights resident on one device."""

    def __init__(self, model, dtype="float32", device=None):
        if not isinstance(model, KerasModel):
            raise TypeError("model must be a KerasModel")
        self.dtype = DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
        self.ctx = _lib.context(device)
        self.T, self.F = model.T, model.F
        self.last_range_bits = 0
        if self.dtype == _lib.AVSE_F32_SPLIT:
            _warn_concat_exponents(model)
        blob = model.to_blob()
        # the CDLL is held here: at interpreter exit the module globals may be gone before this object
        self._cdll = _lib.load()
        assert blob.size == blob_floats(self.T, self.F) == self._cdll.avse_weights_blob_floats_shape(self.T, self.F)
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(self.ctx.device_index):
            _lib.check(_lib.load().avse_weights_load_shape(self.ctx.handle, blob.ctypes.data_as(ctypes.c_void_p),
                                                           blob.size, self.dtype, self.T, self.F,
                                                           ctypes.byref(self.handle)), "avse_weights_load_shape")

    @property
    def audio_shape(self):
        return (80, self.T)

    def act_exponents(self):
        """avse_weights_act_exponents: per plan layer, the power-of-two exponent its split-pair activations carry."""
        e = (ctypes.c_int * 20)()
        _lib.check(self._cdll.avse_weights_act_exponents(self.handle, e, 20), "avse_weights_act_exponents")
        return dict(zip(_lib.LAYER_NAMES, list(e)))

    def __del__(self):
        h, lib = getattr(self, "handle", None), getattr(self, "_cdll", None)
        if h is not None and h.value and lib is not None:
            lib.avse_weights_destroy(h)
            self.handle = None


def present_mask(video_present, n, video_rows, what="video_present"):
    """A video_present argument as the host uint8 array [n] libavse reads: a host bool array or sequence of length n,
    `video_rows` (None: no video given) of them set.  Shapes only, so a bad mask is a ValueError before any device or
    library work."""
    if isinstance(video_present, torch.Tensor):
        if video_present.is_cuda:
            raise TypeError(f"{what} is host data: a numpy array, a sequence or a CPU tensor")
        video_present = video_present.numpy()
    m = np.asarray(video_present)
    if m.ndim != 1 or m.shape[0] != n:
        raise ValueError(f"{what} has shape {m.shape}, expected [{n}]")
    m = np.ascontiguousarray(m.astype(bool), dtype=np.uint8)
    if int(m.sum()) != (0 if video_rows is None else int(video_rows)):
        raise ValueError(f"{what} marks {int(m.sum())} clips with video but video has "
                         f"{'no' if video_rows is None else int(video_rows)} rows: video is packed, one row per marked clip")
    return m


def _check_forward_args(weights, audio, video, vnorm_mean, vnorm_std, present=None):
    _dev_f32(audio, "audio", (80, weights.T))
    N = audio.shape[0]
    vdt = _lib.AVSE_VIDEO_F32      # video=None: either dtype
    if video is not None:
        vdt = _dev_video(video, "video", (128, 128, weights.F))
        if present is None and video.shape[0] != N:
            raise ValueError("audio and video batch sizes differ")
    if (vnorm_mean is None) != (vnorm_std is None):
        raise ValueError("vnorm_mean and vnorm_std must both be given")
    if vnorm_mean is not None:
        if video is None and present is None:   # a mixed caller always carries its normaliser
            raise ValueError("video=None (all-zero video) takes no normaliser")
        _dev_f32(vnorm_mean, "vnorm_mean", (128, 128))
        _dev_f32(vnorm_std, "vnorm_std", (128, 128))
    devs = {weights.ctx.device_index, audio.device.index} | ({video.device.index} if video is not None else set())
    if len(devs) != 1:
        raise ValueError(f"weights live on cuda:{weights.ctx.device_index} but audio / video are on "
                         f"{audio.device} / {None if video is None else video.device}")
    return N, vdt


def forward(weights, audio, video, vnorm_mean=None, vnorm_std=None, out=None, checked=False, on_range="recompute",
            video_present=None):
    """K2-K5: network forward.  audio [N, 80, 20], video [N, 128, 128, 5] float32 device tensors
    (video un-normalised when vnorm_* are given; video may also be the crops' uint8 values, 4-byte aligned: the
    result is the float32 call's, bit for bit).  Returns [N, 80, 20] float32.  ([N, 80, T] / [N, 128, 128, F]
    for weights of another network shape, e.g. T = 24 at 29.97 fps.)

    video=None means an all-zero video input (BASELINE configs[2], the audio branch alone): the video
    encoder's output is then one constant vector, computed once per weights object and broadcast.

    checked=False (default): plain asynchronous avse_forward on torch's current stream, capturable in a graph; a
    float32_split forward leaves its range-guard bits in the context for Context.range_status / RangePipeline.
    checked=True: avse_forward_checked — BLOCKS the host until the stream has run the forward and, when an activation
    left the f16 pair range, recomputes the batch on the exact-fp32 kernels (on_range="recompute") or raises
    _lib.RangeError (on_range="error"); not allowed while the stream is capturing.  weights.last_range_bits holds the
    guard bits of the last checked call (0: every pair in range).  The synchronous reference-shaped API
    (network.SpeechEnhancementNetwork.predict / evaluate, the CLI predict) opts in for float32_split weights.

    video_present=mask (avse_forward_mixed): a host bool array or sequence [N], True where the clip has video.  video
    is then PACKED: mask.sum() rows, the clips with video in order (None when there are none); vnorm_* apply to them.
    A clip without video is the all-zero normalised input, so with float32 and float32_split weights out[i] has the
    bits of forward(video)[i] where the mask is set and of forward(video=None)[i] where it is not.  The network was not
    trained with missing video: the quality of its audio-only estimate is unmeasured.  Such a call is asynchronous but
    not capturable, unless the mask is all True or all False."""
    present = None
    if video_present is not None:
        if not isinstance(audio, torch.Tensor) or audio.dim() < 1:
            raise TypeError("audio must be a ROCm device tensor")
        present = present_mask(video_present, audio.shape[0], None if video is None else video.shape[0])
    N, vdt = _check_forward_args(weights, audio, video, vnorm_mean, vnorm_std, present)
    if out is None:
        out = torch.empty((N, 80, weights.T), dtype=torch.float32, device=audio.device)
    _dev_f32(out, "out", (80, weights.T))
    if out.device != audio.device or out.shape[0] != N:
        raise ValueError(f"out must be [N, 80, {weights.T}] on the inputs' device")
    if N == 0:
        return out
    with torch.cuda.device(audio.device):
        if checked:
            mode = {"recompute": _lib.AVSE_RANGE_RECOMPUTE, "error": _lib.AVSE_RANGE_ERROR}[on_range]
            bits = ctypes.c_uint32()
            if present is not None:
                rc = _lib.load().avse_forward_mixed_checked(
                    weights.ctx.handle, weights.handle, _lib.ptr(audio), _lib.ptr(video), vdt, _lib.ptr(vnorm_mean),
                    _lib.ptr(vnorm_std), present.ctypes.data_as(ctypes.c_void_p), N, _lib.ptr(out),
                    _lib.stream_handle(audio.device), mode, ctypes.byref(bits))
            else:
                rc = _lib.load().avse_forward_checked_video(
                    weights.ctx.handle, weights.handle, _lib.ptr(audio), _lib.ptr(video), vdt, _lib.ptr(vnorm_mean),
                    _lib.ptr(vnorm_std), N, _lib.ptr(out), _lib.stream_handle(audio.device), mode, ctypes.byref(bits))
            weights.last_range_bits = bits.value
            _check_video(rc, "avse_forward_checked", video)
            if bits.value:
                import warnings
                warnings.warn(f"float32_split forward of {N} clips: {_lib.range_bit_names(bits.value)} left the f16 pair "
                              "range; the batch was recomputed on the exact-fp32 kernels", RuntimeWarning, stacklevel=2)
        elif present is not None:
            # the library reads `present` during the call (it builds the row map from it): nothing to keep alive
            _check_video(_lib.load().avse_forward_mixed(
                weights.ctx.handle, weights.handle, _lib.ptr(audio), _lib.ptr(video), vdt, _lib.ptr(vnorm_mean),
                _lib.ptr(vnorm_std), present.ctypes.data_as(ctypes.c_void_p), N, _lib.ptr(out),
                _lib.stream_handle(audio.device)), "avse_forward_mixed", video)
        else:
            _check_video(_lib.load().avse_forward_video(
                weights.ctx.handle, weights.handle, _lib.ptr(audio), _lib.ptr(video), vdt, _lib.ptr(vnorm_mean),
                _lib.ptr(vnorm_std), N, _lib.ptr(out), _lib.stream_handle(audio.device)), "avse_forward", video)
    return out


class RangePipeline:
    """Deferred range verification of unchecked float32_split forwards (avse_range_snapshot): after each forward,
    `submit(recompute)` enqueues a snapshot of the context's range guard into a pinned host word and an event; the
    snapshot of batch k is read once the stream has passed it — at the `depth`-th later submit, or at `drain()` — so the
    host never waits for the batch it just enqueued (avse_forward_checked waits for every batch before the next is
    launched).  A batch whose bits are set is recomputed by its `recompute` callable (e.g. ops.forward(...,
    checked=True) into the same output, which must then still hold that batch's inputs); `bits` accumulates every
    batch's guard bits and `recomputed` counts the batches redone."""

    def __init__(self, ctx, depth=2):
        self.ctx = ctx
        self.depth = max(1, int(depth))
        self.words = torch.zeros(self.depth, dtype=torch.int32, pin_memory=True)
        self.events = [torch.cuda.Event() for _ in range(self.depth)]
        self.pending = []
        self.k = 0
        self.bits = 0
        self.recomputed = 0

    def submit(self, recompute=None):
        slot = self.k % self.depth
        if len(self.pending) == self.depth:
            self._retire()
        dev = torch.device("cuda", self.ctx.device_index)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().avse_range_snapshot(self.ctx.handle, _lib.stream_handle(dev),
                                                       ctypes.c_void_p(self.words.data_ptr() + 4 * slot)),
                       "avse_range_snapshot")
            self.events[slot].record()
        self.pending.append((slot, recompute))
        self.k += 1

    def _retire(self):
        slot, recompute = self.pending.pop(0)
        self.events[slot].synchronize()
        b = int(self.words[slot].item()) & 0xFFFFFFFF
        if b:
            self.bits |= b
            if recompute is not None:
                recompute()
                self.recomputed += 1

    def drain(self):
        while self.pending:
            self._retire()
        return self.bits


def forward_profile(weights, audio, video, vnorm_mean=None, vnorm_std=None, out=None):
    """forward() with HIP events between kernel launches (synchronises); returns (out, {stage: ms})."""
    N, vdt = _check_forward_args(weights, audio, video, vnorm_mean, vnorm_std)
    if out is None:
        out = torch.empty((N, 80, weights.T), dtype=torch.float32, device=audio.device)
    ms = (ctypes.c_float * _lib.AVSE_NUM_STAGES)()
    with torch.cuda.device(audio.device):
        _check_video(_lib.load().avse_forward_profile_video(
            weights.ctx.handle, weights.handle, _lib.ptr(audio), _lib.ptr(video), vdt, _lib.ptr(vnorm_mean),
            _lib.ptr(vnorm_std), N, _lib.ptr(out), _lib.stream_handle(audio.device), ms), "avse_forward_profile", video)
    return out, dict(zip(_lib.STAGE_NAMES, [float(x) for x in ms]))


def video_normalize_(video, mean, std):
    """In place: video[s, :, :, f] = (video[s, :, :, f] - mean) / std (data_processor.py:208-212)."""
    if isinstance(video, torch.Tensor) and video.dtype == torch.uint8:
        raise TypeError("video must be float32, got torch.uint8: uint8 video cannot be normalised in place; it takes "
                        "the normaliser fused, by passing it to predict (ops.forward's vnorm_mean / vnorm_std)")
    _dev_f32(video, "video")
    _dev_f32(mean, "mean")
    _dev_f32(std, "std")
    S, H, W, F = video.shape
    if S == 0:
        return video
    ctx = _lib.context(video.device)
    with torch.cuda.device(video.device):
        _lib.check(_lib.load().avse_video_normalize(ctx.handle, _lib.ptr(video), S, H, W, F, _lib.ptr(mean),
                                                    _lib.ptr(std), _lib.stream_handle(video.device)),
                   "avse_video_normalize")
    return video


def video_stats(video):
    """VideoNormalizer's fit (data_processor.py:203-206) on the device: video [S, H, W, F] float32 device tensor ->
    (mean [H, W], std [H, W]) float32 device tensors, np.mean / np.std over axes (0, 3) from one streaming read
    (float64 sums about each pixel's first value, include/avse.h avse_video_stats).  uint8 video (4-byte aligned):
    exact integer sums (avse_video_stats_video)."""
    vdt = _dev_video(video, "video")
    if video.dim() != 4:
        raise ValueError("video must be [slices, height, width, frames_per_slice]")
    S, H, W, F = video.shape
    if 0 in (S, H, W, F):
        raise ValueError("video_stats of an empty video")
    mean = torch.empty((H, W), dtype=torch.float32, device=video.device)
    std = torch.empty((H, W), dtype=torch.float32, device=video.device)
    ctx = _lib.context(video.device)
    with torch.cuda.device(video.device):
        _check_video(_lib.load().avse_video_stats_video(ctx.handle, _lib.ptr(video), vdt, S, H, W, F, _lib.ptr(mean),
                                                        _lib.ptr(std), _lib.stream_handle(video.device)),
                     "avse_video_stats", video)
    return mean, std


def _is_packed(x):
    """A (samples tensor, int64 offsets) tuple, as against a sequence of signals (whose entries must be int16)."""
    if not (isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], torch.Tensor)):
        return False
    dt = x[1].dtype if isinstance(x[1], (torch.Tensor, np.ndarray)) else np.asarray(x[1]).dtype
    return dt in (torch.int64, np.dtype(np.int64))


def _int16_signals(x, name):
    """The host-side check of mix_pairs' signal arguments, before anything touches a device: a sequence of mono int16
    signals (1-D, or [n, 1]; numpy or tensors) -> (list of 1-D signals, int64 offsets [U + 1]); or an already packed
    pair (1-D int16 device tensor, int64 offsets) -> (tensor, offsets).  Anything else is a TypeError."""
    if _is_packed(x):
        packed, off = x
        if packed.dtype != torch.int16:
            raise TypeError(f"{name}: the packed samples must be int16, got {packed.dtype}")
        if not packed.is_cuda or not packed.is_contiguous():
            raise TypeError(f"{name}: the packed samples must be a contiguous ROCm device tensor")
        off = np.ascontiguousarray(np.asarray(off.cpu() if isinstance(off, torch.Tensor) else off), dtype=np.int64)
        if off.ndim != 1 or off.size < 1 or off[0] < 0 or np.any(np.diff(off) < 0) or off[-1] > packed.numel():
            raise ValueError(f"{name}: offsets must be [U + 1] non-decreasing element offsets into the packed samples")
        return packed, off
    sigs = []
    for k, a in enumerate(x):
        if not isinstance(a, torch.Tensor):
            a = np.asarray(a)
        dt = a.dtype
        if dt not in (torch.int16, np.dtype(np.int16)):
            raise TypeError(f"{name}[{k}] must hold int16 samples, got {dt}")
        if a.ndim == 2 and a.shape[1] == 1:
            a = a[:, 0]
        if a.ndim != 1:
            raise TypeError(f"{name}[{k}] must be one channel of samples, got shape {tuple(a.shape)}")
        sigs.append(a)
    off = np.zeros(len(sigs) + 1, dtype=np.int64)
    np.cumsum([a.shape[0] for a in sigs], out=off[1:])
    return sigs, off


def _pack_int16(sigs, dev):
    """_int16_signals' first result -> one 1-D int16 tensor on `dev` (never empty: the C-ABI takes no NULL buffer)."""
    if isinstance(sigs, torch.Tensor):
        packed = sigs
    elif all(isinstance(a, np.ndarray) for a in sigs):
        packed = torch.from_numpy(np.concatenate(sigs) if sigs else np.zeros(0, np.int16)).to(dev)
    else:
        packed = torch.cat([a.to(dev) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                            for a in sigs])
    if packed.numel() == 0:
        packed = torch.zeros(1, dtype=torch.int16, device=dev)
    return packed


def mix_pairs(speech, noise, L, snr_db=0, return_mix64=True, device=None):
    """The pair mixing of preprocess_audio_pair (data_processor.py:119-139) for a ragged group of U pairs in one
    avse_mix_pairs call: each noise looped cyclically to its speech's length, scaled by AudioMixer.snr_factor for
    snr_db (a number, or one per pair), added to the speech, everything padded / truncated to L samples.

    speech / noise: a sequence of mono int16 signals (numpy or tensors, 1-D or [n, 1]), or a packed pair
    (1-D int16 device tensor, int64 offsets [U + 1]).  Multi-channel or non-int16 input raises TypeError.
    Returns (rows [3, U, L] float32: mixture, speech, scaled noise; mix64 [U, L] float64 or None; factor [U] float64),
    device tensors equal to the numpy path's float64 results (and their float32 casts) bit for bit for utterances
    below 2^23 samples (include/avse.h).  rows.view(3 * U, L) feeds spectrogram()."""
    sp, so = _int16_signals(speech, "speech")
    nz, no = _int16_signals(noise, "noise")
    U = so.size - 1
    if no.size - 1 != U:
        raise ValueError(f"{U} speech signals but {no.size - 1} noise signals")
    L = int(L)
    if L <= 0:
        raise ValueError("L must be positive")
    if np.any(np.diff(so) == 0):
        raise _lib.AvseError("avse_mix_pairs refused (status 1, AVSE_ERR_INVALID): speech signal "
                             f"{int(np.argmin(np.diff(so)))} is empty")
    if np.ndim(snr_db) == 0:
        snr_lin = None if float(snr_db) == 0.0 else np.full(U, 10.0 ** (snr_db / 10.0), dtype=np.float64)
    else:
        if len(snr_db) != U:
            raise ValueError(f"snr_db has {len(snr_db)} entries for {U} pairs")
        snr_lin = np.array([10.0 ** (d / 10.0) for d in snr_db], dtype=np.float64)
    for t in (sp, nz):
        if isinstance(t, torch.Tensor) and device is None:
            device = t.device
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    ctx = _lib.context(dev)
    rows = torch.empty((3, U, L), dtype=torch.float32, device=dev)
    mix64 = torch.empty((U, L), dtype=torch.float64, device=dev) if return_mix64 else None
    factor = torch.empty((U,), dtype=torch.float64, device=dev)
    if U == 0:
        return rows, mix64, factor
    sp, nz = _pack_int16(sp, dev), _pack_int16(nz, dev)
    so_d, no_d = torch.from_numpy(so).to(dev), torch.from_numpy(no).to(dev)
    lin_d = torch.from_numpy(snr_lin).to(dev) if snr_lin is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().avse_mix_pairs(ctx.handle, _lib.ptr(sp), _lib.ptr(so_d), _lib.ptr(nz), _lib.ptr(no_d),
                                              _lib.ptr(lin_d), U, L, _lib.ptr(rows), _lib.ptr(mix64), _lib.ptr(factor),
                                              _lib.stream_handle(dev)), "avse_mix_pairs")
    return rows, mix64, factor


def _eval_signals(x, name):
    """eval_pairs' signal argument -> a list of 1-D signals (numpy arrays or tensors, int16 or floating point):
    a sequence of 1-D (or [n, 1]) signals, or one 2-D array / tensor whose rows are the signals."""
    if isinstance(x, (np.ndarray, torch.Tensor)):
        if x.ndim != 2:
            raise TypeError(f"{name}: a single array must be 2-D [pairs, samples]; pass a list for ragged signals")
        x = list(x)
    sigs = []
    for k, a in enumerate(x):
        if not isinstance(a, torch.Tensor):
            a = np.asarray(a)
        floating = a.dtype.is_floating_point if isinstance(a, torch.Tensor) else np.issubdtype(a.dtype, np.floating)
        if not floating and a.dtype not in (torch.int16, np.dtype(np.int16)):
            raise TypeError(f"{name}[{k}] must hold int16 or floating-point samples, got {a.dtype}")
        if a.ndim == 2 and a.shape[1] == 1:
            a = a[:, 0]
        if a.ndim != 1:
            raise TypeError(f"{name}[{k}] must be mono (1-D), got shape {tuple(a.shape)}")
        sigs.append(a)
    return sigs


def _pack_f32(sigs, dev):
    """Signals (already cut) -> one 1-D float32 tensor on `dev`: one concatenation on the side the signals live on."""
    if all(isinstance(a, np.ndarray) for a in sigs):
        return torch.from_numpy(np.concatenate([a.astype(np.float32, copy=False) for a in sigs])).to(dev)
    return torch.cat([(a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)))
                      .to(device=dev, dtype=torch.float32) for a in sigs])


EVAL_MAX_SAMPLES = 1 << 24


def _eval_packed(ref, deg, sample_rate, device):
    """eval_pairs' / eval_pairs_ext's arguments, checked -> (packed ref, packed deg, host offsets [n + 1], device,
    sample rate): every refusal happens before anything touches a device."""
    sr = int(sample_rate)
    if not 8000 <= sr <= 48000:
        raise ValueError(f"sample_rate {sample_rate} outside 8000 .. 48000")
    if _is_packed(ref):
        rp, off = ref
        dp = deg[0] if _is_packed(deg) else deg
        for t, name in ((rp, "ref"), (dp, "deg")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise TypeError(f"{name}: the packed samples must be a ROCm device tensor")
            if t.dtype != torch.float32 or t.ndim != 1 or not t.is_contiguous():
                raise TypeError(f"{name}: the packed samples must be a contiguous 1-D float32 tensor")
        off = np.ascontiguousarray(np.asarray(off.cpu() if isinstance(off, torch.Tensor) else off), dtype=np.int64)
        if off.ndim != 1 or off.size < 2 or off[0] < 0 or np.any(np.diff(off) < 0) or \
                off[-1] > min(rp.numel(), dp.numel()):
            raise ValueError("offsets must be [n + 1] non-decreasing element offsets into both packed buffers")
        dev = rp.device
    else:
        rs, ds = _eval_signals(ref, "ref"), _eval_signals(deg, "deg")
        if len(rs) != len(ds):
            raise ValueError(f"{len(rs)} reference signals but {len(ds)} degraded signals")
        if not rs:
            raise ValueError("eval_pairs needs at least one pair")
        lens = [min(int(a.shape[0]), int(b.shape[0])) for a, b in zip(rs, ds)]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        dev = None
    lens = np.diff(off)
    if np.any(lens == 0):
        raise _lib.AvseError(f"avse_eval_pairs refused (status 1, AVSE_ERR_INVALID): pair {int(np.argmin(lens))} is empty")
    if np.any(lens > EVAL_MAX_SAMPLES):
        raise _lib.AvseError(f"avse_eval_pairs refused (status 1, AVSE_ERR_INVALID): pair {int(np.argmax(lens))} has "
                             f"more than 2^24 samples")
    if dev is None:      # only now: every refusal above happens before anything touches a device
        for t in rs + ds:
            if isinstance(t, torch.Tensor) and t.is_cuda and device is None:
                device = t.device
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        rp = _pack_f32([a[:k] for a, k in zip(rs, lens)], dev)
        dp = _pack_f32([a[:k] for a, k in zip(ds, lens)], dev)
    return rp, dp, off, dev, sr


def eval_pairs(ref, deg, sample_rate=16000, device=None):
    """The evaluate stage (speech_enhancement_evaluator.py:34-64 with open measures in PESQ's place): SNR, SI-SDR,
    segmental SNR and STOI of n (clean, degraded) pairs in one avse_eval_pairs call (include/avse.h has the definitions).

    ref / deg: sequences of mono signals (numpy or tensors, int16 or floating point, ragged), or one 2-D array / tensor
    [n, samples] each; pair u is cut to min(len ref[u], len deg[u]).  Device tensors are packed on the device (no host
    copy).  Or the packed form: ref = (1-D float32 device tensor, int64 offsets [n + 1]) and deg = a 1-D float32 device
    tensor laid out by the same offsets.
    Returns a float64 device tensor [n, 5]: snr, si_sdr, seg_snr, stoi, stoi_kept (_lib.EVAL_METRIC_NAMES)."""
    rp, dp, off, dev, sr = _eval_packed(ref, deg, sample_rate, device)
    n = off.size - 1
    ctx = _lib.context(dev)
    off_d = torch.from_numpy(off).to(dev)
    out = torch.empty((n, _lib.AVSE_EVAL_NMETRICS), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        # the offsets were built here: the scratch is sized for their span, not for the buffers' allocations
        _lib.check(_lib.load().avse_eval_pairs_sized(ctx.handle, _lib.ptr(rp), _lib.ptr(dp), _lib.ptr(off_d), n,
                                                     int(off[-1] - off[0]), sr, _lib.ptr(out),
                                                     _lib.stream_handle(dev)), "avse_eval_pairs")
    return out


def eval_pairs_ext(ref, deg, sample_rate=16000, any_rate=True, device=None):
    """eval_pairs with ESTOI as a sixth column, and (any_rate) STOI, its frame count and ESTOI at every sample rate in
    8000 .. 48000 instead of NaN / 0 where max(up, down) > 24 (44100, 22050, 11025, ..): one avse_eval_pairs_ext call.
    The same inputs and the same refusals as eval_pairs; columns 0 .. 4 are eval_pairs' bits wherever it computes them.
    Returns a float64 device tensor [n, 6]: _lib.EVAL_METRIC_NAMES_EXT."""
    rp, dp, off, dev, sr = _eval_packed(ref, deg, sample_rate, device)
    n = off.size - 1
    ctx = _lib.context(dev)
    off_d = torch.from_numpy(off).to(dev)
    out = torch.empty((n, _lib.AVSE_EVAL_NMETRICS_EXT), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().avse_eval_pairs_ext(ctx.handle, _lib.ptr(rp), _lib.ptr(dp), _lib.ptr(off_d), n,
                                                   int(off[-1] - off[0]), sr,
                                                   _lib.AVSE_EVAL_ANY_RATE if any_rate else 0, _lib.ptr(out),
                                                   _lib.stream_handle(dev)), "avse_eval_pairs_ext")
    return out


def mse(pred, target):
    """Keras mean_squared_error over every element -> 0-dim device tensor."""
    _dev_f32(pred, "pred")
    _dev_f32(target, "target")
    if pred.numel() != target.numel():
        raise ValueError("pred/target sizes differ")
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    ctx = _lib.context(pred.device)
    with torch.cuda.device(pred.device):
        _lib.check(_lib.load().avse_mse(ctx.handle, _lib.ptr(pred), _lib.ptr(target), pred.numel(), _lib.ptr(loss),
                                        _lib.stream_handle(pred.device)), "avse_mse")
    return loss


def to_device(x, device=None):
    """numpy / tensor -> contiguous float32 device tensor (host->device copy only)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def stream_counts(n_samples, n_video_slices, flushed=False, session=None):
    """avse_stream_counts (host only, no GPU): (frames analysed, slices through the network, samples emitted) of a stream
    that has received n_samples samples and n_video_slices video slices (flushed: after its flush).  session=None
    is the 25-fps geometry (n_fft 640, hop 160, 20 frames per slice)."""
    out = [ctypes.c_int64() for _ in range(3)]
    _lib.check(_lib.load().avse_stream_counts(session.handle if session is not None else None, int(n_samples),
                                              int(n_video_slices), int(bool(flushed)), *[ctypes.byref(o) for o in out]),
               "avse_stream_counts")
    return tuple(o.value for o in out)


def stream_supported(sample_rate=16000, n_fft=640, hop_length=160, frames_per_slice=20, n_mels=80, fmin=0.0, fmax=8000.0,
                     return_message=False):
    """avse_stream_supported (host only, no GPU): 0 when stream_create serves this geometry and mel bank (25 fps at 16,
    32 and 48 kHz: n_fft 640 / 1280 / 1920 = 4 hops; 30 fps at 24 and 48 kHz: n_fft 800 / 1600 = 4 hops; 80 bands under
    8 kHz), else the status it would raise with (3:
    unsupported, 1: invalid).  return_message: -> (status, the library's reason; "" for status 0)."""
    lib = _lib.load()
    rc = int(lib.avse_stream_supported(int(sample_rate), int(n_fft), int(hop_length), int(frames_per_slice), int(n_mels),
                                       float(fmin), float(fmax)))
    if not return_message:
        return rc
    return rc, (lib.avse_last_error().decode(errors="replace") if rc else "")


class StreamSession:
    """avse_stream: the device state of n_streams streams (stream_create).  ns / vs / fl are the host totals per stream
    (samples, video slices, flushed), mirroring the library's counters; n / v / flushed are the same as scalars, valid
    while the streams are in step (the lock-step calls keep them so; stream_push_each may not)."""

    def __init__(self, weights, handle, n_streams, spf, video_dtype, max_slices):
        self.weights, self.handle = weights, handle      # the weights (and their context) outlive the session
        self.n_streams, self.spf, self.video_dtype, self.max_slices = n_streams, spf, video_dtype, max_slices
        self.ns, self.vs, self.fl = [0] * n_streams, [0] * n_streams, [False] * n_streams
        self._v_present, self.k_present = None, [[] for _ in range(n_streams)]
        self._cdll = _lib.load()

    @property
    def in_step(self):
        return len(set(zip(self.ns, self.vs, self.fl))) == 1

    def _common(self, values, name):
        if not self.in_step:
            raise RuntimeError(f"StreamSession.{name}: the streams are not in step; read the per-stream lists ns / vs / fl")
        return values[0]

    n = property(lambda self: self._common(self.ns, "n"))
    v = property(lambda self: self._common(self.vs, "v"))
    flushed = property(lambda self: self._common(self.fl, "flushed"))

    def __del__(self):
        h, lib = getattr(self, "handle", None), getattr(self, "_cdll", None)
        if h is not None and h.value and lib is not None:
            lib.avse_stream_destroy(h)
            self.handle = None


def stream_create(weights, n_streams, sample_rate=16000, n_fft=640, hop_length=160, frames_per_slice=20, n_mels=80,
                  fmin=0.0, fmax=8000.0, amin=1e-5, top_db=80.0, video_dtype=torch.float32, max_slices=4):
    """avse_stream_create on the weights' context -> StreamSession.  video_dtype: torch.float32 or torch.uint8, the
    element type every push's video will have.  Geometries the streaming kernels do not serve (29.97 fps, 30 fps at
    16 kHz, 44.1 kHz: stream_supported says which do: 640 / 160 at 16 kHz, 1280 / 320 at 32 kHz, 1920 / 480 at 48 kHz for
    25-fps video, 800 / 200 at 24 kHz and 1600 / 400 at 48 kHz for 30-fps video, with frames_per_slice 24 and the
    [80, 24] x 6-frame weights) raise _lib.AvseError (status 3)."""
    if not isinstance(weights, DeviceWeights):
        raise TypeError("weights must be DeviceWeights")
    if int(n_streams) < 1 or int(max_slices) < 1:
        raise ValueError("n_streams and max_slices must be positive")
    if video_dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"video_dtype must be torch.float32 or torch.uint8, got {video_dtype}")
    vdt = _lib.AVSE_VIDEO_U8 if video_dtype == torch.uint8 else _lib.AVSE_VIDEO_F32
    h = ctypes.c_void_p()
    with torch.cuda.device(weights.ctx.device_index):
        _lib.check(_lib.load().avse_stream_create(
            weights.ctx.handle, weights.handle, int(n_streams), int(sample_rate), int(n_fft), int(hop_length),
            int(frames_per_slice), int(n_mels), float(fmin), float(fmax), float(amin),
            float(-1.0 if top_db is None else top_db), vdt, int(max_slices), ctypes.byref(h)), "avse_stream_create")
    return StreamSession(weights, h, int(n_streams), int(frames_per_slice), vdt, int(max_slices))


def _stream_call(sess, flush, samples, video, vnorm_mean, vnorm_std, return_spectrograms):
    w = sess.weights
    dev = torch.device("cuda", w.ctx.device_index)
    B = sess.n_streams
    n_new = v_new = 0
    if samples is not None:
        _dev_f32(samples, "samples")
        if samples.dim() != 2 or samples.shape[0] != B:
            raise ValueError(f"samples must be [{B}, n]")
        n_new = int(samples.shape[1])
    if video is not None:
        if _dev_video(video, "video", (128, 128, w.F)) != sess.video_dtype:
            raise TypeError(f"video is {video.dtype}, the session was created for the other video dtype")
        if video.dim() != 5 or video.shape[0] != B:
            raise ValueError(f"video must be [{B}, v, 128, 128, {w.F}]")
        v_new = int(video.shape[1])
    if (vnorm_mean is None) != (vnorm_std is None):
        raise ValueError("vnorm_mean and vnorm_std must both be given")
    if vnorm_mean is not None:
        _dev_f32(vnorm_mean, "vnorm_mean", (128, 128))
        _dev_f32(vnorm_std, "vnorm_std", (128, 128))
    for t in (samples, video, vnorm_mean, vnorm_std):
        if t is not None and t.device.index != dev.index:
            raise ValueError(f"the session lives on {dev} but an argument is on {t.device}")
    # what the call will emit, from the host totals (the library keeps no getter for them: n / v mirror its counters).
    # A flush with n > slice * v is refused here by avse_stream_counts, as the library would; a call on a flushed
    # session emits nothing and is left to the library to refuse.
    in_step = sess.in_step
    if not in_step:
        # the streams' counters differ (stream_push_each): the library runs the per-stream step with these counts for
        # every stream, reports the largest count and packs the spectrograms; the results come back per stream
        todo = [flush and not f for f in sess.fl]
        ks, es = _stream_expect(sess, [n_new] * B, [v_new] * B, todo)
        n_out, k_new = max(es), sum(ks)
        mel_shape = (k_new, 80, sess.spf)
    else:
        _, k0, e0 = stream_counts(sess.n, sess.v, sess.flushed, sess)
        k1, e1 = k0, e0
        if not sess.flushed:
            _, k1, e1 = stream_counts(sess.n + n_new, sess.v + v_new, flush, sess)
        n_out, k_new = e1 - e0, k1 - k0
        mel_shape = (B, k_new, 80, sess.spf)
    out = torch.empty((B, n_out), dtype=torch.float32, device=dev)
    mel = pred = None
    if return_spectrograms:
        mel = torch.empty(mel_shape, dtype=torch.float32, device=dev)
        pred = torch.empty_like(mel)
    got = ctypes.c_int64()
    lib = _lib.load()
    with torch.cuda.device(dev):
        if flush:
            rc = lib.avse_stream_flush(sess.handle, _lib.ptr(vnorm_mean), _lib.ptr(vnorm_std), _lib.ptr(out), n_out,
                                       ctypes.byref(got), _lib.ptr(mel), _lib.ptr(pred), _lib.stream_handle(dev))
        else:
            rc = lib.avse_stream_push(sess.handle, _lib.ptr(samples), n_new, n_new, _lib.ptr(video), v_new,
                                      _lib.ptr(vnorm_mean), _lib.ptr(vnorm_std), _lib.ptr(out), n_out, ctypes.byref(got),
                                      _lib.ptr(mel), _lib.ptr(pred), _lib.stream_handle(dev))
    _lib.check(rc, "avse_stream_flush" if flush else "avse_stream_push")
    if got.value != n_out:
        raise _lib.AvseError(f"the session emitted {got.value} samples, the host totals give {n_out}")
    for b in range(B):
        sess.ns[b] += n_new
        sess.vs[b] += v_new
        sess.fl[b] = sess.fl[b] or flush
    if not in_step:
        return _stream_split(out, mel, pred, ks, es, return_spectrograms)
    return (out, mel, pred) if return_spectrograms else out


def _stream_expect(sess, n_new, v_new, flush):
    """Per stream, what a call with these per-stream counts completes and emits: (slices [B], samples [B]), from the host
    totals.  A flush with n > slice * v is refused here by avse_stream_counts, as the library would; input for a flushed
    stream emits nothing and is left to the library to refuse."""
    ks, es = [], []
    for b in range(sess.n_streams):
        _, k0, e0 = stream_counts(sess.ns[b], sess.vs[b], sess.fl[b], sess)
        k1, e1 = k0, e0
        if not sess.fl[b]:
            _, k1, e1 = stream_counts(sess.ns[b] + n_new[b], sess.vs[b] + v_new[b], flush[b], sess)
        ks.append(k1 - k0)
        es.append(e1 - e0)
    return ks, es


def _stream_split(out, mel, pred, ks, es, return_spectrograms):
    """[B, max n_out] and the packed [sum k, 80, spf] spectrograms of a per-stream step -> per-stream lists."""
    outs = [out[b, :e] for b, e in enumerate(es)]
    if not return_spectrograms:
        return outs
    first = np.concatenate([[0], np.cumsum(ks)]).astype(int)
    return (outs, [mel[first[b]:first[b + 1]] for b in range(len(ks))],
            [pred[first[b]:first[b + 1]] for b in range(len(ks))])


def _host_i64(values):
    a = np.ascontiguousarray(values, dtype=np.int64)
    return a, ctypes.c_void_p(a.ctypes.data)


class NoVideo:
    """k video slices without video (camera off, mouth lost, packets late) as an entry of stream_push_each's `video`:
    they carry no bytes, count as video slices everywhere, and are predicted from the all-zero normalised video (the
    network was not trained with missing video; the quality of its audio-only estimate is unmeasured)."""

    def __init__(self, k=1):
        if int(k) != k or int(k) < 0:
            raise ValueError(f"NoVideo(k) needs a slice count k >= 0, got {k!r}")
        self.k = int(k)

    def __repr__(self):
        return f"NoVideo({self.k})"


def _stream_pack_each(session, samples, video, flush, vnorm_mean, vnorm_std):
    """stream_push_each's arguments, checked and packed on the device (one torch.cat each)
    -> (packed samples, offsets [B], n_new [B], packed video, v_new [B], flush [B]); session._v_present is set to the
    host flags [sum v_new] of the slices (None: every slice has video)."""
    w = session.weights
    dev = torch.device("cuda", w.ctx.device_index)
    B = session.n_streams
    samples = [None] * B if samples is None else list(samples)
    video = [None] * B if video is None else list(video)
    flush = [False] * B if flush is None else [bool(f) for f in flush]
    if not (len(samples) == len(video) == len(flush) == B):
        raise ValueError(f"samples, video and flush must have one entry per stream ({B})")
    n_new, v_new, s_parts, v_parts, flags = [], [], [], [], []
    for b in range(B):
        x, vid = samples[b], video[b]
        if x is not None and x.numel():
            _dev_f32(x, f"samples[{b}]")
            if x.dim() != 1:
                raise ValueError(f"samples[{b}] must be 1-D")
            s_parts.append(x)
        n_new.append(0 if x is None else int(x.numel()))
        nv = 0
        # a tensor, None, NoVideo(k), or a list of tensors and NoVideo in arrival order
        for part in (vid if isinstance(vid, (list, tuple)) else [vid]):
            if isinstance(part, NoVideo):
                flags += [0] * part.k
                nv += part.k
            elif part is not None and part.shape[0]:
                if _dev_video(part, f"video[{b}]", (128, 128, w.F)) != session.video_dtype:
                    raise TypeError(f"video[{b}] is {part.dtype}, the session was created for the other video dtype")
                if part.dim() != 4:
                    raise ValueError(f"video[{b}] must be [v, 128, 128, {w.F}]")
                v_parts.append(part)
                flags += [1] * int(part.shape[0])
                nv += int(part.shape[0])
        v_new.append(nv)
    if (vnorm_mean is None) != (vnorm_std is None):
        raise ValueError("vnorm_mean and vnorm_std must both be given")
    if vnorm_mean is not None:
        _dev_f32(vnorm_mean, "vnorm_mean", (128, 128))
        _dev_f32(vnorm_std, "vnorm_std", (128, 128))
    for t in s_parts + v_parts + [vnorm_mean, vnorm_std]:
        if t is not None and t.device.index != dev.index:
            raise ValueError(f"the session lives on {dev} but an argument is on {t.device}")
    packed = torch.cat(s_parts) if s_parts else None
    vpacked = torch.cat(v_parts) if v_parts else None
    off = np.concatenate([[0], np.cumsum(n_new)[:-1]])
    session._v_present = None if all(flags) else np.ascontiguousarray(flags, dtype=np.uint8)
    return packed, off, n_new, vpacked, v_new, flush


def stream_push_each(session, samples=None, video=None, flush=None, vnorm_mean=None, vnorm_std=None,
                     return_spectrograms=False):
    """avse_stream_push_each: every stream moves by its own amount.  samples: a list of B 1-D float32 device tensors
    (None or empty for a stream without new samples), video: a list of B [v, 128, 128, F] tensors in the session's dtype
    (None for a stream without new video), flush: a list of B bools (streams to close as stream_flush does); any of the
    three may be None as a whole.  The inputs are packed on the device (one torch.cat each).  An entry of video may
    also be NoVideo(k), k slices without video, or a list of tensors and NoVideo in arrival order
    (avse_stream_push_each_mixed); session.k_present then says, per stream, which of the slices the call completed had
    video, and stream_blank(session) counts the blank slices received.
    -> a list of B 1-D tensors, stream b's newly final samples; with return_spectrograms also two lists of [k_b, 80, spf]
    tensors, the slices the network saw and predicted for the k_b slices stream b completed in this call.  Asynchronous
    on torch's current stream; a stream without input or flush launches no blocks."""
    packed, off, n_new, vpacked, v_new, flush = _stream_pack_each(session, samples, video, flush, vnorm_mean, vnorm_std)
    out, mel, pred, ks, es = _stream_push_packed(session, packed, off, n_new, vpacked, v_new, flush, vnorm_mean, vnorm_std,
                                                 return_spectrograms, present=session._v_present)
    return _stream_split(out, mel, pred, ks, es, return_spectrograms)


def _stream_push_packed(session, packed, off, n_new, vpacked, v_new, flush, vnorm_mean, vnorm_std, return_spectrograms,
                        present=None):
    """The call of stream_push_each on checked, packed arguments: stream b's n_new[b] samples start at element off[b] of
    the float32 buffer `packed` (any layout: tight, or the rows of a [B, stride] buffer), its v_new[b] video slices lie
    stream-major in `vpacked`.  -> (out [B, max n_out], mel, pred, slices per stream, samples per stream).
    present: host uint8 [sum v_new], 0 for a slice without video (vpacked then holds only the others); None: all have.
    session.k_present is set to the per-stream lists of which completed slices had video."""
    dev = torch.device("cuda", session.weights.ctx.device_index)
    B = session.n_streams
    ks, es = _stream_expect(session, n_new, v_new, flush)
    out = torch.empty((B, max(es)), dtype=torch.float32, device=dev)
    mel = pred = None
    if return_spectrograms:
        mel = torch.empty((sum(ks), 80, session.spf), dtype=torch.float32, device=dev)
        pred = torch.empty_like(mel)
    (_off, p_off), (_n, p_n), (_v, p_v) = _host_i64(off), _host_i64(n_new), _host_i64(v_new)
    fl = np.ascontiguousarray(flush, dtype=np.uint8)
    got, got_k = np.full(B, -1, np.int64), np.full(B, -1, np.int64)
    kp = np.ones(max(1, sum(ks)), np.uint8)
    with torch.cuda.device(dev):
        rc = _lib.load().avse_stream_push_each_mixed(
            session.handle, _lib.ptr(packed), p_off, p_n, _lib.ptr(vpacked), p_v,
            ctypes.c_void_p(present.ctypes.data) if present is not None else None, ctypes.c_void_p(fl.ctypes.data),
            _lib.ptr(vnorm_mean), _lib.ptr(vnorm_std), _lib.ptr(out), int(out.shape[1]), ctypes.c_void_p(got.ctypes.data),
            _lib.ptr(mel), _lib.ptr(pred), ctypes.c_void_p(got_k.ctypes.data), ctypes.c_void_p(kp.ctypes.data),
            _lib.stream_handle(dev))
    _lib.check(rc, "avse_stream_push_each")
    first = np.concatenate([[0], np.cumsum(ks)]).astype(int)
    session.k_present = [[bool(x) for x in kp[first[b]:first[b + 1]]] for b in range(B)]
    if got.tolist() != es or got_k.tolist() != ks:
        raise _lib.AvseError(f"the session emitted {got.tolist()} samples of {got_k.tolist()} slices, the host totals "
                             f"give {es} of {ks}")
    for b in range(B):
        session.ns[b] += n_new[b]
        session.vs[b] += v_new[b]
        session.fl[b] = session.fl[b] or flush[b]
    return out, mel, pred, ks, es


def stream_blank(session):
    """avse_stream_blank: blank slices (NoVideo) received per stream since its last reset, as a list."""
    n = np.zeros(session.n_streams, np.int64)
    _lib.check(_lib.load().avse_stream_blank(session.handle, ctypes.c_void_p(n.ctypes.data)), "avse_stream_blank")
    return n.tolist()


def stream_reset_each(session, streams):
    """avse_stream_reset_each: the listed streams go back to the state after stream_create (their slots are free for new
    callers), ordered on torch's current stream; the others are untouched."""
    which = np.zeros(session.n_streams, np.uint8)
    for b in streams:
        if not 0 <= int(b) < session.n_streams:
            raise ValueError(f"no stream {b} in a session of {session.n_streams}")
        which[int(b)] = 1
    dev = torch.device("cuda", session.weights.ctx.device_index)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().avse_stream_reset_each(session.handle, ctypes.c_void_p(which.ctypes.data),
                                                      _lib.stream_handle(dev)), "avse_stream_reset_each")
    for b in np.flatnonzero(which):
        session.ns[b], session.vs[b], session.fl[b] = 0, 0, False


def stream_state(session):
    """avse_stream_state: the library's per-stream totals -> (samples [B], video slices [B], flushed [B]) as lists."""
    B = session.n_streams
    n, v, f = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.uint8)
    _lib.check(_lib.load().avse_stream_state(session.handle, ctypes.c_void_p(n.ctypes.data), ctypes.c_void_p(v.ctypes.data),
                                             ctypes.c_void_p(f.ctypes.data)), "avse_stream_state")
    return n.tolist(), v.tolist(), [bool(x) for x in f]


def stream_push(session, samples=None, video=None, vnorm_mean=None, vnorm_std=None, return_spectrograms=False):
    """avse_stream_push: samples [B, n] float32 (or None), video [B, v, 128, 128, F] in the session's dtype (or None)
    -> the [B, n_out] samples that became final; with return_spectrograms also the [B, k, 80, spf] slices the network saw
    and predicted for the k slices this call completed.  Asynchronous on torch's current stream.
    On a session whose streams are not in step (after stream_push_each) every stream still receives these counts, and
    the results come back per stream as from stream_push_each: lists of B tensors."""
    return _stream_call(session, False, samples, video, vnorm_mean, vnorm_std, return_spectrograms)


def stream_flush(session, vnorm_mean=None, vnorm_std=None, return_spectrograms=False):
    """avse_stream_flush: closes the streams as the offline call on the zero-padded signal of the video's length and
    returns the remaining samples (stream_push's return values).  Afterwards only stream_reset is legal."""
    return _stream_call(session, True, None, None, vnorm_mean, vnorm_std, return_spectrograms)


def stream_reset(session):
    """avse_stream_reset: back to the state after stream_create, ordered on torch's current stream."""
    dev = torch.device("cuda", session.weights.ctx.device_index)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().avse_stream_reset(session.handle, _lib.stream_handle(dev)), "avse_stream_reset")
    B = session.n_streams
    session.ns, session.vs, session.fl = [0] * B, [0] * B, [False] * B


# ---- sliding sessions: windows at a stride of video frames ----
def slide_supported(sample_rate=16000, n_fft=640, hop_length=160, frames_per_slice=20, video_frames=5, stride=1, n_mels=80,
                    fmin=0.0, fmax=8000.0, return_message=False):
    """avse_slide_supported (host only, no GPU): 0 when slide_create serves this geometry, bank and stride
    (stream_supported's rule, 1 <= stride <= video_frames, frames_per_slice % video_frames == 0), else the status it
    would raise with.  return_message: -> (status, the library's reason; "" for status 0)."""
    lib = _lib.load()
    rc = int(lib.avse_slide_supported(int(sample_rate), int(n_fft), int(hop_length), int(frames_per_slice),
                                      int(video_frames), int(stride), int(n_mels), float(fmin), float(fmax)))
    if not return_message:
        return rc
    return rc, (lib.avse_last_error().decode(errors="replace") if rc else "")


def slide_counts(n_samples, n_video_frames, flushed=False, stride=1, session=None, geometry=None):
    """avse_slide_counts (host only, no GPU): (frames analysed, windows through the network, frames predicted, samples
    emitted) of a stream that has received n_samples samples and n_video_frames video frames.  session: its geometry
    and stride (`stride` is then ignored); else geometry = (n_fft, hop, frames_per_slice, video_frames), by default
    (640, 160, 20, 5), with `stride`."""
    out = [ctypes.c_int64() for _ in range(4)]
    refs = [ctypes.byref(o) for o in out]
    lib = _lib.load()
    if session is not None:
        rc = lib.avse_slide_counts(session.handle, session.stride, int(n_samples), int(n_video_frames),
                                   int(bool(flushed)), *refs)
    elif geometry is not None:
        n_fft, hop, spf, F = (int(x) for x in geometry)
        rc = lib.avse_slide_counts_geom(n_fft, hop, spf, F, int(stride), int(n_samples), int(n_video_frames),
                                        int(bool(flushed)), *refs)
    else:
        rc = lib.avse_slide_counts(None, int(stride), int(n_samples), int(n_video_frames), int(bool(flushed)), *refs)
    _lib.check(rc, "avse_slide_counts")
    return tuple(o.value for o in out)


class SlideSession:
    """avse_slide: the device state of n_streams sliding streams (slide_create).  ns / fs / fl are the host totals per
    stream (samples, video frames, flushed), mirroring the library's counters."""

    def __init__(self, weights, handle, n_streams, spf, stride, video_dtype, max_windows):
        self.weights, self.handle = weights, handle      # the weights (and their context) outlive the session
        self.n_streams, self.spf, self.stride = n_streams, spf, stride
        self.video_dtype, self.max_windows = video_dtype, max_windows
        self.ns, self.fs, self.fl = [0] * n_streams, [0] * n_streams, [False] * n_streams
        self._cdll = _lib.load()

    @property
    def in_step(self):
        return len(set(zip(self.ns, self.fs, self.fl))) == 1

    def __del__(self):
        h, lib = getattr(self, "handle", None), getattr(self, "_cdll", None)
        if h is not None and h.value and lib is not None:
            lib.avse_slide_destroy(h)
            self.handle = None


def slide_create(weights, n_streams, stride=1, sample_rate=16000, n_fft=640, hop_length=160, frames_per_slice=20, n_mels=80,
                 fmin=0.0, fmax=8000.0, amin=1e-5, top_db=80.0, video_dtype=torch.float32, max_windows=8):
    """avse_slide_create on the weights' context -> SlideSession: a streaming session whose network windows start at
    every `stride`-th video frame (1 .. the weights' video frames per slice).  max_windows (1 .. 80): the most windows
    one call may complete per stream, and how many windows either input may run ahead of the other."""
    if not isinstance(weights, DeviceWeights):
        raise TypeError("weights must be DeviceWeights")
    if int(n_streams) < 1 or int(max_windows) < 1:
        raise ValueError("n_streams and max_windows must be positive")
    if video_dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"video_dtype must be torch.float32 or torch.uint8, got {video_dtype}")
    vdt = _lib.AVSE_VIDEO_U8 if video_dtype == torch.uint8 else _lib.AVSE_VIDEO_F32
    h = ctypes.c_void_p()
    with torch.cuda.device(weights.ctx.device_index):
        _lib.check(_lib.load().avse_slide_create(
            weights.ctx.handle, weights.handle, int(n_streams), int(sample_rate), int(n_fft), int(hop_length),
            int(frames_per_slice), int(stride), int(n_mels), float(fmin), float(fmax), float(amin),
            float(-1.0 if top_db is None else top_db), vdt, int(max_windows), ctypes.byref(h)), "avse_slide_create")
    return SlideSession(weights, h, int(n_streams), int(frames_per_slice), int(stride), vdt, int(max_windows))


def _slide_expect(sess, n_new, f_new, flush):
    """Per stream, what a call with these per-stream counts completes and emits: (windows [B], samples [B]), from the
    host totals.  Input for a flushed stream emits nothing and is left to the library to refuse."""
    ws, es = [], []
    for b in range(sess.n_streams):
        _, w0, _, e0 = slide_counts(sess.ns[b], sess.fs[b], sess.fl[b], session=sess)
        w1, e1 = w0, e0
        if not sess.fl[b]:
            _, w1, _, e1 = slide_counts(sess.ns[b] + n_new[b], sess.fs[b] + f_new[b], flush[b], session=sess)
        ws.append(w1 - w0)
        es.append(e1 - e0)
    return ws, es


def slide_push_each(session, samples=None, video=None, flush=None, vnorm_mean=None, vnorm_std=None,
                    return_spectrograms=False):
    """avse_slide_push_each: every stream moves by its own amount.  samples: a list of B 1-D float32 device tensors
    (None or empty for a stream without new samples), video: a list of B [k, 128, 128] tensors of video FRAMES in the
    session's dtype (None for a stream without new video), flush: a list of B bools; any of the three may be None as a
    whole.  -> a list of B 1-D tensors, stream b's newly final samples; with return_spectrograms also two lists of
    [w_b, 80, spf] tensors, the whole windows the network saw and predicted for the w_b windows stream b completed in
    this call.  Asynchronous on torch's current stream."""
    w = session.weights
    dev = torch.device("cuda", w.ctx.device_index)
    B = session.n_streams
    samples = [None] * B if samples is None else list(samples)
    video = [None] * B if video is None else list(video)
    flush = [False] * B if flush is None else [bool(f) for f in flush]
    if not (len(samples) == len(video) == len(flush) == B):
        raise ValueError(f"samples, video and flush must have one entry per stream ({B})")
    n_new, f_new, s_parts, v_parts = [], [], [], []
    for b in range(B):
        x, vid = samples[b], video[b]
        if isinstance(vid, NoVideo):
            raise ValueError("NoVideo in a sliding session: a window that is partly blank needs a rule (not built)")
        if x is not None and x.numel():
            _dev_f32(x, f"samples[{b}]")
            if x.dim() != 1:
                raise ValueError(f"samples[{b}] must be 1-D")
            s_parts.append(x)
        n_new.append(0 if x is None else int(x.numel()))
        if vid is not None and vid.shape[0]:
            if _dev_video(vid, f"video[{b}]", (128, 128)) != session.video_dtype:
                raise TypeError(f"video[{b}] is {vid.dtype}, the session was created for the other video dtype")
            if vid.dim() != 3:
                raise ValueError(f"video[{b}] must be [k, 128, 128] (video frames)")
            v_parts.append(vid)
        f_new.append(0 if vid is None else int(vid.shape[0]))
    if (vnorm_mean is None) != (vnorm_std is None):
        raise ValueError("vnorm_mean and vnorm_std must both be given")
    if vnorm_mean is not None:
        _dev_f32(vnorm_mean, "vnorm_mean", (128, 128))
        _dev_f32(vnorm_std, "vnorm_std", (128, 128))
    for t in s_parts + v_parts + [vnorm_mean, vnorm_std]:
        if t is not None and t.device.index != dev.index:
            raise ValueError(f"the session lives on {dev} but an argument is on {t.device}")
    packed = (s_parts[0] if len(s_parts) == 1 else torch.cat(s_parts)) if s_parts else None
    vpacked = (v_parts[0] if len(v_parts) == 1 else torch.cat(v_parts)) if v_parts else None
    off = np.concatenate([[0], np.cumsum(n_new)[:-1]])
    ws, es = _slide_expect(session, n_new, f_new, flush)
    out = torch.empty((B, max(es)), dtype=torch.float32, device=dev)
    mel = pred = None
    if return_spectrograms:
        mel = torch.empty((sum(ws), 80, session.spf), dtype=torch.float32, device=dev)
        pred = torch.empty_like(mel)
    (_off, p_off), (_n, p_n), (_f, p_f) = _host_i64(off), _host_i64(n_new), _host_i64(f_new)
    fl = np.ascontiguousarray(flush, dtype=np.uint8)
    got, got_w = np.full(B, -1, np.int64), np.full(B, -1, np.int64)
    with torch.cuda.device(dev):
        rc = _lib.load().avse_slide_push_each(
            session.handle, _lib.ptr(packed), p_off, p_n, _lib.ptr(vpacked), p_f, ctypes.c_void_p(fl.ctypes.data),
            _lib.ptr(vnorm_mean), _lib.ptr(vnorm_std), _lib.ptr(out), int(out.shape[1]), ctypes.c_void_p(got.ctypes.data),
            _lib.ptr(mel), _lib.ptr(pred), ctypes.c_void_p(got_w.ctypes.data), _lib.stream_handle(dev))
    _lib.check(rc, "avse_slide_push_each")
    if got.tolist() != es or got_w.tolist() != ws:
        raise _lib.AvseError(f"the session emitted {got.tolist()} samples of {got_w.tolist()} windows, the host totals "
                             f"give {es} of {ws}")
    for b in range(B):
        session.ns[b] += n_new[b]
        session.fs[b] += f_new[b]
        session.fl[b] = session.fl[b] or flush[b]
    return _stream_split(out, mel, pred, ws, es, return_spectrograms)


def slide_reset_each(session, streams=None):
    """avse_slide_reset_each: the listed streams (None: all, avse_slide_reset, which also mends a broken session) go
    back to the state after slide_create, ordered on torch's current stream; the others are untouched."""
    dev = torch.device("cuda", session.weights.ctx.device_index)
    if streams is None:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().avse_slide_reset(session.handle, _lib.stream_handle(dev)), "avse_slide_reset")
        streams = range(session.n_streams)
    else:
        which = np.zeros(session.n_streams, np.uint8)
        for b in streams:
            if not 0 <= int(b) < session.n_streams:
                raise ValueError(f"no stream {b} in a session of {session.n_streams}")
            which[int(b)] = 1
        with torch.cuda.device(dev):
            _lib.check(_lib.load().avse_slide_reset_each(session.handle, ctypes.c_void_p(which.ctypes.data),
                                                         _lib.stream_handle(dev)), "avse_slide_reset_each")
        streams = np.flatnonzero(which)
    for b in streams:
        session.ns[b], session.fs[b], session.fl[b] = 0, 0, False


def slide_state(session):
    """avse_slide_state: the library's per-stream totals -> (samples [B], video frames [B], flushed [B]) as lists."""
    B = session.n_streams
    n, f, fl = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.uint8)
    _lib.check(_lib.load().avse_slide_state(session.handle, ctypes.c_void_p(n.ctypes.data), ctypes.c_void_p(f.ctypes.data),
                                            ctypes.c_void_p(fl.ctypes.data)), "avse_slide_state")
    return n.tolist(), f.tolist(), [bool(x) for x in fl]


# ---- offline sliding: whole utterances through a flushed sliding session's windows ----
def _slide_geometry(n_slices, frames_per_slice, video_frames, stride):
    """The host checks the three offline sliding calls share -> (n_slices as int64 [U], spf, F, stride)."""
    spf, F, s = int(frames_per_slice), int(video_frames), int(stride)
    if spf < 1 or F < 1 or spf % F:
        raise ValueError(f"frames_per_slice {spf} must be a positive multiple of video_frames {F}")
    if not 1 <= s <= F:
        raise ValueError(f"the stride must be 1 .. {F} (video_frames), got {s}")
    ns = np.ascontiguousarray(np.asarray(n_slices), dtype=np.int64)
    if ns.ndim != 1:
        raise ValueError("n_slices must be 1-D")
    if ns.size and ns.min() < 0:
        raise ValueError("negative counts")
    return ns, spf, F, s


def slide_window_counts(n_slices, frames_per_slice=20, video_frames=5, stride=1):
    """Per utterance of n_slices[u] slices, (windows W_u, predicted columns P_u) of the flushed sliding stream, as int64
    arrays: avse_slide_counts_geom's totals (the hop and n_fft do not enter them)."""
    ns, spf, F, s = _slide_geometry(n_slices, frames_per_slice, video_frames, stride)
    lengths, inverse = np.unique(ns, return_inverse=True)      # one library call per distinct length
    wp = np.array([slide_counts(0, F * S, True, stride=s, geometry=(2, 1, spf, F))[1:3] for S in lengths.tolist()],
                  dtype=np.int64).reshape(-1, 2)
    return wp[inverse, 0], wp[inverse, 1]


def slide_windows(mel_packed, n_frames, n_slices, frames_per_slice=20, video_frames=5, stride=1, n_mels=80, top_db=80.0):
    """avse_slide_windows: the network's audio input for the windows of a ragged batch.  mel_packed: the 1-D packed
    UNCLAMPED [n_mels, T_u] blocks (spectrogram_ragged(top_db=None, frames_per_slice=0)), n_frames the T_u, n_slices the
    S_u.  Returns [sum W_u, n_mels, frames_per_slice]: window j of an utterance is its frames [q s j, q s j + spf)
    clamped at (the maximum of its frames up to the window's last) - top_db (None: no clamp)."""
    _dev_f32(mel_packed, "mel_packed")
    ns, spf, F, s = _slide_geometry(n_slices, frames_per_slice, video_frames, stride)
    nf = np.ascontiguousarray(np.asarray(n_frames), dtype=np.int64)
    if nf.shape != ns.shape:
        raise ValueError("n_frames and n_slices must be of one size")
    if nf.size and (nf < spf * ns).any():
        raise ValueError("an utterance has fewer frames than its slices' windows read")
    if mel_packed.dim() != 1 or int(nf.sum()) * n_mels != mel_packed.numel():
        raise ValueError("n_frames do not add up to the packed buffer")
    W, _ = slide_window_counts(ns, spf, F, s)
    dev = mel_packed.device
    out = torch.empty((int(W.sum()), n_mels, spf), dtype=torch.float32, device=dev)
    if out.numel():
        ctx = _lib.context(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().avse_slide_windows(
                ctx.handle, _lib.ptr(mel_packed), nf.ctypes.data, ns.ctypes.data, int(ns.size), spf, F, s, int(n_mels),
                float(-1.0 if top_db is None else top_db), _lib.ptr(out), _lib.stream_handle(dev)), "avse_slide_windows")
    return out


def slide_video_windows(video, n_slices, stride=1, w0=0, n=None, out=None):
    """avse_slide_video_windows: the network's video input for windows [w0, w0 + n) of the batch's window list (n None:
    to its end).  video: [sum S_u, 128, 128, F] slices, float32 or uint8.  Returns [n, 128, 128, F] of the same dtype
    (into the first n rows of `out` when given): window j of an utterance is its frames s j .. s j + F - 1."""
    _dev_video(video, "video")
    if video.dim() != 4 or tuple(video.shape[1:3]) != (128, 128):
        raise ValueError("video must be [slices, 128, 128, frames]")
    F = int(video.shape[3])
    ns, _, _, s = _slide_geometry(n_slices, F, F, stride)
    if int(ns.sum()) != video.shape[0]:
        raise ValueError("n_slices do not add up to the video's slices")
    if F not in (5, 6):
        raise ValueError("video windows are built for 5 and 6 video frames per slice")
    W, _ = slide_window_counts(ns, F, F, s)
    total = int(W.sum())
    w0 = int(w0)
    n = total - w0 if n is None else int(n)
    if w0 < 0 or n < 0 or w0 + n > total:
        raise ValueError(f"windows [{w0}, {w0 + n}) lie outside the batch's {total} windows")
    if out is None:
        out = torch.empty((n,) + tuple(video.shape[1:]), dtype=video.dtype, device=video.device)
    else:
        _dev_video(out, "out")
        if out.dtype != video.dtype or out.device != video.device or out.dim() != 4 or out.shape[0] < n or \
                tuple(out.shape[1:]) != tuple(video.shape[1:]):
            raise ValueError(f"out must hold {n} windows of the video's shape, dtype and device")
    if n:
        dev = video.device
        ctx = _lib.context(dev)
        vdt = _lib.AVSE_VIDEO_U8 if video.dtype == torch.uint8 else _lib.AVSE_VIDEO_F32
        with torch.cuda.device(dev):
            _lib.check(_lib.load().avse_slide_video_windows(
                ctx.handle, _lib.ptr(video), vdt, ns.ctypes.data, int(ns.size), F, s, w0, n, _lib.ptr(out),
                _lib.stream_handle(dev)), "avse_slide_video_windows")
    return out[:n]


def slide_keep(pred, n_slices, video_frames=5, stride=1):
    """avse_slide_keep: the kept columns of the predicted windows pred [sum W_u, n_mels, spf] -> (the 1-D packed
    [n_mels, P_u] blocks, the P_u): istft_ragged's 1-D input and its counts."""
    _dev_f32(pred, "pred")
    if pred.dim() != 3:
        raise ValueError("pred must be [windows, n_mels, frames_per_slice]")
    n_mels, spf = int(pred.shape[1]), int(pred.shape[2])
    ns, spf, F, s = _slide_geometry(n_slices, spf, video_frames, stride)
    W, P = slide_window_counts(ns, spf, F, s)
    if int(W.sum()) != pred.shape[0]:
        raise ValueError("n_slices do not add up to pred's windows")
    dev = pred.device
    total = int(P.sum()) * n_mels
    packed = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    if total:
        ctx = _lib.context(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().avse_slide_keep(
                ctx.handle, _lib.ptr(pred), ns.ctypes.data, int(ns.size), spf, F, s, n_mels, _lib.ptr(packed),
                _lib.stream_handle(dev)), "avse_slide_keep")
    return packed[:total], P


def resample_supported(sr_in, sr_out, return_message=False):
    """avse_resample_supported (host only, no GPU): 0 when sr_in -> sr_out is served (max(up, down) <= 640 after
    reduction), else the status resample / resampler_create would raise with (3: unsupported, 1: invalid).
    return_message: -> (status, the library's reason; "" for status 0)."""
    lib = _lib.load()
    rc = int(lib.avse_resample_supported(int(sr_in), int(sr_out)))
    if not return_message:
        return rc
    return rc, (lib.avse_last_error().decode(errors="replace") if rc else "")


def resample_counts(sr_in, sr_out, n_in, flushed=False):
    """avse_resample_counts (host only, no GPU): the outputs that are final after n_in inputs,
    max(0, ceil((n_in up - H) / down)), or all ceil(n_in up / down) of a flushed stream."""
    out = ctypes.c_int64()
    _lib.check(_lib.load().avse_resample_counts(int(sr_in), int(sr_out), int(n_in), int(bool(flushed)), ctypes.byref(out)),
               "avse_resample_counts")
    return out.value


def resample(signals, sr_in, sr_out):
    """scipy.signal.resample_poly(x, up, down) with its defaults in one avse_resample_ragged call: signals is a [U, n]
    float32 device tensor (-> [U, ceil(n up / down)]) or a list of 1-D float32 device tensors (-> a list of 1-D tensors,
    views of one buffer).  float64 taps and sums, rounded once to float32; equal rates copy the bits."""
    batch = isinstance(signals, torch.Tensor)
    if batch:
        _dev_f32(signals, "signals")
        if signals.dim() != 2:
            raise ValueError(f"signals must be [U, n] or a list of 1-D tensors, got shape {tuple(signals.shape)}")
        U, n = int(signals.shape[0]), int(signals.shape[1])
        buf, dev = signals, signals.device
        lens = np.full(U, n, np.int64)
        off = np.arange(U, dtype=np.int64) * n
    else:
        signals = list(signals)
        if not signals:
            raise ValueError("resample needs at least one signal")
        for k, t in enumerate(signals):
            _dev_f32(t, f"signals[{k}]")
            if t.dim() != 1:
                raise ValueError(f"signals[{k}] must be 1-D, got shape {tuple(t.shape)}")
        U, dev = len(signals), signals[0].device
        lens = np.array([t.numel() for t in signals], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        buf = torch.cat(signals)
    n_out = np.array([resample_counts(sr_in, sr_out, int(n), True) for n in lens], dtype=np.int64)
    out_off = np.concatenate([[0], np.cumsum(n_out)[:-1]]).astype(np.int64)
    out = torch.empty(max(int(n_out.sum()), 1), dtype=torch.float32, device=dev)
    if U:
        ctx = _lib.context(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().avse_resample_ragged(
                ctx.handle, _lib.ptr(buf), off.ctypes.data, lens.ctypes.data, U, int(sr_in), int(sr_out), _lib.ptr(out),
                out_off.ctypes.data, _lib.stream_handle(dev)), "avse_resample_ragged")
    if batch:
        return out[:int(n_out.sum())].view(U, int(n_out[0]) if U else 0)
    return [out[int(o):int(o) + int(m)] for o, m in zip(out_off, n_out)]


class Resampler:
    """avse_resampler: the device state of n_streams streams at one rate pair (resampler_create).  ns / outs / fl are the
    host totals per stream (inputs received, outputs emitted, flushed), mirroring the library's counters."""

    def __init__(self, ctx, handle, n_streams, sr_in, sr_out):
        self.ctx, self.handle = ctx, handle      # the context outlives the resampler
        self.n_streams, self.sr_in, self.sr_out = n_streams, sr_in, sr_out
        self.ns, self.outs, self.fl = [0] * n_streams, [0] * n_streams, [False] * n_streams
        self._cdll = _lib.load()

    def expect(self, n_new, flush):
        """Per stream, the outputs a call with these counts emits, from the host totals (input for a flushed stream
        emits nothing and is left to the library to refuse)."""
        es = []
        for b in range(self.n_streams):
            e = 0
            if not self.fl[b]:
                e = resample_counts(self.sr_in, self.sr_out, self.ns[b] + n_new[b], flush[b]) - self.outs[b]
            es.append(e)
        return es

    def __del__(self):
        h, lib = getattr(self, "handle", None), getattr(self, "_cdll", None)
        if h is not None and h.value and lib is not None:
            lib.avse_resampler_destroy(h)
            self.handle = None


def resampler_create(n_streams, sr_in, sr_out, device=None):
    """avse_resampler_create on the device's context -> Resampler.  A rate pair resample_supported refuses raises
    _lib.AvseError (status 3)."""
    if int(n_streams) < 1:
        raise ValueError("n_streams must be positive")
    ctx = _lib.context(device)
    h = ctypes.c_void_p()
    with torch.cuda.device(ctx.device_index):
        _lib.check(_lib.load().avse_resampler_create(ctx.handle, int(n_streams), int(sr_in), int(sr_out), ctypes.byref(h)),
                   "avse_resampler_create")
    return Resampler(ctx, h, int(n_streams), int(sr_in), int(sr_out))


def _resampler_push_packed(r, packed, off, n_new, flush, out_stride=None):
    """The call of resampler_push_each on checked, packed arguments (stream b's n_new[b] samples start at element off[b] of
    `packed`) -> (out [B, out_stride or the largest count], outputs per stream)."""
    dev = torch.device("cuda", r.ctx.device_index)
    B = r.n_streams
    es = r.expect(n_new, flush)
    stride = max(es) if out_stride is None else int(out_stride)
    out = torch.empty((B, stride), dtype=torch.float32, device=dev)
    (_off, p_off), (_n, p_n) = _host_i64(off), _host_i64(n_new)
    fl = np.ascontiguousarray(flush, dtype=np.uint8)
    got = np.full(B, -1, np.int64)
    with torch.cuda.device(dev):
        rc = _lib.load().avse_resampler_push_each(r.handle, _lib.ptr(packed), p_off, p_n, ctypes.c_void_p(fl.ctypes.data),
                                                  _lib.ptr(out), stride, ctypes.c_void_p(got.ctypes.data),
                                                  _lib.stream_handle(dev))
    _lib.check(rc, "avse_resampler_push_each")
    if got.tolist() != es:
        raise _lib.AvseError(f"the resampler emitted {got.tolist()} samples, the host totals give {es}")
    for b in range(B):
        r.ns[b] += n_new[b]
        r.outs[b] += es[b]
        r.fl[b] = r.fl[b] or flush[b]
    return out, es


def resampler_push_each(resampler, samples=None, flush=None, out_stride=None):
    """avse_resampler_push_each: samples is a list of B 1-D float32 device tensors (None or empty for an idle stream),
    flush a list of B bools (streams to close: their remaining outputs come out, with zeros past the end as the one-shot
    call has them) -> a list of B 1-D tensors, the outputs that became final.  The concatenation of a stream's outputs is,
    bit for bit, resample() of its whole signal, however it was cut.  out_stride: the row length of the output buffer
    (default: the largest count); one too small is refused by the library with the state unchanged.  Asynchronous on
    torch's current stream."""
    dev = torch.device("cuda", resampler.ctx.device_index)
    B = resampler.n_streams
    samples = [None] * B if samples is None else list(samples)
    flush = [False] * B if flush is None else [bool(f) for f in flush]
    if not (len(samples) == len(flush) == B):
        raise ValueError(f"samples and flush must have one entry per stream ({B})")
    n_new, parts = [], []
    for b, x in enumerate(samples):
        if x is not None and x.numel():
            _dev_f32(x, f"samples[{b}]")
            if x.dim() != 1:
                raise ValueError(f"samples[{b}] must be 1-D")
            if x.device.index != dev.index:
                raise ValueError(f"the resampler lives on {dev} but samples[{b}] is on {x.device}")
            parts.append(x)
        n_new.append(0 if x is None else int(x.numel()))
    packed = torch.cat(parts) if parts else None
    off = np.concatenate([[0], np.cumsum(n_new)[:-1]])
    out, es = _resampler_push_packed(resampler, packed, off, n_new, flush, out_stride)
    return [out[b, :e] for b, e in enumerate(es)]


def resampler_reset_each(resampler, streams=None):
    """avse_resampler_reset_each: the listed streams (None: all) go back to the state after resampler_create."""
    B = resampler.n_streams
    which = np.ones(B, np.uint8) if streams is None else np.zeros(B, np.uint8)
    for b in ([] if streams is None else streams):
        if not 0 <= int(b) < B:
            raise ValueError(f"no stream {b} in a resampler of {B}")
        which[int(b)] = 1
    dev = torch.device("cuda", resampler.ctx.device_index)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().avse_resampler_reset_each(resampler.handle, ctypes.c_void_p(which.ctypes.data),
                                                         _lib.stream_handle(dev)), "avse_resampler_reset_each")
    for b in np.flatnonzero(which):
        resampler.ns[b], resampler.outs[b], resampler.fl[b] = 0, 0, False


def resampler_state(resampler):
    """avse_resampler_state: the library's per-stream totals -> (inputs [B], outputs [B], flushed [B]) as lists."""
    B = resampler.n_streams
    n, m, f = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.uint8)
    _lib.check(_lib.load().avse_resampler_state(resampler.handle, ctypes.c_void_p(n.ctypes.data),
                                                ctypes.c_void_p(m.ctypes.data), ctypes.c_void_p(f.ctypes.data)),
               "avse_resampler_state")
    return n.tolist(), m.tolist(), [bool(x) for x in f]


def frame_rate(fps):
    """A frame rate as a rational: an int, a fractions.Fraction or a (num, den) pair is taken as it is; a float becomes
    Fraction(x).limit_denominator(1001), so 29.97 is 2997/100 and 30000 / 1001 (NTSC, as a float) is 30000/1001.  Pass
    the pair or the Fraction where the float would be ambiguous."""
    if isinstance(fps, (tuple, list)):
        if len(fps) != 2:
            raise ValueError(f"a frame rate is a number or a (num, den) pair, got {fps!r}")
        return Fraction(int(fps[0]), int(fps[1]))
    if isinstance(fps, (int, Fraction)):
        return Fraction(fps)
    return Fraction(float(fps)).limit_denominator(1001)


def _rates(fps_in, fps_out):
    a, b = frame_rate(fps_in), frame_rate(fps_out)
    return a.numerator, a.denominator, b.numerator, b.denominator


def _dev_frames(t, name, dims):
    """Mouth crops before retiming: a float32 or uint8 device tensor [..., 128, 128] with `dims` dimensions."""
    dt = _dev_video(t, name, (128, 128))
    if t.dim() != dims:
        raise ValueError(f"{name} must be {'[U, n, 128, 128]' if dims == 4 else '[n, 128, 128]'}, got shape {tuple(t.shape)}")
    return dt


def retime_supported(fps_in, fps_out, return_message=False):
    """avse_retime_supported (host only, no GPU): 0 when fps_in -> fps_out is served (max(p, q) <= 65536 for the reduced
    p / q = fps_in / fps_out), else the status retime / retimer_create would raise with (3: unsupported, 1: invalid).
    Rates as frame_rate takes them.  return_message: -> (status, the library's reason; "" for status 0)."""
    lib = _lib.load()
    rc = int(lib.avse_retime_supported(*_rates(fps_in, fps_out)))
    if not return_message:
        return rc
    return rc, (lib.avse_last_error().decode(errors="replace") if rc else "")


def retime_counts(fps_in, fps_out, frames_per_slice, n, flushed=False):
    """avse_retime_counts (host only, no GPU) -> (output frames, slices) that are final after n input frames:
    G(n) = floor((n - 1) q / p) + 1 frames (0 for n = 0), or all ceil(n q / p) of a flushed stream; slices = frames div
    frames_per_slice."""
    f, k = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().avse_retime_counts(*_rates(fps_in, fps_out), int(frames_per_slice), int(n), int(bool(flushed)),
                                              ctypes.byref(f), ctypes.byref(k)), "avse_retime_counts")
    return f.value, k.value


def retime(frames, fps_in, fps_out, frames_per_slice):
    """Linear frame-rate conversion into the session's slices in one avse_retime_ragged call: frames is a
    [U, n, 128, 128] float32 or uint8 device tensor (-> [U, S, 128, 128, F]) or a list of [n_u, 128, 128] tensors of one
    dtype (-> a list of [S_u, 128, 128, F] tensors, views of one buffer), S = ceil(n q / p) div F.  Output frame j blends
    input frames j p div q and the next by (j p mod q) / q (include/avse.h states the rounding); past the end the last
    frame is repeated, and the frames that do not fill a slice are dropped."""
    F = int(frames_per_slice)
    batch = isinstance(frames, torch.Tensor)
    if batch:
        vdt = _dev_frames(frames, "frames", 4)
        U, n = int(frames.shape[0]), int(frames.shape[1])
        buf, dev = frames, frames.device
        lens = np.full(U, n, np.int64)
    else:
        frames = list(frames)
        if not frames:
            raise ValueError("retime needs at least one utterance")
        vdt = _dev_frames(frames[0], "frames[0]", 3)
        for k, t in enumerate(frames):
            if _dev_frames(t, f"frames[{k}]", 3) != vdt:
                raise TypeError("the utterances' frames must have one dtype")
        U, dev = len(frames), frames[0].device
        lens = np.array([t.shape[0] for t in frames], dtype=np.int64)
        buf = torch.cat(frames)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    ks = np.array([retime_counts(fps_in, fps_out, F, int(n), True)[1] for n in lens], dtype=np.int64)
    total = int(ks.sum())
    out = torch.empty((max(total, 1), 128, 128, F), dtype=buf.dtype, device=dev)
    got = np.full(max(U, 1), -1, np.int64)
    if U:
        ctx = _lib.context(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().avse_retime_ragged(
                ctx.handle, _lib.ptr(buf) if buf.numel() else None, off.ctypes.data, lens.ctypes.data, U, vdt,
                *_rates(fps_in, fps_out), F, _lib.ptr(out), total, got.ctypes.data, _lib.stream_handle(dev)),
                "avse_retime_ragged")
        if got.tolist() != ks.tolist():
            raise _lib.AvseError(f"the retimer wrote {got.tolist()} slices, the host counts give {ks.tolist()}")
    if batch:
        return out[:total].view(U, int(ks[0]) if U else 0, 128, 128, F)
    first = np.concatenate([[0], np.cumsum(ks)]).astype(int)
    return [out[first[u]:first[u + 1]] for u in range(U)]


class Retimer:
    """avse_retimer: the device state of n_streams streams at one rate pair (retimer_create).  ns / ks / fl are the host
    totals per stream (frames received, slices handed out, flushed), mirroring the library's counters."""

    def __init__(self, ctx, handle, n_streams, fps_in, fps_out, frames_per_slice, video_dtype):
        self.ctx, self.handle = ctx, handle      # the context outlives the retimer
        self.n_streams, self.fps_in, self.fps_out, self.F = n_streams, fps_in, fps_out, frames_per_slice
        self.video_dtype = video_dtype
        self.ns, self.ks, self.fl = [0] * n_streams, [0] * n_streams, [False] * n_streams
        self._cdll = _lib.load()

    def expect(self, n_new, flush):
        """Per stream, the slices a call with these counts completes, from the host totals (input for a flushed stream
        completes nothing and is left to the library to refuse)."""
        ks = []
        for b in range(self.n_streams):
            k = 0
            if not self.fl[b]:
                k = retime_counts(self.fps_in, self.fps_out, self.F, self.ns[b] + n_new[b], flush[b])[1] - self.ks[b]
            ks.append(k)
        return ks

    def __del__(self):
        h, lib = getattr(self, "handle", None), getattr(self, "_cdll", None)
        if h is not None and h.value and lib is not None:
            lib.avse_retimer_destroy(h)
            self.handle = None


def retimer_create(n_streams, fps_in, fps_out, frames_per_slice, video_dtype=torch.float32, device=None):
    """avse_retimer_create on the device's context -> Retimer.  Rates as frame_rate takes them; a pair retime_supported
    refuses raises _lib.AvseError (status 3).  video_dtype: torch.float32 or torch.uint8, the element type of every
    push's frames and of the slices."""
    if int(n_streams) < 1:
        raise ValueError("n_streams must be positive")
    if video_dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"video_dtype must be torch.float32 or torch.uint8, got {video_dtype}")
    vdt = _lib.AVSE_VIDEO_U8 if video_dtype == torch.uint8 else _lib.AVSE_VIDEO_F32
    a, b = frame_rate(fps_in), frame_rate(fps_out)
    ctx = _lib.context(device)
    h = ctypes.c_void_p()
    with torch.cuda.device(ctx.device_index):
        _lib.check(_lib.load().avse_retimer_create(ctx.handle, int(n_streams), *_rates(a, b), int(frames_per_slice), vdt,
                                                   ctypes.byref(h)), "avse_retimer_create")
    return Retimer(ctx, h, int(n_streams), a, b, int(frames_per_slice), vdt)


def _retimer_pack(r, frames):
    """retimer_push_each's frames, checked and packed on the device (one torch.cat) -> (packed frames or None, first
    frame per stream [B], frames per stream [B])."""
    dev = torch.device("cuda", r.ctx.device_index)
    n_new, parts = [], []
    for b, x in enumerate(frames):
        if x is not None and x.shape[0]:
            if _dev_frames(x, f"frames[{b}]", 3) != r.video_dtype:
                raise TypeError(f"frames[{b}] is {x.dtype}, the retimer was created for the other video dtype")
            if x.device.index != dev.index:
                raise ValueError(f"the retimer lives on {dev} but frames[{b}] is on {x.device}")
            parts.append(x)
        n_new.append(0 if x is None else int(x.shape[0]))
    packed = (parts[0] if len(parts) == 1 else torch.cat(parts)) if parts else None
    return packed, np.concatenate([[0], np.cumsum(n_new)[:-1]]), n_new


def _retimer_push_packed(r, packed, off, n_new, flush, out_slices=None):
    """The call of retimer_push_each on checked, packed arguments (stream b's n_new[b] frames start at frame off[b] of
    `packed`) -> (the completed slices [sum k, 128, 128, F] stream-major, slices per stream)."""
    dev = torch.device("cuda", r.ctx.device_index)
    B = r.n_streams
    ks = r.expect(n_new, flush)
    cap = sum(ks) if out_slices is None else int(out_slices)
    out = torch.empty((cap, 128, 128, r.F), dtype=torch.uint8 if r.video_dtype == _lib.AVSE_VIDEO_U8 else torch.float32,
                      device=dev)
    (_off, p_off), (_n, p_n) = _host_i64(off), _host_i64(n_new)
    fl = np.ascontiguousarray(flush, dtype=np.uint8)
    got = np.full(B, -1, np.int64)
    with torch.cuda.device(dev):
        rc = _lib.load().avse_retimer_push_each(r.handle, _lib.ptr(packed), p_off, p_n, ctypes.c_void_p(fl.ctypes.data),
                                                _lib.ptr(out) if cap else None, cap, ctypes.c_void_p(got.ctypes.data),
                                                _lib.stream_handle(dev))
    _lib.check(rc, "avse_retimer_push_each")
    if got.tolist() != ks:
        raise _lib.AvseError(f"the retimer completed {got.tolist()} slices, the host totals give {ks}")
    for b in range(B):
        r.ns[b] += n_new[b]
        r.ks[b] += ks[b]
        r.fl[b] = r.fl[b] or flush[b]
    return out, ks


def retimer_push_each(retimer, frames=None, flush=None, out_slices=None):
    """avse_retimer_push_each: frames is a list of B [n_b, 128, 128] device tensors in the retimer's dtype (None or empty
    for an idle stream), flush a list of B bools (streams to close: their remaining frames come out as copies of the
    last one, and the frames that do not fill a slice are dropped) -> a list of B [k_b, 128, 128, F] tensors, the slices
    that became complete, views of one buffer in stream_push_each's packed video layout.  The concatenation of a stream's
    slices is, bit for bit, retime() of all its frames, however they were cut.  out_slices: the slices the output buffer
    holds (default: what the call completes); one too small is refused by the library with the state unchanged.
    Asynchronous on torch's current stream."""
    B = retimer.n_streams
    frames = [None] * B if frames is None else list(frames)
    flush = [False] * B if flush is None else [bool(f) for f in flush]
    if not (len(frames) == len(flush) == B):
        raise ValueError(f"frames and flush must have one entry per stream ({B})")
    packed, off, n_new = _retimer_pack(retimer, frames)
    out, ks = _retimer_push_packed(retimer, packed, off, n_new, flush, out_slices)
    first = np.concatenate([[0], np.cumsum(ks)]).astype(int)
    return [out[first[b]:first[b + 1]] for b in range(B)]


def retimer_reset_each(retimer, streams=None):
    """avse_retimer_reset_each: the listed streams (None: all) go back to the state after retimer_create."""
    B = retimer.n_streams
    which = np.ones(B, np.uint8) if streams is None else np.zeros(B, np.uint8)
    for b in ([] if streams is None else streams):
        if not 0 <= int(b) < B:
            raise ValueError(f"no stream {b} in a retimer of {B}")
        which[int(b)] = 1
    dev = torch.device("cuda", retimer.ctx.device_index)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().avse_retimer_reset_each(retimer.handle, ctypes.c_void_p(which.ctypes.data),
                                                       _lib.stream_handle(dev)), "avse_retimer_reset_each")
    for b in np.flatnonzero(which):
        retimer.ns[b], retimer.ks[b], retimer.fl[b] = 0, 0, False


def retimer_state(retimer):
    """avse_retimer_state: the library's per-stream totals -> (frames [B], slices [B], flushed [B]) as lists."""
    B = retimer.n_streams
    n, m, f = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.uint8)
    _lib.check(_lib.load().avse_retimer_state(retimer.handle, ctypes.c_void_p(n.ctypes.data),
                                              ctypes.c_void_p(m.ctypes.data), ctypes.c_void_p(f.ctypes.data)),
               "avse_retimer_state")
    return n.tolist(), m.tolist(), [bool(x) for x in f]


class Trainer:
    """libavse training step (avse_trainer_*, train.hip): one Keras fit step of SpeechEnhancementNetwork.train
    (network.py:177-206) — BatchNormalization on batch statistics, Dropout after each video pooling, MSE, Adam.
    Parameters / gradients / Adam moments stay on the device in the canonical blob layout."""

    def __init__(self, model, max_batch=16, device=None):
        if not isinstance(model, KerasModel):
            raise TypeError("model must be a KerasModel")
        self.ctx = _lib.context(device)
        self.max_batch = int(max_batch)
        self.T, self.F = model.T, model.F
        blob = model.to_blob()
        self._cdll = _lib.load()   # held for __del__ (see DeviceWeights)
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(self.ctx.device_index):
            _lib.check(_lib.load().avse_trainer_create_shape(self.ctx.handle, blob.ctypes.data_as(ctypes.c_void_p),
                                                             blob.size, self.max_batch, self.T, self.F,
                                                             ctypes.byref(self.handle)), "avse_trainer_create_shape")
        self._loss = torch.zeros((), dtype=torch.float32, device=torch.device("cuda", self.ctx.device_index))

    def step(self, audio, video, target, vnorm_mean=None, vnorm_std=None, lr=5e-4, dropout=0.25, seed=0,
             grads_only=False):
        """One fit step on a batch: audio / target [N, 80, 20], video [N, 128, 128, 5] (raw crops when vnorm_* are
        given) float32 device tensors; video may also be uint8 crops (4-byte aligned, with vnorm_* for a normalised
        fit).  Returns the batch MSE before the update as a 0-dim device tensor."""
        _dev_f32(audio, "audio", (80, self.T))
        _dev_f32(target, "target", (80, self.T))
        vdt = _dev_video(video, "video", (128, 128, self.F))
        N = audio.shape[0]
        if video.shape[0] != N or target.shape[0] != N:
            raise ValueError("audio, video and target batch sizes differ")
        if N > self.max_batch:
            raise ValueError(f"batch of {N} exceeds the trainer's max_batch {self.max_batch}")
        if (vnorm_mean is None) != (vnorm_std is None):
            raise ValueError("vnorm_mean and vnorm_std must both be given")
        devs = {self.ctx.device_index, audio.device.index, video.device.index, target.device.index}
        if len(devs) != 1:
            raise ValueError("trainer and batch tensors must share one device")
        with torch.cuda.device(audio.device):
            _check_video(_lib.load().avse_trainer_step_video(
                self.handle, _lib.ptr(audio), _lib.ptr(video), vdt, _lib.ptr(target), _lib.ptr(vnorm_mean),
                _lib.ptr(vnorm_std), N, float(lr), float(dropout), int(seed) & 0xFFFFFFFF,
                _lib.AVSE_TRAIN_GRADS_ONLY if grads_only else 0, _lib.ptr(self._loss),
                _lib.stream_handle(audio.device)), "avse_trainer_step", video)
        return self._loss.clone()

    def _read(self, what):
        out = np.empty(blob_floats(self.T, self.F), dtype=np.float32)
        _lib.check(_lib.load().avse_trainer_read(self.handle, what, out.ctypes.data_as(ctypes.c_void_p), out.size),
                   "avse_trainer_read")
        return out

    def model(self):
        """Current parameters (incl. BN moving statistics) as a KerasModel."""
        return KerasModel.from_blob(self._read(_lib.AVSE_TRAIN_PARAMS), self.T, self.F)

    def gradients(self):
        """Gradients of the last step, {tensor name: array} (moving statistics: zero)."""
        return KerasModel.from_blob(self._read(_lib.AVSE_TRAIN_GRADS), self.T, self.F).tensors

    @property
    def iterations(self):
        v = ctypes.c_int64()
        _lib.check(_lib.load().avse_trainer_iterations(self.handle, ctypes.byref(v)), "avse_trainer_iterations")
        return v.value

    def __del__(self):
        h, lib = getattr(self, "handle", None), getattr(self, "_cdll", None)
        if h is not None and h.value and lib is not None:
            lib.avse_trainer_destroy(h)
            self.handle = None
