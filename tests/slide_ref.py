"""Float64 reference of a sliding streaming session (include/avse.h avse_slide_*), built from
oracle/librosa_ref.py and oracle/keras_ref.py and following the definitions literally: the unclamped mel-dB of the closed
signal, a causal clamp per window, K.forward per window, the kept columns, reconstruct_signal_from_spectrogram over the
mixture's phase of the predicted frames.  It knows nothing of pushes: a flushed stream does not depend on its cuts."""
import numpy as np

from oracle import keras_ref as K
from oracle import librosa_ref as R


def totals(n, f, stride, flushed=False, n_fft=640, hop=160, spf=20, F=5):
    """(frames, windows, predicted, emitted) of a stream after n samples and f video frames, from the definitions."""
    q = spf // F
    frames = q * f if flushed else (0 if n < n_fft // 2 + 1 else (n - n_fft // 2) // hop + 1)
    wa = (frames - spf) // (q * stride) + 1 if frames >= spf else 0
    wv = (f - F) // stride + 1 if f >= F else 0
    w = min(wa, wv)
    predicted = spf + q * stride * (w - 1) if w > 0 else 0
    emitted = (hop * (predicted - 1) if predicted > 0 else 0) if flushed else max(0, hop * predicted - n_fft // 2)
    return frames, w, predicted, emitted


def slide_reference(sig, frames, mean, std, layers, stride, sr=16000, n_fft=640, hop=160, spf=20, top_db=80.0):
    """The flushed stream of samples `sig` [n] and video `frames` [f, 128, 128] (n <= hop q f).
    -> dict(unclamped [80, q f], mel [W, 80, spf] as the network sees each window, pred [W, 80, spf], wave [emitted],
    floors [W], predicted)."""
    f = frames.shape[0]
    F = layers_video_frames(layers)
    q = spf // F
    assert spf % F == 0 and 1 <= stride <= F and len(sig) <= hop * q * f
    x = R.fit_length(np.asarray(sig, np.float32), hop * q * f)
    D = R.stft(x, n_fft=n_fft, hop_length=hop)
    mag, phase = R.magphase(D)
    un = R.amplitude_to_db(np.dot(R.mel_filterbank(sr, n_fft, n_mels=80, fmin=0, fmax=8000), mag), top_db=None)
    un = un[:, :q * f]                                  # frames 0 .. q f - 1 (the offline call drops frame q f too)
    W = (f - F) // stride + 1 if f >= F else 0
    mel, vid, floors = [], [], []
    for j in range(W):
        t0 = q * stride * j
        floor = un[:, :t0 + spf].max() - top_db if top_db is not None and top_db >= 0 else -np.inf
        floors.append(floor)
        mel.append(np.maximum(un[:, t0:t0 + spf], floor))
        vid.append(np.moveaxis(frames[stride * j:stride * j + F], 0, -1))      # [128, 128, F], frame innermost
    mel = np.stack(mel)
    vn = R.video_normalize(np.stack(vid).astype(np.float32), mean, std).astype(np.float32)
    pred = K.forward(layers, mel.astype(np.float32), vn)
    kept = [pred[0]] + [pred[j][:, spf - q * stride:] for j in range(1, W)]
    spec = np.concatenate(kept, axis=1).astype(np.float32)
    predicted = spec.shape[1]
    assert predicted == spf + q * stride * (W - 1)
    wave = R.reconstruct_signal_from_spectrogram(spec, phase[:, :predicted], sr, n_fft, hop)
    return dict(unclamped=un, mel=mel, pred=pred, wave=wave, floors=np.array(floors), predicted=predicted)


def layers_video_frames(layers):
    """F of a KerasModel.layer_dict(): the input channels of the first video convolution."""
    for name in ("v_conv1", "video_conv1"):
        if name in layers:
            w = layers[name]["kernel"] if isinstance(layers[name], dict) else layers[name][0]
            return int(np.asarray(w).shape[2])
    raise KeyError("no first video convolution in the layer dict")
