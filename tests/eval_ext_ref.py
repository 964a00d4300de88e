"""Float64 reference of what avse_eval_pairs_ext adds to avse_eval_pairs (include/avse.h): STOI at every sample rate
(no limit on max(up, down)) and ESTOI, written from the header's step list with numpy on eval_ref's pieces.  Nothing
of eval_ref is assigned to: its MAX_RATIO still holds for the tests of the default entry points.

`dtype=np.float32` runs the framing, FFT, band, STOI-segment and ESTOI arithmetic in float32 (the resampling, the
frame energies and the mask stay float64): the yardstick the GPU tests derive their STOI and ESTOI gates from."""
import numpy as np

import eval_ref as R

NMETRICS = 6
ESTOI = 5
N_SEG = R.N_SEG


def mask_margin(s, sr):
    """The smallest |e_i - (max(e) - 40)| in dB over the pair's frames at any rate (inf without frames)."""
    up, down = R.ratio(sr)
    e = R.frame_energies(R.resample(np.asarray(s, np.float64), up, down))
    if e.size == 0:
        return float("inf")
    return float(np.min(np.abs(e - (e.max() - R.DYN_RANGE))))


def band_envelopes(s, y, sr, dtype=np.float64):
    """Steps 1 .. 3 -> (X [15, M], Y [15, M], K); X and Y are None when M = K - 1 < 30."""
    up, down = R.ratio(sr)
    x10 = R.resample(s, up, down)
    y10 = R.resample(y, up, down)
    e = R.frame_energies(x10)
    if e.size == 0:
        return None, None, 0.0
    starts = np.array(list(R.frame_starts(x10.size)), dtype=np.int64)
    kept = starts[e > e.max() - R.DYN_RANGE]
    K = kept.size
    if K - 1 < N_SEG:
        return None, None, float(K)
    W = R.stoi_window().astype(dtype)
    xs = np.zeros((K - 1) * R.HOP + R.N_FRAME, dtype)
    ys = np.zeros_like(xs)
    x10 = x10.astype(dtype)
    y10 = y10.astype(dtype)
    for k, i in enumerate(kept):
        xs[k * R.HOP:k * R.HOP + R.N_FRAME] += W * x10[i:i + R.N_FRAME]
        ys[k * R.HOP:k * R.HOP + R.N_FRAME] += W * y10[i:i + R.N_FRAME]

    def bands(sig):
        fr = np.stack([W * sig[i:i + R.N_FRAME] for i in R.frame_starts(sig.size)])          # [M, 256]
        if dtype == np.float32:
            import scipy.fft     # numpy's rfft computes in float64; scipy keeps float32
            spec = scipy.fft.rfft(fr, R.NFFT, axis=1).astype(np.complex64)
        else:
            spec = np.fft.rfft(fr, R.NFFT, axis=1)
        p = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
        return np.stack([np.sqrt(np.sum(p[:, lo:hi], axis=1, dtype=dtype)) for lo, hi in R.BAND_RANGES])   # [15, M]

    X, Y = bands(xs), bands(ys)
    assert X.shape == Y.shape == (R.NUM_BANDS, K - 1)
    return X, Y, float(K)


def stoi_of_bands(X, Y, dtype=np.float64):
    """Step 4 on X, Y [15, M], M >= 30."""
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    eps = dtype(R.EPS)
    clip = dtype(1.0 + 10.0 ** (-R.BETA / 20.0))
    d = []
    for m in range(N_SEG, X.shape[1] + 1):
        xseg, yseg = X[:, m - N_SEG:m], Y[:, m - N_SEG:m]
        a = np.sqrt(np.sum(xseg * xseg, axis=1, keepdims=True) / (np.sum(yseg * yseg, axis=1, keepdims=True) + eps))
        yp = np.minimum(a * yseg, xseg * clip)
        xm = xseg - np.mean(xseg, axis=1, keepdims=True)
        ym = yp - np.mean(yp, axis=1, keepdims=True)
        d.append(np.sum(xm * ym, axis=1) / (np.sqrt(np.sum(xm * xm, axis=1)) * np.sqrt(np.sum(ym * ym, axis=1)) + eps))
    return float(np.mean(np.array(d, dtype=np.float64)))


def _normalised(seg, eps):
    """A 15 x 30 segment: per band minus its mean over (norm + eps), then per frame the same over the bands."""
    seg = seg - np.mean(seg, axis=1, keepdims=True)
    seg = seg / (np.sqrt(np.sum(seg * seg, axis=1, keepdims=True)) + eps)
    seg = seg - np.mean(seg, axis=0, keepdims=True)
    return seg / (np.sqrt(np.sum(seg * seg, axis=0, keepdims=True)) + eps)


def estoi_of_bands(X, Y, dtype=np.float64):
    """Step 5 on X, Y [15, M], M >= 30: the mean over m = 30 .. M of d_m = (1 / 30) sum x y."""
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    eps = dtype(R.EPS)
    d = []
    for m in range(N_SEG, X.shape[1] + 1):
        x = _normalised(X[:, m - N_SEG:m], eps)
        y = _normalised(Y[:, m - N_SEG:m], eps)
        d.append(np.sum(x * y, dtype=dtype) / dtype(N_SEG))
    return float(np.mean(np.array(d, dtype=np.float64)))


def stoi(s, y, sr, dtype=np.float64):
    """-> (STOI, K) at any rate in 8000 .. 48000."""
    X, Y, K = band_envelopes(s, y, sr, dtype)
    return (float("nan") if X is None else stoi_of_bands(X, Y, dtype)), K


def estoi(s, y, sr, dtype=np.float64):
    X, Y, _ = band_envelopes(s, y, sr, dtype)
    return float("nan") if X is None else estoi_of_bands(X, Y, dtype)


def eval_pair_ext(s, y, sr=16000, dtype=np.float64):
    """The six slots of one pair (cut to the common length by the caller), as AVSE_EVAL_ANY_RATE gives them."""
    s = np.asarray(s, np.float64).ravel()
    y = np.asarray(y, np.float64).ravel()
    assert s.size == y.size
    if s.size == 0:
        return np.full(NMETRICS, np.nan)
    X, Y, K = band_envelopes(s, y, sr, dtype)
    st = float("nan") if X is None else stoi_of_bands(X, Y, dtype)
    es = float("nan") if X is None else estoi_of_bands(X, Y, dtype)
    return np.array([R.snr(s, y), R.si_sdr(s, y), R.seg_snr(s, y, sr), st, K, es], dtype=np.float64)


def eval_pairs_ext(ref, deg, sample_rate=16000, dtype=np.float64):
    """[n, 6] float64; each pair cut to min(len ref, len deg)."""
    rows = []
    for s, y in zip(ref, deg):
        s = np.asarray(s).ravel()
        y = np.asarray(y).ravel()
        n = min(s.size, y.size)
        rows.append(eval_pair_ext(s[:n], y[:n], sample_rate, dtype))
    return np.stack(rows) if rows else np.zeros((0, NMETRICS))


# ---- the GPU tests' inputs (tests/test_gpu_eval_ext.py, tools/eval_ext_checks.py) ----------------------------------
# (name, sample rate, samples, seed, snr_db, stationary, K or None where it is not pinned)
CASES = (
    ("speech_44100", 44100, 44100, 400, 5.0, False, 50),
    ("speech_22050", 22050, 22050, 401, 0.0, False, 50),
    ("speech_11025", 11025, 11025, 402, 10.0, False, 60),
    ("speech_16001", 16001, 16001, 403, 5.0, False, 59),
    ("speech_47999", 47999, 30000, 404, 5.0, False, 47),
    ("speech_16000", 16000, 16000, 405, 5.0, False, 50),
    ("speech_8000", 8000, 8000, 406, 0.0, False, 49),
    ("boundary_44100_18063", 44100, 18063, 410, 10.0, True, 30),
    ("boundary_44100_18064", 44100, 18064, 411, 10.0, True, 31),
    ("boundary_44100_18700", 44100, 18700, 412, 10.0, True, 32),
    ("boundary_22050_9032", 22050, 9032, 413, 10.0, True, 31),
    ("boundary_22050_9031", 22050, 9031, 414, 10.0, True, 30),
    ("boundary_16001_6555", 16001, 6555, 415, 10.0, True, 31),
    ("boundary_16001_6554", 16001, 6554, 416, 10.0, True, 30),
    ("noframes_44100_1000", 44100, 1000, 417, 10.0, True, 0),
)


def cases():
    """[(name, sr, clean, degraded, K)]"""
    return [(name, sr) + R.speech_like(seed, n, sr, snr_db, stationary=stat) + (K,)
            for name, sr, n, seed, snr_db, stat, K in CASES]
