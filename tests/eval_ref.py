"""Float64 reference of avse_eval_pairs (include/avse.h): SNR, scale-invariant SDR, segmental SNR and STOI for one
(clean, degraded) pair, written from the header's definitions with numpy.  scipy is used only by the tests that pin
the resampling formula against scipy.signal.resample_poly.

`dtype=np.float32` runs the STOI framing, FFT and band arithmetic in float32 (the resampling, the frame energies and
the mask stay float64): the yardstick the GPU tests derive their STOI gate from."""
import math

import numpy as np

EPS = 2.0 ** -52
NMETRICS = 5
SNR, SI_SDR, SEG_SNR, STOI, STOI_KEPT = range(5)
FS = 10000
N_FRAME, HOP, NFFT, NUM_BANDS, MIN_FREQ, N_SEG, BETA, DYN_RANGE = 256, 128, 512, 15, 150.0, 30, -15.0, 40.0
MAX_RATIO = 24
BAND_RANGES = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69),
               (69, 87), (87, 109), (109, 138), (138, 174), (174, 219))


def band_table():
    """The 15 half-open bin ranges: the bins nearest to 150 * 2^(j/3) * 2^(-+1/6) Hz on the 10000 / 512 Hz grid."""
    f = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    out = []
    for j in range(NUM_BANDS):
        cf = MIN_FREQ * 2.0 ** (j / 3.0)
        lo = int(np.argmin((f - cf * 2.0 ** (-1.0 / 6.0)) ** 2))
        hi = int(np.argmin((f - cf * 2.0 ** (1.0 / 6.0)) ** 2))
        out.append((lo, hi))
    return tuple(out)


def stoi_window():
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * (np.arange(N_FRAME) + 1.0) / (N_FRAME + 1.0)))


def ratio(sr):
    g = math.gcd(FS, int(sr))
    return FS // g, int(sr) // g


def _i0(x):
    """Modified Bessel function of the first kind, order 0: its power series."""
    x = np.asarray(x, np.float64)
    q = x * x / 4.0
    term = np.ones_like(q)
    total = np.ones_like(q)
    for k in range(1, 64):
        term = term * q / (k * k)
        total = total + term
    return total


def resample_taps(up, down):
    """scipy.signal.resample_poly's default filter for (up, down): firwin(2H + 1, 1 / max, window=('kaiser', 5.0))
    scaled by up, H = 10 max(up, down)."""
    mx = max(up, down)
    H = 10 * mx
    fc = 1.0 / mx
    i = np.arange(2 * H + 1, dtype=np.float64) - H
    h = fc * np.sinc(fc * i) * _i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (i / H) ** 2))) / _i0(5.0)
    h = h / h.sum()
    return h * up


def resample(x, up, down):
    """y[k] = sum_j h[H + k down - j up] x[j] over the j keeping the index in [0, 2H]; ceil(n up / down) outputs."""
    x = np.asarray(x, np.float64)
    if up == down:
        return x.copy()
    n = x.size
    h = resample_taps(up, down)
    H = (h.size - 1) // 2
    n10 = -(-n * up // down)
    y = np.zeros(n10)
    if n == 0:
        return y
    k = np.arange(n10, dtype=np.int64)
    j0 = -((H - k * down) // up)          # ceil((k down - H) / up)
    ntap = 2 * H // up + 1
    for t in range(ntap):                 # ascending j: the order the kernel accumulates in
        j = j0 + t
        idx = H + k * down - j * up
        ok = (idx >= 0) & (idx <= 2 * H) & (j >= 0) & (j < n)
        y[ok] += h[idx[ok]] * x[j[ok]]
    return y


def snr(s, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(np.sum(s * s) / np.sum((s - y) ** 2)))


def si_sdr(s, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        s2 = np.sum(s * s)
        a = np.sum(s * y) / s2
        return float(10.0 * np.log10(a * a * s2 / np.sum((a * s - y) ** 2)))


def seg_snr(s, y, sr):
    win = (3 * int(sr) + 50) // 100      # round(0.03 sr), halves up
    skip = win // 4
    n = s.size
    if n < win:
        return float("nan")
    w = 0.5 * (1.0 - np.cos(2.0 * np.pi * (np.arange(win) + 1.0) / (win + 1.0)))
    vals = []
    for i in range(0, n - win + 1, skip):
        ws = w * s[i:i + win]
        wd = w * (s[i:i + win] - y[i:i + win])
        v = 10.0 * np.log10(np.sum(ws * ws) / (np.sum(wd * wd) + EPS) + EPS)
        vals.append(min(max(v, -10.0), 35.0))
    return float(np.sum(np.array(vals)) / len(vals))


def frame_starts(n):
    return range(0, n - N_FRAME, HOP)      # i < n - 256, strict


def frame_energies(x10):
    """e_i = 20 log10(||W x_i|| + eps) of the clean resampled signal, float64."""
    W = stoi_window()
    return np.array([20.0 * np.log10(np.sqrt(np.sum((W * x10[i:i + N_FRAME]) ** 2)) + EPS)
                     for i in frame_starts(x10.size)])


def mask_margin(s, sr):
    """The smallest |e_i - (max(e) - 40)| in dB over the pair's frames (inf without frames or without STOI)."""
    up, down = ratio(sr)
    if max(up, down) > MAX_RATIO:
        return float("inf")
    e = frame_energies(resample(np.asarray(s, np.float64), up, down))
    if e.size == 0:
        return float("inf")
    return float(np.min(np.abs(e - (e.max() - DYN_RANGE))))


def stoi(s, y, sr, dtype=np.float64):
    """-> (STOI, K).  (nan, 0.0) when max(up, down) > 24."""
    up, down = ratio(sr)
    if max(up, down) > MAX_RATIO:
        return float("nan"), 0.0
    x10 = resample(s, up, down)
    y10 = resample(y, up, down)
    e = frame_energies(x10)
    starts = np.array(list(frame_starts(x10.size)), dtype=np.int64)
    if e.size == 0:
        return float("nan"), 0.0
    kept = starts[e > e.max() - DYN_RANGE]
    K = kept.size
    W = stoi_window().astype(dtype)
    xs = np.zeros((K - 1) * HOP + N_FRAME, dtype)
    ys = np.zeros_like(xs)
    x10 = x10.astype(dtype)
    y10 = y10.astype(dtype)
    for k, i in enumerate(kept):
        xs[k * HOP:k * HOP + N_FRAME] += W * x10[i:i + N_FRAME]
        ys[k * HOP:k * HOP + N_FRAME] += W * y10[i:i + N_FRAME]
    M = K - 1
    if M < N_SEG:
        return float("nan"), float(K)
    ctype = np.complex64 if dtype == np.float32 else np.complex128

    def bands(sig):
        fr = np.stack([W * sig[i:i + N_FRAME] for i in frame_starts(sig.size)])          # [M, 256]
        if dtype == np.float32:
            import scipy.fft     # numpy's rfft computes in float64; scipy keeps float32
            spec = scipy.fft.rfft(fr, NFFT, axis=1).astype(ctype)
        else:
            spec = np.fft.rfft(fr, NFFT, axis=1)
        p = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
        return np.stack([np.sqrt(np.sum(p[:, lo:hi], axis=1, dtype=dtype)) for lo, hi in BAND_RANGES])   # [15, M]

    X = bands(xs)
    Y = bands(ys)
    assert X.shape[1] == M
    eps = dtype(EPS)
    clip = dtype(1.0 + 10.0 ** (-BETA / 20.0))
    d = []
    for m in range(N_SEG, M + 1):
        xseg = X[:, m - N_SEG:m]
        yseg = Y[:, m - N_SEG:m]
        a = np.sqrt(np.sum(xseg * xseg, axis=1, keepdims=True) / (np.sum(yseg * yseg, axis=1, keepdims=True) + eps))
        yp = np.minimum(a * yseg, xseg * clip)
        xm = xseg - np.mean(xseg, axis=1, keepdims=True)
        ym = yp - np.mean(yp, axis=1, keepdims=True)
        d.append(np.sum(xm * ym, axis=1) /
                 (np.sqrt(np.sum(xm * xm, axis=1)) * np.sqrt(np.sum(ym * ym, axis=1)) + eps))
    return float(np.mean(np.array(d, dtype=np.float64))), float(K)


def eval_pair(s, y, sr=16000, dtype=np.float64):
    """The five metrics of one pair (cut to the common length by the caller)."""
    s = np.asarray(s, np.float64).ravel()
    y = np.asarray(y, np.float64).ravel()
    assert s.size == y.size
    if s.size == 0:
        return np.full(NMETRICS, np.nan)
    st, K = stoi(s, y, sr, dtype)
    return np.array([snr(s, y), si_sdr(s, y), seg_snr(s, y, sr), st, K], dtype=np.float64)


def eval_pairs(ref, deg, sample_rate=16000, dtype=np.float64):
    """[n, 5] float64; each pair cut to min(len ref, len deg)."""
    rows = []
    for s, y in zip(ref, deg):
        s = np.asarray(s).ravel()
        y = np.asarray(y).ravel()
        n = min(s.size, y.size)
        rows.append(eval_pair(s[:n], y[:n], sample_rate, dtype))
    return np.stack(rows) if rows else np.zeros((0, NMETRICS))


def speech_like(seed, n, sr=16000, snr_db=10.0, pause_ends=False, stationary=False):
    """Fixed-seed test input: int16-scale coloured noise under a 3 Hz envelope with gated pauses (or stationary noise),
    plus white noise at snr_db, both rounded to integers.  -> (clean, degraded) float32."""
    rng = np.random.default_rng(seed)
    m = max(n, 512)                        # a short signal is the head of a 512-sample one: its scale stays int16's
    white = rng.normal(0.0, 1.0, m + 63)
    col = np.convolve(white, np.exp(-np.arange(64) / 6.0), mode="valid")     # low-pass coloured
    col = (col / np.std(col))[:n]
    t = np.arange(n) / float(sr)
    if stationary:
        env = np.ones(n)
    else:
        env = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * t + rng.uniform(0.0, 2.0 * np.pi))
        gate = (np.sin(2.0 * np.pi * 0.9 * t + rng.uniform(0.0, 2.0 * np.pi)) > -0.5).astype(np.float64)
        env = env * (gate + (1.0 - gate) * 1e-3)
        if pause_ends:
            edge = min(n // 4, int(0.08 * sr))
            env[:edge] *= 1e-4
            env[n - edge:] *= 1e-4
    clean = np.round(4000.0 * env * col)
    p = np.mean(clean ** 2)
    noise = rng.normal(0.0, 1.0, n) * np.sqrt(max(p, 1.0) / 10.0 ** (snr_db / 10.0))
    deg = np.round(clean + noise)
    return clean.astype(np.float32), deg.astype(np.float32)


# ---- the GPU tests' inputs (tests/test_gpu_eval.py, tools/eval_checks.py) ------------------------------------------
RAGGED_LENGTHS = (1, 7, 479, 480, 481, 6553, 6554, 12001, 16000, 23999, 47840, 48000)
# (sample rate, samples): stationary noise, every frame kept; M = 29 / 30 / 31 and the no-frame case per resampling path
BOUNDARY = ((16000, 400), (16000, 6553), (16000, 6554), (16000, 6760), (8000, 3276), (8000, 3278), (10000, 4096),
            (10000, 4097))
MASK_MARGIN_DB = 0.01


def ragged_cases():
    """The one-launch batch at 16 kHz: [(name, clean, degraded)] with 0 dB and 10 dB noise, one pair with deg == ref
    (16000 samples) and one whose pauses silence the first and the last frames (23999 samples)."""
    out = []
    for k, n in enumerate(RAGGED_LENGTHS):
        # the pairs shorter than one envelope period are stationary: a gated pause would leave them a few units of noise
        s, y = speech_like(100 + k, n, 16000, snr_db=(0.0, 10.0)[k % 2], pause_ends=(n == 23999), stationary=(n < 1000))
        if n == 16000:
            y = s.copy()
        out.append(("ragged_%d" % n, s, y))
    return out


def boundary_cases():
    return [("boundary_%d_%d" % (sr, n), sr) + speech_like(200 + k, n, sr, 10.0, stationary=True)
            for k, (sr, n) in enumerate(BOUNDARY)]
