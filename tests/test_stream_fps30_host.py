"""Host side of streaming with 30-fps video ("30-fps video"): the rule of which geometries stream
(avse_stream_supported, no GPU) with n_fft 800 / hop 200 at 24 kHz and 1600 / 400 at 48 kHz added, and the float64 facts
the 800-point kernels (csrc/frame800.h) rest on, against oracle/librosa_ref.py: the mel bank at 48 kHz is the 24 kHz bank
and both end at bin 266, a real 800-point frame is a packed 400-point transform split 20 x 20, and a frame of 1600
samples is two interleaved 800-point frames with a twiddle combine, in both directions.  The gates are those of
tests/test_stream_rates_host.py."""
import numpy as np
import pytest

from oracle import librosa_ref as R

RATES = {24000: (800, 200), 48000: (1600, 400)}
KTOP = 266          # last bin the bank touches; bin 267 is 8010 Hz


def test_stream_supported_accepts_the_30_fps_geometries():
    from avse_amd import ops
    for sr, (n_fft, hop) in RATES.items():
        assert ops.stream_supported(sr, n_fft, hop, frames_per_slice=24) == 0, sr
        assert ops.stream_supported(sr, n_fft, hop, frames_per_slice=24, return_message=True) == (0, "")


@pytest.mark.parametrize("sr,n_fft,hop,fmax,why", [
    (16000, 800, 200, 8000.0, "800 is the 24 kHz frame"),
    (24000, 1600, 400, 8000.0, "1600 is the 48 kHz frame"),
    (48000, 1601, 400, 8000.0, "29.97 fps: int(48000 / 29.97) is odd"),
    (48000, 1600, 400, 24000.0, "the bank reaches above bin 266"),
])
def test_stream_supported_refuses_with_a_message(sr, n_fft, hop, fmax, why):
    from avse_amd import ops
    rc, msg = ops.stream_supported(sr, n_fft, hop, frames_per_slice=24, fmax=fmax, return_message=True)
    print(f"{sr} / {n_fft} / {hop} / fmax {fmax}: status {rc}: {msg}")
    assert rc == 3 and msg, why
    if n_fft == 1601:
        assert "4 * hop" in msg


def test_the_frame_rule_of_the_reference_gives_these_geometries():
    from avse_amd import data_processor
    for sr, (n_fft, hop) in RATES.items():
        g = data_processor.frame_geometry(sr, 200, 1, 30.0)
        assert (g["n_fft"], g["hop_length"], g["spectrogram_samples_per_slice"]) == (n_fft, hop, 24)
        assert 24 * hop == sr // 5                                           # a slice is exactly 24 hops: no drift
    assert data_processor.frame_geometry(48000, 200, 1, 29.97)["n_fft"] == 1601


def test_the_bank_is_one_bank_and_ends_at_bin_266():
    fb24 = R.mel_filterbank(24000, 800, n_mels=80, fmin=0, fmax=8000)
    fb48 = R.mel_filterbank(48000, 1600, n_mels=80, fmin=0, fmax=8000)
    assert fb24.shape == (80, 401) and fb48.shape == (80, 801)
    assert np.array_equal(fb48[:, :401], fb24)                               # max |difference| 0
    for fb in (fb24, fb48):
        assert not fb[:, KTOP + 1:].any() and fb[:, KTOP].any()              # last non-zero column 266
        assert not fb[:, 0].any() and fb[:, 1].any()
        widths = [np.flatnonzero(row)[-1] - (np.flatnonzero(row)[0] & ~3) + 1 for row in fb]
        print(f"widest band from a 4-aligned start: {max(widths)} bins")
        assert max(widths) <= 24                                             # the kernels' band table
        pinv = np.linalg.pinv(fb)
        assert not pinv[KTOP + 1:].any()                                     # the ISTFT inverts bins 0 .. 266 only
    assert np.array_equal(np.linalg.pinv(fb48)[:KTOP + 1], np.linalg.pinv(fb24)[:KTOP + 1])


def dft20(v):
    """The 20-point DFT along axis 0 (the kernels' butterfly is this, 4 x 5)."""
    n = np.arange(20)
    return np.exp(-2j * np.pi * np.outer(n, n) / 20) @ v


def rfft800_split(xw):
    """rfft of 800 real samples, bins 0 .. 266, as csrc/frame800.h computes it: the packed 400-point transform
    z[n] = x[2n] + i x[2n+1], n = n1 + 20 n2, k = k2 + 20 k1, then the untangling of the pairs (k, 400 - k), k <= 200."""
    z = (xw[0::2] + 1j * xw[1::2]).reshape(20, 20)                           # [n2, n1]
    n1, k2 = np.arange(20)[None, :], np.arange(20)[:, None]
    y = dft20(z) * np.exp(-2j * np.pi * n1 * k2 / 400)                       # step 1: [k2, n1], twiddle W400^{n1 k2}
    Z = dft20(y.T).reshape(400)                                              # step 2: [k1, k2] -> Z[k2 + 20 k1]
    k = np.arange(201)
    zk, zm = Z[k], np.conj(Z[(400 - k) % 400])
    E, WO = 0.5 * (zk + zm), -0.5j * np.exp(-2j * np.pi * k / 800) * (zk - zm)
    X = np.empty(401, np.complex128)
    X[k] = E + WO                                                            # X[k]
    X[400 - k[:200]] = np.conj(E - WO)[:200]                                 # X[400 - k] = conj(Y)
    return X[:KTOP + 1]


@pytest.mark.parametrize("sr", sorted(RATES))
def test_analysis_identities_against_the_oracle(sr):
    """The 20 x 20 split with its untangling is rfft of the windowed 800-sample frame; at 48 kHz
    X[k] = sum_r W_N^{rk} DFT800(xw[r::2])[k], k <= 266, each phase computed by that split."""
    N, hop = RATES[sr]
    P = N // 800
    rng = np.random.default_rng(11)
    x = rng.normal(0, 3000, 6 * N)
    D = R.stft(x, n_fft=N, hop_length=hop)                                   # complex64 [N / 2 + 1, T]
    win = R.hann_periodic(N)
    xp = np.pad(x, N // 2, mode="reflect")
    k = np.arange(KTOP + 1)
    worst = worst32 = worst_split = 0.0
    for t in (0, 3, D.shape[1] - 1):
        xw = win * xp[hop * t:hop * t + N]
        ref = np.fft.rfft(xw)[:KTOP + 1]                                     # what R.stft computes before its cast
        peak = np.abs(ref).max()
        for r in range(P):                                                   # the split itself, on every phase
            ph = np.fft.rfft(xw[r::P])
            worst_split = max(worst_split, np.abs(rfft800_split(xw[r::P]) - ph[:KTOP + 1]).max() / np.abs(ph).max())
        X = sum(np.exp(-2j * np.pi * r * k / N) * rfft800_split(xw[r::P]) for r in range(P))
        worst = max(worst, np.abs(X - ref).max() / peak)
        worst32 = max(worst32, np.abs(X - D[:KTOP + 1, t]).max() / peak)
    print(f"{sr}: 20 x 20 split {worst_split:.1e}, analysis identity {worst:.1e} of the frame's peak (float64), "
          f"{worst32:.1e} against the complex64 oracle")
    assert worst_split <= 1e-13 and worst <= 1e-13 and worst32 <= 3e-7


@pytest.mark.parametrize("sr", sorted(RATES))
def test_synthesis_identities_against_the_oracle(sr):
    """For Z zero above bin 266 the phase-r samples of irfft(Z, N) are irfft800(Y_r) / P, Y_r[k] = Z[k] W_N^{-rk}: no
    Nyquist term (bin 266 < 400); and the same through the oracle's overlap-add."""
    N, hop = RATES[sr]
    P = N // 800
    rng = np.random.default_rng(12)
    win = R.hann_periodic(N)
    k = np.arange(KTOP + 1)
    Z = np.zeros((N // 2 + 1, 5), np.complex128)
    Z[:KTOP + 1] = rng.normal(size=(KTOP + 1, 5)) + 1j * rng.normal(size=(KTOP + 1, 5))

    def frames_of(Zb):
        out = np.empty((N, Zb.shape[1]))
        for r in range(P):
            Y = np.zeros((401, Zb.shape[1]), np.complex128)
            Y[:KTOP + 1] = Zb[:KTOP + 1] * np.exp(2j * np.pi * r * k / N)[:, None]
            out[r::P] = np.fft.irfft(Y, n=800, axis=0) / P
        return out

    full = np.fft.irfft(Z, n=N, axis=0)
    err = np.abs(frames_of(Z) - full).max() / np.abs(full).max()
    print(f"{sr}: synthesis identity {err:.1e} of the peak")
    assert err <= 1e-13
    Zc = Z.astype(np.complex64).astype(np.complex128)                        # complex128: numpy's irfft keeps the input's precision
    y_ref = R.istft(Zc, hop_length=hop, dtype=np.float64)
    fr = frames_of(Zc)
    y = np.zeros(N + hop * 4)
    for t in range(5):
        y[hop * t:hop * t + N] += win * fr[:, t]
    wss = R.window_sumsquare(5, hop, N, dtype=np.float64)
    nz = wss > np.finfo(np.float64).tiny
    y[nz] /= wss[nz]
    err = np.abs(y[N // 2:-(N // 2)] - y_ref).max() / np.abs(y_ref).max()
    print(f"{sr}: two-phase frames through the oracle's overlap-add: {err:.1e} of the peak")
    assert err <= 1e-12
