"""Host side of streaming at 32 and 48 kHz ("32 and 48 kHz"): the one rule of which geometries
stream (avse_stream_supported, no GPU), and the float64 facts the P-phase kernels rest on, against oracle/librosa_ref.py:
the mel bank at 32 / 48 kHz is the 16 kHz bank on bins 0 .. 319, and a frame of N = 640 P samples is P interleaved
640-point frames with a twiddle combine, in both directions."""
import numpy as np
import pytest

from oracle import librosa_ref as R

RATES = {16000: (640, 160), 32000: (1280, 320), 48000: (1920, 480)}


def test_stream_supported_accepts_the_built_geometries():
    from avse_amd import ops
    for sr, (n_fft, hop) in RATES.items():
        assert ops.stream_supported(sr, n_fft, hop) == 0, sr
        assert ops.stream_supported(sr, n_fft, hop, return_message=True) == (0, "")


@pytest.mark.parametrize("sr,n_fft,hop,fmax,why", [
    (44100, 1764, 441, 8000.0, "passes the drift condition, but 1764 is no multiple of 640"),
    (16000, 533, 133, 8000.0, "29.97 fps: slices drift"),
    (48000, 1920, 480, 24000.0, "the bank reaches above bin 320"),
    (48000, 1920, 400, 8000.0, "n_fft != 4 * hop"),
])
def test_stream_supported_refuses_with_a_message(sr, n_fft, hop, fmax, why):
    from avse_amd import ops
    rc, msg = ops.stream_supported(sr, n_fft, hop, fmax=fmax, return_message=True)
    print(f"{sr} / {n_fft} / {hop} / fmax {fmax}: status {rc}: {msg}")
    assert rc == 3 and msg, why
    if sr == 44100:       # the message names the rates that are built
        assert "16" in msg and "32" in msg and "48" in msg


def test_stream_supported_is_the_rule_of_create_and_rejects_nonsense():
    from avse_amd import _lib, ops
    assert ops.stream_supported(0, 640, 160) == 1 and ops.stream_supported(16000, 640, 160, n_mels=0) == 1
    assert ops.stream_supported(16000, 640, 160, n_mels=40) == 3          # the kernels are built for 80 bands
    assert ops.stream_supported(32000, 1920, 480) == 3                     # 1920 is the 48 kHz frame
    assert "avse_stream_supported" in _lib.SIGNATURES


@pytest.mark.parametrize("sr", [32000, 48000])
def test_the_bank_is_the_16_khz_bank_and_ends_below_bin_320(sr):
    n_fft = RATES[sr][0]
    fb16 = R.mel_filterbank(16000, 640, n_mels=80, fmin=0, fmax=8000)
    fb = R.mel_filterbank(sr, n_fft, n_mels=80, fmin=0, fmax=8000)
    assert fb.shape == (80, n_fft // 2 + 1)
    assert np.array_equal(fb[:, :321], fb16)                               # max |difference| 0
    assert not fb[:, 320:].any() and fb[:, 319].any()                      # last non-zero column 319
    widths = [np.flatnonzero(row)[-1] - (np.flatnonzero(row)[0] & ~1) + 1 for row in fb]
    assert max(widths) <= 24                                               # the kernels' band table (even starts)
    pinv = np.linalg.pinv(fb)
    assert not pinv[320:].any()                                            # the ISTFT inverts bins 0 .. 319 only


@pytest.mark.parametrize("sr", [32000, 48000])
def test_polyphase_identities_against_the_oracle(sr):
    """analysis: X[k] = sum_r W_N^{rk} DFT640(xw[r::P])[k], k <= 320; synthesis: the phase-r samples of irfft(Z, N) are
    irfft640(Y_r) / P for Z zero above bin 320."""
    N, hop = RATES[sr]
    P = N // 640
    rng = np.random.default_rng(11)
    x = rng.normal(0, 3000, 6 * N)
    D = R.stft(x, n_fft=N, hop_length=hop)                                 # complex64 [N / 2 + 1, T]
    win = R.hann_periodic(N)
    xp = np.pad(x, N // 2, mode="reflect")
    k = np.arange(321)
    worst = worst32 = 0.0
    for t in (0, 3, D.shape[1] - 1):
        xw = win * xp[hop * t:hop * t + N]
        X = sum(np.exp(-2j * np.pi * r * k / N) * np.fft.fft(xw[r::P])[:321] for r in range(P))
        ref = np.fft.rfft(xw)[:321]                                        # what R.stft computes before its cast
        peak = np.abs(ref).max()
        worst = max(worst, np.abs(X - ref).max() / peak)
        worst32 = max(worst32, np.abs(X - D[:321, t]).max() / peak)
    print(f"{sr}: analysis identity {worst:.1e} of the frame's peak (float64), {worst32:.1e} against the complex64 oracle")
    assert worst <= 1e-13 and worst32 <= 3e-7
    # synthesis, on a band-limited spectrum (bin 320 non-zero: the general form)
    Z = np.zeros((N // 2 + 1, 5), np.complex128)
    Z[:321] = rng.normal(size=(321, 5)) + 1j * rng.normal(size=(321, 5))
    full = np.fft.irfft(Z, n=N, axis=0)
    frames = np.empty_like(full)
    for r in range(P):
        Y = Z[:321] * np.exp(2j * np.pi * r * k / N)[:, None]
        Y[320] = 2 * Y[320].real
        frames[r::P] = np.fft.irfft(Y, n=640, axis=0) / P
    err = np.abs(frames - full).max() / np.abs(full).max()
    print(f"{sr}: synthesis identity {err:.1e} of the peak")
    assert err <= 1e-13
    # and through the oracle's overlap-add: the same waveform
    Zc = Z.astype(np.complex64).astype(np.complex128)                      # complex128: numpy's irfft keeps the input's precision
    y_ref = R.istft(Zc, hop_length=hop, dtype=np.float64)
    y = np.zeros(N + hop * 4)
    for t in range(5):
        fr = np.empty(N)
        for r in range(P):
            Y = Zc[:321, t] * np.exp(2j * np.pi * r * k / N)
            Y[320] = 2 * Y[320].real
            fr[r::P] = np.fft.irfft(Y, n=640) / P
        y[hop * t:hop * t + N] += win * fr
    wss = R.window_sumsquare(5, hop, N, dtype=np.float64)
    nz = wss > np.finfo(np.float64).tiny
    y[nz] /= wss[nz]
    err = np.abs(y[N // 2:-(N // 2)] - y_ref).max() / np.abs(y_ref).max()
    print(f"{sr}: polyphase frames through the oracle's overlap-add: {err:.1e} of the peak")
    assert err <= 1e-12
