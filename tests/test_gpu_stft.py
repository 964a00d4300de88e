"""K1 parity: libavse spectrogram vs the numpy librosa restatement (oracle/librosa_ref.py).

Tolerances (stated here, DESIGN.md "Parity"): the HIP kernel computes in float32 (the oracle in
float64 like librosa's np.fft path), so mel-dB values are compared with
  max |dB_gpu - dB_oracle| <= 1e-3 dB and RMS <= 1e-4 dB (measured round 1: ~1.2e-5 dB max),
and the complex STFT relative to the utterance's peak |X|: max <= 2e-6 * peak-based scale.
Slice / frame / hop indices are integers and compared exactly.
"""
import numpy as np
import pytest
import torch

from audio_edge_inputs import clamp_conditions, oracle_pre, segments_533_input, sliced_segments_input
from conftest import synth_audio
from oracle import librosa_ref as R

pytestmark = pytest.mark.gpu

DB_MAX = 1e-3
DB_RMS = 1e-4


def _ops():
    from avse_amd import ops
    return ops


def _check_db(got, ref):
    d = np.abs(got.astype(np.float64) - ref)
    assert d.max() <= DB_MAX, f"max dB error {d.max()}"
    assert np.sqrt(np.mean(d ** 2)) <= DB_RMS, f"rms dB error {np.sqrt(np.mean(d ** 2))}"


@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
def test_segments_match_oracle(gpu, pad_mode):
    ops = _ops()
    rng = np.random.default_rng(1)
    x = synth_audio(rng, 64, 3200)
    got = ops.spectrogram(torch.from_numpy(x).to(gpu), pad_mode=pad_mode).cpu().numpy()
    assert got.shape == (64, 80, 21)
    for u in range(64):
        ref, _ = R.signal_to_spectrogram(x[u], 16000, 640, 160, pad_mode=pad_mode)
        _check_db(got[u], ref)


def test_sliced_segments_drop_last_frame_but_keep_its_max(gpu):
    ops = _ops()
    # the LAST frame is the loudest, so the top_db floor depends on the dropped frame — and the rest of the utterance is
    # quiet enough for the clamp to reach it (audio_edge_inputs.wide: 34-50 % of the elements at the floor, the oracle
    # 2-5 dB away from "maximum over the kept frames only"; a plain synth_audio tail x 8 left the clamped share at 0,
    # so nothing here depended on the maximum)
    x = sliced_segments_input()
    for u in range(16):
        clamp_conditions(oracle_pre(x[u], 640, 160)[0], 80.0, 20, dropped=True)
    got = ops.spectrogram(torch.from_numpy(x).to(gpu), frames_per_slice=20).cpu().numpy()
    assert got.shape == (16, 1, 80, 20)
    for u in range(16):
        ref = R.preprocess_audio_signal(x[u], 16000, 200, 1, 25.0)
        _check_db(got[u], ref)


@pytest.mark.parametrize("n_samples", [48000, 47000, 50000])
def test_utterance_slicing(gpu, n_samples):
    """preprocess_audio_signal on a 3-s utterance (15 slices; 301 frames -> chunked top_db path)."""
    ops = _ops()
    from avse_amd import data_processor as dp
    from avse_amd.audio_io import AudioSignal
    rng = np.random.default_rng(3)
    x = synth_audio(rng, 1, n_samples)[0]
    sig = AudioSignal(x.copy(), 16000)
    got = dp.preprocess_audio_signal(sig, 200, 15, 25.0)
    assert sig.get_number_of_samples() == 48000          # padded / truncated in place
    ref = R.preprocess_audio_signal(x, 16000, 200, 15, 25.0)
    assert got.shape == ref.shape == (15, 80, 20)
    _check_db(got, ref)


def test_batched_utterances(gpu):
    ops = _ops()
    rng = np.random.default_rng(4)
    x = synth_audio(rng, 6, 48000)
    got = ops.spectrogram(torch.from_numpy(x).to(gpu), frames_per_slice=20).cpu().numpy()
    assert got.shape == (6, 15, 80, 20)
    for u in range(6):
        _check_db(got[u], R.preprocess_audio_signal(x[u], 16000, 200, 15, 25.0))


def test_complex_stft_matches(gpu):
    ops = _ops()
    rng = np.random.default_rng(5)
    x = synth_audio(rng, 4, 3200)
    _, D = ops.spectrogram(torch.from_numpy(x).to(gpu), return_stft=True)
    D = D.cpu().numpy()
    for u in range(4):
        ref = R.stft(x[u], 640, 160).astype(np.complex128)
        err = np.abs(D[u] - ref).max() / np.abs(ref).max()
        assert err < 2e-6, err


def test_29_97_fps_utterances(gpu):
    """n_fft = int(16000/29.97) = 533 = 13 x 41 (k_spec533, the prime-factor kernel): 2-s utterances, 241 frames in
    chunks of 25 (the atomicMax top_db path)."""
    ops = _ops()
    rng = np.random.default_rng(6)
    g = R.frame_geometry(16000, 200, 10, 29.97)
    assert (g["n_fft"], g["hop_length"], g["spectrogram_samples_per_slice"]) == (533, 133, 24)
    x = synth_audio(rng, 2, g["signal_length"])
    got = ops.spectrogram(torch.from_numpy(x).to(gpu), n_fft=533, hop_length=133, frames_per_slice=24).cpu().numpy()
    for u in range(2):
        _check_db(got[u], R.preprocess_audio_signal(x[u], 16000, 200, 10, 29.97))


def test_silence_is_floor(gpu):
    ops = _ops()
    x = np.zeros((2, 3200), np.float32)
    got = ops.spectrogram(torch.from_numpy(x).to(gpu)).cpu().numpy()
    assert np.all(got == np.float32(-100.0))


def test_tone_peaks_in_expected_band(gpu):
    ops = _ops()
    sr = 16000
    t = np.arange(3200) / sr
    x = (10000 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)[None]
    got = ops.spectrogram(torch.from_numpy(x).to(gpu)).cpu().numpy()[0]
    fb = R.mel_filterbank(sr, 640, 80, 0, 8000)
    expected_band = int(np.argmax(fb[:, 40]))          # bin 40 = 1000 Hz
    assert int(np.argmax(got[:, 10])) == expected_band


def test_config2_batch_4096(gpu):
    """BASELINE configs[1] (STFT only, 4096 200-ms segments): the kernel at the benchmarked size, 256 spread
    segments against the oracle; the sliced layout is the unsliced one without its last frame."""
    ops = _ops()
    import bench
    rng = np.random.default_rng(77)
    x, _ = bench.synth(rng, 4096, video=False)
    d = torch.from_numpy(x).to(gpu)
    got = ops.spectrogram(d, frames_per_slice=20).cpu().numpy()
    full = ops.spectrogram(d).cpu().numpy()
    assert got.shape == (4096, 1, 80, 20) and full.shape == (4096, 80, 21)
    np.testing.assert_array_equal(got[:, 0], full[:, :, :20])
    for u in sorted(set(np.linspace(0, 4095, 256).astype(int))):
        _check_db(got[u], R.preprocess_audio_signal(x[u], 16000, 200, 1, 25.0))


@pytest.mark.parametrize("n_mels,fmin,fmax,sr,top_db", [(64, 0.0, 8000.0, 16000, 80.0), (80, 50.0, 7600.0, 16000, 80.0),
                                                       (72, 0.0, 11025.0, 22050, None), (17, 0.0, 8000.0, 16000, 60.0)])
def test_segment_kernel_other_banks(gpu, n_mels, fmin, fmax, sr, top_db):
    """200-ms segments (3200 samples, n_fft 640, hop 160) with other Slaney banks against the restated librosa chain:
    banks whose bands fit the padded 24-bin rows run the segment kernel k_spec_seg (80 bands from 50 Hz), wider ones
    (17 / 64 bands, 72 at 22.05 kHz) k_spec640's generic band loop; top_db off and at 60 dB."""
    ops = _ops()
    rng = np.random.default_rng(11)
    x = synth_audio(rng, 40, 3200)
    got = ops.spectrogram(torch.from_numpy(x).to(gpu), sample_rate=sr, n_mels=n_mels, fmin=fmin, fmax=fmax,
                          top_db=top_db).cpu().numpy()
    assert got.shape == (40, n_mels, 21)
    fb = R.mel_filterbank(sr, 640, n_mels, fmin, fmax)
    for u in range(40):
        mag, _ = R.magphase(R.stft(x[u], 640, 160))
        _check_db(got[u], R.amplitude_to_db(fb @ mag, top_db=top_db))


@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
def test_533_segments_match_oracle(gpu, pad_mode):
    """29.97 / 30 fps 200-ms segments: 3200 samples -> 25 frames of n_fft 533 / hop 133 in one k_spec533 block (top_db
    in-kernel), unsliced and sliced to 24 frames (the dropped 25th frame still sets the top_db floor: it is made the
    loudest)."""
    ops = _ops()
    x = segments_533_input()     # audio_edge_inputs.wide: the clamp is at work and its floor is set by frame 24
    for u in range(48):
        clamp_conditions(oracle_pre(x[u], 533, 133)[0], 80.0, 24, dropped=True)
    d = torch.from_numpy(x).to(gpu)
    got = ops.spectrogram(d, n_fft=533, hop_length=133, pad_mode=pad_mode).cpu().numpy()
    sl = ops.spectrogram(d, n_fft=533, hop_length=133, pad_mode=pad_mode, frames_per_slice=24).cpu().numpy()
    assert got.shape == (48, 80, 25) and sl.shape == (48, 1, 80, 24)
    np.testing.assert_array_equal(sl[:, 0], got[:, :, :24])
    for u in range(48):
        ref, _ = R.signal_to_spectrogram(x[u], 16000, 533, 133, pad_mode=pad_mode)
        _check_db(got[u], ref)
        if pad_mode == "reflect":
            _check_db(sl[u], R.preprocess_audio_signal(x[u], 16000, 200, 1, 29.97))


def test_533_complex_stft_and_bench_batch(gpu):
    """k_spec533's complex STFT (every one of the 267 bins: the 13 x 21 prime-factor outputs map onto them once) against
    the oracle, on 3-s utterances (chunked); and 512 segments (the fps_time / bench batch) spread-checked."""
    ops = _ops()
    rng = np.random.default_rng(13)
    x = synth_audio(rng, 3, 48000)
    _, D = ops.spectrogram(torch.from_numpy(x).to(gpu), n_fft=533, hop_length=133, return_stft=True)
    D = D.cpu().numpy()
    for u in range(3):
        ref = R.stft(x[u], 533, 133).astype(np.complex128)
        assert D[u].shape == ref.shape == (267, 361)
        err = np.abs(D[u] - ref).max() / np.abs(ref).max()
        assert err < 2e-6, err
    xb = synth_audio(rng, 512, 3200)
    got = ops.spectrogram(torch.from_numpy(xb).to(gpu), n_fft=533, hop_length=133, frames_per_slice=24).cpu().numpy()
    for u in range(0, 512, 37):
        _check_db(got[u], R.preprocess_audio_signal(xb[u], 16000, 200, 1, 29.97))


def test_other_n_fft_direct_dft(gpu):
    """n_fft without a fast kernel (600, hop 150) runs the direct-DFT fallback."""
    ops = _ops()
    rng = np.random.default_rng(14)
    x = synth_audio(rng, 3, 6400)
    got = ops.spectrogram(torch.from_numpy(x).to(gpu), n_fft=600, hop_length=150).cpu().numpy()
    for u in range(3):
        ref, _ = R.signal_to_spectrogram(x[u], 16000, 600, 150)
        _check_db(got[u], ref)
