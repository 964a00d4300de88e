"""avse_istft on the branches and edges tests/test_gpu_istft.py does not reach: the direct inverse k_istft_dft (the
reference's 24-fps geometry among its sizes), k_istft640 + k_ola away from the fused kernel (another bank, other
hops), the chunk edges of k_istft_fused (OF = 30 hops) and k_istft532 (16 frames), and the rule "phase is 1 where
D == 0" in each of the four inverse kernels.

Predictions are the mixture's own oracle mel dB plus N(0, 1 dB) noise (tests/audio_edge_inputs.py, `wide` mixtures);
the phase comes from the device's own STFT of the mixture.  Bounds (DESIGN.md "Parity"): the waveform within relative
RMS 1e-4 of the float64 oracle over the utterance, and per block of `hop` samples an error RMS of at most
1e-4 x max(the oracle's RMS in that block, the oracle's RMS over the utterance), so an error confined to a few samples
at one chunk seam cannot hide in the whole-waveform figure.  Output lengths are exact.
Measured figures: profiles/audio_edge_checks.txt.
"""
import numpy as np
import pytest
import torch

import audio_edge_inputs as A
from oracle import librosa_ref as R

pytestmark = pytest.mark.gpu


def _device_stft(x, gpu, n_fft, hop, bank=A.DEFAULT_BANK):
    from avse_amd import ops
    _, D = ops.spectrogram(torch.from_numpy(x).to(gpu), n_fft=n_fft, hop_length=hop, return_stft=True, **bank)
    return D


def _check_waves(what, got, refs, hop):
    worst_u, worst_b = 0.0, 0.0
    for g, r in zip(got, refs):
        assert g.shape == r.shape, (g.shape, r.shape)
        assert np.isfinite(g).all()
        whole, block = A.wave_errors(g, r, hop)
        worst_u, worst_b = max(worst_u, whole), max(worst_b, block)
    A.record(what, wave_rel_rms=worst_u, wave_block=worst_b)
    assert worst_u <= A.WAVE_REL, f"{what}: waveform relative RMS {worst_u}"
    assert worst_b <= A.WAVE_REL, f"{what}: worst block of {hop} samples {worst_b}"


def _run_case(gpu, name, T=None, spf=0, what=""):
    """ops.istft on the first T frames of istft_case(name) (all of them by default), the prediction unsliced or as
    slices of spf frames, against A.oracle_reconstruct per utterance."""
    from avse_amd import ops
    c = A.istft_case(name)
    n_fft, hop, bank = c["n_fft"], c["hop"], c["bank"]
    T = T or c["pred"].shape[2]
    pred = c["pred"][:, :, :T]
    mel = np.stack([A.slices(p, spf) for p in pred]) if spf else pred
    D = _device_stft(c["x"], gpu, n_fft, hop, bank)
    assert D.shape[2] == c["D"][0].shape[1] >= T
    y = ops.istft(torch.from_numpy(np.ascontiguousarray(mel)).to(gpu), D, n_fft=n_fft, hop_length=hop, **bank)
    y = y.cpu().numpy()
    assert y.shape == (3, hop * (T - 1))
    refs = [A.oracle_reconstruct(pred[u], c["D"][u], n_fft, hop, bank) for u in range(3)]
    _check_waves(f"{name} T {T} spf {spf} {what}", y, refs, hop)


def test_direct_inverse_at_24_fps(gpu):
    """k_istft_dft (and the sliced k_spec_dft for the phase) through data_processor.reconstruct_speech_signal at the
    reference's 24-fps geometry: n_fft 666, hop 166, 2 slices of 19 frames of a 6400-sample mixture -> 6142 samples."""
    from avse_amd import data_processor as dp
    from avse_amd.audio_io import AudioSignal
    c = A.istft_case("dft666")
    got, refs = [], []
    for u in range(3):
        pred = A.slices(c["pred"][u], 19)
        assert pred.shape == (2, 80, 19)
        got.append(dp.reconstruct_speech_signal(AudioSignal(c["x"][u].copy(), 16000), pred, 24.0).get_data(0))
        refs.append(R.reconstruct_speech_signal(c["x"][u], 16000, pred, 24.0))
        assert got[-1].shape == (6142,)
    _check_waves("dft666 reconstruct_speech_signal 24 fps k_istft_dft + k_ola", got, refs, 166)


@pytest.mark.parametrize("name", ["dft401", "dft1024"])
def test_direct_inverse_other_sizes(gpu, name):
    """k_istft_dft + k_ola through ops.istft, unsliced: analysis n_fft 401 (201 bins: the inverse size is 400) and
    1024 / 256."""
    _run_case(gpu, name, what="k_istft_dft + k_ola")


@pytest.mark.parametrize("name", ["ola64", "ola_hop320", "ola_hop100"])
def test_unfused_640_other_bank_and_hops(gpu, name):
    """k_istft640 + k_ola where launch_istft cannot take the fused kernel: 64 bands up to 7600 Hz at hop 160, and the
    80 bands at hops 320 and 100."""
    _run_case(gpu, name, what="k_istft640 + k_ola")


@pytest.mark.parametrize("T", A.FUSED_T)
def test_fused_chunk_edges_unsliced(gpu, T):
    """k_istft_fused at T - 1 = 1, 29, 30, 31, 60, 61 output hops (chunks of OF = 30): a single hop, one hop short of
    a chunk, exactly one and two chunks, and a last chunk of one hop; the STFT holds 63 frames."""
    _run_case(gpu, "fused", T=T, what="k_istft_fused")


@pytest.mark.parametrize("name", ["fused61", "fused65"])
def test_fused_sliced_with_longer_stft(gpu, name):
    """k_istft_fused on T = 60 frames given as 3 slices of 20, the mixture STFT holding T + 1 and T + 5 frames."""
    _run_case(gpu, name, T=60, spf=20, what="k_istft_fused")


@pytest.mark.parametrize("T", A.I532_T)
def test_532_chunk_edges(gpu, T):
    """k_istft532 + k_ola at T = 2, 16 (one whole chunk of I532_CH = 16 frames), 17 (a one-frame second chunk), 33."""
    _run_case(gpu, "i532", T=T, what="k_istft532 + k_ola")


@pytest.mark.parametrize("name", sorted(A.ZERO_GEOMETRIES))
def test_zero_stft_frames_take_phase_one(gpu, name):
    """librosa.magphase gives a phase of 1 where D == 0.  A `wide` mixture whose silent stretch spans several whole
    windows has exactly zero STFT frames; the prediction puts energy within 6 dB of the utterance's maximum there, so
    those frames carry most of the waveform (conditions on the oracle: A.zero_frame_case).  fused: k_istft_fused;
    dense: k_istft640 + k_ola (the dense_istft option); i532: k_istft532; dft666: k_istft_dft."""
    from avse_amd import _lib, ops
    c = A.zero_frame_case(name)
    n_fft, hop, spf = c["n_fft"], c["hop"], c["spf"]
    D = _device_stft(c["x"], gpu, n_fft, hop)
    T = c["pred"].shape[2]
    Dn = D.cpu().numpy()
    for u in range(2):   # the device STFT is exactly zero in the frames where the oracle's is (and only there)
        np.testing.assert_array_equal(np.all(Dn[u][:, :T] == 0, axis=0), np.all(c["D"][u][:, :T] == 0, axis=0))
    mel = torch.from_numpy(np.stack([A.slices(p, spf) for p in c["pred"]])).to(gpu)
    with _lib.context(gpu).options(dense_istft=int(name == "dense")):
        y = ops.istft(mel, D, n_fft=n_fft, hop_length=hop)
        torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert y.shape == (2, hop * (T - 1))
    _check_waves(f"zero frames {name} {n_fft}/{hop}", y, c["ref"], hop)
