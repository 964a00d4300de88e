"""Input conditions of the audio edge tests (tests/test_gpu_stft_edges.py, tests/test_gpu_istft_edges.py), on the CPU.

A parity test only guards what its input can tell apart.  These tests take every input the device tests use
(tests/audio_edge_inputs.py builds them from fixed seeds) and assert, on the float64 oracle alone, that
  * the top_db clamp is at work: 10-70 % of each utterance's elements sit at the floor, the long utterances hold
    elements at exactly -100 dB before the clamp, and the oracle is more than 10 dB away from "no clamp";
  * where slicing drops trailing frames, the oracle is more than 1 dB away from "maximum over the kept frames only";
  * where a kernel walks several utterances, neighbouring utterances' floors are at least 5 dB apart, so that a
    maximum read from the wrong utterance (k_spec_seg's parity rows, a chunk's atomicMax slot) shows;
  * a zero STFT frame carries a large share of the ISTFT oracle's waveform, and a phase of 0 instead of 1 there
    moves it by more than 0.2 relative RMS;
  * every column of the slicing fixture's signals is the only one within 1 dB of itself, so a device column can
    only match the oracle column the fixture's frame_ids name.
So each clamp test fails against the two wrong semantics (no clamp; maximum over the kept frames) by construction.
"""
import numpy as np
import pytest

import audio_edge_inputs as A
from oracle import librosa_ref as R

CLAMP_PARAMS = [(n, pm) for n in A.CLAMP_CASES for pm in A.CLAMP_PAD_MODES.get(n, ("reflect",))]


@pytest.mark.parametrize("name,pad_mode", CLAMP_PARAMS)
def test_clamp_case_conditions(name, pad_mode):
    c = A.clamp_case(name)
    assert c["x"].dtype == np.float32 and np.isfinite(c["x"]).all()
    out, figures, apart = A.clamp_oracle(name, pad_mode)          # asserts the conditions
    assert set(out) == set(c["check"])
    # the two wrong semantics fail the device tests' own bound on the utterances meant to catch them
    for u, f in zip(c["check"], figures):
        assert 0.10 <= f["share"] <= 0.70
        if c["dropped"][u]:
            assert f["vs_kept"] > 1.0 > A.DB_MAX
        if c["silent"][u]:
            assert f["silent"] > 0
    assert max(f["vs_none"] for f in figures) > 10.0 and apart >= 5.0


def test_seg_spread_covers_the_block_walk():
    """The 128 checked utterances of the 1100-segment case: whole walks of three- and two-utterance blocks, the first
    and last block of each kind, and u, u + 512 pairs on both parity rows."""
    us, pairs = A.seg_spread()
    assert len(us) == len(set(us)) == 128 and max(us) < A.SEG_U
    n3 = A.SEG_U - 2 * A.SEG_GRID                                  # blocks 0 .. n3 - 1 walk three utterances
    for b in (0, n3 - 1, n3, A.SEG_GRID - 1):
        walk = list(range(b, A.SEG_U, A.SEG_GRID))
        assert len(walk) == (3 if b < n3 else 2) and set(walk) <= set(us)
    assert sum(v == u + A.SEG_GRID for u, v in pairs) >= 70
    assert {(u // A.SEG_GRID) & 1 for u in us} == {0, 1}


@pytest.mark.parametrize("which", ["sliced_segments", "segments_533"])
def test_rewritten_dropped_frame_inputs(which):
    """The inputs of test_sliced_segments_drop_last_frame_but_keep_its_max and test_533_segments_match_oracle."""
    x, n_fft, hop, spf = ((A.sliced_segments_input(), 640, 160, 20) if which == "sliced_segments"
                          else (A.segments_533_input(), 533, 133, 24))
    deepest = 0.0
    for xu in x:
        f = A.clamp_conditions(A.oracle_pre(xu, n_fft, hop)[0], 80.0, spf, dropped=True)
        deepest = max(deepest, f["vs_none"])
    assert deepest > 10.0


@pytest.mark.parametrize("row,n_fft,hop,L,spf,bank,pad_modes", A.SWEEP)
def test_sweep_geometry_runs_in_the_oracle(row, n_fft, hop, L, spf, bank, pad_modes):
    x = A.sweep_input(n_fft, hop, L)
    T = R.n_frames(L, n_fft, hop)
    assert T == A.SWEEP_FRAMES.get((n_fft, hop, L), T)
    for pm in pad_modes:
        pre, D = A.oracle_pre(x[0], n_fft, hop, pm, bank)
        assert pre.shape == (bank["n_mels"], T) and D.shape == (1 + n_fft // 2, T)
        assert np.isfinite(pre).all()
        if L >= 2000:      # long enough for the envelope's quiet quarter: the clamp is at work in the sweep too
            assert np.abs(A.clamp(pre) - pre).max() > 10.0


@pytest.mark.parametrize("name", sorted(A.ZERO_GEOMETRIES))
def test_zero_frame_conditions(name):
    c = A.zero_frame_case(name)                                    # asserts the conditions
    for n_zero, inside, moved in c["figures"]:
        assert n_zero >= 3 and inside >= 0.3 and moved > 0.2


@pytest.mark.parametrize("name", sorted(A.ISTFT_GEOMETRIES))
def test_istft_inputs_have_the_stated_frames(name):
    c = A.istft_case(name)
    n_fft, hop, L, bank = A.ISTFT_GEOMETRIES[name]
    T = R.n_frames(L, n_fft, hop)
    assert c["pred"].shape == (3, bank["n_mels"], T) and c["pred"].dtype == np.float32
    if name == "fused":
        assert T > max(A.FUSED_T)
    if name == "i532":
        assert T > max(A.I532_T)
    assert {"fused61": 61, "fused65": 65}.get(name, T) == T


@pytest.mark.parametrize("i", range(10))
def test_slicing_fixture_columns_are_unique(i):
    """Every oracle column is the only one within 1 dB (maximum over bands) of itself, except the all-silent columns of
    the zero-padded 47000- and 31000-sample cases: matching a device column to column frame_ids[s][j] pins the frame."""
    c = A.slicing_case(i, 2)
    fx = c["fx"]
    ids = np.array(fx["frame_ids"])
    assert ids.shape == (fx["out_shape"][0], fx["out_shape"][2]) and ids.max() < fx["n_frames"]
    padded = fx["n_samples_in"] < fx["signal_length"] - fx["n_fft"]
    for db, unique in zip(c["full"], c["unique"]):
        silent = np.all(db == db.min(), axis=0) if padded else np.zeros(db.shape[1], bool)
        assert unique[~silent].all(), np.nonzero(~unique & ~silent)[0]
        assert padded == bool(silent.any())
