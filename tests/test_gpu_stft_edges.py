"""avse_spectrogram at the inputs and geometries where its kernels can go wrong unnoticed by tests/test_gpu_stft.py:
utterances on which the top_db clamp is at work (tests/audio_edge_inputs.py `wide`: > 100 dB of range, the maximum in
the frame that slicing drops, neighbouring utterances' floors 10 dB apart), every branch of launch_spectrogram, chunk
edges, odd lengths, other hops, a misaligned base pointer, and the slicing pinned to the reference's own frame_ids.

Bounds (DESIGN.md "Parity"): mel dB max 1e-3 / RMS 1e-4 against the float64 oracle (tests/test_gpu_stft.py's), the
complex STFT within 2e-6 of the utterance's peak |X| and, the inputs being `wide`, within 2e-6 of each frame's own peak
|X| (so a quiet frame cannot hide behind the loud one; a frame whose oracle STFT is exactly zero must be exactly zero).
The conditions that make each input tell the wrong clamp semantics apart are asserted on the oracle before the device
output is looked at (A.clamp_oracle; tests/test_audio_edge_inputs.py runs the same assertions without a GPU).
Measured figures: profiles/audio_edge_checks.txt.
"""
import numpy as np
import pytest
import torch

import audio_edge_inputs as A
from conftest import synth_audio
from oracle import librosa_ref as R
from test_gpu_stft import DB_MAX, _check_db

pytestmark = pytest.mark.gpu


def _ops():
    from avse_amd import ops
    return ops


def _spec(x, c, gpu, pad_mode="reflect", sliced=True, return_stft=False, n_fft=None, hop=None, spf=None, bank=None,
          top_db="case"):
    """ops.spectrogram for the case / geometry -> numpy (mel dB, complex STFT or None)."""
    bank = bank or c["bank"]
    d = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    out = _ops().spectrogram(d, n_fft=n_fft or c["n_fft"], hop_length=hop or c["hop"], pad_mode=pad_mode,
                             frames_per_slice=(c["spf"] if spf is None else spf) if sliced else 0,
                             top_db=c["top_db"] if top_db == "case" else top_db, return_stft=return_stft, **bank)
    if return_stft:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy(), None


def _expect(pre, top_db, spf):
    ref = A.clamp(pre, top_db)
    return A.slices(ref, spf) if spf else ref


def _check_stft(got, ref, what):
    peak, frame = A.stft_errors(got, ref)
    assert peak <= A.STFT_REL, f"{what}: STFT error {peak} of the utterance's peak |X|"
    assert frame <= A.STFT_REL, f"{what}: STFT error {frame} of a frame's own peak |X|"
    return peak, frame


def _compare(name, c, oracle, rows, mel, D, sliced, what):
    """Rows `rows` of the case (mel[i] is utterance rows[i]) against the oracle; records the worst figures."""
    worst = dict(db_max=0.0, db_rms=0.0)
    if D is not None:
        worst.update(stft_peak=0.0, stft_frame=0.0)
    for i, u in enumerate(rows):
        pre, Dref = oracle[u]
        ref = _expect(pre, c["top_db"], c["spf"] if sliced else 0)
        assert mel[i].shape == ref.shape, (mel[i].shape, ref.shape)
        mx, rms = A.db_errors(mel[i], ref)
        worst["db_max"], worst["db_rms"] = max(worst["db_max"], mx), max(worst["db_rms"], rms)
        if D is not None:
            pk, fr = A.stft_errors(D[i], Dref)
            worst["stft_peak"], worst["stft_frame"] = max(worst["stft_peak"], pk), max(worst["stft_frame"], fr)
    A.record(f"{name} {what}", **worst)
    for i, u in enumerate(rows):
        pre, Dref = oracle[u]
        _check_db(mel[i], _expect(pre, c["top_db"], c["spf"] if sliced else 0))
        if D is not None:
            _check_stft(D[i], Dref, f"{name} {what} utterance {u}")


# ---------------------------------------------------------------------------------------------------------------
# B. the clamp, one case per kernel and mechanism
# ---------------------------------------------------------------------------------------------------------------
def test_clamp_k_spec_seg(gpu):
    """k_spec_seg (the persistent segment kernel), unsliced and sliced to 20 frames: 1100 segments on a grid of
    2 x CUs = 512 blocks, so every block walks 2-3 utterances and both parity rows of its maxima are used; the maximum
    sits in frame 20, which the slice drops, and utterance u carries the ladder gain, so the floor of u differs from
    those of u +- 1 and u +- 512 by 10 dB.  128 utterances (whole block walks, A.seg_spread) against the oracle."""
    c = A.clamp_case("seg")
    oracle, _, _ = A.clamp_oracle("seg")
    d = torch.from_numpy(c["x"]).to(gpu)
    assert d.data_ptr() % 16 == 0
    full, _ = _spec(d, c, gpu, sliced=False)
    sl, _ = _spec(d, c, gpu, sliced=True)
    assert full.shape == (A.SEG_U, 80, 21) and sl.shape == (A.SEG_U, 1, 80, 20)
    np.testing.assert_array_equal(sl[:, 0], full[:, :, :20])
    _compare("seg", c, oracle, c["check"], full[c["check"]], None, False, "k_spec_seg unsliced")
    _compare("seg", c, oracle, c["check"], sl[c["check"]], None, True, "k_spec_seg sliced 20")


def test_clamp_k_spec640_single_chunk_with_stft(gpu):
    """k_spec640<true, true>, single chunk (in-kernel clamp): the 128 checked segments of the k_spec_seg case with
    return_stft (the RI path), sliced to 20 and unsliced; dB and complex STFT."""
    c = A.clamp_case("seg")
    oracle, _, _ = A.clamp_oracle("seg")
    rows = c["check"]
    for sliced in (True, False):
        mel, D = _spec(c["x"][rows], c, gpu, sliced=sliced, return_stft=True)
        _compare("seg", c, oracle, rows, mel, D, sliced, f"k_spec640<1,1> single sliced={int(sliced)}")


@pytest.mark.parametrize("name", ["seg17", "seg64"])
@pytest.mark.parametrize("return_stft", [False, True])
def test_clamp_k_spec640_wide_bank_single_chunk(gpu, name, return_stft):
    """k_spec640<false, false> and k_spec640<false, true>, single chunk: the 17- and 64-band banks of
    test_segment_kernel_other_banks (bands wider than the padded 24-bin rows: the generic band loop) on the segment
    input, levelled for the bank, sliced to 20; top_db 75 for the 17 bands."""
    c = A.clamp_case(name)
    oracle, _, _ = A.clamp_oracle(name)
    mel, D = _spec(c["x"], c, gpu, return_stft=return_stft)
    _compare(name, c, oracle, c["check"], mel, D, True, f"k_spec640<0,{int(return_stft)}> single")


@pytest.mark.parametrize("name,return_stft", [("chunk640", False), ("chunk640", True), ("chunk640_17", False),
                                              ("chunk640_17", True)])
def test_clamp_k_spec640_chunked(gpu, name, return_stft):
    """k_spec640 over 15 chunks of 21 frames + one of 6, every chunk's atomicMax, then k_spec_clamp: 4 utterances of
    48000 samples sliced to 20 with the maximum in the dropped frame 300 (the last chunk), mid-utterance, in chunk 0
    and nowhere (no burst).  chunk640 runs k_spec640<true, false> / <true, true>, chunk640_17 (the wide bank)
    k_spec640<false, false> / <false, true>."""
    c = A.clamp_case(name)
    oracle, _, _ = A.clamp_oracle(name)
    mel, D = _spec(c["x"], c, gpu, return_stft=return_stft)
    fast = int(name == "chunk640")
    _compare(name, c, oracle, c["check"], mel, D, True, f"k_spec640<{fast},{int(return_stft)}> multi + k_spec_clamp")


def test_clamp_k_spec533_single_block(gpu):
    """k_spec533, one block per utterance (in-kernel clamp): 64 segments of 3200 samples, sliced to 24, the maximum in
    the dropped frame 24, the ladder."""
    c = A.clamp_case("seg533")
    oracle, _, _ = A.clamp_oracle("seg533")
    for return_stft in (False, True):
        mel, D = _spec(c["x"], c, gpu, return_stft=return_stft)
        _compare("seg533", c, oracle, c["check"], mel, D, True, f"k_spec533 single ri={int(return_stft)}")


def test_clamp_k_spec533_chunked(gpu):
    """k_spec533 over 10 chunks of 25 frames (atomicMax per chunk) + k_spec_clamp: 3 utterances of 32000 samples sliced
    to 24, the maximum in the dropped frame 240, mid-utterance and in chunk 0."""
    c = A.clamp_case("chunk533")
    oracle, _, _ = A.clamp_oracle("chunk533")
    for return_stft in (False, True):
        mel, D = _spec(c["x"], c, gpu, return_stft=return_stft)
        _compare("chunk533", c, oracle, c["check"], mel, D, True, f"k_spec533 multi + k_spec_clamp ri={int(return_stft)}")


@pytest.mark.parametrize("name", ["dft666", "dft401"])
@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
def test_clamp_k_spec_dft(gpu, name, pad_mode):
    """k_spec_dft + k_spec_clamp: the reference's 24-fps geometry (n_fft 666, hop 166, 6400 samples sliced to 19: the
    maximum in the dropped frame 38) and 401 / 100 unsliced, 3 utterances with the ladder, both pad modes."""
    c = A.clamp_case(name)
    oracle, _, _ = A.clamp_oracle(name, pad_mode)
    for return_stft in (False, True):
        mel, D = _spec(c["x"], c, gpu, pad_mode=pad_mode, return_stft=return_stft)
        _compare(name, c, oracle, c["check"], mel, D, bool(c["spf"]),
                 f"k_spec_dft + k_spec_clamp {pad_mode} ri={int(return_stft)}")


# ---------------------------------------------------------------------------------------------------------------
# C. geometry sweep
# ---------------------------------------------------------------------------------------------------------------
def _kernel_of(n_fft, hop, L, bank, ri):
    T = R.n_frames(L, n_fft, hop)
    if n_fft == 640:
        return f"k_spec640<{int(bank['n_mels'] == 80)},{int(ri)}> {'single' if T <= 21 else 'multi'}"
    if n_fft == 533:
        return f"k_spec533 {'single' if T <= 25 else 'multi'}"
    return "k_spec_dft"


@pytest.mark.parametrize("row,n_fft,hop,L,spf,bank,pad_modes", A.SWEEP,
                         ids=[f"row{r[0]}-{r[1]}-{r[2]}-{r[3]}" for r in A.SWEEP])
def test_geometry_sweep(gpu, row, n_fft, hop, L, spf, bank, pad_modes):
    """Rows of the sweep (3 `wide` utterances with the ladder, dB and complex STFT against the oracle, with and without
    the complex output):
      1  640 / 160 chunk edges, T = 3 (a signal shorter than one window), 22 (a one-frame last chunk), 42 (an exact
         multiple of CHUNK = 21), 43: k_spec640<true, *> single and multi chunk, both pad modes
      2  640 / 160, 3361 samples (no multiple of the hop) and 3333 (odd: the bases of utterances 1, 3, .. are only
         4-byte aligned where load_frame reads float2)
      4  hops 100 and 320 at n_fft 640 (k_spec640, not the segment kernel)
      5  the 17-band bank with the complex output over 3 chunks: k_spec640<false, true> multi (dB composed from
         R.stft, R.magphase, R.mel_filterbank, R.amplitude_to_db)
      6  533 / 133 chunk edges, T = 3, 25 (one whole chunk of P533_CH = 25), 26 (a one-frame second chunk), 50, 51:
         k_spec533 single and multi, both pad modes
      7  533 / 100
      8  666 / 166 sliced to 19 (the 24-fps geometry) with the complex output: k_spec_dft + k_spec_clamp
      9  401 / 100, 400 / 100, 1024 / 256: k_spec_dft at odd and even sizes, both pad modes"""
    ops = _ops()
    x = A.sweep_input(n_fft, hop, L)
    d = torch.from_numpy(x).to(gpu)
    T = R.n_frames(L, n_fft, hop)
    assert ops.n_frames(L, hop, n_fft) == T
    c = dict(n_fft=n_fft, hop=hop, spf=spf, bank=bank, top_db=80.0)
    for pad_mode in pad_modes:
        oracle = {u: A.oracle_pre(x[u], n_fft, hop, pad_mode, bank) for u in range(3)}
        for ri in (True, False):
            mel, D = _spec(d, c, gpu, pad_mode=pad_mode, return_stft=ri)
            assert mel.shape == ((3, T // spf, bank["n_mels"], spf) if spf else (3, bank["n_mels"], T))
            _compare(f"row {row} {n_fft}/{hop} L {L}", c, oracle, range(3), mel, D, bool(spf),
                     f"{_kernel_of(n_fft, hop, L, bank, ri)} {pad_mode}")


@pytest.mark.parametrize("spf", [0, 20])
def test_misaligned_base_leaves_the_segment_kernel(gpu, spf):
    """Row 3: 3200-sample segments whose base pointer is offset by one float (4-byte aligned only).  k_spec_seg stages
    samples with 16-byte buffer loads, so launch_spectrogram must take k_spec640<true, false> (single chunk) instead;
    the result is compared with the oracle and with the aligned call (k_spec_seg).  The two kernels agree bit for bit
    (the same transform and summation order; k_spec_seg's extra leading band terms are x * 0 added to an exact 0)."""
    c = A.clamp_case("seg")
    oracle, _, _ = A.clamp_oracle("seg")
    rows = c["check"]
    x = c["x"][rows]
    buf = torch.empty(x.size + 4, dtype=torch.float32, device=gpu)
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + x.size].view(x.shape)
    off.copy_(torch.from_numpy(x))
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    mis, _ = _spec(off, c, gpu, sliced=bool(spf))
    ali, _ = _spec(x, c, gpu, sliced=bool(spf))
    _compare("seg", c, oracle, rows, mis, None, bool(spf), f"misaligned base spf={spf} (k_spec640<1,0> single)")
    A.record(f"seg misaligned vs aligned spf={spf}", max_abs_db=float(np.abs(mis.astype(np.float64) - ali).max()))
    np.testing.assert_array_equal(mis, ali)


# ---------------------------------------------------------------------------------------------------------------
# argument edges that launch no kernel
# ---------------------------------------------------------------------------------------------------------------
def test_argument_edges(gpu):
    from avse_amd import _lib
    ops = _ops()
    x = torch.from_numpy(synth_audio(np.random.default_rng(5), 1, 400)).to(gpu)
    with pytest.raises(_lib.AvseError):
        ops.spectrogram(x[:, :320].contiguous())                         # reflect needs n_samples > n_fft // 2
    got = ops.spectrogram(x[:, :321].contiguous()).cpu().numpy()
    _check_db(got[0], R.signal_to_spectrogram(x[0, :321].cpu().numpy(), 16000, 640, 160)[0])
    assert ops.spectrogram(x[:, :320].contiguous(), pad_mode="constant").shape == (1, 80, 3)
    with pytest.raises(_lib.AvseError):
        ops.spectrogram(torch.zeros(1, 4096, device=gpu), n_fft=2049, hop_length=512)
    # avse_istft: n_frames that is no multiple of frames_per_slice (ops.istft never passes one: the C ABI directly)
    mel = torch.zeros(1, 2, 80, 20, device=gpu)
    D = torch.zeros(1, 321, 41, 2, device=gpu)
    out = torch.zeros(1, 160 * 40, device=gpu)
    ctx = _lib.context(gpu)
    with torch.cuda.device(gpu):
        rc = _lib.load().avse_istft(ctx.handle, _lib.ptr(mel), _lib.ptr(D), 1, 30, 41, 20, 16000, 640, 160, 80, 0.0,
                                    8000.0, _lib.ptr(out), _lib.stream_handle(gpu))
    with pytest.raises(_lib.AvseError):
        _lib.check(rc, "avse_istft")
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                                 # nothing was launched


# ---------------------------------------------------------------------------------------------------------------
# D. slicing pinned to the reference fixture
# ---------------------------------------------------------------------------------------------------------------
def _check_columns(got, c, k, what):
    fx = c["fx"]
    assert got.shape == tuple(fx["out_shape"])
    full, unique = c["full"][k], c["unique"][k]
    ids = np.array(fx["frame_ids"])
    worst = 0.0
    for s in range(ids.shape[0]):
        ref = full[:, ids[s]]                                            # the oracle's unsliced columns frame_ids[s][:]
        worst = max(worst, float(np.abs(got[s].astype(np.float64) - ref).max()))
    assert worst <= DB_MAX, f"{what}: a device column is {worst} dB from the oracle column the fixture names"
    return worst, int(unique[ids.ravel()].sum())


@pytest.mark.parametrize("i", range(10))
def test_slicing_matches_reference_frame_ids(gpu, i):
    """preprocess_audio_signal / preprocess_audio_batch for the 10 cases of tests/golden/slicing.json (written by the
    reference's own code): the padded / truncated length, the output shape, and device column (s, j) equal to the
    oracle's unsliced column frame_ids[s][j], which the CPU module shows to be the only column within 1 dB of it
    (the all-silent padded tail of the 47000 / 31000 cases apart)."""
    from avse_amd import data_processor as dp
    from avse_amd.audio_io import AudioSignal
    c = A.slicing_case(i, 2)
    fx = c["fx"]
    sig = AudioSignal(c["x"][0].copy(), 16000)
    got = dp.preprocess_audio_signal(sig, 200, fx["n_video_slices"], fx["fps"])
    assert sig.get_number_of_samples() == fx["signal_length"]
    g = dp.frame_geometry(16000, 200, fx["n_video_slices"], fx["fps"])
    assert (g["n_fft"], g["hop_length"], g["n_frames"]) == (fx["n_fft"], fx["hop_length"], fx["n_frames"])
    worst, pinned = _check_columns(got, c, 0, "preprocess_audio_signal")
    batch = dp.preprocess_audio_batch(torch.from_numpy(c["x"]).to(gpu), 16000, 200, fx["n_video_slices"], fx["fps"])
    batch = batch.cpu().numpy()
    for k in range(2):
        worst = max(worst, _check_columns(batch[k], c, k, f"preprocess_audio_batch[{k}]")[0])
    A.record(f"slicing case {i} ({fx['n_samples_in']} samples, {fx['fps']} fps)", db_max=worst, pinned_columns=pinned,
             columns=int(np.prod(np.array(fx["frame_ids"]).shape)))
