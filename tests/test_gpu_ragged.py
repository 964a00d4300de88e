"""Ragged STFT / ISTFT (avse_spectrogram_ragged / avse_istft_ragged and everything built on them): every utterance of
a mixed-length batch must equal, bit for bit, the equal-length call on that utterance alone, and independently match
the librosa oracle under the gates of test_gpu_stft.py / test_gpu_istft.py.

Shapes sit around the kernels' chunk sizes: 21 frames (n_fft 640), 25 (n_fft 533), 30 output hops (fused ISTFT).

Frame counts at n_fft 533: librosa's centred count is 1 + (L - 1) // hop for an odd n_fft, so the lengths 3192 and 3325
give T = 24 and 25 (one chunk of 25 each); 3193 and 3326 are added to them to reach T = 25 and 26, the pair "one
chunk / one frame into a second chunk"."""
import functools
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from audio_edge_inputs import (DB_MAX, DB_RMS, STFT_REL, clamp, clamp_conditions, db_errors, oracle_pre,
                               oracle_reconstruct, slices, wide)
from conftest import synth_audio, synth_video

pytestmark = pytest.mark.gpu

LENS640 = [3200, 400, 3360, 6721, 4799, 16000, 3200]      # T = 21, 3, 22, 43, 30, 101, 21
EDGE, LOUD, QUIET = 4, 5, 6        # `wide` with the burst in frames the slicing drops; a loud / quiet neighbour pair
LENS533 = [3192, 3325, 8000, 1000, 3193, 3326]            # T = 24, 25, 61, 8, 25, 26
GEO = {640: dict(n_fft=640, hop_length=160), 533: dict(n_fft=533, hop_length=133), 600: dict(n_fft=600, hop_length=150)}


@functools.lru_cache(maxsize=None)
def signals(n_fft):
    rng = np.random.default_rng(9000 + n_fft)
    if n_fft == 600:
        return [synth_audio(rng, 1, L)[0] for L in (3000, 3000, 4200, 3000)]
    lens = LENS640 if n_fft == 640 else LENS533
    x = [synth_audio(rng, 1, L)[0] for L in lens]
    if n_fft == 640:
        x[EDGE] = wide(x[EDGE], (LENS640[EDGE] - 100, LENS640[EDGE]))
        x[QUIET] = (x[QUIET] * 3e-4).astype(np.float32)   # 70 dB under its loud neighbour
    else:
        x[2] = wide(x[2], (7900, 8000))                   # T = 61, 2 slices of 24: frames 48 .. 60 are dropped
    return x


@functools.lru_cache(maxsize=None)
def oracle(n_fft, pad_mode):
    """Per utterance (dB before the clamp, complex STFT) from the float64 oracle; computed once per module."""
    g = GEO[n_fft]
    return [oracle_pre(x, g["n_fft"], g["hop_length"], pad_mode) for x in signals(n_fft)]


_solo = {}


def solo(ops, gpu, n_fft, pad_mode, spf, stft):
    """The equal-length ops.spectrogram on every utterance alone (the reference of the bitwise checks), once per case."""
    key = (n_fft, pad_mode, spf, stft)
    if key not in _solo:
        out = []
        for x in signals(n_fft):
            if spf and ops.n_frames(len(x), GEO[n_fft]["hop_length"], n_fft) < spf:
                # zero slices: the equal-length call has no mel buffer to pass; the STFT does not depend on the slicing
                out.append((np.zeros((0, 80, spf), np.float32), solo(ops, gpu, n_fft, pad_mode, 0, stft)[len(out)][1]))
                continue
            r = ops.spectrogram(torch.from_numpy(x[None]).to(gpu), pad_mode=pad_mode, frames_per_slice=spf,
                                return_stft=stft, **GEO[n_fft])
            out.append((r[0][0].cpu().numpy(), r[1][0].cpu().numpy()) if stft else (r[0].cpu().numpy(), None))
        _solo[key] = out
    return _solo[key]


def ragged(ops, gpu, xs, packing, **kw):
    """-> (counts, views, stft views or None), the views as numpy, from one spectrogram_ragged call on the list (tight packing: odd
    offsets) or on the rows of a zero-initialised [U][max L] buffer."""
    if packing == "tight":
        arg = [torch.from_numpy(x).to(gpu) for x in xs]
    else:
        stride = max(len(x) for x in xs)
        buf = torch.zeros((len(xs), stride), dtype=torch.float32, device=gpu)
        for u, x in enumerate(xs):
            buf[u, :len(x)] = torch.from_numpy(x).to(gpu)
        arg = (buf, np.arange(len(xs)) * stride, [len(x) for x in xs])
    r = ops.spectrogram_ragged(arg, **kw)
    views = [v.cpu().numpy() for v in r[2]]
    return r[1], views, ([v.cpu().numpy() for v in r[4]] if len(r) == 5 else None)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_bitwise(ops, gpu, n_fft, pad_mode, spf, stft):
    xs = signals(n_fft)
    want = solo(ops, gpu, n_fft, pad_mode, spf, stft)
    kw = dict(pad_mode=pad_mode, frames_per_slice=spf, return_stft=stft, **GEO[n_fft])
    got = {p: ragged(ops, gpu, xs, p, **kw) for p in ("tight", "rows")}
    for p, (counts, views, sviews) in got.items():
        for u in range(len(xs)):
            assert same_bits(views[u], want[u][0]), (p, u, "mel")
            assert int(counts[u]) == (want[u][0].shape[0] if spf else want[u][0].shape[1]), (p, u)
            if stft:
                assert same_bits(sviews[u], want[u][1]), (p, u, "stft")
    for u in range(len(xs)):
        assert same_bits(got["tight"][1][u], got["rows"][1][u]), u
        if stft:
            assert same_bits(got["tight"][2][u], got["rows"][2][u]), u
    return got["tight"]


@pytest.mark.parametrize("stft", [False, True])
@pytest.mark.parametrize("spf", [0, 20])
@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
def test_stft_640_equals_each_utterance_alone(gpu, pad_mode, spf, stft):
    from avse_amd import ops
    counts, views, _ = check_bitwise(ops, gpu, 640, pad_mode, spf, stft)
    if spf:
        assert [int(c) for c in counts] == [1, 0, 1, 2, 1, 5, 1]
        assert views[1].shape == (0, 80, 20)               # T = 3: zero slices, no mel
    else:
        assert [int(c) for c in counts] == [21, 3, 22, 43, 30, 101, 21]


@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
def test_stft_640_matches_the_oracle(gpu, pad_mode):
    from avse_amd import ops
    ref = oracle(640, pad_mode)
    # the edge utterance: its maximum lies in a frame the slicing drops and the clamp reaches the kept frames, so a
    # floor taken over the kept frames only, or no clamp, would show (asserted on the oracle before the device runs)
    fig = clamp_conditions(ref[EDGE][0], 80.0, 20, dropped=True)
    # the quiet neighbour: a floor leaking from the loud utterance before it would clamp a tenth of it or more
    leak = float(np.mean(ref[QUIET][0] < ref[LOUD][0].max() - 80.0))
    assert leak > 0.10 and float(np.mean(ref[QUIET][0] < ref[QUIET][0].max() - 80.0)) < leak / 2, leak
    xs = signals(640)
    kw = dict(pad_mode=pad_mode, **GEO[640])
    _, flat, sflat = ragged(ops, gpu, xs, "tight", return_stft=True, **kw)
    _, sl, _ = ragged(ops, gpu, xs, "tight", frames_per_slice=20, **kw)
    for u in range(len(xs)):
        full = clamp(ref[u][0])
        mx, rms = db_errors(flat[u], full)
        print(f"ragged stft 640 {pad_mode} u{u}: dB max {mx:.2e} rms {rms:.2e}")
        assert mx <= DB_MAX and rms <= DB_RMS, (u, mx, rms)
        if sl[u].shape[0]:
            mx, rms = db_errors(sl[u], slices(full, 20))
            assert mx <= DB_MAX and rms <= DB_RMS, (u, "sliced", mx, rms)
        err = float(np.abs(sflat[u].astype(np.complex128) - ref[u][1]).max() / np.abs(ref[u][1]).max())
        print(f"ragged stft 640 {pad_mode} u{u}: stft {err:.2e} of the peak")
        assert err < STFT_REL, (u, err)
    print(f"edge utterance: clamped share {fig['share']:.2f}, kept-frames-only floor off by {fig['vs_kept']:.1f} dB")


def test_stft_neighbours_do_not_share_a_floor(gpu):
    """A loud utterance on both sides of a quiet one: the quiet one's output is that of its solo run."""
    from avse_amd import ops
    xs = signals(640)
    trio = [xs[LOUD], xs[QUIET], xs[3]]
    for spf in (0, 20):
        _, views, sviews = ragged(ops, gpu, trio, "tight", frames_per_slice=spf, return_stft=True, **GEO[640])
        _, alone, salone = ragged(ops, gpu, [xs[QUIET]], "tight", frames_per_slice=spf, return_stft=True, **GEO[640])
        assert same_bits(views[1], alone[0]) and same_bits(sviews[1], salone[0])
        assert same_bits(views[1], solo(ops, gpu, 640, "reflect", spf, True)[QUIET][0])


@pytest.mark.parametrize("spf", [0, 24])
@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
def test_stft_533_equals_each_utterance_alone_and_the_oracle(gpu, pad_mode, spf):
    from avse_amd import ops
    counts, views, sviews = check_bitwise(ops, gpu, 533, pad_mode, spf, True)
    check_bitwise(ops, gpu, 533, pad_mode, spf, False)
    T = [24, 25, 61, 8, 25, 26]
    assert [int(c) for c in counts] == ([t // 24 for t in T] if spf else T)
    ref = oracle(533, pad_mode)
    if spf:
        clamp_conditions(ref[2][0], 80.0, 24, dropped=True)
    for u in range(len(T)):
        full = clamp(ref[u][0])
        if spf == 0 or views[u].shape[0]:
            mx, rms = db_errors(views[u], slices(full, 24) if spf else full)
            assert mx <= DB_MAX and rms <= DB_RMS, (u, mx, rms)
        err = float(np.abs(sviews[u].astype(np.complex128) - ref[u][1]).max() / np.abs(ref[u][1]).max())
        assert err < STFT_REL, (u, err)


def test_stft_other_n_fft_walks_equal_length_runs(gpu):
    """n_fft 600 (the direct DFT): runs [3000, 3000], [4200], [3000] through the equal-length kernels."""
    from avse_amd import ops
    for spf in (0, 5):
        check_bitwise(ops, gpu, 600, "reflect", spf, True)


def test_stft_equal_lengths_are_the_equal_length_launch(gpu):
    from avse_amd import ops
    x = synth_audio(np.random.default_rng(77), 7, 3200)
    xt = torch.from_numpy(x).to(gpu)
    for spf, stft in ((20, False), (0, False), (20, True)):
        want = ops.spectrogram(xt, frames_per_slice=spf, return_stft=stft)
        got = ops.spectrogram_ragged(list(xt), frames_per_slice=spf, return_stft=stft)
        wm = (want[0] if stft else want).cpu().numpy()
        assert same_bits(got[0].cpu().numpy().reshape(wm.shape), wm), (spf, stft)
        if stft:
            assert same_bits(got[3].cpu().numpy().reshape(want[1].shape), want[1].cpu().numpy())


# ---- ISTFT -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def istft_inputs(n_fft):
    """Per utterance (pred [80, n_frames] float32: the mixture's own oracle dB + N(0, 1 dB), as the existing ISTFT
    tests build theirs; the oracle STFT of a synth_audio mixture with n_frames + 1 frames)."""
    hop = GEO[n_fft]["hop_length"]
    frames = [20, 31, 32, 40, 100, 1] if n_fft == 640 else [24, 48, 24]
    rng = np.random.default_rng(8000 + n_fft)
    out = []
    for nf in frames:
        x = synth_audio(rng, 1, hop * nf + (n_fft & 1))[0]
        pre, D = oracle_pre(x, n_fft, hop, "constant")
        assert D.shape[1] == nf + 1
        pred = (clamp(pre) + rng.normal(0, 1.0, pre.shape)).astype(np.float32)[:, :nf]
        out.append((np.ascontiguousarray(pred), D.astype(np.complex64)))
    return frames, out


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def check_istft(ops, gpu, n_fft, pick, spf):
    frames, data = istft_inputs(n_fft)
    hop = GEO[n_fft]["hop_length"]
    preds = [torch.from_numpy(data[u][0]).to(gpu) for u in pick]
    Ds = [torch.from_numpy(data[u][1]).to(gpu) for u in pick]
    if spf:      # [80][T] -> [T / spf][80][spf], the forward's output layout
        mel = torch.cat([p.view(80, -1, spf).permute(1, 0, 2) for p in preds]).contiguous()
        counts = [frames[u] // spf for u in pick]
    else:
        mel = torch.cat([p.reshape(-1) for p in preds])
        counts = [frames[u] for u in pick]
    ys = ops.istft_ragged(mel, counts, torch.cat([d.reshape(-1) for d in Ds]), [frames[u] + 1 for u in pick],
                          **GEO[n_fft])
    assert len(ys) == len(pick)
    for k, u in enumerate(pick):
        m1 = preds[k].view(80, -1, spf).permute(1, 0, 2)[None].contiguous() if spf else preds[k][None]
        # (one frame gives no samples: the equal-length call has no output buffer to pass)
        want = ops.istft(m1, Ds[k][None], **GEO[n_fft])[0].cpu().numpy() if frames[u] >= 2 else np.zeros(0, np.float32)
        got = ys[k].cpu().numpy()
        assert got.shape == (hop * (frames[u] - 1),)
        assert same_bits(got, want), (u, spf)
        if frames[u] >= 2:
            r = rel_rms(got, oracle_reconstruct(data[u][0], data[u][1], n_fft, hop))
            print(f"ragged istft {n_fft} T {frames[u]} spf {spf}: rel rms {r:.2e}")
            assert r < 1e-4, (u, r)


def test_istft_640_equals_each_utterance_alone_and_the_oracle(gpu):
    from avse_amd import ops
    check_istft(ops, gpu, 640, [0, 3, 4], 20)                 # n_frames 20, 40, 100: the sliced layout
    check_istft(ops, gpu, 640, [0, 1, 2, 3, 4, 5], 0)         # all six, [80][T]; n_frames == 1 contributes no samples
    check_istft(ops, gpu, 640, [5, 1, 5], 0)                  # an empty first and last utterance


def test_istft_533_walks_equal_length_runs(gpu):
    from avse_amd import ops
    check_istft(ops, gpu, 533, [0, 1, 2], 24)
    check_istft(ops, gpu, 533, [0, 2, 1], 0)                  # a run of two


# ---- pipeline, preprocess, predictor ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float32_split"])
def test_enhance_ragged_equals_each_utterance_alone(gpu, dtype):
    from avse_amd import ops, pipeline
    from avse_amd.model import KerasModel
    rng = np.random.default_rng(31)
    S = [1, 2, 5, 2]
    lens = [3200, 6000, 16500, 6400]                          # exact, padded, truncated, exact
    sigs = [torch.from_numpy(synth_audio(rng, 1, L)[0]).to(gpu) for L in lens]
    vids = [torch.from_numpy(synth_video(rng, s)).to(gpu) for s in S]
    dw = ops.DeviceWeights(KerasModel.init(seed=3, randomize=True), dtype)
    enh = pipeline.Enhancer(dw, chunk=4)                      # 10 clips in chunks of 4: a chunk spans utterances
    got = enh.enhance_ragged(sigs, vids)
    assert len(got) == 4
    for u in range(4):
        want = enh(sigs[u][None], vids[u][None])[0].cpu().numpy()
        assert want.shape == (160 * (20 * S[u] - 1),)
        assert same_bits(got[u].cpu().numpy(), want), u


def _audio(x, sr=16000):
    from avse_amd.audio_io import AudioSignal
    return AudioSignal(np.asarray(x, np.int16), sr)


def test_preprocess_audio_pairs_ragged_equals_the_grouped_path(gpu):
    from avse_amd import data_processor as dp
    rng = np.random.default_rng(32)
    n_slices = [1, 3, 2]
    speech = [rng.normal(0, 3000, n).astype(np.int16) for n in (3000, 10000, 6400)]      # padded, truncated, exact
    noise = [rng.normal(0, 2000, n).astype(np.int16) for n in (900, 20000, 5000)]
    args = ([_audio(s) for s in speech], [_audio(n) for n in noise], 200, n_slices, 25.0)
    want = dp.preprocess_audio_pairs(*args, snr_db=[0, 5, -5])
    got = dp.preprocess_audio_pairs(*args, snr_db=[0, 5, -5], ragged=True)
    assert len(got) == len(want) == 3
    for k in range(3):
        for j in range(3):
            assert got[k][j].shape == (n_slices[k], 80, 20) and same_bits(got[k][j], want[k][j]), (k, j)
        a, b = got[k][3], want[k][3]
        assert a.get_sample_rate() == b.get_sample_rate() and same_bits(a.get_data(), b.get_data()), k


def test_ragged_batch_predictor_equals_predict_one(gpu, tmp_path):
    """Samples of three lengths, written and preprocessed as the CLI test's dataset: one batch, whatever the length."""
    from scipy.io import wavfile
    from avse_amd import speech_enhancer as se
    from avse_amd.network import SpeechEnhancementNetwork
    rng = np.random.default_rng(33)
    Entry = namedtuple("Entry", ["speaker_id", "video_path", "audio_path"])
    samples = []
    for k, (n_frames, n_samples) in enumerate(((10, 6400), (25, 16000), (15, 9000))):
        t = np.arange(n_samples) / 16000
        speech = 3000 * np.sin(2 * np.pi * rng.uniform(150, 300) * t) * (1 + np.sin(2 * np.pi * 3 * t))
        a, v, n = (os.path.join(str(tmp_path), "%s%d.%s" % (w, k, e)) for w, e in (("a", "wav"), ("v", "npy"), ("n", "wav")))
        wavfile.write(a, 16000, speech.astype(np.int16))
        np.save(v, rng.integers(0, 256, (n_frames, 128, 128), dtype=np.uint8))
        wavfile.write(n, 16000, rng.normal(0, 2000, 5000 + 997 * k).astype(np.int16))
        samples.append(se.preprocess_sample(Entry("s", v, a), n))
    assert [s.mixed_spectrograms.shape[0] for s in samples] == [2, 5, 3]
    net = SpeechEnhancementNetwork.build((80, 20), (128, 128, 5), seed=5)
    pred = se.RaggedBatchPredictor(net)
    assert pred.groups(samples) == [[0, 1, 2]] and len(se.sample_groups(samples)) == 3
    got = pred(samples)
    for smp, (loss, sig) in zip(samples, got):
        want_loss, want_sig = se.predict_one(net, None, smp)
        assert loss == want_loss
        assert same_bits(sig.get_data(), want_sig.get_data())
