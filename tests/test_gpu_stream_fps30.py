"""Streaming with 30-fps video ("30-fps video"): n_fft 800 / hop 200 at 24 kHz and, as two interleaved
800-point frames, n_fft 1600 / hop 400 at 48 kHz (csrc/frame800.h; the base-800 instances of k_stream_spec /
k_stream_synth / k_stream_ola / k_stream_reset) with the [80, 24] x 6-frame network, against the float64 oracle pipeline
at that rate, against the offline device path (a direct DFT at these n_fft), against themselves under every cut of the
input, stream by stream, and beside a 25-fps session.

Shapes: B <= 3 streams of S = 4 slices of 24 frames (L = 4 x 4800 or 4 x 9600 samples), the smallest at which every
session transition occurs (frame 0's reflection, a partial slice carried, several slices completed by one push, video
ahead and behind, the flush's padding).  The gates are the project's own: DB_MAX / DB_RMS (test_gpu_stft) for the mel-dB
the network sees, relative RMS 1e-4 for the waveform in float32 and float32_split, WAVE_BF16 / MEL_BF16
(test_gpu_pipeline) for bfloat16."""
import functools

import numpy as np
import pytest
import torch

from conftest import synth_audio, synth_video
from oracle import keras_ref as K
from oracle import librosa_ref as R
from test_gpu_pipeline import MEL_BF16, WAVE_BF16, rel_rms
from test_gpu_stft import DB_MAX, DB_RMS
from test_gpu_stream_each import run_each, timeline
from test_gpu_streaming import run_stream, same_bits
import test_gpu_streaming as S25

pytestmark = pytest.mark.gpu

RATES = (24000, 48000)
KEYS = ("out", "mel", "pred")
S, SPF, FPS = 4, 24, 30.0


def geom(sr):
    """-> (P, n_fft, hop, slice, L) of the 30-fps geometry at sr"""
    n_fft = sr // 30
    return n_fft // 800, n_fft, n_fft // 4, sr // 5, S * (sr // 5)


@functools.lru_cache(None)
def inputs():
    """The video of three utterances, its normaliser and the (24, 6) model: made once; the tests only read them."""
    from avse_amd.model import KerasModel
    rng = np.random.default_rng(5)
    synth_audio(rng, 3, geom(24000)[4], 24000)                              # (the draws audio() makes before the video's)
    video = synth_video(rng, 3 * S, f=6).reshape(3, S, 128, 128, 6)
    mean, std = R.video_normalizer_fit(video.reshape(3 * S, 128, 128, 6))
    return video, mean, std, KerasModel.init(seed=8, randomize=True, audio_shape=(80, SPF), video_shape=(128, 128, 6))


@functools.lru_cache(None)
def audio(sr):
    """Three utterances at sr (int16-scale): made once; the tests only read them."""
    return synth_audio(np.random.default_rng(5), 3, geom(sr)[4], sr)


@functools.lru_cache(None)
def weights(dtype):
    from avse_amd import ops
    return ops.DeviceWeights(inputs()[3], dtype)


def tone_utterance(sr):
    """Utterance 0 with its first slice replaced by a quiet 440-Hz tone."""
    sl = geom(sr)[3]
    x2 = audio(sr)[0].copy()
    x2[:sl] = np.round(2 * np.sin(2 * np.pi * 440 * np.arange(sl) / float(sr)))
    return x2


@functools.lru_cache(None)
def oracle(sr, which, causal=False):
    """tests/test_gpu_stream_rates.py's oracle at 30 fps.  which: 0..2 (utterance u), "tone" (with utterance 0's video)
    or "short" (utterance 0 cut by 700 samples)
    -> dict(unclamped [80, 97], mel [S, 80, 24] as the network sees it, pred [S, 80, 24], wave [L - hop])."""
    video, mean, std, model = inputs()
    _, n_fft, hop, _, L = geom(sr)
    u = which if isinstance(which, int) else 0
    sig = {"tone": tone_utterance(sr), "short": audio(sr)[0][:L - 700]}.get(which, audio(sr)[u])
    sig = R.fit_length(sig, L)
    D = R.stft(sig, n_fft=n_fft, hop_length=hop)
    mag, phase = R.magphase(D)
    un = R.amplitude_to_db(np.dot(R.mel_filterbank(sr, n_fft, n_mels=80, fmin=0, fmax=8000), mag), top_db=None)
    if causal:
        mel = np.stack([np.maximum(un[:, SPF * k:SPF * k + SPF], un[:, :SPF * k + SPF].max() - 80.0) for k in range(S)])
    else:
        mel = R.preprocess_audio_signal(sig, sr, 200, S, FPS)
    vn = R.video_normalize(video[u], mean, std).astype(np.float32)
    pred = K.forward(model.layer_dict(), mel.astype(np.float32), vn)
    if causal:
        wave = R.reconstruct_signal_from_spectrogram(np.concatenate(list(pred.astype(np.float32)), axis=1),
                                                     phase[:, :SPF * S], sr, n_fft, hop)
    else:
        wave = R.reconstruct_speech_signal(sig, sr, pred.astype(np.float32), FPS)
    return dict(unclamped=un, mel=mel, pred=pred, wave=wave)


def enhancer(sr, dtype, B, **kw):
    from avse_amd.pipeline import StreamEnhancer
    return StreamEnhancer(weights(dtype), B, video_frame_rate=FPS, sample_rate=sr, **kw)


def run(enh, x, video, pushes, video_at=None, flush=True):
    """test_gpu_streaming.run_stream with this file's normaliser."""
    return run_stream(enh, x, video, pushes, video_at, flush, mean=inputs()[1], std=inputs()[2])


@functools.lru_cache(None)
def streamed(sr, dtype, B=2):
    """Utterances 0 .. B - 1 pushed one slice per call with one video slice each, then flushed; shared by the tests."""
    sl = geom(sr)[3]
    return run(enhancer(sr, dtype, B), audio(sr)[:B], inputs()[0][:B], [sl] * S, video_at=[1] * S)


def expected_n_out(enh, pushes, video_at, flush=True):
    from avse_amd import ops
    n = v = prev = 0
    out = []
    for p, nv in zip(pushes, video_at):
        n, v = n + p, v + nv
        e = ops.stream_counts(n, v, session=enh.session)[2]
        out.append(e - prev)
        prev = e
    return out + ([ops.stream_counts(n, v, flushed=True, session=enh.session)[2] - prev] if flush else [])


def odd_cut(sr):
    """Four pushes, none a multiple of the hop (test_gpu_streaming's "odd", scaled to this slice)."""
    _, _, _, sl, L = geom(sr)
    a = 5000 * sl // 3200
    return [321, 7, a, L - 328 - a]


# ---- 1. oracle parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,dtype", [(24000, "float32"), (24000, "float32_split"), (48000, "float32"),
                                      (48000, "float32_split"), (48000, "bfloat16")])
def test_stream_matches_the_oracle_at_30_fps(gpu, sr, dtype):
    B = 2
    P, n_fft, hop, sl, L = geom(sr)
    for u in range(B):      # the precondition of "the stream is the offline result": the floor never binds
        un = oracle(sr, u)["unclamped"]
        print(f"{sr} Hz utterance {u}: unclamped mel-dB range {un.max() - un.min():.1f} dB")
        assert un.max() - un.min() < 80.0
    got = streamed(sr, dtype)
    assert got["out"].shape == (B, L - hop) and got["mel"].shape == got["pred"].shape == (B, S, 80, SPF)
    assert got["n_out"] == [0, sl - 2 * hop, sl, sl, sl + hop]
    assert got["n_out"] == expected_n_out(enhancer(sr, dtype, 1), [sl] * S, [1] * S)
    wave_gate = WAVE_BF16 if dtype == "bfloat16" else 1e-4
    for u in range(B):
        ref = oracle(sr, u)
        d = got["mel"][u].astype(np.float64) - ref["mel"]
        dmax, drms = np.abs(d).max(), np.sqrt(np.mean(d ** 2))
        err, perr = rel_rms(got["out"][u], ref["wave"]), rel_rms(got["pred"][u], ref["pred"])
        print(f"{sr} Hz {dtype} stream {u}: mel_db max {dmax:.2e} dB, RMS {drms:.2e} dB; predicted mel-dB rel RMS "
              f"{perr:.3e}; waveform rel RMS {err:.3e} vs the oracle")
        assert dmax <= DB_MAX and drms <= DB_RMS, (u, dmax, drms)
        assert err <= wave_gate, (u, err)
        if dtype == "bfloat16":
            assert perr <= MEL_BF16, (u, perr)


# ---- 2. against the offline device path ------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_stream_matches_the_offline_enhancer_at_30_fps(gpu, sr):
    """The offline path at these n_fft is a direct DFT (k_spec_dft / k_istft_dft), so the two cannot be bit-equal: each
    is gated at 1e-4 against the oracle, hence 2e-4 against each other."""
    from avse_amd import ops
    from avse_amd.pipeline import Enhancer
    B, dtype = 2, "float32_split"
    video, mean, std, _ = inputs()
    got = streamed(sr, dtype)
    off = Enhancer(weights(dtype), video_frame_rate=FPS, sample_rate=sr)(
        ops.to_device(audio(sr)[:B]), ops.to_device(video[:B]), ops.to_device(mean), ops.to_device(std)).cpu().numpy()
    assert off.shape == got["out"].shape
    for u in range(B):
        e, eoff = rel_rms(got["out"][u], off[u]), rel_rms(off[u], oracle(sr, u)["wave"])
        print(f"{sr} Hz stream {u}: waveform rel RMS {e:.3e} vs the offline Enhancer (itself {eoff:.3e} vs the oracle)")
        assert e <= 2e-4, (u, e)


# ---- 3. the causal floor ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_floor_is_causal_at_30_fps(gpu, sr):
    sl = geom(sr)[3]
    x, video = audio(sr), inputs()[0]
    xb = np.stack([tone_utterance(sr), x[0]])
    vb = np.stack([video[0], video[0]])
    causal, offline_mel = oracle(sr, "tone", causal=True), R.preprocess_audio_signal(tone_utterance(sr), sr, 200, S, FPS)
    un = causal["unclamped"]
    differ = float(np.mean(causal["mel"][0] != offline_mel[0]))
    print(f"{sr} Hz oracle: range {un.max() - un.min():.1f} dB; the causal and the offline clamp differ on "
          f"{100 * differ:.1f} % of slice 0, by up to {np.abs(causal['mel'] - offline_mel).max():.1f} dB; later slices "
          f"equal: {np.array_equal(causal['mel'][1:], offline_mel[1:])}")
    assert un.max() - un.min() > 80.0 and differ > 0.5                                             # the input bites
    got = run(enhancer(sr, "float32_split", 2), xb, vb, [sl] * S, video_at=[1] * S)
    d = got["mel"][0].astype(np.float64) - causal["mel"]
    print(f"{sr} Hz stream mel_db vs the causal oracle: max {np.abs(d).max():.2e} dB, RMS {np.sqrt(np.mean(d ** 2)):.2e} dB")
    assert np.abs(d).max() <= DB_MAX and np.sqrt(np.mean(d ** 2)) <= DB_RMS
    assert np.abs(got["mel"][0][0] - offline_mel[0]).max() > 1.0          # not the offline clamp
    err = rel_rms(got["out"][0], causal["wave"])
    print(f"{sr} Hz stream waveform vs the causal oracle pipeline: rel RMS {err:.3e}")
    assert err <= 1e-4
    # floors are per stream: the unmodified utterance beside it is what it is in the shared run's session
    ref = streamed(sr, "float32_split")
    for key in KEYS:
        assert same_bits(got[key][1], ref[key][0]), key


# ---- 4. cut invariance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_output_does_not_depend_on_the_cut_at_30_fps(gpu, sr):
    """The cuts of tests/test_gpu_stream_rates.py scaled to this slice (q = slice / 3200 = 3 / 2 or 3)."""
    B = 2
    P, n_fft, hop, sl, L = geom(sr)
    x, video = audio(sr)[:B], inputs()[0][:B]
    enh = enhancer(sr, "float32_split", B)
    small = [1000 * sl // 3200] * 12 + [800 * sl // 3200]
    odd = odd_cut(sr)
    patterns = {"slices": [sl] * 4, "aligned": [sl + hop, sl, sl, sl - hop], "whole": [L], "small": small, "odd": odd}
    cases = [(name, p, [S] + [0] * (len(p) - 1)) for name, p in patterns.items()]
    cases.append(("not divisible by the hop or P", [321, 7, odd[2] + 1, odd[3] - 1], [S, 0, 0, 0]))
    cases.append(("video two slices late", [sl] * 4, [0, 0, 3, 1]))
    cases.append(("video slice by slice", small, [1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0]))
    assert any(n % hop and n % 2 for _, p, _ in cases for n in p)
    first = streamed(sr, "float32_split")       # one slice per call, video with it
    for name, pushes, video_at in cases:
        assert sum(pushes) == L, name
        enh.reset()
        got = run(enh, x, video, pushes, video_at)
        assert got["n_out"] == expected_n_out(enh, pushes, video_at), name
        assert got["out"].shape == (B, L - hop), name
        for key in KEYS:
            assert same_bits(first[key], got[key]), (name, key)
    # a flush 700 samples short is the zero-padded stream
    enh1 = enhancer(sr, "float32_split", 1)
    short = run(enh1, x[:1, :L - 700], video[:1], [sl, sl, sl, sl - 700])
    enh1.reset()
    padded = np.concatenate([x[:1, :L - 700], np.zeros((1, 700), np.float32)], axis=1)
    full = run(enh1, padded, video[:1], [sl] * 4)
    assert short["out"].shape == (1, L - hop)
    for key in KEYS:
        assert same_bits(short[key], full[key]), key
    err = rel_rms(short["out"][0], oracle(sr, "short")["wave"])
    print(f"{sr} Hz flush of a stream 700 samples short: waveform rel RMS {err:.3e} vs the oracle on fit_length")
    assert err <= 1e-4


# ---- 5. independent streams ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_lock_step_streams_are_independent_at_30_fps(gpu, sr):
    """Stream b of a B = 3 lock-step session has the bits of its own B = 1 session; uint8 video gives the float32-video
    bits."""
    dtype = "float32_split"
    x, video = audio(sr), inputs()[0]
    pushes, video_at = odd_cut(sr), [2, 0, 1, 1]
    all3 = run(enhancer(sr, dtype, 3), x, video, pushes, video_at)
    for b in range(3):
        single = run(enhancer(sr, dtype, 1), x[b:b + 1], video[b:b + 1], pushes, video_at)
        for key in KEYS:
            assert same_bits(all3[key][b], single[key][0]), (b, key)
    u8 = run(enhancer(sr, dtype, 3, video_dtype=torch.uint8), x, video.astype(np.uint8), pushes, video_at)
    for key in KEYS:
        assert same_bits(all3[key], u8[key]), key


@pytest.mark.parametrize("sr", RATES)
def test_independent_streams_at_30_fps(gpu, sr):
    """push_each with three streams at their own paces: stream 1 idles for a tick, stream 2 hangs up early (close) and
    its slot is taken by a new caller (open); most calls leave a stream idle.  Each stream has the bits of a session of
    its own."""
    from avse_amd import ops
    dtype = "float32_split"
    P, n_fft, hop, sl, L = geom(sr)
    video, mean, std, _ = inputs()
    x = audio(sr)
    md, sd = ops.to_device(mean), ops.to_device(std)
    slices = (tuple([sl] * 4), (1, 1, 1, 1), (0, 1, 2, 3, 6))
    odd = (tuple(odd_cut(sr)), (2, 0, 1, 1), (0, 2, 3, 4, 5))                 # idle in call 1
    enh = enhancer(sr, dtype, 3)
    assert [enh.open() for _ in range(3)] == [0, 1, 2]
    plan = timeline([slices, odd, ((sl, sl), (1, 1), (0, 1, 6))])
    part1 = run_each(enh, [x[0], x[1], x[2]], [video[0], video[1], video[2]], plan[:2], mean, std, check_counts=False)
    assert enh.counts["samples"] == [2 * sl, 321, 2 * sl]
    last = enh.close(2, md, sd)                                          # the early flush, the reset, the free slot
    assert enh.open() == 2 and enh.counts["samples"][2] == 0
    plan2 = timeline([((sl, sl), (1, 1), (2, 3, 6)), (odd[0][1:], odd[1][1:], odd[2][1:]), ((sl, sl), (1, 1), (2, 4, 5))])
    part2 = run_each(enh, [x[0][2 * sl:], x[1][321:], x[1]], [video[0][2:], video[1][2:], video[1]], plan2[2:], mean, std,
                     check_counts=False)

    def own(sig, vid, pushes, video_at):
        got = run(enhancer(sr, dtype, 1), sig[None, :sum(pushes)], vid[None, :sum(video_at)], list(pushes), list(video_at))
        return {k: got[k][0] for k in KEYS}
    whole = lambda b: {k: np.concatenate([part1[b][k], part2[b][k]]) for k in KEYS}
    for b, ref in ((0, own(x[0], video[0], slices[0], slices[1])), (1, own(x[1], video[1], odd[0], odd[1]))):
        for key in KEYS:
            assert same_bits(whole(b)[key], ref[key]), (b, key)
    first = own(x[2], video[2], (sl, sl), (1, 1))                         # slot 2's first caller: two slices, then close
    assert same_bits(np.concatenate([part1[2]["out"], last.cpu().numpy()]), first["out"])
    second = own(x[1], video[1], (sl, sl), (1, 1))                        # and its second
    for key in KEYS:
        assert same_bits(part2[2][key], second[key]), key
    assert same_bits(whole(0)["out"], streamed(sr, dtype)["out"][0])      # which is also the lock-step session's


# ---- 6. beside the 25-fps family -------------------------------------------------------------------------------
def test_a_30_fps_session_beside_a_25_fps_one_and_the_refusals(gpu):
    from avse_amd import _lib, ops
    from avse_amd.pipeline import StreamEnhancer
    dtype = "float32_split"
    w25, w30 = S25.weights(dtype), weights(dtype)
    with pytest.raises(ValueError):                                       # a (24, 6) model in a 25-fps session, as before
        StreamEnhancer(w30, 1)
    with pytest.raises(_lib.AvseError, match="status 1"):
        ops.stream_create(w30, 1)                                         # (the library's own check of the weights' shape)
    with pytest.raises(_lib.AvseError, match="status 3"):
        StreamEnhancer(w30, 1, video_frame_rate=30.0, sample_rate=16000)  # n_fft 533: slices drift
    with pytest.raises(_lib.AvseError, match="status 3"):
        ops.stream_create(w30, 1, sample_rate=16000, n_fft=800, hop_length=200, frames_per_slice=24)
    x16, video25, mean25, std25, _ = S25.inputs()
    alone = S25.run_stream(StreamEnhancer(w25, 1), x16[:1], video25[:1], [3200] * S, video_at=[1] * S)
    # the two sessions pushed alternately on one context
    video, mean, std, _ = inputs()
    ma, sa, mb, sb = (ops.to_device(t) for t in (mean25, std25, mean, std))
    e16, e48 = StreamEnhancer(w25, 1), enhancer(48000, dtype, 1)
    xa, xb = ops.to_device(x16[:1]), ops.to_device(audio(48000)[:1])
    va, vb = ops.to_device(video25[:1]), ops.to_device(video[:1])
    oa, ob = [], []
    for k in range(S):
        oa.append(e16.push(xa[:, 3200 * k:3200 * k + 3200].contiguous(), va[:, k:k + 1].contiguous(), ma, sa))
        ob.append(e48.push(xb[:, 9600 * k:9600 * k + 9600].contiguous(), vb[:, k:k + 1].contiguous(), mb, sb))
    oa.append(e16.flush(ma, sa))
    ob.append(e48.flush(mb, sb))
    assert same_bits(torch.cat(oa, dim=1).cpu().numpy(), alone["out"])
    assert same_bits(torch.cat(ob, dim=1).cpu().numpy()[0], streamed(48000, dtype)["out"][0])
    assert e16.range_bits == 0
