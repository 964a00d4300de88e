"""Streaming at 32 and 48 kHz ("32 and 48 kHz"): frames of N = 640 P samples (P = 2, 3) computed as
P interleaved 640-point frames (csrc/frame_poly.h; the P = 2, 3 instances of k_stream_spec / k_stream_synth /
k_stream_ola) against the float64 oracle pipeline at that rate, against the offline device path (a direct DFT at these
rates), and against themselves under every cut of the input.

Shapes are those of tests/test_gpu_streaming.py scaled by P: B <= 3 streams of S = 4 slices, L = 12800 P samples, that
file's video, normaliser and model.  The gates are that file's: DB_MAX / DB_RMS for the mel-dB the network sees, its
bfloat16 gates for the network's bfloat16 kernels, relative RMS 1e-4 for the waveform."""
import functools

import numpy as np
import pytest
import torch

from conftest import synth_audio
from oracle import keras_ref as K
from oracle import librosa_ref as R
from test_gpu_pipeline import MEL_BF16, WAVE_BF16, rel_rms
from test_gpu_stft import DB_MAX, DB_RMS
from test_gpu_stream_each import run_each, timeline
from test_gpu_streaming import PATTERNS, S, inputs, run_stream, same_bits, weights

pytestmark = pytest.mark.gpu

RATES = (32000, 48000)
KEYS = ("out", "mel", "pred")


def geom(sr):
    """-> (P, n_fft, hop, slice, L) of the 25-fps geometry at sr"""
    P = sr // 16000
    return P, 640 * P, 160 * P, 3200 * P, 12800 * P


@functools.lru_cache(None)
def audio(sr):
    """Three utterances at sr (int16-scale): made once; the tests only read them."""
    return synth_audio(np.random.default_rng(5), 3, geom(sr)[4], sr)


def tone_utterance(sr):
    """Utterance 0 with its first slice replaced by a quiet 440-Hz tone (test_gpu_streaming.tone_utterance at sr)."""
    sl = geom(sr)[3]
    x2 = audio(sr)[0].copy()
    x2[:sl] = np.round(2 * np.sin(2 * np.pi * 440 * np.arange(sl) / float(sr)))
    return x2


@functools.lru_cache(None)
def oracle(sr, which, causal=False):
    """test_gpu_streaming.oracle at sr.  which: 0..2 (utterance u) or "tone" (with utterance 0's video)
    -> dict(unclamped [80, 81], mel [S, 80, 20] as the network sees it, pred [S, 80, 20], wave [L - hop])."""
    _, video, mean, std, model = inputs()
    _, n_fft, hop, _, L = geom(sr)
    u = which if isinstance(which, int) else 0
    sig = R.fit_length(tone_utterance(sr) if which == "tone" else audio(sr)[u], L)
    D = R.stft(sig, n_fft=n_fft, hop_length=hop)
    mag, phase = R.magphase(D)
    un = R.amplitude_to_db(np.dot(R.mel_filterbank(sr, n_fft, n_mels=80, fmin=0, fmax=8000), mag), top_db=None)
    if causal:
        mel = np.stack([np.maximum(un[:, 20 * k:20 * k + 20], un[:, :20 * k + 20].max() - 80.0) for k in range(S)])
    else:
        mel = R.preprocess_audio_signal(sig, sr, 200, S, 25.0)
    vn = R.video_normalize(video[u], mean, std).astype(np.float32)
    pred = K.forward(model.layer_dict(), mel.astype(np.float32), vn)
    if causal:
        wave = R.reconstruct_signal_from_spectrogram(np.concatenate(list(pred.astype(np.float32)), axis=1),
                                                     phase[:, :20 * S], sr, n_fft, hop)
    else:
        wave = R.reconstruct_speech_signal(sig, sr, pred.astype(np.float32), 25.0)
    return dict(unclamped=un, mel=mel, pred=pred, wave=wave)


def enhancer(sr, dtype, B, **kw):
    from avse_amd.pipeline import StreamEnhancer
    return StreamEnhancer(weights(dtype), B, sample_rate=sr, **kw)


@functools.lru_cache(None)
def streamed(sr, dtype, B=2):
    """Utterances 0 .. B - 1 pushed one slice per call with one video slice each, then flushed; shared by the tests."""
    sl = geom(sr)[3]
    return run_stream(enhancer(sr, dtype, B), audio(sr)[:B], inputs()[1][:B], [sl] * S, video_at=[1] * S)


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


# ---- 1. oracle parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,dtype", [(32000, "float32"), (32000, "float32_split"), (48000, "float32"),
                                      (48000, "float32_split"), (48000, "bfloat16")])
def test_stream_matches_the_oracle_at_the_rate(gpu, sr, dtype):
    B = 2
    P, n_fft, hop, sl, L = geom(sr)
    for u in range(B):      # the precondition of "the stream is the offline result": the floor never binds
        un = oracle(sr, u)["unclamped"]
        print(f"{sr} Hz utterance {u}: unclamped mel-dB range {un.max() - un.min():.1f} dB")
        assert un.max() - un.min() < 80.0
    got = streamed(sr, dtype)
    assert got["out"].shape == (B, L - hop) and got["mel"].shape == got["pred"].shape == (B, S, 80, 20)
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
def test_stream_matches_the_offline_enhancer(gpu, sr):
    """The offline path at these rates is a direct DFT (k_spec_dft / k_istft_dft), so the two cannot be bit-equal: each
    is gated at 1e-4 against the oracle, hence 2e-4 against each other."""
    from avse_amd import ops
    from avse_amd.pipeline import Enhancer
    B, dtype = 2, "float32_split"
    _, video, mean, std, _ = inputs()
    got = streamed(sr, dtype)
    off = Enhancer(weights(dtype), sample_rate=sr)(ops.to_device(audio(sr)[:B]), ops.to_device(video[:B]),
                                                   ops.to_device(mean), ops.to_device(std)).cpu().numpy()
    assert off.shape == got["out"].shape
    for u in range(B):
        e, eoff = rel_rms(got["out"][u], off[u]), rel_rms(off[u], oracle(sr, u)["wave"])
        print(f"{sr} Hz stream {u}: waveform rel RMS {e:.3e} vs the offline Enhancer (itself {eoff:.3e} vs the oracle)")
        assert e <= 2e-4, (u, e)


# ---- 3. the causal floor ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_floor_is_causal_at_the_rate(gpu, sr):
    sl = geom(sr)[3]
    x, video = audio(sr), inputs()[1]
    xb = np.stack([tone_utterance(sr), x[0]])
    vb = np.stack([video[0], video[0]])
    causal, offline_mel = oracle(sr, "tone", causal=True), R.preprocess_audio_signal(tone_utterance(sr), sr, 200, S, 25.0)
    un = causal["unclamped"]
    raised = lambda m: float(np.mean(m[0] != un[:, :20]))
    print(f"{sr} Hz oracle: range {un.max() - un.min():.1f} dB; the causal floor raises {100 * raised(causal['mel']):.1f} % of "
          f"slice 0, the offline clamp {100 * raised(offline_mel):.1f} %; they differ on "
          f"{100 * np.mean(causal['mel'][0] != offline_mel[0]):.1f} % of it, by up to "
          f"{np.abs(causal['mel'] - offline_mel).max():.1f} dB")
    assert un.max() - un.min() > 80.0 and raised(causal["mel"]) > 0.5                             # the input bites
    assert np.mean(causal["mel"][0] != offline_mel[0]) > 0.5 and np.abs(causal["mel"][0] - offline_mel[0]).max() > 1.0
    got = run_stream(enhancer(sr, "float32_split", 2), xb, vb, [sl] * S, video_at=[1] * S)
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
def test_output_does_not_depend_on_the_cut_at_the_rate(gpu, sr):
    B = 2
    P, n_fft, hop, sl, L = geom(sr)
    x, video = audio(sr)[:B], inputs()[1][:B]
    enh = enhancer(sr, "float32_split", B)
    cases = [(name, [P * n for n in p], [S] + [0] * (len(p) - 1)) for name, p in PATTERNS.items()]
    cases.append(("not divisible by P", [321, 7, 5000 * P + 1, L - 5000 * P - 329], [S, 0, 0, 0]))
    cases.append(("video two slices late", [sl] * 4, [0, 0, 3, 1]))
    cases.append(("video slice by slice", [1000 * P] * 12 + [800 * P], [1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0]))
    first = streamed(sr, "float32_split")       # one slice per call, video with it
    for name, pushes, video_at in cases:
        assert sum(pushes) == L, name
        enh.reset()
        got = run_stream(enh, x, video, pushes, video_at)
        assert got["n_out"] == expected_n_out(enh, pushes, video_at), name
        assert got["out"].shape == (B, L - hop), name
        for key in KEYS:
            assert same_bits(first[key], got[key]), (name, key)


# ---- 5. independent streams ------------------------------------------------------------------------------------
def test_independent_streams_at_48_khz(gpu):
    """push_each with three streams at their own paces: stream 1 idles for a tick, stream 2 hangs up early (close) and
    its slot is taken by a new caller (open).  Each stream has the bits of a session of its own."""
    from avse_amd import ops
    sr, dtype = 48000, "float32_split"
    P, n_fft, hop, sl, L = geom(sr)
    x, video, mean, std, _ = inputs()
    x = audio(sr)
    md, sd = ops.to_device(mean), ops.to_device(std)
    slices = (tuple([sl] * 4), (1, 1, 1, 1), (0, 1, 2, 3, 6))
    odd = (tuple(P * n for n in PATTERNS["odd"]), (2, 0, 1, 1), (0, 2, 3, 4, 5))      # idle in call 1
    enh = enhancer(sr, dtype, 3)
    assert [enh.open() for _ in range(3)] == [0, 1, 2]
    plan = timeline([slices, odd, ((sl, sl), (1, 1), (0, 1, 6))])
    part1 = run_each(enh, [x[0], x[1], x[2]], [video[0], video[1], video[2]], plan[:2], check_counts=False)
    assert enh.counts["samples"] == [2 * sl, 321 * P, 2 * sl]
    last = enh.close(2, md, sd)                                          # the early flush, the reset, the free slot
    assert enh.open() == 2 and enh.counts["samples"][2] == 0
    plan2 = timeline([((sl, sl), (1, 1), (2, 3, 6)), (odd[0][1:], odd[1][1:], odd[2][1:]), ((sl, sl), (1, 1), (2, 4, 5))])
    part2 = run_each(enh, [x[0][2 * sl:], x[1][321 * P:], x[1]], [video[0][2:], video[1][2:], video[1]], plan2[2:],
                     check_counts=False)

    def own(sig, vid, pushes, video_at):
        got = run_stream(enhancer(sr, dtype, 1), sig[None, :sum(pushes)], vid[None, :sum(video_at)], list(pushes), list(video_at))
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


# ---- 6. refusals, and the 16 kHz session beside a 48 kHz one -----------------------------------------------------
def test_refusals_and_the_16_khz_session_beside_a_48_khz_one(gpu):
    from avse_amd import _lib, ops
    from avse_amd.pipeline import StreamEnhancer
    dtype = "float32_split"
    dw = weights(dtype)
    with pytest.raises(_lib.AvseError, match="status 3"):
        ops.stream_create(dw, 1, sample_rate=44100, n_fft=1764, hop_length=441)
    with pytest.raises(_lib.AvseError, match="status 3"):
        ops.stream_create(dw, 1, sample_rate=48000, n_fft=1920, hop_length=480, fmax=24000.0)
    x16, video, mean, std, _ = inputs()
    alone = run_stream(StreamEnhancer(dw, 1), x16[:1], video[:1], [3200] * S, video_at=[1] * S)
    # the two sessions pushed alternately on one context
    md, sd = ops.to_device(mean), ops.to_device(std)
    e16, e48 = StreamEnhancer(dw, 1), enhancer(48000, dtype, 1)
    xa, xb, vd = ops.to_device(x16[:1]), ops.to_device(audio(48000)[:1]), ops.to_device(video[:1])
    oa, ob = [], []
    for k in range(S):
        oa.append(e16.push(xa[:, 3200 * k:3200 * k + 3200].contiguous(), vd[:, k:k + 1].contiguous(), md, sd))
        ob.append(e48.push(xb[:, 9600 * k:9600 * k + 9600].contiguous(), vd[:, k:k + 1].contiguous(), md, sd))
    oa.append(e16.flush(md, sd))
    ob.append(e48.flush(md, sd))
    assert same_bits(torch.cat(oa, dim=1).cpu().numpy(), alone["out"])
    assert same_bits(torch.cat(ob, dim=1).cpu().numpy()[0], streamed(48000, dtype)["out"][0])
    assert e16.range_bits == 0
