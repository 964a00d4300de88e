"""Streaming at any sample rate (pipeline.StreamEnhancer(input_rate=R)): resampler in -> session ->
resampler out, against the composition of the one-shot calls (bit for bit: the resamplers do not depend on the cuts and
the session does not either), against B = 1 sessions of their own, and against the float64 oracle
eval_ref.resample -> oracle pipeline at 16 kHz -> eval_ref.resample.

Shapes: 3 slices (0.6 s: 26,460 samples at 44.1 kHz, 9,600 at 16 kHz) for B <= 3 streams, with the video, normaliser,
model and weights of tests/test_gpu_streaming.py; 2 slices of tests/test_gpu_stream_fps30.py's at 30 fps."""
import functools

import numpy as np
import pytest
import torch

import eval_ref
import test_gpu_stream_fps30 as F30
from conftest import synth_audio
from oracle import keras_ref as K
from oracle import librosa_ref as R
from test_gpu_pipeline import rel_rms
from test_gpu_stream_each import run_each, timeline
from test_gpu_streaming import inputs, run_stream, same_bits, weights

pytestmark = pytest.mark.gpu

RATE, S3 = 44100, 3
L_IN, L_MID, L_OUT = 26460, 9600, 26019          # samples in, at 16 kHz, and returned: (3 * 3200 - 160) * 441 / 160
KEYS = ("out", "mel", "pred")


@functools.lru_cache(None)
def audio():
    """Three utterances of three slices at 44.1 kHz (int16-scale): made once; the tests only read them."""
    return synth_audio(np.random.default_rng(11), 3, L_IN, RATE)


def video():
    return inputs()[1][:, :S3]


def enhancer(B, dtype="float32_split", **kw):
    from avse_amd.pipeline import StreamEnhancer
    return StreamEnhancer(weights(dtype), B, input_rate=RATE, **kw)


@functools.lru_cache(None)
def composition(dtype, u0, B):
    """ops.resample(44100 -> 16000) -> a plain StreamEnhancer pushed once and flushed -> ops.resample(16000 -> 44100),
    for utterances u0 .. u0 + B - 1 -> dict(out [B, L_OUT], mel / pred [B, 3, 80, 20]) as numpy."""
    from avse_amd import ops
    from avse_amd.pipeline import StreamEnhancer
    mid = ops.resample(ops.to_device(audio()[u0:u0 + B]), RATE, 16000)
    assert mid.shape == (B, L_MID)
    got = run_stream(StreamEnhancer(weights(dtype), B), mid.cpu().numpy(), video()[u0:u0 + B], [L_MID])
    assert got["out"].shape == (B, L_MID - 160)
    out = ops.resample(ops.to_device(got["out"]), 16000, RATE)
    assert out.shape == (B, L_OUT)
    return dict(out=out.cpu().numpy(), mel=got["mel"], pred=got["pred"])


@functools.lru_cache(None)
def oracle(u):
    """eval_ref.resample -> the float64 oracle pipeline at 16 kHz -> eval_ref.resample, for utterance u
    -> dict(unclamped [80, 61], wave [L_OUT])."""
    _, vid, mean, std, model = inputs()
    sig = R.fit_length(eval_ref.resample(audio()[u], 160, 441), L_MID)
    mag, _ = R.magphase(R.stft(sig, n_fft=640, hop_length=160))
    un = R.amplitude_to_db(np.dot(R.mel_filterbank(16000, 640, n_mels=80, fmin=0, fmax=8000), mag), top_db=None)
    mel = R.preprocess_audio_signal(sig, 16000, 200, S3, 25.0)
    vn = R.video_normalize(vid[u, :S3], mean, std).astype(np.float32)
    pred = K.forward(model.layer_dict(), mel.astype(np.float32), vn)
    wave = R.reconstruct_speech_signal(sig, 16000, pred.astype(np.float32), 25.0)
    assert wave.shape == (L_MID - 160,)
    return dict(unclamped=un, wave=eval_ref.resample(wave, 441, 160))


# ---- 1. odd cuts equal the composition -------------------------------------------------------------------------
def test_odd_cuts_equal_the_composition(gpu):
    B = 2
    enh = enhancer(B)
    # none a multiple of anything: a push shorter than the resampler's history (56), two that complete no slice
    pushes = [321, 7, 8500, 9000, 31, L_IN - 17859]
    got = run_stream(enh, audio()[:B], video()[:B], pushes, video_at=[1, 0, 0, 1, 0, 1])
    assert sum(pushes) == L_IN and got["out"].shape == (B, L_OUT) and got["mel"].shape == (B, S3, 80, 20)
    c = enh.counts
    assert c["received"] == L_IN and c["returned"] == L_OUT and c["samples"] == L_MID and c["emitted"] == L_MID - 160
    ref = composition("float32_split", 0, B)
    for key in KEYS:
        assert same_bits(got[key], ref[key]), key
    # and again after a reset: the three objects start over together
    enh.reset()
    again = run_stream(enh, audio()[:B], video()[:B], [L_IN], video_at=[S3])
    for key in KEYS:
        assert same_bits(again[key], ref[key]), key


# ---- 2. independent streams ------------------------------------------------------------------------------------
def test_each_stream_has_the_bits_of_its_own_session(gpu):
    """Stream 0 slice by slice, stream 1 in odd cuts and idle in most calls, stream 2 in small pushes with its video two
    calls late; then slot 1 is closed and reopened for utterance 2."""
    from avse_amd import ops
    sl = L_IN // S3
    small = [2205] * 12
    schedules = [((sl, sl, sl), (1, 1, 1), (1, 4, 7, 10)),
                 ((321, 7, 13000, L_IN - 13328), (2, 0, 0, 1), (0, 2, 3, 9, 13)),
                 (tuple(small), (0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1), tuple(range(13)))]
    plan = timeline(schedules)
    assert sum(1 for c in plan if len(c) < 3) > len(plan) // 2
    enh = enhancer(3)
    got = run_each(enh, audio(), video(), plan, check_counts=False)
    assert ops.stream_state(enh.session) == ([L_MID] * 3, [S3] * 3, [True] * 3)
    assert enh.resampler_in.ns == [L_IN] * 3 and enh.resampler_out.outs == [L_OUT] * 3
    assert enh.counts["received"] == L_IN and enh.counts["returned"] == L_OUT      # in step again: scalars
    for b, (pushes, video_at, _) in enumerate(schedules):
        own = run_stream(enhancer(1), audio()[b:b + 1], video()[b:b + 1], list(pushes), list(video_at))
        for key in KEYS:
            assert same_bits(got[b][key], own[key][0]), (b, key)
        ref = composition("float32_split", b, 1)      # which is the composition's, too
        assert same_bits(got[b]["out"], ref["out"][0]), b
    # a caller leaves slot 1 mid-stream and the next one takes it
    enh.reset()
    mean, std = ops.to_device(inputs()[2]), ops.to_device(inputs()[3])
    xd, vd = ops.to_device(audio()), ops.video_to_device(video())
    slot0, slot1 = enh.open(), enh.open()
    assert (slot0, slot1) == (0, 1)
    enh.push_each([None, xd[1][:12000], None], [None, vd[1][:2], None], None, mean, std)
    assert enh.counts["received"] == [0, 12000, 0] and enh.counts["samples"][1] == ops.resample_counts(RATE, 16000, 12000)
    last = enh.close(slot1, mean, std)
    assert last.dim() == 1 and enh.resampler_in.ns[1] == enh.resampler_out.outs[1] == enh.session.ns[1] == 0
    assert enh.open() == 1
    a = enh.push_each([None, xd[2], None], [None, vd[2], None], None, mean, std)[1]
    b = enh.close(1, mean, std)
    assert same_bits(torch.cat([a, b]).cpu(), composition("float32_split", 2, 1)["out"][0])


# ---- 3. against the float64 oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float32_split"])
def test_stream_matches_the_float64_oracle(gpu, dtype):
    B = 2
    for u in range(B):      # the precondition of "the stream is the offline result": the floor never binds
        un = oracle(u)["unclamped"]
        print(f"utterance {u} at 16 kHz: unclamped mel-dB range {un.max() - un.min():.1f} dB")
        assert un.max() - un.min() < 80.0
    sl = L_IN // S3
    got = run_stream(enhancer(B, dtype), audio()[:B], video()[:B], [sl] * S3, video_at=[1] * S3)
    assert got["out"].shape == (B, L_OUT)
    for u in range(B):
        err = rel_rms(got["out"][u], oracle(u)["wave"])
        print(f"{dtype} stream {u} at input_rate {RATE}: waveform rel RMS {err:.3e} vs the float64 oracle (gate 1e-4)")
        assert err <= 1e-4, (u, err)


# ---- 4. 30 fps -------------------------------------------------------------------------------------------------
def test_30_fps_session_at_24_khz_behind_44100(gpu):
    from avse_amd import ops
    from avse_amd.pipeline import StreamEnhancer
    B, S2, n_in, n_mid = 2, 2, 17640, 9600
    w30 = F30.weights("float32_split")
    vid = F30.inputs()[0][:B, :S2]
    x = audio()[:B, :n_in]
    kw = dict(video_frame_rate=30.0, sample_rate=24000)
    run = lambda enh, sig, pushes, at: run_stream(enh, sig, vid, pushes, at, mean=F30.inputs()[1], std=F30.inputs()[2])
    got = run(StreamEnhancer(w30, B, input_rate=RATE, **kw), x, [5000, 777, n_in - 5777], [1, 0, 1])
    mid = ops.resample(ops.to_device(np.ascontiguousarray(x)), RATE, 24000)
    assert mid.shape == (B, n_mid)
    plain = run(StreamEnhancer(w30, B, **kw), mid.cpu().numpy(), [n_mid], [S2])
    ref = ops.resample(ops.to_device(plain["out"]), 24000, RATE).cpu().numpy()
    assert plain["out"].shape == (B, n_mid - 200) and ref.shape == (B, -(-(n_mid - 200) * 147 // 80))
    assert same_bits(got["out"], ref)
    for key in ("mel", "pred"):
        assert same_bits(got[key], plain[key]), key


# ---- 5. nothing else changed, and the refusals -----------------------------------------------------------------
def test_without_input_rate_nothing_changed(gpu):
    from avse_amd import _lib, ops
    from avse_amd.pipeline import StreamEnhancer
    w = weights("float32_split")
    for enh in (StreamEnhancer(w, 1), StreamEnhancer(w, 1, input_rate=None), StreamEnhancer(w, 1, input_rate=16000)):
        assert enh.input_rate is None and enh.resampler_in is None and enh.resampler_out is None
        assert set(enh.counts) == {"samples", "video_slices", "frames", "slices", "emitted"}
    with pytest.raises(_lib.AvseError):
        StreamEnhancer(w, 1, sample_rate=44100)
    assert ops.stream_supported(44100, 1764, 441) == 3
    with pytest.raises(_lib.AvseError, match="16000 / 16001"):
        StreamEnhancer(w, 1, input_rate=16001)


def test_a_refused_call_leaves_the_three_objects_as_they_were(gpu):
    """The session's limits apply to the resampled counts and are decided before the first launch."""
    from avse_amd import _lib, ops
    B = 1
    enh = enhancer(B, max_slices=1)
    ref = composition("float32_split", 0, 1)
    mean, std = ops.to_device(inputs()[2]), ops.to_device(inputs()[3])
    xd, vd = ops.to_device(audio()[:B]), ops.video_to_device(video()[:B])
    sl = L_IN // S3
    state = lambda: (ops.resampler_state(enh.resampler_in), ops.stream_state(enh.session), ops.resampler_state(enh.resampler_out))
    outs = [enh.push(xd[:, :sl].contiguous(), vd[:, :1].contiguous(), mean, std)]
    before = state()
    with pytest.raises(_lib.AvseError, match="stream 0: .*max_slices"):           # two slices of samples, no video
        enh.push(xd[:, sl:3 * sl].contiguous(), None, mean, std)
    with pytest.raises(_lib.AvseError, match="stream 0: .*max_slices"):           # two slices completed by one call
        enh.push(xd[:, sl:3 * sl].contiguous(), vd[:, 1:3].contiguous(), mean, std)
    with pytest.raises(_lib.AvseError, match="stream 0: flush: more samples"):    # a flush the video does not cover
        enh.push_each([xd[0, sl:sl + 100]], None, [True], mean, std)
    assert state() == before
    for k in (1, 2):
        outs.append(enh.push(xd[:, k * sl:(k + 1) * sl].contiguous(), vd[:, k:k + 1].contiguous(), mean, std))
    outs.append(enh.flush(mean, std))
    with pytest.raises(_lib.AvseError, match="after"):
        enh.push(xd[:, :10].contiguous(), None, mean, std)
    with pytest.raises(_lib.AvseError, match="after"):
        enh.flush(mean, std)
    assert same_bits(torch.cat(outs, dim=1).cpu(), ref["out"])
