"""Streaming from a camera at any frame rate (pipeline.StreamEnhancer(input_fps=R)): retimer ->
session (or retimer -> resampler -> session -> resampler with input_rate), against ops.retime -> the same
StreamEnhancer without input_fps fed those slices, bit for bit: the retimer does not depend on the cuts and the session
does not either.

Shapes: 3 slices (9,600 samples at 16 kHz) for B <= 3 streams, with the audio, video, normaliser, model and weights of
tests/test_gpu_streaming.py.  The camera's frames are the fixture's 4 x 5 frames per stream read as a 30-fps (or
30000/1001-fps) sequence of 20: ceil(20 * 5 / 6) = 17 frames at 25 fps, three slices and two frames dropped."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from test_gpu_stream_each import run_each, timeline
from test_gpu_streaming import inputs, run_stream, same_bits, weights

pytestmark = pytest.mark.gpu

S3, L3, N_FRAMES = 3, 9600, 20
KEYS = ("out", "mel", "pred")
NTSC = Fraction(30000, 1001)


def audio():
    return inputs()[0][:, :L3]


@functools.lru_cache(None)
def camera(u8=False):
    """[3, 20, 128, 128]: the fixture's slices [3, 4, 128, 128, 5] unrolled into frames; made once, only read."""
    v = np.ascontiguousarray(inputs()[1].transpose(0, 1, 4, 2, 3).reshape(3, N_FRAMES, 128, 128))
    return v.astype(np.uint8) if u8 else v


def enhancer(B, fps=30, u8=False, **kw):
    from avse_amd.pipeline import StreamEnhancer
    return StreamEnhancer(weights("float32_split"), B, input_fps=fps, video_dtype=torch.uint8 if u8 else torch.float32, **kw)


@functools.lru_cache(None)
def composition(fps, u0, B, u8=False):
    """ops.retime(all frames) -> a plain StreamEnhancer pushed once and flushed, for utterances u0 .. u0 + B - 1."""
    from avse_amd import ops
    from avse_amd.pipeline import StreamEnhancer
    slices = ops.retime(ops.video_to_device(camera(u8)[u0:u0 + B]), fps, 25, 5)
    assert slices.shape == (B, S3, 128, 128, 5)
    plain = StreamEnhancer(weights("float32_split"), B, video_dtype=torch.uint8 if u8 else torch.float32)
    got = run_stream(plain, audio()[u0:u0 + B], slices.cpu().numpy(), [L3])
    assert got["out"].shape == (B, L3 - 160) and got["mel"].shape == (B, S3, 80, 20)
    return {k: got[k] for k in KEYS}


# ---- 1. odd cuts equal the composition -------------------------------------------------------------------------
@pytest.mark.parametrize("fps,u8", [(30, False), (NTSC, False), (30, True)])
def test_odd_cuts_equal_the_composition(gpu, fps, u8):
    B = 2
    enh = enhancer(B, fps, u8)
    assert enh.retimer is not None and enh.input_fps == fps and enh.resampler_in is None
    # frames ahead of the samples and behind them, a call with a single frame, one with none
    pushes, frames_at = [321, 7, 4000, 3000, L3 - 7328], [7, 1, 0, 9, 3]
    got = run_stream(enh, audio()[:B], camera(u8)[:B], pushes, video_at=frames_at)
    assert sum(pushes) == L3 and sum(frames_at) == N_FRAMES
    c = enh.counts
    assert c["video_frames"] == N_FRAMES and c["video_slices"] == S3 and c["samples"] == L3 and c["emitted"] == L3 - 160
    ref = composition(fps, 0, B, u8)
    for key in KEYS:
        assert same_bits(got[key], ref[key]), key
    # and again after a reset: the retimer and the session start over together
    enh.reset()
    assert enh.counts["video_frames"] == 0
    again = run_stream(enh, audio()[:B], camera(u8)[:B], [L3], video_at=[N_FRAMES])
    for key in KEYS:
        assert same_bits(again[key], ref[key]), key


# ---- 2. independent streams ------------------------------------------------------------------------------------
def test_each_stream_has_the_bits_of_its_own_session(gpu):
    """Stream 0 a slice's worth per call, stream 1 in odd cuts and idle in most calls, stream 2 in small pushes with its
    frames late; each against a B = 1 object of its own with the same schedule, and against the composition."""
    small = [800] * 12
    schedules = [((3200, 3200, 3200), (6, 6, 8), (1, 4, 7, 10)),
                 ((321, 7, 5000, L3 - 5328), (11, 0, 0, 9), (0, 2, 3, 9, 13)),
                 (tuple(small), (0, 0, 1, 0, 7, 0, 0, 5, 0, 0, 3, 4), tuple(range(13)))]
    plan = timeline(schedules)
    enh = enhancer(3)
    got = run_each(enh, audio(), camera(), plan, check_counts=False)
    assert enh.counts["video_frames"] == N_FRAMES and enh.retimer.ks == [S3] * 3
    for b, (pushes, frames_at, _) in enumerate(schedules):
        own = run_stream(enhancer(1), audio()[b:b + 1], camera()[b:b + 1], list(pushes), list(frames_at))
        ref = composition(30, b, 1)
        for key in KEYS:
            assert same_bits(got[b][key], own[key][0]), (b, key)
            assert same_bits(got[b][key], ref[key][0]), (b, key)
    # a caller leaves slot 1 mid-stream and the next one takes it
    from avse_amd import ops
    enh.reset()
    mean, std = ops.to_device(inputs()[2]), ops.to_device(inputs()[3])
    xd, vd = ops.to_device(audio()), ops.video_to_device(camera())
    assert (enh.open(), enh.open()) == (0, 1)
    enh.push_each([None, xd[1][:3000], None], [None, vd[1][:9], None], None, mean, std)
    assert enh.counts["video_frames"] == [0, 9, 0] and enh.counts["video_slices"][1] == ops.retime_counts(30, 25, 5, 9)[1]
    last = enh.close(1, mean, std)
    assert last.dim() == 1 and enh.retimer.ns[1] == enh.retimer.ks[1] == enh.session.vs[1] == 0
    assert enh.open() == 1
    a = enh.push_each([None, xd[2], None], [None, vd[2], None], None, mean, std)[1]
    b = enh.close(1, mean, std)
    assert same_bits(torch.cat([a, b]).cpu(), composition(30, 2, 1)["out"][0])


# ---- 3. together with input_rate -------------------------------------------------------------------------------
def test_with_input_rate_it_is_the_composition_of_the_one_shot_calls(gpu):
    from avse_amd import ops
    from avse_amd.pipeline import StreamEnhancer
    from conftest import synth_audio
    B, RATE, n_in = 2, 44100, 26460                                   # 0.6 s at 44.1 kHz -> 9,600 samples at 16 kHz
    x = synth_audio(np.random.default_rng(12), B, n_in, RATE)
    enh = StreamEnhancer(weights("float32_split"), B, input_rate=RATE, input_fps=30)
    got = run_stream(enh, x, camera()[:B], [321, 9000, 31, n_in - 9352], video_at=[5, 0, 14, 1])
    c = enh.counts
    assert c["received"] == n_in and c["video_frames"] == N_FRAMES and c["samples"] == L3
    mid = ops.resample(ops.to_device(x), RATE, 16000)
    slices = ops.retime(ops.video_to_device(camera()[:B]), 30, 25, 5)
    plain = run_stream(StreamEnhancer(weights("float32_split"), B), mid.cpu().numpy(), slices.cpu().numpy(), [L3])
    ref = ops.resample(ops.to_device(plain["out"]), 16000, RATE).cpu().numpy()
    assert same_bits(got["out"], ref)
    for key in ("mel", "pred"):
        assert same_bits(got[key], plain[key]), key


# ---- 4. refusals, and nothing else changed ---------------------------------------------------------------------
@pytest.mark.parametrize("rate", [None, 44100])
def test_a_refused_call_leaves_every_object_as_it_was(gpu, rate):
    """The session's limits apply to the retimed counts and are decided before the retimer is launched."""
    from avse_amd import _lib, ops
    enh = enhancer(1, max_slices=1, **({} if rate is None else dict(input_rate=rate)))
    mean, std = ops.to_device(inputs()[2]), ops.to_device(inputs()[3])
    vd = ops.video_to_device(camera()[:1])
    xd = torch.zeros(1, 100, device=gpu)

    def state():
        rs = [ops.resampler_state(r) for r in (enh.resampler_in, enh.resampler_out) if r is not None]
        return ops.retimer_state(enh.retimer), ops.stream_state(enh.session), rs, dict(enh.counts)
    enh.push(xd, vd[:, :3].contiguous(), mean, std)
    before = state()
    assert before[0] == ([3], [0], [False])
    with pytest.raises(_lib.AvseError, match="stream 0: .*max_slices"):           # 16 frames: two more slices of video
        enh.push(None, vd[:, 3:19].contiguous(), mean, std)
    with pytest.raises(_lib.AvseError, match="stream 0: .*max_slices"):
        enh.push_each(None, [vd[0, 3:19]], None, mean, std)
    assert state() == before
    out = enh.push(None, vd[:, 3:8].contiguous(), mean, std)                      # and a call that fits goes through
    assert out.shape == (1, 0) and ops.retimer_state(enh.retimer) == ([8], [1], [False])
    enh.flush(mean, std)
    with pytest.raises(_lib.AvseError, match="after"):
        enh.push(None, vd[:, 8:9].contiguous(), mean, std)
    with pytest.raises(_lib.AvseError, match="after"):
        enh.flush(mean, std)
    assert ops.retimer_state(enh.retimer) == ([8], [1], [True])


def test_without_input_fps_nothing_changed(gpu):
    from avse_amd import _lib
    from avse_amd.pipeline import StreamEnhancer
    w = weights("float32_split")
    for enh in (StreamEnhancer(w, 1), StreamEnhancer(w, 1, input_fps=None), StreamEnhancer(w, 1, input_fps=25),
                StreamEnhancer(w, 1, input_fps=25.0)):
        assert enh.input_fps is None and enh.retimer is None
        assert set(enh.counts) == {"samples", "video_slices", "frames", "slices", "emitted"}
    with pytest.raises(ValueError, match="29.97 fps gives"):                       # as before this feature
        StreamEnhancer(w, 1, video_frame_rate=29.97)
    with pytest.raises(_lib.AvseError, match="65537 / 1"):
        StreamEnhancer(w, 1, video_frame_rate=25, input_fps=25 * 65537)
    enh = StreamEnhancer(w, 1, input_fps=29.97)                                    # the camera rate the session refuses
    assert enh.input_fps == Fraction(2997, 100)
