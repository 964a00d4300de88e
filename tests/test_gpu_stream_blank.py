"""Streams whose video is missing (pipeline.NoVideo, avse_stream_push_each_mixed): a blank slice
counts as a video slice, carries no bytes and is predicted from the all-zero normalised video, so every stream has, bit
for bit, the output of a session of its own that was fed zeros (no normaliser) for those slices.  B = 3 streams of
S = 4 slices, max_slices 4, the schedules of tests/test_gpu_stream_each.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_pipeline import MEL_BF16, WAVE_BF16, rel_rms
from test_gpu_stream_each import FLUSH, KEYS, ODD, SLICES, SMALL_LATE, timeline
from test_gpu_streaming import L, S, inputs, same_bits, weights

pytestmark = pytest.mark.gpu

# stream 0 has full video, stream 1 none, stream 2 on slices 0 and 2
PRESENT = np.array([[1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 1, 0]], bool)
# video two calls early: slices (blank flags among them) wait in the queue for their samples
EARLY = (SMALL_LATE[0], (2, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0), SMALL_LATE[2])
PLANS = {"interleaved": (SLICES, ODD, SMALL_LATE), "early": (EARLY, SLICES, ODD), "late": (SMALL_LATE, EARLY, SLICES)}


def play(enh, x, video, present, plan, mean=None, std=None):
    """Plays `plan` (test_gpu_stream_each.timeline) through enh.push_each; slice k of stream b goes in as video or,
    where present[b][k] is False, as NoVideo.  -> per stream dict(out, mel, pred, had: which completed slices had video)."""
    from avse_amd import ops
    from avse_amd.pipeline import NoVideo
    B = enh.session.n_streams
    xd = [ops.to_device(x[b]) for b in range(B)]
    vd = [ops.video_to_device(video[b]) for b in range(B)]
    pos, vpos = [0] * B, [0] * B
    got = [dict(out=[], mel=[], pred=[], had=[]) for _ in range(B)]
    for call in plan:
        samples, vids, flush = [None] * B, [None] * B, [False] * B
        for b, what in call.items():
            if what == FLUSH:
                flush[b] = True
                continue
            n, v = what
            samples[b] = xd[b][pos[b]:pos[b] + n]
            vids[b] = [vd[b][k:k + 1] if present[b][k] else NoVideo(1) for k in range(vpos[b], vpos[b] + v)] or None
            pos[b], vpos[b] = pos[b] + n, vpos[b] + v
        o, m, q = enh.push_each(samples, vids, flush, mean, std, return_spectrograms=True)
        for b in range(B):
            got[b]["out"].append(o[b]); got[b]["mel"].append(m[b]); got[b]["pred"].append(q[b])
            got[b]["had"] += enh.last_video_present[b]
            assert len(enh.last_video_present[b]) == m[b].shape[0]
    return [{k: (torch.cat(v).cpu().numpy() if k != "had" else v) for k, v in g.items()} for g in got]


@functools.lru_cache(None)
def own_session(dtype, b, sched):
    """The reference: a B = 1 plain session fed utterance b on its schedule, zeros for its blank slices, no normaliser."""
    from avse_amd.pipeline import StreamEnhancer
    x, video = inputs()[0], inputs()[1]
    v = video[b].copy()
    v[~PRESENT[b]] = 0
    return play(StreamEnhancer(weights(dtype), 1), x[b:b + 1], v[None], np.ones((1, S), bool), timeline([sched]))[0]


# ---- 1. premise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float32_split"])
def test_no_video_is_the_zero_video_forward(gpu, dtype):
    """ops.forward(video=None) == ops.forward(zeros, no normaliser), bit for bit: the definition of a blank slice."""
    from avse_amd import ops
    from test_gpu_forward import make_inputs
    mel, _ = make_inputs(3, 900)
    m = ops.to_device(mel)
    none = ops.forward(weights(dtype), m, None).cpu().numpy()
    zeros = ops.forward(weights(dtype), m, torch.zeros((3, 128, 128, 5), device=m.device)).cpu().numpy()
    assert same_bits(none, zeros)


# ---- 2. own-session bits, no normaliser ------------------------------------------------------------------------
@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("dtype,video_u8", [("float32", False), ("float32_split", False), ("float32_split", True),
                                            ("bfloat16", False)])
def test_each_stream_has_the_bits_of_its_own_zero_fed_session(gpu, dtype, video_u8, plan):
    from avse_amd import ops
    from avse_amd.pipeline import StreamEnhancer
    x, video = inputs()[0], inputs()[1]
    scheds = PLANS[plan]
    enh = StreamEnhancer(weights(dtype), 3, video_dtype=torch.uint8 if video_u8 else torch.float32)
    got = play(enh, x, video.astype(np.uint8) if video_u8 else video, PRESENT, timeline(list(scheds)))
    assert ops.stream_state(enh.session)[:2] == ([L] * 3, [S] * 3)
    assert ops.stream_blank(enh.session) == [0, 4, 2] and enh.counts["blank_slices"] == [0, 4, 2]
    for b, sched in enumerate(scheds):
        assert got[b]["had"] == PRESENT[b].tolist(), (b, got[b]["had"])
        assert got[b]["out"].shape == (L - 160,) and got[b]["mel"].shape == (S, 80, 20)
        if dtype != "bfloat16":
            ref = own_session(dtype, b, sched)      # uint8 crops give the float32-video bits
            for key in KEYS:
                assert same_bits(got[b][key], ref[key]), (b, key)
            continue
        # bfloat16: its forward is not batch-invariant bit for bit, so the B = 1 session of the same dtype is met
        # within the bfloat16 gates (the analysis is float32 and exact)
        ref = own_session(dtype, b, sched)
        assert same_bits(got[b]["mel"], ref["mel"]), b
        err, perr = rel_rms(got[b]["out"], ref["out"]), rel_rms(got[b]["pred"], ref["pred"])
        print(f"bfloat16 stream {b} ({plan}): waveform rel RMS {err:.3e}, predicted mel-dB rel RMS {perr:.3e}")
        assert err <= WAVE_BF16 and perr <= MEL_BF16, (b, err, perr)


# ---- 3. with a normaliser --------------------------------------------------------------------------------------
def test_blank_slices_under_a_normaliser(gpu):
    from avse_amd import ops
    from avse_amd.pipeline import StreamEnhancer
    x, video, mean, std, _ = inputs()
    dw = weights("float32_split")
    md, sd = ops.to_device(mean), ops.to_device(std)
    xs = np.stack([x[0]] * 3)                      # the same audio in every stream: only the video differs
    enh = StreamEnhancer(dw, 3)
    got = play(enh, xs, video, PRESENT, timeline([SLICES, SLICES, SLICES]), md, sd)
    alone = play(StreamEnhancer(dw, 1), xs[:1], video[:1], PRESENT[:1], timeline([SLICES]), md, sd)[0]
    for b in range(3):
        assert same_bits(got[b]["mel"], alone["mel"]), b
        assert got[b]["had"] == PRESENT[b].tolist()
        mel = ops.to_device(got[b]["mel"])
        for k in range(S):
            ref = ops.forward(dw, mel[k:k + 1], ops.to_device(video[b][k:k + 1]), md, sd) if PRESENT[b][k] else \
                ops.forward(dw, mel[k:k + 1], None)
            assert same_bits(got[b]["pred"][k], ref.cpu().numpy()[0]), (b, k)
    assert ops.stream_blank(enh.session) == [0, 4, 2] and enh.counts["blank_slices"] == [0, 4, 2]
    assert ops.stream_state(enh.session)[1] == [S] * 3 and enh.counts["video_slices"] == S


# ---- 4. no stall -----------------------------------------------------------------------------------------------
def test_a_stream_without_video_goes_on_emitting(gpu):
    from avse_amd import _lib, ops
    from avse_amd.pipeline import NoVideo, StreamEnhancer
    x = inputs()[0]
    xd = ops.to_device(x[:1])
    enh = StreamEnhancer(weights("float32_split"), 1)
    total = 0
    for k in range(6):                              # more than max_slices slices of audio: each comes out
        a = (k % S) * 3200
        total += enh.push(xd[:, a:a + 3200].contiguous(), NoVideo(1)).shape[1]
        assert total == ops.stream_counts(3200 * (k + 1), k + 1)[2]
    total += enh.flush().shape[1]
    assert total == ops.stream_counts(3200 * 6, 6, flushed=True)[2] and enh.counts["blank_slices"] == 6
    # audio and None: the stream waits for its video and is refused after max_slices, as before
    enh = StreamEnhancer(weights("float32_split"), 1)
    for k in range(4):
        assert enh.push(xd[:, :3200].contiguous(), None).shape[1] == 0
    with pytest.raises(_lib.AvseError, match="queued ahead of the video"):
        enh.push(xd[:, :3200].contiguous(), None)


# ---- 5. reset --------------------------------------------------------------------------------------------------
def test_reset_clears_queued_blank_flags(gpu):
    from avse_amd import ops
    from avse_amd.pipeline import NoVideo, StreamEnhancer
    x, video = inputs()[0], inputs()[1]
    dtype = "float32_split"
    full = np.ones((3, S), bool)
    fresh = play(StreamEnhancer(weights(dtype), 3), x, video, full, timeline([SLICES, ODD, SMALL_LATE]))
    enh = StreamEnhancer(weights(dtype), 3)
    half = timeline([SLICES, ODD, SMALL_LATE])[:6]
    first = play(enh, x, video, full, half)
    enh.push_each(video=[None, NoVideo(1), None])  # a blank flag queued ahead of stream 1's audio
    assert ops.stream_blank(enh.session)[1] == 1
    untouched = ops.stream_state(enh.session)[0][0]
    enh.reset_streams([1])
    assert ops.stream_blank(enh.session) == [0, 0, 0] and ops.stream_state(enh.session)[1][1] == 0
    # stream 1 again from the start, with full video, while the others stay where they were
    again = play(enh, x[1:2].repeat(3, 0), video[1:2].repeat(3, 0), full, [{1: c[1]} for c in timeline([SLICES, ODD, SMALL_LATE]) if 1 in c])
    for key in KEYS:
        assert same_bits(again[1][key], fresh[1][key]), key
    assert first[0]["out"].shape[0] > 0 and ops.stream_state(enh.session)[0][0] == untouched


# ---- 6. refusals -----------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_as_it_was(gpu):
    from avse_amd import _lib, ops
    from avse_amd.pipeline import NoVideo, StreamEnhancer
    x, video = inputs()[0], inputs()[1]
    dtype = "float32_split"
    plan = timeline([SLICES, ODD, SMALL_LATE])
    ref = play(StreamEnhancer(weights(dtype), 3), x, video, PRESENT, plan)
    enh = StreamEnhancer(weights(dtype), 3)
    s = enh.session
    lib = _lib.load()
    dev = torch.device("cuda", s.weights.ctx.device_index)
    zero = np.zeros(3, np.int64)
    n_out = np.zeros(3, np.int64)
    # v_present marks a slice of stream 2 present, video == NULL
    v_new, flags = np.array([0, 1, 1], np.int64), np.array([0, 1], np.uint8)
    with torch.cuda.device(dev):
        rc = lib.avse_stream_push_each_mixed(s.handle, None, None, ctypes.c_void_p(zero.ctypes.data), None,
                                             ctypes.c_void_p(v_new.ctypes.data), ctypes.c_void_p(flags.ctypes.data), None,
                                             None, None, None, 0, ctypes.c_void_p(n_out.ctypes.data), None, None, None, None,
                                             _lib.stream_handle(dev))
    assert rc == 1 and lib.avse_last_error().startswith(b"stream 2: ")
    # a blank slice past the queue limit (max_slices video slices ahead of the samples)
    with pytest.raises(_lib.AvseError, match="stream 1: more than max_slices video slices"):
        enh.push_each(video=[None, NoVideo(5), None])
    assert ops.stream_state(s) == ([0] * 3, [0] * 3, [False] * 3) and ops.stream_blank(s) == [0] * 3
    got = play(enh, x, video, PRESENT, plan)
    for b in range(3):
        for key in KEYS:
            assert same_bits(got[b][key], ref[b][key]), (b, key)
