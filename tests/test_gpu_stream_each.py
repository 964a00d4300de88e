"""Independent streams of one session (pipeline.StreamEnhancer.push_each / reset_streams, avse_stream_push_each /
avse_stream_reset_each / avse_stream_state; DESIGN.md §3 K17 "Independent streams").

The acceptance criterion is exact: the forward is batch-invariant and the per-stream kernels run the lock-step kernels'
frame code, so every stream must produce, bit for bit, what a session of its own (B = 1, lock-step calls) produces for
the same schedule.  Shapes are those of tests/test_gpu_streaming.py: B = 3 streams of S = 4 slices, max_slices 4."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_pipeline import MEL_BF16, WAVE_BF16, rel_rms
from test_gpu_streaming import L, PATTERNS, S, inputs, oracle, run_stream, same_bits, tone_utterance, weights

pytestmark = pytest.mark.gpu

FLUSH = "flush"
KEYS = ("out", "mel", "pred")


def timeline(schedules):
    """schedules[b] = (pushes, video_at, calls): stream b makes its i-th push in call calls[i] and is flushed in call
    calls[len(pushes)] -> the list of calls, each {stream: (n, v) or FLUSH}."""
    plan = [dict() for _ in range(1 + max(c[-1] for _, _, c in schedules))]
    for b, (pushes, video_at, calls) in enumerate(schedules):
        assert len(calls) == len(pushes) + 1 == len(video_at) + 1
        for n, v, c in zip(pushes, video_at, calls):
            plan[c][b] = (n, v)
        plan[calls[-1]][b] = FLUSH
    return plan


def run_each(enh, x, video, plan, mean=None, std=None, check_counts=True):
    """Plays `plan` (timeline) through enh.push_each; stream b reads x[b] and video[b] from where it stands.
    -> per stream dict(out [emitted], mel / pred [slices, 80, 20]) and the per-call (n_out, k_new) lists."""
    from avse_amd import ops
    _, _, m0, s0, _ = inputs()
    mean, std = ops.to_device(m0 if mean is None else mean), ops.to_device(s0 if std is None else std)
    B = enh.session.n_streams
    xd = [ops.to_device(x[b]) for b in range(B)]
    vd = [ops.video_to_device(video[b]) for b in range(B)]
    pos, vpos, done = [0] * B, [0] * B, [False] * B
    got = [dict(out=[], mel=[], pred=[]) for _ in range(B)]
    for call in plan:
        samples, vids, flush = [None] * B, [None] * B, [False] * B
        before = [ops.stream_counts(pos[b], vpos[b], done[b]) if check_counts else None for b in range(B)]
        for b, what in call.items():
            if what == FLUSH:
                flush[b] = done[b] = True
                continue
            n, v = what
            samples[b] = xd[b][pos[b]:pos[b] + n]
            vids[b] = vd[b][vpos[b]:vpos[b] + v] if v else None
            pos[b], vpos[b] = pos[b] + n, vpos[b] + v
        o, m, q = enh.push_each(samples, vids, flush, mean, std, return_spectrograms=True)
        for b in range(B):
            if check_counts:     # host_n_out / host_k_new are avse_stream_counts differences (ops checks the library's)
                after = ops.stream_counts(pos[b], vpos[b], done[b])
                assert o[b].shape == (after[2] - before[b][2],), (b, call)
                assert m[b].shape == q[b].shape == (after[1] - before[b][1], 80, 20), (b, call)
            got[b]["out"].append(o[b]); got[b]["mel"].append(m[b]); got[b]["pred"].append(q[b])
    return [{k: torch.cat(v).cpu().numpy() for k, v in g.items()} for g in got]


@functools.lru_cache(None)
def alone(dtype, which, pushes, video_at, n_slices=S):
    """The reference: a B = 1 lock-step session fed utterance `which` ("tone": the tone utterance with utterance 0's
    video) in `pushes` with video by `video_at`, flushed.  Made once per schedule; the tests only read it."""
    from avse_amd.pipeline import StreamEnhancer
    x, video = inputs()[0], inputs()[1]
    sig, vid = (tone_utterance(), video[0]) if which == "tone" else (x[which], video[which])
    got = run_stream(StreamEnhancer(weights(dtype), 1), sig[None, :sum(pushes)], vid[None, :n_slices], list(pushes),
                     list(video_at))
    return {k: got[k][0] for k in KEYS}


def assert_bits(got, ref, what):
    for key in KEYS:
        assert same_bits(got[key], ref[key]), (what, key)


# the three schedules of test 4, interleaved: most calls have an idle stream, the counters are never equal, and the
# streams are flushed in calls 11, 13 and 14
SLICES = (tuple(PATTERNS["slices"]), (1, 1, 1, 1), (1, 4, 7, 10, 11))
ODD = (tuple(PATTERNS["odd"]), (2, 0, 1, 1), (0, 2, 3, 9, 14))
SMALL_LATE = (tuple(PATTERNS["small"]), (0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0), tuple(range(14)))   # video two calls late


# ---- 4. own-schedule bits --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,video_u8", [("float32", False), ("float32_split", False), ("float32_split", True),
                                            ("bfloat16", False)])
def test_each_stream_has_the_bits_of_its_own_session(gpu, dtype, video_u8):
    from avse_amd import ops
    from avse_amd.pipeline import StreamEnhancer
    x, video = inputs()[0], inputs()[1]
    plan = timeline([SLICES, ODD, SMALL_LATE])
    assert sum(1 for c in plan if len(c) < 3) > len(plan) // 2          # most calls leave a stream idle
    enh = StreamEnhancer(weights(dtype), 3, video_dtype=torch.uint8 if video_u8 else torch.float32)
    got = run_each(enh, x, video.astype(np.uint8) if video_u8 else video, plan)
    n, v, f = ops.stream_state(enh.session)
    assert n == [L] * 3 and v == [S] * 3 and f == [True] * 3
    for b, sched in enumerate((SLICES, ODD, SMALL_LATE)):
        ref = alone(dtype, b, sched[0], sched[1])      # (uint8 crops give the float32-video bits: test_gpu_streaming)
        assert got[b]["out"].shape == (L - 160,) and got[b]["mel"].shape == (S, 80, 20)
        if dtype != "bfloat16":
            assert_bits(got[b], ref, f"stream {b}")
            continue
        # bfloat16: the analysis is float32 and exact; the network's bfloat16 kernels are reported, and gated at the
        # bounds of test_stream_matches_oracle_and_offline_enhancer
        assert same_bits(got[b]["mel"], ref["mel"]), b
        print(f"bfloat16 stream {b}: pred bits equal {same_bits(got[b]['pred'], ref['pred'])}, "
              f"out bits equal {same_bits(got[b]['out'], ref['out'])}")
        o = oracle(b)
        err, perr = rel_rms(got[b]["out"], o["wave"]), rel_rms(got[b]["pred"], o["pred"])
        print(f"bfloat16 stream {b}: waveform rel RMS {err:.3e}, predicted mel-dB rel RMS {perr:.3e} vs the oracle")
        assert err <= WAVE_BF16 and perr <= MEL_BF16, (b, err, perr)
    if dtype != "bfloat16":
        err = rel_rms(got[0]["out"], oracle(0)["wave"])
        print(f"{dtype} stream 0: waveform rel RMS {err:.3e} vs the oracle")
        assert err <= 1e-4


# ---- 5. leave and join -----------------------------------------------------------------------------------------
def test_a_slot_is_reused_by_the_next_caller(gpu):
    from avse_amd.pipeline import StreamEnhancer
    dtype = "float32_split"
    x, video, mean, std, _ = inputs()
    # the input bites: the first occupant of slot 1 (utterance 1, two slices) leaves a running maximum that, kept by
    # mistake, would clamp the quiet first slice of the tone utterance far above its own causal floor
    tone = oracle("tone", causal=True)
    un0, right = tone["unclamped"][:, :20], tone["mel"][0]
    stale_max = max(oracle(1)["unclamped"][:, :40].max(), un0.max())
    stale = np.maximum(un0, stale_max - 80.0)
    changed = float(np.mean(stale != right))
    print(f"oracle: a stale running maximum ({stale_max:.1f} dB against {un0.max():.1f} dB) changes {100 * changed:.1f} % of "
          f"the second occupant's slice 0")
    assert changed > 0.5

    enh = StreamEnhancer(weights(dtype), 3)
    slots = [enh.open() for _ in range(3)]
    assert slots == [0, 1, 2]
    half = (tuple([1600] * 8), (1, 0) * 4, tuple(range(9)))               # slot 2: 100-ms packets, calls 0 .. 7, flush 8
    first = ((3200, 3200), (1, 1), (0, 1, 2))                              # slot 1: two slices, then the caller hangs up
    plan = timeline([(SLICES[0], SLICES[1], (0, 1, 2, 3, 4)), first, half])
    xs, vs = [x[0], x[1], x[2]], [video[0], video[1], video[2]]
    part1 = run_each(enh, xs, vs, plan[:3])
    assert enh.counts["samples"] == [9600, 6400, 4800] and enh.session.fl == [False, True, False]
    enh.reset_streams([1])
    assert enh.counts["samples"] == [9600, 0, 4800] and enh.session.fl == [False, False, False]
    # slot 1 starts over with the tone utterance (utterance 0's video); slots 0 and 2 go on where they were
    second = ((3200,) * 4, (1,) * 4, (3, 4, 5, 6, 7))
    plan2 = timeline([((3200,), (1,), (3, 4)), second, ((1600,) * 5, (0, 1, 0, 1, 0), (3, 4, 5, 6, 7, 8))])
    from avse_amd import ops
    part2 = run_each(enh, [x[0][9600:], tone_utterance(), x[2][4800:]], [video[0][3:], video[0], video[2][2:]], plan2[3:],
                     check_counts=False)      # (positions restart at 0 here, so the counts are not those of the streams)
    md, sd = ops.to_device(mean), ops.to_device(std)
    whole = lambda b: {k: np.concatenate([part1[b][k], part2[b][k]]) for k in KEYS}
    assert_bits(part1[1], alone(dtype, 1, (3200, 3200), (1, 1), 2), "slot 1, first occupant")
    assert_bits(part2[1], alone(dtype, "tone", (3200,) * 4, (1,) * 4), "slot 1, second occupant")
    assert_bits(whole(0), alone(dtype, 0, SLICES[0], SLICES[1]), "slot 0")
    assert_bits(whole(2), alone(dtype, 2, (1600,) * 8, (1, 0) * 4), "slot 2")
    d = part2[1]["mel"][0].astype(np.float64) - right
    assert np.abs(d).max() < 1.0, "the second occupant's first slice has its own causal floor"

    # close(): flush + reset + free in one step; the slot's last samples are the flush's
    enh.reset()
    slot = enh.open()
    o = enh.push_each([ops.to_device(x[1][:6400]), None, None], [ops.to_device(video[1][:2]), None, None], None, md, sd)
    last = enh.close(slot, md, sd)
    ref = alone(dtype, 1, (3200, 3200), (1, 1), 2)
    assert same_bits(torch.cat([o[slot], last]).cpu().numpy(), ref["out"])
    assert enh.open() == slot and enh.session.ns == [0, 0, 0]


# ---- 6. the lock-step calls ------------------------------------------------------------------------------------
def test_lock_step_calls_on_unequal_streams(gpu):
    """After push_each has left the counters unequal, push / flush feed every stream the same counts, each from where it
    stands, and each stream still has the bits of its own session."""
    from avse_amd import _lib, ops
    from avse_amd.pipeline import StreamEnhancer
    dtype = "float32_split"
    x, video, mean, std, _ = inputs()
    md, sd = ops.to_device(mean), ops.to_device(std)
    xd, vd = ops.to_device(x), ops.to_device(video)
    enh = StreamEnhancer(weights(dtype), 3)
    outs = [[o] for o in enh.push_each([xd[0, :3200], xd[1, :1000], None], [vd[0, :1], None, None], None, md, sd)]
    pos, vpos = [3200, 1000, 0], [1, 0, 0]
    assert not enh.session.in_step
    for n, v in ((3200, 1), (3200, 2)):
        samples = torch.stack([xd[b, pos[b]:pos[b] + n] for b in range(3)])
        vids = torch.stack([vd[b, vpos[b]:vpos[b] + v] for b in range(3)])
        got = enh.push(samples, vids, md, sd)
        assert isinstance(got, list) and len(got) == 3           # per-stream results while the streams differ
        for b in range(3):
            outs[b].append(got[b])
            pos[b], vpos[b] = pos[b] + n, vpos[b] + v
    assert ops.stream_state(enh.session) == (pos, vpos, [False] * 3)
    for b, o in enumerate(enh.flush(md, sd)):
        outs[b].append(o)
    assert ops.stream_state(enh.session)[2] == [True] * 3
    refs = [alone(dtype, 0, (3200, 3200, 3200), (1, 1, 2)), alone(dtype, 1, (1000, 3200, 3200), (0, 1, 2), 3),
            alone(dtype, 2, (3200, 3200), (1, 2), 3)]
    for b in range(3):
        assert same_bits(torch.cat(outs[b]).cpu().numpy(), refs[b]["out"]), b
    with pytest.raises(_lib.AvseError, match="status 1"):      # every stream is flushed
        enh.flush(md, sd)


def test_lock_step_path_is_untouched(gpu):
    """Lock-step pushes on streams that never diverged: the same bits on a fresh session, on a session that was used
    stream by stream and reset, and per stream on a session of its own."""
    from avse_amd.pipeline import StreamEnhancer
    dtype = "float32_split"
    x, video = inputs()[0], inputs()[1]
    pushes, video_at = PATTERNS["odd"], [2, 0, 1, 1]
    fresh = run_stream(StreamEnhancer(weights(dtype), 3), x, video, pushes, video_at)
    used = StreamEnhancer(weights(dtype), 3)
    run_each(used, x, video, timeline([SLICES, ODD, SMALL_LATE])[:6])
    assert not used.session.in_step
    used.reset()
    assert used.session.in_step and used.counts["samples"] == 0
    again = run_stream(used, x, video, pushes, video_at)
    for key in KEYS:
        assert same_bits(fresh[key], again[key]), key
        for b in range(3):
            assert same_bits(fresh[key][b], alone(dtype, b, tuple(pushes), tuple(video_at))[key]), (key, b)


# ---- 7. refusals with a live session ---------------------------------------------------------------------------
def test_refusals_name_the_stream_and_leave_no_trace(gpu):
    from avse_amd import _lib, ops
    from avse_amd.pipeline import StreamEnhancer
    dtype = "float32_split"
    x, video, mean, std, _ = inputs()
    md, sd = ops.to_device(mean), ops.to_device(std)
    xd, vd = ops.to_device(x), ops.to_device(video)
    lib = _lib.load()
    enh = StreamEnhancer(weights(dtype), 3, max_slices=1)
    h, st = enh.session.handle, _lib.stream_handle(xd.device)
    buf = torch.empty((3, 4000), dtype=torch.float32, device=xd.device)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)

    def c_push(n_new, v_new, flush=None, samples=None, vids=None, out=buf, stride=4000):
        """straight on the C-ABI: ops always passes counts and an out_stride the call can take"""
        n, v = np.array(n_new, np.int64), np.array(v_new, np.int64)
        off = np.concatenate([[0], np.cumsum(np.maximum(n, 0))[:-1]]).astype(np.int64)
        fl = None if flush is None else np.array(flush, np.uint8)
        n_out = np.full(3, -7, np.int64)
        rc = lib.avse_stream_push_each(h, _lib.ptr(samples), ptr(off), ptr(n), _lib.ptr(vids), ptr(v),
                                       None if fl is None else ptr(fl), _lib.ptr(md), _lib.ptr(sd), _lib.ptr(out), stride,
                                       ptr(n_out), None, None, None, st)
        return rc, lib.avse_last_error(), n_out.tolist()

    def refused(want, stream, *args, **kw):
        state = ops.stream_state(enh.session)
        rc, msg, n_out = c_push(*args, **kw)
        assert rc == 1 and want in msg and b"stream %d:" % stream in msg, (rc, msg)
        assert n_out == [-7] * 3 and ops.stream_state(enh.session) == state      # nothing written, nothing counted
        return msg

    # streams 0 and 2 take their first slice; stream 1 stays behind (n = 3200, v = 1: no slice done yet)
    outs = [[o] for o in enh.push_each([xd[0, :3200], None, xd[2, :3200]], [vd[0, :1], None, vd[2, :1]], None, md, sd)]
    sig = torch.cat([xd[1, :6720]])
    refused(b"negative", 1, [0, -1, 0], [0, 0, 0])
    refused(b"negative", 2, [0, 0, 0], [0, 0, -3])
    refused(b"more than max_slices slices", 1, [0, 6720, 0], [0, 2, 0], samples=sig, vids=vd[1, :2].contiguous())
    refused(b"ahead of the video", 1, [0, 3300, 0], [0, 0, 0], samples=sig)
    refused(b"ahead of the samples", 0, [0, 0, 0], [2, 0, 0], vids=vd[0, 1:3].contiguous())
    refused(b"n > slice * v", 2, [0, 0, 100], [0, 0, 0], flush=[0, 0, 1], samples=xd[2, 3200:3300].contiguous())
    step = xd[0, 3200:3360].contiguous()                   # completes slice 0 of stream 0: it emits 2880 samples
    refused(b"out_stride", 0, [160, 0, 0], [0, 0, 0], samples=step, stride=2879)
    refused(b"out_stride", 0, [160, 0, 0], [0, 0, 0], samples=step, out=None)
    # stream 1 is flushed empty; after that it takes no input and no second flush, the others are not affected
    rc, msg, n_out = c_push([0, 0, 0], [0, 0, 0], flush=[0, 1, 0])
    assert rc == 0 and n_out == [0, 0, 0], msg
    assert ops.stream_state(enh.session) == ([3200, 0, 3200], [1, 0, 1], [False, True, False])
    enh.session.fl[1] = True                                # the host mirror follows the direct call
    refused(b"after its flush", 1, [0, 5, 0], [0, 0, 0], samples=sig)
    refused(b"after its flush", 1, [0, 0, 0], [0, 0, 0], flush=[0, 1, 0])
    with pytest.raises(_lib.AvseError, match="stream 1"):   # and through ops
        enh.push_each([None, xd[1, :5], None], None, None, md, sd)
    # the refused calls left no trace: streams 0 and 2 finish with the bits of a run without them
    for k in range(1, S):
        got = enh.push_each([xd[0, 3200 * k:3200 * k + 3200], None, xd[2, 3200 * k:3200 * k + 3200]],
                            [vd[0, k:k + 1], None, vd[2, k:k + 1]], None, md, sd)
        outs[0].append(got[0]); outs[2].append(got[2])
    got = enh.push_each(flush=[True, False, True], vmean=md, vstd=sd)
    for b in (0, 2):
        outs[b].append(got[b])
        assert same_bits(torch.cat(outs[b]).cpu().numpy(), alone(dtype, b, SLICES[0], SLICES[1])["out"]), b
    assert enh.range_bits == 0


# ---- 8. the video's alignment ----------------------------------------------------------------------------------
def test_video_off_a_16_byte_boundary_gives_the_aligned_bits(gpu):
    """tests/test_gpu_streaming.py's test of this name through avse_stream_push_each (straight on the C-ABI: ops packs
    the streams' video into a fresh, aligned tensor): both streams of a B = 2 session take the same two slices from a
    packed video 4 bytes past a 16-byte boundary and from an aligned one, and are flushed."""
    from avse_amd import _lib, ops
    from avse_amd.pipeline import StreamEnhancer
    from test_gpu_streaming import offset_video
    B = 2
    x, video, mean, std, _ = inputs()
    md, sd = ops.to_device(mean), ops.to_device(std)
    xd, vd = ops.to_device(x[:B, :6400]), ops.to_device(video[:B, :2])
    lib = _lib.load()
    enh = StreamEnhancer(weights("float32"), B)
    h, st = enh.session.handle, _lib.stream_handle(xd.device)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)

    def c_push(samples, vids, n_new, v_new, flush):
        n, v, fl = np.full(B, n_new, np.int64), np.full(B, v_new, np.int64), np.full(B, flush, np.uint8)
        off = np.arange(B, dtype=np.int64) * n_new
        out = torch.zeros((B, 3400), dtype=torch.float32, device=xd.device)
        mel, pred = (torch.zeros((B, 80, 20), dtype=torch.float32, device=xd.device) for _ in range(2))
        n_out, k_new = np.full(B, -7, np.int64), np.full(B, -7, np.int64)
        rc = lib.avse_stream_push_each(h, _lib.ptr(samples), ptr(off), ptr(n), _lib.ptr(vids), ptr(v), ptr(fl), _lib.ptr(md),
                                       _lib.ptr(sd), _lib.ptr(out), 3400, ptr(n_out), _lib.ptr(mel), _lib.ptr(pred),
                                       ptr(k_new), st)
        assert rc == 0, lib.avse_last_error()
        assert n_out[0] == n_out[1] and k_new[0] == k_new[1]
        return out[:, :n_out[0]], mel[:B * k_new[0]], pred[:B * k_new[0]]

    runs = []
    for floats in (1, 0):
        enh.reset()
        got = []
        for k in range(2):
            vid = offset_video(vd[:, k].contiguous(), floats)       # packed: stream 0's slice, then stream 1's
            got.append(c_push(xd[:, 3200 * k:3200 * k + 3200].contiguous(), vid, 3200, 1, 0))
        got.append(c_push(None, None, 0, 0, 1))
        assert [g[0].shape[1] for g in got] == [0, 2880, 3360] and [g[1].shape[0] for g in got] == [0, B, B]
        runs.append([torch.cat([g[0] for g in got], dim=1).cpu().numpy()] +
                    [torch.cat([g[i] for g in got]).cpu().numpy() for i in (1, 2)])
    for key, off, aligned in zip(KEYS, *runs):
        assert np.isfinite(off).all() and same_bits(off, aligned), key
    # and they are the lock-step session's
    ref = run_stream(StreamEnhancer(weights("float32"), B), x[:B, :6400], video[:B, :2], [3200, 3200], [1, 1])
    assert same_bits(runs[0][0], ref["out"])
