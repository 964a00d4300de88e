"""The frame retimer on the device (ops.retime / retimer_*, avse_retime_* / avse_retimer_*) against
the numpy restatement of its definition (tests/retime_ref.py), bit for bit: the arithmetic is exact integers for uint8
and a fixed float64 sequence for float32, so there is no tolerance.

Shapes: 128 x 128 frames, B <= 4 streams, at most 37 input frames per stream."""
import functools

import numpy as np
import pytest
import torch

import retime_ref
from test_retime_host import RATIOS

pytestmark = pytest.mark.gpu

DTYPES = {"uint8": np.uint8, "float32": np.float32}
N_MAX = 37
STREAM_RATIOS = [(6, 5), (1200, 1001), (3, 5), (12, 5), (5, 6), (1, 1)]


@functools.lru_cache(None)
def frames(dtype, seed=0, ties=False):
    """[N_MAX, 128, 128] frames, made once; the tests only read them.  uint8: random bytes; ties: consecutive frames
    differ in parity at every pixel, so a + b is odd wherever two neighbours are blended half and half.  float32:
    random normal around 50."""
    rng = np.random.default_rng(100 + seed)
    if dtype == "uint8":
        A = rng.integers(0, 256, (N_MAX, 128, 128)).astype(np.uint8)
        if ties:
            A = ((A >> 1 << 1) | (np.arange(N_MAX)[:, None, None] & 1)).astype(np.uint8)
        return A
    return (rng.normal(0, 50, (N_MAX, 128, 128))).astype(np.float32)


@functools.lru_cache(None)
def reference(dtype, seed, ratio, F, n, ties=False):
    return retime_ref.slices(frames(dtype, seed, ties)[:n], ratio[0], ratio[1], F)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ---- 1. the one-shot call is the definition --------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 6])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_one_shot_equals_the_definition(gpu, dtype, F):
    from avse_amd import ops
    ns = [0, 1, 2, F, F + 1, N_MAX]
    for ratio in sorted(RATIOS):
        a, b = RATIOS[ratio]
        ties = ratio == (5, 4) and dtype == "uint8"
        A = frames(dtype, 0, ties)
        got = ops.retime([dev(A[:n], gpu) for n in ns], a, b, F)
        assert len(got) == len(ns)
        for n, g in zip(ns, got):
            want = reference(dtype, 0, ratio, F, n, ties)
            assert g.shape[0] == ops.retime_counts(a, b, F, n, True)[1] == want.shape[0], (ratio, n)
            assert same(g.cpu().numpy(), want), (ratio, n)
        if ties:    # output 2 sits half way between frames 2 and 3: an odd sum rounds up
            x, y = A[2].astype(int), A[3].astype(int)
            assert np.all((x + y) % 2 == 1)
            assert np.array_equal(got[-1][0, :, :, 2].cpu().numpy(), (x + y + 1) // 2)
    # the batched form: [U, n, 128, 128] -> [U, S, 128, 128, F]
    A = np.stack([frames(dtype, 0)[:13], frames(dtype, 1)[:13]])
    got = ops.retime(dev(A, gpu), 30, 25, F)
    assert got.shape == (2, 11 // F, 128, 128, F)
    for u in range(2):
        assert same(got[u].cpu().numpy(), reference(dtype, u, (6, 5), F, 13))
    if dtype == "float32":      # r == 0 hands a's bits on: -0.0, inf and nan survive an equal-rate regrouping
        S = frames(dtype, 0)[:F].copy()
        S[0, 0, :4] = [-0.0, np.inf, -np.inf, np.nan]
        got = ops.retime(dev(S[None], gpu), 25, 25, F)
        assert same(got[0, 0].cpu().numpy(), np.ascontiguousarray(S.transpose(1, 2, 0)))


# ---- 2. the cuts do not matter ---------------------------------------------------------------------------------
def play(r, A, plan, gpu):
    """plan: a list of calls, each {stream: n frames or "flush" or (n, "flush")}; stream b reads A[b] from where it
    stands -> per stream the concatenated slices, and checks every call's counts against retime_counts."""
    from avse_amd import ops
    B = r.n_streams
    pos, done = [0] * B, [False] * B
    got = [[] for _ in range(B)]
    for call in plan:
        fr, fl = [None] * B, [False] * B
        before = [ops.retime_counts(r.fps_in, r.fps_out, r.F, pos[b], done[b])[1] for b in range(B)]
        for b, what in call.items():
            n, f = (what[0], True) if isinstance(what, tuple) else ((0, True) if what == "flush" else (what, False))
            fr[b] = dev(A[b][pos[b]:pos[b] + n], gpu) if n else None
            pos[b] += n
            fl[b] = f
            done[b] = done[b] or f
        out = ops.retimer_push_each(r, fr, fl)
        for b in range(B):
            after = ops.retime_counts(r.fps_in, r.fps_out, r.F, pos[b], done[b])[1]
            assert out[b].shape == (after - before[b], 128, 128, r.F), (b, call)      # host_k_new
            got[b].append(out[b])
    assert ops.retimer_state(r) == (pos, [sum(x.shape[0] for x in g) for g in got], done)
    return [torch.cat(g).cpu().numpy() for g in got]


@pytest.mark.parametrize("dtype,F", [("uint8", 5), ("float32", 5), ("uint8", 6), ("float32", 6)])
def test_any_cut_gives_the_one_shot_bits(gpu, dtype, F):
    from avse_amd import ops
    B = 4
    lens = [N_MAX, 31, 2 * F + 1, 20]
    A = [frames(dtype, b)[:lens[b]] for b in range(B)]
    tdt = torch.uint8 if dtype == "uint8" else torch.float32
    for ratio in STREAM_RATIOS:
        a, b_ = RATIOS[ratio]
        want = [reference(dtype, b, ratio, F, lens[b]) for b in range(B)]
        r = ops.retimer_create(B, a, b_, F, tdt, gpu)
        # whole, then closed
        got = play(r, A, [{b: (lens[b], "flush") for b in range(B)}], gpu)
        for b in range(B):
            assert same(got[b], want[b]), (ratio, "whole", b)
        # odd cuts that differ per stream, idle streams, a stream flushed in a call of its own, another with its last
        # frames; the first cut of stream 1 completes no slice, the 4 F frames of stream 0 complete three or more at
        # every ratio up to 6 / 5
        ops.retimer_reset_each(r)
        plan = [{0: 1, 1: 2, 3: 7},
                {0: 4 * F, 2: 1},
                {1: 1, 2: 2 * F - 1, 3: 1},
                {0: 2, 1: 17, 2: (1, "flush")},
                {0: lens[0] - 4 * F - 3, 3: 12},
                {1: 11, 3: "flush"},
                {0: "flush", 1: "flush"}]
        assert ops.retime_counts(a, b_, F, 2)[1] == 0
        if ratio[0] <= ratio[1] * 6 // 5:
            assert ops.retime_counts(a, b_, F, 4 * F + 1)[1] - ops.retime_counts(a, b_, F, 1)[1] >= 3
        got = play(r, A, plan, gpu)
        for b in range(B):
            assert same(got[b], want[b]), (ratio, "odd cuts", b)
    # frame by frame, in lock step and with a straggler, for the two camera rates
    for ratio in [(6, 5), (1200, 1001)]:
        a, b_ = RATIOS[ratio]
        r = ops.retimer_create(2, a, b_, F, tdt, gpu)
        plan = [{0: 1, 1: 1} if i % 3 else {0: 1} for i in range(lens[1])] + [{0: "flush", 1: "flush"}]
        n1 = sum(1 for c in plan if 1 in c and c[1] == 1)
        got = play(r, A[:2], plan, gpu)
        assert same(got[0], reference(dtype, 0, ratio, F, lens[1]))
        assert same(got[1], reference(dtype, 1, ratio, F, n1))


# ---- 3. flush, reset -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_flush_clamps_to_the_last_frame_and_drops_the_partial_slice(gpu, dtype):
    from avse_amd import ops
    F, B = 5, 3
    tdt = torch.uint8 if dtype == "uint8" else torch.float32
    # 15 -> 25 fps: 6 frames are final as 9 outputs (1 slice); a flush makes them ceil(6 * 5 / 3) = 10, the last one a
    # copy of frame 5 (position 5.4 clamps), and the second slice is complete
    r = ops.retimer_create(B, 15, 25, F, tdt, gpu)
    A = [frames(dtype, b)[:6] for b in range(B)]
    first = ops.retimer_push_each(r, [dev(a, gpu) for a in A])
    assert [x.shape[0] for x in first] == [1, 1, 1]
    last = ops.retimer_push_each(r, None, [True, False, True])
    assert [x.shape[0] for x in last] == [1, 0, 1]
    for b in (0, 2):
        assert same(torch.cat([first[b], last[b]]).cpu().numpy(), reference(dtype, b, (3, 5), F, 6))
        assert same(last[b][0, :, :, 4].cpu().numpy(), A[b][5])
    # stream 1 goes on: 7 frames -> 11 final outputs, and its flush (12 outputs) drops the two left over
    more = ops.retimer_push_each(r, [None, dev(frames(dtype, 1)[6:7], gpu), None])
    assert [x.shape[0] for x in more] == [0, 1, 0]
    end = ops.retimer_push_each(r, None, [False, True, False])
    assert [x.shape[0] for x in end] == [0, 0, 0]
    assert same(torch.cat([first[1], more[1]]).cpu().numpy(), reference(dtype, 1, (3, 5), F, 7))
    assert ops.retimer_state(r) == ([6, 7, 6], [2, 2, 2], [True, True, True])


def test_reset_each_leaves_the_other_streams_alone(gpu):
    from avse_amd import ops
    F, B = 5, 3
    r = ops.retimer_create(B, 30, 25, F, torch.uint8, gpu)
    A = [frames("uint8", b) for b in range(B)]
    got = [[] for _ in range(B)]
    out = ops.retimer_push_each(r, [dev(a[:8], gpu) for a in A])          # 6 final outputs: one slice, one pending
    for b in range(B):
        got[b].append(out[b])
    ops.retimer_reset_each(r, [1])                                       # a caller left; the next one starts at frame 0
    assert ops.retimer_state(r)[0] == [8, 0, 8]
    out = ops.retimer_push_each(r, [dev(A[0][8:20], gpu), dev(A[2][:9], gpu), dev(A[2][8:20], gpu)],
                                [True, True, True])
    for b in (0, 2):
        got[b].append(out[b])
        assert same(torch.cat(got[b]).cpu().numpy(), reference("uint8", b, (6, 5), F, 20)), b
    assert same(out[1].cpu().numpy(), reference("uint8", 2, (6, 5), F, 9))


# ---- 4. refusals, and nothing written past the completed slices -------------------------------------------------
def raw_push(r, fr, off, n_new, flush, out, cap, shift=(0, 0)):
    """avse_retimer_push_each itself, on a caller's `out` -> (status, host_k_new).  shift: bytes added to the two device
    pointers (a call that must be refused for its alignment)."""
    import ctypes
    from avse_amd import _lib
    at = lambda t, d: _lib.ptr(t) if not d else ctypes.c_void_p(t.data_ptr() + d)
    i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64)
    off, n_new, fl = i64(off), i64(n_new), np.ascontiguousarray(flush, dtype=np.uint8)
    got = np.full(r.n_streams, -9, np.int64)
    with torch.cuda.device(out.device if out is not None else fr.device):
        rc = _lib.load().avse_retimer_push_each(r.handle, at(fr, shift[0]), off.ctypes.data, n_new.ctypes.data,
                                                fl.ctypes.data, at(out, shift[1]), cap, got.ctypes.data,
                                                _lib.stream_handle(fr.device))
    return rc, got.tolist()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_refusals_leave_no_trace_and_nothing_is_written_past_the_slices(gpu, dtype):
    from avse_amd import _lib, ops
    F, B, INVALID = 5, 2, 1
    tdt = torch.uint8 if dtype == "uint8" else torch.float32
    sentinel = 0xA5 if dtype == "uint8" else -12345.0
    r = ops.retimer_create(B, 30, 25, F, tdt, gpu)
    A = [frames(dtype, b)[:20] for b in range(B)]
    fr = dev(np.concatenate([A[0][:13], A[1][:13]]), gpu)                # 11 final outputs each: two slices
    out = torch.full((6, 128, 128, F), sentinel, dtype=tdt, device=gpu)
    state = ops.retimer_state(r)
    lib = _lib.load()
    for bad, names in ((dict(n_new=[13, -1]), "stream 1: negative"), (dict(cap=3), "stream 1: out"),
                       (dict(out=None), "stream 0: out"), (dict(cap=-1), "negative"),
                       (dict(n_new=[2 ** 40 + 1, 13]), "stream 0: counts too large"),      # totals past 2^40 frames
                       (dict(n_new=[13, 2 ** 62]), "stream 1: counts too large"),
                       (dict(shift=(2, 0)), "4-byte aligned"), (dict(shift=(0, 1)), "4-byte aligned"),
                       (dict(shift=(4, 2)), "4-byte aligned")):
        kw = dict(fr=fr, off=[0, 13], n_new=[13, 13], flush=[0, 0], out=out, cap=4)
        kw.update(bad)
        rc, k = raw_push(r, **kw)
        assert rc == INVALID and k == [-9, -9], (bad, rc, k)
        assert names in lib.avse_last_error().decode(), (bad, lib.avse_last_error())
        assert ops.retimer_state(r) == state
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())                                 # no refused call launched anything
    rc, k = raw_push(r, fr, [0, 13], [13, 13], [0, 0], out, 6)
    assert rc == 0 and k == [2, 2]
    torch.cuda.synchronize()
    assert bool((out[4:] == sentinel).all())                             # four slices completed, four written
    rc, k2 = raw_push(r, dev(np.concatenate([A[0][13:], A[1][13:]]), gpu), [0, 7], [7, 7], [1, 0], out[4:], 2)
    assert rc == 0 and k2 == [1, 1]                                      # stream 0 closed: 17 outputs; stream 1: 16 final
    for bad in (dict(n_new=[1, 0]), dict(flush=[1, 0])):                 # stream 0 after its flush
        kw = dict(fr=fr, off=[0, 0], n_new=[0, 0], flush=[0, 0], out=out, cap=6)
        kw.update(bad)
        rc, k = raw_push(r, **kw)
        assert rc == INVALID and "stream 0" in lib.avse_last_error().decode() and "after" in lib.avse_last_error().decode()
    rc, k3 = raw_push(r, fr, [0, 0], [0, 0], [0, 1], None, 0)           # its 17th output fills no slice: no `out` needed
    assert rc == 0 and k3 == [0, 0]
    got = out.cpu().numpy()
    assert same(np.concatenate([got[0:2], got[4:5]]), reference(dtype, 0, (6, 5), F, 20))
    assert same(np.concatenate([got[2:4], got[5:6]]), reference(dtype, 1, (6, 5), F, 20))
    # the one-shot call: a sentinel slice behind the packed output, frames and out off a 16-byte boundary
    pad = 4 if dtype == "uint8" else 1                                   # 4 bytes
    raw = torch.zeros(pad + 13 * 128 * 128, dtype=tdt, device=gpu)
    raw[pad:] = dev(A[0][:13], gpu).reshape(-1)
    buf = torch.full((pad + 3 * 128 * 128 * F,), sentinel, dtype=tdt, device=gpu)
    k = np.full(1, -9, np.int64)
    off, n = np.zeros(1, np.int64), np.full(1, 13, np.int64)
    args = lambda cap: (_lib.context(gpu).handle, _lib.ptr(raw[pad:]), off.ctypes.data, n.ctypes.data, 1,
                        1 if dtype == "uint8" else 0, 30, 1, 25, 1, F, _lib.ptr(buf[pad:]), cap, k.ctypes.data,
                        _lib.stream_handle(gpu))
    assert (raw[pad:].data_ptr() % 16, buf[pad:].data_ptr() % 16) == (4, 4)
    assert lib.avse_retime_ragged(*args(1)) == INVALID and k[0] == -9 and b"utterance 0" in lib.avse_last_error()
    n[0] = 2 ** 40 + 1                                                   # totals past 2^40 frames
    assert lib.avse_retime_ragged(*args(3)) == INVALID and k[0] == -9
    assert b"utterance 0: counts too large" in lib.avse_last_error()
    n[0] = 13
    import ctypes
    odd = list(args(3))
    odd[1] = ctypes.c_void_p(raw[pad:].data_ptr() + 2)                   # frames off a 4-byte boundary
    assert lib.avse_retime_ragged(*odd) == INVALID and k[0] == -9 and b"4-byte aligned" in lib.avse_last_error()
    torch.cuda.synchronize()
    assert bool((buf == sentinel).all())                                 # no refused call launched anything
    assert lib.avse_retime_ragged(*args(3)) == 0 and k[0] == 2
    res = buf[pad:].cpu().numpy().reshape(3, 128, 128, F)
    assert same(res[:2], reference(dtype, 0, (6, 5), F, 13))
    assert np.all(res[2] == sentinel) and bool((buf[:pad] == sentinel).all())
    # a push on frames and out off a 16-byte boundary gives the aligned bits
    r1 = ops.retimer_create(1, 30, 25, F, tdt, gpu)
    rc, k = raw_push(r1, raw[pad:], [0], [13], [1], buf[pad:], 3)
    assert rc == 0 and k == [2]
    assert same(buf[pad:].cpu().numpy().reshape(3, 128, 128, F)[:2], reference(dtype, 0, (6, 5), F, 13))
