"""The device resampler (ops.resample / ops.resampler_*, csrc/resample.hip) against the float64
reference tests/eval_ref.py resample (scipy.signal.resample_poly's defaults, restated) and against itself under every
cut of the input.

Shapes: signals of at most 4999 samples, so every case is a handful of blocks; the lengths 0, 1, T - 1, T, T + 1
(T = 2H / up + 1, the history a stream keeps) are where the edge handling of the definition changes, 4999 spans more
than one block of 256 outputs at every ratio."""
import functools
import math

import numpy as np
import pytest
import torch

import eval_ref

pytestmark = pytest.mark.gpu

# (up, down) -> (sr_in, sr_out)
ONE_SHOT = {(160, 441): (44100, 16000), (441, 160): (16000, 44100), (640, 441): (11025, 16000),
            (441, 640): (16000, 11025), (2, 1): (8000, 16000), (80, 147): (44100, 24000)}
STREAMED = ((44100, 16000), (16000, 44100), (11025, 16000))


def ratio(a, b):
    g = math.gcd(a, b)
    return b // g, a // g


def taps_per_output(up, down):
    return 20 * max(up, down) // up + 1


@functools.lru_cache(None)
def signal(seed, n):
    """N(0, 3000) rounded to int16 scale: made once per (seed, n); the tests only read it."""
    return np.clip(np.round(np.random.default_rng(seed).normal(0, 3000, n)), -32768, 32767).astype(np.float32)


@functools.lru_cache(None)
def whole(pair, seed, n):
    """ops.resample of signal(seed, n) as one call of its own -> numpy"""
    from avse_amd import ops
    return ops.resample([ops.to_device(signal(seed, n))], *pair)[0].cpu().numpy()


def same_bits(a, b):
    a, b = torch.as_tensor(a).contiguous(), torch.as_tensor(b).contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. one-shot parity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", sorted(ONE_SHOT))
def test_one_shot_matches_the_reference(gpu, r):
    from avse_amd import ops
    up, down = r
    pair = ONE_SHOT[r]
    assert ratio(*pair) == r
    T = taps_per_output(up, down)
    lengths = [0, 1, T - 1, T, T + 1, 4999]
    sigs = [signal(100 + i, n) for i, n in enumerate(lengths)]
    got = ops.resample([ops.to_device(s) for s in sigs], *pair)      # one ragged call
    assert len(got) == len(sigs)
    for n, x, y in zip(lengths, sigs, got):
        ref = eval_ref.resample(x, up, down)
        y = y.cpu().numpy()
        assert y.shape == ref.shape == (-(-n * up // down),)
        assert ops.resample_counts(*pair, n, True) == ref.size
        if n == 0:
            continue
        err, peak = np.abs(y.astype(np.float64) - ref).max(), np.abs(ref).max()
        print(f"{up}/{down} n={n}: max |y - ref| {err:.3e} = {err / peak:.3e} of the peak {peak:.1f} (gate 2^-23 = 1.19e-07)")
        assert err <= 2.0 ** -23 * peak, (r, n, err, peak)
    # the [U, n] form: the same bits per row
    x2 = np.stack([signal(7, 700), signal(8, 700)])
    y2 = ops.resample(ops.to_device(x2), *pair)
    assert y2.shape == (2, -(-700 * up // down))
    for u in range(2):
        assert same_bits(y2[u].cpu(), whole(pair, 7 + u, 700))


# ---- 2. cut invariance -----------------------------------------------------------------------------------------
def stream_all(rs, pair, xs, schedule):
    """Runs `schedule` (a list of calls, each a list of (n_new, flush) per stream) on resampler rs, checking host_n_out
    against the differences of resample_counts at every step -> the concatenated outputs per stream (numpy)."""
    from avse_amd import ops
    B = len(xs)
    xd = [ops.to_device(x) for x in xs]
    pos, done, outs = [0] * B, [0] * B, [[] for _ in range(B)]
    for call in schedule:
        parts = [xd[b][pos[b]:pos[b] + n] if n else None for b, (n, _) in enumerate(call)]
        got = ops.resampler_push_each(rs, parts, [fl for _, fl in call])
        for b, (n, fl) in enumerate(call):
            pos[b] += n
            total = ops.resample_counts(*pair, pos[b], fl or rs.fl[b])
            assert got[b].numel() == total - done[b], (b, call)
            done[b] = total
            outs[b].append(got[b])
    assert ops.resampler_state(rs) == (pos, done, [True] * B)
    return [torch.cat(o).cpu() for o in outs]


@pytest.mark.parametrize("pair", STREAMED)
def test_output_does_not_depend_on_the_cuts(gpu, pair):
    from avse_amd import ops
    up, down = ratio(*pair)
    T = taps_per_output(up, down)
    B = 3
    n = [60 + (T - 1) + T + 997 + 1500, 2600, 3 * T + 11]
    xs = [signal(20 + b, n[b]) for b in range(B)]
    want = [whole(pair, 20 + b, n[b]) for b in range(B)]
    rs = ops.resampler_create(B, *pair)
    # stream 0: sixty 1-sample pushes, then T - 1, T, a zero-length push, 997, the rest; flushed in a call of its own
    # stream 1: idle in most calls, everything in one push, flushed with that push
    # stream 2: pushed in two parts late, flushed last
    idle = (0, False)
    sched = [[(1, False), idle, idle] for _ in range(60)]
    sched += [[(T - 1, False), idle, idle], [(T, False), (n[1], True), idle], [(0, False), idle, (T + 5, False)],
              [(997, False), idle, idle], [(1500, False), idle, (n[2] - T - 5, False)], [(0, True), idle, idle],
              [idle, idle, (0, True)]]
    got = stream_all(rs, pair, xs, sched)
    for b in range(B):
        assert same_bits(got[b], want[b]), (pair, b)
    # slots reset and reused: stream 1's slot now takes stream 2's signal in one push, the others stay flushed
    ops.resampler_reset_each(rs, [1])
    assert ops.resampler_state(rs)[0][1] == 0 and not rs.fl[1] and rs.fl[0]
    again = ops.resampler_push_each(rs, [None, ops.to_device(xs[2]), None], [False, True, False])
    assert again[0].numel() == 0 and again[2].numel() == 0
    assert same_bits(again[1].cpu(), want[2])
    # all slots back; one push of everything for every stream
    ops.resampler_reset_each(rs)
    once = ops.resampler_push_each(rs, [ops.to_device(x) for x in xs], [True] * B)
    for b in range(B):
        assert same_bits(once[b].cpu(), want[b]), (pair, b)


# ---- 3. refusals -----------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_streams_as_they_were(gpu):
    from avse_amd import _lib, ops
    pair = (44100, 16000)
    B = 2
    xs = [signal(30 + b, 2000) for b in range(B)]
    want = [whole(pair, 30 + b, 2000) for b in range(B)]
    xd = [ops.to_device(x) for x in xs]
    rs = ops.resampler_create(B, *pair)
    outs = [[], []]

    def push(parts, flush, **kw):
        for b, o in enumerate(ops.resampler_push_each(rs, parts, flush, **kw)):
            outs[b].append(o)

    push([xd[0][:900], xd[1][:1000]], [False, True])
    state = ops.resampler_state(rs)
    need = max(ops.resample_counts(*pair, 2000) - ops.resample_counts(*pair, 900), 0)
    with pytest.raises(_lib.AvseError, match="stream 0: .*out_stride"):
        ops.resampler_push_each(rs, [xd[0][900:], None], [False, False], out_stride=need - 1)
    with pytest.raises(_lib.AvseError, match="stream 1: .*after its flush"):
        ops.resampler_push_each(rs, [xd[0][900:], xd[1][1000:]], [False, False])
    with pytest.raises(_lib.AvseError, match="stream 1: .*after its flush"):
        ops.resampler_push_each(rs, [None, None], [False, True])
    assert ops.resampler_state(rs) == state and (rs.ns, rs.outs, rs.fl) == state
    push([xd[0][900:], None], [True, False], out_stride=need + 200)
    assert same_bits(torch.cat(outs[0]).cpu(), want[0])
    assert same_bits(torch.cat(outs[1]).cpu(), ops.resample([xd[1][:1000].contiguous()], *pair)[0].cpu())
    assert want[1].size > torch.cat(outs[1]).numel()
    # unsupported pairs and bad stream counts at create
    with pytest.raises(_lib.AvseError, match="16000 / 16001"):
        ops.resampler_create(1, 16001, 16000)
    with pytest.raises(_lib.AvseError):
        ops.resampler_create(1025, 44100, 16000)
    with pytest.raises(_lib.AvseError, match="16000 / 16001"):
        ops.resample([xd[0]], 16001, 16000)


# ---- 4. equal rates --------------------------------------------------------------------------------------------
def test_equal_rates_copy_the_bits(gpu):
    from avse_amd import ops
    x = signal(40, 777).copy()
    x[:4] = [-0.0, 0.0, np.float32(1e-42), -32768.0]        # a negative zero and a denormal keep their bits
    xd = ops.to_device(x)
    assert same_bits(ops.resample([xd], 16000, 16000)[0].cpu(), x)
    assert same_bits(ops.resample(xd.view(1, -1), 48000, 48000)[0].cpu(), x)
    rs = ops.resampler_create(1, 24000, 24000)
    a = ops.resampler_push_each(rs, [xd[:300]])[0]
    b = ops.resampler_push_each(rs, [xd[300:]], [True])[0]
    assert a.numel() == 300 and same_bits(torch.cat([a, b]).cpu(), x)


# ---- 5. interleaved use ----------------------------------------------------------------------------------------
def test_two_resamplers_and_a_session_on_one_context(gpu):
    """Two resamplers and a 16 kHz session used alternately: each gives the bits it gives alone (the one-shot call's for
    the resamplers, whose taps and rows a neighbour's call must not disturb)."""
    from avse_amd import ops
    from avse_amd.pipeline import StreamEnhancer
    from test_gpu_streaming import inputs, run_stream, weights
    x, video = inputs()[0][:1], inputs()[1][:1]
    alone = run_stream(StreamEnhancer(weights("float32_split"), 1), x, video, [3200] * 4, video_at=[1] * 4)
    down, up = (44100, 16000), (16000, 44100)
    xs = {down: signal(50, 4000), up: signal(51, 1500)}
    want = {p: whole(p, 50 + i, xs[p].size) for i, p in enumerate((down, up))}
    rs = {p: ops.resampler_create(1, *p) for p in (down, up)}
    xd = {p: ops.to_device(xs[p]) for p in (down, up)}
    outs = {down: [], up: []}
    enh = StreamEnhancer(weights("float32_split"), 1)
    _, _, m0, s0, _ = inputs()
    mean, std = ops.to_device(m0), ops.to_device(s0)
    sx, sv = ops.to_device(x), ops.video_to_device(video)
    sess = []
    for i in range(4):
        for p in (down, up):
            q = xs[p].size // 4
            part = xd[p][i * q:(i + 1) * q if i < 3 else None]
            outs[p].append(ops.resampler_push_each(rs[p], [part], [i == 3])[0])
        sess.append(enh.push(sx[:, 3200 * i:3200 * (i + 1)].contiguous(), sv[:, i:i + 1].contiguous(), mean, std))
        ops.resample([xd[down][:500].contiguous()], 11025, 16000)       # a third ratio through the context's cache
    sess.append(enh.flush(mean, std))
    for p in (down, up):
        assert same_bits(torch.cat(outs[p]).cpu(), want[p]), p
    assert same_bits(torch.cat(sess, dim=1).cpu(), alone["out"])
