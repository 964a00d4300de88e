"""The sliding streaming session (pipeline.SlidingStreamEnhancer, avse_slide_*) against the float64
reference tests/slide_ref.py, against the existing session (stride F), and against itself under other cuts.

Shapes: B <= 3 streams of 12,800 samples and 20 video frames at 16 kHz (test_gpu_streaming's utterances and video, the
video taken frame by frame).  Twenty frames hold every transition: window 0, windows that straddle two slots of the mel
ring, several windows in one push, the frame left over at stride 2, and the flush."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import slide_ref
from test_gpu_pipeline import MEL_BF16, WAVE_BF16, rel_rms
from test_gpu_stft import DB_MAX, DB_RMS
from test_gpu_streaming import inputs, run_stream, same_bits, tone_utterance, weights

pytestmark = pytest.mark.gpu

L, NF = 12800, 20
KEYS = ("out", "mel", "pred")


def as_frames(video):
    """[.., S, 128, 128, F] slices -> [.., S * F, 128, 128] frames: frame F k + i is video[.., k, :, :, i]."""
    v = np.moveaxis(video, -1, -3)
    return np.ascontiguousarray(v).reshape(video.shape[:-4] + (video.shape[-4] * video.shape[-1], 128, 128))


@functools.lru_cache(None)
def frames():
    """[3, 20, 128, 128]: the video of test_gpu_streaming.inputs(), frame by frame."""
    return as_frames(inputs()[1])


@functools.lru_cache(None)
def reference(which, stride):
    """slide_ref of utterance `which` (0..2, "tone": the quiet-tone utterance with utterance 0's video, "short":
    utterance 0 cut by 700 samples) at `stride`: made once, shared, read only."""
    x, _, mean, std, model = inputs()
    u = which if isinstance(which, int) else 0
    sig = {"tone": tone_utterance(), "short": x[0][:L - 700]}.get(which, x[u])
    return slide_ref.slide_reference(sig, frames()[u], mean, std, model.layer_dict(), stride)


def run_slide(enh, x, vid, pushes, frames_at, flush=True, mean=None, std=None):
    """Feeds x [B, n] in `pushes` and the frames vid [B, f, 128, 128] by `frames_at` (frames delivered with each push),
    lock-step -> dict(out [B, emitted], mel / pred [B, windows, 80, spf], n_out and windows per call)."""
    from avse_amd import ops
    m0, s0 = inputs()[2], inputs()[3]
    mean, std = ops.to_device(m0 if mean is None else mean), ops.to_device(s0 if std is None else std)
    xd, vd = ops.to_device(x), ops.video_to_device(vid)
    outs, mels, preds, n_outs, ws = [], [], [], [], []
    a = va = 0

    def keep(res):
        o, m, q = res
        outs.append(o); mels.append(m); preds.append(q); n_outs.append(o.shape[1]); ws.append(m.shape[1])
    for p, nf in zip(pushes, frames_at):
        keep(enh.push(xd[:, a:a + p].contiguous() if p else None, vd[:, va:va + nf].contiguous() if nf else None, mean, std,
                      return_spectrograms=True))
        a, va = a + p, va + nf
    if flush:
        keep(enh.flush(mean, std, return_spectrograms=True))
    cat = lambda ts: torch.cat(ts, dim=1).cpu().numpy()
    return dict(out=cat(outs), mel=cat(mels), pred=cat(preds), n_out=n_outs, windows=ws)


def expected_calls(enh, pushes, frames_at, flush=True):
    """(samples, windows) each call emits / completes, from the host totals."""
    from avse_amd import ops
    n = f = 0
    prev = (0, 0, 0, 0)
    es, ws = [], []
    steps = [(p, nf, False) for p, nf in zip(pushes, frames_at)] + ([(0, 0, True)] if flush else [])
    for p, nf, fl in steps:
        n, f = n + p, f + nf
        c = ops.slide_counts(n, f, fl, session=enh.session)
        es.append(c[3] - prev[3]); ws.append(c[1] - prev[1])
        prev = c
    return es, ws


def check_against_reference(got, ref, dtype, label, gate_pred=True):
    """mel_db within DB_MAX / DB_RMS, pred_db and the waveform within the project's gates for `dtype`."""
    d = got["mel"].astype(np.float64) - ref["mel"]
    dmax, drms = np.abs(d).max(), np.sqrt(np.mean(d ** 2))
    err, perr = rel_rms(got["out"], ref["wave"]), rel_rms(got["pred"], ref["pred"])
    print(f"{label}: mel_db max {dmax:.2e} dB, RMS {drms:.2e} dB; predicted mel-dB rel RMS {perr:.3e}; waveform rel RMS "
          f"{err:.3e} vs slide_ref")
    assert dmax <= DB_MAX and drms <= DB_RMS, (label, dmax, drms)
    assert err <= (WAVE_BF16 if dtype == "bfloat16" else 1e-4), (label, err)
    if gate_pred:
        assert perr <= (MEL_BF16 if dtype == "bfloat16" else 1e-4), (label, perr)


def enhancer(dtype, B, stride, **kw):
    from avse_amd.pipeline import SlidingStreamEnhancer
    return SlidingStreamEnhancer(weights(dtype), B, stride=stride, **kw)


# ---- 1. oracle parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype,video_u8", [("float32", False), ("float32_split", False), ("bfloat16", False),
                                            ("float32_split", True)])
def test_slide_matches_the_reference(gpu, dtype, video_u8, stride):
    B = 2
    x, vid = inputs()[0][:B], frames()[:B]
    ticks = ([640] * NF, [1] * NF)
    enh = enhancer(dtype, B, stride)
    got = run_slide(enh, x, vid, *ticks)
    if video_u8:            # the crops' own bytes: the float32-video run's bits
        got8 = run_slide(enhancer(dtype, B, stride, video_dtype=torch.uint8), x, vid.astype(np.uint8), *ticks)
        for key in KEYS:
            assert same_bits(got[key], got8[key]), key
        got = got8
    es, ws = expected_calls(enh, *ticks)
    assert got["n_out"] == es and got["windows"] == ws
    if stride == 1:
        assert sum(ws) == 16 and got["out"].shape == (B, 12640) and got["mel"].shape == got["pred"].shape == (B, 16, 80, 20)
        assert ws[:5] == [0, 0, 0, 0, 0] and ws[5:] == [1] * 15 + [1]      # window j with frame j + 4; the flush's last
    else:
        assert sum(ws) == 8 and got["out"].shape == (B, 12000) and sum(es[:-1]) == 11840
        assert enh.counts["predicted"] == 76 and enh.counts["windows"] == 8
        assert ws[-1] == 0                       # the flush completes no window: frame 19 is past the last full stride
    assert np.isfinite(got["out"]).all()
    for u in ([0] if stride == 1 else [0, 1]):
        check_against_reference({k: got[k][u] for k in KEYS}, reference(u, stride), dtype, f"{dtype} stride {stride} stream {u}")
    if dtype == "float32_split":
        assert enh.range_bits == 0


# ---- 2. stride F is the existing session -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32_split", "bfloat16"])
def test_stride_F_is_the_existing_session_bit_for_bit(gpu, dtype):
    from avse_amd.pipeline import StreamEnhancer
    B = 2
    x, video = inputs()[0][:B], inputs()[1][:B]
    for pushes, slices_at in (([3200] * 4, [1] * 4), ([321, 7, 5000, 7472], [2, 0, 1, 1])):
        plain = run_stream(StreamEnhancer(weights(dtype), B), x, video, pushes, slices_at)
        slid = run_slide(enhancer(dtype, B, 5), x, frames()[:B], pushes, [5 * v for v in slices_at])
        assert slid["n_out"] == plain["n_out"]
        for key in KEYS:
            assert same_bits(slid[key], plain[key]), (pushes, key)


# ---- 3. cutting invariance -------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
def test_output_does_not_depend_on_how_the_input_was_cut(gpu, stride):
    B = 2
    x, vid = inputs()[0][:B], frames()[:B]
    enh = enhancer("float32_split", B, stride, max_windows=16)
    cases = [("one push", [L], [NF]),
             ("a tick per video frame", [640] * NF, [1] * NF),
             ("1000-sample pushes, all video first", [1000] * 12 + [800], [NF] + [0] * 12),
             ("odd pushes, video two frames late", [321, 7, 5000, 7472, 0], [0, 0, 6, 12, 2]),
             ("video frame by frame after all samples", [L] + [0] * NF, [0] + [1] * NF)]
    first = None
    for name, pushes, frames_at in cases:
        enh.reset()
        got = run_slide(enh, x, vid, pushes, frames_at)
        es, ws = expected_calls(enh, pushes, frames_at)
        assert got["n_out"] == es and got["windows"] == ws, name
        assert got["out"].shape == (B, 12640), name
        if first is None:
            first = got
        for key in KEYS:
            assert same_bits(first[key], got[key]), (name, key)
    assert first["mel"].shape == (B, 16 if stride == 1 else 6, 80, 20)
    if stride == 1:
        assert rel_rms(first["out"][0], reference(0, 1)["wave"]) <= 1e-4


# ---- 4. independent streams ------------------------------------------------------------------------------------
def test_streams_are_independent(gpu):
    """A B = 3 session driven by push_each: caller A ticks frame by frame; caller C holds a slot for half an utterance
    and hangs up; caller Bc joins late and moves two frames at a time; caller D takes C's slot.  Each gets the bits of a
    B = 1 session fed the same input."""
    from avse_amd import ops
    x, _, mean, std, _ = inputs()
    md, sd = ops.to_device(mean), ops.to_device(std)
    xd, vd = ops.to_device(x), ops.video_to_device(frames())
    dw = weights("float32_split")
    enh = enhancer("float32_split", 3, 1)
    callers = {      # name: (samples, frames, video frames per tick, first tick)
        "A": (xd[0], vd[0], 1, 0), "C": (xd[2, :6400], vd[2, :10], 1, 0), "Bc": (xd[1], vd[1], 2, 5),
        "D": (xd[2, 6400:], vd[2, 10:], 5, 12)}
    slot, pos, got, slots_seen = {}, {k: 0 for k in callers}, {k: [[], [], []] for k in callers}, {}
    for tick in range(20):
        for name, (_, _, _, start) in callers.items():
            if tick == start:
                slot[name] = slots_seen[name] = enh.open()
        samples, video = [None] * 3, [None] * 3
        for name, b in slot.items():
            sig, vid, k, _ = callers[name]
            a = pos[name]
            samples[b], video[b] = sig[640 * a:640 * (a + k)].contiguous(), vid[a:a + k].contiguous()
            pos[name] = a + k
        res = enh.push_each(samples, video, None, md, sd, return_spectrograms=True)
        for name, b in list(slot.items()):
            for i in range(3):
                got[name][i].append(res[i][b])
            if pos[name] == callers[name][1].shape[0]:      # the caller hangs up: its flush, and the slot is free again
                last = enh.close(b, md, sd, return_spectrograms=True)
                for i in range(3):
                    got[name][i].append(last[i])
                del slot[name]
    assert not slot and slots_seen == {"A": 0, "C": 1, "Bc": 2, "D": 1}      # D took the slot C left
    assert enh.session.ns == [0, 0, 0] and ops.slide_state(enh.session) == ([0] * 3, [0] * 3, [False] * 3)
    for name, (sig, vid, _, _) in callers.items():
        alone = enhancer("float32_split", 1, 1, max_windows=16)
        a = alone.push_each([sig.contiguous()], [vid.contiguous()], [True], md, sd, return_spectrograms=True)
        for i, key in enumerate(KEYS):
            mine = torch.cat(got[name][i]).cpu().numpy()
            assert mine.shape[0] > 0 and same_bits(mine, a[i][0].cpu().numpy()), (name, key)
    assert dw.ctx.range_status() == 0


# ---- 5. the causal floor ---------------------------------------------------------------------------------------
def test_floor_is_causal_per_window(gpu):
    x, vid = tone_utterance()[None], frames()[:1]
    ref = reference("tone", 1)
    un, floors = ref["unclamped"], ref["floors"]
    raised0 = float(np.mean(ref["mel"][0] != un[:, :20]))
    print(f"reference: the floor raises {100 * raised0:.1f} % of window 0 (by up to {(ref['mel'][0] - un[:, :20]).max():.1f} dB); "
          f"floors of windows 0 / 1 / 15: {floors[0]:.1f} / {floors[1]:.1f} / {floors[15]:.1f} dB")
    assert raised0 > 0.5 and (ref["mel"][0] - un[:, :20]).max() > 1.0       # the floor binds in window 0
    assert floors[1] - floors[0] > 1.0 and np.all(np.diff(floors) >= 0)     # and moves between windows
    # window 1 at window 0's floor (a clamp that does not move) is another input
    assert np.abs(np.maximum(un[:, 4:24], floors[0]) - ref["mel"][1]).max() > 1.0
    got = run_slide(enhancer("float32_split", 1, 1), x, vid, [640] * NF, [1] * NF)
    mel = got["mel"][0]
    assert np.abs(mel[0] - un[:, :20]).max() > 1.0 and np.abs(mel[1] - np.maximum(un[:, 4:24], floors[0])).max() > 1.0
    check_against_reference({k: got[k][0] for k in KEYS}, ref, "float32_split", "tone utterance, stride 1")


# ---- 6. a short flush, and the refusals ------------------------------------------------------------------------
def test_flush_pads_with_zeros(gpu):
    x, vid = inputs()[0][:1], frames()[:1]
    enh = enhancer("float32_split", 1, 1)
    short = run_slide(enh, x[:, :L - 700], vid, [640] * 18 + [580, 0], [1] * NF)
    enh.reset()
    padded = np.concatenate([x[:, :L - 700], np.zeros((1, 700), np.float32)], axis=1)
    full = run_slide(enh, padded, vid, [640] * NF, [1] * NF)
    assert short["out"].shape == (1, 12640)
    for key in KEYS:
        assert same_bits(short[key], full[key]), key
    assert rel_rms(short["out"][0], reference("short", 1)["wave"]) <= 1e-4


def test_refusals_leave_the_session_as_it_was(gpu):
    from avse_amd import _lib, ops
    x, vid = inputs()[0][:1], frames()[:1]
    mean, std = inputs()[2], inputs()[3]
    md, sd = ops.to_device(mean), ops.to_device(std)
    xd, vd = ops.to_device(x), ops.video_to_device(vid)
    lib = _lib.load()
    enh = enhancer("float32_split", 1, 1, max_windows=2)
    outs = [enh.push(xd[:, :3200].contiguous(), vd[:, :5].contiguous(), md, sd)]      # 19 frames: no window yet
    assert outs[0].shape == (1, 0)
    state = ([3200], [5], [False])
    assert ops.slide_state(enh.session) == state
    h, st = enh.session.handle, _lib.stream_handle(xd.device)
    buf = torch.empty((1, 8000), dtype=torch.float32, device=xd.device)
    n_out = np.full(1, -7, np.int64)
    zero = np.zeros(1, np.int64)

    def push(n_new, f_new, out=buf, out_stride=8000, flush=0):
        samples = xd[:, 3200:3200 + n_new].contiguous() if n_new else None
        video = vd[:, 5:5 + f_new].contiguous() if f_new else None
        n, f, fl = np.array([n_new], np.int64), np.array([f_new], np.int64), np.array([flush], np.uint8)
        rc = lib.avse_slide_push_each(h, _lib.ptr(samples), ctypes.c_void_p(zero.ctypes.data), ctypes.c_void_p(n.ctypes.data),
                                      _lib.ptr(video), ctypes.c_void_p(f.ctypes.data), ctypes.c_void_p(fl.ctypes.data),
                                      _lib.ptr(md), _lib.ptr(sd), _lib.ptr(out), out_stride, ctypes.c_void_p(n_out.ctypes.data),
                                      None, None, None, st)
        return rc, lib.avse_last_error().decode()
    refused = [
        (push(160, 0, out_stride=2879), "out_stride"),             # window 0 completes: the call emits 2880 samples
        (push(160, 0, out=None), "out_stride"),
        (push(1920, 3), "more than max_windows windows"),          # three windows in one call
        (push(2080, 0), "ahead of the video"),                     # the samples complete windows 0 .. 3, the video 0
        (push(0, 4), "ahead of the samples"),                      # the video completes five windows, the samples none
        (push(100, 0, flush=1), "flush"),                          # n = 3300 > hop q f = 3200
        (push(-1, 0), "negative"),
    ]
    for (rc, why), word in refused:
        assert rc == 1 and word in why and why.startswith("stream 0: "), (word, why)
    assert n_out[0] == -7                                          # no refused call wrote its count
    assert ops.slide_state(enh.session) == state
    # the refused calls left no trace: the rest of the stream is the bits of a run without them
    outs.append(enh.push(xd[:, 3200:3840].contiguous(), vd[:, 5:6].contiguous(), md, sd))
    for k in range(6, NF):
        outs.append(enh.push(xd[:, 640 * k:640 * k + 640].contiguous(), vd[:, k:k + 1].contiguous(), md, sd))
    outs.append(enh.flush(md, sd))
    assert ops.slide_state(enh.session) == ([L], [NF], [True])
    for n_new, f_new, flush in ((160, 0, 0), (0, 1, 0), (0, 0, 1)):      # after the flush only a reset is legal
        rc, why = push(n_new, f_new, flush=flush)
        assert rc == 1 and "after its flush" in why
    with pytest.raises(_lib.AvseError, match="flush after flush"):
        enh.flush(md, sd)
    assert ops.slide_state(enh.session) == ([L], [NF], [True])
    clean = run_slide(enhancer("float32_split", 1, 1), x, vid, [640] * NF, [1] * NF)
    assert same_bits(torch.cat(outs, dim=1).cpu().numpy(), clean["out"])
    # geometry refusals that need real weights: a stride past F, and weights of another shape
    with pytest.raises(_lib.AvseError, match="status 1"):
        enhancer("float32_split", 1, 6)
    out = ctypes.c_void_p()
    dw = weights("float32_split")
    rc = lib.avse_slide_create(dw.ctx.handle, dw.handle, 1, 24000, 800, 200, 24, 1, 80, 0.0, 8000.0, 1e-5, 80.0, 0, 4,
                               ctypes.byref(out))
    assert rc != 0 and not out.value                               # [80, 20] x 5-frame weights at the 30-fps geometry
    assert enh.range_bits == 0


# ---- 7. the other frame families -------------------------------------------------------------------------------
def family_reference(sr, stride, x, vid, mean, std, model, n_fft, hop, spf):
    return slide_ref.slide_reference(x, vid, mean, std, model.layer_dict(), stride, sr=sr, n_fft=n_fft, hop=hop, spf=spf)


def test_three_phase_frames_at_48_khz(gpu):
    """48 kHz / 25 fps: the three-phase 640-point frames (frame_poly.h), stride 1, a tick per video frame."""
    import test_gpu_stream_rates as rates
    from avse_amd.pipeline import SlidingStreamEnhancer
    _, _, mean, std, model = inputs()
    x, vid = rates.audio(48000)[:1], frames()[:1]
    enh = SlidingStreamEnhancer(weights("float32_split"), 1, stride=1, sample_rate=48000)
    got = run_slide(enh, x, vid, [1920] * NF, [1] * NF)
    assert got["out"].shape == (1, 38400 - 480) and got["mel"].shape == (1, 16, 80, 20)
    assert enh.latency_samples == 4 * 480 + 960 + 480
    ref = family_reference(48000, 1, x[0], vid[0], mean, std, model, 1920, 480, 20)
    check_against_reference({k: got[k][0] for k in KEYS}, ref, "float32_split", "48 kHz stride 1", gate_pred=False)


@pytest.mark.parametrize("stride", [1, 2])
def test_800_point_frames_at_30_fps(gpu, stride):
    """24 kHz / 30 fps with the [80, 24] x 6-frame weights (frame800.h), a tick per video frame."""
    import test_gpu_stream_fps30 as fps30
    from avse_amd.pipeline import SlidingStreamEnhancer
    video, mean, std, model = fps30.inputs()
    x, vid = fps30.audio(24000)[:1], as_frames(video)[:1]
    assert vid.shape == (1, 24, 128, 128)
    enh = SlidingStreamEnhancer(fps30.weights("float32_split"), 1, stride=stride, video_frame_rate=30.0, sample_rate=24000)
    got = run_slide(enh, x, vid, [800] * 24, [1] * 24, mean=mean, std=std)
    windows = (24 - 6) // stride + 1
    predicted = 24 + 4 * stride * (windows - 1)
    assert got["mel"].shape == (1, windows, 80, 24) and got["out"].shape == (1, 200 * (predicted - 1))
    ref = family_reference(24000, stride, x[0], vid[0], mean, std, model, 800, 200, 24)
    check_against_reference({k: got[k][0] for k in KEYS}, ref, "float32_split", f"24 kHz 30 fps stride {stride}",
                            gate_pred=False)


# ---- 8. reported, not gated: the composed offline ops, bit for bit ----------------------------------------------
def test_report_bit_equality_with_the_offline_ops(gpu):
    from avse_amd import ops
    x, vid = inputs()[0][:1], frames()[:1]
    mean, std = inputs()[2], inputs()[3]
    dw = weights("float32_split")
    got = run_slide(enhancer("float32_split", 1, 1), x, vid, [640] * NF, [1] * NF)
    xd = ops.to_device(x)
    un, stft = ops.spectrogram(xd, top_db=None, return_stft=True)                 # [1, 80, 81] unclamped
    wins = torch.stack([torch.maximum(un[0, :, 4 * j:4 * j + 20], un[0, :, :4 * j + 20].max() - 80.0) for j in range(16)])
    print(f"window inputs == ops.spectrogram(top_db=None) clamped in torch: {same_bits(got['mel'][0], wins.cpu().numpy())}")
    vd = ops.video_to_device(vid)[0]
    clips = torch.stack([vd[j:j + 5].permute(1, 2, 0) for j in range(16)]).contiguous()
    pred = ops.forward(dw, ops.to_device(got["mel"][0]), clips, ops.to_device(mean), ops.to_device(std))
    print(f"pred_db == ops.forward on the same windows: {same_bits(got['pred'][0], pred.cpu().numpy())}")
    kept = torch.cat([pred[0]] + [pred[j][:, 16:] for j in range(1, 16)], dim=1)[None].contiguous()      # [1, 80, 80]
    with dw.ctx.options(dense_istft=1):
        dense = ops.istft(kept, stft).cpu().numpy()
    print(f"waveform == ops.istft (dense_istft) on the kept columns: {same_bits(got['out'], dense)}")
    assert got["out"].shape == dense.shape == (1, 12640)
