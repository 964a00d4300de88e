"""Streaming enhancement (pipeline.StreamEnhancer, avse_stream_*) against the oracle pipeline and
against the offline path.

Shapes: B <= 3 streams of S = 4 slices (12,800 samples): every state transition of a session (frame 0's reflection, a
partial slice carried over a push, several slices completed by one push, video ahead of the samples and behind them, the
flush's zero padding and right reflection) happens within four slices.

Oracles (float64, oracle/librosa_ref.py + oracle/keras_ref.py):
  offline  R.preprocess_audio_signal -> K.forward -> R.reconstruct_speech_signal, the gate of
           tests/test_gpu_pipeline.py::test_enhancer_matches_oracle_pipeline (relative RMS 1e-4 for float32 and
           float32_split; its MEL_BF16 / WAVE_BF16 for bfloat16);
  causal   the same with slice k clamped at (the maximum of the unclamped mel-dB of frames 0 .. 20 k + 19) - 80 dB
           instead of the whole utterance's maximum - 80 dB: what a stream computes.  The two are the same arrays
           wherever the unclamped range of the utterance is below 80 dB, which test 1 asserts of its inputs first."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import synth_audio, synth_video
from oracle import keras_ref as K
from oracle import librosa_ref as R
from test_gpu_pipeline import MEL_BF16, WAVE_BF16, rel_rms
from test_gpu_stft import DB_MAX, DB_RMS

pytestmark = pytest.mark.gpu

S, L = 4, 12800
PATTERNS = {"slices": [3200] * 4, "aligned": [3360, 3200, 3200, 3040], "whole": [12800], "small": [1000] * 12 + [800],
            "odd": [321, 7, 5000, 7472]}


@functools.lru_cache(None)
def inputs():
    """Three utterances and their video, the normaliser, the model: made once; the tests only read them."""
    from avse_amd.model import KerasModel
    rng = np.random.default_rng(5)
    x = synth_audio(rng, 3, L)
    video = synth_video(rng, 3 * S).reshape(3, S, 128, 128, 5)
    mean, std = R.video_normalizer_fit(video.reshape(3 * S, 128, 128, 5))
    return x, video, mean, std, KerasModel.init(seed=8, randomize=True)


@functools.lru_cache(None)
def weights(dtype):
    from avse_amd import ops
    return ops.DeviceWeights(inputs()[4], dtype)


def tone_utterance():
    """x2 of the causal-floor test: utterance 0 with its first slice replaced by a quiet 440-Hz tone."""
    x2 = inputs()[0][0].copy()
    x2[:3200] = np.round(2 * np.sin(2 * np.pi * 440 * np.arange(3200) / 16000.0))
    return x2


@functools.lru_cache(None)
def oracle(which, causal=False):
    """which: 0..2 (utterance u), "tone" (x2 with utterance 0's video), "short" (utterance 0 cut by 700 samples).
    -> dict(unclamped [80, 81], mel [S, 80, 20] as the network sees it, pred [S, 80, 20], wave [12640])."""
    x, video, mean, std, model = inputs()
    u = which if isinstance(which, int) else 0
    sig = {"tone": tone_utterance(), "short": x[0][:L - 700]}.get(which, x[u])
    sig = R.fit_length(sig, L)
    D = R.stft(sig, n_fft=640, hop_length=160)
    mag, phase = R.magphase(D)
    un = R.amplitude_to_db(np.dot(R.mel_filterbank(16000, 640, n_mels=80, fmin=0, fmax=8000), mag), top_db=None)
    if causal:
        mel = np.stack([np.maximum(un[:, 20 * k:20 * k + 20], un[:, :20 * k + 20].max() - 80.0) for k in range(S)])
    else:
        mel = R.preprocess_audio_signal(sig, 16000, 200, S, 25.0)
    vn = R.video_normalize(video[u], mean, std).astype(np.float32)
    pred = K.forward(model.layer_dict(), mel.astype(np.float32), vn)
    if causal:
        wave = R.reconstruct_signal_from_spectrogram(np.concatenate(list(pred.astype(np.float32)), axis=1),
                                                     phase[:, :20 * S], 16000, 640, 160)
    else:
        wave = R.reconstruct_speech_signal(sig, 16000, pred.astype(np.float32), 25.0)
    return dict(unclamped=un, mel=mel, pred=pred, wave=wave)


def run_stream(enh, x, video, pushes, video_at=None, flush=True, mean=None, std=None):
    """Feeds x [B, n] in `pushes` and video [B, S, ...] by `video_at` (slices delivered with each push; default all
    with the first) -> dict(out [B, emitted], mel / pred [B, slices, 80, 20], n_out per call, the flush's last)."""
    from avse_amd import ops
    _, _, m0, s0, _ = inputs()
    mean, std = ops.to_device(m0 if mean is None else mean), ops.to_device(s0 if std is None else std)
    xd = ops.to_device(x)
    vd = ops.video_to_device(video)
    video_at = [video.shape[1]] + [0] * (len(pushes) - 1) if video_at is None else video_at
    outs, mels, preds, n_outs = [], [], [], []
    a = va = 0
    for p, nv in zip(pushes, video_at):
        o, m, q = enh.push(xd[:, a:a + p].contiguous(), vd[:, va:va + nv].contiguous() if nv else None, mean, std,
                           return_spectrograms=True)
        a, va = a + p, va + nv
        outs.append(o); mels.append(m); preds.append(q); n_outs.append(o.shape[1])
    if flush:
        o, m, q = enh.flush(mean, std, return_spectrograms=True)
        outs.append(o); mels.append(m); preds.append(q); n_outs.append(o.shape[1])
    cat = lambda ts: torch.cat(ts, dim=1).cpu().numpy()
    return dict(out=cat(outs), mel=cat(mels), pred=cat(preds), n_out=n_outs)


def expected_n_out(pushes, video_at, flush=True):
    from avse_amd import ops
    n = v = prev = 0
    out = []
    for p, nv in zip(pushes, video_at):
        n, v = n + p, v + nv
        e = ops.stream_counts(n, v)[2]
        out.append(e - prev)
        prev = e
    return out + ([ops.stream_counts(n, v, flushed=True)[2] - prev] if flush else [])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. offline and oracle parity ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,video_u8", [("float32", False), ("float32_split", False), ("bfloat16", False),
                                            ("float32_split", True)])
def test_stream_matches_oracle_and_offline_enhancer(gpu, dtype, video_u8):
    from avse_amd import ops
    from avse_amd.pipeline import Enhancer, StreamEnhancer
    B = 2
    x, video, mean, std, _ = inputs()
    x, video = x[:B], video[:B]
    for u in range(B):      # the precondition of "the stream is the offline result": the floor never binds
        un = oracle(u)["unclamped"]
        print(f"utterance {u}: unclamped mel-dB range {un.max() - un.min():.1f} dB")
        assert un.max() - un.min() < 80.0
    dw = weights(dtype)
    got = run_stream(StreamEnhancer(dw, B), x, video, [3200] * 4, video_at=[1] * 4)
    assert got["out"].shape == (B, 12640) and got["mel"].shape == got["pred"].shape == (B, S, 80, 20)
    assert got["n_out"] == [0, 2880, 3200, 3200, 3360]
    if video_u8:            # the crops' own bytes: the float32-video run's bits
        enh8 = StreamEnhancer(dw, B, video_dtype=torch.uint8)
        got8 = run_stream(enh8, x, video.astype(np.uint8), [3200] * 4, video_at=[1] * 4)
        for key in ("out", "mel", "pred"):
            assert same_bits(got[key], got8[key]), key
        got = got8
    md, sd = ops.to_device(mean), ops.to_device(std)
    off = Enhancer(dw)(ops.to_device(x), ops.to_device(video), md, sd).cpu().numpy()
    wave_gate = WAVE_BF16 if dtype == "bfloat16" else 1e-4
    for u in range(B):
        ref = oracle(u)
        err, perr, eoff = rel_rms(got["out"][u], ref["wave"]), rel_rms(got["pred"][u], ref["pred"]), \
            rel_rms(got["out"][u], off[u])
        print(f"{dtype} stream {u}: waveform rel RMS {err:.3e} vs the oracle, {eoff:.3e} vs the offline Enhancer; "
              f"predicted mel-dB rel RMS {perr:.3e}")
        assert err <= wave_gate and eoff <= wave_gate, (u, err, eoff)
        if dtype == "bfloat16":
            assert perr <= MEL_BF16, (u, perr)
    # reported, not gated: the shared frame code against the offline kernels, bit for bit
    xd = ops.to_device(x)
    mel_off, stft = ops.spectrogram(xd, frames_per_slice=20, return_stft=True)
    print(f"{dtype}: streamed mel_db == ops.spectrogram bits: {same_bits(got['mel'], mel_off.cpu().numpy())}")
    with dw.ctx.options(dense_istft=1):
        dense = ops.istft(ops.to_device(got["pred"]), stft).cpu().numpy()
    print(f"{dtype}: streamed waveform == dense_istft bits on the same pred_db and STFT: {same_bits(got['out'], dense)}")


# ---- 2. chunking invariance ------------------------------------------------------------------------------------
def test_output_does_not_depend_on_how_the_input_was_cut(gpu):
    from avse_amd.pipeline import StreamEnhancer
    B = 2
    x, video = inputs()[0][:B], inputs()[1][:B]
    enh = StreamEnhancer(weights("float32_split"), B)
    cases = [(name, p, [S] + [0] * (len(p) - 1)) for name, p in PATTERNS.items()]
    cases.append(("video two slices late", [3200] * 4, [0, 0, 3, 1]))
    cases.append(("video slice by slice", [1000] * 12 + [800], [1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0]))
    first = None
    for name, pushes, video_at in cases:
        enh.reset()
        got = run_stream(enh, x, video, pushes, video_at)
        assert got["n_out"] == expected_n_out(pushes, video_at), name
        assert got["out"].shape == (B, 12640), name
        if first is None:
            first = got
        for key in ("out", "mel", "pred"):
            assert same_bits(first[key], got[key]), (name, key)
    assert rel_rms(first["out"][0], oracle(0)["wave"]) <= 1e-4


# ---- 3. the causal floor ---------------------------------------------------------------------------------------
def test_floor_is_causal_and_per_stream(gpu):
    from avse_amd.pipeline import StreamEnhancer
    x, video = inputs()[0], inputs()[1]
    xb = np.stack([tone_utterance(), x[0]])
    vb = np.stack([video[0], video[0]])
    causal, offline_mel = oracle("tone", causal=True), R.preprocess_audio_signal(tone_utterance(), 16000, 200, S, 25.0)
    raised = lambda m: float(np.mean(m[0] != causal["unclamped"][:, :20]))
    print(f"oracle: the causal floor raises {100 * raised(causal['mel']):.1f} % of slice 0, the offline clamp "
          f"{100 * raised(offline_mel):.1f} %; they differ by up to {np.abs(causal['mel'] - offline_mel).max():.1f} dB")
    assert raised(causal["mel"]) > 0.5 and np.abs(causal["mel"][0] - offline_mel[0]).max() > 1.0   # the input bites
    dw = weights("float32_split")
    got = run_stream(StreamEnhancer(dw, 2), xb, vb, [3200] * 4, video_at=[1] * 4)
    d = got["mel"][0].astype(np.float64) - causal["mel"]
    print(f"stream mel_db vs the causal oracle: max {np.abs(d).max():.2e} dB, RMS {np.sqrt(np.mean(d ** 2)):.2e} dB")
    assert np.abs(d).max() <= DB_MAX and np.sqrt(np.mean(d ** 2)) <= DB_RMS
    assert np.abs(got["mel"][0][0] - offline_mel[0]).max() > 1.0          # not the offline clamp
    err = rel_rms(got["out"][0], causal["wave"])
    print(f"stream waveform vs the causal oracle pipeline: rel RMS {err:.3e}")
    assert err <= 1e-4
    # floors are per stream: the unmodified utterance beside it is what it is alone
    alone = run_stream(StreamEnhancer(dw, 1), xb[1:], vb[1:], [3200] * 4, video_at=[1] * 4)
    for key in ("out", "mel", "pred"):
        assert same_bits(got[key][1], alone[key][0]), key
    assert rel_rms(got["out"][1], oracle(0)["wave"]) <= 1e-4


# ---- 4. independence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float32_split"])
def test_streams_and_sessions_are_independent(gpu, dtype):
    from avse_amd.pipeline import StreamEnhancer
    x, video = inputs()[0], inputs()[1]
    dw = weights(dtype)
    pushes, video_at = PATTERNS["odd"], [2, 0, 1, 1]
    enh3 = StreamEnhancer(dw, 3)
    all3 = run_stream(enh3, x, video, pushes, video_at)
    single = []
    for b in range(3):
        single.append(run_stream(StreamEnhancer(dw, 1), x[b:b + 1], video[b:b + 1], pushes, video_at))
        for key in ("out", "mel", "pred"):
            assert same_bits(all3[key][b], single[b][key][0]), (b, key)
    # after reset a session reproduces its first run's bits
    enh3.reset()
    again = run_stream(enh3, x, video, pushes, video_at)
    for key in ("out", "mel", "pred"):
        assert same_bits(all3[key], again[key]), key
    # two sessions of one context pushed alternately equal each run alone
    from avse_amd import ops
    _, _, mean, std, _ = inputs()
    md, sd = ops.to_device(mean), ops.to_device(std)
    ea, eb = StreamEnhancer(dw, 1), StreamEnhancer(dw, 1)
    oa, ob = [], []
    xa, xb, va, vb = (ops.to_device(t) for t in (x[0:1], x[1:2], video[0:1], video[1:2]))
    for k in range(S):
        oa.append(ea.push(xa[:, 3200 * k:3200 * k + 3200].contiguous(), va[:, k:k + 1].contiguous(), md, sd))
        ob.append(eb.push(xb[:, 3200 * k:3200 * k + 3200].contiguous(), vb[:, k:k + 1].contiguous(), md, sd))
    oa.append(ea.flush(md, sd))
    ob.append(eb.flush(md, sd))
    assert same_bits(torch.cat(oa, dim=1).cpu().numpy(), single[0]["out"])
    assert same_bits(torch.cat(ob, dim=1).cpu().numpy(), single[1]["out"])


# ---- 5. the flush's padding ------------------------------------------------------------------------------------
def test_flush_pads_with_zeros_like_fit_length(gpu):
    from avse_amd.pipeline import StreamEnhancer
    x, video = inputs()[0][:1], inputs()[1][:1]
    enh = StreamEnhancer(weights("float32_split"), 1)
    short = run_stream(enh, x[:, :L - 700], video, [3200, 3200, 3200, 2500])
    enh.reset()
    padded = np.concatenate([x[:, :L - 700], np.zeros((1, 700), np.float32)], axis=1)
    full = run_stream(enh, padded, video, [3200] * 4)
    assert short["out"].shape == (1, 12640)
    for key in ("out", "mel", "pred"):
        assert same_bits(short[key], full[key]), key
    # (the zeros put frame 78 at the amin floor, 180 dB under the maximum: the clamp binds there, and only there, where
    # the causal floor is the offline one: every louder frame comes earlier)
    err = rel_rms(short["out"][0], oracle("short")["wave"])
    print(f"flush of a stream 700 samples short: waveform rel RMS {err:.3e} vs the oracle on fit_length")
    assert err <= 1e-4
    # the smallest stream: 100 samples (no frame yet, not even frame 0's reflection) and one video slice, then the flush
    enh.reset()
    tiny = run_stream(enh, x[:, :100], video[:, :1], [100], video_at=[1])
    enh.reset()
    padded = np.concatenate([x[:, :100], np.zeros((1, 3100), np.float32)], axis=1)
    full = run_stream(enh, padded, video[:, :1], [3200], video_at=[1])
    assert tiny["n_out"] == [0, 3040] and full["n_out"] == [0, 3040]
    for key in ("out", "mel", "pred"):
        assert same_bits(tiny[key], full[key]), key
    assert np.isfinite(tiny["out"]).all()


# ---- 6. refusals on the device ---------------------------------------------------------------------------------
def test_refusals_leave_the_session_as_it_was(gpu):
    from avse_amd import _lib, ops
    from avse_amd.pipeline import StreamEnhancer
    x, video, mean, std, model = inputs()
    dw = weights("float32_split")
    lib = _lib.load()
    # 29.97 fps: n_fft 533, 24 frames x 133 samples per 3200-sample slice
    h = ctypes.c_void_p()
    rc = lib.avse_stream_create(dw.ctx.handle, dw.handle, 1, 16000, 533, 133, 24, 80, 0.0, 8000.0, 1e-5, 80.0, 0, 4,
                                ctypes.byref(h))
    assert rc == 3 and not h.value
    with pytest.raises(_lib.AvseError, match="status 3"):
        w24 = ops.DeviceWeights(type(model).init(seed=1, audio_shape=(80, 24), video_shape=(128, 128, 5)), "float32")
        StreamEnhancer(w24, 1, video_frame_rate=29.97)
    # weights of another shape than the geometry: AVSE_ERR_INVALID
    rc = lib.avse_stream_create(dw.ctx.handle, dw.handle, 1, 16000, 640, 160, 24, 80, 0.0, 8000.0, 1e-5, 80.0, 0, 4,
                                ctypes.byref(h))
    assert rc == 1 and not h.value
    md, sd = ops.to_device(mean), ops.to_device(std)
    xd, vd = ops.to_device(x[:1]), ops.to_device(video[:1])
    enh = StreamEnhancer(dw, 1, max_slices=1)
    outs = [enh.push(xd[:, :3200].contiguous(), vd[:, :1].contiguous(), md, sd)]
    before = enh.counts
    # straight on the C-ABI (ops always passes the out_stride the call needs): n = 3200, v = 1, no slice done yet
    h, st = enh.session.handle, _lib.stream_handle(xd.device)
    n_out = ctypes.c_int64(-7)
    buf = torch.empty((1, 4000), dtype=torch.float32, device=xd.device)

    def push(samples, n_new, out, out_stride):
        return lib.avse_stream_push(h, _lib.ptr(samples), n_new, n_new, None, 0, _lib.ptr(md), _lib.ptr(sd), _lib.ptr(out),
                                    out_stride, ctypes.byref(n_out), None, None, st)
    assert push(None, 0, None, 0) == 0 and n_out.value == 0       # no samples, no video: legal, and a no-op
    n_out.value = -7
    step = xd[:, 3200:3360].contiguous()                          # completes slice 0: the call emits 2880 samples
    assert push(step, 160, buf, 2879) == 1 and b"out_stride" in lib.avse_last_error()
    assert push(step, 160, None, 4000) == 1 and b"out_stride" in lib.avse_last_error()
    ahead = xd[:, 3200:6500].contiguous()                         # 3300 samples past the one video slice, max_slices 1
    assert push(ahead, 3300, buf, 4000) == 1 and b"ahead of the video" in lib.avse_last_error()
    assert n_out.value == -7                                      # no refused call wrote its count
    with pytest.raises(_lib.AvseError, match="status 1"):         # would complete two slices at once
        enh.push(xd[:, 3200:9600].contiguous(), vd[:, 1:3].contiguous(), md, sd)
    with pytest.raises(_lib.AvseError, match="status 1"):         # two slices of video ahead of the samples
        enh.push(None, vd[:, 1:4].contiguous(), md, sd)
    with pytest.raises(_lib.AvseError, match="status 1"):         # n > 3200 v
        enh.push(xd[:, 3200:3300].contiguous(), None, md, sd)
        enh.flush(md, sd)
    after = enh.counts
    assert after["samples"] == 3300 and after["video_slices"] == 1          # only the accepted 100 samples counted
    assert (after["slices"], after["emitted"]) == (before["slices"], before["emitted"])
    # the refused calls left no trace: the rest of the stream is the bits of a run without them
    outs.append(enh.push(xd[:, 3300:6400].contiguous(), vd[:, 1:2].contiguous(), md, sd))
    for k in (2, 3):
        outs.append(enh.push(xd[:, 3200 * k:3200 * k + 3200].contiguous(), vd[:, k:k + 1].contiguous(), md, sd))
    outs.append(enh.flush(md, sd))
    with pytest.raises(_lib.AvseError, match="status 1"):         # a push after the flush
        enh.push(xd[:, :160].contiguous(), None, md, sd)
    with pytest.raises(_lib.AvseError, match="status 1"):         # and a second flush
        enh.flush(md, sd)
    clean = run_stream(StreamEnhancer(dw, 1), x[:1], video[:1], [3200] * 4, video_at=[1] * 4)
    assert same_bits(torch.cat(outs, dim=1).cpu().numpy(), clean["out"])
    assert enh.range_bits == 0


# ---- 7. the video's alignment -----------------------------------------------------------------------------------
def offset_video(vd, floats):
    """vd's values in a contiguous view `floats` floats into a fresh buffer: the data pointer is 4 * floats bytes past
    the buffer's (16-byte aligned) start."""
    buf = torch.empty(vd.numel() + 4, dtype=vd.dtype, device=vd.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[floats:floats + vd.numel()].view(vd.shape)
    view.copy_(vd)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * floats) % 16
    return view


def test_video_off_a_16_byte_boundary_gives_the_aligned_bits(gpu):
    """k_stream_route moves a call's video slices 16 bytes per lane when the video pointer is 16-byte aligned and 4 bytes
    per lane otherwise.  The same two slices go to a B = 2 session from tensors 4 bytes past a 16-byte boundary and
    from aligned ones: push 1 queues slice 0 (19 frames: no slice is complete), push 2 stages it from the queue and
    queues slice 1, the flush stages that one.  Everything the session returns must be the same bits."""
    from avse_amd import ops
    from avse_amd.pipeline import StreamEnhancer
    B = 2
    x, video, mean, std, _ = inputs()
    md, sd = ops.to_device(mean), ops.to_device(std)
    xd, vd = ops.to_device(x[:B, :6400]), ops.to_device(video[:B, :2])
    enh = StreamEnhancer(weights("float32"), B)
    runs = []
    for floats in (1, 0):
        enh.reset()
        got = []
        for k in range(2):
            vid = offset_video(vd[:, k:k + 1].contiguous(), floats)
            got.append(enh.push(xd[:, 3200 * k:3200 * k + 3200].contiguous(), vid, md, sd, return_spectrograms=True))
        got.append(enh.flush(md, sd, return_spectrograms=True))
        runs.append([torch.cat([g[i] for g in got], dim=1).cpu().numpy() for i in range(3)])
    assert runs[0][0].shape == (B, 6240) and runs[0][1].shape == runs[0][2].shape == (B, 2, 80, 20)
    for key, off, aligned in zip(("out", "mel", "pred"), *runs):
        assert np.isfinite(off).all() and same_bits(off, aligned), key
