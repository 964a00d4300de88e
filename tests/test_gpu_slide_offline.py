"""The offline sliding path (pipeline.Enhancer(stride=), ops.slide_windows / slide_video_windows / slide_keep,
predict --stride) against the float64 reference tests/slide_ref.py, against the torch composition of
the existing ops bit for bit, against itself (ragged = alone), against a flushed sliding session, and through the CLI.

Shapes: test_gpu_streaming's three utterances cut to 4, 2 and 1 slices (the last has one window and keeps only window 0),
so chunks of 7 windows end inside utterances; one utterance of 14 slices (281 frames: two 256-frame scan chunks); two
slices of the 30-fps geometry.  The references of the 4-slice utterances are test_gpu_slide's, made once per process."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import slide_ref
from test_gpu_slide import KEYS, as_frames, check_against_reference, frames, reference, run_slide
from test_gpu_stft import DB_MAX
from test_gpu_streaming import inputs, same_bits, weights

pytestmark = pytest.mark.gpu

SLICES = (4, 2, 1)          # of utterances 0, 1, 2


@functools.lru_cache(None)
def cut_reference(u, n_slices, stride):
    """slide_ref of utterance u cut to its first n_slices slices (the 4-slice ones are test_gpu_slide.reference's)."""
    if n_slices == 4:
        return reference(u, stride)
    x, _, mean, std, model = inputs()
    return slide_ref.slide_reference(x[u][:3200 * n_slices], frames()[u][:5 * n_slices], mean, std, model.layer_dict(), stride)


def batch(video_u8=False):
    """The ragged batch on the device: signals [3200 S_u] and videos [S_u, 128, 128, 5] of utterances 0..2."""
    from avse_amd import ops
    x, video, _, _, _ = inputs()
    v = video.astype(np.uint8) if video_u8 else video
    return ([ops.to_device(x[u][:3200 * s]) for u, s in enumerate(SLICES)],
            [ops.video_to_device(np.ascontiguousarray(v[u][:s])) for u, s in enumerate(SLICES)])


def norm():
    from avse_amd import ops
    return ops.to_device(inputs()[2]), ops.to_device(inputs()[3])


def offline(enh, sigs, videos, mean=None, std=None):
    """enhance_ragged with the windows -> one dict(out, mel, pred) of numpy arrays per utterance."""
    m, s = norm() if mean is None else (mean, std)
    outs, net_in, pred, W = enh.enhance_ragged(sigs, videos, m, s, return_spectrograms=True)
    torch.cuda.synchronize()
    ends = np.cumsum(W)
    return [dict(out=outs[u].cpu().numpy(), mel=net_in[int(e - w):int(e)].cpu().numpy(), pred=pred[int(e - w):int(e)].cpu().numpy())
            for u, (e, w) in enumerate(zip(ends, W))]


def composed(dw, sig, video, stride, mean, std, spf=20, F=5, **kw):
    """The torch composition of test_gpu_slide.test_report_bit_equality_with_the_offline_ops for one utterance (device
    tensors in): ops.spectrogram(top_db=None), the clamp in torch, ops.forward on torch-stacked windows, torch.cat of the
    kept columns, ops.istft with its default options -> dict(out, mel, pred) of numpy arrays."""
    from avse_amd import ops
    q = spf // F
    qs = q * stride
    S = video.shape[0]
    W = (F * S - F) // stride + 1
    un, stft = ops.spectrogram(sig[None].contiguous(), top_db=None, return_stft=True, **kw)
    wins = torch.stack([torch.maximum(un[0, :, qs * j:qs * j + spf], un[0, :, :qs * j + spf].max() - 80.0) for j in range(W)])
    fr = video.permute(0, 3, 1, 2).reshape(S * F, 128, 128)                 # frame F k + i = video[k, :, :, i]
    clips = torch.stack([fr[stride * j:stride * j + F].permute(1, 2, 0) for j in range(W)]).contiguous()
    pred = ops.forward(dw, wins.contiguous(), clips, mean, std)
    kept = torch.cat([pred[0]] + [pred[j][:, spf - qs:] for j in range(1, W)], dim=1)[None].contiguous()
    out = ops.istft(kept, stft, **kw)
    return dict(out=out[0].cpu().numpy(), mel=wins.cpu().numpy(), pred=pred.cpu().numpy())


# ---- 1. the float64 reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype,video_u8", [("float32", False), ("float32_split", False), ("bfloat16", False),
                                            ("float32_split", True)])
def test_offline_matches_the_reference(gpu, dtype, video_u8, stride):
    from avse_amd import ops
    from avse_amd.pipeline import Enhancer
    enh = Enhancer(weights(dtype), stride=stride)
    got = offline(enh, *batch())
    if video_u8:            # the crops' own bytes: the float32-video run's bits
        got8 = offline(enh, *batch(video_u8=True))
        for a, b in zip(got, got8):
            for key in KEYS:
                assert same_bits(a[key], b[key]), key
        got = got8
    W, P = ops.slide_window_counts(SLICES, 20, 5, stride)
    assert W.tolist() == ([16, 6, 1] if stride == 1 else [8, 3, 1]) and P.tolist() == ([80, 40, 20] if stride == 1 else [76, 36, 20])
    for u, s in enumerate(SLICES):
        assert got[u]["out"].shape == (160 * (P[u] - 1),) and got[u]["mel"].shape == got[u]["pred"].shape == (W[u], 80, 20)
        assert np.isfinite(got[u]["out"]).all()
        check_against_reference(got[u], cut_reference(u, s, stride), dtype, f"{dtype} stride {stride} utterance {u} ({s} slices)")
    if dtype == "float32_split":
        assert enh.range_bits == 0


# ---- 2. the composed existing ops, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["float32", "float32_split", "bfloat16"])
def test_bit_equality_with_the_composed_ops(gpu, dtype, stride):
    """The new kernels only move data and take maxima: the ragged batch in chunks of 7 windows (which end inside
    utterances) against the per-utterance composition of the existing ops.  bfloat16 is gated by tolerance only."""
    from avse_amd.pipeline import Enhancer
    dw = weights(dtype)
    sigs, videos = batch()
    mean, std = norm()
    got = offline(Enhancer(dw, stride=stride, chunk=7), sigs, videos)
    for u in range(len(SLICES)):
        want = composed(dw, sigs[u], videos[u], stride, mean, std)
        if dtype == "bfloat16":
            assert same_bits(got[u]["mel"], want["mel"])
            check_against_reference(got[u], dict(mel=want["mel"].astype(np.float64), pred=want["pred"], wave=want["out"]),
                                    dtype, f"bfloat16 stride {stride} utterance {u} vs the composition")
            continue
        for key in KEYS:
            assert same_bits(got[u][key], want[key]), (dtype, stride, u, key)


# ---- 3. ragged = alone -----------------------------------------------------------------------------------------
def test_each_utterance_is_its_own_call(gpu):
    from avse_amd import ops
    from avse_amd.pipeline import Enhancer
    enh = Enhancer(weights("float32_split"), stride=2, chunk=5)
    sigs, videos = batch()
    mean, std = norm()
    together = offline(enh, sigs, videos)
    for u in range(len(SLICES)):
        alone = offline(enh, [sigs[u]], [videos[u]])[0]
        for key in KEYS:
            assert same_bits(together[u][key], alone[key]), (u, key)
    # __call__ on the equal-length batch is enhance_ragged's rows
    x, video, _, _, _ = inputs()
    xd, vd = ops.to_device(x), ops.video_to_device(video)
    rows = enh(xd, vd, mean, std)
    ragged = enh.enhance_ragged(list(xd), list(vd), mean, std)
    assert rows.shape == (3, 12000) and enh.staged_video_bytes == 5 * 128 * 128 * 5 * 4
    for u in range(3):
        assert same_bits(rows[u].cpu().numpy(), ragged[u].cpu().numpy()), u
    # a signal shorter than its video is padded, a longer one cut, as the slice path does
    short = enh.enhance_ragged([xd[0][:12000].contiguous()], [vd[0]], mean, std)[0]
    padded = enh.enhance_ragged([torch.nn.functional.pad(xd[0][:12000], (0, 900))], [vd[0]], mean, std)[0]
    assert same_bits(short.cpu().numpy(), padded.cpu().numpy())


# ---- 4. the scan's carry, and causality ------------------------------------------------------------------------
LONG_S, LONG_STRIDE = 14, 2


@functools.lru_cache(None)
def long_inputs():
    """One utterance of 14 slices (281 frames, two scan chunks): 60 dB quieter for its first 8 slices, and an 80-ms
    dropout 100 dB down inside the second scan chunk (frames 262 .. 270), where only the carried maximum gives the floor."""
    from conftest import synth_audio, synth_video
    from oracle import librosa_ref as R
    rng = np.random.default_rng(22)
    x = synth_audio(rng, 1, 3200 * LONG_S)[0]
    x[:8 * 3200] *= 1e-3
    x[41920:43200] *= 1e-5
    video = synth_video(rng, LONG_S)
    mean, std = R.video_normalizer_fit(video)
    return x, video, mean, std


@functools.lru_cache(None)
def long_reference():
    x, video, mean, std = long_inputs()
    return slide_ref.slide_reference(x, as_frames(video), mean, std, inputs()[4].layer_dict(), LONG_STRIDE)


def binding(ref, stride=LONG_STRIDE):
    """per window: does the floor raise a value of the reference's window?"""
    qs = 4 * stride
    return np.array([(ref["mel"][j] != ref["unclamped"][:, qs * j:qs * j + 20]).any() for j in range(ref["mel"].shape[0])])


def test_scan_carry_and_causality(gpu):
    from avse_amd import ops
    from avse_amd.pipeline import Enhancer
    x, video, mean, std = long_inputs()
    ref = long_reference()
    un, floors, binds = ref["unclamped"], ref["floors"], binding(ref)
    W = binds.shape[0]
    assert W == 33 and un.shape[1] == 280
    first_late = (256 - 20) // 8 + 1            # the first window whose last frame lies in the second scan chunk
    print(f"reference: the floor binds in windows {np.flatnonzero(binds).tolist()} of {W}; floors of windows 0 / 18 / 32: "
          f"{floors[0]:.1f} / {floors[18]:.1f} / {floors[32]:.1f} dB; maximum of frames 0..255 {un[:, :256].max():.1f} dB, of "
          f"frames 256.. {un[:, 256:].max():.1f} dB")
    assert binds.any() and not binds.all() and not binds[:17].any()      # in some windows, not in all, and only in later ones
    assert binds[first_late:].any()                                       # ... some of them past the first scan chunk,
    assert un[:, 256:].max() < un[:, :256].max() - 1.0                    # where only the carry holds the maximum
    dw = weights("float32_split")
    md, sd = ops.to_device(mean), ops.to_device(std)
    xd, vd = ops.to_device(x), ops.video_to_device(video)
    enh = Enhancer(dw, stride=LONG_STRIDE, chunk=16)
    got = offline(enh, [xd], [vd], md, sd)[0]
    want = composed(dw, xd, vd, LONG_STRIDE, md, sd)
    assert same_bits(got["mel"], want["mel"])
    assert same_bits(got["pred"], want["pred"]) and same_bits(got["out"], want["out"])
    # the floors, recovered from the kernel's output: where the floor binds it is the window's minimum
    mins = got["mel"].reshape(W, -1).min(axis=1).astype(np.float64)
    print(f"floors recovered in the binding windows: max |error| {np.abs(mins[binds] - floors[binds]).max():.2e} dB")
    assert np.abs(mins[binds] - floors[binds]).max() <= DB_MAX
    assert (mins[~binds] >= floors[~binds] - DB_MAX).all()
    check_against_reference(got, ref, "float32_split", "14 slices, stride 2")
    # causality: windows that end before the loud part do not change when it is replaced by silence
    quiet = x.copy()
    quiet[8 * 3200:] = 0.0
    got_q = offline(enh, [ops.to_device(quiet)], [vd], md, sd)[0]
    early = (160 - 2 - 20) // 8 + 1            # windows whose last frame is at most 157: two frames clear of sample 25600
    assert early == 18 and same_bits(got_q["mel"][:early], got["mel"][:early])
    assert same_bits(got_q["pred"][:early], got["pred"][:early])
    assert not same_bits(got_q["mel"][early + 1:], got["mel"][early + 1:])


# ---- 5. F = 6 --------------------------------------------------------------------------------------------------
def test_six_frame_slices_at_30_fps(gpu):
    """24 kHz / 30 fps, n_fft 800, the [80, 24] x 6-frame weights: 2 slices at stride 4, which does not divide F (S - 1) = 6."""
    import test_gpu_stream_fps30 as fps30
    from avse_amd import ops
    from avse_amd.pipeline import Enhancer
    video, mean, std, model = fps30.inputs()
    x, vid = fps30.audio(24000)[0][:2 * 4800], video[0][:2]
    md, sd = ops.to_device(mean), ops.to_device(std)
    dw = fps30.weights("float32_split")
    enh = Enhancer(dw, video_frame_rate=30.0, sample_rate=24000, stride=4)
    xd, vd = ops.to_device(x), ops.video_to_device(np.ascontiguousarray(vid))
    got = offline(enh, [xd], [vd], md, sd)[0]
    assert got["mel"].shape == got["pred"].shape == (2, 80, 24) and got["out"].shape == (200 * (40 - 1),)
    ref = slide_ref.slide_reference(x, as_frames(vid), mean, std, model.layer_dict(), 4, sr=24000, n_fft=800, hop=200, spf=24)
    check_against_reference(got, ref, "float32_split", "24 kHz 30 fps, 2 slices, stride 4", gate_pred=False)
    want = composed(dw, xd, vd, 4, md, sd, spf=24, F=6, sample_rate=24000, n_fft=800, hop_length=200)
    for key in KEYS:
        assert same_bits(got[key], want[key]), key
    # uint8 crops at F = 6: the same bits
    got8 = offline(enh, [xd], [ops.video_to_device(np.ascontiguousarray(vid.astype(np.uint8)))], md, sd)[0]
    for key in KEYS:
        assert same_bits(got[key], got8[key]), key
    with pytest.raises(ValueError, match="weights"):
        Enhancer(weights("float32_split"), video_frame_rate=30.0, sample_rate=24000, stride=4).enhance_ragged([xd], [vd], md, sd)


# ---- 6. the session, reported ----------------------------------------------------------------------------------
def test_cross_check_with_a_flushed_session(gpu):
    """Gated by the reference's tolerances on both sides; the bit comparison is printed, not asserted."""
    from avse_amd.pipeline import Enhancer, SlidingStreamEnhancer
    dw = weights("float32_split")
    sigs, videos = batch()
    got = offline(Enhancer(dw, stride=1), sigs[:1], videos[:1])[0]
    sess = run_slide(SlidingStreamEnhancer(dw, 1, stride=1), inputs()[0][:1], frames()[:1], [640] * 20, [1] * 20)
    sess = {k: sess[k][0] for k in KEYS}
    ref = reference(0, 1)
    check_against_reference(got, ref, "float32_split", "offline, utterance 0, stride 1")
    check_against_reference(sess, ref, "float32_split", "flushed session, utterance 0, stride 1")
    print("offline == flushed SlidingStreamEnhancer, bit for bit: " +
          ", ".join(f"{k} {same_bits(got[k], sess[k])}" for k in ("mel", "pred", "out")))
    assert got["out"].shape == sess["out"].shape == (12640,)


# ---- 7. the ops alone: ranges, both dtypes -----------------------------------------------------------------------
@pytest.mark.parametrize("F,stride", [(5, 1), (5, 3), (6, 4), (6, 5)])
def test_video_windows_of_any_range(gpu, F, stride):
    from avse_amd import ops
    rng = np.random.default_rng(F * 10 + stride)
    slices = [3, 0, 1, 2]
    video = rng.integers(0, 256, (sum(slices), 128, 128, F), dtype=np.uint8)
    W = [(F * s - F) // stride + 1 if s else 0 for s in slices]
    want, k0 = [], 0
    for s in slices:
        fr = np.moveaxis(video[k0:k0 + s], -1, 1).reshape(s * F, 128, 128)
        want += [np.moveaxis(fr[stride * j:stride * j + F], 0, -1) for j in range((F * s - F) // stride + 1 if s else 0)]
        k0 += s
    want = np.stack(want)
    assert ops.slide_window_counts(slices, F, F, stride)[0].tolist() == W
    for dt in (np.uint8, np.float32):
        vd = ops.video_to_device(video.astype(dt))
        whole = ops.slide_video_windows(vd, slices, stride=stride)
        assert whole.dtype == vd.dtype and np.array_equal(whole.cpu().numpy(), want.astype(dt))
        stage = torch.empty((4, 128, 128, F), dtype=vd.dtype, device=vd.device)
        for w0 in range(0, sum(W), 3):      # ranges that start and end inside utterances, into a reused staging buffer
            n = min(3, sum(W) - w0)
            part = ops.slide_video_windows(vd, slices, stride=stride, w0=w0, n=n, out=stage)
            assert part.shape[0] == n and np.array_equal(part.cpu().numpy(), want[w0:w0 + n].astype(dt)), (dt, w0)
    with pytest.raises(ValueError, match="outside"):
        ops.slide_video_windows(vd, slices, stride=stride, w0=sum(W), n=1)


def test_windows_and_keep_without_a_clamp(gpu):
    """top_db None: the windows are the unclamped frames; keep of the windows gives back frames 0 .. P - 1."""
    from avse_amd import ops
    rng = np.random.default_rng(3)
    slices, T = [2, 0, 14, 1], [41, 3, 283, 21]
    blocks = [rng.normal(0, 20, (80, t)).astype(np.float32) for t in T]
    packed = ops.to_device(np.concatenate([b.reshape(-1) for b in blocks]))
    for stride in (1, 5):
        W, P = ops.slide_window_counts(slices, 20, 5, stride)
        wins = ops.slide_windows(packed, T, slices, stride=stride, top_db=None)
        kept, P2 = ops.slide_keep(wins, slices, stride=stride)
        assert P2.tolist() == P.tolist() and wins.shape[0] == W.sum()
        got, at = kept.cpu().numpy(), 0
        for b, p in zip(blocks, P.tolist()):
            assert np.array_equal(got[at:at + 80 * p].reshape(80, p), b[:, :p])
            at += 80 * p
        clamped = ops.slide_windows(packed, T, slices, stride=stride, top_db=30.0).cpu().numpy()
        w0 = 0
        for b, w in zip(blocks, W.tolist()):
            for j in range(w):
                t0 = 4 * stride * j
                assert np.array_equal(clamped[w0 + j], np.maximum(b[:, t0:t0 + 20], b[:, :t0 + 20].max() - np.float32(30.0)))
            w0 += w


def test_windows_and_keep_on_the_scalar_paths(gpu):
    """spf 10 with F 5 (q = 2) and spf 6 with F 6 (q = 1) are legal through the C-ABI and ops, and neither spf nor q is a
    multiple of 4: k_slide_off_windows' one-value loop and k_slide_off_keep<false>, against numpy, with a clamp that
    binds (normal data with sigma 20 dB under a 30-dB floor) and a block of more than one scan chunk."""
    from avse_amd import ops
    rng = np.random.default_rng(4)
    for spf, F, n_mels in ((10, 5, 80), (6, 6, 7)):
        q = spf // F
        slices, extra = [3, 0, 50, 1], [1, 2, 3, 0]
        T = [spf * s + e for s, e in zip(slices, extra)]
        assert max(T) > 256
        blocks = [rng.normal(0, 20, (n_mels, t)).astype(np.float32) for t in T]
        packed = ops.to_device(np.concatenate([b.reshape(-1) for b in blocks]))
        for stride in (1, 2, F):
            kw = dict(frames_per_slice=spf, video_frames=F, stride=stride, n_mels=n_mels)
            W, P = ops.slide_window_counts(slices, spf, F, stride)
            plain = ops.slide_windows(packed, T, slices, top_db=None, **kw)
            clamped = ops.slide_windows(packed, T, slices, top_db=30.0, **kw).cpu().numpy()
            kept, P2 = ops.slide_keep(plain, slices, video_frames=F, stride=stride)
            assert P2.tolist() == P.tolist() and plain.shape == (W.sum(), n_mels, spf)
            got, at, w0, raised = kept.cpu().numpy(), 0, 0, 0
            for b, w, p in zip(blocks, W.tolist(), P.tolist()):
                assert np.array_equal(got[at:at + n_mels * p].reshape(n_mels, p), b[:, :p]), (spf, stride)
                at += n_mels * p
                for j in range(w):
                    t0 = q * stride * j
                    want = np.maximum(b[:, t0:t0 + spf], b[:, :t0 + spf].max() - np.float32(30.0))
                    raised += int((want != b[:, t0:t0 + spf]).sum())
                    assert np.array_equal(clamped[w0 + j], want), (spf, stride, j)
                w0 += w
            assert raised > 0 and at == got.size


# ---- 8. the command line -----------------------------------------------------------------------------------------
def test_cli_predict_with_a_stride(gpu, tmp_path):
    """predict --stride 2 writes Enhancer(stride=2)'s signal; without the flag the files are the slice path's."""
    import shutil
    from scipy.io import wavfile
    from test_gpu_cli import make_dataset, run
    from avse_amd import data_processor, ops
    from avse_amd.audio_io import AudioSignal
    from avse_amd.network import SpeechEnhancementNetwork
    from avse_amd.pipeline import Enhancer
    from avse_amd.speech_enhancer import Layout, load_preprocessed_blob
    tmp = str(tmp_path)
    ds, noise = make_dataset(tmp, n_noise=2)
    base = os.path.join(tmp, "base")
    os.makedirs(base)
    assert "preprocessed 2 samples" in run(["-bd", base, "preprocess", "-dn", "d", "-ds", ds, "-n", noise], tmp)
    run(["-bd", base, "train", "-mn", "m", "-tdn", "d", "-vdn", "d", "--init-only"], tmp)
    layout = Layout(base)
    samples = load_preprocessed_blob(layout.preprocessed("d"))
    network = SpeechEnhancementNetwork.load(layout.model_file("m"), compute_dtype="float32_split")
    normalizer = data_processor.VideoNormalizer.load(layout.normalizer_file("m"))
    dw = network.device_weights()
    m, s = normalizer.device_stats(torch.device("cuda", dw.ctx.device_index))
    sigs = [ops.to_device(np.asarray(smp.mixed_signal.get_data(channel_index=0)).astype(np.float32)) for smp in samples]
    vids = [ops.video_to_device(np.ascontiguousarray(smp.video_samples)) for smp in samples]
    losses = {}
    for stride in (None, 2):
        out = run(["-bd", base, "predict", "-mn", "m", "-dn", "d"] + (["--stride", "2"] if stride else []), tmp)
        losses[stride] = [ln for ln in out.splitlines() if ln.startswith("loss:")]
        run_dir = os.path.join(base, "out", "m", "d")
        wavs = sorted(glob.glob(os.path.join(run_dir, "*", "*", "*", "enhanced.wav")))
        assert len(wavs) == len(samples) == 2
        want = Enhancer(dw, stride=stride).enhance_ragged(sigs, vids, m, s)
        P = int(ops.slide_window_counts([15], 20, 5, stride)[1][0]) if stride else 300
        assert P == 300                       # 15 slices: stride 2 divides F (S - 1) = 70, so no tail is lost here
        for u, smp in enumerate(samples):     # write_prediction's directory of the sample
            name = os.path.splitext(os.path.basename(smp.video_file_path))[0] + "_" + \
                os.path.splitext(os.path.basename(smp.noise_file_path))[0]
            w, = glob.glob(os.path.join(run_dir, "*", smp.speaker_id, name, "enhanced.wav"))
            sr, y = wavfile.read(w)
            assert sr == 16000 and y.shape == (160 * (P - 1),) == tuple(want[u].shape)
            tmpwav = os.path.join(tmp, "want.wav")
            AudioSignal(want[u].cpu().numpy(), 16000).save_to_wav_file(tmpwav)
            assert open(w, "rb").read() == open(tmpwav, "rb").read(), (stride, name)
        shutil.move(run_dir, run_dir + f"_{stride}")
    assert len(losses[None]) == 2 and losses[None] == losses[2]      # the printed loss stays the slice-based one
