"""CPU tests of the uint8 video path (include/avse.h AVSE_VIDEO_U8): what the C-ABI and the Python layer decide on the
host — the additive entry points, the argument checks made before any GPU work, and the `preprocess --video-u8` cache."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

VIDEO_ENTRY_POINTS = ("avse_forward_video", "avse_forward_checked_video", "avse_forward_profile_video",
                      "avse_video_stats_video", "avse_trainer_step_video")


def test_library_exports_the_video_dtype_entry_points():
    from avse_amd import _lib
    lib = _lib.load()
    for f in VIDEO_ENTRY_POINTS:
        assert hasattr(lib, f) and f in _lib.SIGNATURES, f
    assert lib.avse_abi_version() == 3          # additive: the ABI version did not move
    assert (_lib.AVSE_VIDEO_F32, _lib.AVSE_VIDEO_U8) == (0, 1)
    header = open(_lib.HEADER_PATH).read()
    assert "AVSE_VIDEO_F32 = 0" in header and "AVSE_VIDEO_U8 = 1" in header


def test_video_dtype_and_alignment_are_checked_before_any_gpu_work():
    from avse_amd import _lib
    lib = _lib.load()
    assert lib.avse_forward_video(None, None, None, None, 1, None, None, 1, None, None) == 1
    assert lib.avse_trainer_step_video(None, None, None, 1, None, None, None, 1, 0.0, 0.0, 0, 0, None, None) == 1
    buf = (ctypes.c_char * 64)()
    base = ctypes.addressof(buf)
    base += -base % 4
    p = ctypes.c_void_p(base)
    # non-NULL dummies, never read: the dtype and the alignment are refused before the context is touched
    rc = lib.avse_video_stats_video(p, p, 7, 1, 2, 2, 1, p, p, None)
    assert rc == 1 and b"dtype" in lib.avse_last_error()
    for off in (1, 2, 3):
        rc = lib.avse_video_stats_video(p, ctypes.c_void_p(base + off), _lib.AVSE_VIDEO_U8, 1, 2, 2, 1, p, p, None)
        assert rc == 1 and b"align" in lib.avse_last_error(), off
        rc = lib.avse_trainer_step_video(p, p, ctypes.c_void_p(base + off), _lib.AVSE_VIDEO_U8, p, None, None, 1, 0.0, 0.0,
                                         0, 0, None, None)
        assert rc == 1 and b"align" in lib.avse_last_error(), off


def test_crops_as_uint8_takes_only_exact_byte_values():
    from avse_amd.speech_enhancer import crops_as_uint8
    u = np.array([[0, 255], [7, 128]], np.uint8)
    assert crops_as_uint8(u) is u
    for dt in (np.int16, np.int64, np.uint16, np.float32, np.float64):
        out = crops_as_uint8(u.astype(dt))
        assert out.dtype == np.uint8 and np.array_equal(out, u), dt
    for bad in (np.array([0.5], np.float32), np.array([-1], np.int16), np.array([256], np.int32),
                np.array([255.0001], np.float64), np.array([np.nan], np.float32), np.array([np.inf], np.float32),
                np.array([True]), np.array([1 + 0j])):
        with pytest.raises(ValueError):
            crops_as_uint8(bad)


def _crops(tmp_path, name, values):
    path = str(tmp_path / (name + ".npy"))
    np.save(path, values)
    return path


def _sample(video, path="v.npy"):
    from avse_amd.audio_io import AudioSignal
    from avse_amd.speech_enhancer import Sample
    spec = np.zeros((video.shape[0], 80, 20), np.float32)
    return Sample("s1", path, "a.wav", "n.wav", video, spec, spec, spec, AudioSignal(np.zeros(64, np.float64), 16000), 25.0)


def test_video_u8_cache_round_trip_is_uint8_and_a_quarter_of_the_float_bytes(tmp_path):
    from avse_amd import speech_enhancer as se
    rng = np.random.default_rng(0)
    path = _crops(tmp_path, "clip", rng.integers(0, 256, (12, 128, 128), dtype=np.uint8))
    v8, fps = se.preprocess_video_sample(path, 200, video_u8=True)
    vf, _ = se.preprocess_video_sample(path, 200)                     # without the flag: float32 as before
    assert v8.dtype == np.uint8 and vf.dtype == np.float32 and fps == 25.0
    assert v8.shape == vf.shape == (2, 128, 128, 5) and np.array_equal(v8.astype(np.float32), vf)
    blobs = {}
    for name, v in (("u", v8), ("f", vf)):
        blob = str(tmp_path / (name + ".npz"))
        se.save_preprocessed_blob(blob, [_sample(v, path)])
        (back,) = se.load_preprocessed_blob(blob)
        assert back.video_samples.dtype == v.dtype and np.array_equal(back.video_samples, v)
        with np.load(blob, allow_pickle=False) as z:
            blobs[name] = z["s0_video_samples"].nbytes
    assert blobs["u"] * 4 == blobs["f"] == 2 * 128 * 128 * 5 * 4


def test_fractional_float_crops_are_skipped_with_the_flag(tmp_path, capsys):
    from avse_amd import speech_enhancer as se
    Entry = namedtuple("Entry", ["speaker_id", "video_path", "audio_path"])
    frames = np.full((5, 128, 128), 3.0, np.float32)
    whole = _crops(tmp_path, "whole", frames)
    frames[2, 5, 5] = 0.5
    frac = _crops(tmp_path, "frac", frames)
    assert se.preprocess_video_sample(whole, 200, video_u8=True)[0].dtype == np.uint8
    # the video is read first: the sample is dropped before any audio (and GPU) work
    assert se.preprocess_data([Entry("s", frac, "missing.wav")], ["missing_noise.wav"], video_u8=True) == []
    out = capsys.readouterr().out
    assert "failed to preprocess" in out and "whole-number" in out
    assert se.preprocess_data([Entry("s", frac, "missing.wav")] * 2, ["n.wav"] * 2, batch=2, video_u8=True) == []
    assert capsys.readouterr().out.count("whole-number") == 2


def test_cli_flag_defaults_to_float_crops(monkeypatch):
    from avse_amd import speech_enhancer as se
    seen = []
    monkeypatch.setattr(se, "preprocess", lambda args: seen.append(args.video_u8))
    pre = ["-bd", "b", "preprocess", "-dn", "d", "-ds", "ds", "-n", "n"]
    se.main(pre)
    se.main(pre + ["--video-u8"])
    assert seen == [False, True]


def test_make_sample_set_keeps_uint8():
    from avse_amd import speech_enhancer as se
    rng = np.random.default_rng(1)
    samples = [_sample(rng.integers(0, 256, (n, 128, 128, 5), dtype=np.uint8)) for n in (2, 3)]
    video, mixed, speech = se.make_sample_set(samples)
    assert video.dtype == np.uint8 and video.shape == (5, 128, 128, 5) and mixed.shape == speech.shape == (5, 80, 20)
    assert sorted(video.reshape(5, -1).sum(axis=1)) == sorted(
        np.concatenate([s.video_samples for s in samples]).reshape(5, -1).sum(axis=1))


def test_host_normaliser_fit_takes_uint8_and_refuses_to_normalise_it():
    from avse_amd.data_processor import VideoNormalizer
    v = np.random.default_rng(2).integers(0, 256, (3, 8, 8, 5), dtype=np.uint8)
    norm = VideoNormalizer(v)
    assert norm.mean_image.dtype == norm.std_image.dtype == np.float32
    v64 = v.astype(np.float64)
    assert np.array_equal(norm.mean_image, np.mean(v64, axis=(0, 3)).astype(np.float32))
    assert np.array_equal(norm.std_image, np.std(v64, axis=(0, 3)).astype(np.float32))
    with pytest.raises(TypeError, match="fused"):
        norm.normalize(v)
