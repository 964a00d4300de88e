"""CPU tests of the device-side preprocess bindings (avse_mix_pairs, avse_video_stats): what the C-ABI and the Python
layer decide on the host, before any GPU work — argument validation, the input types the batched path takes, and how
pairs are grouped into batches."""
import numpy as np
import pytest


def test_library_exports_the_preprocess_entry_points():
    from avse_amd import _lib
    lib = _lib.load()
    for f in ("avse_mix_pairs", "avse_video_stats"):
        assert hasattr(lib, f) and f in _lib.SIGNATURES
    assert lib.avse_abi_version() == 3          # additive: the ABI version did not move


def test_null_and_negative_arguments_are_rejected_without_gpu_work():
    from avse_amd import _lib
    lib = _lib.load()
    rc = lib.avse_mix_pairs(None, None, None, None, None, None, 1, 16, None, None, None, None)
    assert rc == 1 and b"NULL" in lib.avse_last_error()
    rc = lib.avse_video_stats(None, None, 1, 128, 128, 5, None, None, None)
    assert rc == 1 and b"NULL" in lib.avse_last_error()
    # a non-NULL context and buffers, bad extents: refused before the context is touched (the pointers are never read)
    import ctypes
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n_pairs, L in ((-1, 16), (1, 0), (1, -5)):
        rc = lib.avse_mix_pairs(p, p, p, p, p, None, n_pairs, L, p, None, None, None)
        assert rc == 1 and lib.avse_last_error(), (n_pairs, L)
    for S, H, W, F in ((-1, 8, 8, 5), (0, 8, 8, 5), (4, 0, 8, 5), (4, 8, -1, 5), (4, 8, 8, 0)):
        rc = lib.avse_video_stats(p, p, S, H, W, F, p, p, None)
        assert rc == 1 and lib.avse_last_error(), (S, H, W, F)


def _sig(data, sr=16000):
    from avse_amd.audio_io import AudioSignal
    return AudioSignal(data, sr)


def test_mix_pairs_rejects_multichannel_and_non_int16_input():
    from avse_amd import ops
    good = np.zeros(100, np.int16)
    for bad in (np.zeros((100, 2), np.int16), np.zeros(100, np.float32), np.zeros(100, np.int32),
                np.zeros(100, np.float64)):
        with pytest.raises(TypeError):
            ops.mix_pairs([bad], [good], 64)
        with pytest.raises(TypeError):
            ops.mix_pairs([good], [bad], 64)


def test_preprocess_audio_pairs_rejects_multichannel_and_non_int16_input():
    from avse_amd import data_processor as dp
    good = _sig(np.zeros(3200, np.int16))
    for bad in (_sig(np.zeros((3200, 2), np.int16)), _sig(np.zeros(3200, np.float32)),
                _sig(np.zeros(3200, np.float64))):
        with pytest.raises(TypeError):
            dp.preprocess_audio_pairs([bad], [good], 200, 1, 25.0)
        with pytest.raises(TypeError):
            dp.preprocess_audio_pairs([good, good], [good, bad], 200, 1, 25.0)


def test_mix_pairs_refuses_an_empty_speech_signal_on_the_host():
    from avse_amd import _lib, ops
    with pytest.raises(_lib.AvseError, match="AVSE_ERR_INVALID"):
        ops.mix_pairs([np.zeros(4, np.int16), np.zeros(0, np.int16)], [np.zeros(4, np.int16)] * 2, 64)


def test_pair_groups_split_by_length_and_frame_rate_and_keep_input_order():
    from avse_amd import data_processor as dp
    sigs = [_sig(np.zeros(10, np.int16)) for _ in range(6)] + [_sig(np.zeros(10, np.int16), sr=8000)]
    n_slices = [15, 15, 10, 15, 10, 15, 15]
    fps = [25.0, 30.0, 25.0, 25.0, 25.0, 30.0, 25.0]
    groups = dp.pair_groups(sigs, 200, n_slices, fps)
    # (signal_length, n_fft, sample_rate) in first-seen order, the indices of each group ascending
    assert groups == [((48000, 640, 16000), [0, 3]), ((48000, 533, 16000), [1, 5]), ((32000, 640, 16000), [2, 4]),
                      ((24000, 320, 8000), [6])]
    assert dp.pair_groups(sigs[:3], 200, 15, 25.0) == [((48000, 640, 16000), [0, 1, 2])]
    with pytest.raises(ValueError):
        dp.pair_groups(sigs, 200, [15, 15], 25.0)


def test_cli_flags_default_to_the_per_sample_paths(monkeypatch):
    """--batch 0 and no --device-normalizer are the defaults: the existing loops stay what a plain command line runs."""
    import inspect
    from avse_amd import speech_enhancer as se
    assert inspect.signature(se.preprocess_data).parameters["batch"].default == 0
    seen = []
    monkeypatch.setattr(se, "preprocess", lambda args: seen.append(args.batch))
    monkeypatch.setattr(se, "train", lambda args: seen.append(args.device_normalizer))
    pre = ["-bd", "b", "preprocess", "-dn", "d", "-ds", "ds", "-n", "n"]
    tr = ["-bd", "b", "train", "-mn", "m", "-tdn", "d", "-vdn", "d"]
    se.main(pre)
    se.main(pre + ["--batch", "8"])
    se.main(tr)
    se.main(tr + ["--device-normalizer"])
    assert seen == [0, 8, False, True]


def test_preprocess_batch_falls_back_pair_by_pair_and_skips_only_what_fails(monkeypatch, capsys):
    """The catch-and-skip of preprocess_data in the batched loop: an entry whose files do not load is skipped, and when
    the batched audio call fails the group is redone on preprocess_sample, losing only the pair that fails there."""
    from collections import namedtuple
    from avse_amd import speech_enhancer as se
    Entry = namedtuple("Entry", ["speaker_id", "video_path", "audio_path"])
    entries = [Entry("s", "v%d" % i, "a%d" % i) for i in range(5)]
    noises = ["n%d" % i for i in range(5)]

    def video(path, ms):
        if path == "v1":
            raise IOError("no such video")
        return np.zeros((2, 128, 128, 5), np.float32), 25.0

    calls = []

    def pairs(speech, noise, ms, n_slices, fps):
        calls.append((len(speech), list(n_slices), list(fps)))
        raise TypeError("float wav")

    def sample(entry, noise, ms=200):
        if entry.audio_path == "a3":
            raise ValueError("bad pair")
        return (entry.audio_path, noise)

    monkeypatch.setattr(se, "preprocess_video_sample", video)
    monkeypatch.setattr(se.AudioSignal, "from_wav_file", classmethod(lambda cls, path: path))
    monkeypatch.setattr(se.data_processor, "preprocess_audio_pairs", pairs)
    monkeypatch.setattr(se, "preprocess_sample", sample)
    got = se.preprocess_data(entries, noises, batch=3)
    # groups [0, 1, 2] and [3, 4]: entry 1 is dropped before the batched call, entry 3 by the fallback
    assert calls == [(2, [2, 2], [25.0, 25.0]), (2, [2, 2], [25.0, 25.0])]
    assert got == [("a0", "n0"), ("a2", "n2"), ("a4", "n4")]
    out = capsys.readouterr().out
    assert out.count("failed to preprocess") == 2 and "no such video" in out and "bad pair" in out
