"""CPU tests of the evaluate stage: what the C-ABI decides on the host, the float64 reference's self-checks
(tests/eval_ref.py), the host tables under AddressSanitizer / UndefinedBehaviorSanitizer (a stand-alone program,
tests/native/eval_tables_check.cpp), and the evaluator module with the device call replaced by the reference."""
import ctypes
import json
import os
import shutil
import stat
import subprocess
import wave

import numpy as np
import pytest

import eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-visual-speech-enhancement_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- ABI ---------------------------------------------------------------------------------------------------------
def test_library_exports_avse_eval_pairs():
    from avse_amd import _lib
    lib = _lib.load()
    for f in ("avse_eval_pairs", "avse_eval_pairs_sized"):
        assert hasattr(lib, f) and f in _lib.SIGNATURES
    assert lib.avse_abi_version() == 3          # additive: the ABI version did not move
    assert _lib.AVSE_EVAL_NMETRICS == len(_lib.EVAL_METRIC_NAMES) == R.NMETRICS == 5


def test_bad_arguments_are_rejected_without_gpu_work():
    from avse_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.avse_eval_pairs(None, None, None, None, 1, 16000, None, None) == 1 and b"NULL" in lib.avse_last_error()
    for hole in range(5):                       # each pointer argument NULL in turn
        args = [p, p, p, p, p]
        args[hole] = None
        rc = lib.avse_eval_pairs(args[0], args[1], args[2], args[3], 1, 16000, args[4], None)
        assert rc == 1 and b"NULL" in lib.avse_last_error(), hole
    # a non-NULL context and buffers, bad extents: refused before the context is touched (the pointers are never read)
    for n_pairs, sr in ((0, 16000), (-3, 16000), (1, 7999), (1, 48001), (1, 0)):
        assert lib.avse_eval_pairs(p, p, p, p, n_pairs, sr, p, None) == 1 and lib.avse_last_error(), (n_pairs, sr)
        assert lib.avse_eval_pairs_sized(p, p, p, p, n_pairs, 100, sr, p, None) == 1, (n_pairs, sr)
    # the sized form: a total outside 0 .. n_pairs * 2^24 (a pair of more than 2^24 samples) is refused
    for n_pairs, total in ((1, -1), (1, (1 << 24) + 1), (3, 3 * (1 << 24) + 1)):
        rc = lib.avse_eval_pairs_sized(p, p, p, p, n_pairs, total, 16000, p, None)
        assert rc == 1 and b"total_samples" in lib.avse_last_error(), (n_pairs, total)
    assert lib.avse_eval_pairs_sized(None, p, p, p, 1, 100, 16000, p, None) == 1 and b"NULL" in lib.avse_last_error()


def test_eval_pairs_refuses_bad_input_on_the_host():
    from avse_amd import _lib, ops
    s = np.zeros(100, np.float32)
    with pytest.raises(TypeError):
        ops.eval_pairs([np.zeros((100, 2), np.float32)], [s], 16000)
    with pytest.raises(TypeError):
        ops.eval_pairs([s.astype(np.int32)], [s], 16000)
    with pytest.raises(ValueError):
        ops.eval_pairs([s, s], [s], 16000)
    with pytest.raises(ValueError):
        ops.eval_pairs([s], [s], 7999)
    with pytest.raises(_lib.AvseError, match="AVSE_ERR_INVALID"):
        ops.eval_pairs([s, np.zeros(0, np.float32)], [s, s], 16000)
    import torch
    with pytest.raises(TypeError):              # the packed form lives on the device
        ops.eval_pairs((torch.zeros(100), np.array([0, 100], np.int64)), torch.zeros(100), 16000)


# ---- the reference's self-checks ----------------------------------------------------------------------------------
def test_reference_band_table():
    assert R.band_table() == R.BAND_RANGES


def test_reference_identical_signals():
    s, _ = R.speech_like(1, 16000)
    row = R.eval_pair(s, s.copy(), 16000)
    assert np.isposinf(row[R.SNR]) and np.isposinf(row[R.SI_SDR]) and row[R.SEG_SNR] == 35.0
    assert abs(row[R.STOI] - 1.0) <= 1e-12 and row[R.STOI_KEPT] > 30
    z = R.eval_pair(np.zeros(8000), np.zeros(8000), 16000)
    assert np.isnan(z[R.SNR]) and np.isnan(z[R.SI_SDR])
    assert np.isnan(R.eval_pair(np.zeros(0), np.zeros(0))).all()


@pytest.mark.parametrize("up,down", [(5, 8), (5, 4), (5, 24)])
def test_reference_resampling_is_resample_poly(up, down):
    from scipy.signal import resample_poly
    x = np.random.default_rng(up * 100 + down).uniform(-1.0, 1.0, 5003)
    got, want = R.resample(x, up, down), resample_poly(x, up, down)
    assert got.shape == want.shape == (-(-5003 * up // down),)
    assert np.abs(got - want).max() <= 1e-14
    assert np.array_equal(R.resample(x, 1, 1), x)


def test_reference_float32_mode_moves_only_the_stoi():
    s, y = R.speech_like(2, 12000)
    a, b = R.eval_pair(s, y), R.eval_pair(s, y, dtype=np.float32)
    assert np.array_equal(a[[0, 1, 2, 4]], b[[0, 1, 2, 4]]) and 0.0 < abs(a[R.STOI] - b[R.STOI]) < 1e-6


# ---- host tables, sanitized ----------------------------------------------------------------------------------------
def test_eval_tables_sanitized(tmp_path):
    from scipy.signal import firwin
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host sources are built with the kernels' compiler")
    exe = str(tmp_path / "eval_tables_check")
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++20", "-O2", "-g", "-ffp-contract=off",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tests", "native", "eval_tables_check.cpp"),
                         os.path.join(CSRC, "eval_tables.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"exit status {run.returncode}\n{run.stderr[-4000:]}"
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    got = json.loads(run.stdout)
    for up, down in ((5, 8), (5, 4), (5, 24)):
        H = 10 * max(up, down)
        want = firwin(2 * H + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
        taps = np.array(got["taps_%d_%d" % (up, down)])
        assert taps.shape == want.shape
        # the taps are at most up * fc in size and a double-precision I0 series is good to a few ulp
        assert np.abs(taps - want).max() <= 1e-12, (up, down, np.abs(taps - want).max())
        assert abs(taps.sum() / up - 1.0) <= 1e-14
    assert got["taps_1_1"] == [1.0]
    assert np.abs(np.array(got["W"]) - R.stoi_window()).max() <= 1e-15
    assert [tuple(b) for b in got["bands"]] == list(R.BAND_RANGES)
    k = np.arange(256)
    tw = np.array(got["twiddle"]).reshape(256, 2)
    assert np.abs(tw[:, 0] - np.cos(2 * np.pi * k / 512)).max() <= 1e-15
    assert np.abs(tw[:, 1] + np.sin(2 * np.pi * k / 512)).max() <= 1e-15
    w480 = 0.5 * (1.0 - np.cos(2.0 * np.pi * (np.arange(480) + 1.0) / 481.0))
    assert np.abs(np.array(got["segw_480"]) - w480).max() <= 1e-15
    assert got["ratios"] == {"8000": [5, 4, 240], "10000": [1, 1, 300], "16000": [5, 8, 480], "22050": [200, 441, 662],
                             "44100": [100, 441, 1323], "48000": [5, 24, 1440]}
    assert {sr: list(R.ratio(int(sr))) for sr in got["ratios"]} == {sr: v[:2] for sr, v in got["ratios"].items()}
    assert abs(got["i0_5"] - 27.239871823604442) <= 1e-13


# ---- the evaluator module ------------------------------------------------------------------------------------------
def write_wav(path, data, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if data.ndim == 1 else data.shape[1])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(data, dtype="<i2").tobytes())


@pytest.fixture
def tree(tmp_path):
    """<dir>/<speaker>/<sample>/{source,enhanced,mixture}.wav: two speakers, one sample without enhanced.wav, one
    stereo sample (channel 0 counts) and one 8 kHz sample."""
    sigs = {}
    for k, (spk, smp, sr, n) in enumerate((("s1", "b_clip", 16000, 9000), ("s1", "a_clip", 16000, 12000),
                                           ("s1", "c_broken", 16000, 8000), ("s2", "x_clip", 8000, 6000),
                                           ("s2", "y_stereo", 16000, 10000))):
        d = tmp_path / spk / smp
        d.mkdir(parents=True)
        src, mix = R.speech_like(50 + k, n, sr, 0.0)
        _, enh = R.speech_like(50 + k, n, sr, 10.0)
        src, mix, enh = src.astype(np.int16), mix.astype(np.int16), enh[:n - 100].astype(np.int16)   # enhanced is shorter
        if smp == "y_stereo":
            junk = np.full(n, 123, np.int16)
            write_wav(d / "source.wav", np.stack([src, junk], axis=1), sr)
        else:
            write_wav(d / "source.wav", src, sr)
        write_wav(d / "mixture.wav", mix, sr)
        if smp != "c_broken":
            write_wav(d / "enhanced.wav", enh, sr)
        sigs[(spk, smp)] = (sr, src, enh, mix)
    return tmp_path, sigs


def reference_eval_pairs(ref, deg, sample_rate=16000):
    import torch
    return torch.from_numpy(R.eval_pairs(ref, deg, sample_rate))


def test_evaluator_walks_the_tree_like_the_reference(tree, monkeypatch, capsys):
    from avse_amd import ops, speech_enhancement_evaluator as ev
    root, sigs = tree
    calls = []

    def fake(ref, deg, sample_rate=16000):
        calls.append((len(ref), sample_rate))
        return reference_eval_pairs(ref, deg, sample_rate)

    monkeypatch.setattr(ops, "eval_pairs", fake)
    monkeypatch.setattr(ev.os, "listdir", lambda p, _ld=os.listdir: sorted(_ld(p), reverse=(p == str(root))))
    table = ev.evaluate(str(root), batch=2)
    out = capsys.readouterr().out
    # the reference's order: speakers as os.listdir gives them (reversed here), samples sorted; the broken one skipped
    order = [("s2", "x_clip"), ("s2", "y_stereo"), ("s1", "a_clip"), ("s1", "b_clip")]
    assert [(r["speaker"], r["sample"]) for r in table] == order
    assert out.count("evaluating ") == 5 and out.count("failed to evaluate") == 1 and "skipping" in out
    assert [ln.split()[1].rstrip(".") for ln in out.splitlines() if ln.startswith("evaluating ")] == \
        ["x_clip", "y_stereo", "a_clip", "b_clip", "c_broken"]
    # device batches of at most `batch` samples (two pairs per sample), grouped by sample rate
    assert sorted(calls) == sorted([(2, 8000), (4, 16000), (2, 16000)])
    for r in table:
        sr, src, enh, mix = sigs[(r["speaker"], r["sample"])]
        assert r["sample_rate"] == sr
        n = min(src.size, enh.size)
        assert np.array_equal(r["enhanced"], R.eval_pair(src[:n], enh[:n], sr), equal_nan=True)
        assert np.array_equal(r["mixture"], R.eval_pair(src, mix, sr), equal_nan=True)
        for k, name in enumerate(ev.METRICS):
            assert "mixture %s: %f, enhanced %s: %f" % (name, r["mixture"][k], name, r["enhanced"][k]) in out
    enh = np.stack([r["enhanced"] for r in table])
    mixs = np.stack([r["mixture"] for r in table])
    for k, name in enumerate(ev.METRICS):
        assert "mean enhanced %s:  %s std enhanced %s:  %s" % (name, np.mean(enh[:, k]), name, np.std(enh[:, k])) in out
        assert "mean mixture %s:  %s std mixture %s:  %s" % (name, np.mean(mixs[:, k]), name, np.std(mixs[:, k])) in out
    assert "pesq:" not in out


def test_evaluator_skips_the_samples_of_a_failing_device_batch(tree, monkeypatch, capsys):
    from avse_amd import ops, speech_enhancement_evaluator as ev
    root, _ = tree

    from avse_amd import _lib
    error = [_lib.AvseError("no 8 kHz today")]

    def fake(ref, deg, sample_rate=16000):
        if sample_rate == 8000:
            raise error[0]
        return reference_eval_pairs(ref, deg, sample_rate)

    monkeypatch.setattr(ops, "eval_pairs", fake)
    table = ev.evaluate(str(root), batch=64)
    out = capsys.readouterr().out
    assert sorted(r["sample"] for r in table) == ["a_clip", "b_clip", "y_stereo"]
    assert out.count("failed to evaluate pesq (") == 2 and "no 8 kHz today" in out
    assert all(r["enhanced"].shape == (5,) and r["mixture"].shape == (5,) for r in table)
    # only the binding's refusals are skipped: any other error (a device error among them) ends the run
    error[0] = RuntimeError("HIP error")
    with pytest.raises(RuntimeError, match="HIP error"):
        ev.evaluate(str(root), batch=64)


def test_evaluator_pesq_wrapper_and_cli(tree, monkeypatch, capsys, tmp_path_factory):
    from avse_amd import ops, speech_enhancement_evaluator as ev
    root, _ = tree
    stub = tmp_path_factory.mktemp("bin") / "pesq"
    stub.write_text("#!/bin/sh\n[ \"$1\" = +16000 ] || exit 3\n[ -f \"$2\" ] && [ -f \"$3\" ] || exit 4\n"
                    "echo 'P.862 Prediction (Raw MOS, MOS-LQO):  = 2.345\t2.101'\n")
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    d = root / "s1" / "a_clip"
    assert ev.pesq(str(stub), str(d / "source.wav"), str(d / "enhanced.wav")) == (2.345, 2.101)
    monkeypatch.setattr(ops, "eval_pairs", reference_eval_pairs)
    seen = []
    monkeypatch.setattr(ev, "evaluate", lambda *a, _e=ev.evaluate, **k: seen.append(a) or _e(*a, **k))
    ev.main([str(root), str(stub)])
    out = capsys.readouterr().out
    assert seen == [(str(root), str(stub))]
    assert out.count("mixture pesq: 2.345000, enhanced pesq: 2.345000") == 4
    four = [2.345] * 4
    assert "mean enhanced pesq:  %s std enhanced pesq:  %s" % (np.mean(four), np.std(four)) in out
    assert "mean mixture pesq:  %s std mixture pesq:  %s" % (np.mean(four), np.std(four)) in out
    ev.main([str(root)])
    assert "pesq:" not in capsys.readouterr().out


def test_root_shim_imports_the_evaluator():
    import importlib.util
    spec = importlib.util.spec_from_file_location("root_evaluator_shim", os.path.join(ROOT, "speech_enhancement_evaluator.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from avse_amd import speech_enhancement_evaluator as ev
    assert mod.main is ev.main and mod.evaluate is ev.evaluate
