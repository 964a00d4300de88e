"""CPU tests of avse_eval_pairs_ext (ESTOI, STOI at every rate): what the C-ABI decides on the host, the float64
reference's self-checks (tests/eval_ext_ref.py), the conditions on the GPU tests' inputs, the by-phase resampling table
under AddressSanitizer / UndefinedBehaviorSanitizer (a stand-alone program, tests/native/eval_phase_taps_check.cpp), and
the evaluator's extended mode with the device call replaced by the reference."""
import ctypes
import functools
import json
import os
import shutil
import subprocess
import wave

import numpy as np
import pytest

import eval_ext_ref as E
import eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-visual-speech-enhancement_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- ABI ---------------------------------------------------------------------------------------------------------
def test_library_exports_avse_eval_pairs_ext():
    from avse_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "avse_eval_pairs_ext") and "avse_eval_pairs_ext" in _lib.SIGNATURES
    assert lib.avse_abi_version() == 3 and _lib.AVSE_EVAL_NMETRICS == 5          # additive
    assert _lib.AVSE_EVAL_NMETRICS_EXT == len(_lib.EVAL_METRIC_NAMES_EXT) == E.NMETRICS == 6
    assert _lib.EVAL_METRIC_NAMES_EXT == _lib.EVAL_METRIC_NAMES + ("estoi",) and _lib.AVSE_EVAL_ANY_RATE == 1
    header = open(_lib.HEADER_PATH).read()
    assert "#define AVSE_EVAL_NMETRICS_EXT 6" in header and "AVSE_EVAL_ANY_RATE = 1" in header
    assert "AVSE_EVAL_ESTOI = 5" in header and "#define AVSE_EVAL_NMETRICS 5" in header


def test_bad_arguments_are_rejected_without_gpu_work():
    from avse_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.avse_eval_pairs_ext
    assert f(None, None, None, None, 1, 100, 16000, 0, None, None) == 1 and b"NULL" in lib.avse_last_error()
    for hole in range(5):                       # each pointer argument NULL in turn
        args = [p, p, p, p, p]
        args[hole] = None
        rc = f(args[0], args[1], args[2], args[3], 1, 100, 16000, 1, args[4], None)
        assert rc == 1 and b"NULL" in lib.avse_last_error(), hole
    # a non-NULL context and buffers, bad extents: refused before the context is touched (the pointers are never read)
    for flags in (0, 1):
        for n_pairs, sr in ((0, 16000), (-3, 16000), (1, 7999), (1, 48001), (1, 0)):
            assert f(p, p, p, p, n_pairs, 100, sr, flags, p, None) == 1 and lib.avse_last_error(), (n_pairs, sr)
        for n_pairs, total in ((1, -1), (1, (1 << 24) + 1), (3, 3 * (1 << 24) + 1)):
            rc = f(p, p, p, p, n_pairs, total, 44100, flags, p, None)
            assert rc == 1 and b"total_samples" in lib.avse_last_error(), (n_pairs, total)
    for flags in (2, 3, 4, 1 << 30, -1):        # an unknown flag bit
        assert f(p, p, p, p, 1, 100, 16000, flags, p, None) == 1 and b"flag" in lib.avse_last_error(), flags


def test_eval_pairs_ext_refuses_bad_input_on_the_host():
    from avse_amd import _lib, ops
    s = np.zeros(100, np.float32)
    with pytest.raises(TypeError):
        ops.eval_pairs_ext([np.zeros((100, 2), np.float32)], [s], 44100)
    with pytest.raises(TypeError):
        ops.eval_pairs_ext([s.astype(np.int32)], [s], 44100)
    with pytest.raises(ValueError):
        ops.eval_pairs_ext([s, s], [s], 44100)
    with pytest.raises(ValueError):
        ops.eval_pairs_ext([s], [s], 48001)
    with pytest.raises(_lib.AvseError, match="AVSE_ERR_INVALID"):
        ops.eval_pairs_ext([s, np.zeros(0, np.float32)], [s, s], 44100, any_rate=False)
    import torch
    with pytest.raises(TypeError):              # the packed form lives on the device
        ops.eval_pairs_ext((torch.zeros(100), np.array([0, 100], np.int64)), torch.zeros(100), 44100)


# ---- the reference's self-checks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", [(100, 441), (200, 441), (10000, 16001)])
def test_reference_resampling_at_large_ratios_is_resample_poly(up, down):
    """eval_ref.resample is general: at the ratios of 44100, 22050 and 16001 Hz it is scipy's resample_poly."""
    from scipy.signal import resample_poly
    x = np.random.default_rng(up + down).uniform(-1.0, 1.0, 5003)
    got, want = R.resample(x, up, down), resample_poly(x, up, down)
    assert got.shape == want.shape == (-(-5003 * up // down),)
    err = np.abs(got - want).max() / np.abs(x).max()
    print(f"{up}/{down}: max |reference - resample_poly| = {err:.2e} of the peak (gate 1e-12)")
    assert err <= 1e-12


@functools.lru_cache(maxsize=None)
def _bands(seed, snr_db=5.0):
    s, y = R.speech_like(seed, 44100, 44100, snr_db)
    X, Y, K = E.band_envelopes(s, y, 44100)
    assert X is not None and K - 1 >= E.N_SEG
    return s, y, X, Y


def test_reference_estoi_properties():
    s, y, X, Y = _bands(31)
    assert abs(E.estoi(s, s, 44100) - 1.0) <= 1e-12
    d = E.estoi(s, y, 44100)
    assert d == E.estoi_of_bands(X, Y) and -1.0 <= d <= 1.0 and d < 0.999
    # scale of the degraded signal and the order of the two signals do not matter
    assert abs(E.estoi(s, 3.7 * y.astype(np.float64), 44100) - d) <= 1e-12
    assert abs(E.estoi_of_bands(X, Y) - E.estoi_of_bands(Y, X)) <= 1e-12
    # as signals, where both orders keep the same frames (the mask is the first signal's): stationary noise
    a, b = R.speech_like(32, 22050, 44100, 10.0, stationary=True)
    assert E.band_envelopes(a, b, 44100)[2] == E.band_envelopes(b, a, 44100)[2] == E.band_envelopes(a, a, 44100)[2]
    assert abs(E.estoi(a, b, 44100) - E.estoi(b, a, 44100)) <= 1e-12
    # bounded: opposite envelopes reach the lower end
    lo = E.estoi_of_bands(X, X.max() - X)
    assert -1.0 - 1e-12 <= lo <= 1.0 + 1e-12
    rng = np.random.default_rng(7)
    for _ in range(5):
        v = E.estoi_of_bands(rng.uniform(0.0, 1.0, (15, 40)), rng.uniform(0.0, 1.0, (15, 40)))
        assert -1.0 <= v <= 1.0


def test_reference_estoi_stays_finite_on_all_zero_bands():
    """Bands that are exactly zero over a whole segment normalise to zero rows (0 / (0 + eps)), nothing divides by 0."""
    _, _, X, _ = _bands(31)
    Z = X.copy()
    Z[[0, 7, 14]] = 0.0
    v = E.estoi_of_bands(Z, Z)
    assert np.isfinite(v) and abs(v - 1.0) <= 1e-12
    assert np.isfinite(E.estoi_of_bands(np.zeros((15, 33)), np.zeros((15, 33))))
    assert np.isfinite(E.estoi_of_bands(Z, Z, dtype=np.float32))


def test_reference_agrees_with_eval_ref_where_both_compute():
    s, y = R.speech_like(3, 12000, 16000, 5.0)
    a, b = R.eval_pair(s, y, 16000), E.eval_pair_ext(s, y, 16000)
    assert np.array_equal(a, b[:5]) and np.isfinite(b[E.ESTOI])
    a32, b32 = R.eval_pair(s, y, 16000, np.float32), E.eval_pair_ext(s, y, 16000, np.float32)
    assert np.array_equal(a32, b32[:5]) and 0.0 < abs(b32[E.ESTOI] - b[E.ESTOI]) < 1e-6
    assert np.isnan(E.eval_pair_ext(np.zeros(0), np.zeros(0))).all()
    assert R.MAX_RATIO == 24 and np.isnan(R.eval_pair(s[:5000], y[:5000], 44100)[R.STOI])    # eval_ref is untouched


def test_gpu_case_inputs_keep_the_mask_margin_and_their_frame_counts():
    """Conditions on the GPU tests' inputs (tests/test_gpu_eval_ext.py), asserted in the float64 reference alone: no
    frame energy within 0.01 dB of max - 40, and the K of the table (M = K - 1 on both sides of 30 per path)."""
    for name, sr, s, y, K in E.cases():
        margin = E.mask_margin(s, sr)
        row = E.eval_pair_ext(s, y, sr)
        print(f"{name}: mask margin {margin:.3f} dB, K {row[R.STOI_KEPT]:.0f}, STOI {row[R.STOI]:.6f}, "
              f"ESTOI {row[E.ESTOI]:.6f}")
        assert margin >= R.MASK_MARGIN_DB, (name, margin)
        assert row[R.STOI_KEPT] == K, (name, row[R.STOI_KEPT], K)
        assert bool(np.isfinite(row[R.STOI])) == bool(np.isfinite(row[E.ESTOI])) == (K - 1 >= 30), name
        if np.isfinite(row[E.ESTOI]):
            assert -1.0 <= row[E.ESTOI] <= 1.0
    lengths = {(sr, n): -(-n * R.ratio(sr)[0] // R.ratio(sr)[1]) for _, sr, n, *_ in E.CASES}
    assert lengths[(22050, 9031)] == lengths[(16001, 6554)] == 4096 and lengths[(44100, 18063)] == 4096


# ---- the by-phase table, sanitized ----------------------------------------------------------------------------------
def test_phase_taps_sanitized(tmp_path):
    from scipy.signal import firwin
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host sources are built with the kernels' compiler")
    exe = str(tmp_path / "eval_phase_taps_check")
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++20", "-O2", "-g", "-ffp-contract=off",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tests", "native", "eval_phase_taps_check.cpp"),
                         os.path.join(CSRC, "eval_tables.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"exit status {run.returncode}\n{run.stderr[-4000:]}"
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    got = json.loads(run.stdout)
    assert sorted(got) == sorted(["100_441", "200_441", "400_441", "10000_16001", "10000_47999", "10000_8001"])
    for key, g in got.items():
        up, down = (int(v) for v in key.split("_"))
        H = 10 * max(up, down)
        T = 2 * H // up + 1
        assert (g["H"], g["T"], g["rows"]) == (H, T, up * T), key
        # the walk over the table is the definition's sum, term for term
        assert g["checked"] > 600 and g["worst"] == 0.0, (key, g["worst"])
        # row `phase` starts with a zero exactly when phase + (T - 1) up passes 2H (firwin's own zeros aside)
        assert g["zeros"] >= up - 1 - (2 * H) % up, key
        want = firwin(2 * H + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
        taps = np.array(g["taps_every_1009"])
        assert taps.shape == want[::1009].shape and np.abs(taps - want[::1009]).max() <= 1e-12, key
    g = got["100_441"]
    h, table = np.array(g["taps"]), np.array(g["table"]).reshape(100, g["T"])
    assert g["T"] == 89 and h.size == 8821
    assert np.abs(h - firwin(8821, 1.0 / 441, window=("kaiser", 5.0)) * 100).max() <= 1e-12
    for phase in range(100):
        for q in range(89):
            i = phase + 100 * (88 - q)
            assert table[phase, q] == (h[i] if i <= 8820 else 0.0), (phase, q)


# ---- the evaluator module ------------------------------------------------------------------------------------------
def write_wav(path, data, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(data, dtype="<i2").tobytes())


@pytest.fixture
def tree(tmp_path):
    """<dir>/<speaker>/<sample>/{source,enhanced,mixture}.wav: two speakers, three 16 kHz samples and one at 8 kHz."""
    sigs = {}
    for k, (spk, smp, sr, n) in enumerate((("s1", "b_clip", 16000, 9000), ("s1", "a_clip", 16000, 12000),
                                           ("s2", "x_clip", 8000, 6000), ("s2", "y_clip", 16000, 10000))):
        d = tmp_path / spk / smp
        d.mkdir(parents=True)
        src, mix = R.speech_like(60 + k, n, sr, 0.0)
        _, enh = R.speech_like(60 + k, n, sr, 10.0)
        src, mix, enh = src.astype(np.int16), mix.astype(np.int16), enh[:n - 100].astype(np.int16)   # enhanced is shorter
        for name, sig in (("source", src), ("mixture", mix), ("enhanced", enh)):
            write_wav(d / (name + ".wav"), sig, sr)
        sigs[(spk, smp)] = (sr, src, enh, mix)
    return tmp_path, sigs


def reference_eval_pairs_ext(ref, deg, sample_rate=16000, any_rate=True):
    import torch
    assert any_rate
    return torch.from_numpy(E.eval_pairs_ext(ref, deg, sample_rate))


def test_evaluator_extended_prints_estoi_and_returns_rows_of_six(tree, monkeypatch, capsys):
    from avse_amd import ops, speech_enhancement_evaluator as ev
    root, sigs = tree
    calls = []

    def fake(ref, deg, sample_rate=16000, any_rate=True):
        calls.append((len(ref), sample_rate))
        return reference_eval_pairs_ext(ref, deg, sample_rate, any_rate)

    def never(*a, **k):
        raise AssertionError("the extended evaluator calls ops.eval_pairs_ext only")

    monkeypatch.setattr(ops, "eval_pairs_ext", fake)
    monkeypatch.setattr(ops, "eval_pairs", never)
    table = ev.evaluate(str(root), batch=2, extended=True)
    out = capsys.readouterr().out
    assert sorted(calls) == sorted([(2, 8000), (4, 16000), (2, 16000)])
    assert sorted(r["sample"] for r in table) == ["a_clip", "b_clip", "x_clip", "y_clip"]
    names = ev.METRICS + ("estoi",)
    slots = (0, 1, 2, 3, 5)
    lines = out.splitlines()
    for r in table:
        sr, src, enh, mix = sigs[(r["speaker"], r["sample"])]
        n = min(src.size, enh.size)
        assert r["enhanced"].shape == r["mixture"].shape == (6,)
        assert np.array_equal(r["enhanced"], E.eval_pair_ext(src[:n], enh[:n], sr), equal_nan=True)
        assert np.array_equal(r["mixture"], E.eval_pair_ext(src, mix, sr), equal_nan=True)
        per = ["mixture %s: %f, enhanced %s: %f" % (name, r["mixture"][k], name, r["enhanced"][k])
               for name, k in zip(names, slots)]
        at = lines.index(per[0])
        assert lines[at:at + 5] == per            # the estoi line follows stoi's
    enh = np.stack([r["enhanced"] for r in table])
    mixs = np.stack([r["mixture"] for r in table])
    means = [ln for ln in lines if ln.startswith("mean ")]
    want = []
    for name, k in zip(names, slots):
        want.append("mean enhanced %s:  %s std enhanced %s:  %s" % (name, np.mean(enh[:, k]), name, np.std(enh[:, k])))
        want.append("mean mixture %s:  %s std mixture %s:  %s" % (name, np.mean(mixs[:, k]), name, np.std(mixs[:, k])))
    assert means == want
    assert "stoi_kept" not in out and "pesq:" not in out


def test_evaluator_default_never_calls_eval_pairs_ext(tree, monkeypatch, capsys):
    from avse_amd import ops, speech_enhancement_evaluator as ev
    import torch
    root, _ = tree

    def never(*a, **k):
        raise AssertionError("ops.eval_pairs_ext called without --extended")

    monkeypatch.setattr(ops, "eval_pairs_ext", never)
    monkeypatch.setattr(ops, "eval_pairs", lambda ref, deg, sample_rate=16000:
                        torch.from_numpy(R.eval_pairs(ref, deg, sample_rate)))
    table = ev.evaluate(str(root))
    assert all(r["enhanced"].shape == (5,) for r in table) and "estoi" not in capsys.readouterr().out
    ev.main([str(root)])
    assert "estoi" not in capsys.readouterr().out


def test_cli_flag_extended(tree, monkeypatch, capsys):
    from avse_amd import ops, speech_enhancement_evaluator as ev
    root, _ = tree
    monkeypatch.setattr(ops, "eval_pairs_ext", reference_eval_pairs_ext)
    seen = []
    monkeypatch.setattr(ev, "evaluate", lambda *a, _e=ev.evaluate, **k: seen.append((a, k)) or _e(*a, **k))
    ev.main(["--extended", str(root)])
    assert seen == [((str(root), None), {"extended": True})]
    out = capsys.readouterr().out
    assert sum(ln.startswith("mixture estoi: ") for ln in out.splitlines()) == 4
    assert "mean enhanced estoi: " in out and "mean mixture estoi: " in out
