"""GPU tests of avse_eval_pairs_ext (ops.eval_pairs_ext): ESTOI, and STOI at every rate from 8 to 48 kHz, against the
float64 reference tests/eval_ext_ref.py.

Gates (none of them taken from what the device gives):
  K                    equal exactly; NaN and +-inf in the same slots
  SNR, SI-SDR, seg SNR 1e-9 dB: at most 48,000 non-negative float64 terms, so a reordered sum moves by at most
                       n 2^-53 relative, under 5e-11 dB through the logarithm (tests/test_gpu_eval.py)
  STOI, ESTOI          each 8 x the largest |float32 - float64| of the reference over this file's cases (its framing,
                       FFT, band and segment arithmetic in float32), at most 1e-5: the fourth decimal must not move
The conditions on the inputs (mask margin, frame counts) are asserted on the CPU, in tests/test_eval_ext_host.py."""
import functools

import numpy as np
import pytest
import torch

import eval_ext_ref as E
import eval_ref as R

pytestmark = pytest.mark.gpu

TOL_DB = 1e-9
CEILING = 1e-5
BIG_RATES = (44100, 22050, 11025, 16001, 47999)


@functools.lru_cache(maxsize=None)
def table():
    """{name: (sr, clean, degraded, float64 row, float32-mode row)} of eval_ext_ref.CASES."""
    out = {}
    for name, sr, s, y, _ in E.cases():
        r64 = E.eval_pair_ext(s, y, sr)
        r64.setflags(write=False)
        out[name] = (sr, s, y, r64, E.eval_pair_ext(s, y, sr, dtype=np.float32))
    return out


@functools.lru_cache(maxsize=None)
def ragged():
    cases = R.ragged_cases()
    ref64 = np.stack([E.eval_pair_ext(s, y, 16000) for _, s, y in cases])
    ref32 = np.stack([E.eval_pair_ext(s, y, 16000, dtype=np.float32) for _, s, y in cases])
    ref64.setflags(write=False)
    return cases, ref64, ref32


@functools.lru_cache(maxsize=None)
def gates():
    """{slot: gate} for STOI and ESTOI: 8 x the largest |float32 - float64| of the reference over every case of this
    file, at most 1e-5."""
    r64 = np.concatenate([np.stack([v[3] for v in table().values()]), ragged()[1]])
    r32 = np.concatenate([np.stack([v[4] for v in table().values()]), ragged()[2]])
    assert np.array_equal(r64[:, R.STOI_KEPT], r32[:, R.STOI_KEPT], equal_nan=True)
    out = {}
    for slot in (R.STOI, E.ESTOI):
        ok = np.isfinite(r64[:, slot])
        assert np.array_equal(ok, np.isfinite(r32[:, slot])) and ok.any()
        worst = float(np.abs(r32[ok, slot] - r64[ok, slot]).max())
        assert worst > 0.0
        out[slot] = min(8.0 * worst, CEILING)
        print(f"slot {slot}: float32 yardstick {worst:.3e}, gate {out[slot]:.3e}")
    return out


def check_rows(names, got, want, slots=range(6)):
    assert got.shape == want.shape and got.shape[1] == 6
    gate = gates()
    for name, g, w in zip(names, got, want):
        print(f"{name}: device {g.tolist()} reference {w.tolist()}")
        assert np.array_equal(np.isnan(g), np.isnan(w)), (name, g, w)
        assert np.array_equal(np.isposinf(g), np.isposinf(w)) and np.array_equal(np.isneginf(g), np.isneginf(w)), (name, g, w)
        if not np.isnan(w[R.STOI_KEPT]):
            assert g[R.STOI_KEPT] == w[R.STOI_KEPT], (name, g, w)
        for slot in (R.SNR, R.SI_SDR, R.SEG_SNR):
            if np.isfinite(w[slot]) and slot in slots:
                print(f"  slot {slot}: |device - reference| = {abs(g[slot] - w[slot]):.3e} dB (gate {TOL_DB:.0e})")
                assert abs(g[slot] - w[slot]) <= TOL_DB, (name, slot, g[slot], w[slot])
        for slot, label in ((R.STOI, "STOI"), (E.ESTOI, "ESTOI")):
            if np.isfinite(w[slot]) and slot in slots:
                print(f"  {label}: |device - reference| = {abs(g[slot] - w[slot]):.3e} (gate {gate[slot]:.3e})")
                assert abs(g[slot] - w[slot]) <= gate[slot], (name, label, g[slot], w[slot], gate[slot])


def bits(t):
    return t.cpu().numpy().view(np.uint64)


def of_rate(sr):
    return [(name, v) for name, v in table().items() if v[0] == sr]


@pytest.mark.parametrize("sr", BIG_RATES)
def test_large_ratio_rates_in_one_ragged_launch(gpu, sr):
    """Every case of one rate in one ragged call: at 44100 the speech pair, M = 29 / 30 / 31 and the no-frame pair."""
    from avse_amd import ops
    rows = of_rate(sr)
    assert len(rows) >= 1 and max(R.ratio(sr)) > R.MAX_RATIO
    got = ops.eval_pairs_ext([v[1] for _, v in rows], [v[2] for _, v in rows], sr)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (len(rows), 6)
    check_rows([n for n, _ in rows], got.cpu().numpy(), np.stack([v[3] for _, v in rows]))


def test_estoi_on_the_existing_resampling_path(gpu):
    from avse_amd import ops
    for sr in (16000, 8000):
        (name, v), = of_rate(sr)
        for any_rate in (True, False):
            got = ops.eval_pairs_ext([v[1]], [v[2]], sr, any_rate=any_rate)
            check_rows([name], got.cpu().numpy(), v[3][None])
    cases, ref64, _ = ragged()
    got = ops.eval_pairs_ext([s for _, s, _ in cases], [y for _, _, y in cases], 16000)
    assert tuple(got.shape) == (len(cases), 6)
    check_rows([n for n, _, _ in cases], got.cpu().numpy(), ref64)
    finite = np.isfinite(ref64[:, E.ESTOI])
    assert finite.sum() >= 4 and abs(ref64[[n for n, _, _ in cases].index("ragged_16000"), E.ESTOI] - 1.0) <= 1e-12


def test_slots_0_to_4_are_the_default_calls_bits(gpu):
    from avse_amd import ops
    cases, _, _ = ragged()
    groups = [(16000, [s for _, s, _ in cases], [y for _, _, y in cases])]
    for k, sr in enumerate((8000, 10000, 48000)):
        s, y = R.speech_like(430 + k, sr, sr, 5.0)
        groups.append((sr, [s], [y]))
    for sr, S, Y in groups:
        want = ops.eval_pairs(S, Y, sr)
        for any_rate in (True, False):
            got = ops.eval_pairs_ext(S, Y, sr, any_rate=any_rate)
            assert torch.equal(bits_t(got[:, :5]), bits_t(want)), (sr, any_rate)
        assert torch.isfinite(got[:, 5]).any()
    # 44100 without the flag: the default call's refusal of STOI, and NaN for ESTOI
    _, s, y, _, _ = table()["speech_44100"]
    want = ops.eval_pairs([s], [y], 44100)
    got = ops.eval_pairs_ext([s], [y], 44100, any_rate=False)
    assert torch.equal(bits_t(got[:, :5]), bits_t(want))
    assert torch.isnan(got[0, 3]) and got[0, 4] == 0.0 and torch.isnan(got[0, 5])
    both = ops.eval_pairs_ext([s], [y], 44100, any_rate=True)
    assert torch.equal(bits_t(both[:, :3]), bits_t(want[:, :3])) and torch.isfinite(both[0, 3:]).all()


def bits_t(t):
    """The float64 tensor's bit patterns (torch.equal on the values would call two NaNs different)."""
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("sr", (44100, 16000))
def test_batch_invariance_and_repeatability(gpu, sr):
    """A pair's six numbers are the same bits alone, inside the batch, in the reversed batch, at an odd element offset
    of the packed form, and in a second call."""
    from avse_amd import ops
    if sr == 44100:
        names = [n for n, _ in of_rate(sr)]
        S, Y = [v[1] for _, v in of_rate(sr)], [v[2] for _, v in of_rate(sr)]
    else:
        cases = ragged()[0][4:10]
        names, S, Y = [n for n, _, _ in cases], [s for _, s, _ in cases], [y for _, _, y in cases]
    full = bits(ops.eval_pairs_ext(S, Y, sr))
    assert np.array_equal(full, bits(ops.eval_pairs_ext(S, Y, sr)))
    assert np.array_equal(full, bits(ops.eval_pairs_ext(S[::-1], Y[::-1], sr))[::-1])
    for u, name in enumerate(names):
        assert np.array_equal(bits(ops.eval_pairs_ext([S[u]], [Y[u]], sr))[0], full[u]), name
    pad = np.zeros(3, np.float32)
    rp = torch.from_numpy(np.concatenate([pad] + S)).cuda()
    dp = torch.from_numpy(np.concatenate([pad] + Y)).cuda()
    off = 3 + np.concatenate([[0], np.cumsum([s.size for s in S])]).astype(np.int64)
    assert np.array_equal(bits(ops.eval_pairs_ext((rp, off), dp, sr)), full)


def test_table_cache_keeps_the_two_filters_of_a_rate_apart(gpu):
    """The context keeps four table sets by (rate, large-ratio filter): a default call and an any-rate call at 44100
    alternate, then five rates in a row turn the cache over; every result is what the same call gives on its own."""
    from avse_amd import ops
    _, s, y, r64, _ = table()["speech_44100"]
    first = ops.eval_pairs([s], [y], 44100)
    ext = ops.eval_pairs_ext([s], [y], 44100, any_rate=True)
    again = ops.eval_pairs([s], [y], 44100)
    assert torch.equal(bits_t(first), bits_t(again)) and torch.isnan(again[0, 3]) and again[0, 4] == 0.0
    check_rows(["speech_44100"], ext.cpu().numpy(), r64[None])
    names = ("speech_22050", "speech_11025", "speech_16001", "speech_47999", "speech_16000")
    alone = {}
    for name in names + ("speech_44100",):
        sr, s, y, r64, _ = table()[name]
        alone[name] = ops.eval_pairs_ext([s], [y], sr)
        check_rows([name], alone[name].cpu().numpy(), r64[None])
    assert torch.equal(bits_t(alone["speech_44100"]), bits_t(ext))
    for name in names[::-1]:                                    # each of these was replaced in the meantime
        sr, s, y, _, _ = table()[name]
        assert torch.equal(bits_t(ops.eval_pairs_ext([s], [y], sr)), bits_t(alone[name])), name
    _, s, y, _, _ = table()["speech_44100"]
    assert torch.equal(bits_t(ops.eval_pairs([s], [y], 44100)), bits_t(first))


def _raw_ext(rp, dp, off_d, out, sr, total, flags):
    from avse_amd import _lib
    ctx = _lib.context(rp.device)
    _lib.check(_lib.load().avse_eval_pairs_ext(ctx.handle, _lib.ptr(rp), _lib.ptr(dp), _lib.ptr(off_d),
                                               off_d.numel() - 1, int(total), sr, flags, _lib.ptr(out),
                                               _lib.stream_handle(rp.device)), "avse_eval_pairs_ext")


def test_eval_pairs_ext_in_a_captured_graph(gpu):
    """After one call of the same size, rate and flags (scratch and tables exist), avse_eval_pairs_ext is captured into
    a graph and replayed on new data in the same buffers: no allocation, no synchronisation, the direct call's bits."""
    from avse_amd import _lib, ops
    rows = of_rate(44100)[:3]
    S, Y = [v[1] for _, v in rows], [v[2] for _, v in rows]
    off = np.concatenate([[0], np.cumsum([s.size for s in S])]).astype(np.int64)
    rp, dp = torch.from_numpy(np.concatenate(S)).cuda(), torch.from_numpy(np.concatenate(Y)).cuda()
    off_d = torch.from_numpy(off).cuda()
    out = torch.zeros((3, 6), dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _raw_ext(rp, dp, off_d, out, 44100, off[-1], _lib.AVSE_EVAL_ANY_RATE)     # warm: scratch, tables
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    direct = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _raw_ext(rp, dp, off_d, out, 44100, off[-1], _lib.AVSE_EVAL_ANY_RATE)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits_t(out), bits_t(direct)) and torch.equal(bits_t(direct), bits_t(ops.eval_pairs_ext(S, Y, 44100)))
    dp.copy_(rp)                 # new data in the captured buffers: deg == ref
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = ops.eval_pairs_ext(S, S, 44100)
    assert torch.equal(bits_t(out), bits_t(want))
    assert torch.isposinf(out[:, 0]).all() and abs(float(out[0, 5]) - 1.0) <= 1e-12


def test_evaluator_extended_on_the_device(gpu, tmp_path, capsys):
    """speech_enhancement_evaluator.evaluate(extended=True) over three samples at 44.1 kHz, through the real ops."""
    from scipy.io import wavfile
    from avse_amd import speech_enhancement_evaluator as ev
    want = {}
    for k, (smp, n) in enumerate((("b", 40000), ("a", 44100), ("c", 36000))):
        d = tmp_path / "spk" / smp
        d.mkdir(parents=True)
        src, mix = R.speech_like(440 + k, n, 44100, 0.0)
        _, enh = R.speech_like(440 + k, n, 44100, 10.0)
        for name, sig in ((smp, src), (smp + " cut", src[:n - 77])):
            margin = E.mask_margin(sig, 44100)
            print(f"{name}: mask margin {margin:.3f} dB")
            assert margin >= R.MASK_MARGIN_DB, (name, margin)
        for name, sig in (("source", src), ("mixture", mix), ("enhanced", enh[:n - 77])):
            wavfile.write(str(d / (name + ".wav")), 44100, sig.astype(np.int16))
        want[smp] = (E.eval_pair_ext(src[:n - 77], enh[:n - 77], 44100), E.eval_pair_ext(src, mix, 44100))
    rows = ev.evaluate(str(tmp_path), batch=64, extended=True)
    assert [r["sample"] for r in rows] == ["a", "b", "c"] and all(r["sample_rate"] == 44100 for r in rows)
    for r in rows:
        assert r["enhanced"].shape == (6,)
        check_rows([r["sample"] + "/enhanced", r["sample"] + "/mixture"], np.stack([r["enhanced"], r["mixture"]]),
                   np.stack(want[r["sample"]]))
    assert np.isfinite(np.stack([r["enhanced"] for r in rows])[:, [3, 5]]).all()
    out = capsys.readouterr().out
    assert sum(ln.startswith("mixture estoi: ") for ln in out.splitlines()) == 3 and "mean enhanced estoi: " in out
