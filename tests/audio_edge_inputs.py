"""Inputs, oracle expectations and error measures shared by the audio edge tests (test_audio_edge_inputs.py on the
CPU, test_gpu_stft_edges.py / test_gpu_istft_edges.py on the device).  Not collected by pytest.

conftest.synth_audio has a 26-45 dB dynamic range, so librosa's top_db = 80 clamp never touches it and a kernel that
ignored top_db, took the maximum over the kept frames only or read another utterance's maximum would still match the
oracle.  `wide` spreads one utterance over > 100 dB; `clamp_conditions` asserts, on the float64 oracle alone, that an
input does tell these semantics apart.  Every input a device test uses is built here from a fixed seed, so the CPU
module checks the very arrays the device sees.
"""
import functools

import numpy as np

from conftest import synth_audio
from oracle import librosa_ref as R

DB_MAX = 1e-3          # tests/test_gpu_stft.py
DB_RMS = 1e-4
STFT_REL = 2e-6        # of the utterance's peak |X|; for `wide` inputs also of each frame's own peak
WAVE_REL = 1e-4        # waveform relative RMS, whole utterance and per block of `hop` samples

DEFAULT_BANK = dict(sample_rate=16000, n_mels=80, fmin=0.0, fmax=8000.0)
BANK17 = dict(sample_rate=16000, n_mels=17, fmin=0.0, fmax=8000.0)     # wider than the 24-bin rows: generic band loop
BANK64 = dict(sample_rate=16000, n_mels=64, fmin=0.0, fmax=8000.0)
BANK64_7600 = dict(sample_rate=16000, n_mels=64, fmin=0.0, fmax=7600.0)


def wide(x, loud):
    """x [..., L] times a gain envelope: 1e-3 everywhere, 1e-4 on the first quarter, exactly 0 on the next eighth,
    1 on loud = (lo, hi).  float32.  The silent stretch holds +0.0 only (x * 0.0 is -0.0 for a negative sample): numpy's
    FFT of a frame of mixed +-0.0 returns -0.0 real parts in a few bins, for which np.angle is pi and librosa's phase
    -1, an accident of the FFT's signed zeros; of an all +0.0 frame it returns +0.0, the phase 1 of the rule "phase is
    1 where D == 0" that the kernels implement (|D|^2 > 0 ? D / |D| : 1)."""
    L = x.shape[-1]
    g = np.full(L, 1e-3)
    g[:L // 4] = 1e-4
    g[L // 4:L // 4 + L // 8] = 0.0
    g[loud[0]:loud[1]] = 1.0
    return (x * g + 0.0).astype(np.float32)


def ladder(n):
    """Per-utterance gains 10^(-(u mod 7) / 2): 0, -10, ... -60 dB, so neighbouring utterances' floors differ."""
    return (10.0 ** (-(np.arange(n) % 7) / 2.0))[:, None]


def level(x, n_fft, hop, bank=None):
    """x [U, L] with every utterance scaled so that its oracle dB maximum is the batch's median.  synth_audio's
    harmonic (200-3000 Hz) lands in Slaney bands of very different weight, which moves an utterance's maximum by up
    to 12 dB; levelled, the ladder's 10-dB steps are what separates neighbouring floors."""
    mx = np.array([oracle_pre(xu, n_fft, hop, "reflect", bank or DEFAULT_BANK)[0].max() for xu in x])
    return (x * 10.0 ** ((np.median(mx) - mx) / 20.0)[:, None]).astype(np.float32)


def oracle_pre(x, n_fft, hop, pad_mode="reflect", bank=DEFAULT_BANK):
    """(mel dB before the top_db clamp [n_mels, T] float64, complex STFT [1 + n_fft // 2, T]) of one utterance: the
    chain of R.signal_to_spectrogram with the bank as a parameter."""
    D = R.stft(x, n_fft, hop, pad_mode=pad_mode)
    mag, _ = R.magphase(D)
    fb = R.mel_filterbank(bank["sample_rate"], n_fft, bank["n_mels"], bank["fmin"], bank["fmax"])
    return R.amplitude_to_db(fb @ mag, top_db=None), D


def clamp(pre, top_db=80.0):
    """librosa's clamp: the maximum over the WHOLE array."""
    return pre if top_db is None else np.maximum(pre, pre.max() - top_db)


def slices(db, spf):
    """[n_mels, T] -> [T // spf, n_mels, spf] (trailing frames dropped), as preprocess_audio_signal."""
    n = db.shape[1] // spf
    return np.stack([db[:, i * spf:(i + 1) * spf] for i in range(n)])


def clamp_conditions(pre, top_db=80.0, spf=0, silent=False, dropped=False):
    """The per-utterance conditions of a clamp test on the oracle dB `pre` (before the clamp); returns the figures.
    (How far the clamp moves the oracle is a condition on the case, in clamp_oracle: the ladder's -50 and -60 dB
    utterances sit so close to amin's -100 dB that their clamp is only 2-8 dB deep.)"""
    full = clamp(pre, top_db)
    share = float(np.mean(pre <= pre.max() - top_db))
    assert 0.10 <= share <= 0.70, f"clamped share {share}"
    vs_none = float(np.abs(full - pre).max())
    out = dict(share=share, vs_none=vs_none)
    if silent:
        out["silent"] = float(np.mean(pre == -100.0))
        assert out["silent"] > 0, "no element at exactly -100 dB before the clamp"
    if dropped:
        kept = pre[:, :(pre.shape[1] // spf) * spf]
        assert pre.max() > kept.max(), "the maximum is not in a dropped frame"
        out["vs_kept"] = float(np.abs(clamp(kept, top_db) - full[:, :kept.shape[1]]).max())
        assert out["vs_kept"] > 1.0, f"maximum over the kept frames only differs by {out['vs_kept']} dB"
    return out


def floors_differ(floors, pairs):
    """Utterance floors (max - top_db) of the given (u, v) neighbours differ by at least 5 dB."""
    worst = min(abs(floors[u] - floors[v]) for u, v in pairs)
    assert worst >= 5.0, f"two neighbouring utterances' floors are {worst} dB apart"
    return worst


# ------------------------------------------------------------------------------------------------------------
# clamp cases: name -> dict(x [U, L], n_fft, hop, spf, bank, top_db, check = utterances compared with the oracle,
# dropped / silent = per-utterance flags for clamp_conditions, pairs = neighbours whose floors must differ)
# ------------------------------------------------------------------------------------------------------------
SEG_U = 1100           # k_spec_seg: grid 2 x 256 CUs = 512 blocks, so blocks 0..75 walk 3 utterances, the rest 2
SEG_GRID = 512


def seg_spread():
    """128 utterances of the 1100: all of 24 three-utterance blocks (the first and last of them included) and of 28
    two-utterance blocks (first and last included) -> every block's first and last utterance and u, u + 512 pairs of
    both parities."""
    b3 = sorted(set(np.linspace(0, SEG_U - 2 * SEG_GRID - 1, 24).astype(int)))
    b2 = sorted(set(np.linspace(SEG_U - 2 * SEG_GRID, SEG_GRID - 1, 28).astype(int)))
    us = [b + SEG_GRID * k for b in b3 for k in range(3)] + [b + SEG_GRID * k for b in b2 for k in range(2)]
    pairs = [(u, u + SEG_GRID) for u in us if u + SEG_GRID in us]
    pairs += [(u, u + 1) for u in us if u + 1 in us]
    return sorted(us), pairs


@functools.lru_cache(maxsize=None)
def clamp_case(name):
    if name == "seg":                   # k_spec_seg (unsliced / sliced to 20), k_spec640 single chunk with RI
        x = level(wide(synth_audio(np.random.default_rng(101), SEG_U, 3200), (3080, 3200)), 640, 160) * ladder(SEG_U)
        us, pairs = seg_spread()
        return dict(x=x.astype(np.float32), n_fft=640, hop=160, spf=20, bank=DEFAULT_BANK, top_db=80.0, check=us,
                    dropped=[True] * SEG_U, silent=[False] * SEG_U, pairs=pairs)
    if name in ("seg17", "seg64"):      # k_spec640<false, *> single chunk: the banks of test_segment_kernel_other_banks
        x = clamp_case("seg")["x"][:40]
        # (top_db = 60, that test's value for the 17 bands, would clamp 0.85 of this input: 75 keeps a non-default value)
        bank, top_db = (BANK17, 75.0) if name == "seg17" else (BANK64, 80.0)
        x = (level(x, 640, 160, bank) * ladder(40)).astype(np.float32)   # levelled for this bank
        return dict(x=x, n_fft=640, hop=160, spf=20, bank=bank, top_db=top_db, check=list(range(40)),
                    dropped=[True] * 40, silent=[False] * 40, pairs=[(u, u + 1) for u in range(39)])
    if name in ("chunk640", "chunk640_17"):   # k_spec640 multi chunk + atomicMax + k_spec_clamp
        s = synth_audio(np.random.default_rng(102), 4, 48000)
        bank = BANK17 if name.endswith("17") else DEFAULT_BANK
        x = np.stack([wide(s[0], (47900, 48000)),      # the maximum in the dropped frame 300
                      wide(s[1], (23600, 24400)),      # mid-utterance
                      wide(s[2], (1000, 1800)),        # chunk 0
                      wide(s[3], (0, 0))])             # no burst
        x = (level(x, 640, 160, bank) * ladder(4)).astype(np.float32)
        return dict(x=x, n_fft=640, hop=160, spf=20, bank=bank, top_db=80.0, check=list(range(4)),
                    dropped=[True, False, False, False], silent=[True] * 4, pairs=[(0, 1), (1, 2), (2, 3)])
    if name == "seg533":                # k_spec533 single block
        x = level(wide(synth_audio(np.random.default_rng(103), 64, 3200), (3100, 3200)), 533, 133) * ladder(64)
        return dict(x=x.astype(np.float32), n_fft=533, hop=133, spf=24, bank=DEFAULT_BANK, top_db=80.0,
                    check=list(range(64)), dropped=[True] * 64, silent=[False] * 64,
                    pairs=[(u, u + 1) for u in range(63)])
    if name == "chunk533":              # k_spec533 multi chunk
        s = synth_audio(np.random.default_rng(404), 3, 32000)
        x = level(np.stack([wide(s[0], (31900, 32000)), wide(s[1], (15600, 16400)), wide(s[2], (1000, 1800))]),
                  533, 133) * ladder(3)
        return dict(x=x.astype(np.float32), n_fft=533, hop=133, spf=24, bank=DEFAULT_BANK, top_db=80.0,
                    check=list(range(3)), dropped=[True, False, False], silent=[True] * 3, pairs=[(0, 1), (1, 2)])
    if name == "dft666":                # k_spec_dft + k_spec_clamp at the 24-fps geometry, sliced to 19
        x = level(wide(synth_audio(np.random.default_rng(105), 3, 6400), (6300, 6400)), 666, 166) * ladder(3)
        return dict(x=x.astype(np.float32), n_fft=666, hop=166, spf=19, bank=DEFAULT_BANK, top_db=80.0,
                    check=list(range(3)), dropped=[True] * 3, silent=[True] * 3, pairs=[(0, 1), (1, 2)])
    if name == "dft401":                # k_spec_dft + k_spec_clamp, unsliced
        x = level(wide(synth_audio(np.random.default_rng(106), 3, 2000), (900, 1100)), 401, 100) * ladder(3)
        return dict(x=x.astype(np.float32), n_fft=401, hop=100, spf=0, bank=DEFAULT_BANK, top_db=80.0,
                    check=list(range(3)), dropped=[False] * 3, silent=[False] * 3, pairs=[(0, 1), (1, 2)])
    raise KeyError(name)


CLAMP_CASES = ["seg", "seg17", "seg64", "chunk640", "chunk640_17", "seg533", "chunk533", "dft666", "dft401"]
CLAMP_PAD_MODES = {"dft666": ("reflect", "constant"), "dft401": ("reflect", "constant")}


@functools.lru_cache(maxsize=None)
def clamp_oracle(name, pad_mode="reflect"):
    """{u: (pre-clamp dB, complex STFT)} for the case's checked utterances, with the conditions asserted."""
    c = clamp_case(name)
    out = {u: oracle_pre(c["x"][u], c["n_fft"], c["hop"], pad_mode, c["bank"]) for u in c["check"]}
    figures = [clamp_conditions(out[u][0], c["top_db"], c["spf"], c["silent"][u], c["dropped"][u]) for u in c["check"]]
    deepest = max(f["vs_none"] for f in figures)
    assert deepest > 10.0, f"the clamp moves the oracle by only {deepest} dB"
    floors = {u: out[u][0].max() - c["top_db"] for u in c["check"]}
    apart = floors_differ(floors, c["pairs"])
    return out, figures, apart


# the rewritten inputs of tests/test_gpu_stft.py's two dropped-frame tests
def sliced_segments_input():
    """test_sliced_segments_drop_last_frame_but_keep_its_max: 16 segments, the maximum in the dropped frame 20."""
    return wide(synth_audio(np.random.default_rng(2), 16, 3200), (3080, 3200))


def segments_533_input():
    """test_533_segments_match_oracle: 48 segments, the maximum in the dropped frame 24."""
    return wide(synth_audio(np.random.default_rng(12), 48, 3200), (3100, 3200))


# ------------------------------------------------------------------------------------------------------------
# geometry sweep of avse_spectrogram: (row, n_fft, hop, L, spf, bank, pad modes)
# ------------------------------------------------------------------------------------------------------------
BOTH = ("reflect", "constant")
REFLECT = ("reflect",)
SWEEP = (
    [("1", 640, 160, L, 0, DEFAULT_BANK, BOTH) for L in (321, 3360, 6560, 6720)]        # T = 3, 22, 42, 43
    + [("2", 640, 160, L, 0, DEFAULT_BANK, REFLECT) for L in (3361, 3333)]
    + [("4", 640, 100, 3200, 0, DEFAULT_BANK, REFLECT), ("4", 640, 320, 3333, 0, DEFAULT_BANK, REFLECT)]
    + [("5", 640, 160, 6720, 0, BANK17, REFLECT)]
    # T = 3, 25, 26, 50, 51 (chunks of 25: 6650 samples are exactly two chunks, one more sample adds a one-frame third)
    + [("6", 533, 133, L, 0, DEFAULT_BANK, BOTH) for L in (267, 3325, 3326, 6650, 6651)]
    + [("7", 533, 100, 3200, 0, DEFAULT_BANK, REFLECT)]
    + [("8", 666, 166, 6400, 19, DEFAULT_BANK, BOTH)]
    + [("9", 401, 100, 2000, 0, DEFAULT_BANK, BOTH), ("9", 400, 100, 1601, 0, DEFAULT_BANK, BOTH),
       ("9", 1024, 256, 4096, 0, DEFAULT_BANK, BOTH)])
SWEEP_FRAMES = {(640, 160, 321): 3, (640, 160, 3360): 22, (640, 160, 6560): 42, (640, 160, 6720): 43,
                (533, 133, 267): 3, (533, 133, 3325): 25, (533, 133, 3326): 26, (533, 133, 6650): 50,
                (533, 133, 6651): 51}


@functools.lru_cache(maxsize=None)
def sweep_input(n_fft, hop, L):
    """3 `wide` utterances with the burst in the last 100 samples (the last frame, for a multi-chunk length the last
    chunk, sets the top_db floor) and the gain ladder."""
    seed = 1000 + 7 * n_fft + 3 * hop + L
    return (wide(synth_audio(np.random.default_rng(seed), 3, L), (L - 100, L)) * ladder(3)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------
# error measures
# ------------------------------------------------------------------------------------------------------------
def db_errors(got, ref):
    d = np.abs(np.asarray(got, np.float64) - ref)
    return float(d.max()), float(np.sqrt(np.mean(d ** 2)))


def stft_errors(got, ref):
    """(max |got - ref| over the utterance's peak |X|, worst frame's max error over that frame's own peak |X|); a frame
    whose oracle STFT is exactly zero must be exactly zero (its ratio counts as 0, anything else as inf)."""
    ref = ref.astype(np.complex128)
    e = np.abs(np.asarray(got).astype(np.complex128) - ref)
    peak = np.abs(ref).max(axis=0)
    fe = e.max(axis=0)
    per_frame = np.where(peak > 0, fe / np.where(peak > 0, peak, 1.0), np.where(fe > 0, np.inf, 0.0))
    return float(e.max() / np.abs(ref).max()), float(per_frame.max())


def wave_errors(got, ref, hop):
    """(relative RMS over the utterance, worst block of `hop` samples: error RMS over max(the oracle's RMS in that
    block, the oracle's RMS over the utterance))."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    whole = np.sqrt(np.mean(ref ** 2))
    n = (len(ref) + hop - 1) // hop
    worst = 0.0
    for b in range(n):
        r, g = ref[b * hop:(b + 1) * hop], got[b * hop:(b + 1) * hop]
        worst = max(worst, float(np.sqrt(np.mean((g - r) ** 2)) / max(np.sqrt(np.mean(r ** 2)), whole)))
    return float(np.sqrt(np.mean((got - ref) ** 2)) / whole), worst


@functools.lru_cache(maxsize=None)
def _pinv(n_fft, sample_rate, n_mels, fmin, fmax):
    return np.linalg.pinv(R.mel_filterbank(sample_rate, n_fft, n_mels, fmin, fmax))


def oracle_reconstruct(pred, D, n_fft, hop, bank=DEFAULT_BANK, phase=None):
    """reconstruct_signal_from_spectrogram (data_processor.py:99-116) with the bank as a parameter: pred [n_mels, T]
    mel dB, D the mixture's complex STFT [1 + n_fft // 2, >= T] (or `phase` in place of magphase(D)'s)."""
    T = pred.shape[1]
    amp = R.db_to_amplitude(np.asarray(pred, np.float64))
    if phase is None:
        _, phase = R.magphase(D[:, :T])
    return R.istft((_pinv(n_fft, bank["sample_rate"], bank["n_mels"], bank["fmin"], bank["fmax"]) @ amp) * phase,
                   hop_length=hop)


def prediction(x, n_fft, hop, rng, bank=DEFAULT_BANK, top_db=80.0):
    """A network-like prediction for the mixture x: its own oracle mel dB plus N(0, 1 dB) noise -> (pred [n_mels, T]
    float32, the mixture's oracle STFT)."""
    pre, D = oracle_pre(x, n_fft, hop, "reflect", bank)
    return (clamp(pre, top_db) + rng.normal(0, 1.0, pre.shape)).astype(np.float32), D


# ------------------------------------------------------------------------------------------------------------
# ISTFT inputs: name -> dict(x [U, L], n_fft, hop, bank, pred [U, n_mels, T], D = the oracle STFTs)
# ------------------------------------------------------------------------------------------------------------
ISTFT_GEOMETRIES = {
    # name: (n_fft, hop, L, bank)                      kernel
    "dft666": (666, 166, 6400, DEFAULT_BANK),          # k_istft_dft at the 24-fps geometry (2 slices of 19 frames)
    "dft401": (401, 100, 2000, DEFAULT_BANK),          # k_istft_dft, inverse size 400
    "dft1024": (1024, 256, 4096, DEFAULT_BANK),        # k_istft_dft
    "ola64": (640, 160, 6400, BANK64_7600),            # k_istft640 + k_ola: not 80 bands
    "ola_hop320": (640, 320, 6400, DEFAULT_BANK),      # k_istft640 + k_ola: hop != 160
    "ola_hop100": (640, 100, 3200, DEFAULT_BANK),
    "fused": (640, 160, 160 * 62, DEFAULT_BANK),       # 63 STFT frames: T = 2 .. 62 of them (chunks of OF = 30 hops)
    "fused61": (640, 160, 9600, DEFAULT_BANK),         # 61 STFT frames for T = 60 sliced to 20
    "fused65": (640, 160, 10240, DEFAULT_BANK),        # 65
    "i532": (533, 133, 133 * 34, DEFAULT_BANK),        # 35 STFT frames: T = 2 .. 33 of them (chunks of 16 frames)
}
FUSED_T = (2, 30, 31, 32, 61, 62)
I532_T = (2, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def istft_case(name):
    n_fft, hop, L, bank = ISTFT_GEOMETRIES[name]
    rng = np.random.default_rng(2000 + sorted(ISTFT_GEOMETRIES).index(name))
    x = (wide(synth_audio(rng, 3, L), (L - 100, L)) * ladder(3)).astype(np.float32)
    pd = [prediction(xu, n_fft, hop, rng, bank) for xu in x]
    return dict(x=x, n_fft=n_fft, hop=hop, bank=bank, pred=np.stack([p for p, _ in pd]), D=[d for _, d in pd])


# name: (n_fft, hop, frames per slice, L); the silent eighth of L is at least three windows long (2000 samples are 3.0
# windows of 666 and hold only 3 zero frames, too few to move the waveform by 0.2: 19200 samples hold 6)
ZERO_GEOMETRIES = {"fused": (640, 160, 20, 16000), "dense": (640, 160, 20, 16000), "i532": (533, 133, 24, 16000),
                   "dft666": (666, 166, 19, 19200)}


@functools.lru_cache(maxsize=None)
def zero_frame_case(name):
    """The rule "phase is 1 where D == 0": a `wide` mixture whose STFT is exactly zero over several frames, and a
    prediction that puts energy within 6 dB of the utterance's maximum into those frames.  Conditions (asserted here, on
    the oracle): the oracle waveform's RMS inside the silent stretch is at least 0.3 of the whole, and a phase of 0 in
    the zero frames changes the waveform by more than 0.2 relative RMS."""
    n_fft, hop, spf, ZERO_L = ZERO_GEOMETRIES[name]
    rng = np.random.default_rng(3000 + n_fft)
    x = wide(synth_audio(rng, 2, ZERO_L), (ZERO_L - 100, ZERO_L))
    assert ZERO_L // 8 >= 3 * n_fft
    preds, Ds, refs, figures = [], [], [], []
    for xu in x:
        pred, D = prediction(xu, n_fft, hop, rng)
        T = (pred.shape[1] // spf) * spf
        top = pred.max()                  # the utterance's maximum: in the burst, which at 666 / 166 lies past frame T
        pred = pred[:, :T]
        zero = np.all(D[:, :T] == 0, axis=0)
        assert zero.sum() >= 3, zero.sum()
        pred[:, zero] = (top - rng.uniform(0, 6.0, (pred.shape[0], int(zero.sum())))).astype(np.float32)
        ref = oracle_reconstruct(pred, D, n_fft, hop)
        _, phase = R.magphase(D[:, :T])
        phase0 = np.where(zero[None, :], 0.0, phase)
        alt = oracle_reconstruct(pred, D, n_fft, hop, phase=phase0)
        lo, hi = ZERO_L // 4, ZERO_L // 4 + ZERO_L // 8
        whole = np.sqrt(np.mean(ref.astype(np.float64) ** 2))
        inside = float(np.sqrt(np.mean(ref[lo:hi].astype(np.float64) ** 2)) / whole)
        moved = float(np.sqrt(np.mean((alt.astype(np.float64) - ref) ** 2)) / whole)
        assert inside >= 0.3, f"waveform RMS inside the silent stretch is {inside} of the whole"
        assert moved > 0.2, f"a phase of 0 in the zero frames moves the waveform by only {moved}"
        preds.append(pred); Ds.append(D); refs.append(ref); figures.append((int(zero.sum()), inside, moved))
    return dict(x=x, n_fft=n_fft, hop=hop, spf=spf, pred=np.stack(preds), D=Ds, ref=refs, figures=figures)


# ------------------------------------------------------------------------------------------------------------
# slicing pinned to tests/golden/slicing.json (frame_ids written by the reference's own preprocess_audio_signal)
# ------------------------------------------------------------------------------------------------------------
def slicing_fixture():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slicing.json")) as fd:
        return json.load(fd)["preprocess_audio_signal"]


@functools.lru_cache(maxsize=None)
def slicing_case(i, n_signals=1):
    """Fixture case i on synth_audio signals of n_samples_in samples -> dict(fx, x [n, n_samples_in], full = the
    oracle's unsliced clamped dB [80, n_frames] per signal, unique = per signal and column: no other column within
    1 dB (maximum over bands) of it)."""
    fx = slicing_fixture()[i]
    x = synth_audio(np.random.default_rng(4000 + i), n_signals, fx["n_samples_in"])
    full, unique = [], []
    for xu in x:
        db = clamp(oracle_pre(R.fit_length(xu, fx["signal_length"]), fx["n_fft"], fx["hop_length"])[0])
        assert db.shape == (80, fx["n_frames"])
        dist = np.abs(db[:, :, None] - db[:, None, :]).max(axis=0)        # [T, T] column distances
        np.fill_diagonal(dist, np.inf)
        full.append(db)
        unique.append(dist.min(axis=1) > 1.0)
    return dict(fx=fx, x=x, full=full, unique=unique)


def record(case, **figures):
    """One line per device comparison (pytest -s shows them; profiles/audio_edge_checks.txt keeps a run's lines)."""
    print("audio-edge  %-44s %s" % (case, "  ".join(
        f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items())))
