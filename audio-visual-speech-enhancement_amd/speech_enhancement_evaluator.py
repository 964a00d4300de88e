"""The evaluate stage of the reference CLI (its `speech_enhancement_evaluator.py`), with open measures
computed on the device in PESQ's place: SNR, scale-invariant SDR, segmental SNR and STOI (ops.eval_pairs,
include/avse.h avse_eval_pairs).  PESQ itself stays what it is in the reference, an external binary: when its path is
given, it is run per sample as the reference runs it.

    python speech_enhancement_evaluator.py [--extended] ENHANCEMENT_DIR [PESQ_BIN_PATH]

--extended adds ESTOI and computes STOI at every sample rate from 8 to 48 kHz (ops.eval_pairs_ext), 44.1 kHz included;
walks ENHANCEMENT_DIR/<speaker>/<sample>/{source,enhanced,mixture}.wav as `predict` writes them."""
import argparse
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

from . import _lib, ops
from .audio_io import AudioSignal

METRICS = ("snr", "si_sdr", "seg_snr", "stoi")      # the printed slots of avse_eval_pairs, in slot order
ESTOI_SLOT = 5                                       # avse_eval_pairs_ext's sixth slot, printed after stoi
WAVS = ("source", "enhanced", "mixture")
MOS_LINE = re.compile(r"\(Raw MOS, MOS-LQO\):\s+= (-?[0-9.]+?)\s+([0-9.]+?)$", re.MULTILINE)
SKIP = "failed to evaluate pesq (%s). skipping"      # the reference's message, kept although PESQ is optional here


def pesq(binary, clean_wav, degraded_wav):
    """`binary +16000 source.wav enhanced.wav` on copies of the two files in a scratch directory of their own ->
    (raw MOS, MOS-LQO) from the tool's `(Raw MOS, MOS-LQO):` line."""
    with tempfile.TemporaryDirectory(prefix="avse_pesq_") as work:
        pair = []
        for name, wav in (("source.wav", clean_wav), ("enhanced.wav", degraded_wav)):
            pair.append(shutil.copy2(wav, os.path.join(work, name)))
        text = subprocess.check_output([binary, "+16000"] + pair, cwd=work).decode(errors="replace")
    found = MOS_LINE.search(text)
    if found is None:
        raise ValueError("no (Raw MOS, MOS-LQO) line in the output of %s" % binary)
    return float(found.group(1)), float(found.group(2))


def sample_dirs(root):
    """(speaker, sample, directory) in the reference's order: speakers as os.listdir gives them, samples sorted."""
    for speaker in os.listdir(root):
        for sample in sorted(os.listdir(os.path.join(root, speaker))):
            yield speaker, sample, os.path.join(root, speaker, sample)


def load_sample(directory):
    """Channel 0 of the three wav files -> ({name: samples}, sample rate).  Raises on a missing file, on differing
    sample rates and on an empty signal."""
    signals, rates = {}, set()
    for name in WAVS:
        wav = AudioSignal.from_wav_file(os.path.join(directory, name + ".wav"))
        signals[name] = wav.get_data(channel_index=0)
        rates.add(wav.get_sample_rate())
        if signals[name].shape[0] == 0:
            raise ValueError("%s.wav is empty" % name)
    if len(rates) != 1:
        raise ValueError("sample rates differ: %s" % sorted(rates))
    return signals, rates.pop()


def columns(extended):
    """(name, slot) of the printed metrics, in print order."""
    return [(name, slot) for slot, name in enumerate(METRICS)] + ([("estoi", ESTOI_SLOT)] if extended else [])


class _Batches:
    """Samples waiting for a device call, per sample rate; a full group (or, at the end, every group) is evaluated in
    one ops.eval_pairs call (extended: ops.eval_pairs_ext) over its (source, enhanced) pairs followed by its
    (source, mixture) pairs."""

    def __init__(self, size, done, extended=False):
        self.size, self.done, self.waiting, self.extended = max(1, int(size)), done, {}, extended

    def add(self, row, signals):
        group = self.waiting.setdefault(row["sample_rate"], [])
        group.append((row, signals))
        if len(group) >= self.size:
            self.run(row["sample_rate"])

    def run(self, rate):
        group = self.waiting.pop(rate, [])
        if not group:
            return
        clean = [sig["source"] for _, sig in group]
        degraded = [sig["enhanced"] for _, sig in group] + [sig["mixture"] for _, sig in group]
        try:
            if self.extended:
                table = ops.eval_pairs_ext(clean + clean, degraded, sample_rate=rate).cpu().numpy()
            else:
                table = ops.eval_pairs(clean + clean, degraded, sample_rate=rate).cpu().numpy()
        except (_lib.AvseError, ValueError, TypeError) as refusal:
            # what the binding refuses costs this group only; any other error (a device error among them) ends the run
            for _ in group:
                print(SKIP % refusal)
            return
        for k, (row, _) in enumerate(group):
            row["enhanced"], row["mixture"] = table[k], table[len(group) + k]
            for name, slot in columns(self.extended):
                print("mixture %s: %f, enhanced %s: %f" % (name, row["mixture"][slot], name, row["enhanced"][slot]))
            self.done.append(row)

    def run_all(self):
        for rate in list(self.waiting):
            self.run(rate)


def evaluate(enhancement_dir_path, pesq_bin_path=None, batch=64, extended=False):
    """Per sample, the metrics of (source, enhanced) and (source, mixture), in device batches of up to `batch` samples
    of one sample rate.  Prints the reference's lines per metric and returns the per-sample table, in the reference's
    order: [{speaker, sample, sample_rate, enhanced [5], mixture [5], (enhanced_pesq, mixture_pesq)}].
    extended: rows of 6 from ops.eval_pairs_ext (STOI at every sample rate, ESTOI), and the estoi lines after stoi's."""
    done = []
    batches = _Batches(batch, done, extended)
    order = {}
    for speaker, sample, directory in sample_dirs(enhancement_dir_path):
        print("evaluating %s..." % sample)
        try:
            signals, rate = load_sample(directory)
            row = {"speaker": speaker, "sample": sample, "sample_rate": rate}
            if pesq_bin_path:
                clean_wav = os.path.join(directory, "source.wav")
                row["enhanced_pesq"] = pesq(pesq_bin_path, clean_wav, os.path.join(directory, "enhanced.wav"))[0]
                row["mixture_pesq"] = pesq(pesq_bin_path, clean_wav, os.path.join(directory, "mixture.wav"))[0]
                print("mixture pesq: %f, enhanced pesq: %f" % (row["mixture_pesq"], row["enhanced_pesq"]))
        except Exception as e:      # a sample that does not load is skipped, as in the reference
            print(SKIP % e)
            continue
        order[id(row)] = len(order)
        batches.add(row, signals)
    batches.run_all()
    done.sort(key=lambda row: order[id(row)])     # groups finish out of order; the table keeps the walk's order

    for name, slot in columns(extended):
        for kind in ("enhanced", "mixture"):
            values = [row[kind][slot] for row in done]
            print("mean %s %s: " % (kind, name), np.mean(values), "std %s %s: " % (kind, name), np.std(values))
    if pesq_bin_path:
        for kind in ("enhanced", "mixture"):
            values = [row[kind + "_pesq"] for row in done]
            print("mean %s pesq: " % kind, np.mean(values), "std %s pesq: " % kind, np.std(values))
    return done


def main(argv=None):
    cli = argparse.ArgumentParser(description="SNR, SI-SDR, segmental SNR and STOI (and PESQ, given its binary) of "
                                              "every sample under a predict output directory")
    cli.add_argument("enhancement_dir", help="<dir>/<speaker>/<sample>/{source,enhanced,mixture}.wav")
    cli.add_argument("pesq_bin_path", nargs="?", default=None, help="the external PESQ binary (optional)")
    cli.add_argument("--extended", action="store_true",
                     help="also ESTOI, and STOI at every sample rate from 8 to 48 kHz (44.1 kHz included)")
    given = cli.parse_args(argv)
    if given.extended:
        evaluate(given.enhancement_dir, given.pesq_bin_path, extended=True)
    else:
        evaluate(given.enhancement_dir, given.pesq_bin_path)


if __name__ == "__main__":
    main()
