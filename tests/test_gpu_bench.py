"""bench.py's command line on the device: a plain run prints the headline only and --dump-outputs writes what its last
timed step computed; --full adds the figures that take runs of their own.  Small batches: the benchmarked sizes are
checked in test_gpu_split.py / test_gpu_forward.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import keras_ref as K
from oracle import librosa_ref as R
from test_gpu_forward import FP32_REL, rel_rms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "breakdown", "legs", "cpu_baseline", "parity"}


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_step(gpu, tmp_path):
    import bench
    from avse_amd.model import KerasModel
    N = 8
    d = run_bench("--batch", str(N), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump"))
    assert HEADLINE <= set(d) and not FULL_ONLY & set(d), sorted(d)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "fp32_split" and d["unit"] == "clips/s"
    assert d["ms_per_step"] > 0 and abs(d["value"] - N / (d["ms_per_step"] * 1e-3)) <= 1e-2 * d["value"]
    assert d["range_guard"]["bits"] == 0 and "blocking_checked_per_step_clips_per_s" not in d["range_guard"]
    assert sorted(os.listdir(tmp_path / "dump")) == ["mel.npy", "out.npy"]
    out, mel = np.load(tmp_path / "dump" / "out.npy"), np.load(tmp_path / "dump" / "mel.npy")
    assert out.dtype == np.float32 and mel.dtype == np.float32 and out.shape == mel.shape == (N, 80, 20)
    # the dump is the benchmark's own seeded batch through STFT + forward: against the oracle on the same inputs
    audio_np, video_np = bench.synth(np.random.default_rng(1234), N)
    mean_np = video_np.mean(axis=(0, 3)).astype(np.float32)
    std_np = video_np.std(axis=(0, 3)).astype(np.float32)
    mel_ref = np.stack([R.preprocess_audio_signal(audio_np[i], 16000, 200, 1, 25.0)[0] for i in range(N)])
    assert np.abs(mel - mel_ref).max() < 2e-2, np.abs(mel - mel_ref).max()       # dB; the bound of smoke()
    vn = R.video_normalize(video_np, mean_np, std_np).astype(np.float32)
    ref = K.forward(KerasModel.init(seed=0, randomize=True).layer_dict(), mel, vn)
    print(f"dumped out vs oracle: rel RMS {rel_rms(out, ref):.3e}")
    assert rel_rms(out, ref) <= FP32_REL


def test_full_run_adds_roofline_and_breakdown(gpu):
    d = run_bench("--batch", "8", "--steps", "2", "--warmup", "1", "--full", "--no-legs", "--no-cpu-baseline",
                  "--profile-reps", "1")
    assert HEADLINE <= set(d) and {"roofline", "breakdown"} <= set(d), sorted(d)
    assert d["roofline"]["avg_launch_ms"] > 0 and d["breakdown"]["stage_ms"]["v_conv2"] > 0
    assert "blocking_checked_per_step_clips_per_s" in d["range_guard"]
