"""Times of the device-side preprocess against the host paths it stands beside:
  * data_processor.preprocess_audio_pairs for U pairs of 3-s utterances against the per-sample loop of
    speech_enhancer.preprocess_audio_pair (noise_at_snr + AudioMixer.mix + three preprocess_audio_signal), both from
    signals in memory and both ending with the results on the host; and the device part alone (mix_pairs + one
    spectrogram over the 3 U rows) between HIP events;
  * VideoNormalizer.fit_device on a [S, 128, 128, 5] device tensor (HIP events; bytes read / time beside the HBM peak)
    against VideoNormalizer(numpy) on the host.
    python tools/prep_time.py [--pairs 64] [--slices 4096] [--reps 100] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import avse_pkg  # noqa: E402

avse_pkg.load()
from avse_amd import _lib, data_processor as dp, ops  # noqa: E402
from avse_amd.audio_io import AudioMixer, AudioSignal  # noqa: E402
from avse_amd.speech_enhancer import noise_at_snr  # noqa: E402

HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0     # MI355X: spec peak, streaming ceiling measured by microbenchmarks


def events_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fn, reps, warmup=2):
    """Host clock around calls that end with their results on the host (a device-to-host copy synchronises)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def per_sample(speech, noise):
    out = []
    for sp, nz in zip(speech, noise):
        s = AudioSignal(sp, 16000)
        n = noise_at_snr(AudioSignal(nz, 16000), s.get_number_of_samples(), s)
        m = AudioMixer.mix([s, n], mixing_weights=[1, 1])
        out.append([dp.preprocess_audio_signal(x, 200, 15, 25.0) for x in (m, s, n)] + [m])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--slices", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prep_time.py measures on the GPU: none visible")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "source_digest": _lib.source_digest(), "reps": a.reps}

    U = a.pairs
    speech = [np.clip(np.round(rng.normal(0, 3000, 48000)), -32768, 32767).astype(np.int16) for _ in range(U)]
    noise = [np.clip(np.round(rng.normal(0, 2000, int(n))), -32768, 32767).astype(np.int16)
             for n in rng.integers(16000, 160000, U)]
    sp_sig, nz_sig = [AudioSignal(s, 16000) for s in speech], [AudioSignal(n, 16000) for n in noise]
    got = dp.preprocess_audio_pairs(sp_sig, nz_sig, 200, 15, 25.0)
    ref = per_sample(speech, noise)
    equal = all(np.array_equal(g[k], r[k]) for g, r in zip(got, ref) for k in range(3)) and \
        all(np.array_equal(g[3].get_data(), r[3].get_data()) for g, r in zip(got, ref))
    batched = wall_ms(lambda: dp.preprocess_audio_pairs(sp_sig, nz_sig, 200, 15, 25.0), a.reps)
    loop = wall_ms(lambda: per_sample(speech, noise), max(10, a.reps // 5))
    sp_d = [torch.from_numpy(s).to(dev) for s in speech]
    nz_d = [torch.from_numpy(n).to(dev) for n in noise]
    packed = ((torch.cat(sp_d), np.arange(U + 1, dtype=np.int64) * 48000),
              (torch.cat(nz_d), np.concatenate([[0], np.cumsum([len(n) for n in noise])]).astype(np.int64)))

    def device_part():
        rows, _, _ = ops.mix_pairs(packed[0], packed[1], 48000)
        ops.spectrogram(rows.view(3 * U, 48000), frames_per_slice=20)

    res["pairs"] = {"n_pairs": U, "samples": 48000, "bit_equal_to_per_sample": bool(equal),
                    "batched_wall_ms_median_min": batched, "per_sample_loop_wall_ms_median_min": loop,
                    "speedup_median": loop[0] / batched[0],
                    "device_part_ms_events": events_ms(device_part, a.reps),
                    "mix_pairs_only_ms_events": events_ms(lambda: ops.mix_pairs(packed[0], packed[1], 48000), a.reps)}
    print(json.dumps(res["pairs"]), flush=True)
    del sp_d, nz_d, packed

    S = a.slices
    video = torch.from_numpy(rng.integers(0, 256, (S, 128, 128, 5), dtype=np.uint8)).to(dev).to(torch.float32)
    nbytes = video.numel() * 4
    ms = events_ms(lambda: ops.video_stats(video), a.reps)
    host = video.cpu().numpy()
    t0 = time.perf_counter()
    ref_norm = dp.VideoNormalizer(host)
    host_s = time.perf_counter() - t0
    fit = dp.VideoNormalizer.fit_device(video)
    res["video_stats"] = {"shape": [S, 128, 128, 5], "bytes": nbytes, "device_ms_events": ms,
                          "achieved_GBps": nbytes / ms / 1e6, "hbm_peak_GBps": HBM_PEAK_GBS,
                          "hbm_achievable_GBps": HBM_ACHIEVABLE_GBS, "share_of_peak": nbytes / ms / 1e6 / HBM_PEAK_GBS,
                          "host_numpy_fit_s": host_s, "speedup_vs_host": host_s * 1e3 / ms,
                          "max_abs_diff_mean_vs_host_fit": float(np.abs(fit.mean_image - ref_norm.mean_image).max()),
                          "max_abs_diff_std_vs_host_fit": float(np.abs(fit.std_image - ref_norm.std_image).max())}
    print(json.dumps(res["video_stats"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fd:
            json.dump(res, fd, indent=1)


if __name__ == "__main__":
    main()
