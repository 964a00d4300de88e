#!/usr/bin/env python
"""Times one tick of the frame retimer: every stream receives 6 camera frames at 30 fps and hands one
25-fps slice [128][128][5] to the session, at 64 and 1024 streams, uint8 and float32, through avse_retimer_push_each
itself (the C-ABI call on preallocated buffers, so the host's part is the row arithmetic and one pinned copy).

Two phases of the 6-frame cycle are timed, because they move different amounts of memory:
  aligned  the streams stand at a multiple of 6 frames: a tick completes exactly one slice and leaves no frame pending
           (reads 6 frames + the last frame of the tick before, writes 1 slice + the new last frame);
  offset   the streams stand 3 frames into the cycle: a tick completes one slice whose first 2 frames were pending,
           and leaves 2 frames of the next (reads 6 frames + the last frame + the pending slice, writes 2 slices' worth
           + the last frame).
Each figure is HIP-event time over a window of back-to-back ticks divided by their number (warm-up first; the median
and the extremes of several windows; a window holds as many ticks as fill --min-window-ms), so it holds the row upload
and the launch as a caller pays them.  The timed loop is the bare C-ABI call; its status and counts are checked after
the window.  Beside it stands the host clock around the same loop before the synchronise (host_enqueue_us per call).
For the copy, a host figure as long as the event time means the window measures how fast the host submits.  For the
retimer the two are equal by construction (the host waits on the staging ring once four calls are queued), so they
cannot say where the time goes: the kernel trace below does.  In the same process a plain device copy (Tensor.copy_) of half the tick's bytes read plus
written, which reads and writes that many between them, is timed the same way; the ratio is retimer / copy.
The kernel's own duration needs a trace: run the tool under `rocprofv3 --kernel-trace --stats` in a run of its own
(--runs 1 --min-window-ms 20 keeps it short).

  python tools/retime_time.py --out profiles/retime_time.txt
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", default="64,1024")
    ap.add_argument("--dtypes", default="uint8,float32")
    ap.add_argument("--ticks", type=int, default=50, help="fewest back-to-back ticks per timed window")
    ap.add_argument("--min-window-ms", type=float, default=250.0, help="a window holds enough ticks to last this long")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import avse_pkg
    avse_pkg.load()
    from avse_amd import _lib, ops
    if not torch.cuda.is_available():
        sys.exit("retime_time: no ROCm GPU visible to torch; nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    F, N_IN, PIX = 5, 6, 128 * 128
    lines = []

    def window(fn, n):
        """-> (HIP-event ms, host ms spent enqueuing) per call over n back-to-back calls of fn."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n, 1e3 * (t1 - t0) / n

    def run(fn, check=lambda: None):
        """-> (ms per call: median, min, max of the windows; host enqueue ms per call, median; calls per window)."""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        check()
        est = max(window(fn, args.ticks))
        n = max(args.ticks, int(args.min_window_ms / est) + 1)
        got = sorted(window(fn, n) for _ in range(args.runs))
        check()
        ms = [g[0] for g in got]
        return ms[len(ms) // 2], ms[0], ms[-1], sorted(g[1] for g in got)[len(got) // 2], n

    for dtype in args.dtypes.split(","):
        tdt, esz = (torch.uint8, 1) if dtype == "uint8" else (torch.float32, 4)
        for B in (int(b) for b in args.streams.split(",")):
            g = torch.Generator(device="cpu").manual_seed(B)
            frames = torch.randint(0, 256, (B * N_IN, 128, 128), generator=g, dtype=torch.uint8).to(dev).to(tdt)
            out = torch.empty((B, 128, 128, F), dtype=tdt, device=dev)
            off = np.arange(B, dtype=np.int64) * N_IN
            n_new = np.full(B, N_IN, np.int64)
            got = np.zeros(B, np.int64)
            for phase, prime in (("aligned", 0), ("offset", 3)):
                r = ops.retimer_create(B, 30, 25, F, tdt, dev)
                if prime:
                    k, n_prime = np.zeros(B, np.int64), np.full(B, prime, np.int64)
                    _lib.check(lib.avse_retimer_push_each(r.handle, _lib.ptr(frames), off.ctypes.data, n_prime.ctypes.data,
                                                          None, _lib.ptr(out), B, k.ctypes.data, _lib.stream_handle(dev)),
                               "prime")
                    assert not k.any()

                # the arguments are made once: the timed call is the library's entry point and nothing else
                call = (r.handle, _lib.ptr(frames), off.ctypes.data, n_new.ctypes.data, None, _lib.ptr(out), B,
                        got.ctypes.data, _lib.stream_handle(dev))
                status = [0]

                def tick():
                    status[0] |= lib.avse_retimer_push_each(*call)

                def check():
                    assert status[0] == 0 and got.min() == 1 == got.max(), (status, got[:4])

                # frames of 128 x 128 elements moved per stream and tick (retime.hip k_retime)
                pend = 2 if prime else 0
                read = N_IN + 1 + (F if pend else 0)            # the tick's frames, the last frame, the pending slice
                written = F + 1 + (F if pend else 0)            # the slice, the new last frame, the new pending slice
                nbytes = (read + written) * PIX * esz * B
                src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                t_med, t_min, t_max, t_host, t_n = run(tick, check)
                c_med, c_min, c_max, c_host, c_n = run(lambda: dst.copy_(src))
                line = dict(what="retimer_tick", dtype=dtype, streams=B, phase=phase, frames_in=N_IN, slices_out=1,
                            bytes_read_plus_written=nbytes, ticks_per_window=t_n, copies_per_window=c_n, runs=args.runs,
                            retimer_host_enqueue_us=round(1e3 * t_host, 2), copy_host_enqueue_us=round(1e3 * c_host, 2),
                            retimer_us=dict(median=round(1e3 * t_med, 2), min=round(1e3 * t_min, 2), max=round(1e3 * t_max, 2)),
                            copy_us=dict(median=round(1e3 * c_med, 2), min=round(1e3 * c_min, 2), max=round(1e3 * c_max, 2)),
                            retimer_TB_s=round(nbytes / (1e9 * t_med), 3), copy_TB_s=round(nbytes / (1e9 * c_med), 3),
                            ratio=round(t_med / c_med, 2))
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
                del r, src, dst
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
