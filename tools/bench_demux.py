"""Timing of the video intake's colour conversion (hip.yuv420_to_rgb, csrc/demux.hip) beside the mux's (hip.rgb_to_yuv420) on the same
frames in the same run, and of the host-to-device copy the I420 upload halves.

    python tools/bench_demux.py [--calls 20] [--inner 20]

For 32 frames of 1920 x 1080 and 8 of 512 x 512: the frames are made once (seeded RGB -> I420 by the mux's kernel), then the two
directions are timed in turn, ``--calls`` samples each, a sample being ``--inner`` back-to-back launches between two HIP events
divided by their number (a single launch of ~50 us would mostly time its own enqueue).  Both move 4.5 bytes per pixel.  Prints one
JSON line per size: medians, the ratio demux / mux per chroma mode, the rate, the time of a pure copy of those bytes at ``--hbm_tbs``
(the chip's measured float4-copy rate), and the median host-to-device times of the I420 rows and of the RGB frames (pinned host
buffers)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vface_amd import hip  # noqa: E402

SIZES = ((32, 1920, 1080), (8, 512, 512))


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def measure(frames, W, H, calls, inner, hbm_tbs):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    rgb = torch.randint(0, 256, (frames, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    i420 = hip.rgb_to_yuv420(rgb)
    back = torch.empty_like(rgb)
    scratch = torch.empty_like(i420)
    runs = {"mux": lambda: hip.rgb_to_yuv420(rgb, out=scratch)}
    for mode in ("centre", "left", "nearest"):
        runs["demux_" + mode] = lambda mode=mode: hip.yuv420_to_rgb(i420, W, H, chroma=mode, out=back)
    for fn in runs.values():        # warm-up: code objects loaded, every shape launched
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(calls):          # alternating, so a busy moment on a shared machine falls on all of them
        for name, fn in runs.items():
            ms[name].append(sample(fn, inner))
    host_yuv = i420.cpu().pin_memory()
    host_rgb = rgb.cpu().pin_memory()
    copies = {"h2d_i420": lambda: scratch.copy_(host_yuv, non_blocking=True), "h2d_rgb": lambda: back.copy_(host_rgb, non_blocking=True)}
    for fn in copies.values():
        fn()
    torch.cuda.synchronize()
    for name in copies:
        ms[name] = []
    for _ in range(calls):
        for name, fn in copies.items():
            ms[name].append(sample(fn, 1))
    med = {name: statistics.median(v) for name, v in ms.items()}
    moved = rgb.numel() + i420.numel()
    rec = {"what": "yuv420_to_rgb beside rgb_to_yuv420", "frames": frames, "width": W, "height": H, "calls": calls, "inner": inner,
           "bytes_moved": moved, "copy_bound_ms_at_hbm_rate": moved / (hbm_tbs * 1e12) * 1e3, "hbm_tbs": hbm_tbs,
           "i420_bytes": i420.numel(), "rgb_bytes": rgb.numel()}
    for name, v in ms.items():
        rec[name + "_ms_median"], rec[name + "_ms_min"], rec[name + "_ms_max"] = med[name], min(v), max(v)
    for mode in ("centre", "left", "nearest"):
        rec[f"ratio_demux_{mode}_over_mux"] = med["demux_" + mode] / med["mux"]
        rec[f"demux_{mode}_tb_per_s"] = moved / (med["demux_" + mode] * 1e-3) / 1e12
    rec["mux_tb_per_s"] = moved / (med["mux"] * 1e-3) / 1e12
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--hbm_tbs", type=float, default=6.29)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("An MI355X is required: there is nothing to time without one.")
    for frames, W, H in SIZES:
        print(json.dumps(measure(frames, W, H, a.calls, a.inner, a.hbm_tbs)), flush=True)


if __name__ == "__main__":
    main()
