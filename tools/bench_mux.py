"""Timing of the mux's colour conversion (hip.rgb_to_yuv420, csrc/mux.hip) and of the device-to-host copy it halves.

    python tools/bench_mux.py [--frames 32] [--width 1920] [--height 1080] [--calls 20]

Prints one JSON line: the median of ``--calls`` event-timed launches, the bytes it moves (3 in + 1.5 out per pixel), the rate, the
time a pure copy of those bytes takes at ``--hbm_tbs`` (the measured float4-copy rate of the chip, 6.29 TB/s), and the median
device-to-host time of the I420 payload beside that of the RGB frames (pinned host buffers, same run)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vface_amd import hip  # noqa: E402


def timed(fn, calls):
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--hbm_tbs", type=float, default=6.29)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    rgb = torch.randint(0, 256, (a.frames, a.height, a.width, 3), dtype=torch.uint8, device=dev, generator=gen)
    out = torch.empty(a.frames, hip.i420_frame_bytes(a.width, a.height), dtype=torch.uint8, device=dev)
    for _ in range(3):
        hip.rgb_to_yuv420(rgb, out=out)
    torch.cuda.synchronize()
    kernel_ms = timed(lambda: hip.rgb_to_yuv420(rgb, out=out), a.calls)
    moved = rgb.numel() + out.numel()
    host_yuv = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)
    host_rgb = torch.empty(rgb.shape, dtype=torch.uint8, pin_memory=True)
    for h, d in ((host_yuv, out), (host_rgb, rgb)):
        h.copy_(d, non_blocking=True)
    torch.cuda.synchronize()
    d2h_yuv = timed(lambda: host_yuv.copy_(out, non_blocking=True), a.calls)
    d2h_rgb = timed(lambda: host_rgb.copy_(rgb, non_blocking=True), a.calls)
    med = statistics.median(kernel_ms)
    print(json.dumps({
        "what": "rgb_to_yuv420", "frames": a.frames, "width": a.width, "height": a.height, "calls": a.calls,
        "kernel_ms_median": med, "kernel_ms_min": min(kernel_ms), "kernel_ms_max": max(kernel_ms),
        "bytes_moved": moved, "tb_per_s": moved / (med * 1e-3) / 1e12,
        "copy_bound_ms_at_hbm_rate": moved / (a.hbm_tbs * 1e12) * 1e3, "hbm_tbs": a.hbm_tbs,
        "d2h_i420_ms_median": statistics.median(d2h_yuv), "d2h_rgb_ms_median": statistics.median(d2h_rgb),
        "i420_bytes": out.numel(), "rgb_bytes": rgb.numel()}))


if __name__ == "__main__":
    main()
