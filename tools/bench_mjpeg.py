"""Timing of the Motion-JPEG encoder (hip.jpeg_coefficients + hip.jpeg_entropy, csrc/mjpeg.hip) and of what it sends to the host,
beside the raw path (hip.rgb_to_yuv420 and its copy) on the same frames in the same run.

    python tools/bench_mjpeg.py [--calls 20] [--inner 5] [--quality 90]

For 32 frames of 1920 x 1080 and 8 of 512 x 512, on a smooth pattern (sinusoids + ramp + sigma = 4 noise) and on uniform noise: the
two encoder stages and the I420 conversion are timed in turn, ``--calls`` samples each, a sample being ``--inner`` back-to-back
calls between two HIP events divided by their number; then the device-to-host copies (pinned host buffers) of the compressed
bytes and of the I420 planes.  The restart interval is one MCU row, as ``MJPEGWriter`` sets it.  Prints one JSON line per (size,
pattern): microseconds per call, bytes copied to the host, file bytes per frame.  No threshold: these are the numbers of DESIGN §9."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vface_amd import hip  # noqa: E402
from vface_amd.scripts import mjpeg  # noqa: E402

SIZES = ((32, 1920, 1080), (8, 512, 512))


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def pattern(name, frames, W, H, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    if name == "noise":
        return torch.randint(0, 256, (frames, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    f = torch.arange(frames, device=dev, dtype=torch.float32)[:, None, None]
    y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    x = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    smooth = torch.stack([128 + 60 * torch.sin(x / 11 + f) + 40 * torch.cos(y / 7) + 0.02 * x,
                          128 + 70 * torch.sin((x + y) / 17 + 0.5 * f) + 0.03 * y,
                          100 + 50 * torch.cos(x / 5) * torch.sin(y / 13 + f) + 0.02 * (x + y)], dim=-1)
    smooth = smooth + 4.0 * torch.randn(smooth.shape, device=dev, generator=gen)
    return smooth.round().clamp(0, 255).to(torch.uint8)


def measure(name, frames, W, H, quality, calls, inner):
    dev = torch.device("cuda", 0)
    rgb = pattern(name, frames, W, H, dev)
    tables = tuple(torch.tensor(t, dtype=torch.uint8, device=dev) for t in mjpeg.quant_tables(quality))
    restart = hip.jpeg_mcu_grid(W, H)[1]
    coef = hip.jpeg_coefficients(rgb, *tables)
    scans, lengths = hip.jpeg_entropy(coef, restart)
    i420 = hip.rgb_to_yuv420(rgb)
    runs = {"coefficients": lambda: hip.jpeg_coefficients(rgb, *tables, out=coef),
            "entropy": lambda: hip.jpeg_entropy(coef, restart, out=scans),
            "rgb_to_yuv420": lambda: hip.rgb_to_yuv420(rgb, out=i420)}
    for fn in runs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(calls):          # alternating, so a busy moment on a shared machine falls on all of them
        for k, fn in runs.items():
            ms[k].append(sample(fn, inner))
    sizes = lengths.cpu().tolist()
    total = sum(sizes)
    host_scan, host_yuv = torch.empty(total, dtype=torch.uint8).pin_memory(), torch.empty(i420.shape, dtype=torch.uint8).pin_memory()
    copies = {"d2h_scans": lambda: host_scan.copy_(scans[:total], non_blocking=True), "d2h_i420": lambda: host_yuv.copy_(i420, non_blocking=True)}
    for fn in copies.values():
        fn()
    torch.cuda.synchronize()
    for k, fn in copies.items():
        ms[k] = [sample(fn, 1) for _ in range(calls)]
    header = len(mjpeg.jpeg_header(W, H, mjpeg.quant_tables(quality), restart))
    per_frame = [8 + (header + n + 2) + ((header + n + 2) & 1) + 16 for n in sizes]          # chunk, padding, index entry
    rec = {"what": "jpeg_coefficients + jpeg_entropy beside rgb_to_yuv420", "pattern": name, "frames": frames, "width": W, "height": H,
           "quality": quality, "restart": restart, "calls": calls, "inner": inner, "bytes_to_host": total + 4 * frames,
           "i420_bytes_to_host": i420.numel(), "rgb_bytes": rgb.numel(), "file_bytes_per_frame": sum(per_frame) / frames,
           "y4m_bytes_per_frame": i420.shape[1] + 6, "bits_per_pixel": 8.0 * total / (frames * W * H),
           "workspace_bytes": int(hip.load().vface_jpeg_entropy_workspace_bytes(math.prod(hip.jpeg_mcu_grid(W, H)), frames, restart))}
    for k, v in ms.items():
        rec[k + "_us_median"], rec[k + "_us_min"], rec[k + "_us_max"] = 1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("An MI355X is required: there is nothing to time without one.")
    for frames, W, H in SIZES:
        for name in ("smooth", "noise"):
            print(json.dumps(measure(name, frames, W, H, a.quality, a.calls, a.inner)), flush=True)


if __name__ == "__main__":
    main()
