"""Timing of the PNG encoder (hip.png_filter + hip.png_deflate, csrc/png.hip; scripts/png.py) and of everything it leaves to the
host, beside the default path -- Pillow's ``Image.save`` on one core -- on the same frames in the same run.

    python tools/bench_png.py [--calls 10] [--inner 3] [--pillow_frames 4] [--out sweep.jsonl]

For 32 frames of 1920 x 1080 and 32 of 512 x 512, on three kinds of content -- a smooth synthetic gradient, the same with Gaussian
noise of sigma 2 (the closest here to decoded video) and uniform noise -- and for stripe_rows in 4, 8, 16, 32: the two kernels'
stages are timed in turn, ``--calls`` samples each, a sample being ``--inner`` back-to-back calls between two HIP events divided by
their number; then the two device-to-host copies (the lengths and checksum halves; the compressed bytes; pinned host buffers) and the
host's framing and CRC.  ``PNGEncoder.encode`` is timed whole as well (a host clock around a call that ends in the copies).  Pillow
saves ``--pillow_frames`` of the same frames to memory at its default level.  Frame 0 of every run is decoded by Pillow and compared.
Prints one JSON line per (size, content, stripe_rows); ``--out`` also appends them to a file.  No threshold: these are the numbers of
DESIGN §9, and ``hip.PNG_STRIPE_ROWS`` is set from them."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vface_amd import hip  # noqa: E402
from vface_amd.scripts import png  # noqa: E402

SIZES = ((32, 1920, 1080), (32, 512, 512))
CONTENTS = ("smooth", "noisy", "noise")
STRIPE_ROWS = (4, 8, 16, 32)


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def content(kind, frames, W, H, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    if kind == "noise":
        return torch.randint(0, 256, (frames, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    f = torch.arange(frames, device=dev, dtype=torch.float32)[:, None, None]
    y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    x = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    img = torch.stack([128 + 100 * torch.sin(x / 97 + y / 131 + 0.1 * f), 128 + 90 * torch.cos(x / 61 + 0.2 * f) * torch.sin(y / 83),
                       (x + y + 3 * f) * (255.0 / (W + H + 96))], dim=-1)
    if kind == "noisy":
        img = img + 2.0 * torch.randn(img.shape, device=dev, generator=gen)
    return img.round().clamp(0, 255).to(torch.uint8)


def pillow(rgb, count):
    """Pillow's save of ``count`` frames spread over the batch -> (median seconds per frame, mean file bytes)."""
    secs, sizes = [], []
    for f in np.linspace(0, rgb.shape[0] - 1, count).astype(int):
        frame = rgb[f].cpu().numpy()
        t0 = time.perf_counter()
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, "PNG")
        secs.append(time.perf_counter() - t0)
        sizes.append(buf.tell())
    return statistics.median(secs), sum(sizes) / len(sizes)


def measure(kind, rgb, stripe_rows, calls, inner, base):
    frames, H, W, _ = rgb.shape
    enc = png.PNGEncoder(W, H, stripe_rows=stripe_rows)
    files = enc.encode(rgb)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[0]))), rgb[0].cpu().numpy()), "frame 0 does not decode to itself"
    rows = hip.png_filter(rgb)
    out, meta, _ = hip.png_deflate(rows, stripe_rows)
    runs = {"filter": lambda: hip.png_filter(rgb, out=rows), "deflate": lambda: hip.png_deflate(rows, stripe_rows, out=out)}
    for fn in runs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(calls):          # alternating, so a busy moment on a shared machine falls on both
        for k, fn in runs.items():
            ms[k].append(sample(fn, inner))
    lengths = meta[:frames].cpu().tolist()
    total = sum(lengths)
    host_meta, host_out = torch.empty(meta.shape, dtype=torch.int32).pin_memory(), torch.empty(total, dtype=torch.uint8).pin_memory()
    copies = {"d2h_meta": lambda: host_meta.copy_(meta, non_blocking=True), "d2h_bytes": lambda: host_out.copy_(out[:total], non_blocking=True)}
    for fn in copies.values():
        fn()
    torch.cuda.synchronize()
    for k, fn in copies.items():
        ms[k] = [sample(fn, 1) for _ in range(calls)]
    data, halves = host_out.numpy().tobytes(), host_meta[frames:].tolist()
    framing = []
    for _ in range(max(3, calls // 3)):
        t0, at = time.perf_counter(), 0
        for f, n in enumerate(lengths):
            h = halves[2 * f * enc.stripes:2 * (f + 1) * enc.stripes]
            adler = png.adler32_combine([(h[2 * s], h[2 * s + 1], enc._stripe_bytes[s]) for s in range(enc.stripes)])
            png.png_file(W, H, data[at:at + n], adler)
            at += n
        framing.append(1e3 * (time.perf_counter() - t0))
    whole = []
    for _ in range(max(3, calls // 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.encode(rgb)
        whole.append(1e3 * (time.perf_counter() - t0))
    rec = {"what": "png_filter + png_deflate + copies + host framing beside Pillow's save", "content": kind, "frames": frames, "width": W,
           "height": H, "stripe_rows": stripe_rows, "calls": calls, "inner": inner, "rgb_bytes": rgb.numel(),
           "bytes_to_host": total + 4 * meta.numel(), "gpu_file_bytes_per_frame": sum(len(x) for x in files) / frames,
           "workspace_bytes": int(hip.load().vface_png_deflate_workspace_bytes(1 + 3 * W, H, frames, stripe_rows)),
           "host_framing_ms_median": statistics.median(framing), "encode_call_ms_median": statistics.median(whole),
           "encode_call_ms_min": min(whole), "encode_call_ms_max": max(whole)}
    for k, v in ms.items():
        rec[k + "_us_median"], rec[k + "_us_min"], rec[k + "_us_max"] = 1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v)
    rec["gpu_ms_per_frame"] = rec["encode_call_ms_median"] / frames
    rec.update(base)
    rec["pillow_over_gpu"] = rec["pillow_ms_per_frame"] / rec["gpu_ms_per_frame"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--pillow_frames", type=int, default=4)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("An MI355X is required: there is nothing to time without one.")
    dev = torch.device("cuda", 0)
    for frames, W, H in SIZES:
        for kind in CONTENTS:
            rgb = content(kind, frames, W, H, dev)
            secs, size = pillow(rgb, a.pillow_frames)
            base = {"pillow_ms_per_frame": 1e3 * secs, "pillow_file_bytes_per_frame": size, "pillow_frames": a.pillow_frames}
            for stripe_rows in STRIPE_ROWS:
                line = json.dumps(measure(kind, rgb, stripe_rows, a.calls, a.inner, base))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
