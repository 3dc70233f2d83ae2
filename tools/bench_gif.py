"""Timing of the GIF writer (hip.gif_histogram, gif_boxes, gif_palette, gif_map, gif_lzw, csrc/gif.hip; scripts/gif.py) and of
everything it leaves to the host, beside Pillow's ``save(save_all=True)`` of the same frames on one core in the same run.

    python tools/bench_gif.py [--calls 5] [--inner 2] [--pillow_frames 4] [--out sweep.jsonl]

For 32, 6 and 1 frames of 1920 x 1080 and of 512 x 512, on three kinds of content -- a smooth synthetic gradient, the same with
Gaussian noise of sigma 2 (the closest here to decoded video) and uniform noise -- the four quantiser stages are timed in turn,
``--calls`` samples each, a sample being ``--inner`` back-to-back calls between two HIP events divided by their number; then, for
seg_pixels in 1024, 2048, 4096, 8192 and 16384, the LZW entry point, the three device-to-host copies (offsets, palettes, image data;
pinned host buffers), the host's framing, and ``GIFWriter.write`` whole (a host clock around a call that ends in the copies and the
file write, to a file in memory's stead: os.devnull).  Pillow quantises and saves ``--pillow_frames`` of the same frames to memory.
Frame 0 of every run is decoded by Pillow and compared with palette[indices] of the device.  Prints one JSON line per (size,
frames, content, seg_pixels); ``--out`` also appends them to a file.  No threshold: these are the numbers of DESIGN §9, and
``hip.GIF_SEG_PIXELS`` is set from them."""
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
from vface_amd.scripts import gif  # noqa: E402

SIZES = ((1920, 1080), (512, 512))
FRAMES = (32, 6, 1)
CONTENTS = ("smooth", "noisy", "noise")
SEG_PIXELS = (1024, 2048, 4096, 8192, 16384)


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
    """Pillow's quantising GIF save of ``count`` frames spread over the batch, as one animated file -> (seconds per frame, bytes per frame)."""
    ims = [Image.fromarray(rgb[f].cpu().numpy()) for f in np.linspace(0, rgb.shape[0] - 1, min(count, rgb.shape[0])).astype(int)]
    t0 = time.perf_counter()
    buf = io.BytesIO()
    ims[0].save(buf, "GIF", save_all=True, append_images=ims[1:], duration=100, loop=0)
    return (time.perf_counter() - t0) / len(ims), buf.tell() / len(ims)


def timed(runs, calls, inner):
    for fn in runs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(calls):              # alternating, so a busy moment on a shared machine falls on all
        for k, fn in runs.items():
            ms[k].append(sample(fn, inner))
    return ms


def measure(kind, rgb, calls, inner, base, emit):
    frames, H, W, _ = rgb.shape
    counts = hip.gif_histogram(rgb)
    labels, ncolors = hip.gif_boxes(counts)
    pal = hip.gif_palette(rgb, labels)
    idx = hip.gif_map(rgb, pal, ncolors)
    quant = timed({"histogram": lambda: hip.gif_histogram(rgb, out=counts), "boxes": lambda: hip.gif_boxes(counts, labels=labels, ncolors=ncolors),
                   "palette": lambda: hip.gif_palette(rgb, labels, out=pal), "map": lambda: hip.gif_map(rgb, pal, ncolors, out=idx)}, calls, inner)
    for seg in SEG_PIXELS:
        out, offsets = hip.gif_lzw(idx, seg)
        ms = dict(quant)
        ms.update(timed({"lzw": lambda: hip.gif_lzw(idx, seg, out=out)}, calls, inner))
        ends = offsets.cpu().tolist()
        total = ends[-1]
        host_off, host_pal = torch.empty(frames + 1, dtype=torch.int64).pin_memory(), torch.empty(pal.shape, dtype=torch.uint8).pin_memory()
        host_out = torch.empty(total, dtype=torch.uint8).pin_memory()
        copies = {"d2h_offsets": lambda: host_off.copy_(offsets, non_blocking=True), "d2h_palettes": lambda: host_pal.copy_(pal, non_blocking=True),
                  "d2h_bytes": lambda: host_out.copy_(out[:total], non_blocking=True)}
        for fn in copies.values():
            fn()
        torch.cuda.synchronize()
        for k, fn in copies.items():
            ms[k] = [sample(fn, 1) for _ in range(calls)]
        data, pals, head = host_out.numpy().tobytes(), host_pal.numpy().tobytes(), gif.frame_header(W, H)
        framing = []
        for _ in range(max(3, calls // 2)):
            t0 = time.perf_counter()
            b"".join(head + pals[768 * f:768 * (f + 1)] + data[ends[f]:ends[f + 1]] for f in range(frames))
            framing.append(1e3 * (time.perf_counter() - t0))
        w = gif.GIFWriter(os.devnull, W, H, seg_pixels=seg)
        w.write(rgb)
        whole = []
        for _ in range(max(3, calls // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w.write(rgb)
            whole.append(1e3 * (time.perf_counter() - t0))
        w.close()
        first = gif.gif_header(W, H) + head + pals[:768] + data[:ends[1]] + gif.TRAILER
        want = pal[0].cpu().numpy()[idx[0].cpu().numpy()].reshape(H, W, 3)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(first)).convert("RGB")), want), "frame 0 does not decode to palette[indices]"
        rec = {"what": "gif stages + copies + host framing beside Pillow's save_all", "content": kind, "frames": frames, "width": W, "height": H,
               "seg_pixels": seg, "calls": calls, "inner": inner, "rgb_bytes": rgb.numel(), "bytes_to_host": total + 768 * frames + 8 * (frames + 1),
               "gpu_image_bytes_per_frame": total / frames, "ncolors_min": int(ncolors.min()),
               "workspace_bytes": int(hip.load().vface_gif_lzw_workspace_bytes(W * H, frames, seg)),
               "host_framing_ms_median": statistics.median(framing), "write_call_ms_median": statistics.median(whole),
               "write_call_ms_min": min(whole), "write_call_ms_max": max(whole)}
        for k, v in ms.items():
            rec[k + "_us_median"], rec[k + "_us_min"], rec[k + "_us_max"] = 1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v)
        rec["gpu_ms_per_frame"] = rec["write_call_ms_median"] / frames
        rec.update(base)
        rec["pillow_over_gpu"] = rec["pillow_ms_per_frame"] / rec["gpu_ms_per_frame"]
        emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--pillow_frames", type=int, default=4)
    ap.add_argument("--frames", type=int, nargs="*", default=list(FRAMES))
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("An MI355X is required: there is nothing to time without one.")
    dev = torch.device("cuda", 0)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for W, H in SIZES:
        for kind in CONTENTS:
            whole = content(kind, max(a.frames), W, H, dev)
            secs, size = pillow(whole, a.pillow_frames)
            base = {"pillow_ms_per_frame": 1e3 * secs, "pillow_file_bytes_per_frame": size, "pillow_frames": min(a.pillow_frames, max(a.frames))}
            for frames in a.frames:
                measure(kind, whole[:frames].contiguous(), a.calls, a.inner, base, emit)


if __name__ == "__main__":
    main()
