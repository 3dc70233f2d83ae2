"""Timing of the PNG decoder (hip.png_inflate / hip.png_inflate_parallel + hip.png_unfilter, csrc/png_in.hip, csrc/png_in_par.hip;
scripts/png_in.py) stage by stage, beside the default path -- Pillow's ``Image.open().convert("RGB")`` on one core -- on the same
files in the same run.

    python tools/bench_png_in.py [--calls 7] [--pillow_frames 4] [--sizes 512x512,1920x1080] [--batches 1,6,32] [--out sweep.jsonl]
                                 [--chunks 4096,8192,16384,32768,65536] [--contents smooth,noisy,noise] [--writers pillow,encoder]

For batches of 1, 6 and 32 frames of 512 x 512 and 1920 x 1080, on three kinds of content -- a smooth synthetic gradient, the same with
Gaussian noise of sigma 2 (the closest here to decoded video) and uniform noise -- as Pillow wrote them (level 6) and as
``png.PNGEncoder`` wrote them: the host's parse and CRC of the files (a host clock), the one upload from pinned memory, the inflate
and the unfilter (``--calls`` samples each between two HIP events; the median and the spread are printed), the one small copy back,
and ``png_in.decode`` whole (a host clock around a call that ends in the copy back).  Pillow decodes ``--pillow_frames`` of the same
files from memory.  Frame 0 of every run is compared with Pillow's first.  The parallel inflate runs in the same run on the same buffers: ``inflate_parallel`` holds the whole call per ``chunk_bytes`` of
``--chunks`` (HIP events, as the serial call), the share of files that fell back and the segments per file at each; ``parallel_stages``
the six launches one by one at the default chunk size -- ``find``, ``count``, ``validate``, ``write``, ``resolve``, ``fallback`` -- as
the profiler saw them in one call; ``decode_whole_parallel`` is ``png_in.decode(inflate="parallel")``.  Its rows are compared with
the serial call's.  Prints one JSON line per (size, content, writer, batch);
``--out`` also appends them to a file.  No threshold: these are the numbers of DESIGN §9, "Frames in, PNG"."""
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
from bench_png import content  # noqa: E402
from vface_amd import hip  # noqa: E402
from vface_amd.scripts import png, png_in  # noqa: E402

CONTENTS = ("smooth", "noisy", "noise")


def events(fn, calls):
    """``calls`` samples of fn between two HIP events, one warm-up in front -> milliseconds."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def clock(fn, calls):
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def pillow_files(rgb):
    out = []
    for frame in rgb:
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, "PNG")
        out.append(buf.getvalue())
    return out


def pillow_decode(files, count):
    """Pillow's decode of ``count`` files spread over the batch -> median milliseconds per frame."""
    picks = sorted({int(i) for i in np.linspace(0, len(files) - 1, min(count, len(files)))})
    ms = []
    for i in picks:
        t0 = time.perf_counter()
        with Image.open(io.BytesIO(files[i])) as im:
            np.asarray(im.convert("RGB"))
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


STAGE_KERNELS = {"find": "png_par_find_kernel", "count": "png_par_count_kernel", "validate": "png_par_validate_kernel",
                 "write": "png_par_write_kernel", "resolve": "png_par_resolve_kernel", "fallback": "png_inflate_kernel"}


def stage_ms(fn):
    """The device time of each launch of ONE call of fn, by kernel name, as the profiler records it -> {stage: ms}, or None where
    the profiler yields no kernel records."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    found = {}
    for e in prof.events():
        for stage, kernel in STAGE_KERNELS.items():
            if kernel in e.name:
                found[stage] = round(found.get(stage, 0.0) + getattr(e, "device_time", getattr(e, "cuda_time", 0.0)) / 1e3, 4)
    return found or None


def measure_parallel(streams, offsets, lengths, expect, rows, meta, chunks, calls, dev):
    """The parallel inflate on the buffers of the serial measurement -> the record's ``inflate_parallel`` and ``parallel_stages``."""
    F = offsets.numel()
    want, want_meta = rows.clone(), meta[:5].clone()
    out, info = torch.empty_like(rows), torch.empty((F, 4), dtype=torch.int32, device=dev)
    sweep = {}
    for chunk_bytes in chunks:
        def call():
            hip.png_inflate_parallel(streams, offsets, lengths, expect, chunk_bytes, out=out, meta=meta[:5], info=info)
        ms = events(call, calls)
        assert torch.equal(out, want) and torch.equal(meta[:5], want_meta), f"the parallel inflate differs from the serial one at {chunk_bytes}"
        host = info.cpu().numpy()
        sweep[str(chunk_bytes)] = {**stats(ms), "fell_back": int((host[:, 0] == 0).sum()), "segments_per_file": round(float(host[:, 0].mean()), 1)}
    stages = stage_ms(lambda: hip.png_inflate_parallel(streams, offsets, lengths, expect, hip.PNG_INFLATE_CHUNK_BYTES, out=out, meta=meta[:5], info=info))
    return sweep, stages


def measure(files, W, H, dev, calls, pillow_frames, chunks=()):
    F = len(files)
    with Image.open(io.BytesIO(files[0])) as im:
        first = np.asarray(im.convert("RGB"))
    parsed = []
    parse_ms = clock(lambda: parsed.append([png_in.parse_png(d, f"<{k}>") for k, d in enumerate(files)]), 3)
    frames = png_in.PNGFrames(W, H, parsed[-1])
    got = png_in.decode(frames, dev)
    assert np.array_equal(got[0].cpu().numpy(), first), "frame 0 differs from Pillow's"
    bpp = frames[0].bpp
    expect = (1 + bpp * W) * H
    p = frames.packed()
    buf = torch.empty_like(p["buffer"], device=dev)
    upload_ms = events(lambda: buf.copy_(p["buffer"], non_blocking=True), calls)
    offsets = buf[:8 * F].view(torch.int64)
    lengths = buf[p["lengths_at"]:p["lengths_at"] + 4 * F].view(torch.int32)
    streams = buf[p["streams_at"]:]
    meta = torch.empty((6, F), dtype=torch.int32, device=dev)
    rows = torch.empty((F, expect), dtype=torch.uint8, device=dev)
    rgb = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    inflate_ms = events(lambda: hip.png_inflate(streams, offsets, lengths, expect, out=rows, meta=meta[:5]), calls)
    unfilter_ms = events(lambda: hip.png_unfilter(rows, W, H, bpp, meta[0], out=rgb, status=meta[5]), calls)
    back_ms = clock(lambda: meta.cpu(), calls)
    whole_ms = clock(lambda: png_in.decode(frames, dev), calls)
    assert torch.equal(rgb, got)
    compressed = sum(len(r.body) for r in frames.records)
    extra = {}
    if chunks:
        sweep, stages = measure_parallel(streams, offsets, lengths, expect, rows, meta, chunks, calls, dev)
        assert torch.equal(png_in.decode(frames, dev, inflate="parallel"), got)
        whole_par = clock(lambda: png_in.decode(frames, dev, inflate="parallel"), calls)
        extra = {"inflate_parallel": sweep, "parallel_stages": stages, "decode_whole_parallel": stats(whole_par),
                 "decode_parallel_ms_per_frame": round(statistics.median(whole_par) / F, 4),
                 "auto_takes": png_in.inflate_path("auto", compressed, F)}
    return {**extra, "frames": F, "W": W, "H": H, "bpp": bpp, "compressed_bytes_per_frame": compressed // F, "rgb_bytes_per_frame": H * W * 3,
            "parse_crc_host": stats(parse_ms), "upload": stats(upload_ms), "inflate": stats(inflate_ms), "unfilter": stats(unfilter_ms),
            "copy_back": stats(back_ms), "decode_whole": stats(whole_ms),
            "decode_ms_per_frame": round(statistics.median(whole_ms) / F, 4),
            "gpu_path_ms_per_frame": round((statistics.median(whole_ms) + statistics.median(parse_ms)) / F, 4),
            "pillow_decode_ms_per_frame": round(pillow_decode(files, pillow_frames), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--pillow_frames", type=int, default=4)
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--batches", default="1,6,32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--chunks", default="4096,8192,16384,32768,65536", help="chunk_bytes of the parallel inflate to sweep ('' = serial only)")
    ap.add_argument("--contents", default=",".join(CONTENTS))
    ap.add_argument("--writers", default="pillow,encoder")
    args = ap.parse_args()
    chunks = [int(c) for c in args.chunks.split(",") if c]
    dev = torch.device("cuda", 0)
    batches = [int(b) for b in args.batches.split(",")]
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for kind in args.contents.split(","):
            frames = content(kind, max(batches), W, H, dev)
            written = {"pillow": pillow_files(frames.cpu().numpy()), "encoder": png.PNGEncoder(W, H).encode(frames)}
            for writer, files in written.items():
                if writer not in args.writers.split(","):
                    continue
                for F in batches:
                    rec = {"content": kind, "writer": writer, **measure(files[:F], W, H, dev, args.calls, args.pillow_frames, chunks)}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if args.out:
                        with open(args.out, "a") as f:
                            f.write(line + "\n")


if __name__ == "__main__":
    main()
