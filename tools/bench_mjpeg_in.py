"""Timing of the Motion-JPEG way in (scripts/mjpeg_in.py, csrc/mjpeg_in.hip): the three launches of the decoder and the colour
conversion behind them, the upload they need, the Y4M ``video_in`` stage (upload + convert) on the same frames in the same run, and
Pillow's (libjpeg-turbo's) decode of the same files on the host.

    python tools/bench_mjpeg_in.py [--calls 10] [--quality 90] [--subseq_bytes 128 [64 256 ..]] [--cases NAME ..]

Five cases, one JSON line each:
  writer_1080p   32 frames of 1920 x 1080 as ``MJPEGWriter`` writes them: one restart interval per MCU row, so 68 lanes per frame
  pillow_1080p   the same frames as Pillow writes them: NO restart markers (what ffmpeg writes too), so ONE interval per frame
  writer_512     8 frames of 512 x 512 from the writer
  pillow_1080p_flat        32 flat frames from Pillow: the stream on which guessed states never fall into step with the true ones
  pillow_1080p_noise_q100  8 frames of uniform noise from Pillow at quality 100: long codes, late synchronisation
The frames of the first three are smooth seeded pictures (sinusoids, a ramp, sigma = 4 noise): noise alone would not compress.
``decode_entropy`` is timed in BOTH forms in the same run -- ``hip.jpeg_decode_entropy`` (one lane per restart interval) and
``hip.jpeg_decode_entropy_parallel`` at every ``--subseq_bytes`` -- and the two results are compared bit for bit before anything is
timed; ``rounds`` (synchronisation rounds that changed a state, summed over the call) and the subsequence count stand beside each
parallel time.  Each launch is timed between two HIP events, ``--calls`` samples after a warm-up, alternating so that a busy moment
on a shared machine falls on all of them; medians, minima and maxima are reported.  Host-to-device copies come from pinned buffers."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vface_amd import hip  # noqa: E402
from vface_amd.scripts import mjpeg, mjpeg_in  # noqa: E402

DEV = torch.device("cuda", 0)
CASES = (("writer_1080p", 32, 1920, 1080, "writer"), ("pillow_1080p", 32, 1920, 1080, "pillow"), ("writer_512", 8, 512, 512, "writer"),
         ("pillow_1080p_flat", 32, 1920, 1080, "pillow_flat"), ("pillow_1080p_noise_q100", 8, 1920, 1080, "pillow_noise"))


def pictures(frames, W, H):
    gen = torch.Generator(device=DEV).manual_seed(0)
    f, y, x = torch.meshgrid(torch.arange(frames, device=DEV), torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    planes = [128 + 60 * torch.sin(x / 11.0 + f) + 40 * torch.cos(y / 7.0) + 0.02 * x, 128 + 70 * torch.sin((x + y) / 17.0 + 0.5 * f) + 0.03 * y,
              100 + 50 * torch.cos(x / 5.0) * torch.sin(y / 13.0 + f) + 0.02 * (x + y)]
    rgb = torch.stack(planes, dim=-1) + 4.0 * torch.randn(frames, H, W, 3, device=DEV, generator=gen)
    return rgb.round().clamp(0, 255).to(torch.uint8)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def measure(name, frames, W, H, source, calls, quality, sizes):
    if source == "pillow_flat":
        rgb = torch.tensor([90, 140, 200], dtype=torch.uint8, device=DEV).expand(frames, H, W, 3).contiguous()
    elif source == "pillow_noise":
        rgb = torch.randint(0, 256, (frames, H, W, 3), dtype=torch.uint8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        quality = 100
    else:
        rgb = pictures(frames, W, H)
    host = rgb.cpu().numpy()
    if source == "writer":
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "clip.avi")
            with mjpeg.MJPEGWriter(path, W, H, quality=quality) as w:
                w.write(rgb)
            with mjpeg_in.MJPEGReader(path) as r:
                read = r.read(range(frames))
                jpegs = [r.frame_bytes(i) for i in range(frames)]
    else:
        from PIL import Image
        jpegs = []
        for i in range(frames):
            buf = io.BytesIO()
            Image.fromarray(host[i]).save(buf, "JPEG", quality=quality, subsampling=2)
            jpegs.append(buf.getvalue())
        records = []
        for i, jpeg in enumerate(jpegs):
            frame = mjpeg_in.parse_jpeg(jpeg, name, i)
            records.append(mjpeg_in.FrameRecord(i, jpeg[frame.scan[0]:frame.scan[1]], frame.restart, mjpeg_in.quant_block(frame),
                                                mjpeg_in.huffman_block(frame)))
        read = mjpeg_in.MJPEGFrames(name, W, H, records)
    packed = {k: v.pin_memory() for k, v in read.packed().items()}
    mcus = mjpeg_in.mcu_count(W, H)
    most = max(hip.jpeg_interval_count(mcus, r.restart) for r in read.records)
    dev = {k: v.to(DEV) for k, v in packed.items()}
    state = {}

    def scan_index():
        state["ranges"], state["status"] = hip.jpeg_scan_index(dev["scans"], dev["offsets"], dev["lengths"], dev["restart"], mcus, most)

    def entropy():
        state["coef"], _ = hip.jpeg_decode_entropy(dev["scans"], state["ranges"], state["status"], dev["restart"], dev["tables"], mcus)

    def entropy_parallel(size):
        def run():
            state["coef_parallel"], _ = hip.jpeg_decode_entropy_parallel(dev["scans"], state["ranges"], state["status"], dev["restart"],
                                                                         dev["tables"], mcus, size)
        return run

    def planes():
        state["rows"] = hip.jpeg_planes(state["coef"], dev["quant"], W, H)

    def colour():
        state["rgb"] = hip.yuv420_to_rgb(state["rows"], W, H, matrix="bt601", full_range=True, chroma="centre")

    def upload():
        for k, v in packed.items():
            dev[k].copy_(v, non_blocking=True)
    steps = {"h2d_scans_and_tables": upload, "scan_index": scan_index, "decode_entropy": entropy, "planes": planes, "yuv420_to_rgb": colour}
    # the Y4M stage on the same frames: the I420 rows of the decoded pictures, uploaded and converted
    for fn in steps.values():
        fn()
    torch.cuda.synchronize()
    assert state["status"].cpu().tolist() == [0] * frames, state["status"].cpu().tolist()
    # the parallel form: the same coefficients, its round counts, then a step of its own per subsequence size
    rounds = {}
    for size in sizes:
        coef, status, r = hip.jpeg_decode_entropy_parallel(dev["scans"], state["ranges"], state["status"], dev["restart"], dev["tables"], mcus,
                                                           size, return_rounds=True)
        assert torch.equal(coef, state["coef"]) and status.cpu().tolist() == [0] * frames, (name, size)
        rounds[size] = int(r.sum())
        steps[f"decode_entropy_parallel_{size}"] = entropy_parallel(size)
    i420_host = state["rows"].cpu().pin_memory()
    i420_dev = torch.empty_like(state["rows"])
    y4m_rgb = torch.empty_like(state["rgb"])

    def y4m_stage():
        i420_dev.copy_(i420_host, non_blocking=True)
        hip.yuv420_to_rgb(i420_dev, W, H, matrix="bt601", full_range=True, chroma="centre", out=y4m_rgb)
    steps["y4m_video_in"] = y4m_stage
    y4m_stage()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(calls):
        for k, fn in steps.items():
            ms[k].append(timed(fn)[0])
    from PIL import Image
    pillow = []
    for _ in range(3):
        t0 = time.perf_counter()
        for jpeg in jpegs:
            Image.open(io.BytesIO(jpeg)).convert("RGB").load()
        pillow.append((time.perf_counter() - t0) * 1e3)
    rec = {"what": "motion-JPEG in", "case": name, "frames": frames, "width": W, "height": H, "quality": quality, "calls": calls,
           "restart_interval_mcus": read.records[0].restart, "lanes_per_frame": most, "scan_bytes": int(sum(len(r.scan) for r in read.records)),
           "uploaded_bytes": int(sum(v.numel() * v.element_size() for v in packed.values())), "i420_bytes": int(i420_host.numel()),
           "pillow_cpu_decode_ms_median": statistics.median(pillow), "pillow_cpu_decode_ms_min": min(pillow)}
    for k, v in ms.items():
        rec[k + "_ms_median"], rec[k + "_ms_min"], rec[k + "_ms_max"] = statistics.median(v), min(v), max(v)
    rec["subseq_bytes"] = list(sizes)
    for size in sizes:
        rec[f"rounds_{size}"] = rounds[size]
        # (about: every frame's bytes spread evenly over its intervals)
        rec[f"subsequences_{size}"] = sum((len(r.scan) // hip.jpeg_interval_count(mcus, r.restart) // size + 1)
                                          * hip.jpeg_interval_count(mcus, r.restart) for r in read.records)
    rec["entropy_auto"] = mjpeg_in.entropy_path(read, mcus)
    rec["longest_interval_bytes"] = max(len(r.scan) / hip.jpeg_interval_count(mcus, r.restart) for r in read.records)
    rec["decoder_ms_median"] = sum(rec[k + "_ms_median"] for k in ("scan_index", "decode_entropy", "planes", "yuv420_to_rgb"))
    rec["video_in_ms_median"] = rec["decoder_ms_median"] + rec["h2d_scans_and_tables_ms_median"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subseq_bytes", type=int, nargs="+", default=[mjpeg_in.SUBSEQ_BYTES],
                    help="subsequence sizes of the parallel entropy decoder to time (multiples of 4 in 4..1024): a sweep")
    ap.add_argument("--cases", nargs="+", default=[c[0] for c in CASES], choices=[c[0] for c in CASES])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("An MI355X is required: there is nothing to time without one.")
    for name, frames, W, H, source in CASES:
        if name in a.cases:
            print(json.dumps(measure(name, frames, W, H, source, a.calls, a.quality, a.subseq_bytes)), flush=True)


if __name__ == "__main__":
    main()
