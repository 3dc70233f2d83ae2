#!/usr/bin/env python3
"""Milliseconds per frame of the identity features -- ``IDLoss.extract_feats`` = the pooling and crop chain + ArcFace IR-SE50 -- on the
MI355X, through ``vface_amd.arcface.ArcFaceEngine.extract_feats_from_frames`` on 512 x 512 frames with a mask (the per-batch call of
the inference script: the resize to the CLIP image is inside ``vface_id_prep``), at B = 1, 8 and 32.

    python tools/bench_arcface.py [--batches 1 8 32] [--dtype fp16] [--reps 20] [--warmup 3]

Prints one JSON line per batch size: the median over ``reps`` of a device-event window around one eager call (all launches on the
current stream), its spread, and ms per frame.  Weights and frames are synthetic (seeded).  The network is 6.3 G multiply-adds per
frame (counted below from the shapes); the rate is that over the measured time, an end-to-end figure (about 250 eager launches,
their gaps included), not a kernel's share of peak.  It gates nothing; the number is recorded in DESIGN 9 beside the UNet's ms per
frame.  No GPU: the run fails, it does not fall back."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vface_amd import arcface  # noqa: E402
from vface_amd.utils import synth  # noqa: E402


def flops_per_frame() -> float:
    macs, hw = 112 * 112 * 27 * 64, 112 * 112
    for cin, depth, stride in arcface.UNITS:
        out = hw // (stride * stride)
        macs += hw * 9 * cin * depth + out * 9 * depth * depth + (out * cin * depth if cin != depth else 0) + 2 * depth * depth // 16
        hw = out
    return 2.0 * (macs + 25088 * 512)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512, help="side of the frames")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_arcface.py needs the MI355X")
    dt = torch.float16 if opt.dtype == "fp16" else torch.bfloat16
    from vface_amd.src.Face_models.encoders.model_irse import Backbone
    net = synth.fill_arcface_(Backbone(112, 50, "ir_se", 0.6), seed=5)
    eng = arcface.ArcFaceEngine(net.state_dict(), dt, "cuda:0")
    del net
    for B in opt.batches:
        frames = torch.stack([synth.synth_normal(f"bench_arcface.{f}", (3, opt.size, opt.size)).clamp(-1, 1) for f in range(B)]).cuda()
        mask = synth.synth_mask(B, opt.size, opt.size).cuda()
        for _ in range(opt.warmup):
            out = eng.extract_feats_from_frames(frames, mask)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        ms = []
        for _ in range(opt.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.extract_feats_from_frames(frames, mask)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        med = statistics.median(ms)
        print(json.dumps({"bench": "arcface_extract_feats_from_frames", "dtype": opt.dtype, "B": B, "frame": opt.size,
                          "ms_per_call": round(med, 3), "ms_per_frame": round(med / B, 4), "min_ms": round(min(ms), 3),
                          "max_ms": round(max(ms), 3), "reps": opt.reps,
                          "tflops_end_to_end": round(flops_per_frame() * B / (med * 1e-3) / 1e12, 1),
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
