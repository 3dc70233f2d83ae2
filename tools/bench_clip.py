#!/usr/bin/env python3
"""Milliseconds per frame of E = FrozenCLIPEmbedder (ViT-L/14, visual_projection, mapper2, final_ln2) on the MI355X, through
``vface_amd.clip.ClipEngine.encode_from_frames`` on 512 x 512 frames (the resize is inside the patch gather), at B = 8 and 32.

    python tools/bench_clip.py [--batches 8 32] [--dtype fp16] [--reps 20] [--warmup 3]

Prints one JSON line per batch size: the median over ``reps`` of a device-event window around one eager call (all launches on the
current stream), its spread, and ms per frame.  Weights and frames are synthetic (seeded).  The useful work is 2 x parameters x
tokens multiply-adds per frame plus the attention's (counted below from the shapes): the rate is that over the measured time, an
end-to-end figure of the encoder, not a kernel's share of peak.  It gates nothing; the number is recorded in DESIGN 9 beside the
UNet's ms per frame.  No GPU: the run fails, it does not fall back."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vface_amd import clip  # noqa: E402
from vface_amd.utils import synth  # noqa: E402


def flops_per_frame(cfg) -> float:
    C, I, L, T = cfg["hidden"], cfg["mlp"], cfg["layers"], (cfg["image"] // 14) ** 2 + 1
    per_token = L * (4 * C * C + 2 * C * I)                    # q, k, v, out and the two MLP matrices, multiply-adds
    attn = L * 2 * T * T * C                                   # Q K^T and P V over all heads
    head = C * 768 + 5 * (2 * 768 * 768 + 8 * 768 * 768)
    return 2.0 * (T * per_token + attn + (T - 1) * 640 * C + head)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512, help="side of the frames")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip.py needs the MI355X")
    dt = torch.float16 if opt.dtype == "fp16" else torch.bfloat16
    cfg = dict(clip.VIT_L14)
    sd = {k: synth.synth_tensor(k, s, 5) for k, s in clip.state_shapes(cfg).items()}
    eng = clip.ClipEngine(sd, cfg, dt, "cuda:0")
    del sd
    for B in opt.batches:
        frames = torch.stack([synth.synth_normal(f"bench_clip.{f}", (3, opt.size, opt.size)).clamp(-1, 1) for f in range(B)]).cuda()
        for _ in range(opt.warmup):
            out = eng.encode_from_frames(frames)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
        ms = []
        for _ in range(opt.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.encode_from_frames(frames)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        med = statistics.median(ms)
        print(json.dumps({"bench": "clip_encode_from_frames", "dtype": opt.dtype, "B": B, "frame": opt.size, "ms_per_call": round(med, 3),
                          "ms_per_frame": round(med / B, 4), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                          "reps": opt.reps, "tflops_end_to_end": round(flops_per_frame(cfg) * B / (med * 1e-3) / 1e12, 1),
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
