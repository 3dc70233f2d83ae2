#!/usr/bin/env python3
"""Timings of the widened rows at the sizes the 8-frame / 16-frame workloads use, HIP events on the launch
stream: the RAFT-shaped flow producer (F - 1 pairs of 512 x 512 frames, 20 updates), the paste-back (F decoded 512 x 512
crops -> 1024 canvas -> 1024 x 1024 frames) and the frame intake (F frames of 1080 x 1920 -> 1024 x 1024 aligned crops -> 512 x 512
sampler tensors), each next to the same Pillow calls on the host, and the face parser (F aligned 1024 x 1024 crops -> 512 x 512 label
maps) launch by launch.
usage: python tools/bench_widening.py [--frames 8] [--only intake | parse]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vface_amd.utils import synth

DEV = "cuda:0"


def time_ms(fn, iters=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--frame_size", type=int, default=1024)
    ap.add_argument("--only", choices=["intake", "parse"], default=None, help="time this row alone")
    a = ap.parse_args()
    F_, R, S = a.frames, a.res, a.frame_size
    if a.only == "intake":
        return bench_intake(F_, R)
    if a.only == "parse":
        return bench_parse(F_)
    from vface_amd.raft import RAFT
    from vface_amd.scripts import temporal_flow as tflow
    from vface_amd.scripts.paste_back import PasteBack
    from vface_amd.scripts.inputs import _quad_coeffs
    raft = RAFT()
    synth.fill_module_(raft, seed=0, prefix="raft.")
    raft = raft.to(DEV).eval()
    video = torch.stack([synth.synth_normal(f"w.img{f}", (3, R, R)).clamp(-1, 1) for f in range(F_)]).to(DEV)
    t = time_ms(lambda: tflow.return_flow(video, raft), iters=3)
    print(f"return_flow: {F_ - 1} pairs of {R}x{R}, 20 updates: {t:8.1f} ms  ({t / (F_ - 1):6.1f} ms per pair)", flush=True)
    for it in (1, 12):
        tt = time_ms(lambda: raft(video[1:], video[:-1], num_flow_updates=it), iters=3)
        print(f"   the same with {it:2d} update(s): {tt:8.1f} ms", flush=True)
    dec = torch.stack([synth.synth_normal(f"w.dec{f}", (3, R, R)) * 0.6 for f in range(F_)]).to(DEV)
    frames = torch.randint(0, 256, (F_, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(DEV)
    q = S / 4.0
    co = np.stack([_quad_coeffs(1024, [(q + 3 * f, q), (3 * q, q + f), (3 * q - f, 3 * q), (q, 3 * q - 2 * f)]) for f in range(F_)])
    pb = PasteBack(H=R, W=R, device=DEV, encode_decode=None)
    t = time_ms(lambda: pb.paste(dec, frames, co))
    print(f"paste-back without the background round trip: {F_} frames {S}x{S}: {t:8.2f} ms  ({t / F_ * 1e3:6.0f} us per frame)", flush=True)
    from vface_amd.ldm.models.autoencoder import FFHQ_VAE_CONFIG, AutoencoderKL
    vae = AutoencoderKL(**FFHQ_VAE_CONFIG, compute_dtype=torch.float16)
    synth.fill_module_(vae, seed=0, prefix="vae.")
    vae = vae.to(DEV)
    rt = lambda x: vae.decode(vae.encode(x).mode(1.0))
    pb2 = PasteBack(H=R, W=R, device=DEV, encode_decode=rt)
    t2 = time_ms(lambda: pb2.paste(dec, frames, co), iters=3)
    print(f"paste-back with the VAE encode + decode of the background (:610-623): {t2:8.1f} ms  ({t2 / F_:6.1f} ms per frame)", flush=True)
    # the host route of the reference for scale: one frame through Pillow (resize, transform, composite), decoded crop already on the host
    from PIL import Image
    import time
    x = torch.clamp((dec[0] + 1.0) / 2.0, 0, 1).permute(1, 2, 0).cpu().numpy()
    fr = frames[0].cpu().numpy()
    t0 = time.time()
    for _ in range(3):
        img = Image.fromarray((255. * x).astype(np.uint8)).resize((1024, 1024), Image.BILINEAR)
        sw = img.convert("RGBA")
        sw.putalpha(255)
        bg = Image.fromarray(fr).convert("RGBA")
        bg.alpha_composite(sw.transform((S, S), Image.PERSPECTIVE, co[0], Image.BILINEAR))
    print(f"the same three Pillow calls on the host (no VAE, no PCIe): {(time.time() - t0) / 3 * 1e3:8.1f} ms per frame", flush=True)

    bench_intake(F_, R)
    bench_parse(F_)


def bench_parse(F_, size=1024):
    """The face parser (vface_amd/parsing.py) on F aligned crops of size x size: every launch of one ``FaceParser.labels`` call with
    its own HIP-event time and the HBM bytes it has to move (compulsory traffic: operands once, result once), then the call as a
    whole.  The per-launch times are taken in one pass with an event pair round each launch; the whole call is timed without them."""
    from vface_amd import hip
    from vface_amd.pretrained.face_parsing import FaceParser
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    import cases_parse as cp
    crops = torch.from_numpy(np.stack([cp.crop(size // 2, size // 2, 50 + f) for f in range(F_)])).to(DEV)
    fp = FaceParser(seg_ckpt=None, size=size, device=DEV)
    fp.labels(crops)
    torch.cuda.synchronize()

    def out_rows(n, H, W, st, up):
        vh, vw = (2 * H, 2 * W) if up else (H, W)
        return n * ((vh - 1) // st + 1) * ((vw - 1) // st + 1)
    nbytes = {
        "parse_prefilter": lambda a, k: a[0].numel() + a[1].shape[0] * 16,
        "im2col": lambda a, k: k["nimg"] * k["H"] * k["W"] * k["C_"] * 2 + a[1].numel() * 2,
        "gemm": lambda a, k: (k["M"] * k["K"] + k["N"] * k["K"]) * 2 + k["M"] * k["N"] * a[2].element_size(),
        "conv3x3": lambda a, k: (k["nimg"] * k["H"] * k["W"] * k["cin"] + 9 * k["cin"] * k["cout"]) * 2
        + out_rows(k["nimg"], k["H"], k["W"], k.get("stride", 1), k.get("upsample", False)) * k["cout"] * 2,
        "channel_norm_act": lambda a, k: k["M"] * k["C_"] * 2 * (2 + (k.get("residual") is not None)),
        "channel_stats": lambda a, k: k["nimg"] * k["hw"] * k["C_"] * 2 + k["nimg"] * k["C_"] * 8,
        "pooled_linear": lambda a, k: k["N"] * k["K"] * 4 + k["nimg"] * (k["K"] + k["N"]) * 4,
        "channel_gate": lambda a, k: k["M"] * k["C_"] * 2 * (2 + (k.get("rten") is not None)),
        "maxpool3x3s2": lambda a, k: k["nimg"] * k["H"] * k["W"] * k["C_"] * 2 + a[1].shape[0] * k["C_"] * 2,
        "upsample_argmax_u8": lambda a, k: a[0].numel() * 4 + k["F"] * k["H"] * k["W"],
    }
    rows, saved = [], {}
    for name, fb in nbytes.items():
        saved[name] = getattr(hip, name)

        def wrapped(*a, _name=name, _fb=fb, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = saved[_name](*a, **k)
            e1.record()
            shape = "x".join(str(k[key]) for key in ("nimg", "F", "M", "H", "W", "hw", "cin", "C_", "K", "cout", "N") if key in k)
            rows.append((_name, shape, e0, e1, _fb(a, k)))
            return r
        setattr(hip, name, wrapped)
    try:
        fp.labels(crops)
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(hip, name, fn)
    print(f"face parser: {F_} crops {size}x{size} -> {size // 2}x{size // 2} label maps, {len(rows)} launches (one pass, an event pair each)", flush=True)
    total, tbytes = 0.0, 0
    for name, shape, e0, e1, nb in rows:
        t = e0.elapsed_time(e1)
        total, tbytes = total + t, tbytes + nb
        print(f"   {name:20s} {shape:28s} {t * 1e3:8.1f} us  {nb / 1e6:8.2f} MB  {nb / max(t, 1e-6) / 1e6:7.1f} GB/s", flush=True)
    print(f"   sum of the launches {total:8.2f} ms  {tbytes / 1e6:8.1f} MB  ({total / F_:6.2f} ms per frame)", flush=True)
    t = time_ms(lambda: fp.labels(crops))
    print(f"   FaceParser.labels as one call (median of 5, allocations included): {t:8.2f} ms  ({t / F_:6.2f} ms per frame)", flush=True)


def bench_intake(F_, R, image_size=1024, Hs=1080, Ws=1920):
    """The frame intake (scripts/intake.py) at the reference's sizes: F frames of 1080 x 1920 -> 1024 x 1024 aligned crops -> R x R
    sampler tensors, launch by launch with the HBM bytes each one has to move (compulsory traffic: every input byte it touches
    once, every output byte once), and the same Pillow / numpy / torch calls on the host for one frame."""
    import time
    from PIL import Image
    from vface_amd import hip
    from vface_amd.scripts.intake import FrameIntake, crop_plan
    from vface_amd.scripts.intake import REMOVE_MASK_TAR_FFHQ
    S, lat = image_size, (R // 8, R // 8)
    frames = torch.randint(0, 256, (F_, Hs, Ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(DEV)
    labels = torch.randint(0, 19, (F_, R, R), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).to(DEV)
    quads = np.empty((F_, 4, 2))
    for f in range(F_):          # a face 600 px wide, rotated 7 degrees, drifting
        th = np.deg2rad(7.0)
        c, x = np.array([Ws / 2 + 5.0 * f, Hs / 2 + 2.0 * f]), 300.0 * np.array([np.cos(th), np.sin(th)])
        y = np.flipud(x) * [-1, 1]
        quads[f] = np.stack([c - x - y, c - x + y, c + x + y, c + x - y])
    fi = FrameIntake(image_size=S, H=R, W=R, latent=lat, device=DEV)
    plans = [crop_plan(q, Ws, Hs, S) for q in quads]
    assert all(p[0] <= 1 for p in plans)
    co = torch.from_numpy(np.stack([p[3] for p in plans])).to(DEV)
    win = torch.tensor([p[2] for p in plans], dtype=torch.int32).to(DEV)
    window_px = sum((p[2][2] - p[2][0]) * (p[2][3] - p[2][1]) for p in plans)
    crops = hip.quad_crop(frames, co, win, S)
    tx, ty = fi._table(S, R, "bicubic"), fi._table(S, R, "bicubic")
    half = hip.resample_u8(crops, R, 0, *tx)
    small = hip.resample_u8(half, R, 1, *ty)
    member = hip.label_membership(REMOVE_MASK_TAR_FFHQ, DEV)
    rows = [("quad_crop", lambda: hip.quad_crop(frames, co, win, S), window_px * 3 + F_ * S * S * 3),
            ("resample_u8 bicubic, x", lambda: hip.resample_u8(crops, R, 0, *tx), F_ * (S * S * 3 + S * R * 3)),
            ("resample_u8 bicubic, y", lambda: hip.resample_u8(half, R, 1, *ty), F_ * (S * R * 3 + R * R * 3)),
            ("dataset_tensors (+ mask_latent)", lambda: hip.dataset_tensors(small, labels, member, lat),
             F_ * (R * R * 4 + R * R * 7 * 4 + lat[0] * lat[1] * 4))]
    print(f"frame intake: {F_} frames {Hs}x{Ws} -> {S}x{S} crops -> {R}x{R} tensors (median of 5, output allocation included)", flush=True)
    total = 0.0
    for name, fn, nbytes in rows:
        t = time_ms(fn)
        total += t
        print(f"   {name:34s} {t * 1e3:8.1f} us  {nbytes / 1e6:7.1f} MB  {nbytes / t / 1e6:7.1f} GB/s", flush=True)
    print(f"   sum of the launches                {total * 1e3:8.1f} us  ({total / F_ * 1e3:6.1f} us per frame)", flush=True)
    t = time_ms(lambda: fi(frames, quads, labels, REMOVE_MASK_TAR_FFHQ))
    print(f"   FrameIntake.__call__ (host scalars, coefficient upload, inv_transforms included): {t:8.2f} ms", flush=True)
    # the reference's host route for one frame: crop_image (:115-123, :142), resize (:139), tensors (:157-221), Resize (:459)
    fr, lab, q0 = frames[0].cpu().numpy(), labels[0].cpu().numpy(), quads[0]
    t0 = time.time()
    for _ in range(3):
        _, _, window, _ = crop_plan(q0, Ws, Hs, S)
        img = Image.fromarray(fr).crop(window)
        img = img.transform((S, S), Image.QUAD, (q0 - window[0:2] + 0.5).flatten(), Image.BILINEAR)
        img_p = img.convert("RGB").resize((R, R))
        image = (torch.from_numpy(np.array(img_p)).permute(2, 0, 1).float().div(255) - 0.5) / 0.5
        conv = np.zeros_like(lab)
        conv[np.isin(lab, REMOVE_MASK_TAR_FFHQ)] = 255
        m = 1 - torch.from_numpy(conv)[None].float().div(255)
        inpaint = image * m
        torch.nn.functional.interpolate(m[None], size=lat, mode="bilinear", align_corners=False)
    print(f"   the same Pillow / numpy / torch calls on the host (no PCIe): {(time.time() - t0) / 3 * 1e3:8.1f} ms per frame", flush=True)


if __name__ == "__main__":
    main()
