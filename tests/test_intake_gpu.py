"""Frame intake on the GPU (csrc/intake.hip, scripts/intake.py): every kernel against live Pillow / torch doing what the reference's
lines do (REFace/src/utils/alignmengt.py:99-145, ldm/data/video_swap_dataset.py:135-240, scripts/VFace_inference_batch.py:459) and
against tests/golden/intake.npz (the reference's own `crop_image` outputs), bit for bit; `FrameIntake.__call__` against the
reference's statement sequence run on the host; the loop intake -> paste-back against Pillow; and the CLI's `--intake`."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import cases_intake as ci  # noqa: E402
import intake_model as model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REMOVE = [1, 2, 3, 5, 6, 7, 9]          # project_ffhq.yaml remove_mask_tar_FFHQ: seven labels


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "intake.npz"), allow_pickle=False)


def pillow_crop_image(frame: np.ndarray, quad: np.ndarray, size: int) -> np.ndarray:
    """crop_image's statements (alignmengt.py:100-123, :142; enable_padding False) with live Pillow."""
    quad = quad.copy()
    img = Image.fromarray(frame)
    x = (quad[3] - quad[1]) / 2
    qsize = np.hypot(*x) * 2
    shrink = int(np.floor(qsize / size * 0.5))
    if shrink > 1:
        rsize = (int(np.rint(float(img.size[0]) / shrink)), int(np.rint(float(img.size[1]) / shrink)))
        img = img.resize(rsize, Image.LANCZOS)
        quad /= shrink
        qsize /= shrink
    border = max(int(np.rint(qsize * 0.1)), 3)
    crop = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))),
            int(np.ceil(max(quad[:, 1]))))
    crop = (max(crop[0] - border, 0), max(crop[1] - border, 0), min(crop[2] + border, img.size[0]),
            min(crop[3] + border, img.size[1]))
    if crop[2] - crop[0] < img.size[0] or crop[3] - crop[1] < img.size[1]:
        img = img.crop(crop)
        quad -= crop[0:2]
    return np.asarray(img.transform((size, size), Image.QUAD, (quad + 0.5).flatten(), Image.BILINEAR))


def rotated_quad(c, half, degrees):
    th = np.deg2rad(degrees)
    return ci.quad(c, (half * np.cos(th), half * np.sin(th)))


@pytest.mark.parametrize("names,size", [(["inside", "rot45", "partly_out"], 32), (["shrink6", "corner", "shrink2"], 16),
                                        (["rot45", "corner", "inside"], 24)])
def test_quad_crop_is_pillows_crop_and_quad_transform(golden, names, size):
    """hip.quad_crop, F = 3 with a different window and different coefficients per frame in one launch.  A launch has one output
    size, so the six cases (sizes 32, 32, 32, 24, 16, 16) take three launches; each is filled up to three frames with other cases
    at that size.  Every frame equals live Pillow; every case at its own size also equals the reference's recorded crop.  The
    kernel does the Crop + Transform steps only, so a shrink case enters it as Pillow's Lanczos-resized frame, in the top-left
    corner of a frame padded with bytes its window never reaches."""
    from vface_amd import hip
    from vface_amd.scripts.intake import crop_plan
    frame = ci.frame()
    srcs, plans, refs = [], [], []
    for n in names:
        _, c, x, out_size, _ = next(k for k in ci.CASES if k[0] == n)
        quad = ci.quad(c, x)
        shrink, rsize, window, coeffs = crop_plan(quad, ci.FRAME_W, ci.FRAME_H, size)
        src = frame if shrink <= 1 else np.asarray(Image.fromarray(frame).resize(rsize, Image.LANCZOS))
        srcs.append(src)
        plans.append((window, coeffs))
        refs.append(pillow_crop_image(frame, quad, size))
        if out_size == size:
            assert np.array_equal(refs[-1], golden[f"{n}.crop"])
    # one [3, Hs, Ws, 3] batch: smaller (shrunk) frames sit in the top-left corner of a 0xA5-filled frame
    Hs, Ws = max(s.shape[0] for s in srcs), max(s.shape[1] for s in srcs)
    batch = np.full((3, Hs, Ws, 3), 0xA5, np.uint8)
    for f, s in enumerate(srcs):
        batch[f, :s.shape[0], :s.shape[1]] = s
    for (window, _), s in zip(plans, srcs):
        assert window[2] <= s.shape[1] and window[3] <= s.shape[0]
    # sentinel-padded output buffer
    pad = 4096
    buf = torch.full((pad + 3 * size * size * 3 + pad,), 0x5A, dtype=torch.uint8, device=DEV)
    out = buf[pad:pad + 3 * size * size * 3].view(3, size, size, 3)
    co = torch.from_numpy(np.stack([p[1] for p in plans])).to(DEV)
    win = torch.tensor([p[0] for p in plans], dtype=torch.int32)
    got = hip.quad_crop(torch.from_numpy(batch).to(DEV), co, win, size, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:pad] == 0x5A).all() and (host[-pad:] == 0x5A).all()
    for f in range(3):
        assert np.array_equal(got[f].cpu().numpy(), refs[f]), names[f]
    if size == 16:
        assert len({s.shape for s in srcs}) == 3          # three source sizes, so three unlike windows in one launch


def test_quad_crop_refusals_leave_the_output_untouched():
    from vface_amd import hip
    frames = torch.zeros(1, 20, 30, 3, dtype=torch.uint8, device=DEV)
    co = torch.zeros(1, 8, dtype=torch.float64, device=DEV)
    out = torch.full((1, 8, 8, 3), 7, dtype=torch.uint8, device=DEV)
    ok_win = torch.tensor([[0, 0, 30, 20]], dtype=torch.int32)
    for kw in (dict(frames=frames.cpu()), dict(quads=co.cpu()), dict(quads=co.float()),
               dict(windows=torch.tensor([[0, 0, 31, 20]], dtype=torch.int32)),
               dict(windows=torch.tensor([[5, 0, 5, 20]], dtype=torch.int32)),
               dict(windows=torch.tensor([[-1, 0, 5, 20]], dtype=torch.int32)), dict(out_size=0)):
        args = dict(frames=frames, quads=co, windows=ok_win, out_size=8, out=out)
        args.update(kw)
        with pytest.raises(hip.VFaceHipError):
            hip.quad_crop(**args)
    assert (out == 7).all()


def test_frame_intake_crop_is_the_references_crop_image(golden):
    """FrameIntake.crop against the fixture: the cases of one output size per call -- at 16 both shrink cases (two Lanczos sizes,
    so two groups) and, in the same call, a frame that is not shrunk at all."""
    from vface_amd.scripts.intake import FrameIntake
    frame = torch.from_numpy(ci.frame()).to(DEV)
    for size in (32, 24, 16):
        names = [k[0] for k in ci.CASES if k[3] == size]
        quads = [golden[f"{n}.quad"] for n in names]
        if size == 16:
            names.append(None)
            quads.append(ci.quad((60.0, 45.0), (9.0, 3.0)))
        got = FrameIntake(image_size=size, device=DEV).crop(frame[None].expand(len(names), -1, -1, -1).contiguous(), np.stack(quads))
        assert got.shape == (len(names), size, size, 3) and got.dtype == torch.uint8
        for f, n in enumerate(names):
            ref = golden[f"{n}.crop"] if n else pillow_crop_image(ci.frame(), quads[f], size)
            assert np.array_equal(got[f].cpu().numpy(), ref), (size, n)
    with pytest.raises(NotImplementedError):
        FrameIntake(image_size=32, device=DEV).crop(frame[None], golden["inside.quad"][None], enable_padding=True)


@pytest.mark.parametrize("S", [1024, 1536])
def test_quad_crop_at_the_real_frame_size(S):
    """2 frames of 1080 x 1920, quad rotated 7 degrees.  1024 is the reference's crop size: 2^20 pixels, one pass of the grid
    (the cap is 8192 blocks of 256 threads = 2^21 pixels).  S = 1536 (2.36 M pixels > 2^21) makes every thread of the first
    262144 take a second trip through the grid-stride loop."""
    from vface_amd.scripts.intake import FrameIntake
    assert (S * S > 8192 * 256) == (S == 1536)
    rng = np.random.default_rng(S)
    frames = rng.integers(0, 256, (2, 1080, 1920, 3), dtype=np.uint8)
    quads = np.stack([rotated_quad((960.0, 540.0), 300.0, 7.0), rotated_quad((1700.5, 400.25), 290.0, 7.0)])
    got = FrameIntake(image_size=S, device=DEV).crop(torch.from_numpy(frames).to(DEV), quads).cpu().numpy()
    for f in range(2):
        assert np.array_equal(got[f], pillow_crop_image(frames[f], quads[f], S))
    assert (got[1].reshape(-1, 3).max(1) == 0).mean() > 0.02          # the second quad leaves the frame on the right


@pytest.mark.parametrize("h,w,ow,oh", [(1024, 1024, 512, 512), (50, 70, 33, 91)])
def test_resize_u8_bicubic_is_pillows_default_resize(h, w, ow, oh):
    from vface_amd.scripts.intake import FrameIntake
    rng = np.random.default_rng(h + w)
    frames = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    frames[:, h // 4:h // 2] = 255                     # saturated bands: the negative lobes overshoot and the clip is used
    frames[:, h // 2:3 * h // 4] = 0
    got = FrameIntake(device=DEV).resize_u8(torch.from_numpy(frames).to(DEV), ow, oh).cpu().numpy()
    for f in range(2):
        assert np.array_equal(got[f], np.asarray(Image.fromarray(frames[f]).resize((ow, oh))))
    if h == 50:
        assert np.array_equal(got[0], model.resize_u8(frames[0], ow, oh, "bicubic"))


def _dataset_inputs():
    rng = np.random.default_rng(21)
    crop = rng.integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    label = rng.integers(0, 19, (2, 48, 64), dtype=np.uint8)
    label[1, 5, 7] = 255
    return crop, label


def _reference_dataset_tensors(crop: np.ndarray, label: np.ndarray):
    """video_swap_dataset.py:157-163, :214-221 with torch on the CPU (ToTensor = /255 of the uint8 image, CHW)."""
    t = (torch.from_numpy(crop).permute(2, 0, 1).float().div(255) - 0.5) / 0.5                # get_tensor() :214
    mask = np.isin(label, REMOVE)                                                             # :157
    conv = np.zeros_like(label)
    conv[mask] = 255                                                                          # :160-161
    m = 1 - torch.from_numpy(conv)[None].float().div(255)                                     # :219
    return t, t * m, m                                                                        # :221


def test_dataset_tensors_are_the_references_statements():
    from vface_amd import hip
    crop, label = _dataset_inputs()
    member = hip.label_membership(REMOVE, DEV)
    c, l = torch.from_numpy(crop).to(DEV), torch.from_numpy(label).to(DEV)
    for (oh, ow), exact in (((6, 8), True), ((7, 9), False)):
        image, inpaint, mask, mlat = (t.cpu() for t in hip.dataset_tensors(c, l, member, (oh, ow)))
        assert image.shape == (2, 3, 48, 64) and mask.shape == (2, 1, 48, 64) and mlat.shape == (2, 1, oh, ow)
        for f in range(2):
            t, ti, m = _reference_dataset_tensors(crop[f], label[f])
            assert torch.equal(image[f], t) and torch.equal(mask[f], m) and torch.equal(inpaint[f], ti)
            ref = torch.nn.functional.interpolate(m[None], size=(oh, ow), mode="bilinear", align_corners=False)[0]   # :459
            mo = model.dataset_tensors(crop[f], label[f], REMOVE, oh, ow)
            assert np.array_equal(mlat[f].numpy(), mo[3])             # the kernel's order, bit for bit
            assert np.array_equal(image[f].numpy(), mo[0]) and np.array_equal(inpaint[f].numpy(), mo[1])
            if exact:                                                 # factor 8: every weight is 0.5, sums of four {0, 1} / 4
                assert torch.equal(mlat[f], ref)
            else:
                assert (mlat[f] - ref).abs().max().item() <= 2e-6
        assert 0 < mask.mean() < 1 and mask[1, 0, 5, 7] == 1          # 255 is not on the list


def test_dataset_tensors_refusals_leave_the_outputs_untouched():
    from vface_amd import hip
    crop, label = _dataset_inputs()
    member = hip.label_membership(REMOVE, DEV)
    c, l = torch.from_numpy(crop).to(DEV), torch.from_numpy(label).to(DEV)
    outs = [torch.full(s, 3.0, device=DEV) for s in ((2, 3, 48, 64), (2, 3, 48, 64), (2, 1, 48, 64), (2, 1, 6, 8))]
    bad = [dict(crop=c.cpu()), dict(label=l.cpu()), dict(member=member.cpu()),
           dict(label=l[:, :40].contiguous()), dict(label=l[:, :, :32].contiguous()),        # a label map of another size
           dict(latent=(0, 8)), dict(latent=(6, -1)),
           dict(crop=c[:, :0].contiguous(), label=l[:, :0].contiguous()),                   # H = 0
           dict(crop=c[:, :, :0].contiguous(), label=l[:, :, :0].contiguous())]             # W = 0
    for kw in bad:
        args = dict(crop=c, label=l, member=member, latent=(6, 8))
        args.update(kw)
        with pytest.raises(hip.VFaceHipError):
            hip.dataset_tensors(out=tuple(outs), **args)
    with pytest.raises(hip.VFaceHipError):
        hip.label_membership([1, 256], DEV)
    assert all(bool((t == 3.0).all()) for t in outs)
    # ... and the C entry point itself refuses non-positive sizes before any launch
    lib = hip.load()
    p = [t.data_ptr() for t in (c, l, member, *outs)]
    for W, H, OW, OH, F_ in ((0, 48, 8, 6, 2), (64, -1, 8, 6, 2), (64, 48, 0, 6, 2), (64, 48, 8, 6, 0)):
        assert lib.vface_dataset_tensors(p[0], p[1], p[2], W, H, p[3], p[4], p[5], p[6], OW, OH, F_, None) < 0
    torch.cuda.synchronize()
    assert all(bool((t == 3.0).all()) for t in outs)


def _intake_case():
    rng = np.random.default_rng(33)
    F_, Hs, Ws = 3, 200, 260
    frames = rng.integers(0, 256, (F_, Hs, Ws, 3), dtype=np.uint8)
    quads = np.stack([rotated_quad((130.0, 100.0), 40.0, 5.0), rotated_quad((30.5, 90.25), 45.0, -12.0),
                      rotated_quad((130.0, 100.0), 130.0, 20.0)])         # inside; partly outside; large enough to be shrunk by 2
    labels = rng.integers(0, 19, (F_, 32, 32), dtype=np.uint8)
    return frames, quads, labels


def test_frame_intake_equals_the_references_host_sequence():
    """`FrameIntake.__call__` against crop_image + VideoDataset.__getitem_gray__ + :459 executed statement by statement with
    Pillow, numpy and torch on the host: F = 3 frames of 200 x 260, image_size 64, H = W = 32, latent 4 x 4."""
    from vface_amd.scripts.intake import FrameIntake, crop_plan, inv_transforms
    frames, quads, labels = _intake_case()
    S, H, W, lh, lw = 64, 32, 32, 4, 4
    assert [crop_plan(q, 260, 200, S)[0] > 1 for q in quads] == [False, False, True]
    fi = FrameIntake(image_size=S, H=H, W=W, latent=(lh, lw), device=DEV)
    image, inpaint, mask, mlat, inv = fi(torch.from_numpy(frames).to(DEV), quads, torch.from_numpy(labels).to(DEV), REMOVE)
    assert inv.shape == (3, 8) and np.array_equal(inv, inv_transforms(quads, S))
    for f in range(3):
        crop = Image.fromarray(pillow_crop_image(frames[f], quads[f], S))            # crop_faces_by_quads :259
        img_p = crop.convert("RGB").resize((W, H))                                   # video_swap_dataset.py:139
        t, ti, m = _reference_dataset_tensors(np.array(img_p), labels[f])
        assert torch.equal(image[f].cpu(), t) and torch.equal(inpaint[f].cpu(), ti) and torch.equal(mask[f].cpu(), m)
        ref = torch.nn.functional.interpolate(m[None], size=(lh, lw), mode="bilinear", align_corners=False)[0]   # :459
        assert torch.equal(mlat[f].cpu(), ref)                                       # factor 8: exact
    from vface_amd import hip
    with pytest.raises(hip.VFaceHipError):
        fi(torch.from_numpy(frames), quads, torch.from_numpy(labels).to(DEV), REMOVE)         # host frames


def test_intake_then_paste_back_closes_the_loop():
    """The intake's own crops pasted back through `PasteBack` with the intake's `inv_transforms` (no VAE round trip), against
    Pillow doing the same two transforms on the host: QUAD + BILINEAR out, resize + PERSPECTIVE + alpha composite back."""
    from vface_amd.scripts.intake import FrameIntake
    from vface_amd.scripts.paste_back import PasteBack
    rng = np.random.default_rng(44)
    F_, Sq, S, H = 2, 180, 64, 32
    frames = rng.integers(0, 256, (F_, Sq, Sq, 3), dtype=np.uint8)            # square frames: PasteBack.background's condition
    quads = np.stack([rotated_quad((90.0, 95.0), 35.0, 9.0), rotated_quad((150.0, 40.0), 38.0, -15.0)])
    labels = torch.zeros(F_, H, H, dtype=torch.uint8, device=DEV)
    fi = FrameIntake(image_size=S, H=H, W=H, latent=(4, 4), device=DEV)
    fr = torch.from_numpy(frames).to(DEV)
    image, _, _, _, inv = fi(fr, quads, labels, REMOVE)
    pb = PasteBack(H=H, W=H, canvas=S, device=DEV, encode_decode=None)
    got = pb.paste(image, fr, inv).cpu().numpy()
    assert np.array_equal(fr.cpu().numpy(), frames)                            # the originals are not written
    for f in range(F_):
        crop = Image.fromarray(pillow_crop_image(frames[f], quads[f], S)).resize((H, H))
        x = (torch.from_numpy(np.array(crop)).permute(2, 0, 1).float().div(255) - 0.5) / 0.5
        xs = torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0).permute(1, 2, 0).numpy()              # :597-598
        sw = Image.fromarray((255. * xs).astype(np.uint8)).resize((S, S), Image.BILINEAR).convert("RGBA")    # :606-608
        sw.putalpha(255)
        bg = Image.fromarray(frames[f]).convert("RGBA")
        bg.alpha_composite(sw.transform((Sq, Sq), Image.PERSPECTIVE, inv[f], Image.BILINEAR))     # :632-633
        ref = np.asarray(bg)[..., :3]
        assert np.array_equal(got[f], ref)
        changed = (got[f] != frames[f]).any(-1).mean()
        assert 0.05 < changed < 0.6                                            # something was pasted, and not everywhere


def small_cfg():
    return dict(image_size=32, in_channels=9, out_channels=4, model_channels=64,attention_resolutions=[4, 2, 1],
                num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True,
                transformer_depth=1, context_dim=768, legacy=False)


def test_cli_intake(tmp_path):
    """`--synthetic --with_vae --intake --paste_back` with the small UNet of tests/test_unet_gpu.py's CLI smoke test; and a run
    WITHOUT the flag equals, in `samples`, `run_synthetic` on options that do not know the flag at all (the namespace an older
    parser produces): its absence changes nothing."""
    import yaml
    from vface_amd.scripts import VFace_inference_batch as cli
    ypath = tmp_path / "small.yaml"
    ypath.write_text(yaml.safe_dump({"model": {"params": {"unet_config": {"params": small_cfg()}}}}))
    base = ["--synthetic", "--with_vae", "--frame_size", "320", "--config", str(ypath), "--n_frames", "2",
            "--n_samples", "2", "--H", "256", "--W", "256", "--max_steps", "1", "--ddim_steps", "50", "--skip_save"]
    res = cli.main(base + ["--intake", "--paste_back", "--Base_dir", str(tmp_path / "a")])
    b = res["batches"][0]
    assert b["finite"] and b["pixels"] == [2, 3, 256, 256] and b["pasted"] == [2, 320, 320, 3]
    assert b["stage_seconds"]["intake"] > 0 and "vae_encode" in b["stage_seconds"] and "paste_back" in b["stage_seconds"]
    # without the flag (and without the paste-back, which `samples` do not depend on)
    opt = cli.build_parser().parse_args(base + ["--Base_dir", str(tmp_path / "b")])
    opt.return_samples = True
    torch.manual_seed(opt.seed)
    with_attr = cli.run_synthetic(opt)
    assert "intake" not in with_attr["batches"][0]["stage_seconds"]
    assert opt.intake is False
    del opt.intake
    opt.Base_dir = str(tmp_path / "c")
    torch.manual_seed(opt.seed)
    without_attr = cli.run_synthetic(opt)
    assert torch.equal(with_attr["batches"][0]["samples"], without_attr["batches"][0]["samples"])
    with pytest.raises(SystemExit):
        cli.main(["--synthetic", "--intake", "--config", str(ypath), "--n_frames", "2", "--n_samples", "2", "--H", "256", "--W", "256",
                  "--max_steps", "1", "--Base_dir", str(tmp_path / "d")])
