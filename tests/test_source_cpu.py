"""Source intake without a GPU (csrc/intake.hip source_tensors_kernel, scripts/intake.py FrameIntake.source, scripts/source.py):
the numpy model of the kernel (tests/source_model.py, which the GPU must equal bit for bit) against the reference's statements for
the source image (REFace/scripts/VFace_inference_batch.py:324-355, :462, :468) restated with live Pillow and torch; the condition the
8-bit resize keeps; the ABI; the CLI's flag.

The 8-bit 224 x 224 resize of :343 is albumentations' ``A.Resize`` = ``cv2.INTER_LINEAR``.  OpenCV is not installed where these tests
run, so parity with ``cv2.resize`` is NOT pinned: ``q`` below is the model's own 11-bit fixed-point resize, held only to
"never a full 8-bit level from the exact bilinear value"."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import source_model as sm
from conftest import ROOT

PRESERVE = [1, 2, 3, 5, 6, 7, 9]        # project_ffhq.yaml:217-224 preserve_mask_src_FFHQ
SIZES = [((1024, 1024), (224, 224)), ((40, 40), (14, 14)), ((28, 28), (14, 14)), ((10, 10), (14, 14)), ((37, 53), (14, 28))]   # (h, w)


def _images(h, w, seed):
    rng = np.random.default_rng(seed)
    return {"random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "white": np.full((h, w, 3), 255, np.uint8),
            "binary": (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)}


@pytest.mark.parametrize("size_in,size_out", SIZES)
def test_fixed_point_resize_is_never_a_full_level_from_bilinear(size_in, size_out):
    (h, w), (oh, ow) = size_in, size_out
    worst = 0.0
    for name, img in _images(h, w, h * 1000 + w).items():
        q = sm.resize_linear_u8(img, ow, oh)                       # (asserts 0..255 before the cast)
        assert q.shape == (oh, ow, 3) and q.dtype == np.uint8
        err = np.abs(q.astype(np.float64) - sm.bilinear_f64(img, ow, oh)).max()
        worst = max(worst, err)
        assert err < 1.0, (name, err)
        if name == "white":
            assert (q == 255).all()
    for v in (0, 1, 137, 254, 255):                                # a constant image stays constant
        assert (sm.resize_linear_u8(np.full((h, w, 3), v, np.uint8), ow, oh) == v).all(), v
    print(f"{h}x{w} -> {oh}x{ow}: worst |q - bilinear64| = {worst:.4f}")


def test_fraction_one_half_and_edge_clamps():
    taps, weights = sm.linear_taps(28, 14)                         # every centre falls between two samples
    assert (weights == 1024).all() and np.array_equal(taps[:, 0], np.arange(14) * 2) and np.array_equal(taps[:, 1], np.arange(14) * 2 + 1)
    taps, weights = sm.linear_taps(10, 14)                         # upscale: the first centre is left of sample 0, the last right of 9
    assert tuple(taps[0]) == (0, 1) and tuple(weights[0]) == (2048, 0)
    assert tuple(taps[-1]) == (9, 9) and tuple(weights[-1]) == (2048, 0)
    assert taps.min() >= 0 and taps.max() <= 9


@pytest.mark.parametrize("n_in,n_out", [(1024, 224), (40, 14), (28, 14), (10, 14), (37, 14), (53, 28), (16, 28), (300, 224), (1, 3), (5, 1)])
def test_host_tables_are_the_models(n_in, n_out):
    from vface_amd.scripts.resample import linear_taps_u8
    taps, weights = linear_taps_u8(n_in, n_out)
    mt, mw = sm.linear_taps(n_in, n_out)
    assert taps.dtype == np.int32 and weights.dtype == np.int16 and taps.shape == weights.shape == (n_out, 2)
    assert np.array_equal(taps, mt) and np.array_equal(weights, mw)
    assert (weights.astype(np.int64).sum(1) == 2048).all() and weights.min() >= 0
    assert taps.min() >= 0 and taps.max() <= n_in - 1
    with pytest.raises(ValueError):
        linear_taps_u8(0, 4)


def _case(S, H, W, seed):
    rng = np.random.default_rng(seed)
    crop = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    label = rng.integers(0, 12, (H, W), dtype=np.uint8)
    label[rng.random((H, W)) < 0.1] = rng.integers(12, 256, 1, dtype=np.uint8)[0]       # values outside the parser's range
    label[0, 0], label[-1, -1] = 255, 9
    return crop, label


def reference_source_tensors(crop: np.ndarray, label: np.ndarray, H: int, W: int, oh: int, ow: int, oc: int, q: np.ndarray):
    """VFace_inference_batch.py:324-355, :462, :468 with live Pillow / torch.  ``ToTensor`` = ``.float().div(255)``; the tensor
    ``Resize`` = ``F.interpolate(bilinear, align_corners=False, antialias=False)``; ``q`` stands for ``A.Resize(oc, oc)`` of the crop
    (:343, OpenCV: not available, see the module docstring)."""
    interp = lambda t, size: F.interpolate(t[None], size=size, mode="bilinear", align_corners=False, antialias=False)[0]
    ref_mask = np.isin(label, PRESERVE)                                                       # :332
    conv = np.zeros_like(label)
    conv[ref_mask] = 255                                                                      # :335-336
    reference_mask_tensor = torch.from_numpy(conv)[None].float().div(255)                     # :341
    mask_ref = interp(reference_mask_tensor, (oc, oc))                                        # :342
    mean, std = torch.tensor(sm.CLIP_MEAN).view(3, 1, 1), torch.tensor(sm.CLIP_STD).view(3, 1, 1)
    ref_img = torch.from_numpy(q).permute(2, 0, 1).float().div(255).sub(mean).div(std)        # :345 get_tensor_clip() (:96-104)
    ref_img = ref_img * mask_ref                                                              # :346
    img = Image.fromarray(crop).convert("RGB").resize((W, H), Image.BILINEAR)                 # :350
    ref_img_inv_ori = (torch.from_numpy(np.array(img)).permute(2, 0, 1).float().div(255) - 0.5) / 0.5     # :351 get_tensor()
    ref_img_inv_ori = ref_img_inv_ori * reference_mask_tensor                                 # :352
    inpaint = ref_img_inv_ori.clone() * (1 - reference_mask_tensor)                           # :354-355
    inpaint_mask_src = interp(1 - reference_mask_tensor, (oh, ow))                            # :462, :468
    return dict(mask=reference_mask_tensor, masked=ref_img_inv_ori, inpaint=inpaint, mask_latent=inpaint_mask_src, clip_image=ref_img,
                mask_ref=mask_ref, img=np.array(img))


# (S, (H, W), OC, (OH, OW)): the GPU test's small cases and an integer-factor one, where the mask resizes are exact
CASES = [(40, (24, 20), 14, (3, 5)), (28, (16, 16), 14, (2, 2)), (10, (12, 12), 14, (4, 4)), (37, (21, 33), 28, (7, 11)),
         (64, (56, 56), 28, (7, 7))]


@pytest.mark.parametrize("S,hw,oc,lat", CASES)
def test_model_against_the_references_statements(S, hw, oc, lat):
    (H, W), (oh, ow) = hw, lat
    crop, label = _case(S, H, W, S + oc)
    q = sm.resize_linear_u8(crop, oc, oc)
    ref = reference_source_tensors(crop, label, H, W, oh, ow, oc, q)
    mask, masked, inpaint, mlat, clip_image, q2 = sm.source_tensors(crop, ref["img"], label, PRESERVE, oh, ow, oc)
    t = torch.from_numpy
    assert np.array_equal(q, q2)
    assert torch.equal(t(mask), ref["mask"]) and torch.equal(t(masked), ref["masked"]) and torch.equal(t(inpaint), ref["inpaint"])
    assert not inpaint.any() and 0 < mask.mean() < 1                  # x m (1 - m): zero, as the reference computes it
    assert mask[0, 0, 0] == 0 and mask[0, -1, -1] == 1                # 255 is not on the list, 9 is
    d_lat = (t(mlat) - ref["mask_latent"]).abs().max().item()
    d_ref = (t(sm.resize_map_f32(mask[0], oc, oc)) - ref["mask_ref"][0]).abs().max().item()
    d_clip = (t(clip_image) - ref["clip_image"]).abs().max().item()
    print(f"S {S} {H}x{W} oc {oc} latent {oh}x{ow}: mask_latent {d_lat:.3e} mask_ref {d_ref:.3e} clip_image {d_clip:.3e}")
    assert d_lat <= 2e-6 and d_ref <= 2e-6
    assert d_clip <= 5e-6               # 2e-6 x the largest CLIP-normalised magnitude (2.146) + one rounding of the product
    if S == 64:                         # factor 8 and factor 2: every weight is 0.5
        assert d_lat == 0.0 and d_ref == 0.0


def test_abi_symbol_null_refusal_and_version():
    lib_path = os.path.join(ROOT, "vface_amd", "lib", "libvface_hip.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as ge
        ge.build()
    from vface_amd import hip
    assert hasattr(ctypes.CDLL(lib_path), "vface_source_tensors")
    lib = hip.load()
    assert lib.vface_abi_version() == 8
    restype, argtypes = hip.SIGNATURES["vface_source_tensors"]
    assert restype is ctypes.c_int and len(argtypes) == 22
    assert lib.vface_source_tensors(*[None if a is ctypes.c_void_p else 0 for a in argtypes]) == -1       # VFACE_ERR_ARG, nothing launched
    with pytest.raises(hip.VFaceHipError):          # host tensors: no CPU fallback
        z = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
        tp, tw = torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int16)
        hip.source_tensors(z, z, torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(256, dtype=torch.uint8), (tp, tw, tp, tw), (2, 2), 4)


def test_frame_intake_source_refuses_host_tensors_and_missing_labels():
    from vface_amd import hip
    from vface_amd.scripts.intake import FrameIntake, SourceTensors
    from vface_amd.scripts.VFace_inference_batch import PRESERVE_MASK_SRC_FFHQ
    assert list(PRESERVE_MASK_SRC_FFHQ) == PRESERVE
    assert SourceTensors._fields == ("crop", "labels", "clip_image", "mask", "masked", "inpaint_image", "inpaint_mask_latent")
    fi = FrameIntake(image_size=32, H=16, W=16, latent=(2, 2), device="cuda:0")
    frames, quads = torch.zeros(1, 80, 96, 3, dtype=torch.uint8), np.array([[[20., 20.], [20., 60.], [60., 60.], [60., 20.]]])
    with pytest.raises(ValueError, match="labels_u8.*parser"):
        fi.source(frames, quads)
    with pytest.raises(hip.VFaceHipError, match="GPU"):
        fi.source(frames, quads, labels_u8=torch.zeros(1, 16, 16, dtype=torch.uint8))


class _Reached(Exception):
    pass


class _FirstGpuCall(Exception):
    pass


def test_cli_flag(tmp_path, monkeypatch):
    from vface_amd.ldm.models import autoencoder
    from vface_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from vface_amd.scripts import VFace_inference_batch as cli
    from vface_amd.scripts import intake
    base = ["--synthetic", "--with_vae", "--n_frames", "2", "--n_samples", "2", "--max_steps", "1", "--Base_dir", str(tmp_path)]
    with pytest.raises(SystemExit, match="--source_intake.*--intake"):
        cli.main(base + ["--source_intake"])
    with pytest.raises(SystemExit, match="--intake"):
        cli.run_synthetic(cli.build_parser().parse_args(base + ["--source_intake"]))
    assert cli.build_parser().parse_args(base).source_intake is False
    assert cli.build_parser().parse_args(base + ["--intake", "--source_intake"]).source_intake is True

    # flag off: FrameIntake.source is never reached -- run_synthetic up to its first GPU call (the model's move to the device)
    def source(*a, **k):
        raise _Reached()

    def to(self, *a, **k):
        raise _FirstGpuCall()
    small_unet = dict(image_size=8, in_channels=9, out_channels=4, model_channels=32, attention_resolutions=[4, 2, 1], num_res_blocks=1,
                      channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1, context_dim=768,
                      use_checkpoint=True, legacy=False)
    small_vae = dict(embed_dim=4, ddconfig=dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32,
                                                ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0))
    monkeypatch.setattr(intake.FrameIntake, "source", source)
    monkeypatch.setattr(LatentDiffusion, "to", to)
    monkeypatch.setattr(cli, "load_unet_config", lambda path: dict(small_unet))
    monkeypatch.setattr(autoencoder, "FFHQ_VAE_CONFIG", small_vae)
    with pytest.raises(_FirstGpuCall):
        cli.run_synthetic(cli.build_parser().parse_args(base + ["--intake"]))
