"""Host side of the frame intake (vface_amd/scripts/intake.py, resample.py) and the CPU model of its kernels
(tests/intake_model.py), without a GPU: against live Pillow and against tests/golden/intake.npz, the reference's own outputs
(`crop_image`, `calc_alignment_coefficients`, `compute_transform` of REFace/src/utils/alignmengt.py, recorded by
tests/golden/make_intake_golden.py).  Everything here is bit for bit."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import cases_intake as ci  # noqa: E402
import intake_model as model  # noqa: E402

PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "intake.npz"), allow_pickle=False)


def banded_image(h=90, w=120, seed=3):
    """Noise with saturated 255 and 0 bands beside it, so that a filter with negative lobes overshoots at both ends."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[10:30, :] = 255
    img[30:50, :] = 0
    img[:, 20:45] = 255
    img[:, 45:70] = 0
    return img


def unclipped_sums(img, axis, bounds, kk):
    """What one pass accumulates before the clip (min and max over the image)."""
    a = np.moveaxis(img.astype(np.int64), 1 if axis == 0 else 0, 0)
    lo, hi = 0, 0
    for o in range(bounds.shape[0]):
        x0, n = int(bounds[o, 0]), int(bounds[o, 1])
        ss = (1 << 21) + np.tensordot(kk[o, :n].astype(np.int64), a[x0:x0 + n], axes=(0, 0))
        lo, hi = min(lo, int((ss >> 22).min())), max(hi, int((ss >> 22).max()))
    return lo, hi


@pytest.mark.parametrize("filter", ["bicubic", "lanczos"])
@pytest.mark.parametrize("ow,oh", [(60, 45), (17, 90), (120, 31), (64, 64)])
def test_bicubic_and_lanczos_tables_reproduce_pillows_resize(filter, ow, oh):
    from vface_amd.scripts.resample import resample_coeffs
    img = banded_image()
    ref = np.asarray(Image.fromarray(img).resize((ow, oh), PIL_FILTER[filter]))
    assert np.array_equal(model.resize_u8(img, ow, oh, filter), ref)
    # condition: the negative lobes are exercised -- some sample leaves 0..255 at each end before the clip
    h, w, _ = img.shape
    lo, hi = 0, 0
    cur = img
    for axis, (n_in, n_out) in enumerate([(w, ow), (h, oh)]):
        if n_in == n_out:
            continue
        b, k = resample_coeffs(n_in, n_out, filter)
        assert (k < 0).any()
        l, u = unclipped_sums(cur, axis, b, k)
        lo, hi = min(lo, l), max(hi, u)
        cur = model.resample_u8(cur, axis, b, k)
    assert lo < 0 and hi > 255, (lo, hi)


def test_pillows_default_rgb_resize_is_bicubic():
    img = banded_image()
    assert np.array_equal(np.asarray(Image.fromarray(img).resize((64, 64))), model.resize_u8(img, 64, 64, "bicubic"))


def _bilinear_tables_before_the_filter_argument(in_size, out_size):
    """resample_coeffs as it stood when it knew only the triangle filter (scripts/paste_back.py), kept here verbatim as the pin."""
    import math
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, ksize), np.float64)
    total = np.zeros(out_size, np.float64)
    for x in range(ksize):
        a = np.abs((x + xmin - center + 0.5) * inv)
        col = np.where((x < xmax) & (a < 1.0), 1.0 - a, 0.0)
        w[:, x] = col
        total = total + col
    nz = total != 0.0
    w[nz] = w[nz] / total[nz, None]
    w[np.arange(ksize)[None, :] >= xmax[:, None]] = 0.0
    fixed = w * float(1 << 22)
    kk = np.where(w < 0, np.trunc(-0.5 + fixed), np.trunc(0.5 + fixed)).astype(np.int32)
    return np.stack([xmin, xmax], 1).astype(np.int32), kk


@pytest.mark.parametrize("n_in,n_out", [(512, 1024), (1024, 512), (50, 33), (70, 91), (37, 100), (41, 17), (1080, 1024), (64, 64)])
def test_bilinear_tables_are_unchanged(n_in, n_out):
    from vface_amd.scripts import paste_back, resample
    assert paste_back.resample_coeffs is resample.resample_coeffs
    old = _bilinear_tables_before_the_filter_argument(n_in, n_out)
    for new in (resample.resample_coeffs(n_in, n_out), resample.resample_coeffs(n_in, n_out, "bilinear")):
        assert new[0].dtype == old[0].dtype and new[1].dtype == old[1].dtype
        assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1])
    with pytest.raises(ValueError):
        resample.resample_coeffs(n_in, n_out, "box")


def test_quad_from_landmarks_is_compute_transform(golden):
    from vface_amd.scripts.intake import quad_from_landmarks
    for seed, integer in ci.LANDMARK_SETS:
        lm = golden[f"lm{seed}.lm"]
        assert np.array_equal(lm, ci.landmarks(seed, integer)) and (lm.dtype.kind == "i") == integer
        c, x, y = golden[f"lm{seed}.c"], golden[f"lm{seed}.x"], golden[f"lm{seed}.y"]
        ref = np.stack([c - x - y, c - x + y, c + x + y, c + x - y])               # alignmengt.py:211
        got = quad_from_landmarks(lm)
        assert got.dtype == np.float64 and np.array_equal(got, ref)
    with pytest.raises(ValueError):
        quad_from_landmarks(np.zeros((5, 2)))


def test_inv_transforms_is_calc_alignment_coefficients(golden):
    from vface_amd.scripts.intake import inv_transforms
    for size in (32, 24, 16):
        names = [n for n, _, _, s, _ in ci.CASES if s == size]
        got = inv_transforms(np.stack([golden[f"{n}.quad"] for n in names]), size)
        assert got.shape == (len(names), 8) and got.dtype == np.float64
        for i, n in enumerate(names):
            assert np.array_equal(got[i], golden[f"{n}.inv"]), n


@pytest.mark.parametrize("name,c,x,size,out", ci.CASES, ids=[c[0] for c in ci.CASES])
def test_crop_model_is_crop_image(golden, name, c, x, size, out):
    """The CPU model of FrameIntake.crop (host scalars + Lanczos shrink + quad_crop in the kernel's order) against the reference's
    recorded `crop_image` output and against live Pillow running crop_image's statements (alignmengt.py:100-123, :142)."""
    from vface_amd.scripts.intake import crop_plan
    frame = ci.frame()
    assert np.array_equal(frame, golden["frame"])
    quad = ci.quad(c, x)
    assert np.array_equal(quad, golden[f"{name}.quad"])
    got, inside = model.crop(frame, quad, size)
    assert got.shape == (size, size, 3)
    assert np.array_equal(got, golden[f"{name}.crop"])
    # live Pillow: resize (if the face is large), crop, transform(QUAD, BILINEAR)
    shrink, rsize, window, _ = crop_plan(quad, ci.FRAME_W, ci.FRAME_H, size)
    img, q = Image.fromarray(frame), quad.copy()
    assert (shrink > 1) == name.startswith("shrink") and (shrink <= 1 or shrink == int(name[6:]))
    if shrink > 1:
        img = img.resize(rsize, Image.LANCZOS)
        q /= shrink
    img = img.crop(window)
    q -= window[0:2]
    live = np.asarray(img.transform((size, size), Image.QUAD, (q + 0.5).flatten(), Image.BILINEAR))
    assert np.array_equal(got, live)
    # conditions: an "out" case fills 5 % .. 60 % of its pixels with zeros (neither the fill nor the fetch path is vacuous),
    # the others fetch everywhere
    filled = 1.0 - inside.mean()
    if out:
        assert 0.05 <= filled <= 0.60, filled
        assert (got[~inside] == 0).all()
    else:
        assert filled == 0.0


def test_crop_plan_refuses_padding_and_quads_off_the_frame():
    from vface_amd.scripts.intake import crop_plan
    with pytest.raises(NotImplementedError):
        crop_plan(ci.quad((60, 45), (12, 12)), 120, 90, 32, enable_padding=True)
    with pytest.raises(ValueError):
        crop_plan(ci.quad((500, 500), (12, 12)), 120, 90, 32)


def test_dataset_tensor_model_is_the_references_statements():
    """intake_model.dataset_tensors against video_swap_dataset.py:157-163, :214-221 and VFace_inference_batch.py:459 run with
    torch: the three full-size tensors equal, the resized mask within the 2e-6 that separates ATen's CPU interpolate from the
    kernel's order (tests/test_paste_gpu.py allows the same arithmetic the same)."""
    import torch
    rng = np.random.default_rng(9)
    crop = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    label = rng.integers(0, 19, (48, 64), dtype=np.uint8)
    remove = [1, 2, 3, 5, 6, 7, 9]
    for oh, ow in ((6, 8), (7, 9)):
        image, inpaint, mask, mlat = model.dataset_tensors(crop, label, remove, oh, ow)
        t = (torch.from_numpy(crop).permute(2, 0, 1).float().div(255) - 0.5) / 0.5
        conv = np.zeros_like(label)
        conv[np.isin(label, remove)] = 255
        m = 1 - torch.from_numpy(conv)[None].float().div(255)
        assert torch.equal(torch.from_numpy(image.copy()), t) and torch.equal(torch.from_numpy(mask), m)
        assert torch.equal(torch.from_numpy(inpaint), t * m)
        ref = torch.nn.functional.interpolate(m[None], size=(oh, ow), mode="bilinear", align_corners=False)[0]
        assert (torch.from_numpy(mlat) - ref).abs().max().item() <= 2e-6
