"""What the identity network's GPU tests rest on, without a GPU.

1. The per-element bounds of arcface_bounds.py admit torch's own fp32 evaluation of each kernel and refuse one-line defects of it;
   for ``vface_id_prep``: moving ANY bin edge of either pool by one, up or down, moves some output beyond the bound.
2. tests/arcface_model.py -- the emulation whose error, times 1.25, is test_arcface_gpu.py's tolerance -- against the reference's
   recorded outputs (tests/golden/arcface.npz):
   * A CONDITION, NOT A MEASUREMENT: in fp16 and in bf16 its error may not exceed the error of the reference's own ``.half()`` /
     ``.bfloat16()`` run (``e_ref16`` / ``e_ref_bf16``, read from the fixture), for the network (rel-L2) and for every unit case
     (max abs);
   * each seeded one-line defect lands past the whole-network tolerance (1.25 x the clean emulation's rel-L2), and its unit-level
     counterpart past the unit tolerance (the same, on the unit's output).
   The pooling defect at this level is the upper bin edge taken as a floor instead of a ceiling (one short wherever the division is
   inexact): ONE moved edge of 112 changes the features by less than bf16's tolerance, so that form is held at the kernel's level (1)."""
import pytest
import torch
import torch.nn.functional as F

import arcface_bounds as ab
import arcface_model as am
from arcface_model import ca
from conftest import load_golden
from kernel_bounds import assert_within, rnd

DTS = [torch.float16, torch.bfloat16]
E_REF = {torch.float16: "e_ref16", torch.bfloat16: "e_ref_bf16"}


def _outside(got, ref, bound):
    return int(((got.double() - ref).abs() > bound).sum())


# ------------------------------------------------------------------------------------------------ 1: the per-element bounds
@pytest.mark.parametrize("dt", DTS)
def test_prelu_bound_admits_fp32_and_refuses_defects(dt):
    M, C_ = 48, 72
    x = rnd((M, C_), 1, dt, 2.0)
    slope = torch.cat([torch.linspace(-0.5, 0.5, C_ - 2), torch.tensor([0.0, 1.0])])
    za, zb = rnd((C_,), 2, torch.float32) + 1.5, rnd((C_,), 3, torch.float32)
    y, by, z, bz = ab.prelu_ref_and_bound(x, slope, dt, za, zb)
    f = x.float()
    y32 = torch.where(f > 0, f, slope * f)
    assert_within(y32.to(dt), y, by, "prelu")
    assert_within((za * y32 + zb).to(dt), z, bz, "prelu z")
    n = int((x.double() < 0).sum())
    assert _outside(F.relu(f).to(dt), y, by) > 0.9 * n, "ReLU instead of PReLU"
    assert _outside(torch.where(f > 0, f, slope.flip(0) * f).to(dt), y, by) > 0.5 * n, "another channel's slope"
    assert _outside((za * y32.to(dt).float() + zb).to(dt), z, bz) > 0.02 * n, "z from the rounded y"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H,W,s", [(6, 4, 2), (7, 5, 2), (7, 5, 1)])
def test_se_gate_add_bound_admits_fp32_and_refuses_defects(dt, H, W, s):
    nimg, C_ = 3, 16
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    M = nimg * OH * OW
    res, xin = rnd((M, C_), 4, dt), rnd((nimg * H * W, C_), 5, dt)
    g = torch.sigmoid(rnd((nimg, C_), 6, torch.float32))
    za, zb = rnd((C_,), 7, torch.float32) + 1.5, rnd((C_,), 8, torch.float32)
    sc = ab.strided_rows(xin, nimg, H, W, s)
    assert sc.shape[0] == M
    y, by, z, bz = ab.se_gate_add_ref_and_bound(res, g, sc, dt, nimg=nimg, za=za, zb=zb)
    y32 = torch.addcmul(sc.float(), res.float(), g.repeat_interleave(OH * OW, 0))
    assert_within(y32.to(dt), y, by, "se_gate_add")
    assert_within((za * y32 + zb).to(dt), z, bz, "se_gate_add z")
    assert _outside((res.float() + sc.float()).to(dt), y, by) > 0.8 * y.numel(), "gate omitted"
    assert _outside((res.float() * g.flip(0).repeat_interleave(OH * OW, 0) + sc.float()).to(dt), y, by) > 0.5 * y.numel(), "another image's gate"
    assert _outside((za * y32.to(dt).float() + zb).to(dt), z, bz) > 0.02 * y.numel(), "z from the rounded y"
    if s == 2:
        unstrided = xin.reshape(nimg, H, W, C_)[:, :OH, :OW].reshape(M, C_)
        assert _outside(torch.addcmul(unstrided.float(), res.float(), g.repeat_interleave(OH * OW, 0)).to(dt), y, by) > 0.8 * (M - nimg) * C_, \
            "shortcut read unstrided"
        flat = xin[:M]
        assert _outside(torch.addcmul(flat.float(), res.float(), g.repeat_interleave(OH * OW, 0)).to(dt), y, by) > 0.8 * (M - 1) * C_, \
            "shortcut read at the output's row"


def test_l2norm_bound_admits_fp32_and_refuses_defects():
    x = torch.cat([rnd((3, 512), 9, torch.float32), rnd((1, 512), 10, torch.float32) * 1e-25, rnd((1, 512), 11, torch.float32) * 1e25])
    ref, bound = ab.l2norm_ref_and_bound(x)
    mx = x.abs().amax(1, keepdim=True)
    scaled = x / (mx * torch.sqrt(((x / mx) ** 2).sum(1, keepdim=True)))
    assert_within(scaled, ref, bound, "l2norm, scaled sum")
    assert_within(x[:3] / x[:3].norm(dim=1, keepdim=True), ref[:3], bound[:3], "torch.norm on ordinary rows")
    naive = x / torch.sqrt((x * x).sum(1, keepdim=True))
    assert not bool(torch.isfinite(naive[3]).all()) and _outside(naive[4], ref[4], bound[4]) == 512, "squares summed unscaled"
    assert _outside(x[:3], ref[:3], bound[:3]) > 0.99 * 3 * 512, "no normalisation"
    assert _outside(x[:3] / (x[:3] * x[:3]).sum(1, keepdim=True), ref[:3], bound[:3]) > 0.99 * 3 * 512, "divided by the squared norm"


def _torch_fp32_chain(img, clip_img):
    x = img.float()
    if clip_img:
        x = (x * ab.CLIP_STD.float().view(1, 3, 1, 1) + ab.CLIP_MEAN.float().view(1, 3, 1, 1) - 0.5) / 0.5
    if x.shape[2] != 256:
        x = F.adaptive_avg_pool2d(x, (256, 256))
    return F.adaptive_avg_pool2d(x[:, :, 35:223, 32:220], (112, 112))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S,clip_img", [(224, True), (256, True), (224, False), (256, False)])
def test_id_prep_bound_admits_aten_and_refuses_defects(dt, S, clip_img):
    img = torch.randn(1, 3, S, S, generator=torch.Generator().manual_seed(S))
    ref, bound = ab.id_prep_ref_and_bound(img, dt, clip_img=clip_img)
    assert float((ref - am.prep_twin(img.double(), clip_img)).abs().max()) < 1e-13      # the twin's bins are the reference's
    assert_within(_torch_fp32_chain(img, clip_img).to(dt), ref, bound, "ATen's fp32 chain")
    n = ref.numel()
    assert _outside(_torch_fp32_chain(img, not clip_img).to(dt), ref, bound) > 0.9 * n, "clip_img the other way"
    if S != 256:
        assert _outside(_torch_fp32_chain(F.interpolate(img, (256, 256), mode="bilinear"), clip_img).to(dt), ref, bound) > 0.5 * n, "a resize"
        src = img if not clip_img else (img * ab.CLIP_STD.float().view(1, 3, 1, 1) + ab.CLIP_MEAN.float().view(1, 3, 1, 1) - 0.5) / 0.5
        flat = F.adaptive_avg_pool2d(src[:, :, 35 * S // 256:-(-223 * S // 256), 32 * S // 256:-(-220 * S // 256)], (112, 112))
        assert flat.shape == ref.shape and _outside(flat.to(dt), ref, bound) > 0.5 * n, "one flattened pool instead of the nested means"


@pytest.mark.parametrize("S", [224, 256])
def test_any_bin_edge_moved_by_one_is_seen(S):
    """On noise, every edge of every bin that reaches the output, moved one row up or down (the columns' tables are the same
    function), leaves some output beyond the bf16 bound -- the wider of the two."""
    img = torch.randn(1, 3, S, S, generator=torch.Generator().manual_seed(7 + S), dtype=torch.float64)
    ref, bound = ab.id_prep_ref_and_bound(img, torch.bfloat16, clip_img=False)
    checked = 0
    pools = [("shift2", 188, 112, range(112))]
    if S != 256:
        pools.append(("shift1", S, 256, range(35, 223)))
    for kw, n_in, n_out, idx in pools:
        table = am.bins(n_in, n_out)
        for i in idx:
            for end in (0, 1):
                for d in (-1, 1):
                    lo, hi = table[i]
                    lo, hi = (lo + d, hi) if end == 0 else (lo, hi + d)
                    if lo < 0 or hi > n_in or lo >= hi:
                        continue                                    # no such bin
                    got = am.prep_twin(img, clip_img=False, **{kw: (i, end, d)})
                    assert _outside(got, ref, bound) > 0, (kw, i, end, d)
                    checked += 1
    assert checked > (400 if S == 256 else 1100)


# ------------------------------------------------------------------------------------------------ 2: the emulation
@pytest.mark.parametrize("dt", DTS)
def test_emulation_is_no_worse_than_the_references_own_16bit_run(dt):
    g = load_golden("arcface")
    e = am.rel_l2(am.emulated(dt), g["feat64"])
    print(f"network {dt}: emulation rel-L2 {e:.3e}, the reference's own {float(g[E_REF[dt]]):.3e}")
    assert e <= float(g[E_REF[dt]])
    for name in ca.UNIT_CASES:
        sd, x, (cin, depth, stride, H, W, n) = am.unit_case(name)
        err = float((am.run_unit(sd, "u", x, cin, depth, stride, dt) - g[f"{name}.out64"]).abs().max())
        print(f"{name} {dt}: emulation max abs {err:.3e}, the reference's own {float(g[f'{name}.{E_REF[dt]}']):.3e}")
        assert err <= 1.02 * float(g[f"{name}.{E_REF[dt]}"]), name


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("defect", am.DEFECTS)
def test_every_seeded_defect_lands_beyond_the_network_tolerance(dt, defect):
    g = load_golden("arcface")
    tol = am.MARGIN * am.rel_l2(am.emulated(dt), g["feat64"])
    e = am.rel_l2(am.emulated(dt, defect), g["feat64"])
    print(f"{defect} {dt}: rel-L2 {e:.3e} = {e / tol:.1f} x the tolerance {tol:.3e}")
    assert e > tol


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name,defect", [(n, d) for n in ca.UNIT_CASES for d in am.UNIT_DEFECTS
                                         if d != "shortcut_unstrided" or n in ("id_s2", "id_s2_odd")])
def test_unit_level_defects_land_beyond_the_unit_tolerance(dt, name, defect):
    g = load_golden("arcface")
    sd, x, (cin, depth, stride, H, W, n) = am.unit_case(name)
    ref = g[f"{name}.out64"]
    tol = am.MARGIN * am.rel_l2(am.run_unit(sd, "u", x, cin, depth, stride, dt), ref)
    e = am.rel_l2(am.run_unit(sd, "u", x, cin, depth, stride, dt, defect), ref)
    assert e > tol, (e, tol)
