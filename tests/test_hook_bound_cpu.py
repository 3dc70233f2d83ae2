"""The bounds of the hook and sampler kernels on their own, no GPU: ``kernel_bounds.flow_warp_ref_and_bound`` must admit the CPU model
of the warp's rounding points (``hook_model.flow_warp_model``, both division forms) on EVERY element and must refuse each seeded
one-line defect on the shapes and flow families where it is reasoned to show; the flow resample's, the DDIM step's and the timestep
embedding's bounds must admit the oracle's fp32 restatement of each.  That is what shows that test_hook_sampler_kernels_gpu.py can
fail.  The only threshold is 1 (error / bound).  Which defect shows where, reasoned and not fitted:

* xy_swapped -- the row pitch of the source taken as h: another pixel altogether wherever h != w and both exceed 1 -- except
  on outside_up, where iy = 0 puts every tap that carries weight into row 0, which the pitch does not enter.
* neighbour_unclamped -- x1 = x0 + 1, y1 = y0 + 1 without the min: the weight is zero by arithmetic, so the value only changes
  where the tap is not finite -- the element right behind the frame, which the tests poison.  Tap (y1, x1) of a pixel of the last
  row is element h w of the frame whenever ix = w - 1 (outside_right, on_edge), any tap of row y1 = h whenever iy = h - 1
  (outside_down, on_edge).
* ax_unrounded -- alpha x kept in fp32: up to half a unit of ax more in front of the one rounding the bound grants; shows where
  alpha is neither 0 nor 1 and the map has a few thousand elements (smooth family, alpha = 0.8).
* frame_f -- warped from frame f instead of f - 1: frames carry their own scale and offset, so everywhere while alpha != 1.
* ld_prev_as_ld_src -- the halo read with the source's leading dimension: frame 0, given a halo with ld_prev != ld_src.
* recip_for_true -- the reciprocal form where the true division is asked for: the VALUES stay inside the bound (the two forms
  differ by one rounding of the coordinate, which the bound grants), the INDICES do not: on integer flows the coordinate sits on
  the floor() boundary and x0 / y0 differ from ``oracle.flow.gather_indices`` wherever the product with the rounded reciprocal
  comes out an ulp below the integer (maps of 32 cells and more have such columns)."""
import pytest
import torch

from hook_model import DEFECTS, FAMILIES, flow_warp_model, lay_frames, make_flow, make_frames
from kernel_bounds import (U32, ddim_step_ref_and_bound, flow_to_latent_ref_and_bound, flow_warp_ref_and_bound,
                           timestep_embedding_ref_and_bound)
from oracle import ddim as oddim
from oracle import flow as oflow
from oracle import unet as ounet

DTS = [torch.float16, torch.bfloat16]
SHAPES = [(12, 20), (20, 12), (5, 7), (1, 9), (9, 1), (16, 16)]
ALPHA = 0.8


def _setup(dt, h, w, family, C=8, F_=3, alpha=ALPHA):
    x = make_frames(F_ + 1, h * w, C, dt, seed=h + 3 * w)                  # frame 0 of the draw is the halo
    fl = make_flow(family, F_, h, w, seed=5)
    src = lay_frames(x[1:], C + 8, 2, 8)
    prev = lay_frames(x[:1], C + 16, 1, 8)
    kw = dict(F=F_, h=h, w=w, C=C, alpha=alpha, prev=prev[0], prev_off=prev[1], ld_prev=prev[2], flow_prev=fl[0])
    return x, fl, src, kw


def _ratio(got, x, fl, dt, h, w, alpha=ALPHA):
    """Worst err / bound over the frames of the shard (frame f of the shard is x[f + 1], warped from x[f] with flow f)."""
    worst = 0.0
    for f in range(got.shape[0]):
        if not bool(torch.isfinite(got[f].float()).all()):
            return float("inf")
        ref, b = flow_warp_ref_and_bound(x[f + 1], x[f], fl[f], alpha, dt, h, w)
        assert bool((b > 0).all()) and bool(torch.isfinite(b).all())
        worst = max(worst, float(((got[f].double() - ref).abs() / b).max()))
    return worst


def expected_outside(defect, family, h, w):
    if defect == "xy_swapped":
        return h != w and min(h, w) > 1 and family != "outside_up"
    if defect == "neighbour_unclamped":
        return family in ("outside_right", "outside_down", "on_edge")
    if defect == "ax_unrounded":
        return family == "smooth" and h * w >= 240
    if defect in ("frame_f", "ld_prev_as_ld_src"):
        return True
    return False                                                          # recip_for_true: see test_reciprocal_form_...


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_warp_bound_admits_the_model_and_refuses_each_defect(dt, family, h, w):
    x, fl, src, kw = _setup(dt, h, w, family)
    for recip in (False, True):
        got, x0, y0 = flow_warp_model(src[0], src[1], src[2], src[3], fl[1:], recip=recip, **kw)
        r = _ratio(got, x, fl, dt, h, w)
        print(f"{family} {dt} {h}x{w} recip={recip}: worst err / bound {r:.3f}")
        assert r <= 1.0, (recip, r)
        for i in range(x0.shape[0]):
            gx, gy = oflow.gather_indices(fl[1 + i], recip)
            assert torch.equal(x0[i], gx) and torch.equal(y0[i], gy)
    for d in DEFECTS:
        got, _, _ = flow_warp_model(src[0], src[1], src[2], src[3], fl[1:], defect=d, **kw)
        r = _ratio(got, x, fl, dt, h, w)
        print(f"{family} {dt} {h}x{w} defect {d}: worst err / bound {r:.3g}")
        if expected_outside(d, family, h, w):
            assert r > 1.0, (d, r)


def test_every_defect_is_refused_somewhere():
    seen = {d for d in DEFECTS for fam in FAMILIES for h, w in SHAPES if expected_outside(d, fam, h, w)}
    assert seen == set(DEFECTS) - {"recip_for_true"}


@pytest.mark.parametrize("h,w", [(32, 48), (64, 64), (96, 96)])
def test_reciprocal_form_for_true_division_shows_in_the_indices(h, w):
    dt = torch.float16
    x, fl, src, kw = _setup(dt, h, w, "integer")
    got, x0, y0 = flow_warp_model(src[0], src[1], src[2], src[3], fl[1:], defect="recip_for_true", **kw)
    assert _ratio(got, x, fl, dt, h, w) <= 1.0                            # continuous in the coordinate: the values cannot tell
    diff = sum(int(((x0[i] != oflow.gather_indices(fl[1 + i])[0]) | (y0[i] != oflow.gather_indices(fl[1 + i])[1])).sum())
               for i in range(x0.shape[0]))
    assert diff > 0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_warp_bound_at_the_ends_of_alpha(dt, alpha):
    h, w = 12, 20
    x, fl, src, kw = _setup(dt, h, w, "smooth", alpha=alpha)
    got, _, _ = flow_warp_model(src[0], src[1], src[2], src[3], fl[1:], **kw)
    assert _ratio(got, x, fl, dt, h, w, alpha) <= 1.0
    if alpha == 1.0:                                                      # alpha = 1: 1 * x is exact and oma = 0: the frame itself
        assert torch.equal(got, x[1:])


def test_warp_reference_agrees_with_grid_sample_in_fp64():
    """The independent cross-check: torch's own grid_sample in fp64 (align_corners=True, border padding) on the normalised grid."""
    h, w, C, dt = 12, 20, 8, torch.float16
    x = make_frames(2, h * w, C, dt, seed=3)
    for family in FAMILIES:
        fl = make_flow(family, 1, h, w, seed=2)[0]
        ref, _ = flow_warp_ref_and_bound(x[1], x[0], fl, 0.0, dt, h, w)     # alpha = 0: the warp alone
        xs = torch.arange(w, dtype=torch.float64).view(1, w).expand(h, w) + fl[0].double()
        ys = torch.arange(h, dtype=torch.float64).view(h, 1).expand(h, w) + fl[1].double()
        grid = torch.stack([2.0 * xs / max(w - 1, 1) - 1.0, 2.0 * ys / max(h - 1, 1) - 1.0], -1)[None]
        img = x[0].double().reshape(h, w, C).permute(2, 0, 1)[None]
        gs = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)
        assert float((gs[0].permute(1, 2, 0).reshape(h * w, C) - ref).abs().max()) < 1e-12, family


def test_flow_to_latent_bound_admits_fp32_pooling():
    g = torch.Generator().manual_seed(1)
    for f, H, W in ((1, 6, 10), (4, 24, 40), (8, 64, 32)):
        fl = torch.randn((2, 2, H, W), generator=g) * 3.0 + 1.0
        ref, b = flow_to_latent_ref_and_bound(fl, f)
        assert float(((oflow.flow_to_latent(fl, f).double() - ref).abs() / b.clamp_min(1e-300)).max()) <= 1.0
        shifted = torch.nn.functional.avg_pool2d(fl, f) / float(f * f) if f > 1 else fl * (1 + 4 * U32)
        assert float(((shifted.double() - ref).abs() / b.clamp_min(1e-300)).max()) > 1.0     # divided by f^2; a 4 U32 scale error


@pytest.mark.parametrize("idx", [0, 30, 49])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim_bound_admits_the_fp32_update_and_refuses_a_wrong_branch(idx, eta):
    g = torch.Generator().manual_seed(idx)
    eu, ec, er, x, inv, nz = (torch.randn((2, 4, 5, 7), generator=g) * s for s in (1.0, 1.1, 0.9, 1.3, 1.2, 1.0))
    sch = oddim.Schedule(50, eta)
    kw = dict(a_t=float(sch.alphas[idx]), a_prev=float(sch.alphas_prev[idx]), sigma_t=float(sch.sigmas[idx]),
              sqrt_1m_at=float(sch.sqrt_one_minus_alphas[idx]))
    noise = nz if eta else None
    out = ddim_step_ref_and_bound(eu, ec, er, x, inv, noise, scale=3.0, single=0, **kw)
    e_t, e_r = oddim.cfg_combine(eu, ec, er, 3.0)
    xp, p0 = oddim.ddim_update(x, e_t, kw["a_t"], kw["a_prev"], kw["sigma_t"], kw["sqrt_1m_at"], noise)
    xr, _ = oddim.ddim_update(inv, e_r, kw["a_t"], kw["a_prev"], kw["sigma_t"], kw["sqrt_1m_at"])
    worst = lambda got, name: float(((got.double() - out[name][0]).abs() / out[name][1]).max())
    assert worst(xp, "x_prev") <= 1.0 and worst(p0, "pred_x0") <= 1.0
    if not eta:
        assert worst(xr, "x_prev_recon") <= 1.0
    # the cond branch taken for the uncond one; the guidance applied to the recon twin as (eu - er); the noise dropped
    bad, _ = oddim.ddim_update(x, ec + 3.0 * (ec - eu), kw["a_t"], kw["a_prev"], kw["sigma_t"], kw["sqrt_1m_at"], noise)
    assert worst(bad, "x_prev") > 1.0
    if eta:
        assert worst(oddim.ddim_update(x, e_t, kw["a_t"], kw["a_prev"], kw["sigma_t"], kw["sqrt_1m_at"])[0], "x_prev") > 1.0
    # the inversion's update (ddim_w_inv.py:449) as the single-branch form with a_t = a_cur, a_prev = a_next
    a_cur, a_next = torch.tensor(kw["a_t"]), torch.tensor(kw["a_prev"])
    inv_ref = ddim_step_ref_and_bound(eu, None, None, x, None, None, scale=0.0, a_t=float(a_cur), a_prev=float(a_next), sigma_t=0.0,
                                      sqrt_1m_at=float((1 - a_cur).sqrt()), single=1)["x_prev"]
    upd = (x - (1 - a_cur).sqrt() * eu) * a_next.sqrt() / a_cur.sqrt() + (1 - a_next).sqrt() * eu
    assert float(((upd.double() - inv_ref[0]).abs() / inv_ref[1]).max()) <= 1.0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dim", [320, 2, 7])
def test_embedding_bound_admits_the_fp32_chain_and_refuses_swapped_halves(dt, dim):
    t = torch.tensor([0, 999] + oddim.ddim_timesteps(50).tolist(), dtype=torch.int64)
    ref, b = timestep_embedding_ref_and_bound(t, dim, dt)
    got = ounet.timestep_embedding(t, dim).to(dt)
    assert got.shape == ref.shape and float(((got.double() - ref).abs() / b).max()) <= 1.0
    half = dim // 2
    swapped = torch.cat([got[:, half:2 * half], got[:, :half], got[:, 2 * half:]], -1)     # [sin | cos]
    assert float(((swapped.double() - ref).abs() / b).max()) > 1.0
    if dim == 320:                                                        # freqs over dim instead of dim / 2
        args = t[:, None].float() * torch.exp(-9.210340371976184 * torch.arange(half, dtype=torch.float32) / dim)
        wrong = torch.cat([torch.cos(args), torch.sin(args)], -1).to(dt)
        assert float(((wrong.double() - ref).abs() / b).max()) > 1.0
