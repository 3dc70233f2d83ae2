"""The kernels of the shipped ``flow_fix`` hook and of the sampler per element against fp64 on the MI355X: ``vface_flow_warp``,
``vface_flow_to_latent``, ``vface_ddim_step`` and ``vface_timestep_embedding``, every output inside the bounds of
``kernel_bounds`` (``flow_warp_`` / ``flow_to_latent_`` / ``ddim_step_`` / ``timestep_embedding_ref_and_bound``: built from fp64
quantities of the reference alone; test_hook_bound_cpu.py shows that they admit a model of the kernels' rounding points and refuse
one-line defects of it).  The warp's gather indices are held bit for bit to ``oracle.flow.gather_indices`` in both division forms
at every shape.

Buffers of the warp: source frames 8 elements into a NaN buffer, rows ``C + 8`` apart, two rows of NaN right behind every frame;
the halo in a buffer of its own on ``C + 16``; the destination 8 elements into a ``sentinel`` buffer on ``C + 24`` with three gap
rows per frame -- after the call every element outside the destination view has its sentinel bits and no input has changed.
The DDIM step's eps is a ``lde = 8`` view for C = 4 in a NaN buffer that always holds three chunks of rows, the ones the mode must
not read left NaN; its outputs lie inside fp32 sentinel buffers."""
import pytest
import torch

from hook_model import FAMILIES, lay_frames, make_flow, make_frames
from kernel_bounds import (assert_within, ddim_step_ref_and_bound, flow_to_latent_ref_and_bound, flow_warp_ref_and_bound, note,
                           same_bits, sentinel, timestep_embedding_ref_and_bound)

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
ERR_ARG, ERR_ALIGN, ERR_SHAPE = -1, -2, -3          # include/vface_hip.h


def hip():
    from vface_amd import hip as h
    h.load()
    return h


# ------------------------------------------------------------------------------------------------ flow warp
# (h, w, C, F, halo, alpha, flow family, reciprocal form).  96 x 96 x 640 is past the grid cap of 2048 workgroups per frame
# (96 x 96 x 640 / 8 / 256 = 2880: the 768 x 768 workload's level-1 map at level 0's width).
WARP = [
    (64, 64, 8, 2, False, 0.8, "smooth", False),
    (32, 48, 24, 5, True, 0.8, "integer", False),
    (48, 32, 8, 2, True, 0.0, "outside_left", True),
    (1, 40, 24, 1, True, 0.8, "smooth", False),           # F = 1 with a halo
    (40, 1, 8, 2, False, 1.0, "outside_down", False),
    (5, 7, 640, 2, True, 0.8, "on_edge", False),
    (5, 7, 8, 1, False, 0.8, "smooth", False),            # F = 1 without one: a pure copy
    (32, 48, 8, 2, False, 0.8, "outside_right", True),
    (48, 32, 24, 5, False, 0.0, "outside_up", False),
    (64, 64, 24, 2, True, 1.0, "integer", True),
    (5, 7, 24, 5, True, 0.0, "on_edge", True),
    (32, 48, 640, 2, False, 0.8, "smooth", True),
    (1, 40, 8, 2, False, 0.8, "outside_right", False),
    (40, 1, 24, 2, True, 0.8, "outside_up", True),
    (48, 32, 8, 5, True, 0.8, "outside_down", False),
    (64, 64, 8, 2, True, 0.8, "outside_left", False),
    (96, 96, 640, 2, False, 0.8, "smooth", False),
    (32, 48, 8, 1, True, 0.8, "integer", True),
    (1, 40, 8, 2, True, 0.8, "integer", True),
    (96, 96, 8, 2, False, 0.8, "integer", True),
]
assert {c[:2] for c in WARP} >= {(64, 64), (32, 48), (48, 32), (1, 40), (40, 1), (5, 7)} and {c[2] for c in WARP} == {8, 24, 640}
assert {c[3] for c in WARP} == {1, 2, 5} and {c[5] for c in WARP} == {0.0, 0.8, 1.0} and {c[6] for c in WARP} == set(FAMILIES)
assert {(c[3], c[4]) for c in WARP} >= {(1, True), (1, False), (2, True), (2, False), (5, True), (5, False)}
assert all(any(c[6] == fam and c[7] == r for c in WARP) for fam in ("smooth", "integer") for r in (False, True))
assert any(c[0] * c[1] * (c[2] // 8) > 2048 * 256 for c in WARP)
assert all({c[7] for c in WARP if c[:2] == s and c[3] > 1} == {False, True} for s in {c[:2] for c in WARP})      # indices: both forms per shape


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,w,C,F_,halo,alpha,family,recip", WARP)
def test_flow_warp_per_element_strided_poisoned_views(dt, h, w, C, F_, halo, alpha, family, recip):
    hp = hip()
    hw = h * w
    x = make_frames(F_ + 1, hw, C, dt, seed=h + 3 * w + C)                # frame 0 of the draw is the halo
    fl = make_flow(family, F_, h, w, seed=F_)                             # flow f warps frame f of the draw onto frame f + 1
    sb, so, ld_src, fs_src = lay_frames(x[1:], C + 8, 2, 8)
    pb, po, ld_prev, _ = lay_frames(x[:1], C + 16, 1, 8)
    ld_dst, fs_dst, do = C + 24, (hw + 3) * (C + 24), 8
    keep = sentinel(1, do + F_ * fs_dst + ld_dst, dt).flatten()
    sd, pd, dd = sb.to(DEV), pb.to(DEV), keep.to(DEV)
    flow_d = fl[1:].contiguous().to(DEV) if F_ > 1 else None
    fp_d = fl[0].contiguous().to(DEV)
    dbg = {}
    if F_ > 1:
        dbg_keep = torch.full((2, (F_ - 1) * hw + 64), -7, dtype=torch.int32)
        dbg_d = dbg_keep.to(DEV)
        dbg = dict(dbg_x0=dbg_d[0], dbg_y0=dbg_d[1])
    hp.flow_warp(sd[so:], dd[do:], flow_d, F=F_, h=h, w=w, C_=C, ld_src=ld_src, fs_src=fs_src, ld_dst=ld_dst, fs_dst=fs_dst, alpha=alpha,
                 cuda_recip_div=recip, **(dict(prev=pd[po:], ld_prev=ld_prev, flow_prev=fp_d) if halo else {}), **dbg)
    torch.cuda.synchronize()
    got_all = dd.cpu()
    view = lambda t: t[do:do + F_ * fs_dst].as_strided((F_, hw, C), (fs_dst, ld_dst, 1))
    got = view(got_all).clone()
    expect = keep.clone()
    view(expect).copy_(got)
    assert same_bits(got_all, expect), "a store outside the destination view"
    assert same_bits(sd.cpu(), sb) and same_bits(pd.cpu(), pb), "an input changed"
    what = f"warp {dt} {h}x{w} C={C} F={F_} halo={halo} alpha={alpha} {family} recip={recip}"
    if F_ > 1:
        from oracle import flow as oflow
        idx = dbg_d.cpu()
        assert bool((idx[:, (F_ - 1) * hw:] == -7).all()), "a store behind the index buffers"
        for i in range(F_ - 1):
            gx, gy = oflow.gather_indices(fl[1 + i], recip)
            assert torch.equal(idx[0, i * hw:(i + 1) * hw].reshape(h, w), gx), f"{what}: x0 of flow {i}"
            assert torch.equal(idx[1, i * hw:(i + 1) * hw].reshape(h, w), gy), f"{what}: y0 of flow {i}"
    for f in range(F_):
        if f == 0 and not halo:
            assert same_bits(got[0], x[1]), f"{what}: frame 0 without a halo is a copy"
            continue
        ref, bound = flow_warp_ref_and_bound(x[f + 1], x[f], fl[f], alpha, dt, h, w)
        err = assert_within(got[f], ref, bound, f"{what} frame {f}")
        note("flow_warp", err, bound)
        if alpha == 1.0:                                                  # 1 * x + 0 * warp (no drawn input is -0, which would come out +0)
            assert same_bits(got[f], x[f + 1]), f"{what}: alpha = 1 returns the frame itself"


def test_flow_warp_refusals_leave_the_output_untouched():
    hp = hip()
    dt, h, w, C, F_ = torch.float16, 8, 8, 16, 2
    src = torch.zeros(F_ * h * w * C, dtype=dt, device=DEV)
    flow = torch.zeros(F_ - 1, 2, h, w, device=DEV)
    keep = sentinel(F_ * h * w, C, dt).flatten()
    dst = keep.to(DEV)
    one = torch.zeros(h * w, dtype=torch.int32, device=DEV)
    base = dict(F=F_, h=h, w=w, C_=C, ld_src=C, fs_src=h * w * C, ld_dst=C, fs_dst=h * w * C, alpha=0.8)
    hp.flow_warp(src, dst, flow, **base)                                  # the base call itself is accepted
    torch.cuda.synchronize()
    dst.copy_(keep)
    for change, code in ((dict(C_=12), ERR_ALIGN), (dict(ld_src=C + 4), ERR_ALIGN), (dict(ld_dst=C + 2), ERR_ALIGN),
                         (dict(prev=src, ld_prev=C), ERR_ARG),             # a halo without its flow field
                         (dict(dbg_x0=one), ERR_ARG), (dict(dbg_y0=one), ERR_ARG),
                         (dict(h=64, w=64, ld_src=2 ** 20), ERR_SHAPE)):   # one frame view would span 4 GiB: past a buffer descriptor's reach
        with pytest.raises(hp.VFaceHipError, match=rf"\(code {code}\)"):
            hp.flow_warp(src, dst, flow, **{**base, **change})
    torch.cuda.synchronize()
    assert same_bits(dst.cpu(), keep)


# ------------------------------------------------------------------------------------------------ flow resample
@pytest.mark.parametrize("P,H,W,f", [(3, 40, 24, 1), (2, 96, 64, 4), (2, 64, 160, 8), (1, 24, 8, 8), (1, 1024, 1024, 1)])
def test_flow_to_latent_per_element(P, H, W, f):
    """Factors 1, 4 and 8, H != W, a single output row, and factor 1 at 1024 x 1024 (2 x 2^20 outputs: past the cap of 4096
    workgroups, every thread walks its loop twice)."""
    hp = hip()
    g = torch.Generator().manual_seed(H + W + f)
    fl = torch.randn((P, 2, H, W), generator=g) * 3.0 + torch.arange(P * 2, dtype=torch.float32).view(P, 2, 1, 1) - 1.0
    assert P * 2 * (H // f) * (W // f) > 4096 * 256 or H < 1024
    fd = fl.to(DEV)
    got = hp.flow_to_latent(fd, f).cpu()
    assert same_bits(fd.cpu(), fl)
    ref, bound = flow_to_latent_ref_and_bound(fl, f)
    err = assert_within(got, ref, bound, f"flow_to_latent P={P} {H}x{W} f={f}")
    note("flow_to_latent", err, bound)


def test_flow_to_latent_refuses_a_size_that_is_no_multiple_of_the_factor():
    hp = hip()
    for H, W in ((60, 64), (64, 60)):
        with pytest.raises(hp.VFaceHipError, match=rf"\(code {ERR_SHAPE}\)"):
            hp.flow_to_latent(torch.zeros(1, 2, H, W, device=DEV), 8)


# ------------------------------------------------------------------------------------------------ DDIM step
# (single_branch, pred_x0, recon twin, eta, schedule index, F, hw, scale).  The last is past the launch cap (8192 workgroups of 256).
DDIM = [
    (0, True, True, 0.0, 30, 3, 35, 3.0),
    (0, False, False, 1.0, 49, 1, 63, 3.0),
    (0, True, True, 0.0, 0, 3, 9, 0.0),
    (1, False, False, 0.0, 0, 3, 35, 0.0),                # the inversion's call
    (1, True, False, 0.0, 49, 1, 63, 0.0),
    (1, False, False, 0.0, 30, 3, 9, 0.0),
    (2, True, False, 1.0, 30, 3, 35, 3.0),                # the sampler's call with eta != 0
    (2, True, False, 0.0, 49, 3, 63, 3.0),
    (2, False, False, 1.0, 0, 1, 9, 3.0),
    (2, True, False, 0.0, 30, 3, 419 * 419, 3.0),
]
assert {c[0] for c in DDIM} == {0, 1, 2} and {c[4] for c in DDIM} == {0, 30, 49} and {c[5] for c in DDIM} == {1, 3}
assert {(c[0], c[4]) for c in DDIM} == {(s, i) for s in (0, 1, 2) for i in (0, 30, 49)} and {c[7] for c in DDIM} == {0.0, 3.0}
assert any(c[5] * 4 * c[6] > 8192 * 256 for c in DDIM) and all(c[6] % 2 for c in DDIM)


def _framed32(shape, off):
    n = 1
    for s in shape:
        n *= s
    keep = sentinel(1, off + n + 40, torch.float32).flatten()
    return keep, keep.to(DEV), off, n


@pytest.mark.parametrize("single,want_p0,recon,eta,idx,F_,hw,scale", DDIM)
def test_ddim_step_per_element(single, want_p0, recon, eta, idx, F_, hw, scale):
    hp = hip()
    from oracle import ddim as oddim
    C, lde = 4, 8
    g = torch.Generator().manual_seed(100 * single + idx + hw % 97)
    draw = lambda s: torch.randn((F_, C, hw), generator=g) * s
    eu, ec, er, x, inv, nz = draw(1.0), draw(1.1) + 0.2, draw(0.9) - 0.3, draw(1.3), draw(1.2), draw(1.0)
    chunks = {0: (eu, ec, er), 1: (eu,), 2: (eu, ec)}[single]
    eps = torch.full((4 + 3 * F_ * hw, lde), float("nan"))                # the view: 4 rows in, columns 4 .. 7 of the buffer's 8
    for i, e in enumerate(chunks):
        eps[4 + i * F_ * hw:4 + (i + 1) * F_ * hw, 4:4 + C] = e.permute(0, 2, 1).reshape(F_ * hw, C)
    sch = oddim.Schedule(50, eta)
    a_t, a_prev, sigma_t, s1m = (float(v[idx]) for v in (sch.alphas, sch.alphas_prev, sch.sigmas, sch.sqrt_one_minus_alphas))
    if single == 1:                                                       # a_t = a_cur, a_prev = a_next, as ddim_invert passes them
        a_t, a_prev = a_prev, a_t
        s1m = float((1.0 - torch.tensor(a_t, dtype=torch.float32)).sqrt())
    assert (sigma_t != 0.0) == (eta != 0.0)
    noise = nz if eta else None
    ed = eps.to(DEV)
    outs = {"x_prev": _framed32((F_, C, hw), 12)}
    if want_p0:
        outs["pred_x0"] = _framed32((F_, C, hw), 20)
    if recon:
        outs["x_prev_recon"] = _framed32((F_, C, hw), 4)
    arg = lambda name: outs[name][1][outs[name][2]:] if name in outs else None
    xd, invd, nd = x.to(DEV), inv.to(DEV), (noise.to(DEV) if noise is not None else None)
    hp.ddim_step(ed[4:, 4:], xd, invd if single == 0 else None, arg("x_prev"), F=F_, C_=C, hw=hw, lde=lde, scale=scale, a_t=a_t,
                 a_prev=a_prev, sigma_t=sigma_t, sqrt_one_minus_at=s1m, pred_x0=arg("pred_x0"), x_prev_recon=arg("x_prev_recon"),
                 noise=nd, single_branch=single)
    torch.cuda.synchronize()
    assert same_bits(xd.cpu(), x) and same_bits(invd.cpu(), inv) and same_bits(ed.cpu(), eps), "an input changed"
    refs = ddim_step_ref_and_bound(eu, ec if single != 1 else None, er if single == 0 else None, x, inv if single == 0 else None, noise,
                                   scale=scale, a_t=a_t, a_prev=a_prev, sigma_t=sigma_t, sqrt_1m_at=s1m, single=single)
    what = f"ddim single={single} eta={eta} idx={idx} F={F_} hw={hw} scale={scale}"
    for name, (keep, dev, off, n) in outs.items():
        allv = dev.cpu()
        got = allv[off:off + n].clone()
        expect = keep.clone()
        expect[off:off + n] = got
        assert same_bits(allv, expect), f"{what}: a store outside {name}"
        ref, bound = refs[name]
        err = assert_within(got.reshape(F_, C, hw), ref, bound, f"{what} {name}")
        note("ddim_step", err, bound)


# ------------------------------------------------------------------------------------------------ timestep embedding
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dim", [320, 2, 7, 321])
def test_timestep_embedding_per_element(dt, dim):
    """Every timestep of the 50-step schedule plus 0 and 999; dim 320, the smallest (2) and odd ones with their zero pad; one
    sentinel row behind the output."""
    hp = hip()
    from oracle import ddim as oddim
    t = torch.tensor([0, 999] + oddim.ddim_timesteps(50).tolist(), dtype=torch.int64)
    N = t.numel()
    keep = sentinel(N + 1, dim, dt)
    out = keep.to(DEV)
    hp.timestep_embedding(t.to(DEV), out, dim)
    torch.cuda.synchronize()
    allv = out.cpu()
    assert same_bits(allv[N:], keep[N:]), "a store behind the output"
    ref, bound = timestep_embedding_ref_and_bound(t, dim, dt)
    err = assert_within(allv[:N], ref, bound, f"timestep_embedding {dt} dim={dim}")
    note("timestep_embedding", err, bound)
    if dim % 2:
        assert same_bits(allv[:N, dim - 1], torch.zeros(N, dtype=dt)), "the zero pad of an odd dim"
