"""The norms and the fused transformer kernels per element against fp64 on the MI355X: ``vface_layernorm``, the GroupNorm family
(statistics from pixels, finalize / coefficients from column sums, apply), ``vface_st_front``, the three forms of csrc/ffn.hip,
``vface_linear_small``, the out layer (``vface_gn_silu_conv3x3_small``) and the input convolution on 16 stored channels -- every
output element within a bound of kernel_bounds.py built from fp64 quantities of the reference alone, shown by
test_transformer_bound_cpu.py to admit a model of the kernels' rounding points and to refuse one-line defects of it.

Buffers, as in test_gemm_conv_gpu.py: every output (t0, ln, qkv, out16, out32, the column statistics, stats, ab) is a ``Framed``
view inside a sentinel buffer whose frame is compared bit for bit after the call; every input is a ``strided`` view into a wider
NaN-filled buffer, its leading dimension other than its width and within the header's alignment rules (fp32: width + 8, 16-bit:
width + 16, coefficient pairs: C + 8).  Wherever there is more than one image or sample they differ in mean and scale, and rows
carry an offset per 64-row slice where column statistics are checked.  Fused chains are checked stage by stage wherever the
kernel exposes the intermediate (st_front: t0 from x32 and the device's ab, ln from the device's t0, qkv from the device's ln bits;
POST: y from the PRE form's fp32 output of the same inputs) and through the whole chain's bound otherwise.

``gn_apply_kernel`` has two instantiations and no query: the launcher (csrc/pointwise.hip, vface_groupnorm_apply) starts at ppb = 128
pixels per workgroup and halves it ``while (ppb > 4 && nimg * ceil(hw / ppb) < 1024)``; the one-pixel-per-trip form runs ``if (ppb >
32)``, i.e. iff nimg * ceil(hw / 64) >= 1024: nimg = 8, hw = 8200 gives 8 * 129 = 1032 (and 8 * 65 = 520 < 1024 at ppb = 128, so
ppb = 64).  The persistent walks of st_front need more token tiles than CUs: 2 * CUs + 3, the CU count from the device properties."""
import math

import pytest
import torch

from kernel_bounds import (Framed, as_16bit, assert_within, colstats_ref_and_bound, conv_ref_and_bound, ffn_ref_and_bound,
                           gn_apply_ref_and_bound, gn_cols_ref_and_bound, gn_stats_ref_and_bound, layernorm_ref_and_bound,
                           linear_small_ref_and_bound, note, rnd, same_bits, st_front_qkv_ref_and_bound, st_front_t0_ref_and_bound, strided)

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
ERR_ARG, ERR_ALIGN, ERR_SHAPE = -1, -2, -3          # include/vface_hip.h


def hip():
    from vface_amd import hip as h
    h.load()
    return h


def refused(h, code):
    return pytest.raises(h.VFaceHipError, match=rf"\(code {code}\)")


def sview(x):
    """An input on the device as a strided view in a NaN buffer: 4 columns in for fp32 (ld = width + 8), 8 for 16-bit (+ 16)."""
    return strided(x, 4 if x.dtype == torch.float32 else 8)


def pairs_view(t):
    """``[rows, C, 2]`` fp32 pairs (coefficients, column sums) as a view into a NaN buffer ``[rows, C + 8, 2]``, 4 pairs in."""
    buf = torch.full((t.shape[0], t.shape[1] + 8, 2), float("nan"), dtype=torch.float32)
    buf[:, 4:4 + t.shape[1]] = t
    return buf.to(DEV)[:, 4:4 + t.shape[1]]


def image_rows(M, hw, C, seed, ms=1.0):
    """Token rows whose images differ in mean and scale and whose 64-row slices carry an offset of their own."""
    img = torch.arange(M) // hw
    x = rnd((M, C), seed, torch.float32) * (1.0 + 0.5 * (img % 3))[:, None] + ms * (0.7 * (img % 3) - 0.5)[:, None]
    return x + (0.25 * ((torch.arange(M) // 64) % 4))[:, None]


def cols_of(x32, nimg, hw):
    """Per-64-row (sum, sum of squares) in fp32 of ``x32 [nimg hw, C]`` -> ``[nimg hw / 64, C, 2]``."""
    sl = x32.reshape(nimg * hw // 64, 64, -1)
    return torch.stack([sl.sum(1), (sl * sl).sum(1)], -1)


def plain_slices(M):
    return [torch.arange(s, min(s + 64, M)) for s in range(0, M, 64)]


# ================================================================================================ LayerNorm
LN_C = (8, 64, 320, 512, 520, 1024, 1544, 2048)


def ln_rows(M, C, seed):
    """Rows with offset / spread 0, 8 and 64 in turn; the last of several is a constant row of modest value."""
    x = rnd((M, C), seed, torch.float32) + torch.tensor([0.0, 8.0, 64.0])[torch.arange(M) % 3][:, None]
    if M > 1:
        x[M - 1] = 3.0
    return x


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("in32", [True, False])
@pytest.mark.parametrize("C", LN_C)
def test_layernorm(dt, in32, C):
    """``ceil(C / 512)`` chunks per lane (1 .. 4), the lanes past C masked (8, 520, 1544), M below, at and past a workgroup's 4 rows."""
    h = hip()
    g, b = 1.0 + rnd((C,), 2, torch.float32, 0.2), rnd((C,), 3, torch.float32, 0.2)
    for M in (1, 5, 77):
        x = ln_rows(M, C, 10 + M)
        x = x if in32 else x.to(dt)
        xd, out = sview(x), Framed(M, C, dt)
        h.layernorm(xd, g.to(DEV), b.to(DEV), out.view, M=M, C_=C, ldx=xd.stride(0), ldy=out.ld)
        ref, bound = layernorm_ref_and_bound(x, g, b, 1e-5, dt)
        what = f"layernorm {dt} in32={in32} M={M} C={C}"
        note("layernorm", assert_within(out.result(what), ref, bound, what), bound)


def test_layernorm_refusals_launch_nothing():
    h = hip()
    dt = torch.float16
    for C, ldx_extra, code in ((2056, 0, ERR_SHAPE), (12, 0, ERR_ALIGN), (64, 4, ERR_ALIGN)):
        Cb = C + 8 - C % 8 if C % 8 else C
        x = torch.zeros(4, Cb + 16, dtype=dt, device=DEV)
        out = Framed(4, Cb, dt)
        g = torch.ones(Cb, device=DEV)
        with refused(h, code):
            h.layernorm(x, g, g, out.view, M=4, C_=C, ldx=x.stride(0) + ldx_extra, ldy=out.ld)
        out.result("refused", rows=torch.arange(0))


# ================================================================================================ GroupNorm from pixels, and apply
GN_SHAPES = ((32, 32), (64, 64), (64, 32), (96, 32), (320, 32), (2080, 32), (2560, 32))
GN_HW = (1, 7, 100, 128, 130, 257)


def gn_input(nimg, hw, C, groups, seed, ms):
    """Images differ in mean and scale, groups in mean; mean / spread up to ``ms``."""
    scale = torch.tensor([1.0, 0.5, 2.0, 1.5, 0.75, 1.25, 3.0, 0.6])[:nimg, None, None]
    grp = ((torch.arange(C) // (C // groups)) % 5 - 2.0)[None, None, :] * (ms / 2.0)
    return (rnd((nimg, hw, C), seed, torch.float32) + grp) * scale


def run_gn_stats(h, x, nimg, hw, C, groups, eps, what):
    """``vface_groupnorm_stats`` into a framed ``[nimg, groups, 2]``; -> (device view, CPU copy after the frame check)."""
    xd = sview(x.reshape(nimg * hw, C))
    st = Framed(1, nimg * groups * 2, torch.float32)
    lib = h.load()
    partial = torch.empty(lib.vface_groupnorm_partial_floats(nimg, hw, C, groups), dtype=torch.float32, device=DEV)
    in32 = x.dtype == torch.float32
    rc = lib.vface_groupnorm_stats(h._p(xd), xd.stride(0), nimg, hw, C, groups, eps, h._p(partial), h._p(st.view), int(in32),
                                   h.F16 if in32 else h.dtype_code(x.dtype), h._stream())
    h._check(rc, "vface_groupnorm_stats")
    return xd, st, st.result(what + " stats").reshape(nimg, groups, 2)


def run_gn_apply(h, xd, stats_cpu, g, b, nimg, hw, C, groups, silu, dt, what):
    y = Framed(nimg * hw, C, dt)
    h.groupnorm_apply(xd, stats_cpu.to(DEV).contiguous(), g.to(DEV), b.to(DEV), y.view, nimg=nimg, hw=hw, C_=C, ldx=xd.stride(0), ldy=y.ld,
                      groups=groups, silu=silu)
    return y.result(what + " apply").reshape(nimg, hw, C)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("in32", [True, False])
@pytest.mark.parametrize("C,groups", GN_SHAPES)
def test_groupnorm_stats_and_apply(dt, in32, C, groups):
    """cpg of 1, 2, 3, 10, 65, 80 (an 8-channel chunk inside one group, spanning two, holding eight), C / 8 > 256 with and without
    a remainder, hw of 1, below / at / just past the 128-pixel chunk and two chunks + 1; mean / spread 0 and 4; both eps."""
    h = hip()
    g, b = 1.0 + rnd((C,), 6, torch.float32, 0.3), rnd((C,), 7, torch.float32, 0.2)
    for i, hw in enumerate(GN_HW):
        for nimg in (1, 3):
            eps, ms = (1e-5, 1e-6)[(i + nimg) % 2], (0.0, 4.0)[(i + nimg // 2) % 2]
            x = gn_input(nimg, hw, C, groups, 20 + i, ms)
            x = x if in32 else x.to(dt)
            what = f"groupnorm {dt} in32={in32} C={C} groups={groups} hw={hw} nimg={nimg} eps={eps} ms={ms}"
            xd, _, st = run_gn_stats(h, x, nimg, hw, C, groups, eps, what)
            ref, bound = gn_stats_ref_and_bound(x, groups, eps)
            note("groupnorm stats", assert_within(st, ref, bound, what + " stats"), bound)
            for silu in (False, True):
                y = run_gn_apply(h, xd, st, g, b, nimg, hw, C, groups, silu, dt, what)
                ref, bound = gn_apply_ref_and_bound(x, st, g, b, groups, silu, dt)
                note("groupnorm apply", assert_within(y, ref, bound, f"{what} apply silu={silu}"), bound)


def test_groupnorm_stats_at_mean_over_spread_16():
    """The one-pass sums at mean / spread 16 (fp32 input, three images of different scale): asserted against the bound WITH its
    conditioning term (m^2 + v) / v = 257, and the error of rstd relative to rstd printed beside torch's own fp32 group_norm on
    the same input on the same device (a record, no threshold)."""
    h = hip()
    nimg, hw, C, groups, eps = 3, 257, 320, 32, 1e-5
    x = (rnd((nimg, hw, C), 31, torch.float32) + 16.0) * torch.tensor([1.0, 0.5, 2.0])[:, None, None]
    what = "groupnorm mean / spread 16"
    _, _, st = run_gn_stats(h, x, nimg, hw, C, groups, eps, what)
    ref, bound = gn_stats_ref_and_bound(x, groups, eps)
    r = note("groupnorm stats, mean / spread 16", assert_within(st, ref, bound, what), bound)
    ours = float(((st[..., 1].double() - ref[..., 1]).abs() / ref[..., 1]).max())
    xt = x.permute(0, 2, 1).reshape(nimg, C, hw, 1).contiguous().to(DEV)
    _, _, rstd_t = torch.native_group_norm(xt, None, None, nimg, C, hw, groups, eps)
    theirs = float(((rstd_t.cpu().double() - ref[..., 1]).abs() / ref[..., 1]).max())
    print(f"[conditioning] mean / spread 16: |rstd - rstd64| / rstd64 worst {ours:.3e} (err / bound {r:.3f}); torch fp32 group_norm on the device {theirs:.3e}; "
          f"a quarter ulp of fp16 is {2.0 ** -13:.3e}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C,in32", [(64, True), (64, False), (320, True)])
def test_groupnorm_apply_one_pixel_per_trip_form(dt, C, in32):
    """nimg * ceil(hw / 64) = 8 * 129 >= 1024: ppb = 64 > 32, the one-pixel-per-trip instantiation (the rule is quoted in the module
    docstring).  Statistics from the device as everywhere; the reference image by image (8 x 8200 x 320 in fp64 at once is 170 MB)."""
    h = hip()
    nimg, hw, groups = 8, 8200, 32
    assert nimg * -(-hw // 64) >= 1024 > nimg * -(-hw // 128)
    x = gn_input(nimg, hw, C, groups, 41, 4.0)
    x = x if in32 else x.to(dt)
    g, b = 1.0 + rnd((C,), 6, torch.float32, 0.3), rnd((C,), 7, torch.float32, 0.2)
    what = f"groupnorm one pixel per trip {dt} C={C} in32={in32}"
    xd, _, st = run_gn_stats(h, x, nimg, hw, C, groups, 1e-5, what)
    for img in range(nimg):
        ref, bound = gn_stats_ref_and_bound(x[img:img + 1], groups, 1e-5)
        note("groupnorm stats", assert_within(st[img:img + 1], ref, bound, f"{what} stats image {img}"), bound)
    y = run_gn_apply(h, xd, st, g, b, nimg, hw, C, groups, True, dt, what)
    for img in range(nimg):
        ref, bound = gn_apply_ref_and_bound(x[img:img + 1], st[img:img + 1], g, b, groups, True, dt)
        note("groupnorm apply, one pixel per trip", assert_within(y[img:img + 1], ref, bound, f"{what} image {img}"), bound)


def test_groupnorm_refusals_launch_nothing():
    h = hip()
    dt, lib = torch.float16, h.load()
    x = torch.zeros(64, 144, dtype=dt, device=DEV)
    g = torch.ones(256, device=DEV)
    partial = torch.zeros(4096, device=DEV)
    for C, groups, ldx, code in ((128, 128, 144, ERR_SHAPE), (40, 32, 144, ERR_SHAPE), (12, 4, 144, ERR_ALIGN), (64, 32, 140, ERR_ALIGN)):
        st, y = Framed(1, 256, torch.float32), Framed(64, 128, dt)
        assert lib.vface_groupnorm_stats(h._p(x), ldx, 1, 64, C, groups, 1e-5, h._p(partial), h._p(st.view), 0, h.F16, h._stream()) == code
        with refused(h, code):
            h.groupnorm_apply(x, torch.ones(256, device=DEV), g, g, y.view, nimg=1, hw=64, C_=C, ldx=ldx, ldy=y.ld, groups=groups)
        st.result("refused stats", rows=torch.arange(0))
        y.result("refused apply", rows=torch.arange(0))


# ================================================================================================ GroupNorm from column sums
@pytest.mark.parametrize("cpg", [1, 3, 10, 65])
@pytest.mark.parametrize("hw", [64, 128, 4096])
def test_groupnorm_finalize_and_coeffs_from_cols(cpg, hw):
    """(mean, rstd) and (a, b) from column sums with ``ld_colstats = C + 8``: the fp64 fold leaves the final rounding.  Group 0 of
    image 0 has zero variance, group 1 fp32 sums whose E[x^2] - mean^2 is slightly negative (clamped: rstd = eps^-1/2)."""
    h = hip()
    groups, nimg = 32, 3
    C, spi = cpg * groups, hw // 64
    mu = ((torch.arange(C) // cpg) % 5 - 2.0)[None, :] * torch.tensor([1.0, 0.5, 2.0]).repeat_interleave(spi)[:, None]
    s = 64 * mu + 8 * rnd((nimg * spi, C), 51, torch.float32)
    cs = torch.stack([s, s * s / 64 + 63 * (1.0 + 0.1 * rnd((nimg * spi, C), 52, torch.float32)).abs()], -1)
    cs[0:spi, :cpg, 0], cs[0:spi, :cpg, 1] = 64 * 1.5, 64 * 2.25
    cs[0:spi, cpg:2 * cpg, 0], cs[0:spi, cpg:2 * cpg, 1] = 64 * 1.1, 64 * 1.2099999
    g, b = 1.0 + rnd((C,), 6, torch.float32, 0.3), rnd((C,), 7, torch.float32, 0.2)
    csd, gd, bd, lib = pairs_view(cs), g.to(DEV), b.to(DEV), h.load()
    for eps in (1e-5, 1e-6):
        st, ab = Framed(1, nimg * groups * 2, torch.float32), Framed(1, nimg * C * 2, torch.float32)
        h._check(lib.vface_groupnorm_finalize_cols(h._p(csd), csd.stride(0) // 2, nimg, hw, C, groups, eps, h._p(st.view), h._stream()), "finalize_cols")
        h._check(lib.vface_groupnorm_coeffs_from_cols(h._p(csd), csd.stride(0) // 2, nimg, hw, C, groups, eps, h._p(gd), h._p(bd), h._p(ab.view),
                                                      h._stream()), "coeffs_from_cols")
        what = f"groupnorm from cols cpg={cpg} hw={hw} eps={eps}"
        sref, sb, aref, abb = gn_cols_ref_and_bound(cs, nimg, hw, groups, eps, g, b)
        assert float(sref[0, 1, 1]) == 1.0 / math.sqrt(eps) and float(sref[0, 0, 1]) == 1.0 / math.sqrt(eps)
        note("groupnorm finalize from cols", assert_within(st.result(what + " stats").reshape(nimg, groups, 2), sref, sb, what + " stats"), sb)
        note("groupnorm coeffs from cols", assert_within(ab.result(what + " ab").reshape(nimg, C, 2), aref, abb, what + " ab"), abb)


def test_groupnorm_cols_refusals_launch_nothing():
    h = hip()
    lib = h.load()
    cs, g = torch.zeros(8, 72, 2, device=DEV), torch.ones(64, device=DEV)
    for hw, groups, ld, code in ((100, 32, 72, ERR_SHAPE), (64, 128, 72, ERR_SHAPE), (64, 24, 72, ERR_SHAPE), (64, 32, 71, ERR_SHAPE)):
        ab = Framed(1, 2 * 64 * 2, torch.float32)
        assert lib.vface_groupnorm_coeffs_from_cols(h._p(cs), ld, 2, hw, 64, groups, 1e-5, h._p(g), h._p(g), h._p(ab.view), h._stream()) == code
        ab.result("refused", rows=torch.arange(0))


# ================================================================================================ st_front
def st_weights(C, NQ, dt):
    return dict(w_in=rnd((C, C), 23, dt, C ** -0.5), b_in=rnd((C,), 24, torch.float32, 0.1), w_p=rnd((NQ, C), 25, dt, C ** -0.5),
                lg=1.0 + rnd((C,), 28, torch.float32, 0.3), lb=rnd((C,), 29, torch.float32, 0.2))


def st_coeffs(h, x, nimg, hw, C):
    """(a, b) per image from the column sums of ``x`` by the device's own kernel -> CPU ``[nimg, C, 2]``."""
    g, b = 1.0 + rnd((C,), 26, torch.float32, 0.3), rnd((C,), 27, torch.float32, 0.2)
    return h.groupnorm_coeffs_from_cols(cols_of(x, nimg, hw).to(DEV), g.to(DEV), b.to(DEV), nimg=nimg, hw=hw, C_=C, eps=1e-6).cpu()


def launch_st_front(h, xd, abd, wcat, w, t0, qkv, ln, *, M, C, hw, NQ, rows_full, nq_lo, row0=0):
    """One launch on rows [row0, row0 + M) of the framed outputs (``row0`` a multiple of ``hw``)."""
    sl = slice(row0, row0 + M)
    h.st_front(xd[sl], abd[row0 // hw:(row0 + M) // hw], wcat, w["b_in"].to(DEV), w["lg"].to(DEV), w["lb"].to(DEV), t0.view[sl], qkv.view[sl], M=M, C_=C,
               hw=hw, NQ=NQ, rows_full=rows_full, nq_lo=nq_lo, ln=ln.view[sl] if ln is not None else None)


def check_st_front(x, ab, w, t0g, qkvg, lng, qkv_init, *, hw, NQ, rows_full, nq_lo, dt, what, rows=None):
    """Per element on ``rows`` (default all): t0 from x32 and the device's ab; ln from the device's t0; qkv from the device's ln bits
    (or, without ln, the LayerNorm bound pushed through |W_p|); the columns a row range does not project keep their sentinel bits."""
    M = x.shape[0]
    rows = torch.arange(M) if rows is None else rows
    img = torch.unique(rows // hw)
    remap = torch.searchsorted(img, rows // hw)
    # (st_front_t0_ref_and_bound takes whole images: give it one pseudo-image per row's image, hw = 1 row each)
    ref, bound = st_front_t0_ref_and_bound(x[rows], ab[img][remap], 1, w["w_in"], w["b_in"], dt)
    note("st_front t0", assert_within(t0g[rows], ref, bound, what + " t0"), bound)
    lr, lb_, qr, qb = st_front_qkv_ref_and_bound(t0g[rows], w["lg"], w["lb"], 1e-5, w["w_p"], dt, ln=lng[rows] if lng is not None else None)
    if lng is not None:
        note("st_front ln", assert_within(lng[rows], lr, lb_, what + " ln"), lb_)
    full = rows < rows_full
    got = qkvg[rows]
    fam = "st_front qkv" + ("" if lng is not None else " (no ln)")
    if bool(full.any()):
        note(fam, assert_within(got[full], qr[full], qb[full], what + " qkv, full rows"), qb[full])
    if bool((~full).any()):
        note(fam, assert_within(got[~full][:, nq_lo:], qr[~full][:, nq_lo:], qb[~full][:, nq_lo:], what + " qkv, tail rows"), qb[~full][:, nq_lo:])
        assert same_bits(got[~full][:, :nq_lo], qkv_init[rows][~full][:, :nq_lo]), what + ": a tail row's columns below nq_lo were written"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", [64, 128, 320])
@pytest.mark.parametrize("tiles", [1, 2, 3])
def test_st_front(dt, C, tiles):
    """hw = 128: every token tile another image with its own (a, b).  rows_full in M, 128 and 0; nq_lo in 0, 2C and 32; ln on and
    off; NQ = 3C and 3C + 32."""
    h = hip()
    from vface_amd.packing import pack_st_front
    M, hw = 128 * tiles, 128
    x = image_rows(M, hw, C, 21)
    ab = st_coeffs(h, x, tiles, hw, C)
    xd, abd = sview(x), pairs_view(ab)
    for rows_full, nq_lo, want_ln, extra in ((M, 0, True, 0), (128, 2 * C, False, 32), (0, 32, True, 0), (0, 2 * C, False, 32), (128, 32, True, 32)):
        if rows_full == 128 and tiles == 1:
            continue                                  # (that is rows_full = M again)
        NQ = 3 * C + extra
        w = st_weights(C, NQ, dt)
        wcat = pack_st_front(w["w_in"], w["w_p"]).to(DEV)
        t0, qkv, ln = Framed(M, C, torch.float32), Framed(M, NQ, dt), Framed(M, C, dt) if want_ln else None
        init = qkv._v(qkv.keep).clone()
        launch_st_front(h, xd, abd, wcat, w, t0, qkv, ln, M=M, C=C, hw=hw, NQ=NQ, rows_full=rows_full, nq_lo=nq_lo)
        what = f"st_front {dt} C={C} tiles={tiles} rows_full={rows_full} nq_lo={nq_lo} NQ={NQ} ln={want_ln}"
        check_st_front(x, ab, w, t0.result(what + " t0"), qkv.result(what + " qkv"), ln.result(what + " ln") if ln is not None else None, init,
                       hw=hw, NQ=NQ, rows_full=rows_full, nq_lo=nq_lo, dt=dt, what=what)


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("NQ,nq_lo", [(192, 64), (224, 64)])
def test_st_front_persistent_walk_c64_per_element(dt, NQ, nq_lo):
    """2 * CUs + 3 token tiles on at most CUs workgroups: every workgroup walks two or three tiles and its ring of four weight
    stages runs on across the tile boundary at slot phase (C / 32 + projected tiles) % 4.  NQ = 192: 2 + 6 = 8 stages per full
    tile, phase 0 (what every shape of the engine has), and 2 + 4 = 6, phase 2, on the tail rows; NQ = 224, nq_lo = 64: 2 + 7 = 9
    and 2 + 5 = 7, phases 1 and 3.  Per element over all rows."""
    h = hip()
    from vface_amd.packing import pack_st_front
    C, hw = 64, 128
    tiles = 2 * cu_count() + 3
    M, rows_full = 128 * tiles, 128 * (tiles // 2 + 1)
    x = image_rows(M, hw, C, 22)
    ab = st_coeffs(h, x, tiles, hw, C)
    w = st_weights(C, NQ, dt)
    t0, qkv, ln = Framed(M, C, torch.float32), Framed(M, NQ, dt), Framed(M, C, dt)
    init = qkv._v(qkv.keep).clone()
    launch_st_front(h, sview(x), pairs_view(ab), pack_st_front(w["w_in"], w["w_p"]).to(DEV), w, t0, qkv, ln, M=M, C=C, hw=hw, NQ=NQ, rows_full=rows_full,
                    nq_lo=nq_lo)
    what = f"st_front persistent {dt} C=64 NQ={NQ} nq_lo={nq_lo} tiles={tiles}"
    check_st_front(x, ab, w, t0.result(what + " t0"), qkv.result(what + " qkv"), ln.result(what + " ln"), init, hw=hw, NQ=NQ, rows_full=rows_full,
                   nq_lo=nq_lo, dt=dt, what=what)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", [128, 320])
def test_st_front_persistent_walk_equals_chunked_launches(dt, C):
    """The same 2 * CUs + 3 tiles in one persistent launch and in launches of at most one tile per CU (no workgroup walks, no ring
    carried across a tile boundary), bit for bit, at an odd ring phase (NQ = 3C + 32); and per element on the first and the last two
    tiles of each set."""
    h = hip()
    from vface_amd.packing import pack_st_front
    hw, NQ, nq_lo = 128, 3 * C + 32, 2 * C
    ncu = cu_count()
    tiles = 2 * ncu + 3
    tilesA = tiles // 2 + 1
    M, rows_full = 128 * tiles, 128 * tilesA
    x = image_rows(M, hw, C, 23)
    ab = st_coeffs(h, x, tiles, hw, C)
    w = st_weights(C, NQ, dt)
    xd, abd, wcat = sview(x), pairs_view(ab), pack_st_front(w["w_in"], w["w_p"]).to(DEV)
    outs = []
    for chunked in (False, True):
        t0, qkv, ln = Framed(M, C, torch.float32), Framed(M, NQ, dt), Framed(M, C, dt)
        init = qkv._v(qkv.keep).clone()
        if not chunked:
            launch_st_front(h, xd, abd, wcat, w, t0, qkv, ln, M=M, C=C, hw=hw, NQ=NQ, rows_full=rows_full, nq_lo=nq_lo)
        else:
            for lo, hi, full in [(a, min(a + ncu, tilesA), True) for a in range(0, tilesA, ncu)] + \
                                [(a, min(a + ncu, tiles), False) for a in range(tilesA, tiles, ncu)]:
                m = 128 * (hi - lo)
                launch_st_front(h, xd, abd, wcat, w, t0, qkv, ln, M=m, C=C, hw=hw, NQ=NQ, rows_full=m if full else 0, nq_lo=nq_lo, row0=128 * lo)
        what = f"st_front {'chunked' if chunked else 'persistent'} {dt} C={C} tiles={tiles}"
        outs.append((t0.result(what + " t0"), qkv.result(what + " qkv"), ln.result(what + " ln")))
    for name, a, b in zip(("t0", "qkv", "ln"), *outs):
        assert same_bits(a, b), f"st_front {dt} C={C}: {name} of the persistent launch differs in bits from the chunked launches"
    edge = torch.cat([torch.arange(0, 256), torch.arange(rows_full - 256, rows_full + 256), torch.arange(M - 256, M)])
    check_st_front(x, ab, w, *outs[0], init, hw=hw, NQ=NQ, rows_full=rows_full, nq_lo=nq_lo, dt=dt, what=f"st_front persistent {dt} C={C}", rows=edge)


def test_st_front_refusals_launch_nothing():
    h = hip()
    from vface_amd.packing import pack_st_front
    dt, C, M, hw = torch.float16, 64, 256, 128
    w = st_weights(C, 3 * C, dt)
    x = image_rows(M, hw, C, 21)
    xd, abd, wcat = sview(x), pairs_view(st_coeffs(h, x, 2, hw, C)), pack_st_front(w["w_in"], w["w_p"]).to(DEV)
    t0, qkv = Framed(M, C, torch.float32), Framed(M, 3 * C, dt)
    base = dict(M=M, C=C, hw=hw, NQ=3 * C, rows_full=M, nq_lo=0)
    for kw, code in ((dict(NQ=3 * C - 16), ERR_SHAPE), (dict(nq_lo=3 * C), ERR_SHAPE), (dict(rows_full=64), ERR_SHAPE), (dict(rows_full=0), ERR_SHAPE),
                     (dict(nq_lo=16), ERR_SHAPE), (dict(hw=64), ERR_SHAPE), (dict(M=192), ERR_SHAPE)):
        with refused(h, code):
            launch_st_front(h, xd, abd, wcat, w, t0, qkv, None, **{**base, **kw})
    bd, gd, be = w["b_in"].to(DEV), w["lg"].to(DEV), w["lb"].to(DEV)
    for ld_ab, ldt0 in ((C - 8, t0.ld), (abd.stride(0) // 2, t0.ld + 2)):      # ld_ab below C; ldt0 no multiple of 4 floats
        rc = h.load().vface_st_front(h._p(xd), xd.stride(0), h._p(abd), ld_ab, hw, h._p(wcat), h._p(bd), h._p(gd), h._p(be), 1e-5, h._p(t0.view), ldt0,
                                     h._p(qkv.view), qkv.ld, None, 0, M, C, 3 * C, M, 0, h.dtype_code(dt), h._stream())
        assert rc == ERR_ALIGN, (ld_ab, ldt0, rc)
    t0.result("refused t0", rows=torch.arange(0))
    qkv.result("refused qkv", rows=torch.arange(0))


# ================================================================================================ ffn.hip: PLAIN, PRE, POST
def chain_weights(C, dt):
    k = dict(gamma=1.0 + rnd((C,), 33, torch.float32, 0.2), beta=rnd((C,), 34, torch.float32, 0.2), eps=1e-5,
             w1=rnd((8 * C, C), 35, dt, C ** -0.5), b1=rnd((8 * C,), 36, torch.float32, 0.3),
             w2=rnd((C, 4 * C), 37, dt, (4 * C) ** -0.5), b2=rnd((C,), 38, torch.float32, 0.3))
    k["b1"][4 * C:] = torch.linspace(-8.0, 8.0, 4 * C)              # gate biases over [-8, 8]
    return k


class FfnCase:
    """Inputs of one (C, M, rows per sample) on the device, every activation a strided view in a NaN buffer."""

    def __init__(self, h, C, M, rps, dt, rowbias=True):
        from vface_amd import packing
        self.h, self.C, self.M, self.rps, self.dt = h, C, M, rps, dt
        self.k = chain_weights(C, dt)
        k = self.k
        self.x32 = image_rows(M, rps, C, 31)
        self.att, self.resid = rnd((M, C), 41, dt, 0.8), image_rows(M, rps, C, 42)
        self.wo, self.bo = rnd((C, C), 44, dt, C ** -0.5), rnd((C,), 45, torch.float32, 0.2)
        self.rb = rnd((M // rps, C), 46, torch.float32, 0.5) if rowbias else None
        self.wpo, self.b_po, self.x_in = rnd((C, C), 47, dt, C ** -0.5), rnd((C,), 48, torch.float32, 0.2), image_rows(M, rps, C, 49)
        w1p, b1p = packing.pack_geglu(k["w1"], k["b1"])
        d = lambda v: v.to(DEV).contiguous()
        self.dev = dict(gamma=d(k["gamma"]), beta=d(k["beta"]), w1p=d(w1p), b1p=d(b1p), w2p=d(packing.pack_ffn_w2(k["w2"])), b2=d(k["b2"]),
                        pre_w=d(packing.pack_attn_out_ffn(self.wo, w1p)), post_w=d(packing.pack_attn_out_ffn(self.wo, w1p, self.wpo)),
                        bo=d(self.bo), b_po=d(self.b_po), x32=sview(self.x32), att=sview(self.att), resid=sview(self.resid), x_in=sview(self.x_in),
                        rb=sview(self.rb) if rowbias else None)

    def ref_kw(self, form):
        kw = dict(self.k)
        if form == "plain":
            return dict(kw, x32=self.x32)
        kw.update(att=self.att, wo=self.wo, bo=self.bo, rowbias=self.rb, rows_per_sample=self.rps, resid=self.resid)
        if form == "post":
            kw.update(wpo=self.wpo, b_po=self.b_po, x_in=self.x_in)
        return kw

    def launch(self, form, o16, o32, cs=None):
        h, d = self.h, self.dev
        v = lambda f: f.view if f is not None else None
        if form == "plain":
            h.ffn_fused(d["x32"], d["gamma"], d["beta"], d["w1p"], d["b1p"], d["w2p"], d["b2"], v(o16), M=self.M, C_=self.C, out32=v(o32))
        elif form == "pre":
            h.attn_out_ffn_fused(d["att"], d["resid"], d["rb"], d["pre_w"], d["bo"], d["gamma"], d["beta"], d["b1p"], d["w2p"], d["b2"], v(o16), M=self.M,
                                 C_=self.C, rows_per_sample=self.rps, out32=v(o32))
        else:
            h.attn_out_ffn_proj_fused(d["att"], d["resid"], d["rb"], d["post_w"], d["bo"], d["gamma"], d["beta"], d["b1p"], d["w2p"], d["b2"], d["b_po"],
                                      d["x_in"], v(o16), v(o32), cs.stats_arg[:self.M // 64] if cs is not None else None, M=self.M, C_=self.C,
                                      rows_per_sample=self.rps)


FFN_SHAPES = [(128, 128, True), (384, 128, True), (512, 256, True), (384, 128, False)]      # (M, rows per sample, row bias present)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", [64, 128, 320])
@pytest.mark.parametrize("form", ["plain", "pre"])
def test_ffn_fused_plain_and_pre(dt, C, form):
    """The whole chain's bound (none of t1, ln, the hidden activations is exposed).  out32 alone, out16 alone, both: the 16-bit
    output is the fp32 one rounded once, bit for bit, and the same bits whether or not the other output is written."""
    h = hip()
    for M, rps, with_rb in FFN_SHAPES:
        if form == "plain" and not with_rb:
            continue
        case = FfnCase(h, C, M, rps, dt, with_rb)
        ref, e = ffn_ref_and_bound(dt, **case.ref_kw(form))
        what = f"ffn {form} {dt} C={C} M={M} rps={rps} rowbias={with_rb}"
        both16, both32, only16, only32 = Framed(M, C, dt), Framed(M, C, torch.float32), Framed(M, C, dt), Framed(M, C, torch.float32)
        case.launch(form, both16, both32)
        case.launch(form, only16, None)
        case.launch(form, None, only32)
        g32, g16 = both32.result(what + " out32"), both16.result(what + " out16")
        note(f"ffn {form}", assert_within(g32, ref, e, what + " out32"), e)
        assert same_bits(g16, g32.to(dt)), what + ": the 16-bit output is not out32 rounded once"
        assert same_bits(only16.result(what + " out16 alone"), g16) and same_bits(only32.result(what + " out32 alone"), g32), what
        b16 = as_16bit(ref, e, dt)
        note(f"ffn {form} 16-bit", assert_within(g16, ref, b16, what + " out16"), b16)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", [64, 128, 320])
def test_ffn_fused_post(dt, C):
    """y = proj_out(t3) + b_po + x_in against the STAGE bound behind the PRE form's fp32 output of the same inputs (``t3_from``: the
    sibling launch exposes t3's unrounded value) and against the whole chain's bound; with and without column statistics, with
    and without out16 / out32; the statistics against the fp64 sums of y32 as stored, and the same bits without out32."""
    h = hip()
    for M, rps, with_rb in FFN_SHAPES:
        case = FfnCase(h, C, M, rps, dt, with_rb)
        what = f"ffn post {dt} C={C} M={M} rps={rps} rowbias={with_rb}"
        pre32 = Framed(M, C, torch.float32)
        case.launch("pre", None, pre32)
        ref, e = ffn_ref_and_bound(dt, t3_from=pre32.result(what + " the PRE form's out32"), **case.ref_kw("post"))
        cref, ce = ffn_ref_and_bound(dt, **case.ref_kw("post"))
        o16, o32, cs = Framed(M, C, dt), Framed(M, C, torch.float32), Framed(M // 64 + 1, C, torch.float32, pair=True)
        case.launch("post", o16, o32, cs)
        g32, g16 = o32.result(what + " out32"), o16.result(what + " out16")
        note("ffn post (stage behind PRE's out32)", assert_within(g32, ref, e, what + " out32, stage bound"), e)
        note("ffn post (whole chain)", assert_within(g32, cref, ce, what + " out32, chain bound"), ce)
        assert same_bits(g16, g32.to(dt)), what + ": the 16-bit output is not out32 rounded once"
        sref, sb = colstats_ref_and_bound(g32, plain_slices(M))
        gcs = cs.result(what + " colstats", rows=torch.arange(M // 64))[:M // 64]
        note("ffn post colstats", assert_within(gcs, sref, sb, what + " colstats"), sb)
        # without statistics, without out16, without out32: the same bits in what is written
        a32 = Framed(M, C, torch.float32)
        case.launch("post", None, a32, None)
        assert same_bits(a32.result(what + " out32 alone"), g32), what
        b16, bcs = Framed(M, C, dt), Framed(M // 64 + 1, C, torch.float32, pair=True)
        case.launch("post", b16, None, bcs)
        assert same_bits(b16.result(what + " out16 + colstats"), g16), what
        assert same_bits(bcs.result(what + " colstats without out32", rows=torch.arange(M // 64))[:M // 64], gcs), what


def test_ffn_fused_refusals_launch_nothing():
    """The argument, alignment and shape refusals vf_launch_ffn_fused states."""
    h = hip()
    dt, C, M = torch.float16, 64, 128
    case = FfnCase(h, C, M, 128, dt)
    d, o16, o32 = case.dev, Framed(M, C, dt), Framed(M, C, torch.float32)
    common = (d["gamma"], d["beta"], d["b1p"], d["w2p"], d["b2"])
    with refused(h, ERR_ARG):                        # no output at all
        h.ffn_fused(d["x32"], d["gamma"], d["beta"], d["w1p"], d["b1p"], d["w2p"], d["b2"], None, M=M, C_=C)
    with refused(h, ERR_SHAPE):                      # M no multiple of 128
        h.ffn_fused(d["x32"], d["gamma"], d["beta"], d["w1p"], d["b1p"], d["w2p"], d["b2"], o16.view, M=64, C_=C, out32=o32.view)
    with refused(h, ERR_SHAPE):                      # a width it is not built for
        h.ffn_fused(d["x32"], d["gamma"], d["beta"], d["w1p"], d["b1p"], d["w2p"], d["b2"], o16.view, M=M, C_=192, out32=o32.view)
    bad32, bad16 = torch.zeros(M, C + 10, device=DEV)[:, :C], torch.zeros(M, C + 4, dtype=dt, device=DEV)[:, :C]
    with refused(h, ERR_ALIGN):                      # ldx no multiple of 4 floats
        h.ffn_fused(bad32, d["gamma"], d["beta"], d["w1p"], d["b1p"], d["w2p"], d["b2"], o16.view, M=M,
                    C_=C, out32=o32.view)
    with refused(h, ERR_ARG):                        # rows per sample no multiple of 128
        h.attn_out_ffn_fused(d["att"], d["resid"], d["rb"], d["pre_w"], d["bo"], *common[:2], *common[2:], o16.view, M=M, C_=C, rows_per_sample=64,
                             out32=o32.view)
    with refused(h, ERR_ALIGN):                      # ldatt no multiple of 8 elements
        h.attn_out_ffn_fused(bad16, d["resid"], d["rb"], d["pre_w"], d["bo"], *common, o16.view, M=M,
                             C_=C, rows_per_sample=128, out32=o32.view)
    with refused(h, ERR_ALIGN):                      # ld_xin no multiple of 4 floats
        h.attn_out_ffn_proj_fused(d["att"], d["resid"], d["rb"], d["post_w"], d["bo"], *common, d["b_po"],
                                  bad32, o16.view, o32.view, None, M=M, C_=C, rows_per_sample=128)
    o16.result("refused out16", rows=torch.arange(0))
    o32.result("refused out32", rows=torch.arange(0))


# ================================================================================================ linear_small
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", [320, 640, 1280])
@pytest.mark.parametrize("N", [32, 96])
def test_linear_small(dt, K, N):
    """One, two and three 32-row token tiles with their tails, SiLU / fp32 output in the four combinations (and once without a
    bias), ``lda = K + 16``, ``ldw = K + 8``."""
    h = hip()
    w = rnd((N, K), 2, dt, 1 / math.sqrt(K))
    wbuf = torch.full((N, K + 8), float("nan"), dtype=dt)
    wbuf[:, :K] = w
    wd = wbuf.to(DEV)[:, :K]
    for i, M in enumerate((1, 5, 32, 33, 64, 65, 96)):
        a = rnd((M, K), 10 + i, dt)
        ad = sview(a)
        for j, (silu, f32out) in enumerate(((False, False), (True, False), (False, True), (True, True))):
            bias = None if (i + j) % 4 == 3 else rnd((N,), 3 + j, torch.float32)
            out = Framed(M, N, torch.float32 if f32out else dt)
            assert h.linear_small_supported(M, N, K)
            h.linear_small(ad, wd, bias.to(DEV) if bias is not None else None, out.view, M=M, N=N, K=K, silu=silu)
            what = f"linear_small {dt} {M}x{N}x{K} silu={silu} f32={f32out} bias={bias is not None}"
            ref, bound = linear_small_ref_and_bound(a, w, dt, bias, silu, f32out)
            note("linear_small", assert_within(out.result(what), ref, bound, what), bound)


def test_linear_small_refusals_launch_nothing():
    h = hip()
    dt = torch.float16
    a, w, out = torch.zeros(128, 1296, dtype=dt, device=DEV), torch.zeros(96, 1288, dtype=dt, device=DEV), Framed(96, 96, dt)
    lib = h.load()
    for M, N, K, lda, ldw, code in ((97, 96, 320, 1296, 1288, ERR_SHAPE), (24, 48, 320, 1296, 1288, ERR_SHAPE), (24, 96, 256, 1296, 1288, ERR_SHAPE),
                                    (24, 96, 320, 1292, 1288, ERR_ALIGN), (24, 96, 1280, 1296, 1272, ERR_ALIGN)):
        assert not h.linear_small_supported(M, N, K) or code == ERR_ALIGN
        assert lib.vface_linear_small(h._p(a), lda, h._p(w), ldw, None, h._p(out.view), out.ld, 0, 0, M, N, K, h.F16, h._stream()) == code
    out.result("refused", rows=torch.arange(0))


# ================================================================================================ the out layer
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("in32", [True, False])
@pytest.mark.parametrize("cin,cout,H,W", [(64, 4, 8, 16), (64, 3, 9, 17), (128, 4, 20, 24), (640, 4, 8, 16)])
def test_out_layer(dt, in32, cin, cout, H, W):
    """One whole 8 x 16 tile, ragged tiles in both directions, ten 64-channel chunks; one and three images with coefficients of
    their own; ``ldx``, ``ld_ab`` and ``ldo`` wider than the data.  Bound: ``conv_ref_and_bound`` with the fused scale / shift,
    the SiLU and the fp32 output."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    w = rnd((cout, cin, 3, 3), 52, dt, 1 / math.sqrt(9 * cin))
    bias = rnd((cout,), 53, torch.float32, 0.1)
    wp = pack_conv3x3(w.float()).to(dt).to(DEV)
    for nimg in (1, 3):
        M = nimg * H * W
        x = image_rows(M, H * W, cin, 51) + 0.2
        x = x if in32 else x.to(dt)
        ab = torch.stack([(1.0 + 0.3 * rnd((nimg, cin), 54, torch.float32)) * torch.tensor([1.0, 0.6, 1.7])[:nimg, None],
                          0.5 * torch.tensor([1.0, -1.0, 0.3])[:nimg, None] + 0.3 * rnd((nimg, cin), 55, torch.float32)], -1).contiguous()
        out = Framed(M, cout, torch.float32)
        h.gn_silu_conv3x3_small(sview(x), pairs_view(ab), wp, bias.to(DEV), out.view, nimg=nimg, H=H, W=W, cin=cin, cout=cout)
        what = f"out layer {dt} in32={in32} cin={cin} cout={cout} {H}x{W} nimg={nimg}"
        ref, bound = conv_ref_and_bound(x.reshape(nimg, H, W, cin).permute(0, 3, 1, 2), w, dt, bias=bias, scale_shift=ab, silu=True, out_f32=True)
        note("out layer", assert_within(out.result(what), ref, bound, what), bound)


def test_out_layer_refusals_launch_nothing():
    h = hip()
    dt, lib = torch.float16, h.load()
    x, ab, wt = torch.zeros(128, 144, dtype=dt, device=DEV), torch.ones(1, 136, 2, device=DEV), torch.zeros(8, 9 * 128, dtype=dt, device=DEV)
    out = Framed(128, 4, torch.float32)
    for cin, cout, ldx, ld_ab, ldo, code in ((64, 5, 144, 136, out.ld, ERR_SHAPE), (96, 4, 144, 136, out.ld, ERR_SHAPE), (64, 4, 140, 136, out.ld, ERR_ALIGN),
                                             (128, 4, 144, 64, out.ld, ERR_ALIGN), (64, 4, 144, 136, 3, ERR_ALIGN)):
        assert lib.vface_gn_silu_conv3x3_small(h._p(x), ldx, 0, h._p(ab), ld_ab, h._p(wt), None, h._p(out.view), ldo, 1, 8, 16, cin, cout, h.F16,
                                               h._stream()) == code
    out.result("refused", rows=torch.arange(0))


# ================================================================================================ the input convolution on 16 stored channels
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nimg,H,W,cout", [(1, 4, 16, 80), (5, 4, 16, 160), (1, 8, 16, 400), (3, 16, 16, 80)])
def test_input_conv_16_stored_channels(dt, nimg, H, W, cout):
    """csrc/inconv.hip: a wave owns 80 output channels and a workgroup four of them (Cout = 80: one live wave; 160: two; 400: a
    second workgroup row with one), a workgroup walks up to 4 slices of 64 pixels (one slice; five: a tail workgroup of one; two;
    twelve).  The fp32 carrier against ``conv_ref_and_bound``, the 16-bit copy as its single rounding bit for bit, the column
    statistics per element against the fp64 sums of the carrier as stored."""
    h = hip()
    from vface_amd import packing
    x = (rnd((nimg, 16, H, W), 1, dt).float() * torch.tensor([1.0, 0.5, 2.0, 1.5, 0.75])[:nimg, None, None, None] + 1.0).to(dt)
    w = rnd((cout, 16, 3, 3), 2, dt, 1 / 12.0)
    bias = rnd((cout,), 3, torch.float32)
    M = nimg * H * W
    o16, o32, cs = Framed(M, cout, dt), Framed(M, cout, torch.float32), Framed(M // 64 + 1, cout, torch.float32, pair=True)
    xd = strided(x.permute(0, 2, 3, 1).reshape(M, 16).contiguous(), 8)
    h.conv3x3(xd, packing.pack_conv3x3(w.float(), 16).to(device=DEV, dtype=dt), o16.view, nimg=nimg, H=H, W=W, cin=16, cout=cout, ldx=32, ldy=o16.ld,
              bias=bias.to(DEV), colstats=cs.stats_arg, out32=o32.view, split_k=False)
    what = f"input conv {dt} nimg={nimg} {H}x{W} cout={cout}"
    ref, bound = conv_ref_and_bound(x, w, dt, bias=bias, out_f32=True)
    g32, g16 = o32.result(what + " carrier"), o16.result(what + " 16-bit copy")
    note("input conv", assert_within(g32, ref, bound, what), bound)
    assert same_bits(g16, g32.to(dt)), what + ": the 16-bit copy is not the carrier rounded once"
    sref, sb = colstats_ref_and_bound(g32, plain_slices(M))
    note("input conv colstats", assert_within(cs.result(what + " colstats", rows=torch.arange(M // 64))[:M // 64], sref, sb, what + " colstats"), sb)
