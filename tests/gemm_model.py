"""A CPU model of the rounding points of ``vface_gemm`` and of the implicit-GEMM convolutions (csrc/gemm.hip, csrc/conv.hip), plus
seeded DEFECTS of one line each.  It restates the kernels' own comments in torch fp32: it is not a reference (the references are
the fp64 sums of ``kernel_bounds.gemm_ref_and_bound`` / ``conv_ref_and_bound``) -- it shows that the bounds admit a correct kernel
and refuse a subtly wrong one (test_gemm_bound_cpu.py).  Plain module, nothing collected by pytest.

What is modelled: products of two 16-bit values, exact in fp32; accumulation in fp32 over 64-wide K tiles of two 32-deep MFMA
steps; split-K shares of whole K tiles, their fp32 partial sums added in order; the epilogue ``(acc + bias) + rowbias``, then the
residual, then ONE rounding to the 16-bit type (or none: the fp32 forms); GEGLU as ``value * gelu(gate)`` with gelu from the
Abramowitz & Stegun 7.1.26 formula as the comment above ``gelu_erf_f`` in csrc/common.hpp states it; the convolution as the GEMM
of an explicit window matrix, taps outside the image reading zeros; the fused GroupNorm input as ``round(act(x * a + b))`` with the
zero padding applied after it.  Not modelled: the order of the fp32 additions inside an MFMA, v_rcp_f32's and v_exp_f32's last bits."""
import math

import torch

BM, BK, STEP = 128, 64, 32
GEMM_DEFECTS = ("k_tail_dropped", "row_tail", "bias_lane_shift", "rowbias_tile_sample", "residual_after_rounding", "acc16", "geglu_swapped")
CONV_DEFECTS = ("pad_wraps", "pad_trailing_as_symmetric", "stride2_odd")
DEFECTS = GEMM_DEFECTS + CONV_DEFECTS


def gelu_as(x):
    """x Phi(x) in fp32 with Phi from A&S 7.1.26: erfc(z) = (a1 t + ... + a5 t^5) exp(-z^2), t = 1 / (1 + p z), z = |x| / sqrt(2);
    x Phi(x) = max(x, 0) - |x| erfc(z) / 2."""
    p, a = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    ax = x.abs()
    z = ax * f(1.0 / math.sqrt(2.0))
    t = 1.0 / (1.0 + f(p) * z)
    poly = f(a[4])
    for c in (a[3], a[2], a[1], a[0]):
        poly = poly * t + f(c)
    u = 0.5 * (poly * t) * torch.exp(-(z * z))
    return torch.clamp(x, min=0.0) - ax * u


def gemm_model(a, w, dt, *, bias=None, rowbias=None, rows_per_sample=1, residual=None, out_f32=False, splits=1, geglu=False,
               defect=None):
    """The arguments of ``kernel_bounds.gemm_ref_and_bound`` -> ``[M, N]`` (``[M, N / 2]`` with ``geglu``) of type ``dt``, or
    fp32 with ``out_f32``.  ``splits``: the K tiles are dealt ceil(tiles / splits) to a share, as the launcher does."""
    assert defect is None or defect in DEFECTS
    af, wf = a.float(), w.float()
    M, K = af.shape
    N = wf.shape[0]
    if defect == "k_tail_dropped":
        K -= K % BK
    ntk = -(-K // BK)
    per = max(1, -(-ntk // splits))
    parts = []
    for s0 in range(0, max(ntk, 1), per):
        acc = torch.zeros(M, N)
        for kt in range(s0, min(s0 + per, ntk)):
            for k0 in range(kt * BK, min((kt + 1) * BK, K), STEP):
                k1 = min(k0 + STEP, K)
                acc = acc + af[:, k0:k1] @ wf[:, k0:k1].T
            if defect == "acc16":
                acc = acc.to(dt).float()
        parts.append(acc)
    v = parts[0] if len(parts) == 1 else sum(parts[1:], torch.zeros(M, N) + parts[0])
    if bias is not None:
        b = bias.float()
        if defect == "bias_lane_shift":          # the lanes of quad column 1 read their four biases one lane group further on
            n = torch.arange(N)
            b = b[torch.where((n // 4) % 4 == 1, torch.clamp(n + 4, max=N - 1), n)]
        v = v + b[None, :]
    if rowbias is not None:
        m = torch.arange(M)
        if defect == "rowbias_tile_sample":      # the preloaded form taken although the tile straddles samples
            m = (m // BM) * BM
        v = v + rowbias.float()[m // rows_per_sample]
    if geglu:
        val, gate = v[:, :N // 2], v[:, N // 2:]
        if defect == "geglu_swapped":
            val, gate = gate, val
        v = val * gelu_as(gate)
    if residual is not None:
        v = v.to(dt).float() + residual.float() if defect == "residual_after_rounding" else v + residual.float()
    out = v if out_f32 else v.to(dt)
    if defect == "row_tail" and M % BM and M > 1:
        out[M - 1] = out[M - 2]
    return out


def window_matrix(x, KH, KW, stride, upsample, pad, defect=None):
    """``x [nimg, C, H, W]`` -> ``([nimg * OH * OW, KH * KW * C] fp32 in (tap, channel) order, OH, OW)`` by explicit gathers, the way
    the kernel addresses its taps: output pixel (oy, ox), tap (ky, kx) reads pixel (oy stride - top + ky, ox stride - left + kx) of
    the (upsampled) image, or zeros outside it."""
    nimg, C, H, W = x.shape
    VH, VW = (2 * H, 2 * W) if upsample else (H, W)
    pt, pb, pl, pr = pad
    OH, OW = (VH + pt + pb - KH) // stride + 1, (VW + pl + pr - KW) // stride + 1
    if defect == "pad_trailing_as_symmetric" and (pt, pl) == (0, 0):
        pt, pl = 1, 1
    src = torch.cat([x.float().permute(0, 2, 3, 1).reshape(nimg, H * W, C), torch.zeros(nimg, 1, C)], 1)
    oy, ox = torch.meshgrid(torch.arange(OH), torch.arange(OW), indexing="ij")
    y0, x0 = oy * stride - pt, ox * stride - pl
    if defect == "stride2_odd" and stride == 2:
        if VH % 2:
            y0 = torch.where(oy == OH - 1, y0 - 1, y0)
        if VW % 2:
            x0 = torch.where(ox == OW - 1, x0 - 1, x0)
    taps = []
    for ky in range(KH):
        for kx in range(KW):
            iy, ix = y0 + ky, x0 + kx
            ok = (iy >= 0) & (iy < VH) & (ix >= 0) & (ix < VW)
            if defect == "pad_wraps":            # only the flat pixel index is tested: a left / right tap lands in the neighbouring row
                flat = iy * VW + ix
                ok = (iy >= -1) & (iy <= VH) & (flat >= 0) & (flat < VH * VW)
                iy, ix = flat // VW, flat % VW
            sy, sx = (iy // 2, ix // 2) if upsample else (iy, ix)
            idx = torch.where(ok, sy * W + sx, torch.full_like(iy, H * W)).reshape(-1)
            taps.append(src[:, idx, :])                                          # [nimg, OH * OW, C]
    return torch.stack(taps, 2).reshape(nimg * OH * OW, KH * KW * C), OH, OW


def conv_model(x, w, dt, *, stride=1, upsample=False, pad=(1, 1, 1, 1), bias=None, rowbias=None, residual=None, x2=None, w2=None,
               scale_shift=None, silu=False, out_f32=False, splits=1, defect=None):
    """The arguments of ``kernel_bounds.conv_ref_and_bound`` -> ``[nimg * OH * OW, Cout]``."""
    cout, cin, KH, KW = w.shape
    if scale_shift is not None:
        t = x.float() * scale_shift[:, :, 0][:, :, None, None] + scale_shift[:, :, 1][:, :, None, None]
        x = (t / (1.0 + torch.exp(-t)) if silu else t).to(dt)
    cols, OH, OW = window_matrix(x, KH, KW, stride, upsample, pad, defect if defect in CONV_DEFECTS else None)
    wk = w.float().permute(0, 2, 3, 1).reshape(cout, KH * KW * cin)
    if x2 is not None:
        cols, wk = torch.cat([cols, x2.float()], 1), torch.cat([wk, w2.float()], 1)
    return gemm_model(cols.to(dt), wk.to(dt), dt, bias=bias, rowbias=rowbias, rows_per_sample=OH * OW, residual=residual,
                      out_f32=out_f32, splits=splits, defect=defect if defect in GEMM_DEFECTS else None)
