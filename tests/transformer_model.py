"""A CPU model of the rounding points of the norms and of the fused transformer kernels (csrc/pointwise.hip: layernorm_kernel,
gn_partial_kernel, gn_finalize_cols_kernel, gn_coeffs_cols_kernel, gn_apply_kernel; csrc/stfront.hip; csrc/ffn.hip PLAIN / PRE /
POST; csrc/linear_small.hip), plus seeded DEFECTS of one line each.  Like gemm_model.py it restates the kernels' own comments in
torch fp32 and is no reference: the references are the fp64 functions of kernel_bounds.py; this shows that their bounds admit a
correct kernel and refuse a subtly wrong one (test_transformer_bound_cpu.py).  Plain module, nothing collected by pytest.

What is modelled: GroupNorm apply as ONE multiply-add x a + b with (a, b) formed in fp32 and one rounding; fp32 accumulation
(torch's fp32 matmul: another order than the MFMAs', which the bounds allow for); LayerNorm in two passes on the fp32 tile; its
result rounded once as the next operand; the weights AS PACKED by vface_amd.packing, the activations taken in the k order the
packing implies (``packing.ffn_w2_perm``); GEGLU as value * gelu(gate) on the 16 + 16 interleaved rows of a hidden tile with gelu
from ``gemm_model.gelu_as``; the hidden activations rounded once; PRE: the accumulator starts as the residual, bo + the sample's
row bias are added where the values are read; POST: t3 rounded once before proj_out, x_in the accumulator's initial value, the
column sums per 32-token wave, then per pair of waves; GroupNorm sums in fp32 per 128-pixel chunk and group, folded in fp64;
linear_small's four quarter sums added in order.  Not modelled: the order of additions inside an MFMA, v_rsq / v_exp last bits."""
import torch

from gemm_model import gelu_as
from vface_amd.packing import ffn_w2_perm

LN_DEFECTS = ("ln_half_lanes", "ln_var_cm1", "ln_no_eps", "ln_one_pass")
GN_DEFECTS = ("gn_chunk_group", "gn_tail_pixels")
CHAIN_DEFECTS = ("k_unpermuted", "image0_ab", "rowbias_sample0", "geglu_mispaired", "t1_rounded16", "residual_after_rounding",
                 "stats_slices_swapped")
DEFECTS = LN_DEFECTS + GN_DEFECTS + CHAIN_DEFECTS


def f32(t):
    return t.float()


def silu32(f):
    return f / (1.0 + torch.exp(-f))


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_tile(v, gamma, beta, eps, defect=None):
    """The two passes on an fp32 tile ``v [M, C]`` -> fp32 (the caller rounds)."""
    C = v.shape[1]
    sel = v
    if defect == "ln_half_lanes":                  # one lane half only: the 8-channel chunks of h = 0
        sel = v[:, (torch.arange(C) // 8) % 2 == 0]
    n = sel.shape[1]
    mean = sel.sum(1, keepdim=True) / n
    if defect == "ln_one_pass":
        var = (sel * sel).sum(1, keepdim=True) / n - mean * mean
    else:
        d = sel - mean
        var = (d * d).sum(1, keepdim=True) / (n - 1 if defect == "ln_var_cm1" else n)
    rstd = torch.rsqrt(var + (0.0 if defect == "ln_no_eps" else eps))
    return (v - mean) * rstd * f32(gamma)[None, :] + f32(beta)[None, :]


def layernorm_model(x, gamma, beta, eps, dt, defect=None):
    return layernorm_tile(f32(x), gamma, beta, eps, defect).to(dt)


# ------------------------------------------------------------------------------------------------ GroupNorm
def _group_of(C, groups, defect):
    c = torch.arange(C)
    if defect == "gn_chunk_group":                 # the group taken once per 8-channel chunk, from its first channel
        c = (c // 8) * 8
    return c // (C // groups)


def gn_stats_model(x, groups, eps, defect=None):
    """``x [nimg, hw, C]`` -> stats ``[nimg, groups, 2]`` fp32: fp32 (sum, sum of squares) per 128-pixel chunk and group, fp64 fold."""
    nimg, hw, C = x.shape
    g = _group_of(C, groups, defect)
    v = f32(x)
    last = hw - hw % 128 if (defect == "gn_tail_pixels" and hw > 128) else hw
    s = torch.zeros(nimg, groups, dtype=torch.float64)
    q = torch.zeros(nimg, groups, dtype=torch.float64)
    for p0 in range(0, last, 128):
        blk = v[:, p0:min(p0 + 128, last)]
        cs, cq = blk.sum(1), (blk * blk).sum(1)                      # [nimg, C] fp32
        s += torch.zeros(nimg, groups).index_add_(1, g, cs).double()
        q += torch.zeros(nimg, groups).index_add_(1, g, cq).double()
    count = float(hw * (C // groups))
    mean = s / count
    var = torch.clamp(q / count - mean * mean, min=0.0)
    return torch.stack([mean.float(), (1.0 / torch.sqrt(var + eps)).float()], -1)


def gn_cols_model(cs, nimg, hw, groups, eps, gamma=None, beta=None, defect=None):
    """``cs [nimg hw / 64, C, 2]`` fp32 -> stats, or (stats, ab) with ``gamma, beta``: fp64 fold, one rounding, fp32 coefficients."""
    C = cs.shape[1]
    g = _group_of(C, groups, defect)
    c64 = cs.double().reshape(nimg, hw // 64, C, 2).sum(1)
    s = torch.zeros(nimg, groups, dtype=torch.float64).index_add_(1, g, c64[..., 0])
    q = torch.zeros(nimg, groups, dtype=torch.float64).index_add_(1, g, c64[..., 1])
    count = float(hw * (C // groups))
    mean = s / count
    var = torch.clamp(q / count - mean * mean, min=0.0)
    st = torch.stack([mean.float(), (1.0 / torch.sqrt(var + eps)).float()], -1)
    if gamma is None:
        return st
    a = st[:, g, 1] * f32(gamma)[None, :]
    return st, torch.stack([a, f32(beta)[None, :] - st[:, g, 0] * a], -1)


def gn_apply_model(x, stats, gamma, beta, groups, silu, dt, defect=None):
    """``x [nimg, hw, C]``, ``stats [nimg, groups, 2]`` fp32 -> ``[nimg, hw, C]`` of type ``dt``."""
    g = _group_of(x.shape[2], groups, defect)
    a = stats[:, g, 1] * f32(gamma)[None, :]
    b = f32(beta)[None, :] - stats[:, g, 0] * a
    f = f32(x) * a[:, None, :] + b[:, None, :]
    return (silu32(f) if silu else f).to(dt)


# ------------------------------------------------------------------------------------------------ linear_small
def linear_small_model(a, w, dt, bias=None, silu=False, out_f32=False):
    K = a.shape[1]
    parts = [f32(a[:, i * K // 4:(i + 1) * K // 4]) @ f32(w[:, i * K // 4:(i + 1) * K // 4]).T for i in range(4)]
    v = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    if bias is not None:
        v = v + f32(bias)[None, :]
    if silu:
        v = silu32(v)
    return v if out_f32 else v.to(dt)


# ------------------------------------------------------------------------------------------------ st_front
def st_front_model(x32, ab, hw, wcat, b_in, gamma, beta, eps, dt, defect=None):
    """``wcat``: ``packing.pack_st_front`` in ``dt``.  -> ``(t0 fp32 [M, C], ln dt [M, C], qkv dt [M, NQ])``, every projection column of
    every row (the caller compares the part a launch writes)."""
    M, C = x32.shape
    img = torch.arange(M) // hw
    if defect == "image0_ab":                      # a token tile past the first takes image 0's pair
        img = torch.where(torch.arange(M) >= 128, torch.zeros_like(img), img)
    o = (x32 * ab[img, :, 0] + ab[img, :, 1]).to(dt)
    t0 = f32(b_in)[None, :] + f32(o) @ f32(wcat[:C]).T
    ln = layernorm_tile(t0, gamma, beta, eps, defect if defect in LN_DEFECTS else None).to(dt)
    op = f32(ln) if defect == "k_unpermuted" else f32(ln)[:, ffn_w2_perm(C)]
    return t0, ln, (op @ f32(wcat[C:]).T).to(dt)


# ------------------------------------------------------------------------------------------------ ffn.hip
def ffn_model(dt, *, gamma, beta, eps, w1p, b1p, w2p, b2, x32=None, att=None, w_stream=None, bo=None, rowbias=None, rows_per_sample=1,
              resid=None, b_po=None, x_in=None, want_stats=False, defect=None):
    """PLAIN: ``x32`` with ``w1p, b1p`` = ``packing.pack_geglu`` and ``w2p`` = ``pack_ffn_w2``.  PRE: ``att, resid, bo`` [+ ``rowbias``] with
    ``w_stream`` = ``packing.pack_attn_out_ffn(wo, w1p)`` ([C + 8C, C]).  POST: ``w_stream`` with proj_out's rows behind ([C + 8C + C, C])
    and ``b_po, x_in``.  -> ``(out32, out16)`` or, POST, ``(y32, y16, colstats [M / 64, C, 2] | None)``."""
    pre = att is not None
    post = pre and x_in is not None
    M, C = (att if pre else x32).shape
    perm = ffn_w2_perm(C)
    lnd = defect if defect in LN_DEFECTS else None
    if pre:
        acc = f32(resid) + f32(att) @ f32(w_stream[:C]).T                       # the accumulators start as the residual
        side = f32(bo)[None, :].expand(M, C)
        if rowbias is not None:
            sample = torch.arange(M) // rows_per_sample
            if defect == "rowbias_sample0":
                sample = torch.zeros_like(sample)
            side = f32(bo)[None, :] + f32(rowbias)[sample]
        t1 = acc + side
        w1 = w_stream[C:9 * C]
    else:
        t1, w1 = f32(x32), w1p
    ln_in = t1.to(dt).float() if defect == "t1_rounded16" else t1
    ln = layernorm_tile(ln_in, gamma, beta, eps, lnd).to(dt)
    op = f32(ln)[:, perm] if (pre and defect != "k_unpermuted") else f32(ln)
    y = (op @ f32(w1).T + f32(b1p)[None, :]).reshape(M, 4 * C // 16, 2, 16)
    val, gate = y[:, :, 0, :], y[:, :, 1, :]
    if defect == "geglu_mispaired":                # a value row meets its neighbour's gate row
        gate = gate.roll(1, -1)
    h = (val * gelu_as(gate)).reshape(M, 4 * C).to(dt)
    hp = f32(h) if (not pre and defect == "k_unpermuted") else f32(h)[:, ffn_w2_perm(4 * C)]
    g2 = hp @ f32(w2p).T
    if not pre:
        out = (g2 + f32(b2)[None, :]).to(dt).float() + t1 if defect == "residual_after_rounding" else (g2 + f32(b2)[None, :]) + t1
        return out, out.to(dt)
    c = f32(b2)[None, :] + side
    if not post:
        out = (g2 + c).to(dt).float() + acc if defect == "residual_after_rounding" else (acc + g2) + c
        return out, out.to(dt)
    t3 = ((acc + g2) + c).to(dt)
    tp = f32(t3) if defect == "k_unpermuted" else f32(t3)[:, perm]
    g3 = tp @ f32(w_stream[9 * C:]).T
    if defect == "residual_after_rounding":
        y = (g3 + f32(b_po)[None, :]).to(dt).float() + f32(x_in)
    else:
        y = (f32(x_in) + g3) + f32(b_po)[None, :]
    cs = None
    if want_stats:
        w = y.reshape(M // 32, 32, C)
        ws = torch.stack([w.sum(1), (w * w).sum(1)], -1)                        # per 32-token wave
        cs = ws[0::2] + ws[1::2]                                                # per pair of waves = 64-row slice
        if defect == "stats_slices_swapped":
            cs = cs.reshape(M // 128, 2, C, 2).flip(1).reshape(M // 64, C, 2)
    return y, y.to(dt), cs
