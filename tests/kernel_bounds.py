"""Helpers of the per-kernel GPU tests (test_kernels_gpu.py, test_glue_kernels_gpu.py, test_attention_gpu.py, test_gemm_conv_gpu.py):
seeded 16-bit inputs, the unit in the last place of a 16-bit type, sentinel-filled buffers that show a store outside a kernel's slot,
the element-wise bound check that names the worst element, and the fp64 references with their per-element bounds: the attention
kernel's (``attention_ref_and_bound``), the GEMM family's with its epilogues, split-K and GEGLU (``gemm_ref_and_bound``), the
convolutions' (``conv_ref_and_bound``) and the column statistics' (``colstats_ref_and_bound``).  Every bound is built from fp64
quantities of the reference alone; test_attention_bound_cpu.py and test_gemm_bound_cpu.py show that each admits a model of the
kernel's rounding points and refuses one-line defects of it.  Plain functions, nothing collected by pytest."""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                                   # fp32 unit roundoff
TINY32 = 2.0 ** -126                               # smallest normal fp32: what a flushed subnormal intermediate can lose
MANT = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}   # explicit mantissa bits, smallest normal exponent


def rnd(shape, seed, dt, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt)


def ulp(ref64, dt):
    """One unit in the last place of ``dt`` at each element of the fp64 ``ref64`` (the subnormal spacing below the normals)."""
    p, emin = MANT[dt]
    _, e = torch.frexp(ref64.abs())                # |r| = m 2^e, m in [0.5, 1): floor(log2 |r|) = e - 1
    e = torch.where(ref64 == 0, torch.full_like(e, emin + 1), e)
    return torch.exp2((torch.clamp(e - 1, min=emin) - p).double())


def sentinel(rows, cols, dt):
    """-63.5 .. 63.5 in steps of 0.25 along the flat index, period 509 (built in the 16-bit type: the buffers reach 0.75 GB)."""
    period = ((torch.arange(509, dtype=torch.float32) - 254) * 0.25).to(dt)
    return period.repeat(-(-rows * cols // 509))[:rows * cols].reshape(rows, cols)


def same_bits(a, b):
    """Bit-for-bit equality of two tensors of one type (so -0 differs from +0; NaNs must carry the same payload)."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def assert_within(got, ref64, bound, what):
    """Every element of ``got`` within ``bound`` of the fp64 reference; on failure the message names the worst element."""
    got64 = got.double()
    assert got64.shape == ref64.shape, (what, got64.shape, ref64.shape)
    assert bool(torch.isfinite(got64).all()), f"{what}: non-finite output at flat index {int(torch.argmin(torch.isfinite(got64).int()))}"
    err = (got64 - ref64).abs()
    bad = err > bound
    if bool(bad.any()):
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
        worst = int(torch.argmax(ratio))
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), err.shape))
        b = bound.expand_as(err) if isinstance(bound, torch.Tensor) else torch.full_like(err, bound)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} out of bound; worst at {idx}: got {float(got64.flatten()[worst])!r} "
                             f"ref {float(ref64.flatten()[worst])!r} err {float(err.flatten()[worst]):.3e} bound {float(b.flatten()[worst]):.3e}")
    return err


def cpu_fp32_rel_error(fn, x32, factor=4.0, **kw):
    """The allowance for a transcendental step: ``factor`` x the worst relative error of torch's own fp32 ``fn`` against fp64 on the
    very inputs ``x32`` of the case (results below 2^-100 left out: a relative error means nothing on a subnormal), never less
    than ``factor`` x one fp32 ulp (2^-23)."""
    assert x32.dtype == torch.float32
    r64 = fn(x32.double(), **kw)
    r32 = fn(x32, **kw).double()
    ok = torch.isfinite(r64) & (r64.abs() >= 2.0 ** -100)
    rel = float(((r32 - r64).abs()[ok] / r64.abs()[ok]).max()) if bool(ok.any()) else 0.0
    return factor * max(rel, 2.0 ** -23)


def attention_ref_and_bound(q, k, v, scale, dt, chunk_bytes=4.0e8):
    """One (sample, head) of ``vface_attention`` in fp64 and what a correct 16-bit streaming-softmax kernel may differ by, per element.
    ``q [n, dh]``, ``k, v [nk, dh]``: the 16-bit inputs.  Returns ``(o, bound)``, both fp64 ``[n, dh]``, both from fp64 quantities of
    the reference alone.  With u the unit roundoff of ``dt``, s = scale q k^T, w = softmax(s), o = w v, A = scale |q| |k|^T and
    dev_jc = v_jc - o_c: for ANY per-score perturbation d_j the kernel's o' obeys o' - o = sum_j w_j (e^{d_j} - 1) dev_j / sum_k w_k
    e^{d_k} exactly (sum_j w_j dev_j = 0), so with |d_j| <= D, e^{d} - 1 = d + r, |r| <= 0.5 D^2 e^D and a denominator >= e^{-D}:

      bound = e^D (Tq + sum_j w_j ds_j |dev_jc| + 0.5 D^2 e^D sum_j w_j |dev_jc| + tiny sum_j |dev_jc| / L)
              + u |o| + (nk + 16) U32 (sum_j w_j |v_jc| + |o|) + 2 U32 |o| + 0.5 ulp(|o| + all of the above)

    * Tq_c = u sum_d |q_d| |G_dc|, G_dc = scale sum_j w_j k_jd dev_jc: the default form rounds q * scale * log2(e) to 16 bits once, so
      d_j is linear in the dh rounding errors of the query, shared by all its keys -- the sum over keys keeps its signs.
    * ds_j, independent per score: the fp32 dot product (dh + 8) U32 (A_j + max_k A_k) -- the maximum because the default form's
      score v_mfma_f32_16x16x32 carries -m_ref, as large as the largest score, as its C operand through the whole accumulation (the
      one term here that is looser than A_j alone); the subtraction of the reference 4 U32 |s_j - max s|; v_exp_f32 8 U32; the
      rounding of P to 16 bits u.  D = max_j (ds_j + u A_j).
    * tiny / L, L = sum_j exp(s_j - max s): what the absolute floor of a probability loses against a reference that is never above
      the row maximum (lazy, speculative and exact form alike).  fp16: 2^-25, half the subnormal spacing -- gradual underflow of the
      v_cvt_f16_f32 result, the same allowance a softmax rounded to fp16 gets.  bf16: 2^-126, below which v_exp_f32 returns 0.
    * u |o|: numerator and denominator may see differently rounded P (instantiations without a spare V column sum the fp32 P).
    * (nk + 16) U32 (sum_j w_j |v_jc| + |o|): fp32 accumulation of O and (the |o| part) of the denominator, both over nk keys.
    * 2 U32 |o| for the reciprocal and the product, and one final rounding to ``dt`` taken at the largest value the bound admits.
    Queries are walked in chunks so the [chunk, nk, dh] intermediate stays below ``chunk_bytes``."""
    u = 2.0 ** -(MANT[dt][0] + 1)
    tiny = 2.0 ** -25 if dt == torch.float16 else TINY32
    q64, k64, v64 = q.double(), k.double(), v.double()
    n, dh = q64.shape
    nk = k64.shape[0]
    kv = (k64[:, :, None] * v64[:, None, :]).reshape(nk, dh * dh)
    o_all, b_all = [], []
    step = max(1, int(chunk_bytes // (nk * dh * 8)))
    for i in range(0, n, step):
        qc = q64[i:i + step]
        s = (qc @ k64.T) * scale
        A = (qc.abs() @ k64.abs().T) * scale
        mx = s.max(dim=1, keepdim=True).values
        e = torch.exp(s - mx)
        L = e.sum(dim=1, keepdim=True)
        w = e / L
        o = w @ v64
        G = scale * ((w @ kv).reshape(-1, dh, dh) - (w @ k64)[:, :, None] * o[:, None, :])
        Tq = u * torch.einsum("qd,qdc->qc", qc.abs(), G.abs())
        ds = (dh + 8) * U32 * (A + A.max(dim=1, keepdim=True).values) + 4 * U32 * (mx - s) + 8 * U32 + u
        D = (ds + u * A).max(dim=1, keepdim=True).values
        eD = torch.exp(D)
        coef = w * (ds + 0.5 * D * D * eD) + tiny / L
        X = (v64[None, :, :] - o[:, None, :]).abs()
        b = eD * (Tq + torch.bmm(coef[:, None, :], X)[:, 0, :])
        b = b + u * o.abs() + (nk + 16) * U32 * (w @ v64.abs() + o.abs()) + 2 * U32 * o.abs()
        b = b + 0.5 * ulp(o.abs() + b, dt)
        o_all.append(o)
        b_all.append(b)
    return torch.cat(o_all), torch.cat(b_all)


# ------------------------------------------------------------------------------------------------ GEMM and convolution
ACC_ULPS = 1.0            # fp32 roundings allowed per accumulated product, in units of U32 (see gemm_ref_and_bound)
GELU_AS_ABS = 7.5e-8      # |error| of Phi from Abramowitz & Stegun 7.1.26 (csrc/common.hpp, gelu_erf_f)


def unit_roundoff(dt):
    return 2.0 ** -(MANT[dt][0] + 1)


def _pre_and_e32(S, A, K, terms, splits):
    """``pre`` and the fp32 part of the bound from the fp64 sum of products S, the sum of their magnitudes A and the epilogue's
    fp64 addends (absent ones left out)."""
    pre, mag = S.clone(), S.abs()
    for t in terms:
        pre = pre + t
        mag = mag + t.abs()
    e32 = (K + 8) * ACC_ULPS * U32 * A + 3 * U32 * (mag + pre.abs())
    if splits > 1:
        e32 = e32 + (splits + 1) * U32 * A
    return pre, e32


def _rounded(pre, e32, dt, out_f32):
    return e32 + (U32 * pre.abs() if out_f32 else 0.5 * ulp(pre.abs() + e32, dt))


def gelu64(g):
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


def _geglu(pre, e32, dt):
    """out = val gelu(gate) from the two halves of ``pre`` (value columns first), both carrying ``e32``.  With e_v, e_g the two
    halves of e32: |gelu(g + d) - gelu(g)| <= |gelu'(g)| |d| + 0.4 d^2 (gelu'' = phi(g) (2 - g^2), at most 2 phi(0) = 0.798 in
    magnitude), gelu_erf_f differs from gelu by |g| (7.5e-8 + 8 U32) (Phi's absolute error, plus v_rcp, v_exp and the ten fused
    multiply-adds, each relative to a quantity of at most 1/2), then one fp32 product and the rounding."""
    no = pre.shape[1] // 2
    val, g, ev, eg = pre[:, :no], pre[:, no:], e32[:, :no], e32[:, no:]
    phi = torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    d1 = 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0))) + g * phi
    out = val * gelu64(g)
    dgelu = d1.abs() * eg + 0.4 * eg * eg + (g.abs() + eg) * (GELU_AS_ABS + 8 * U32)
    b = (val.abs() + ev) * dgelu + ev * gelu64(g).abs() + 2 * U32 * out.abs()
    return out, b + 0.5 * ulp(out.abs() + b, dt)


def gemm_ref_and_bound(a, w, dt, *, bias=None, rowbias=None, rows_per_sample=1, residual=None, out_f32=False, splits=1, geglu=False,
                       a_err=None):
    """``vface_gemm`` in fp64 and what a correct kernel may differ by, per element.  ``a [M, K]`` (for the dual-source form: the two
    sources side by side), ``w [N, K]``: the 16-bit operands; ``bias [N]``, ``rowbias [M / rows_per_sample, N]`` fp32; ``residual
    [M, N]`` 16-bit or fp32.  ``geglu``: ``w`` and ``bias`` in the module's order (value rows, then gate rows); the result has N / 2
    columns.  Returns ``(ref, bound)``, fp64.  With u the unit roundoff of ``dt``, S = sum_k a w and A = sum_k |a| |w|:

      pre   = S + bias + rowbias + residual
      e32   = (K + 8) U32 A + 3 U32 (|S| + |bias| + |rowbias| + |residual| + |pre|)  [+ (splits + 1) U32 A]
      bound = e32 + 0.5 ulp(|pre| + e32, dt)          16-bit output
      bound = e32 + U32 |pre|                         fp32 output (``out_f32``: VFACE_EPI_OUT_F32 and the out32 carrier)

    * (K + 8) U32 A: the products of two 16-bit values are exact in fp32; K of them summed in fp32 in ANY order (within a
      v_mfma_f32_16x16x32, across its 32-deep steps, across K tiles) are off by at most (K - 1) U32 A to first order; + 8 covers the
      second order up to K = 2^16 and whatever the instruction's internal alignment drops -- the term attention_ref_and_bound uses
      for the same instruction.  ACC_ULPS = 1 is this reading: one HALF fp32 ulp (U32) per addition.
    * 3 U32 (...): the epilogue adds (acc + bias) + rowbias, + residual in fp32, each at most U32 of its result, a result never
      larger than the sum of the magnitudes it was made from; absent addends add nothing.
    * split-K: the partial sums are fp32 and are added in order, then the epilogue as before: (splits + 1) U32 A more.
    * ``a_err`` (fp64 [M, N], optional): what the operands themselves may be off by, already multiplied through |w| -- the
      convolutions' fused input normalisation passes it (conv_ref_and_bound).
    * one rounding to ``dt`` at the largest magnitude the bound admits; the fp32 forms store the sum itself (U32 |pre| stands for
      the third epilogue add where the residual is absent, and for nothing else)."""
    a64, w64 = a.double(), w.double()
    K = a64.shape[1]
    S, A = a64 @ w64.T, a64.abs() @ w64.abs().T
    terms = []
    if bias is not None:
        terms.append(bias.double()[None, :].expand_as(S))
    if rowbias is not None:
        terms.append(rowbias.double().repeat_interleave(rows_per_sample, 0)[:S.shape[0]])
    if residual is not None:
        terms.append(residual.double())
    pre, e32 = _pre_and_e32(S, A, K, terms, splits)
    if a_err is not None:
        e32 = e32 + a_err
    if geglu:
        assert residual is None and rowbias is None and not out_f32
        return _geglu(pre, e32, dt)
    return pre, _rounded(pre, e32, dt, out_f32)


def conv_windows(x64, KH, KW, stride, upsample, pad):
    """``x64 [nimg, C, H, W]`` -> ``(cols [nimg * OH * OW, KH * KW * C] in (tap, channel) order, OH, OW)``: nearest x2 upsampling
    first if asked, zero padding ``pad`` = (top, bottom, left, right)."""
    if upsample:
        x64 = x64.repeat_interleave(2, 2).repeat_interleave(2, 3)
    pt, pb, pl, pr = pad
    xp = F.pad(x64, (pl, pr, pt, pb))
    nimg, C, HP, WP = xp.shape
    OH, OW = (HP - KH) // stride + 1, (WP - KW) // stride + 1
    cols = F.unfold(xp, (KH, KW), stride=stride)                                  # [nimg, C * KH * KW, OH * OW], (channel, tap)
    cols = cols.reshape(nimg, C, KH * KW, OH * OW).permute(0, 3, 2, 1).reshape(nimg * OH * OW, KH * KW * C)
    return cols, OH, OW


def conv_ref_and_bound(x, w, dt, *, stride=1, upsample=False, pad=(1, 1, 1, 1), bias=None, rowbias=None, residual=None, x2=None,
                       w2=None, scale_shift=None, silu=False, out_f32=False, splits=1):
    """``vface_conv3x3`` / ``vface_conv3x3_plus_1x1`` / one ``vface_upsample2x_conv3x3_phase`` in fp64 with the per-element bound of
    gemm_ref_and_bound: the same form with K = taps Cin + C2 and A the same convolution of |x| with |w|.  ``x [nimg, Cin, H, W]``,
    ``w [Cout, Cin, KH, KW]`` 16-bit (a phase: its 2 x 2 pre-summed kernel AS ROUNDED to ``dt``, ``pad`` = (1 - py, py, 1 - px, px));
    ``pad`` = (0, 1, 0, 1) is VFACE_CONV_PAD_TRAILING; ``x2 [M, C2]``, ``w2 [Cout, C2]``: the fused 1x1 shortcut; ``rowbias [nimg,
    Cout]``; ``residual [M, Cout]``.  Returns ``([M = nimg OH OW, Cout], bound)`` in NHWC row order.

    ``scale_shift [nimg, Cin, 2]`` fp32 (+ ``silu``): the fused GroupNorm input.  The reference operand is o = act(x a + b) in fp64,
    zero padding applied AFTER it; the kernel's is round_dt(act32(x a + b)), off by at most
      d = u |o| + r |o| + 2 U32 (|x a| + |b|) |act'(x a + b)|
    (the rounding to ``dt``; r = cpu_fp32_rel_error of the SiLU on the case's own arguments, 0 without it; the fp32 product and sum
    in front of it through the activation's slope), and sum |w| d goes into the bound (``a_err``), with A taken from |o| + d."""
    x64, w64 = x.double(), w.double()
    nimg, cin = x64.shape[:2]
    cout, _, KH, KW = w64.shape
    d = None
    if scale_shift is not None:
        ab = scale_shift.double()
        a_, b_ = ab[:, :, 0][:, :, None, None], ab[:, :, 1][:, :, None, None]
        t = x64 * a_ + b_
        if silu:
            sg = torch.sigmoid(t)
            o, slope = t * sg, (sg * (1.0 + t * (1.0 - sg))).abs()
            r = cpu_fp32_rel_error(F.silu, (x.float() * scale_shift[:, :, 0][:, :, None, None] + scale_shift[:, :, 1][:, :, None, None]))
        else:
            o, slope, r = t, torch.ones_like(t), 0.0
        d = (unit_roundoff(dt) + r) * o.abs() + 2 * U32 * ((x64 * a_).abs() + b_.abs()) * slope
        x64 = o
    cols, OH, OW = conv_windows(x64, KH, KW, stride, upsample, pad)
    wk = w64.permute(0, 2, 3, 1).reshape(cout, KH * KW * cin)
    a_err = None
    if d is not None:
        dcols, _, _ = conv_windows(d, KH, KW, stride, upsample, pad)
        a_err = dcols @ wk.abs().T
        acols = cols.abs() + dcols
    else:
        acols = cols.abs()
    if x2 is not None:
        cols, acols, wk = torch.cat([cols, x2.double()], 1), torch.cat([acols, x2.double().abs()], 1), torch.cat([wk, w2.double()], 1)
    K = cols.shape[1]
    S, A = cols @ wk.T, acols @ wk.abs().T
    terms = []
    if bias is not None:
        terms.append(bias.double()[None, :].expand_as(S))
    if rowbias is not None:
        terms.append(rowbias.double().repeat_interleave(OH * OW, 0))
    if residual is not None:
        terms.append(residual.double())
    pre, e32 = _pre_and_e32(S, A, K, terms, splits)
    if a_err is not None:
        e32 = e32 + a_err
    return pre, _rounded(pre, e32, dt, out_f32)


def colstats_ref_and_bound(stored, slice_rows):
    """The (sum, sum of squares) a producer's epilogue leaves per statistics slice and output column.  ``stored [M, N]``: the values
    as stored (read back from the device: the 16-bit output, or the fp32 carrier where there is one); ``slice_rows``: one index
    tensor of rows per slice.  Returns ``(ref [slices, N, 2], bound)`` fp64: fp32 sums of ``rows`` terms in any order, the squares
    rounded (or fused) in fp32 -- (rows + 4) U32 sum |v| and (rows + 4) U32 sum v^2."""
    v = stored.double()
    ref, bound = [], []
    for rows in slice_rows:
        s = v[rows]
        k = (len(rows) + 4) * U32
        ref.append(torch.stack([s.sum(0), (s * s).sum(0)], -1))
        bound.append(torch.stack([k * s.abs().sum(0), k * (s * s).sum(0)], -1))
    return torch.stack(ref), torch.stack(bound)
