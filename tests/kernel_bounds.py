"""Helpers of the per-kernel GPU tests (test_kernels_gpu.py, test_glue_kernels_gpu.py, test_attention_gpu.py,
test_attention_shared_gpu.py, test_gemm_conv_gpu.py, test_transformer_kernels_gpu.py, test_hook_sampler_kernels_gpu.py): seeded 16-bit inputs, the unit in the last place of a 16-bit type, sentinel-filled buffers and the
``Framed`` output view / ``strided`` input view that show a store outside a kernel's slot or a leading dimension mistaken for a
width, the element-wise bound check that names the worst element, and the fp64 references with their per-element bounds: the
attention kernel's (``attention_ref_and_bound``), the GEMM family's with its epilogues, split-K and GEGLU (``gemm_ref_and_bound``),
the convolutions' (``conv_ref_and_bound``), the column statistics' (``colstats_ref_and_bound``), LayerNorm's
(``layernorm_ref_and_bound``), the GroupNorm family's (``gn_stats_ref_and_bound`` from pixels with the conditioning term of the
one-pass sums, ``gn_cols_ref_and_bound`` from column sums, ``gn_apply_ref_and_bound`` from the device's statistics),
``linear_small_ref_and_bound``, and the fused chains' stage by stage (``st_front_t0_`` / ``st_front_qkv_ref_and_bound``,
``ffn_ref_and_bound`` for PLAIN / PRE / POST) with ``round_operand`` for a value rounded once as the next operand, and the hook and
sampler kernels' (``flow_warp_`` / ``flow_to_latent_`` / ``ddim_step_`` / ``timestep_embedding_ref_and_bound``), the flow
producer's and the face parser's glue kernels' (``pooled_linear_`` / ``channel_gate_ref_and_bound``).  Every bound is
built from fp64 quantities of the reference alone; test_attention_bound_cpu.py, test_gemm_bound_cpu.py,
test_transformer_bound_cpu.py and test_hook_bound_cpu.py show that each admits a model of the kernel's rounding points and refuses one-line defects of it.
Plain functions, nothing collected by pytest."""
import math

import torch
import torch.nn.functional as F

DEV = "cuda"
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


class Framed:
    """A ``[rows, cols]`` view inside a sentinel buffer (``lead`` extra trailing dimension for the statistics' pairs)."""

    def __init__(self, rows, cols, dt, pair=False):
        self.rows, self.cols, self.ld, self.pair = rows, cols, cols + 24, pair
        k = 2 if pair else 1
        self.keep = sentinel(rows + 3, self.ld * k, dt)
        self.dev = self.keep.to(DEV)

    def _v(self, t):
        if self.pair:
            return t.view(self.rows + 3, self.ld, 2)[1:1 + self.rows, 8:8 + self.cols]
        return t[1:1 + self.rows, 8:8 + self.cols]

    @property
    def view(self):
        return self._v(self.dev)

    @property
    def stats_arg(self):
        """what ``hip.gemm(colstats=...)`` takes: its ``stride(0) // 2`` is the leading dimension"""
        return self.dev.view(self.rows + 3, self.ld, 2)[1:, 8:]

    def result(self, what, rows=None):
        """The view's content on the CPU, after the check that nothing outside it (or outside ``rows`` of it) changed."""
        torch.cuda.synchronize()
        allv = self.dev.cpu()
        got = self._v(allv).clone()
        expect = self.keep.clone()
        if rows is None:
            self._v(expect).copy_(got)
        else:
            self._v(expect)[rows] = got[rows]
        assert same_bits(allv, expect), f"{what}: a store outside the output view"
        self.keep = expect
        return got


def strided(x, off):
    """``x [rows, cols]`` on the device as a view ``off`` columns into a buffer ``2 off`` wider (the rest NaN)."""
    buf = torch.full((x.shape[0], x.shape[1] + 2 * off), float("nan"), dtype=x.dtype)
    buf[:, off:off + x.shape[1]] = x
    return buf.to(DEV)[:, off:off + x.shape[1]]


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


WORST = {}                                         # family -> worst err / bound seen (printed; a record of headroom, no threshold)


def note(family, err, bound):
    """Print and keep the worst error / bound of a family: a record of headroom, never a threshold."""
    r = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), r)
    print(f"[headroom] {family}: worst err / bound {r:.3f} (so far {WORST[family]:.3f})")
    return r


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


def softmax_rows_ref_and_bound(S, scale, dt):
    """``vface_softmax_rows``: P = softmax(S scale) over the columns of the fp32 ``S [M, N]`` in fp64, and its per-element bound
    (test_glue_kernels_gpu.py::test_softmax_rows, test_vae_stages_gpu.py).  Relative to p: the exponent of 2 is fma(s, c, -max c)
    with c = fl(scale log2 e): c is off by 2 u relative and each of the two terms rounds once, so the argument is off by 4 u A,
    A = max|s| scale log2 e, for numerator and denominator alike: 8 ln2 u A; the row sum is 16 + 8 + 3 fp32 sums, the reciprocal and
    the product 2 more; E = ``cpu_fp32_rel_error`` of torch's fp32 softmax on these rows for the exp2.  Then 0.5 ulp of the type,
    and 2^-126 for a flushed intermediate."""
    lg = S.double() * scale
    ref = torch.softmax(lg, 1)
    E = cpu_fp32_rel_error(torch.softmax, S * scale, dim=1)
    A = lg.abs().amax(1, keepdim=True) * 1.4426950408889634
    return ref, (E + (8 * math.log(2) * A + 29) * U32) * ref + 0.5 * ulp(ref, dt) + TINY32


# ------------------------------------------------------------------------------------------------ GEMM and convolution
ACC_ULPS = 1.0           # fp32 roundings allowed per accumulated product, in units of U32 (see gemm_ref_and_bound)
GELU_AS_ABS = 7.5e-8      # |error| of Phi from Abramowitz & Stegun 7.1.26 (csrc/common.hpp, gelu_erf_f)


def unit_roundoff(dt):
    return 2.0 ** -(MANT[dt][0] + 1)


def _pre_and_e32(S, A, K, terms, splits, init=None, init_mag=None):
    """``pre`` and the fp32 part of the bound from the fp64 sum of products S, the sum of their magnitudes A and the epilogue's
    fp64 addends (absent ones left out).  ``init``: the accumulator's initial value -- one more term of the sum, carried through
    all K additions, so its magnitude (``init_mag``, default |init|) joins A."""
    if init is not None:
        S, A = S + init, A + (init.abs() if init_mag is None else init_mag)
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


def _geglu(pre, e32, dt, rounded=True):
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
    return out, (b + 0.5 * ulp(out.abs() + b, dt) if rounded else b)


def gemm_ref_and_bound(a, w, dt, *, bias=None, rowbias=None, rows_per_sample=1, residual=None, out_f32=False, splits=1, geglu=False,
                       a_err=None, init=None, init_mag=None, rounded=True):
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
    * ``init`` (fp64 [M, N], optional; ``init_mag`` its magnitude where the kernel carries more than |init|): what the accumulator
      starts from where a fused kernel loads a residual or a bias straight into it -- a term of the sum like the products.
    * one rounding to ``dt`` at the largest magnitude the bound admits; the fp32 forms store the sum itself (U32 |pre| stands for
      the third epilogue add where the residual is absent, and for nothing else).  ``rounded=False`` (GEGLU only): without the
      final rounding -- the fused chains round the hidden activations as the next operand (``round_operand``)."""
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
    pre, e32 = _pre_and_e32(S, A, K, terms, splits, init, init_mag)
    if a_err is not None:
        e32 = e32 + a_err
    if geglu:
        assert residual is None and rowbias is None and not out_f32
        return _geglu(pre, e32, dt, rounded)
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


# ------------------------------------------------------------------------------------------------ norms and the fused transformer chains
U64 = 2.0 ** -53          # fp64 unit roundoff (the GroupNorm folds)
GN_PIX = 128              # pixels per workgroup of gn_partial_kernel (csrc/pointwise.hip)


def as_16bit(ref64, e32, dt):
    """The bound of a 16-bit output whose fp32 value is within ``e32`` of ``ref64``: one rounding at the largest magnitude admitted."""
    return e32 + 0.5 * ulp(ref64.abs() + e32, dt)


def round_operand(o64, e, dt):
    """A value rounded to ``dt`` ONCE as the next GEMM's operand, the rounding modelled as EXACT except near a tie.  ``o64``: the
    fp64 value, ``e``: what the kernel's fp32 value may differ from it by.  Returns ``(r, d)``: r = o64 rounded to nearest even in
    ``dt`` (computed in fp64 on the type's own grid, no double rounding) and d = what the kernel's operand may differ from r by:
    0 where no rounding tie of ``dt`` lies within e of o64 (both round to the same value), q + e otherwise (q the spacing of ``dt``
    at |o64| + e: a tie between the two values moves the result by one spacing, several of them by no more than e + q).
    This is what makes a stage behind a rounding as tight as the stage itself: the alternative u |o| (every operand off by half a
    spacing) is the size of the rounding, which the reference can reproduce, not of the kernel's error, which it cannot."""
    q = ulp(o64.abs() + e, dt)
    t = o64 / q
    r = torch.round(t) * q                                           # round half to even, exact: q is a power of two
    tie = ((t - torch.floor(t)) - 0.5).abs() * q
    return r, torch.where(tie <= e, q + e, torch.zeros_like(o64))


def _rsqrt_interval(var, dvar, eps):
    """rstd = (var + eps)^-1/2 and how far a variance within ``dvar`` of ``var`` -- clamped at 0 as the kernels do -- moves it."""
    r = 1.0 / torch.sqrt(var + eps)
    lo = 1.0 / torch.sqrt(var + dvar + eps)
    hi = 1.0 / torch.sqrt(torch.clamp(var - dvar, min=0.0) + eps)
    return r, torch.maximum(hi - r, r - lo)


def layernorm_ref_and_bound(x, gamma, beta, eps, dt, x_err=None, rounded=True):
    """``vface_layernorm`` (and the LayerNorm stage of stfront.hip / ffn.hip: the same two passes on the fp32 tile) in fp64 and what
    a correct kernel may differ by, per element.  ``x [M, C]`` 16-bit or fp32, ``gamma, beta [C]`` fp32.  Returns ``(y, bound)``.
    With d = x - mean, var = mean(d^2), rstd = (var + eps)^-1/2, t = d rstd gamma, y = t + beta and m1 = mean |x|:

      dmu   = (C + 2) U32 m1                        the fp32 sum of C terms in any order ((C - 1) U32 sum |x|), the division
      dvar  = dmu^2 + (C + 8) U32 var + U32 (var + eps)
              -- a constant shift of every d_i by dmu leaves sum d_i^2 unchanged to FIRST order (sum d = 0): the mean's error
              enters the variance squared; the subtraction's own rounding U32 |d_i| twice, the C squares and their fp32 sum
              (C + 3) U32 var, the division and the addition of eps
      drstd = what dvar moves rstd by (interval, no linearisation: a constant row has var = 0) + r rstd,
              r = cpu_fp32_rel_error(rsqrt) on the case's own var + eps
      e32   = rstd |gamma| (dmu + U32 |d|) + |gamma d| drstd + 2 U32 |t| + U32 (|t| + |beta|)
              -- THE MEAN'S ERROR ENTERS THROUGH rstd |gamma|: a constant row of value v has rstd = eps^-1/2 = 316 and gets
              316 |gamma| (C + 2) U32 |v|, the wide bound it deserves; two products and the sum (or its fused form)
      bound = e32 + 0.5 ulp(|y| + e32, dt)          one rounding (``rounded=False``: e32 alone, for ``round_operand``)

    ``x_err`` (fp64 [M, C], optional): what the INPUT may be off by (a fused kernel normalising its own accumulator tile).  To
    first order dy_i = rstd gamma_i (dx_i - mean(dx) - xh_i mean(xh dx)), xh = d rstd, so
      e32 += rstd |gamma_i| (x_err_i + mean(x_err) + |xh_i| mean(|xh| x_err))."""
    x64, g64, b64 = x.double(), gamma.double()[None, :], beta.double()[None, :]
    C = x64.shape[1]
    mu = x64.mean(1, keepdim=True)
    d = x64 - mu
    var = (d * d).mean(1, keepdim=True)
    dmu = (C + 2) * U32 * x64.abs().mean(1, keepdim=True)
    dvar = dmu * dmu + (C + 8) * U32 * var + U32 * (var + eps)
    rstd, drstd = _rsqrt_interval(var, dvar, eps)
    drstd = drstd + cpu_fp32_rel_error(torch.rsqrt, (var + eps).float()) * rstd
    t = d * rstd * g64
    y = t + b64
    e32 = rstd * g64.abs() * (dmu + U32 * d.abs()) + (g64 * d).abs() * drstd + 2 * U32 * t.abs() + U32 * (t.abs() + b64.abs())
    if x_err is not None:
        xh = (d * rstd).abs()
        e32 = e32 + rstd * g64.abs() * (x_err + x_err.mean(1, keepdim=True) + xh * (xh * x_err).mean(1, keepdim=True))
    return y, (as_16bit(y, e32, dt) if rounded else e32)


def gn_sum_depth(C, groups, hw):
    """How many fp32 additions one term passes through in gn_partial_kernel: a thread's pixel loop (ceil(min(hw, 128) / PP) terms,
    PP = 256 / min(C / 8, 256) pixel lanes), the PP lanes in order, the C / groups channels of the group in order."""
    pp = 256 // min(C // 8, 256)
    return -(-min(hw, GN_PIX) // pp) + pp + C // groups


def gn_stats_ref_and_bound(x, groups, eps):
    """``vface_groupnorm_stats`` from the pixels in fp64 and its per-element bound.  ``x [nimg, hw, C]`` 16-bit or fp32.  Returns
    ``(stats [nimg, groups, 2] = (mean, rstd), bound)``.  The kernel sums x and x^2 in fp32 per thread, per pixel lane and per
    group (D = gn_sum_depth additions on the way of any term: D U32 sum |x|, (D + 1) U32 sum x^2 with the squares' own
    rounding), folds the 128-pixel chunks in fp64 and forms var = E[x^2] - mean^2 in fp64.  With m = mean, v = var:

      dmean = (D + 2) U32 mean |x|
      dvar  = 3 (D + 3) U32 (m^2 + v) + dmean^2 = 3 (D + 3) U32 v * [(m^2 + v) / v] + dmean^2
              -- dE2 <= (D + 3) U32 (m^2 + v) and 2 |m| dmean <= 2 (D + 2) U32 (m^2 + v) since |m| mean |x| <= E[x^2] = m^2 + v:
              the CONDITIONING TERM (m^2 + v) / v of the one-pass form is explicit here, it is what the algorithm implies (at
              mean / spread 16 it is 257), not a property of a particular kernel
      mean:  dmean + U32 |m|                       (the rounding of the fp64 mean to fp32)
      rstd:  what dvar moves (v + eps)^-1/2 by, the clamp of the variance at 0 included, + 2 U32 rstd"""
    nimg, hw, C = x.shape
    cpg = C // groups
    x64 = x.double().reshape(nimg, hw, groups, cpg)
    m = x64.mean((1, 3))
    v = ((x64 - m[:, None, :, None]) ** 2).mean((1, 3))
    D = gn_sum_depth(C, groups, hw)
    dmean = (D + 2) * U32 * x64.abs().mean((1, 3))
    dvar = 3 * (D + 3) * U32 * (m * m + v) + dmean * dmean
    rstd, drstd = _rsqrt_interval(v, dvar, eps)
    return torch.stack([m, rstd], -1), torch.stack([dmean + U32 * m.abs(), drstd + 2 * U32 * rstd], -1)


def gn_cols_ref_and_bound(cs, nimg, hw, groups, eps, gamma=None, beta=None):
    """``vface_groupnorm_finalize_cols`` / ``_coeffs_from_cols`` in fp64 from the very column sums ``cs [nimg hw / 64, C, 2]`` the
    kernel reads.  The fold is fp64 (n = cpg hw / 64 terms), so what is left is the fold's own error and THE FINAL ROUNDING to fp32:
      mean: (n + 2) U64 mean |s| + U32 |m|
      var  = max(E2 - m^2, 0) exactly as the kernel forms and clamps it; dvar = (n + 4) U64 (E2 + m^2) -- a group whose fp32
             sums give a slightly negative variance is clamped in the reference too, and the clamp is continuous
      rstd: what dvar moves it by + 4 U64 rstd + U32 rstd
    With ``gamma, beta``: also ``(ab [nimg, C, 2], bound)`` of a = rstd32 gamma, b = beta - mean32 a in fp32:
      da = |gamma| drstd + U32 |a|;  db = |m| da + |a| dmean + 2 U32 |m a| + U32 |beta|.
    Returns ``(stats, stats_bound)`` or ``(stats, stats_bound, ab, ab_bound)``."""
    C = cs.shape[1]
    cpg, spi = C // groups, hw // 64
    c64 = cs.double().reshape(nimg, spi, groups, cpg, 2)
    n, count = cpg * spi, float(hw * cpg)
    m = c64[..., 0].sum((1, 3)) / count
    E2 = c64[..., 1].sum((1, 3)) / count
    v = torch.clamp(E2 - m * m, min=0.0)
    dmean = (n + 2) * U64 * c64[..., 0].abs().sum((1, 3)) / count
    dvar = (n + 4) * U64 * (E2.abs() + m * m)
    rstd, drstd = _rsqrt_interval(v, dvar, eps)
    drstd = drstd + (4 * U64 + U32) * rstd
    dmean = dmean + U32 * m.abs()
    out = (torch.stack([m, rstd], -1), torch.stack([dmean, drstd], -1))
    if gamma is None:
        return out
    g64, b64 = gamma.double()[None, :], beta.double()[None, :]
    rep = lambda t: t.repeat_interleave(cpg, 1)
    a = rep(rstd) * g64
    b = b64 - rep(m) * a
    da = g64.abs() * rep(drstd) + U32 * a.abs()
    db = rep(m).abs() * da + a.abs() * rep(dmean) + 2 * U32 * (rep(m) * a).abs() + U32 * b64.abs()
    return out + (torch.stack([a, b], -1), torch.stack([da, db], -1))


def scale_shift_act(x, a, b, silu):
    """o = act(x a + b) in fp64 and the fp32 error of it: ``(o, e)`` with e = 2 U32 (|x a| + |b|) |act'| + r |o| -- the product and
    the sum (or their fused form) through the activation's slope, r = cpu_fp32_rel_error of the SiLU on the case's own arguments."""
    x64, a64, b64 = x.double(), a.double(), b.double()
    t = x64 * a64 + b64
    e = 2 * U32 * ((x64 * a64).abs() + b64.abs())
    if not silu:
        return t, e
    sg = torch.sigmoid(t)
    o = t * sg
    r = cpu_fp32_rel_error(F.silu, (x.float() * a.float() + b.float()))
    return o, e * (sg * (1.0 + t * (1.0 - sg))).abs() + r * o.abs() + 0.4 * e * e


def gn_apply_ref_and_bound(x, stats, gamma, beta, groups, silu, dt):
    """``vface_groupnorm_apply`` in fp64 FROM THE STATISTICS AS READ BACK FROM THE DEVICE (``stats [nimg, groups, 2]`` fp32), so
    the bound holds no statistics error: a = rstd gamma and b = beta - mean a formed in fp32 (da = U32 |a|, db = |mean| da +
    2 U32 (|beta| + |mean a|)), the multiply-add x a + b (|x| da + db + ``scale_shift_act``'s 2 U32 (|x a| + |b|)), the SiLU
    allowance, one rounding.  ``x [nimg, hw, C]``.  Returns ``(y [nimg, hw, C], bound)``."""
    nimg, hw, C = x.shape
    cpg = C // groups
    st = stats.double()
    mean, rstd = st[..., 0].repeat_interleave(cpg, 1)[:, None, :], st[..., 1].repeat_interleave(cpg, 1)[:, None, :]
    g64, b64 = gamma.double()[None, None, :], beta.double()[None, None, :]
    a = rstd * g64
    b = b64 - mean * a
    da = U32 * a.abs()
    db = mean.abs() * da + 2 * U32 * (b64.abs() + (mean * a).abs())
    o, e = scale_shift_act(x, a.expand(nimg, hw, C), b.expand(nimg, hw, C), silu)
    slope = 1.1 if silu else 1.0                                      # |SiLU'| <= 1.1
    e = e + slope * (x.double().abs() * da + db)
    return o, as_16bit(o, e, dt)


def linear_small_ref_and_bound(a, w, dt, bias=None, silu=False, out_f32=False):
    """``vface_linear_small`` in fp64: ``gemm_ref_and_bound`` with FOUR partial sums (the four waves' quarters of K meet in LDS in
    a fixed order: ``splits=4``), then the SiLU on the fp32 sum through its slope (|SiLU'| <= 1.1, r = cpu_fp32_rel_error), then
    one rounding -- to ``dt``, or to fp32."""
    pre, e = gemm_ref_and_bound(a, w, dt, bias=bias, out_f32=True, splits=4)
    if silu:
        sg = torch.sigmoid(pre)
        r = cpu_fp32_rel_error(F.silu, pre.float())
        o = pre * sg
        e = (sg * (1.0 + pre * (1.0 - sg))).abs() * e + 0.4 * e * e + r * o.abs()
        pre = o
    return pre, (e + U32 * pre.abs() if out_f32 else as_16bit(pre, e, dt))


def st_front_t0_ref_and_bound(x32, ab, hw, w_in, b_in, dt):
    """Stage 1 of ``vface_st_front``: t0 = round_dt(x a[img] + b[img]) @ W_in^T + b_in in fp64 from x32 and THE DEVICE's ``ab
    [nimg, C, 2]``.  The GroupNorm'd operand is rounded by ``round_operand`` (exact except within the multiply-add's 2 U32 (|x a| +
    |b|) of a tie): with u |o| instead the bound would be 100x the fp32 stage's own and a tile that takes another image's (a, b)
    on images that differ little would pass.  b_in is the accumulator's initial value (``init``).  Returns ``(t0, bound)``, fp32 form."""
    abd = ab.double()
    a, b = abd[..., 0].repeat_interleave(hw, 0), abd[..., 1].repeat_interleave(hw, 0)
    o, e = scale_shift_act(x32, a.float(), b.float(), False)
    r, d = round_operand(o, e, dt)
    return gemm_ref_and_bound(r, w_in, dt, out_f32=True, a_err=d @ w_in.double().abs().T, init=b_in.double()[None, :].expand(r.shape[0], -1))


def st_front_qkv_ref_and_bound(t0, gamma, beta, eps, w_p, dt, ln=None):
    """Stages 2 and 3 of ``vface_st_front`` from the device's ``t0`` (fp32): ``(ln_ref, ln_bound, qkv_ref, qkv_bound)``.  ln: the
    LayerNorm bound on the device's t0.  qkv: with the device's ``ln`` bits, ``gemm_ref_and_bound`` on them (an exact operand);
    without, the fp64 LayerNorm rounded by ``round_operand`` (exact except within the LayerNorm's fp32 error of a tie), its d
    pushed through |W_p| -- u |ln| instead would hide unpermuted k columns of W_p behind sum |ln| |w| u wherever gamma is flat."""
    y, e = layernorm_ref_and_bound(t0, gamma, beta, eps, dt, rounded=False)
    if ln is not None:
        q, qb = gemm_ref_and_bound(ln, w_p, dt)
    else:
        r, d = round_operand(y, e, dt)
        q, qb = gemm_ref_and_bound(r, w_p, dt, a_err=d @ w_p.double().abs().T)
    return y, as_16bit(y, e, dt), q, qb


def ffn_ref_and_bound(dt, *, gamma, beta, eps, w1, b1, w2, b2, x32=None, att=None, wo=None, bo=None, rowbias=None, rows_per_sample=1,
                      resid=None, wpo=None, b_po=None, x_in=None, t3_from=None):
    """The three forms of csrc/ffn.hip in fp64, stage by stage, none of the intermediates being exposed: ``(out, e)`` -- PLAIN
    (``x32``) and PRE (``att, wo, bo, resid`` [+ ``rowbias``]) -- or ``(y, e)`` -- POST (+ ``wpo, b_po, x_in``); e is the fp32
    form (what ``out32`` may differ by; ``as_16bit`` for a 16-bit-only output).  Weights in the MODULE's order (``w1``: value rows,
    then gate rows; no packing).
      t1  = x32                                             PLAIN: exact
          = att Wo^T + bo + rowbias + resid                 PRE: gemm bound, fp32 form, resid the accumulator's initial value (e1)
      ln  = LayerNorm(t1)                                   layernorm bound with x_err = e1, then ``round_operand``
      h   = val gelu(gate), [val; gate] = W1 ln + b1        gemm bound with GEGLU, a_err = d_ln |W1|^T, then ``round_operand``
      out = W2 h + b2 + t1                                  gemm bound, fp32 form, a_err = d_h |W2|^T + e1; PLAIN: t1 an epilogue
                                                            addend; PRE: t1 INSIDE the accumulator through all 4C additions
                                                            (``init``, magnitude |resid| + |att| |Wo|^T + |bo + rowbias|)
      t3  = round(out); y = Wpo t3 + b_po + x_in            POST: ``round_operand``, gemm bound with ``init`` = x_in
    ``t3_from`` (fp32 [M, C], POST only): ``out32`` of the PRE form launched on the same inputs -- the sibling kernel EXPOSES the
    intermediate, its accumulator and its (b2 + bo + rowbias) addend are formed by the same operations, so t3 is that value rounded
    once, exact except within 4 U32 |out| of a tie; y is then one GEMM stage with a bound as tight as a stage's.  Without it the
    chain's bound on y carries every upstream rounding tie through |W2| and |Wpo| and is 10x to 100x wider.
    Every 16-bit rounding is ``round_operand`` (exact except within the stage's own fp32 error of a tie): the defects this chain
    must refuse -- the residual added after the rounding, t1 rounded before the LayerNorm, a workgroup's row bias taken from sample
    0 where row biases differ little -- are OF THE SIZE u |o|, so a bound that granted u |o| per operand could not see them."""
    if t3_from is not None:
        o32 = t3_from.double()
        t3, d_t3 = round_operand(o32, 4 * U32 * o32.abs(), dt)
        return gemm_ref_and_bound(t3, wpo, dt, bias=b_po, out_f32=True, a_err=d_t3 @ wpo.double().abs().T, init=x_in.double())
    if att is None:
        t1, e1, init = x32.double(), None, {}
    else:
        rb = None if rowbias is None else rowbias
        t1, e1 = gemm_ref_and_bound(att, wo, dt, bias=bo, rowbias=rb, rows_per_sample=rows_per_sample, out_f32=True, init=resid.double())
        mag = resid.double().abs() + att.double().abs() @ wo.double().abs().T + (t1 - resid.double() - att.double() @ wo.double().T).abs()
        init = dict(init=t1, init_mag=mag)
    ln, e_ln = layernorm_ref_and_bound(t1, gamma, beta, eps, dt, x_err=e1, rounded=False)
    ln_r, d_ln = round_operand(ln, e_ln, dt)
    h, e_h = gemm_ref_and_bound(ln_r, w1, dt, bias=b1, geglu=True, a_err=d_ln @ w1.double().abs().T, rounded=False)
    h_r, d_h = round_operand(h, e_h, dt)
    a_err = d_h @ w2.double().abs().T + (e1 if e1 is not None else 0.0)
    if att is None:
        out, e_out = gemm_ref_and_bound(h_r, w2, dt, bias=b2, residual=t1, out_f32=True, a_err=a_err)
    else:
        out, e_out = gemm_ref_and_bound(h_r, w2, dt, bias=b2, out_f32=True, a_err=a_err, **init)
    if wpo is None:
        return out, e_out
    t3, d_t3 = round_operand(out, e_out, dt)
    return gemm_ref_and_bound(t3, wpo, dt, bias=b_po, out_f32=True, a_err=d_t3 @ wpo.double().abs().T, init=x_in.double())


# ------------------------------------------------------------------------------------------------ flow warp, flow resample, DDIM step, timestep embedding
COORD_ULPS = 8.0          # fp32 roundings between a flow value and its un-normalised coordinate, in units of U32 (size - 1)


def flow_coords64(flow, h, w):
    """temporal_flow.py:43-49 and ATen's un-normalisation in fp64: ``flow [2, h, w]`` fp32 -> clamped ``(ix, iy)`` fp64 ``[h, w]``."""
    f64 = flow.double()
    xs = torch.arange(w, dtype=torch.float64).view(1, w).expand(h, w)
    ys = torch.arange(h, dtype=torch.float64).view(h, 1).expand(h, w)
    gx = 2.0 * (xs + f64[0]) / float(max(w - 1, 1)) - 1.0
    gy = 2.0 * (ys + f64[1]) / float(max(h - 1, 1)) - 1.0
    ix = torch.clamp(((gx + 1.0) / 2.0) * float(w - 1), 0.0, float(w - 1))
    iy = torch.clamp(((gy + 1.0) / 2.0) * float(h - 1), 0.0, float(h - 1))
    return ix, iy


def flow_warp_ref_and_bound(x, frm, flow, alpha, dt, h, w):
    """One frame of ``vface_flow_warp`` in fp64 and what a correct kernel may differ by, per element.  ``x [h w, C]``: the frame
    itself, ``frm [h w, C]``: the frame it is warped from (the previous one, or the halo), both 16-bit; ``flow [2, h, w]`` fp32.
    Returns ``(ref, bound)`` fp64 ``[h w, C]``, both from fp64 quantities of the reference alone (and from the one fp32 product the
    reference itself rounds to the storage type):

      (ix, iy) = the reference's coordinate in fp64: grid + flow, normalise, un-normalise, border clamp (``flow_coords64``)
      warp     = sum over the four taps of w_tap tap, bilinear, x1 = min(x0 + 1, w - 1), y1 alike (weight 0 where clamped)
      ax       = round_dt(fp32(alpha) * x)         -- python scalar * 16-bit tensor keeps the 16-bit type in the reference: ONE IEEE
                                                      fp32 product rounded to ``dt``, restated exactly in torch fp32 (no error term)
      ref      = ax + fp32(1 - alpha) * warp
      bound    = |oma| 8 U32 S + 2 U32 (|ax| + |oma| S) + |oma| (dcx slope_x + dcy slope_y) + 0.5 ulp(|ref| + all of that)

    * S = sum |w_tap tap|.  8 U32 S: wx1 = ix - floor(ix) is exact, wx0 = 1 - wx1 one rounding, the product of two weights one,
      the product with the tap one, three additions (or their fused forms): six roundings on the way of any tap, + 2 for second
      order and the two weights of a product both being rounded.
    * 2 U32 (...): the product oma * warp and the final fp32 sum.
    * dcx = COORD_ULPS U32 (w - 1): the kernel's fp32 coordinate passes through x + dx, the division, - 1, + 1 and the product
      with (w - 1) -- five roundings (six in the reciprocal form) of numbers that, once inside the map, are no larger than w - 1
      in units of the coordinate; outside the map both coordinates are clamped to the same border.  COORD_ULPS = 8.  A map of
      width 1 has ix = 0 by arithmetic: dcx = 0.
    * slope_x: bilinear interpolation is continuous across cell borders and its x-derivative inside a cell is no larger than the
      larger |tap(x + 1) - tap(x)| of the cell's two rows; the kernel's coordinate may lie across a border from the reference's
      (an integer flow floors to x0 - 1 with weight ~1), so the maximum runs over the footprint AND the cells next to it: columns
      x0 - 1 .. x1 + 1, rows y0 - 1 .. y1 + 1.  slope_y alike.
    * one rounding to ``dt`` at the largest magnitude the bound admits."""
    C = x.shape[1]
    img = frm.double().reshape(h, w, C)
    ix, iy = flow_coords64(flow, h, w)
    x0, y0 = torch.floor(ix).long(), torch.floor(iy).long()
    wx1, wy1 = (ix - x0)[..., None], (iy - y0)[..., None]
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    x1, y1 = torch.clamp(x0 + 1, max=w - 1), torch.clamp(y0 + 1, max=h - 1)
    a, b, c, d = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    warp = a * (wx0 * wy0) + b * (wx1 * wy0) + c * (wx0 * wy1) + d * (wx1 * wy1)
    S = a.abs() * (wx0 * wy0) + b.abs() * (wx1 * wy0) + c.abs() * (wx0 * wy1) + d.abs() * (wx1 * wy1)
    chw = img.permute(2, 0, 1)[None]
    dxm = F.pad((chw[..., 1:] - chw[..., :-1]).abs(), (0, 1))             # |tap(x + 1) - tap(x)|, 0 in the last column
    dym = F.pad((chw[..., 1:, :] - chw[..., :-1, :]).abs(), (0, 0, 0, 1))
    mx = F.max_pool2d(dxm, 3, stride=1, padding=1)[0].permute(1, 2, 0)    # [h, w, C]: the maximum over the 3 x 3 cells around
    my = F.max_pool2d(dym, 3, stride=1, padding=1)[0].permute(1, 2, 0)
    slope_x = torch.maximum(mx[y0, x0], mx[y1, x0])
    slope_y = torch.maximum(my[y0, x0], my[y0, x1])
    ax = (torch.tensor(alpha, dtype=torch.float32) * x.float()).to(dt).double().reshape(h, w, C)
    oma = float(torch.tensor(1.0 - alpha, dtype=torch.float32))
    ref = ax + oma * warp
    o = abs(oma)
    e = o * 8 * U32 * S + 2 * U32 * (ax.abs() + o * S) + o * COORD_ULPS * U32 * ((w - 1) * slope_x + (h - 1) * slope_y)
    return ref.reshape(h * w, C), as_16bit(ref, e, dt).reshape(h * w, C)


def flow_to_latent_ref_and_bound(flow_px, f):
    """``vface_flow_to_latent``: the fp64 mean over each f x f block divided by f, and ``(f f + 2) U32 mean|x| / f``: f f - 1 fp32
    additions in order, each at most U32 of a partial sum no larger than sum |x|, the reciprocal of f^3 and the product."""
    x64 = flow_px.double()
    ref = F.avg_pool2d(x64, f) / f
    return ref, (f * f + 2) * U32 * F.avg_pool2d(x64.abs(), f) / f


def ddim_step_ref_and_bound(eu, ec, er, x, inv, noise, *, scale, a_t, a_prev, sigma_t, sqrt_1m_at, single):
    """``vface_ddim_step`` in fp64 and its per-element fp32 bound.  ``eu, ec, er, x, inv, noise``: fp32 tensors of one shape (``ec``
    / ``er`` / ``inv`` / ``noise`` None where the mode has none); the scalars are taken AS ROUNDED TO fp32, which is what the kernel
    receives.  ddim_w_inv.py:666-667, 686-700; with ``single=1``, a_t = a_cur, a_prev = a_next, scale 0 it is the inversion's
    update (:449) (x - sqrt(1 - a_cur) e) sqrt(a_next) / sqrt(a_cur) + sqrt(1 - a_next) e.

      e    = eu + s (ec - eu)                 de   = 3 U32 (|eu| + |s| |ec - eu|)      the difference, the product, the sum
      num  = x - c e, c = sqrt(1 - a_t)       dnum = c de + 2 U32 (|x| + c |e|)        the product and the difference
      p0   = num / sqrt(a_t)                  dp0  = dnum / sqrt(a_t) + 4 U32 (|x| + c |e|) / sqrt(a_t)
                                              -- sqrtf and the division, relative to the magnitudes num was made from
      dir  = sqrt(1 - a_prev - sigma^2)       ddir = 3 U32 / (2 dir) + 2 U32 dir       two fp32 differences of numbers <= 1 and a
                                              square under the root (d sqrt(a) = da / (2 sqrt(a))), sqrtf itself
      xp   = sqrt(a_prev) p0 + dir e + sigma noise
      dxp  = sqrt(a_prev) dp0 + dir de + ddir |e| + 3 U32 (T + dT),  T = sqrt(a_prev) |p0| + dir |e| + |sigma noise|
                                              -- sqrtf(a_prev) and the three products, the two additions of the three-term sum
    ``pred_x0`` is p0 with dp0.  The recon twin (mode 0): e_r = er + s (er - eu) and the same chain from ``inv``, without noise.
    Returns a dict name -> ``(ref, bound)`` for ``x_prev``, ``pred_x0`` and (mode 0 with ``inv``) ``x_prev_recon``."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    s, a_t, a_prev, sg, c = f32(scale), f32(a_t), f32(a_prev), f32(sigma_t), f32(sqrt_1m_at)
    sat, sap = math.sqrt(a_t), math.sqrt(a_prev)
    dirv = math.sqrt(1.0 - a_prev - sg * sg)
    ddir = 3 * U32 / (2 * dirv) + 2 * U32 * dirv

    def chain(base, diff, x0, nz):
        # e = base + s diff: the guidance eu + s (ec - eu), the recon twin er + s (er - eu), or one branch alone (diff None)
        e = base.double()
        de = torch.zeros_like(e)
        if diff is not None:
            e = base.double() + s * diff
            de = 3 * U32 * (base.double().abs() + abs(s) * diff.abs())
        x64 = x0.double()
        mag = x64.abs() + c * e.abs()
        p0 = (x64 - c * e) / sat
        dp0 = (c * de + 2 * U32 * mag) / sat + 4 * U32 * mag / sat
        t3 = sg * nz.double() if nz is not None else torch.zeros_like(p0)
        xp = sap * p0 + dirv * e + t3
        T = sap * p0.abs() + dirv * e.abs() + t3.abs()
        dT = sap * dp0 + dirv * de + ddir * e.abs()
        return (xp, dT + 3 * U32 * (T + dT)), (p0, dp0)

    out = {}
    out["x_prev"], out["pred_x0"] = chain(eu, None if single == 1 else ec.double() - eu.double(), x, noise)
    if single == 0 and inv is not None:
        out["x_prev_recon"], _ = chain(er, er.double() - eu.double(), inv, None)
    return out


def timestep_embedding_ref_and_bound(t, dim, dt):
    """``vface_timestep_embedding``: fp64 cos / sin of the fp32-rounded chain of util.py:151-171 (freqs = exp(-ln(10000) i / half)
    and args = t * freqs in torch fp32 on the CPU), the zero pad of an odd ``dim``, and

      bound = 8 U32 |arg| + 4 U32 + 0.5 ulp(|ref| + that, dt)

    * 8 U32 |arg|: the kernel's freq and torch's are two fp32 evaluations of the same exp of the same fp32 argument (the product
      with i and the division by half are single IEEE operations on both sides): expf within 2 ulp = 4 U32 relative on the
      device, torch's within 1 ulp = 2 U32; then the product t * freq, one rounding on each side: 2 U32.  |cos'|, |sin'| <= 1, so
      an error of the argument is an error of the result.
    * 4 U32: cosf / sinf within 2 ulp of a result no larger than 1, at any argument up to 999 (full-range reduction).
    * one rounding to ``dt``."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
    args = (t[:, None].float() * freqs[None]).double()
    ref = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    e = (8 * U32 * args.abs() + 4 * U32).repeat(1, 2)
    if dim % 2:
        ref, e = torch.cat([ref, torch.zeros_like(ref[:, :1])], -1), torch.cat([e, torch.zeros_like(e[:, :1])], -1)
    return ref, as_16bit(ref, e, dt)


# ------------------------------------------------------------------------------------------------ the flow producer's glue kernels (csrc/raft.hip)
# Used by test_glue_kernels_gpu.py (synthetic operands, one kernel at a time) and by raft_stages.check_stage (the engine's own
# operands, stage by stage).  Transcendental steps take their allowance from ``cpu_fp32_rel_error`` on the case's own arguments.
def chan_stats_slices(hw):
    """The pixel slices of the statistics launch (vf_chan_stats_slices): what fixes the length of one lane's sum."""
    return 16 if hw >= 16384 else (4 if hw >= 2048 else 1)


def channel_stats_ref_and_bound(x64, eps):
    """nn.InstanceNorm2d's (mean, 1 / sqrt(var + eps)) per image and channel of ``x64 [nimg, hw, C]`` (fp64 of the stored 16-bit
    values), biased variance.  Returns ``(ref [nimg, C, 2], bound [nimg, C, 2])``.
    Bound, u = 2^-24, in moments about the pivot p = the channel's first pixel of the image (any value of the data serves; it
    is within the spread of the channel, so nothing below grows with mean^2).  d = x - p, A1 = mean|d|, A2 = mean d^2,
    delta = mean - p.  A lane sums n = ceil(ceil(hw / S) / 32) values in order, 32 lanes are folded in order, the slices in fp64:
    each fp32 sum is off by at most L u (sum of |terms|), L = n + 32 + 2 (the subtraction d and the square round once each).
      mean = p + sum d / hw            off by  L u A1 + u |mean|        (the second term: the fp32 store)
      var  = sum d^2 / hw - delta^2    off by  dV = L u A2 + 2 |delta| L u A1
      rstd = 1 / sqrt(var + eps)       off by  rstd (dV / (2 (var + eps)) + 2 u)
    A constant channel has d = 0 exactly: mean exact, var = 0, rstd = fp32(1 / sqrt(eps))."""
    hw = x64.shape[1]
    mean, var = x64.mean(1), x64.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    d = x64 - x64[:, :1]
    A1, A2, delta = d.abs().mean(1), (d * d).mean(1), d.mean(1)
    L = -(-(-(-hw // chan_stats_slices(hw))) // 32) + 34
    d_mean = L * U32 * A1 + U32 * mean.abs()
    d_var = L * U32 * A2 + 2 * delta.abs() * L * U32 * A1
    d_rstd = rstd * (d_var / (2 * (var + eps)) + 2 * U32)
    return torch.stack([mean, rstd], -1), torch.stack([d_mean, d_rstd], -1)


def channel_norm_ref_and_bound(x64, stats64, dstats, dt):
    """o = (x - mean) rstd of ``x64 [nimg, hw, C]`` from the fp64 statistics of ``channel_stats_ref_and_bound`` and their bounds,
    rounded to ``dt``: 0.5 ulp(o) + rstd dMean + |x - mean| dRstd + 3 u |o|."""
    mean, rstd, d_mean, d_rstd = stats64[..., 0], stats64[..., 1], dstats[..., 0], dstats[..., 1]
    ref = (x64 - mean[:, None]) * rstd[:, None]
    return ref, 0.5 * ulp(ref, dt) + rstd[:, None] * d_mean[:, None] + (x64 - mean[:, None]).abs() * d_rstd[:, None] + 3 * U32 * ref.abs()


ACT_FN = {"none": lambda v: v, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}
ACT_LIP = {"none": 1.0, "relu": 1.0, "tanh": 1.0, "sigmoid": 0.25}            # Lipschitz constants


def norm_act_pre_ref_and_bound(x64, st64, r64, hw):
    """v = (x - mean) rstd + res in fp64 FROM GIVEN fp32 STATISTICS ``st64 [nimg, C, 2]`` (read back from the device or handed to
    the kernel; None: no normalisation) and the bound dv of its fp32 evaluation: the subtraction and the product round once each
    (2 u |(x - mean) rstd|), the sum with the residual once (u |v|)."""
    v, dv = x64, torch.zeros_like(x64)
    if st64 is not None:
        m = st64[:, :, 0].repeat_interleave(hw, 0)
        s = st64[:, :, 1].repeat_interleave(hw, 0)
        v = (x64 - m) * s
        dv = 2 * U32 * v.abs()
    if r64 is not None:
        v = v + r64
        dv = dv + U32 * v.abs()
    return v, dv


def act_ref_and_bound(v, dv, act, out_dt):
    """Reference act(v) and its bound: the activation's Lipschitz constant times dv, the transcendental allowance relative to the
    result plus 2^-126, one fp32 rounding of the result, and 0.5 ulp of a 16-bit output."""
    ref = ACT_FN[act](v)
    b = ACT_LIP[act] * dv + U32 * ref.abs()
    if act in ("tanh", "sigmoid"):
        b = b + cpu_fp32_rel_error(ACT_FN[act], v.float()) * ref.abs() + TINY32
    if out_dt != torch.float32:
        b = b + 0.5 * ulp(ref, out_dt)
    return ref, b


def gru_gate_ref_and_bound(zr, h32, dt, h_err=None):
    """``vface_gru_gate``: z = sigmoid(zr[:, :Hd]) and r h = sigmoid(zr[:, Hd:]) h32 in fp64 on the 16-bit ``zr [M, 2 Hd]`` and
    the fp32 ``h32`` (or an fp64 reference state off by at most ``h_err``).  Returns ``(z, z_bound, rh, rh_bound)``.  z: the sigmoid
    allowance E z + 2^-126 + 0.5 ulp; r h: (E + u) |r h| [+ r h_err] + 2^-126 (1 + |h|) + 0.5 ulp (one product; a flushed sigmoid
    is multiplied by h)."""
    Hd = zr.shape[1] // 2
    E = cpu_fp32_rel_error(torch.sigmoid, zr.float())
    h64 = h32.double()
    zref = torch.sigmoid(zr[:, :Hd].double())
    r = torch.sigmoid(zr[:, Hd:].double())
    rref = r * h64
    rb = (E + U32) * rref.abs()
    if h_err is not None:
        rb = rb + r * h_err
    return zref, E * zref + TINY32 + 0.5 * ulp(zref, dt), rref, rb + TINY32 * (1 + h64.abs()) + 0.5 * ulp(rref, dt)


def gru_update_ref_and_bound(q, z, h64, dt):
    """h' = (1 - z) h + z tanh(q) in fp64 on the 16-bit q, z and the bound of its fp32 evaluation: 1 - z, its product with h and
    the final sum round the first term three times, the tanh allowance E, the product with z and the sum the second."""
    E = cpu_fp32_rel_error(torch.tanh, q.float())
    a, b = (1 - z.double()) * h64, z.double() * torch.tanh(q.double())
    return a + b, 3 * U32 * a.abs() + (E + 2 * U32) * b.abs() + TINY32


def corr_lookup_ref_and_bound(vols, flow32, B, hh, ww, scale, dt):
    """``vface_corr_lookup``: the 9 x 9 bilinear window per level around (x + fx) / 2^l, (y + fy) / 2^l, zero outside the map,
    feature index l 81 + i 9 + j with i the x offset and j the y offset; ``vols``: fp32 [M, h_l, w_l] per level, ``flow32 [M, 2]``
    fp32.  Returns ``(ref [M, levels 81], bound)``.

    The sample point is the kernel's own fp32 value restated in torch fp32, ``((px + f) * 2^-l) + (i - 4)``: two IEEE roundings
    (the sum px + f and the sum with the offset).  The scaling by a power of two is exact, so a fused multiply-add of the last two
    steps gives the same bits; the one exception, a product in the subnormal range (px = 0 and |f| < 2^-123), moves the point by
    less than 2^-149 cells when the offset is 0 and not at all otherwise (an integer plus less than half its last place), which is
    far below every term of the bound.  Everything after it -- floor, the two weights a = s - floor(s) (exact in fp32: Sterbenz /
    same binade or below), the taps -- is fp64 of those fp32 numbers.  For flows that are multiples of 1/64 (test_corr_lookup)
    every step above is exact and this is the plain fp64 point.
    Bound: each of the four terms passes two products and two sums, and the scale one more: 5 u S with S = scale sum_k w_k |v_k|,
    plus 0.5 ulp of the type."""
    M = B * hh * ww
    m = torch.arange(M)
    px, py = (m % ww).float(), ((m // ww) % hh).float()
    f32 = flow32.float()
    off = torch.arange(9, dtype=torch.float32) - 4
    refs, sizes = [], []
    for l, vol in enumerate(vols):
        hl, wl = vol.shape[-2:]
        inv = torch.tensor(1.0 / (1 << l), dtype=torch.float32)
        sx = (((px + f32[:, 0]) * inv)[:, None, None] + off[None, :, None]).double()           # [M, 9 (i), 1]
        sy = (((py + f32[:, 1]) * inv)[:, None, None] + off[None, None, :]).double()           # [M, 1, 9 (j)]
        x0, y0 = torch.floor(sx), torch.floor(sy)
        ax, ay = sx - x0, sy - y0
        flat = vol.reshape(M, hl * wl)
        val, size = torch.zeros(M, 9, 9, dtype=torch.float64), torch.zeros(M, 9, 9, dtype=torch.float64)
        for dy, wy in ((0, 1 - ay), (1, ay)):
            for dx, wx in ((0, 1 - ax), (1, ax)):
                xx, yy = (x0 + dx).expand(M, 9, 9), (y0 + dy).expand(M, 9, 9)
                inside = (xx >= 0) & (xx < wl) & (yy >= 0) & (yy < hl)
                idx = (yy.clamp(0, hl - 1) * wl + xx.clamp(0, wl - 1)).long().reshape(M, 81)
                v = torch.gather(flat, 1, idx).double().reshape(M, 9, 9) * inside
                val += wy * wx * v
                size += wy * wx * v.abs()
        refs.append(val.reshape(M, 81) * scale)
        sizes.append(size.reshape(M, 81) * scale)
    ref, size = torch.cat(refs, 1), torch.cat(sizes, 1)
    return ref, 5 * U32 * size + 0.5 * ulp(ref, dt)


def convex_upsample_ref_and_bound(mask, flow, B, hh, ww, mult=0.25):
    """``vface_convex_upsample``: out[b, :, 8 y + fy, 8 x + fx] = sum_k softmax_k(mult mask[m, k, fy, fx]) 8 flow[neighbour k of m]
    in fp64 (F.unfold's zero padding: a neighbour outside the map adds 0 to the sum and its weight stays in the softmax).
    ``mask [M, >= 576]`` fp32 (index k 64 + fy 8 + fx), ``flow [M, 2]`` fp32.  Returns ``(ref, bound) [B, 2, 8 hh, 8 ww]``.
    Bound.  Weight k carries a relative error eps_k = E + 3 u |d_k|, d_k = its logit minus the row's largest (E: the softmax
    allowance, measured on these logits; the subtraction and the scaling by log2 e inside __expf round in proportion to |d_k|).
    Numerator and denominator are 9 sums each, every term one product, then one division:
    sum_k w_k (eps_k + 10 u) |8 f_k| + |out| (sum_k w_k eps_k + 10 u), and 2^-126 (sum_k |8 f_k| + 1): an exponential below the
    normal range may be flushed, and it is multiplied by 8 f_k."""
    M = B * hh * ww
    lg = mult * mask[:, :576].reshape(M, 9, 64)
    w = torch.softmax(lg.double(), 1)
    E = cpu_fp32_rel_error(torch.softmax, lg, dim=1)
    eps = E + 3 * U32 * (lg.double().amax(1, keepdim=True) - lg.double())
    f8 = 8 * flow.double().reshape(B, hh, ww, 2).permute(0, 3, 1, 2)
    nb = F.unfold(f8, 3, padding=1).reshape(B, 2, 9, hh * ww).permute(0, 3, 1, 2).reshape(M, 2, 9, 1)       # [M, 2, 9 (k), 1]
    ref = (w[:, None] * nb).sum(2)                                                                         # [M, 2, 64]
    bound = ((w * (eps + 10 * U32))[:, None] * nb.abs()).sum(2) + ref.abs() * ((w * eps).sum(1)[:, None] + 10 * U32) \
        + TINY32 * (nb.abs().sum(2) + 1)
    pix = lambda t: t.reshape(B, hh, ww, 2, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(B, 2, 8 * hh, 8 * ww)
    return pix(ref), pix(bound)


def avgpool2_ref(x):
    """``vface_avgpool2_f32`` of fp32 ``x [R, h, w]``: ((a + b) + c + d) * 0.25 in fp32 in the kernel's order -- three correctly
    rounded adds and an exact scale, so equality is derived.  Odd sizes drop the last row / column."""
    oh_, ow_ = x.shape[1] // 2, x.shape[2] // 2
    c = x[:, :2 * oh_, :2 * ow_]
    return (((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + c[:, 1::2, 0::2]) + c[:, 1::2, 1::2]) * 0.25


def flow_update_ref(flow, delta=None):
    """``vface_flow_update``: flow32 + delta32[:, :2], one IEEE fp32 sum (``delta`` None: the flow itself); the 16-bit copies are
    its rounding."""
    return flow + delta[:, :2] if delta is not None else flow


# ------------------------------------------------------------------------------------------------ the face parser's glue kernels (csrc/parsing.hip)
# Used by test_parse_gpu.py (synthetic operands, one kernel at a time) and by parse_bounds.check_stage (the engine's own operands).
def pooled_linear_ref_and_bound(a, w, b, act):
    """``vface_pooled_linear``: act(a w^T + b) in fp64 on the fp32 ``a [nimg, K]``, ``w [N, K]``, ``b [N]`` (or None); ``act``:
    "none", "relu" or "sigmoid".  Returns ``(ref [nimg, N], bound)``.  A lane adds ceil(K / 64) products in order, six butterfly
    levels follow, then the bias: every partial sum is bounded by S = sum |w a| + |b|, so |error| <= (ceil(K / 64) + 8) u S before
    the activation.  ReLU does not expand it; the sigmoid's slope is <= 1/4 and its own evaluation (expf, a division) is allowed
    4 x the relative error of torch's fp32 sigmoid on these inputs (``cpu_fp32_rel_error``)."""
    a64, w64 = a.double(), w.double()
    K = a64.shape[1]
    pre, S = a64 @ w64.T, a64.abs() @ w64.abs().T
    if b is not None:
        pre, S = pre + b.double(), S + b.double().abs()
    bound = (-(-K // 64) + 8) * U32 * S
    if act == "none":
        return pre, bound
    if act == "relu":
        return pre.clamp_min(0), bound
    assert act == "sigmoid", act
    ref = torch.sigmoid(pre)
    return ref, bound / 4 + cpu_fp32_rel_error(torch.sigmoid, pre.float()) * ref


def channel_gate_ref_and_bound(x, g, hw, dt, rvec=None, rten=None, add_x=False):
    """``vface_channel_gate``: y = x g[image] + r in fp64 for the 16-bit ``x [nimg hw, C]``, the fp32 gate ``g [nimg, C]`` and r one
    of nothing, ``rvec [nimg, C]`` (fp32), ``rten [nimg hw, C]`` (16-bit), ``x`` itself (``add_x``).  The kernel does one fp32 fma
    (the 16-bit operands and the fp32 gate are exact in it), then one rounding to the storage type: bound = u |ref| + d."""
    x64 = x.double()
    ref = x64 * g.double().repeat_interleave(hw, 0)
    if rvec is not None:
        ref = ref + rvec.double().repeat_interleave(hw, 0)
    elif rten is not None:
        ref = ref + rten.double()
    elif add_x:
        ref = ref + x64
    b0 = U32 * ref.abs()
    return ref, b0 + 0.5 * ulp(ref.abs() + b0, dt)
