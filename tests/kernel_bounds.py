"""Helpers of the per-kernel GPU tests (test_kernels_gpu.py, test_glue_kernels_gpu.py, test_attention_gpu.py): seeded 16-bit inputs, the
unit in the last place of a 16-bit type, sentinel-filled buffers that show a store outside a kernel's slot, the element-wise bound
check that names the worst element, and the attention kernel's fp64 reference with its per-element bound.  Plain functions, nothing
collected by pytest."""
import torch

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
