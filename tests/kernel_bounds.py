"""Helpers of the per-kernel GPU tests (test_kernels_gpu.py, test_glue_kernels_gpu.py): seeded 16-bit inputs, the unit in the last
place of a 16-bit type, sentinel-filled buffers that show a store outside a kernel's slot, and the element-wise bound check that
names the worst element.  Plain functions, nothing collected by pytest."""
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
