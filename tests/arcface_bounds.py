"""fp64 references and per-element bounds of the identity network's kernels (csrc/arcface.hip), in the idiom of kernel_bounds.py /
clip_bounds.py: every bound is built from fp64 quantities of the reference alone -- the fp32 evaluation terms derived below, plus
half a unit in the last place of the stored type at the largest value the bound admits.  test_arcface_kernels_gpu.py checks the
kernels against them; test_arcface_bound_cpu.py shows that each admits torch's own fp32 evaluation and refuses one-line defects.
Plain functions, nothing collected by pytest."""
import torch
import torch.nn.functional as F

from clip_bounds import CLIP_MEAN, CLIP_STD, _resize64
from kernel_bounds import U32, as_16bit

POOL, Y0, X0, CROP, OUT, CLIP_SIZE = 256, 35, 32, 188, 112, 224


def _affine(y, e_y, za, zb, dt):
    """z = za y32 + zb as ONE fp32 fma of a y32 within e_y of y: |za| e_y + U32 |z|, then the rounding."""
    z = za.double() * y + zb.double()
    return z, as_16bit(z, za.double().abs() * e_y + U32 * z.abs(), dt)


def prelu_ref_and_bound(x, slope, dt, za=None, zb=None):
    """``vface_prelu``.  ``x [M, C]``: the 16-bit input; ``slope, za, zb [C]`` fp32.  y = x (exact) or slope x (one fp32 product:
    U32 |y|); returns ``(y, bound_y, z, bound_z)``, the last two None without ``za``."""
    x64 = x.double()
    y = torch.where(x64 > 0, x64, slope.double() * x64)
    e_y = torch.where(x64 > 0, torch.zeros_like(y), U32 * y.abs())
    if za is None:
        return y, as_16bit(y, e_y, dt), None, None
    z, bz = _affine(y, e_y, za, zb, dt)
    return y, as_16bit(y, e_y, dt), z, bz


def strided_rows(x, nimg, H, W, s):
    """Rows (n, oy s, ox s) of ``x [nimg H W, C]``: MaxPool2d(1, s), OH = (H - 1) // s + 1."""
    return x.reshape(nimg, H, W, -1)[:, ::s, ::s].reshape(-1, x.shape[1])


def se_gate_add_ref_and_bound(res, g, sc, dt, *, nimg, za=None, zb=None):
    """``vface_se_gate_add`` with the shortcut rows already selected (``sc [M, C]``: ``strided_rows`` of the unit's input, or the
    same-sized tensor).  ``res [M, C]`` 16-bit, ``g [nimg, C]`` fp32.  y = res g + sc is ONE fp32 fma of exactly represented
    operands: U32 |y|.  Returns ``(y, bound_y, z, bound_z)``."""
    M = res.shape[0]
    y = res.double() * g.double().repeat_interleave(M // nimg, 0) + sc.double()
    e_y = U32 * y.abs()
    if za is None:
        return y, as_16bit(y, e_y, dt), None, None
    z, bz = _affine(y, e_y, za, zb, dt)
    return y, as_16bit(y, e_y, dt), z, bz


def l2norm_ref_and_bound(x):
    """``vface_l2norm_rows`` on fp32 rows ``x [B, N]``: ref = x / ||x||.  The kernel: a = x / max|x| (U32 each), a a (U32; 3 U32 on
    the square), N of them summed in fp32 in any order ((N - 1) U32 of a sum of non-negative terms), the square root (halves what
    came before, + U32), the product with the maximum, the division: ((N + 2) / 2 + 3) U32 |ref|, + 2 U32 |ref| for the second order
    and v_sqrt / v_rcp's last bit.  Nothing overflows or vanishes: every square is at most 1 and the largest is 1."""
    x64 = x.double()
    ref = x64 / x64.norm(dim=1, keepdim=True)
    return ref, ((x.shape[1] + 2) / 2.0 + 5.0) * U32 * ref.abs()


def clip_image_ref_and_e32(frames, mask):
    """The CLIP-normalised 224 x 224 image ``vface_id_prep(prep=1)`` forms from ``frames [B, 3, H, W]`` in [-1, 1] (``mask
    [B, H, W]`` or None) by ``vface_clip_patches``' expressions: ``clip_bounds.prep_ref_and_bound`` without its final rounding (the
    value stays in fp32 here).  Returns ``(ref, e32)``."""
    x = frames.double()
    if mask is not None:
        x = x * (1.0 - mask.double())[:, None]
    m, s = CLIP_MEAN.view(1, 3, 1, 1), CLIP_STD.view(1, 3, 1, 1)
    d = (x + 1.0) / 2.0 - m
    t = d / s
    d_tap = (U32 * x.abs() + 0.5 * U32 * (x + 1.0).abs() + U32 * d.abs()) / s + U32 * t.abs()
    ref, mag, slope_x, slope_y, fx, fy = _resize64(t, CLIP_SIZE)
    e_taps = _resize64(d_tap, CLIP_SIZE)[0]
    return ref, e_taps + 8 * U32 * mag + 4 * U32 * (fx + 1.0)[None, :] * slope_x + 4 * U32 * (fy + 1.0)[:, None] * slope_y


def _max_bin(n_in, n_out):
    return max(-((-(i + 1) * n_in) // n_out) - (i * n_in) // n_out for i in range(n_out))


def id_prep_ref_and_bound(img, dt, *, clip_img=True, e_in=None):
    """``vface_id_prep`` on the image the chain sees: ``img [B, 3, H, W]`` (fp32 values, or the fp64 CLIP image with ``e_in`` = what
    the kernel's fp32 image may differ from it by).  Returns ``([B, 3, 112, 112], bound)`` fp64, the composite by torch's own
    ``adaptive_avg_pool2d`` in fp64.  With v the value a source pixel takes:

      clip_img: v = ((x std + mean) - 0.5) / 0.5 -- the product, the sum, the difference, each U32 of its result, and the exact
                division: d = 2 (|std| e_in + U32 |x std| + U32 |x std + mean| + U32 |x std + mean - 0.5|); otherwise d = e_in
      a mean of n values in fp32, summed in order and divided: what the values carry, averaged, + n U32 mean |v| (n - 1 additions
                of partial sums no larger than sum |v|, and the division) -- once with n1 = the 256-pool's largest bin (absent
                for a 256-high image), once with n2 = the 112-pool's largest bin (3 x 3 on 188 -> 112)
      bound = e + 0.5 ulp(|ref| + e, dt)"""
    x = img.double()
    e = torch.zeros_like(x) if e_in is None else e_in
    if clip_img:
        m, s = CLIP_MEAN.view(1, 3, 1, 1), CLIP_STD.view(1, 3, 1, 1)
        p = x * s
        e = 2.0 * (s * e + U32 * p.abs() + U32 * (p + m).abs() + U32 * (p + m - 0.5).abs())
        x = (p + m - 0.5) / 0.5
    mag = x.abs()
    if x.shape[2] != POOL:
        n1 = _max_bin(x.shape[2], POOL) * _max_bin(x.shape[3], POOL)
        mag = F.adaptive_avg_pool2d(mag, (POOL, POOL))
        e = F.adaptive_avg_pool2d(e, (POOL, POOL)) + n1 * U32 * mag
        x = F.adaptive_avg_pool2d(x, (POOL, POOL))
    crop = lambda t: t[:, :, Y0:Y0 + CROP, X0:X0 + CROP]
    n2 = _max_bin(CROP, OUT) ** 2
    ref = F.adaptive_avg_pool2d(crop(x), (OUT, OUT))
    e = F.adaptive_avg_pool2d(crop(e), (OUT, OUT)) + n2 * U32 * F.adaptive_avg_pool2d(crop(mag), (OUT, OUT))
    return ref, as_16bit(ref, e, dt)


def rows8(x):
    """``[B, 3, H, W]`` -> the stem's token rows ``[B H W, 8]``: three values, five zeros."""
    B, C, H, W = x.shape
    out = x.new_zeros(B * H * W, 8)
    out[:, :C] = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
    return out
