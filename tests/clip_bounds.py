"""fp64 references and per-element bounds of the conditioning kernels (csrc/clip.hip), in the idiom of kernel_bounds.py: every bound
is built from fp64 quantities of the reference alone -- half a unit in the last place of the stored type at the largest value the
bound admits, plus the fp32 evaluation terms, each derived below.  test_clip_kernels_gpu.py checks the kernels against them;
test_clip_bound_cpu.py shows that each admits torch's own fp32 evaluation and refuses one-line defects.
Plain functions, nothing collected by pytest."""
import math

import torch
import torch.nn.functional as F

from kernel_bounds import GELU_AS_ABS, U32, as_16bit, gelu64, layernorm_ref_and_bound

PATCH, PATCH_K, PATCH_KP = 14, 588, 640
# TF.normalize builds its mean / std tensors in the image's type: the reference's constants are these decimals ROUNDED TO fp32
CLIP_MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073], dtype=torch.float32).double()
CLIP_STD = torch.tensor([0.26862954, 0.26130258, 0.27577711], dtype=torch.float32).double()
WEIGHTS = (1.0, 10.0, 0.05)                        # clip_weight, ID_weight, Landmarks_weight of configs/project_ffhq.yaml


def patch_matrix(img):
    """``img [B, 3, S, S]`` -> ``[B G G, 588]``: row (b, py, px), column c 196 + ky 14 + kx -- nn.Unfold's own order, which is the
    flattening of the convolution weight [hidden, 3, 14, 14]."""
    B = img.shape[0]
    cols = F.unfold(img, PATCH, stride=PATCH)                       # [B, 588, G G]
    return cols.permute(0, 2, 1).reshape(B * cols.shape[2], PATCH_K)


def source_index(in_size, out_size):
    """The first source row / column of every output row / column of a bilinear resize without align_corners, in INTEGERS:
    floor(max((in (2 o + 1) - out) / (2 out), 0)) -- ATen's `scale (o + 0.5) - 0.5` clamped at 0, as an exact rational."""
    o = torch.arange(out_size, dtype=torch.int64)
    num = in_size * (2 * o + 1) - out_size
    return torch.clamp(torch.div(num, 2 * out_size, rounding_mode="floor"), min=0).clamp(max=in_size - 1)


def _resize64(t, S):
    """fp64 bilinear resize of ``t [B, C, H, W]`` to S x S (align_corners false, no antialias) from exact rational coordinates;
    returns ``(value, sum of |weight tap|, slope_x, slope_y, fx, fy)``."""
    B, C, H, W = t.shape
    oy, ox = torch.arange(S, dtype=torch.float64), torch.arange(S, dtype=torch.float64)
    fy = torch.clamp((H * (2 * oy + 1) - S) / (2 * S), min=0.0)
    fx = torch.clamp((W * (2 * ox + 1) - S) / (2 * S), min=0.0)
    y0, x0 = source_index(H, S), source_index(W, S)
    y1, x1 = torch.clamp(y0 + 1, max=H - 1), torch.clamp(x0 + 1, max=W - 1)
    ly1, lx1 = (fy - y0)[:, None], (fx - x0)[None, :]
    ly0, lx0 = 1.0 - ly1, 1.0 - lx1
    a, b = t[:, :, y0][:, :, :, x0], t[:, :, y0][:, :, :, x1]
    c, d = t[:, :, y1][:, :, :, x0], t[:, :, y1][:, :, :, x1]
    val = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
    mag = ly0 * (lx0 * a.abs() + lx1 * b.abs()) + ly1 * (lx0 * c.abs() + lx1 * d.abs())
    slope_x = torch.maximum((b - a).abs(), (d - c).abs())
    slope_y = torch.maximum((c - a).abs(), (d - b).abs())
    return val, mag, slope_x, slope_y, fx, fy


def prep_ref(img, mask, S, order="normalise_first"):
    """``prep`` in fp64, ``[B, 3, S, S]``.  ``normalise_first``: ddpm.py:907-912 (un_norm, TF.normalize, TF.resize);
    ``resize_first``: scripts/VFace_inference_batch.py:493-496 (un_norm, Resize, TF.normalize).  ``mask [B, H, W]`` or None:
    every pixel times (1 - mask) first.  The two agree to fp64 rounding: the bilinear weights sum to 1."""
    x = img.double()
    if mask is not None:
        x = x * (1.0 - mask.double())[:, None]
    u = (x + 1.0) / 2.0
    m, s = CLIP_MEAN.view(1, 3, 1, 1), CLIP_STD.view(1, 3, 1, 1)
    if order == "normalise_first":
        return _resize64((u - m) / s, S)[0]
    return (_resize64(u, S)[0] - m) / s


def prep_ref_and_bound(img, mask, S, dt):
    """``vface_clip_patches(prep=1)`` as an image ``[B, 3, S, S]`` in fp64 and what a correct fp32 kernel may differ by, per element.
    With x' = x (1 - m), u = (x' + 1) / 2, d = u - mean, t = d / std per source pixel:

      d_tap = (U32 |x'| + 0.5 U32 |x' + 1| + U32 |d|) / std + U32 |t|
              -- 1 - m and the product (2 U32 |x'|) and the sum x' + 1 (U32 of the result), both halved by the exact division by 2;
              the subtraction of the mean; the division by std
      e32   = sum_taps w d_tap + 8 U32 sum_taps w |t| + dcx slope_x + dcy slope_y
              -- 8 U32: lx1 = fx - x0 is exact, lx0 = 1 - lx1 one rounding, two products and an addition per row, a product and an
              addition for the rows: six roundings on the way of any tap, + 2 for the second order (flow_warp_ref_and_bound's count)
              -- dcx = 4 U32 (fx + 1): the kernel's coordinate is fp32(W / S) * (o + 0.5) - 0.5: the division, the product and the
              subtraction, each at most U32 of a number no larger than fx + 1; it moves the value by at most the footprint's
              larger |tap(x1) - tap(x0)| per unit.  The footprint ITSELF is the reference's: test_clip_kernels_gpu.py checks the
              kernel's first source rows and columns against ``source_index`` bit for bit.
      bound = e32 + 0.5 ulp(|ref| + e32, dt)"""
    x = img.double()
    if mask is not None:
        x = x * (1.0 - mask.double())[:, None]
    m, s = CLIP_MEAN.view(1, 3, 1, 1), CLIP_STD.view(1, 3, 1, 1)
    d = (x + 1.0) / 2.0 - m
    t = d / s
    d_tap = (U32 * x.abs() + 0.5 * U32 * (x + 1.0).abs() + U32 * d.abs()) / s + U32 * t.abs()
    ref, mag, slope_x, slope_y, fx, fy = _resize64(t, S)
    e_taps = _resize64(d_tap, S)[0]
    e32 = e_taps + 8 * U32 * mag + 4 * U32 * (fx + 1.0)[None, :] * slope_x + 4 * U32 * (fy + 1.0)[:, None] * slope_y
    return ref, as_16bit(ref, e32, dt)


def embed_ref_and_bound(tok, cls, pos, B, gamma=None, beta=None, eps=1e-5):
    """``vface_clip_embed``: ``[B (P + 1), C]`` fp64 -- the class row, then the patch rows, plus the position table -- and U32 |ref|:
    one fp32 addition of two exactly represented operands.  With ``gamma, beta``: the LayerNorm of those rows in fp64 and
    ``layernorm_ref_and_bound``'s fp32 form (the same two passes) with that U32 |row| as the input's error, plus U32 |y| for the
    stored fp32 value."""
    P, C = pos.shape[0] - 1, pos.shape[1]
    rows = torch.cat([cls.double().view(1, 1, C).expand(B, 1, C), tok.double().view(B, P, C)], 1) + pos.double()[None]
    ref = rows.reshape(B * (P + 1), C)
    if gamma is None:
        return ref, U32 * ref.abs()
    y, e32 = layernorm_ref_and_bound(ref, gamma, beta, eps, torch.float16, x_err=U32 * ref.abs(), rounded=False)
    return y, e32 + U32 * y.abs()


def act_ref_and_bound(v, kind, dt):
    """``vface_act`` in fp64 and its per-element bound.  ``v``: the 16-bit input.
    quick_gelu, ref = v sigma(a), a = 1.702 v, sigma = 1 / (1 + E), E = exp(-a):
      dE / E  <= 3 U32 |a| + 8 U32    -- the constant's rounding and the product (2 U32 |a|), the product with log2(e) inside
                                        __expf (U32 |a|), v_exp_f32 itself (8 U32, attention_ref_and_bound's allowance)
      d sigma / sigma = (1 - sigma) dE / E + 2 U32    -- through 1 / (1 + E); the sum 1 + E and the division
      e32 = |ref| ((1 - sigma) (3 U32 |a| + 8 U32) + 3 U32)
    erf-GELU, ref = v Phi(v): e32 = |v| (7.5e-8 + 8 U32), gelu_erf_f's allowance in kernel_bounds._geglu.
    Then one rounding to ``dt``."""
    v64 = v.double()
    if kind == 0:
        a = 1.702 * v64
        sg = torch.sigmoid(a)
        ref = v64 * sg
        e32 = ref.abs() * ((1.0 - sg) * (3 * U32 * a.abs() + 8 * U32) + 3 * U32)
    else:
        ref = gelu64(v64)
        e32 = v64.abs() * (GELU_AS_ABS + 8 * U32)
    return ref, as_16bit(ref, e32, dt)


def mix_ref_and_bound(operands, B, w_sum=None):
    """``vface_cond_mix`` (ddpm.py:1038-1039) in fp64 with the weights AS ROUNDED TO fp32 (what the kernel receives; the reference's
    `tensor * python float` rounds them the same way).  ``operands``: (tensor [B | 1, N] or None, weight) triples.  Returns
    ``(ref, e32)``: e32 = 3 U32 sum |x w| / |w_sum| + U32 |ref| -- a product per operand and the two additions of numbers no larger
    than sum |x w|, then the division."""
    f32 = lambda w: float(torch.tensor(w, dtype=torch.float32))
    present = [(t.double().expand(B, -1), f32(w)) for t, w in operands if t is not None]
    ws = f32(sum(w for t, w in operands if t is not None) if w_sum is None else w_sum)
    num = sum(t * w for t, w in present)
    mag = sum((t * w).abs() for t, w in present)
    ref = num / ws
    return ref, 3 * U32 * mag / abs(ws) + U32 * ref.abs()


def smooth_frames(B, H, W, seed):
    """``[B, 3, H, W]`` fp32 in [-1, 1]: low-frequency waves plus noise (cases_parse.crop's recipe on a float image)."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    img = torch.zeros(B, 3, H, W)
    for b in range(B):
        for c in range(3):
            for _ in range(3):
                fy, fx, ph, amp = (torch.rand(1, generator=g).item() for _ in range(4))
                img[b, c] += (0.15 + 0.2 * amp) * torch.sin(2 * math.pi * ((0.5 + 5 * fy) * y + (0.5 + 5 * fx) * x + ph))
    return (img + 0.2 * (torch.rand(B, 3, H, W, generator=g) - 0.5)).clamp(-1, 1)
