"""numpy restatement of source_tensors_kernel (csrc/intake.hip) in the kernel's own order, in the role tests/intake_model.py plays
for the frame intake: what the GPU must reproduce bit for bit, itself checked on the CPU (tests/test_source_cpu.py) against the
reference's statements run with live torch.  The 8-bit resize is OpenCV's 11-bit fixed-point 2-tap form as DESIGN §9 states it;
OpenCV is not available to the tests, so parity with ``cv2.resize`` is NOT pinned here or anywhere else."""
import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def linear_taps(n_in: int, n_out: int):
    """(s, s') [n_out, 2] and (w0, w1) [n_out, 2], written independently of vface_amd.scripts.resample.linear_taps_u8 (the CPU
    test compares the two): one output index at a time, Python floats (doubles), round half to even."""
    taps, weights = np.empty((n_out, 2), np.int32), np.empty((n_out, 2), np.int16)
    for d in range(n_out):
        f = (d + 0.5) * n_in / n_out - 0.5
        s = int(np.floor(f))
        t = f - s
        if s < 0:
            s, t = 0, 0.0
        if s >= n_in - 1:
            s, t = n_in - 1, 0.0
        taps[d] = (s, min(s + 1, n_in - 1))
        weights[d] = (round(2048 * (1 - t)), round(2048 * t))        # Python's round() is half-to-even, as rint
    return taps, weights


def resize_linear_u8(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """[h, w, C] uint8 -> [out_h, out_w, C] uint8: horizontal pass R = p[s] w0 + p[s'] w1, vertical pass
    q = (((v0 (R0 >> 4)) >> 16) + ((v1 (R1 >> 4)) >> 16) + 2) >> 2, all in 32-bit integers."""
    h, w = img.shape[:2]
    xt, xw = linear_taps(w, out_w)
    yt, yw = linear_taps(h, out_h)
    p = img.astype(np.int64)
    R = p[:, xt[:, 0]] * xw[:, 0].astype(np.int64)[None, :, None] + p[:, xt[:, 1]] * xw[:, 1].astype(np.int64)[None, :, None]
    assert R.max() < 2 ** 31
    v0, v1 = yw[:, 0].astype(np.int64)[:, None, None], yw[:, 1].astype(np.int64)[:, None, None]
    a, b = v0 * (R[yt[:, 0]] >> 4), v1 * (R[yt[:, 1]] >> 4)
    assert a.max() < 2 ** 31 and b.max() < 2 ** 31                      # the kernel's products are ints
    q = ((a >> 16) + (b >> 16) + 2) >> 2
    assert q.min() >= 0 and q.max() <= 255                              # no clip is ever needed
    return q.astype(np.uint8)


def bilinear_f64(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """The exact 2-tap bilinear value in float64 (half-pixel centres, edge clamp, no antialias): what the fixed-point form approximates."""
    h, w = img.shape[:2]

    def axis(n_in, n_out):
        f = (np.arange(n_out) + 0.5) * n_in / n_out - 0.5
        s = np.floor(f)
        t = f - s
        lo, hi = s < 0, s >= n_in - 1
        s = np.where(lo, 0, np.where(hi, n_in - 1, s)).astype(np.int64)
        t = np.where(lo | hi, 0.0, t)
        return s, np.minimum(s + 1, n_in - 1), t
    xa, xb, tx = axis(w, out_w)
    ya, yb, ty = axis(h, out_h)
    p = img.astype(np.float64)
    rows = p[:, xa] * (1 - tx)[None, :, None] + p[:, xb] * tx[None, :, None]
    return rows[ya] * (1 - ty)[:, None, None] + rows[yb] * ty[:, None, None]


def resize_map_f32(m: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """[H, W] float32 -> [oh, ow]: mask_latent_kernel's / frame_normalise_resize_kernel's fp32 order (tests/intake_model.py)."""
    f = np.float32
    H, W = m.shape
    sy, sx = f(H) / f(oh), f(W) / f(ow)
    fy = np.maximum(sy * (np.arange(oh, dtype=f) + f(0.5)) - f(0.5), f(0.0)).astype(f)
    fx = np.maximum(sx * (np.arange(ow, dtype=f) + f(0.5)) - f(0.5), f(0.0)).astype(f)
    y0, x0 = np.minimum(fy.astype(np.int64), H - 1), np.minimum(fx.astype(np.int64), W - 1)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    ly1, lx1 = (fy - y0.astype(f)).astype(f)[:, None], (fx - x0.astype(f)).astype(f)[None, :]
    ly0, lx0 = f(1.0) - ly1, f(1.0) - lx1
    top = lx0 * m[y0][:, x0] + lx1 * m[y0][:, x1]
    bot = lx0 * m[y1][:, x0] + lx1 * m[y1][:, x1]
    out = ly0 * top + ly1 * bot
    assert out.dtype == f
    return out


def clip_normalise(q: np.ndarray) -> np.ndarray:
    """get_tensor_clip() on a uint8 [h, w, 3] image: /255, - mean, / std in float32, planar."""
    f = np.float32
    mean, std = np.array(CLIP_MEAN, f)[:, None, None], np.array(CLIP_STD, f)[:, None, None]
    out = (q.astype(f).transpose(2, 0, 1) / f(255.0) - mean) / std
    assert out.dtype == f
    return out


def source_tensors(crop: np.ndarray, img: np.ndarray, label: np.ndarray, preserve, oh: int, ow: int, oc: int):
    """source_tensors_kernel for one image: crop [S, S, 3], img [H, W, 3], label [H, W] (uint8).  Returns
    mask [1, H, W], masked [3, H, W], inpaint [3, H, W], mask_latent [1, oh, ow], clip_image [3, oc, oc], clip_u8 [oc, oc, 3]."""
    f = np.float32
    member = np.isin(np.arange(256), list(preserve))
    m = member[label].astype(f)
    keep = (f(1.0) - m).astype(f)
    masked = ((img.astype(f) / f(255.0) - f(0.5)) / f(0.5)).transpose(2, 0, 1) * m[None]
    inpaint = masked * keep[None]
    mlat = resize_map_f32(keep, oh, ow)
    q = resize_linear_u8(crop, oc, oc)
    clip_image = clip_normalise(q) * resize_map_f32(m, oc, oc)[None]
    for t in (masked, inpaint, mlat, clip_image):
        assert t.dtype == f
    return m[None], masked, inpaint, mlat[None], clip_image, q
