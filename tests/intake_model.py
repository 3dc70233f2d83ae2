"""numpy restatement of the frame-intake kernels' operation order (csrc/intake.hip, and resample_u8_kernel of csrc/paste.hip with
any tap tables), in the role tests/attention_model.py plays for attention: what the GPU must reproduce bit for bit, itself checked
on the CPU against Pillow and the reference's recorded outputs (tests/test_intake_cpu.py)."""
import numpy as np


def resample_u8(src: np.ndarray, axis: int, bounds: np.ndarray, kk: np.ndarray) -> np.ndarray:
    """One pass of resample_u8_kernel over [H, W, 3] uint8: axis 0 along x, axis 1 along y; 32-bit integer accumulation from
    2^21, arithmetic shift by 22, clip to 0..255."""
    a = np.moveaxis(src.astype(np.int64), 1 if axis == 0 else 0, 0)         # [in_n, lines, 3]
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.int64)
    for o in range(bounds.shape[0]):
        x0, n = int(bounds[o, 0]), int(bounds[o, 1])
        ss = np.full(a.shape[1:], 1 << 21, np.int64)
        for t in range(n):
            ss = ss + a[x0 + t] * int(kk[o, t])
        assert np.abs(ss).max() < 2 ** 31                                  # the kernel's accumulator is an int
        out[o] = ss >> 22
    out = np.clip(out, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, 1 if axis == 0 else 0)


def resize_u8(img: np.ndarray, out_w: int, out_h: int, filter: str) -> np.ndarray:
    from vface_amd.scripts.resample import resample_coeffs
    h, w, _ = img.shape
    if out_w != w:
        img = resample_u8(img, 0, *resample_coeffs(w, out_w, filter))
    if out_h != h:
        img = resample_u8(img, 1, *resample_coeffs(h, out_h, filter))
    return img


def quad_crop(frame: np.ndarray, coeffs: np.ndarray, window, S: int):
    """quad_crop_kernel for one frame [Hs, Ws, 3]: every product and sum a separate float64 rounding, left to right.  Returns (crop, inside)."""
    x0w, y0w, x1w, y1w = (int(v) for v in window)
    win = frame[y0w:y1w, x0w:x1w].astype(np.float64)
    h, w = win.shape[:2]
    a = [np.float64(v) for v in coeffs]
    py, px = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    xc, yc = px + 0.5, py + 0.5
    xin = a[0] + a[1] * xc + a[2] * yc + a[3] * xc * yc
    yin = a[4] + a[5] * xc + a[6] * yc + a[7] * xc * yc
    inside = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    xin, yin = xin - 0.5, yin - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    xa, xb = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1)
    ya = np.clip(y, 0, h - 1)
    has2 = ((y + 1 >= 0) & (y + 1 < h))[..., None]
    yb = np.where(has2[..., 0], np.clip(y + 1, 0, h - 1), ya)
    p00, p01, p10, p11 = win[ya, xa], win[ya, xb], win[yb, xa], win[yb, xb]
    v1 = p00 + (p01 - p00) * dx
    v2 = np.where(has2, p10 + (p11 - p10) * dx, v1)
    v = v1 + (v2 - v1) * dy
    out = v.astype(np.int64).astype(np.uint8)
    out[~inside] = 0
    return out, inside


def crop(frame: np.ndarray, quad, S: int):
    """FrameIntake.crop for one frame on the host: crop_plan's scalars, the Lanczos shrink, quad_crop.  Returns (crop, inside)."""
    from vface_amd.scripts.intake import crop_plan
    shrink, (rw, rh), window, coeffs = crop_plan(quad, frame.shape[1], frame.shape[0], S)
    if shrink > 1:
        frame = resize_u8(frame, rw, rh, "lanczos")
    return quad_crop(frame, coeffs, window, S)


def dataset_tensors(crop_u8: np.ndarray, label: np.ndarray, remove, oh: int, ow: int):
    """dataset_tensors_kernel + mask_latent_kernel for one frame, float32 in the kernels' order."""
    f = np.float32
    member = np.isin(np.arange(256), list(remove))
    m = (f(1.0) - member[label].astype(f)).astype(f)
    image = ((crop_u8.astype(f) / f(255.0) - f(0.5)) / f(0.5)).transpose(2, 0, 1)
    inpaint = image * m[None]
    H, W = label.shape
    sy, sx = f(H) / f(oh), f(W) / f(ow)
    fy = np.maximum(sy * (np.arange(oh, dtype=f) + f(0.5)) - f(0.5), f(0.0)).astype(f)
    fx = np.maximum(sx * (np.arange(ow, dtype=f) + f(0.5)) - f(0.5), f(0.0)).astype(f)
    y0, x0 = np.minimum(fy.astype(np.int64), H - 1), np.minimum(fx.astype(np.int64), W - 1)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    ly1, lx1 = (fy - y0.astype(f)).astype(f)[:, None], (fx - x0.astype(f)).astype(f)[None, :]
    ly0, lx0 = f(1.0) - ly1, f(1.0) - lx1
    top = lx0 * m[y0][:, x0] + lx1 * m[y0][:, x1]
    bot = lx0 * m[y1][:, x0] + lx1 * m[y1][:, x1]
    mlat = ly0 * top + ly1 * bot
    assert image.dtype == f and inpaint.dtype == f and mlat.dtype == f
    return image, inpaint, m[None], mlat[None]
