"""The face-parsing kernels' arithmetic, restated on the CPU in numpy / torch (fp64 and fp32), as tests/intake_model.py is for the
intake.  Every function takes ``dtype`` = np.float32 (the kernel's own order and roundings, apart from the 16-bit storage the caller
applies) or np.float64 (the yardstick the GPU tests compare with)."""
import numpy as np
import torch
import torch.nn.functional as F

from vface_amd.parsing import BN_EPS, LAYERS, fold_bn

SEG_MEAN = np.array([0.485, 0.456, 0.406], np.float32)
SEG_STD = np.array([0.229, 0.224, 0.225], np.float32)


def taps() -> np.ndarray:
    """fp32 [8]: bicubic((i - 4 + 0.5) / 2), a = -0.5, over its fp32 sum (every value before the division is exact in fp32)."""
    a = np.float32(-0.5)
    x = np.abs((np.arange(8, dtype=np.float32) - np.float32(4) + np.float32(0.5)) / np.float32(2))
    near = (a + 2) * (x * x * x) - (a + 3) * (x * x) + 1
    far = a * (x * x * x) - 5 * a * (x * x) + 8 * a * x - 4 * a
    k = np.where(x <= 1, near, np.where(x < 2, far, 0)).astype(np.float32)
    s = np.float32(0)
    for v in k:
        s = np.float32(s + v)
    return (k / s).astype(np.float32)


def _reflect(i: np.ndarray, n: int) -> np.ndarray:
    return np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def prefilter(crop_u8: np.ndarray, dtype=np.float32) -> np.ndarray:
    """uint8 [..., H2, W2, 3] -> [..., H2/2, W2/2, 3]: / 255, vertical 8 taps, horizontal 8 taps (each a sequential sum), clamp,
    normalise.  In fp64 the taps and the constants are still the kernel's fp32 numbers."""
    k = taps().astype(dtype)
    H2, W2 = crop_u8.shape[-3], crop_u8.shape[-2]
    x = crop_u8.astype(dtype) / dtype(255)
    rows = _reflect(2 * np.arange(H2 // 2)[:, None] - 3 + np.arange(8)[None, :], H2)       # [h, 8]
    v = np.zeros(x.shape[:-3] + (H2 // 2, W2, 3), dtype)
    for t in range(8):
        v = v + k[t] * np.take(x, rows[:, t], axis=-3)
    cols = _reflect(2 * np.arange(W2 // 2)[:, None] - 3 + np.arange(8)[None, :], W2)
    o = np.zeros(x.shape[:-3] + (H2 // 2, W2 // 2, 3), dtype)
    for j in range(8):
        o = o + k[j] * np.take(v, cols[:, j], axis=-2)
    return ((np.clip(o, 0, 1) - SEG_MEAN.astype(dtype)) / SEG_STD.astype(dtype)).astype(dtype)


def maxpool(x: np.ndarray) -> np.ndarray:
    """[N, H, W, C] -> [N, OH, OW, C]: window 3, stride 2, padding 1 with -inf."""
    N, H, W, C = x.shape
    p = np.full((N, H + 2, W + 2, C), -np.inf, x.dtype)
    p[:, 1:-1, 1:-1] = x
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = np.full((N, OH, OW, C), -np.inf, x.dtype)
    for ky in range(3):
        for kx in range(3):
            out = np.maximum(out, p[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2][:, :OH, :OW])
    return out


def gate(x: np.ndarray, g: np.ndarray, r=None) -> np.ndarray:
    """[N, hw, C] * [N, 1, C] + r in fp64 (the kernel: one fp32 fma; the difference is below u |result|)."""
    y = x.astype(np.float64) * g.astype(np.float64)[:, None, :]
    return y if r is None else y + r.astype(np.float64)


def upsample(logits: np.ndarray, H: int, W: int, dtype=np.float32) -> np.ndarray:
    """[F, h, w, C] -> [F, H, W, C]: bilinear, align_corners=True, in ATen's order (scale and source coordinate in fp32 also for
    the fp64 yardstick: the kernel's weights ARE those fp32 numbers; the blend is then exact to fp64)."""
    Fn, h, w, C = logits.shape
    f32 = np.float32

    def axis(n_in, n_out):
        s = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
        src = (s * np.arange(n_out, dtype=f32)).astype(f32)
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        l1 = np.clip((src - i0.astype(f32)).astype(f32), 0, 1)
        return i0, i1, (f32(1) - l1).astype(dtype), l1.astype(dtype)
    y0, y1, ly0, ly1 = axis(h, H)
    x0, x1, lx0, lx1 = axis(w, W)
    v = logits.astype(dtype)
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    top = lx0 * v[:, y0][:, :, x0] + lx1 * v[:, y0][:, :, x1]
    bot = lx0 * v[:, y1][:, :, x0] + lx1 * v[:, y1][:, :, x1]
    return (ly0[None, :, None, None] * top + ly1[None, :, None, None] * bot).astype(dtype)


def argmax_and_margin(full: np.ndarray):
    """[F, H, W, C] -> (first maximal class uint8 [F, H, W], top - runner-up [F, H, W])."""
    lab = np.argmax(full, axis=-1)
    part = np.partition(full, -2, axis=-1)
    return lab.astype(np.uint8), part[..., -1] - part[..., -2]


def seg12_table() -> np.ndarray:
    from vface_amd.parsing import seg12_table as t
    return t().numpy()


# ---- the network --------------------------------------------------------------------------------------------------------------
def _cbr(sd, x, conv, bn, dt, stride=1, relu=True):
    w = sd[conv + ".weight"]
    if bn is not None:
        w, b = fold_bn(w, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"], BN_EPS)
        b = b.to(dt)
    else:
        b = None
    y = F.conv2d(x, w.to(dt), b, stride=stride, padding=w.shape[-1] // 2)
    return F.relu(y) if relu else y


@torch.no_grad()
def net_logits(sd, x: torch.Tensor, dt=torch.float32) -> torch.Tensor:
    """BiSeNet's first head at 1/8 resolution from a state dict, BatchNorm folded as the engine folds it: [N, 3, H, W] ->
    [N, 19, H/8, W/8] (before the reference's bilinear upsampling, model.py:258)."""
    sd = {k: v.double() for k, v in sd.items() if torch.is_floating_point(v)}
    x = x.to(dt)
    r = "cp.resnet"
    x = _cbr(sd, x, f"{r}.conv1", f"{r}.bn1", dt, stride=2)
    x = F.max_pool2d(x, 3, 2, 1)
    feats = {}
    for li, (cout, stride) in enumerate(LAYERS, start=1):
        for bi in (0, 1):
            b = f"{r}.layer{li}.{bi}"
            st = stride if bi == 0 else 1
            t = _cbr(sd, x, f"{b}.conv1", f"{b}.bn1", dt, stride=st)
            t = _cbr(sd, t, f"{b}.conv2", f"{b}.bn2", dt, relu=False)
            s = _cbr(sd, x, f"{b}.downsample.0", f"{b}.downsample.1", dt, stride=st, relu=False) if f"{b}.downsample.0.weight" in sd else x
            x = F.relu(s + t)
        feats[li] = x
    f8, f16, f32_ = feats[2], feats[3], feats[4]

    def arm(name, v):
        feat = _cbr(sd, v, f"{name}.conv.conv", f"{name}.conv.bn", dt)
        att = torch.sigmoid(_cbr(sd, feat.mean((2, 3), keepdim=True), f"{name}.conv_atten", f"{name}.bn_atten", dt, relu=False))
        return feat * att
    avg = _cbr(sd, f32_.mean((2, 3), keepdim=True), "cp.conv_avg.conv", "cp.conv_avg.bn", dt)
    s32 = arm("cp.arm32", f32_) + avg
    up32 = _cbr(sd, F.interpolate(s32, scale_factor=2, mode="nearest"), "cp.conv_head32.conv", "cp.conv_head32.bn", dt)
    s16 = arm("cp.arm16", f16) + up32
    cp8 = _cbr(sd, F.interpolate(s16, scale_factor=2, mode="nearest"), "cp.conv_head16.conv", "cp.conv_head16.bn", dt)
    feat = _cbr(sd, torch.cat([f8, cp8], 1), "ffm.convblk.conv", "ffm.convblk.bn", dt)
    att = _cbr(sd, feat.mean((2, 3), keepdim=True), "ffm.conv1", None, dt)
    att = torch.sigmoid(_cbr(sd, att, "ffm.conv2", None, dt, relu=False))
    feat = feat * att + feat
    mid = _cbr(sd, feat, "conv_out.conv.conv", "conv_out.conv.bn", dt)
    return _cbr(sd, mid, "conv_out.conv_out", None, dt, relu=False)
