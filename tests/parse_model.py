"""The face-parsing kernels' arithmetic, restated on the CPU in numpy / torch (fp64 and fp32), as tests/intake_model.py is for the
intake.  Every function takes ``dtype`` = np.float32 (the kernel's own order and roundings, apart from the 16-bit storage the caller
applies) or np.float64 (the yardstick the GPU tests compare with).  ``engine_taps`` (below) restates the whole engine with its rounding points
under the engine's tap names, with one-line defects, for tests/parse_bounds.py."""
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


# ---- the engine, restated with its rounding points --------------------------------------------------------------------------
# ``engine_taps``: ``vface_amd.parsing.ParseEngine.logits`` on the CPU under the engine's tap names, for ``dt`` in fp16 / bf16.
# * Weights are folded in fp64 (``fold_bn``), rounded to ``dt`` and padded as ``ConvNetEngine.add_conv`` does (``weights``): the
#   stem's cin 3 -> 8, the class head's cout 19 -> 32; the five pooled 1x1 convolutions stay fp32; biases are fp32.
# * Every buffer the engine keeps in 16 bits is rounded where the engine rounds it: each convolution's output, each residual sum,
#   each gated sum.  ReLU in place and the max-pool are exact.
# * What the engine keeps in fp32 stays fp32: the means, the pooled vectors (``conv_avg``, the gates, ``ffm.conv1``), the logits.
#   Means and pooled sums are fp64 sums rounded once to fp32; a gated sum is the fp64 value rounded once to fp32 (the kernel's one
#   fma), then to ``dt``.  Convolutions accumulate in the CPU's fp32 (another order than the MFMA's: what the 1.25 / 2 margins of
#   the network-level test are for).
# * ``defect=``: one of ``DEFECTS``, each a one-line departure from the engine; test_parse_bound_cpu.py shows that
#   parse_bounds.check_stage refuses each at the stage that owns it.
DTS = (torch.float16, torch.bfloat16)
MARGIN_L2 = 1.25      # rel-L2: the project's allowance over an emulation (test_clip_gpu.py, test_vae_stages_gpu.py)
MARGIN_WORST = 2.0    # the worst element: an extreme-value statistic of the same distribution
R = "cp.resnet"
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))      # vface_channel_stats' eps (its rstd half is tapped, not used)

# defect -> the stage of parse_bounds that owns it
DEFECTS = {
    "stem_chunk2_over_chunk1": "stem",              # the second frame chunk's rows are written from row 0
    "stem_chunk2_reads_frame0": "stem",             # the second frame chunk's input starts at frame 0
    "maxpool_window_2x2": "stem",                   # rows 2i, 2i + 1 instead of 2i - 1 .. 2i + 1
    "residual_from_conv1": "layer1.0",              # relu(shortcut + conv1.act) instead of + conv2
    "identity_shortcut_dropped": "layer1.0",        # relu(conv2) in the blocks without a downsample
    "downsample_without_bn_shift": "layer2.0",      # downsample.1's folded shift left out
    "bn_fold_var_for_std": "layer1.0",              # gamma / var instead of gamma / sqrt(var + eps), in the blocks' folds
    "feat8_in_right_half": "ffm",                   # layer2.1 writes cat[:, 128:], which conv_head16 then overwrites
    "cat_halves_swapped": "ffm",                    # cat = [feat_cp8 | feat8]
    "cat_right_half_without_relu": "ffm",           # the ReLU of conv_head16 lands outside cat
    "arm_gate_relu": "arm32",                       # ReLU instead of sigmoid on conv_atten
    "arm32_without_avg": "arm32",                   # feat32_arm without + avg_up
    "avg_of_frame0": "arm32",                       # every frame adds frame 0's avg
    "gate_of_frame0": "arm32",                      # every frame is gated by frame 0's gate
    "arm16_adds_before_gating": "arm16",            # (feat + up32) * gate instead of feat * gate + up32
    "mean_is_sum": "avg",                           # the global mean without the division
    "mean_by_other_levels_hw": "arm16",             # arm16's mean divided by layer 4's hw
    "head_upsample_rows_cols_exchanged": "head32",  # the nearest upsampling walks a [W, H] map (differs where H != W)
    "ffm_without_plus_feat": "ffm",                 # feat * atten without + feat
    "ffm_conv1_without_relu": "ffm",
    "conv_out_without_relu": "out",
    "logits_rounded_to_16bit": "out",               # the class head through the compute type before the fp32 store
    "mean_rounded_to_16bit": "avg",                 # a mean through the compute type
}


def rounder(dt):
    return (lambda t: t) if dt == torch.float32 else (lambda t: t.to(dt).float())


def figures(got, ref64):
    """(rel-L2, worst |err| / rms(ref)) against an fp64 reference."""
    e = got.double() - ref64.double()
    rms = float(ref64.double().pow(2).mean().sqrt().clamp_min(1e-30))
    return float(e.norm() / ref64.double().norm().clamp_min(1e-30)), float(e.abs().max()) / rms


def tok(x):
    """[N, C, H, W] -> token rows [N H W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def img(t, N, H, W):
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


def weights(sd, dt, defect=None):
    """name -> (w, b), keyed as ``ParseEngine.P``: w ``[cout_pad, cin_pad, kh, kw]`` fp32 holding values of ``dt`` and b ``[cout_pad]``
    fp32 (None for a layer with neither a bias nor a BatchNorm); a pooled 1x1 convolution: w fp32 ``[N, K]``, unrounded."""
    sd = {k: v.detach().double().cpu() for k, v in sd.items() if torch.is_floating_point(v)}
    r = rounder(dt)
    P = {}

    def add(name, bn=None, cin_pad=None, cout_pad=None, pooled=False):
        w, b = sd[name + ".weight"], sd.get(name + ".bias")
        if bn is not None:
            var, eps = sd[bn + ".running_var"], BN_EPS
            if defect == "bn_fold_var_for_std" and ".layer" in name:
                var, eps = var * var, 0.0
            w, b = fold_bn(w, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], var, eps, b=b)
            if defect == "downsample_without_bn_shift" and "downsample" in name:
                b = torch.zeros_like(b)
        cout, cin, kh, kw = w.shape
        if pooled:
            P[name] = (w.reshape(cout, cin).float(), None if b is None else b.float())
            return
        wp = torch.zeros(cout_pad or cout, cin_pad or cin, kh, kw, dtype=torch.float64)
        wp[:cout, :cin] = w
        bp = None
        if b is not None:
            bp = torch.zeros(wp.shape[0], dtype=torch.float64)
            bp[:cout] = b
            bp = bp.float()
        P[name] = (r(wp.float()), bp)

    add(f"{R}.conv1", f"{R}.bn1", cin_pad=8)
    for li in range(1, 5):
        for bi in (0, 1):
            b = f"{R}.layer{li}.{bi}"
            add(f"{b}.conv1", f"{b}.bn1")
            add(f"{b}.conv2", f"{b}.bn2")
            if f"{b}.downsample.0.weight" in sd:
                add(f"{b}.downsample.0", f"{b}.downsample.1")
    for arm in ("cp.arm16", "cp.arm32"):
        add(f"{arm}.conv.conv", f"{arm}.conv.bn")
        add(f"{arm}.conv_atten", f"{arm}.bn_atten", pooled=True)
    add("cp.conv_avg.conv", "cp.conv_avg.bn", pooled=True)
    add("cp.conv_head32.conv", "cp.conv_head32.bn")
    add("cp.conv_head16.conv", "cp.conv_head16.bn")
    add("ffm.convblk.conv", "ffm.convblk.bn")
    add("ffm.conv1", pooled=True)
    add("ffm.conv2", pooled=True)
    add("conv_out.conv.conv", "conv_out.conv.bn")
    add("conv_out.conv_out", cout_pad=32)
    return P


def conv_img(P, name, xi, stride=1):
    """'same'-padded convolution of the image ``xi [N, cin_pad, H, W]`` in fp32 -> fp32 token rows (the caller rounds)."""
    w, b = P[name]
    kh, kw = w.shape[2:]
    return tok(F.conv2d(xi, w, b, stride=stride, padding=((kh - 1) // 2, (kw - 1) // 2)))


def conv(P, name, x, N, H, W, stride=1):
    return conv_img(P, name, img(x[:, :P[name][0].shape[1]], N, H, W), stride)


def pooled(P, name, a, act):
    """``vface_pooled_linear`` on fp32 ``a [nimg, K]``: the fp64 sum rounded once to fp32, then the activation in fp32."""
    w, b = P[name]
    pre = a.double() @ w.double().T
    if b is not None:
        pre = pre + b.double()
    pre = pre.float()
    return {"none": lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid}[act](pre)


def gated(x, g, hw, r=None):
    """``vface_channel_gate``: x g[image] + r, one fp32 fma (the fp64 value rounded once to fp32); the caller rounds to ``dt``."""
    y = x.double() * g.double().repeat_interleave(hw, 0)
    return (y if r is None else y + r.double()).float()


@torch.no_grad()
def engine_taps(sd, crops, dt, defect=None, *, x8=None, geom=None, step=None):
    """``ParseEngine.logits(prefilter(crops))`` on the CPU -> dict tap name -> tensor (token rows, 16-bit buffers as fp32 holding
    values of ``dt``), with ``_geom`` = dict(F, H, W).  ``crops``: uint8 ``[F, 2H, 2W, 3]``; or ``x8 [F H W, 8]`` with ``geom`` =
    (F, H, W): the rows of an existing pre-filter output.  ``step``: frames per stem chunk (None: one chunk)."""
    assert defect is None or defect in DEFECTS, defect
    r = rounder(dt)
    P = weights(sd, dt, defect)
    taps = {}

    def tap(name, t):
        taps[name] = t.detach().clone()

    if x8 is None:
        u8 = np.asarray(crops)
        Fn, H, W = u8.shape[0], u8.shape[1] // 2, u8.shape[2] // 2
        x8 = F.pad(r(torch.from_numpy(prefilter(u8, np.float32)).reshape(-1, 3)), (0, 5))
    else:
        Fn, H, W = geom
        x8 = x8.float()
    taps["_geom"] = dict(F=Fn, H=H, W=W)
    tap("x8", x8)

    def means(x, hw, name):
        x64 = x.double().reshape(Fn, hw, -1)
        m = x64.sum(1) if defect == "mean_is_sum" else x64.mean(1)
        if defect == "mean_by_other_levels_hw" and name == "cp.arm16.mean":
            m = x64.sum(1) / ((H // 32) * (W // 32))
        st = torch.stack([m, 1.0 / torch.sqrt(x64.var(1, unbiased=False) + EPS32)], -1).float()
        if defect == "mean_rounded_to_16bit":
            st = r(st)
        tap(name, st)
        return st

    # stem
    h2, w2 = H // 2, W // 2
    step = step or Fn
    x = torch.zeros(Fn * h2 * w2, 64)
    for f0 in range(0, Fn, step):
        n = min(step, Fn - f0)
        src = 0 if (defect == "stem_chunk2_reads_frame0" and f0) else f0
        dst = 0 if (defect == "stem_chunk2_over_chunk1" and f0) else f0
        x[dst * h2 * w2:(dst + n) * h2 * w2] = r(conv(P, f"{R}.conv1", x8[src * H * W:(src + n) * H * W], n, H, W, 2))
    tap(f"{R}.conv1", x)
    x = torch.relu(x)
    tap(f"{R}.conv1.act", x)
    xi = img(x, Fn, h2, w2)
    x = tok(F.max_pool2d(xi, 2, 2) if defect == "maxpool_window_2x2" else F.max_pool2d(xi, 3, 2, 1))
    tap(f"{R}.maxpool", x)
    h, w = h2 // 2, w2 // 2
    feats, cat = {}, None
    for li, (cout, stride) in enumerate(LAYERS, start=1):
        for bi in (0, 1):
            b = f"{R}.layer{li}.{bi}"
            st = stride if bi == 0 else 1
            oh, ow = (h - 1) // st + 1, (w - 1) // st + 1
            t = r(conv(P, f"{b}.conv1", x, Fn, h, w, st))
            tap(f"{b}.conv1", t)
            t = torch.relu(t)
            tap(f"{b}.conv1.act", t)
            t2 = r(conv(P, f"{b}.conv2", t, Fn, oh, ow))
            tap(f"{b}.conv2", t2)
            res = t if defect == "residual_from_conv1" else t2
            if f"{b}.downsample.0" in P:
                s = r(conv(P, f"{b}.downsample.0", x, Fn, h, w, st))
                tap(f"{b}.downsample.0", s)
                y = r(torch.relu(s + res))
            elif defect == "identity_shortcut_dropped":
                y = r(torch.relu(res))
            else:
                y = r(torch.relu(x + res))
            if li == 2 and bi == 1:
                cat = torch.zeros(Fn * oh * ow, 256)
                if defect in ("feat8_in_right_half", "cat_halves_swapped"):
                    cat[:, 128:] = y
                else:
                    cat[:, :128] = y
            tap(f"{b}.sum", y)
            x = y
            tap(f"{b}.out", x)
            h, w = oh, ow
        feats[li] = (x, h, w)
    (f8, h8, w8), (f16, h16, w16), (f32_, h32, w32) = feats[2], feats[3], feats[4]

    def arm(name, v, hh, ww, rvec=None, rten=None):
        hw = hh * ww
        feat = r(conv(P, f"{name}.conv.conv", v, Fn, hh, ww))
        tap(f"{name}.conv", feat)
        feat = torch.relu(feat)
        tap(f"{name}.conv.act", feat)
        st = means(feat, hw, f"{name}.mean")
        g = pooled(P, f"{name}.conv_atten", st[..., 0], "relu" if defect == "arm_gate_relu" else "sigmoid")
        tap(f"{name}.conv_atten", g)
        if defect == "gate_of_frame0":
            g = g[:1].expand_as(g)
        add = rten
        if rvec is not None:
            rv = rvec[:1].expand_as(rvec) if defect == "avg_of_frame0" else rvec
            add = None if defect == "arm32_without_avg" else rv.repeat_interleave(hw, 0)
        if defect == "arm16_adds_before_gating" and rten is not None:
            out = r(gated(feat + rten, g, hw))
        else:
            out = r(gated(feat, g, hw, add))
        tap(f"{name}.out", out)
        return out

    def head(name, v, hh, ww):
        vi = img(v, Fn, hh, ww)
        if defect == "head_upsample_rows_cols_exchanged":
            up = vi.transpose(2, 3).repeat_interleave(2, 2).repeat_interleave(2, 3).reshape(Fn, -1, 2 * hh, 2 * ww)
        else:
            up = vi.repeat_interleave(2, 2).repeat_interleave(2, 3)
        return r(conv_img(P, name, up))

    avg = pooled(P, "cp.conv_avg.conv", means(f32_, h32 * w32, "cp.avg.mean")[..., 0], "relu")
    tap("cp.conv_avg", avg)
    s32 = arm("cp.arm32", f32_, h32, w32, rvec=avg)
    up32 = head("cp.conv_head32.conv", s32, h32, w32)
    tap("cp.conv_head32", up32)
    up32 = torch.relu(up32)
    tap("cp.conv_head32.act", up32)
    s16 = arm("cp.arm16", f16, h16, w16, rten=up32)
    pre = head("cp.conv_head16.conv", s16, h16, w16)
    slot = cat[:, :128] if defect == "cat_halves_swapped" else cat[:, 128:]
    slot.copy_(pre)
    tap("cp.conv_head16", slot)
    tap("cp.conv_head16.act", torch.relu(pre))
    if defect != "cat_right_half_without_relu":
        slot.copy_(torch.relu(pre))
    tap("ffm.cat", cat)
    hw8 = h8 * w8
    feat = r(conv(P, "ffm.convblk.conv", cat, Fn, h8, w8))
    tap("ffm.convblk", feat)
    feat = torch.relu(feat)
    tap("ffm.convblk.act", feat)
    a1 = pooled(P, "ffm.conv1", means(feat, hw8, "ffm.mean")[..., 0], "none" if defect == "ffm_conv1_without_relu" else "relu")
    tap("ffm.conv1", a1)
    a2 = pooled(P, "ffm.conv2", a1, "sigmoid")
    tap("ffm.conv2", a2)
    feat = r(gated(feat, a2, hw8, None if defect == "ffm_without_plus_feat" else feat))
    tap("ffm.out", feat)
    mid = r(conv(P, "conv_out.conv.conv", feat, Fn, h8, w8))
    tap("conv_out.conv", mid)
    if defect != "conv_out_without_relu":
        mid = torch.relu(mid)
    tap("conv_out.conv.act", mid)
    lg = conv(P, "conv_out.conv_out", mid, Fn, h8, w8)
    if defect == "logits_rounded_to_16bit":
        lg = r(lg)
    tap("logits", lg)
    return taps
