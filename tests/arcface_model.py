"""``vface_amd.arcface.ArcFaceEngine`` restated on the CPU in torch: fp64 arithmetic with a rounding to the 16-bit compute type at
every point where the engine stores a tensor -- the network's input rows, the packed weights, every convolution's output, the PReLU's
output, the gated sum ``y`` and the leading BatchNorm ``z`` (both from the UNROUNDED sum), the head's operand -- and fp32-or-better
everywhere the engine keeps fp32 (biases, the squeeze-excite vectors, the head's output, the norm).  ``dt=None`` rounds nothing: that
is the fold itself in fp64, which must reproduce the reference's double run.  What it does not restate is the order of fp32 additions
inside a convolution.  Its error against the fixture's double run, times ``MARGIN``, is the GPU tests' tolerance; ``defect`` seeds the
one-line mistakes test_arcface_bound_cpu.py must see past that tolerance.  ``bins`` / ``prep_twin`` are the host twin of
``vface_id_prep``.  Plain functions, nothing collected by pytest."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

from vface_amd.arcface import BN_EPS, UNITS, bn_pair, fold_head
from vface_amd.convnet import fold_bn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases_arcface as ca  # noqa: E402
import cases_clip as cc  # noqa: E402

MARGIN = 1.25
DEFECTS = ("relu_for_prelu", "gate_omitted", "shortcut_unstrided", "lead_bn_folded", "flatten_not_permuted", "bn1d_dropped",
           "no_l2norm", "pool_bin_off_by_one")
UNIT_DEFECTS = ("relu_for_prelu", "gate_omitted", "shortcut_unstrided", "lead_bn_folded")
CLIP_MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073], dtype=torch.float32).double()
CLIP_STD = torch.tensor([0.26862954, 0.26130258, 0.27577711], dtype=torch.float32).double()
CLIP_MEAN_DECIMAL = torch.tensor([0.48145466, 0.4578275, 0.40821073], dtype=torch.float64)
CLIP_STD_DECIMAL = torch.tensor([0.26862954, 0.26130258, 0.27577711], dtype=torch.float64)
POOL, Y0, X0, CROP, OUT = 256, 35, 32, 188, 112


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def q(x, dt):
    return x if dt is None else x.to(dt).to(x.dtype)


# ---- the host twin of vface_id_prep ------------------------------------------------------------------------------------------------
def bins(n_in: int, n_out: int):
    """PyTorch's adaptive pooling bins in integers: [(floor(i In / Out), ceil((i + 1) In / Out))]."""
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def pool_matrix(n_in: int, n_out: int, shift=None) -> torch.Tensor:
    """fp64 [n_out, n_in]: row i averages its bin.  ``shift = (i, end, d)``: bin i's lower (end 0) or upper (end 1) edge moved by d;
    ``shift = "floor"``: every upper edge floor((i + 1) In / Out) where it should be the ceiling -- one short wherever the division
    is inexact."""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i, (a, b) in enumerate(bins(n_in, n_out)):
        if shift == "floor":
            b = max(((i + 1) * n_in) // n_out, a + 1)
            shift_i = None
        else:
            shift_i = shift
        if shift_i is not None and shift_i[0] == i:
            a, b = (a + shift_i[2], b) if shift_i[1] == 0 else (a, b + shift_i[2])
            a, b = max(a, 0), min(b, n_in)
        m[i, a:b] = 1.0 / (b - a)
    return m


def adaptive_pool(x, out_hw, shift_y=None, shift_x=None):
    """AdaptiveAvgPool2d as two matrices (a bin's mean is separable); the shifts seed an edge defect."""
    py = pool_matrix(x.shape[2], out_hw[0], shift_y).to(x.dtype)
    px = pool_matrix(x.shape[3], out_hw[1], shift_x).to(x.dtype)
    return torch.einsum("ih,bchw,jw->bcij", py, x, px)


def prep_twin(x, clip_img=True, shift1=None, shift2=None, decimal_constants=False):
    """ddpm.py:114-119 on ``x [B, 3, H, W]`` in its own dtype, from the integer bin tables.  ``shift1`` / ``shift2``: a moved edge
    of the 256-pool's / the 112-pool's rows.  ``un_norm_clip``'s constants are Python floats: on an fp32 tensor they act as their
    fp32 roundings (the kernel's constants, the default here), on the double run's tensor as the decimals themselves
    (``decimal_constants``: what the fixture's ``feat64`` was computed with; 3e-8 apart)."""
    if clip_img:
        mean, std = (CLIP_MEAN_DECIMAL, CLIP_STD_DECIMAL) if decimal_constants else (CLIP_MEAN, CLIP_STD)
        x = ((x * std.to(x.dtype).view(1, 3, 1, 1) + mean.to(x.dtype).view(1, 3, 1, 1)) - 0.5) / 0.5
    if x.shape[2] != POOL:
        x = adaptive_pool(x, (POOL, POOL), shift1)
    return adaptive_pool(x[:, :, Y0:Y0 + CROP, X0:X0 + CROP], (OUT, OUT), shift2)


# ---- one unit ----------------------------------------------------------------------------------------------------------------------
def prelu(t, slope):
    return torch.where(t > 0, t, slope.view(1, -1, 1, 1) * t)


def f32(v, dt):
    """A vector the engine keeps in fp32 (``dt=None``: the fold itself, nothing is rounded)."""
    return v if dt is None else v.float().double()


def unit(sd, u, x, y32, cin, depth, stride, dt, nxt=None, defect=None):
    """``x``: the unit's stored input, ``y32``: the unrounded value it was rounded from (the leading BatchNorm reads that one).
    Returns ``(y, y32)`` of the unit's output."""
    r = f"{u}.res_layer"
    a, b = (f32(v, dt) for v in bn_pair(sd, f"{r}.0", BN_EPS))
    w1 = sd[f"{r}.1.weight"]
    if defect == "lead_bn_folded":      # folded into the convolution: the zero padding then carries no shift
        wf = w1 * a.view(1, -1, 1, 1)
        t = F.conv2d(x, q(wf, dt), (w1 * b.view(1, -1, 1, 1)).sum((1, 2, 3)), padding=1)
    else:
        z = q(a.view(1, -1, 1, 1) * y32 + b.view(1, -1, 1, 1), dt)
        t = F.conv2d(z, q(w1, dt), padding=1)
    t = q(t, dt)
    slope = f32(sd[f"{r}.2.weight"], dt)
    t = q(prelu(t, torch.zeros_like(slope) if defect == "relu_for_prelu" else slope), dt)
    w2, b2 = fold_bn(sd[f"{r}.3.weight"], sd[f"{r}.4.weight"], sd[f"{r}.4.bias"], sd[f"{r}.4.running_mean"], sd[f"{r}.4.running_var"],
                     BN_EPS)
    res = q(F.conv2d(t, q(w2, dt), f32(b2, dt), stride=stride, padding=1), dt)
    h = F.relu(F.conv2d(res.mean((2, 3), keepdim=True), f32(sd[f"{r}.5.fc1.weight"], dt)))
    g = torch.sigmoid(F.conv2d(h, f32(sd[f"{r}.5.fc2.weight"], dt)))
    if defect == "gate_omitted":
        g = torch.ones_like(g)
    s = f"{u}.shortcut_layer"
    if f"{s}.0.weight" in sd:
        ws, bs = fold_bn(sd[f"{s}.0.weight"], sd[f"{s}.1.weight"], sd[f"{s}.1.bias"], sd[f"{s}.1.running_mean"],
                         sd[f"{s}.1.running_var"], BN_EPS)
        sc = q(F.conv2d(x, q(ws, dt), f32(bs, dt), stride=stride), dt)
    elif defect == "shortcut_unstrided":
        sc = x[:, :, :res.shape[2], :res.shape[3]]
    else:
        sc = x[:, :, ::stride, ::stride]
    out32 = res * g + sc
    return q(out32, dt), out32


@torch.no_grad()
def run_unit(sd, u, x, cin, depth, stride, dt=None, defect=None):
    """One ``bottleneck_IR_SE`` on a stored input ``x [N, cin, H, W]`` (rounded to ``dt`` first, as the engine is handed it)."""
    sd = {k: v.double() for k, v in sd.items() if torch.is_floating_point(v)}
    x = q(x.double(), dt)
    return unit(sd, u, x, x, cin, depth, stride, dt, defect=defect)[0]


# ---- the network -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def features(sd, x, dt=None, defect=None, normalise=True):
    """``x [B, 3, 112, 112]`` (the network's input) -> fp64 [B, 512]."""
    sd = {k: v.double() for k, v in sd.items() if torch.is_floating_point(v)}
    x = q(x.double(), dt)
    w, b = fold_bn(sd["input_layer.0.weight"], sd["input_layer.1.weight"], sd["input_layer.1.bias"], sd["input_layer.1.running_mean"],
                   sd["input_layer.1.running_var"], BN_EPS)
    t = q(F.conv2d(x, q(w, dt), f32(b, dt), padding=1), dt)
    slope = f32(sd["input_layer.2.weight"], dt)
    y32 = prelu(t, torch.zeros_like(slope) if defect == "relu_for_prelu" else slope)
    y = q(y32, dt)
    for i, (cin, depth, stride) in enumerate(UNITS):
        y, y32 = unit(sd, f"body.{i}", y, y32, cin, depth, stride, dt, defect=defect if defect in UNIT_DEFECTS else None)
    B = y.shape[0]
    if defect == "bn1d_dropped":
        sd = dict(sd)
        sd["output_layer.4.running_mean"] = torch.zeros_like(sd["output_layer.4.running_mean"])
        sd["output_layer.4.running_var"] = torch.ones_like(sd["output_layer.4.running_var"]) - BN_EPS
        sd.pop("output_layer.4.weight", None)
        sd.pop("output_layer.4.bias", None)
    wh, bh = fold_head(sd)
    tok = y.permute(0, 2, 3, 1).reshape(B, -1)          # the engine's rows: p 512 + c
    if defect == "flatten_not_permuted":
        tok = y.reshape(B, -1)                          # c 49 + p against columns in the other order
    raw = f32(tok @ q(wh, dt).T + f32(bh, dt), dt)      # the head's output is fp32
    if not normalise or defect == "no_l2norm":
        return raw
    return raw / raw.norm(dim=1, keepdim=True)


@torch.no_grad()
def extract(sd, img, dt=None, defect=None, clip_img=True, decimal_constants=False):
    """``extract_feats`` from the image the chain sees, ``[B, 3, H, W]``."""
    shift = "floor" if defect == "pool_bin_off_by_one" else None          # the 112-pool's upper row edges: floor for ceil
    return features(sd, prep_twin(img.double(), clip_img, shift2=shift, decimal_constants=decimal_constants), dt, defect)


# ---- the fixture's cases (weights and inputs by seed, tests/golden/cases_arcface.py) ------------------------------------------------


@functools.lru_cache(maxsize=None)
def network():
    """The mirror ``Backbone`` as ``IDLoss`` builds it, with the fixture's weights (on the CPU)."""
    from vface_amd.src.Face_models.encoders.model_irse import Backbone
    from vface_amd.utils import synth
    return synth.fill_arcface_(Backbone(input_size=112, num_layers=50, mode="ir_se", drop_ratio=0.6), seed=ca.WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def unit_case(name):
    """``(state dict under 'u.', input fp32 [N, cin, H, W], (cin, depth, stride, H, W, N))`` of a unit case."""
    from vface_amd.src.Face_models.encoders.model_irse import bottleneck_IR_SE
    from vface_amd.utils import synth
    cin, depth, stride, H, W, n, _ = ca.UNIT_CASES[name]
    m = synth.fill_arcface_(bottleneck_IR_SE(cin, depth, stride), seed=ca.WEIGHT_SEED, prefix=ca.unit_prefix(name))
    return {"u." + k: v for k, v in m.state_dict().items()}, torch.from_numpy(ca.unit_input(name)), (cin, depth, stride, H, W, n)


@functools.lru_cache(maxsize=None)
def frames():
    return torch.from_numpy(cc.frames(ca.FRAMES))


@functools.lru_cache(maxsize=None)
def emulated(dt, defect=None):
    """fp64 [B, 512]: the emulation on the fixture's network input (``prep``), or for the pooling defect from the CLIP image."""
    from conftest import load_golden
    sd = network().state_dict()
    if defect == "pool_bin_off_by_one":
        import clip_bounds as cb
        return extract(sd, cb.prep_ref(frames(), None, 224), dt, defect)
    return features(sd, load_golden("arcface")["prep"], dt, defect)
