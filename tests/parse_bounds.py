"""``check_stage``: one stage of the face parser (vface_amd/parsing.py, ``ParseEngine.logits``) against fp64, per element, from the
taps of a run -- the engine's on the GPU (test_parse_stages_gpu.py) or ``parse_model.engine_taps``'s on the CPU
(test_parse_bound_cpu.py: the clean model passes every stage, twenty-three one-line defects are each refused at the stage that owns
them).

For each launch of the stage the checker
1. assembles the launch's input FROM THE TAPS OF THE PRODUCING LAUNCHES -- never from the buffer the consuming launch reads: the
   rows ``ffm.convblk`` multiplies are ``cat[layer2.1.out tap | cp.conv_head16.act tap]`` built here, and the ``ffm.cat`` tap is
   separately asserted equal to that assembly, so a misplaced or stale half shows;
2. computes the launch in fp64 from those values and the weights as the engine packs them (BatchNorm folded in fp64, rounded to
   the compute type, padded: ``parse_model.weights``) and bounds it per element with kernel_bounds.py's derived bounds:
   ``conv_ref_and_bound`` for the 3 x 3 launches (``upsample=True`` for the two head convolutions) with the split count of
   ``vface_splitk_workspace_bytes`` -- they do go through the split-K rules, by per-sample geometry; ``conv_ref_and_bound`` /
   ``gemm_ref_and_bound`` with ``splits=1`` for the windows (``ParseEngine.split_k = False``), ``out_f32`` for the class head;
   the mean half of ``channel_stats_ref_and_bound``; ``norm_act_pre_ref_and_bound`` + ``act_ref_and_bound`` for the residual sums;
   ``pooled_linear_ref_and_bound`` and ``channel_gate_ref_and_bound``;
3. asserts bit-exact identities where the arithmetic is exact: ReLU in place, the max-pool of the tapped input, a block's output
   against its last launch's tap, the ``cat`` buffer, the zero columns 19..31 of the logits.
``note()`` prints the headroom per family; no threshold is made from it.

Taps: a dict name -> CPU tensor under the names ``ParseEngine.logits`` documents (token rows ``[M, C]``; 16-bit buffers in their own
type or as fp32 holding its values); ``taps["_geom"]`` = dict(F, H, W).  Plain functions, nothing collected by pytest."""
import sys

import numpy as np
import torch
import torch.nn.functional as F

import parse_model as pm
from conftest import GOLDEN
from kernel_bounds import (act_ref_and_bound, assert_within, channel_gate_ref_and_bound, channel_stats_ref_and_bound, conv_ref_and_bound,
                           gemm_ref_and_bound, norm_act_pre_ref_and_bound, note, pooled_linear_ref_and_bound)
from parse_model import EPS32, R, img
from raft_bounds import _eq, splits_of
from vface_amd.parsing import LAYERS, N_CLASSES

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import cases_parse as cp  # noqa: E402

BLOCKS = [f"layer{li}.{bi}" for li in (1, 2, 3, 4) for bi in (0, 1)]


def stages():
    return ["stem"] + BLOCKS + ["avg", "arm32", "head32", "arm16", "head16", "ffm", "out"]


def _f32_flag():
    from vface_amd import hip
    return hip.EPI_OUT_F32


def _conv3(fam, what, P, name, x, N, H, W, got, dt, stride=1, upsample=False):
    """One ``conv3`` launch (3 x 3, stride 1 / 2, or the nearest x2 upsampling in front) from its input rows ``x``."""
    w, b = P[name]
    cout, cin = w.shape[:2]
    vh, vw = (2 * H, 2 * W) if upsample else (H, W)
    M = N * ((vh - 1) // stride + 1) * ((vw - 1) // stride + 1)
    ref, bound = conv_ref_and_bound(img(x.float()[:, :cin], N, H, W), w, dt, stride=stride, upsample=upsample, bias=b,
                                    splits=splits_of(M, cout, 9 * cin, 0, M // N))
    note(fam, assert_within(got, ref, bound, what), bound)


def _window(fam, what, P, name, x, N, H, W, got, dt, stride=1, out_f32=False):
    """One ``window`` launch (im2col + GEMM, or the plain GEMM of a 1 x 1 stride-1 window); ``split_k = False``: one share."""
    w, b = P[name]
    cout, cin, kh, kw = w.shape
    if kh == kw == 1 and stride == 1:
        ref, bound = gemm_ref_and_bound(x.float()[:, :cin], w.reshape(cout, cin), dt, bias=b, out_f32=out_f32, splits=1)
    else:
        ref, bound = conv_ref_and_bound(img(x.float()[:, :cin], N, H, W), w, dt, stride=stride,
                                        pad=((kh - 1) // 2, (kh - 1) // 2, (kw - 1) // 2, (kw - 1) // 2), bias=b, out_f32=out_f32, splits=1)
    note(fam, assert_within(got, ref, bound, what), bound)


def _relu_in_place(taps, pre, post):
    _eq(taps[post], torch.relu(taps[pre].float()), f"{post}: ReLU in place is exact")


def _mean(taps, name, x, N, hw):
    """The mean half of ``vface_channel_stats`` against fp64 of the stored rows ``x``."""
    ref, bound = channel_stats_ref_and_bound(x.double().reshape(N, hw, -1), EPS32)
    got = taps[name]
    assert tuple(got.shape) == tuple(ref.shape), (name, got.shape, ref.shape)
    note("parse mean", assert_within(got[..., 0], ref[..., 0], bound[..., 0], name), bound[..., 0])


def _pooled(taps, P, name, a, tapname, act):
    w, b = P[name]
    ref, bound = pooled_linear_ref_and_bound(a.float(), w, b, act)
    note(f"parse pooled_linear {act}", assert_within(taps[tapname], ref, bound, tapname), bound)


def _gate(taps, name, x, g, hw, dt, **kw):
    ref, bound = channel_gate_ref_and_bound(x, g.float(), hw, dt, **kw)
    note("parse channel_gate", assert_within(taps[name], ref, bound, name), bound)


def _arm(taps, P, dt, arm, x, N, H, W, **r):
    hw = H * W
    _conv3("parse conv3x3", f"{arm}.conv", P, f"{arm}.conv.conv", x, N, H, W, taps[f"{arm}.conv"], dt)
    _relu_in_place(taps, f"{arm}.conv", f"{arm}.conv.act")
    _mean(taps, f"{arm}.mean", taps[f"{arm}.conv.act"], N, hw)
    _pooled(taps, P, f"{arm}.conv_atten", taps[f"{arm}.mean"][..., 0], f"{arm}.conv_atten", "sigmoid")
    _gate(taps, f"{arm}.out", taps[f"{arm}.conv.act"], taps[f"{arm}.conv_atten"], hw, dt, **r)


def geometry(H, W):
    """(h, w) of the maps: after the stem, after the max-pool, and of layer1..4."""
    h2, w2 = H // 2, W // 2
    g = {"stem": (h2, w2), "pool": (h2 // 2, w2 // 2)}
    h, w = g["pool"]
    for li, (_, stride) in enumerate(LAYERS, start=1):
        h, w = (h - 1) // stride + 1, (w - 1) // stride + 1
        g[li] = (h, w)
    return g


def check_stage(taps, sd, dt, stage):
    """Raises AssertionError (naming the launch and the worst element) if ``stage`` of the run that left ``taps`` is out of bound."""
    P = _weights(sd, dt)
    g = taps["_geom"]
    N, H, W = g["F"], g["H"], g["W"]
    geo = geometry(H, W)
    (h8, w8), (h16, w16), (h32, w32) = geo[2], geo[3], geo[4]
    if stage == "stem":
        x8 = taps["x8"]
        assert tuple(x8.shape) == (N * H * W, 8)
        _eq(x8[:, 3:], torch.zeros(N * H * W, 5), "x8: channels 3..7 are zero")
        h2, w2 = geo["stem"]
        _window("parse stem 7x7", f"{R}.conv1", P, f"{R}.conv1", x8, N, H, W, taps[f"{R}.conv1"], dt, stride=2)
        _relu_in_place(taps, f"{R}.conv1", f"{R}.conv1.act")
        want = pm.tok(F.max_pool2d(img(taps[f"{R}.conv1.act"].float(), N, h2, w2), 3, 2, 1))
        _eq(taps[f"{R}.maxpool"], want, f"{R}.maxpool: a maximum is one of its inputs")
    elif stage in BLOCKS:
        h, w = geo["pool"]
        prev = f"{R}.maxpool"
        for li, (cout, stride) in enumerate(LAYERS, start=1):
            for bi in (0, 1):
                b = f"{R}.layer{li}.{bi}"
                st = stride if bi == 0 else 1
                oh, ow = (h - 1) // st + 1, (w - 1) // st + 1
                if stage == f"layer{li}.{bi}":
                    x = taps[prev]
                    _conv3("parse conv3x3", f"{b}.conv1", P, f"{b}.conv1", x, N, h, w, taps[f"{b}.conv1"], dt, stride=st)
                    _relu_in_place(taps, f"{b}.conv1", f"{b}.conv1.act")
                    _conv3("parse conv3x3", f"{b}.conv2", P, f"{b}.conv2", taps[f"{b}.conv1.act"], N, oh, ow, taps[f"{b}.conv2"], dt)
                    short = x
                    if f"{b}.downsample.0" in P:
                        _window("parse 1x1 stride 2", f"{b}.downsample.0", P, f"{b}.downsample.0", x, N, h, w, taps[f"{b}.downsample.0"], dt,
                                stride=st)
                        short = taps[f"{b}.downsample.0"]
                    v, dv = norm_act_pre_ref_and_bound(short.double(), None, taps[f"{b}.conv2"].double(), oh * ow)
                    ref, bound = act_ref_and_bound(v, dv, "relu", dt)
                    note("parse residual sum", assert_within(taps[f"{b}.sum"], ref, bound, f"{b}.sum"), bound)
                    _eq(taps[f"{b}.out"], taps[f"{b}.sum"], f"{b}.out")
                    return
                h, w, prev = oh, ow, f"{b}.out"
    elif stage == "avg":
        _mean(taps, "cp.avg.mean", taps[f"{R}.layer4.1.out"], N, h32 * w32)
        _pooled(taps, P, "cp.conv_avg.conv", taps["cp.avg.mean"][..., 0], "cp.conv_avg", "relu")
    elif stage == "arm32":
        _arm(taps, P, dt, "cp.arm32", taps[f"{R}.layer4.1.out"], N, h32, w32, rvec=taps["cp.conv_avg"].float())
    elif stage == "head32":
        _conv3("parse head conv3x3 upsample", "cp.conv_head32", P, "cp.conv_head32.conv", taps["cp.arm32.out"], N, h32, w32, taps["cp.conv_head32"],
               dt, upsample=True)
        _relu_in_place(taps, "cp.conv_head32", "cp.conv_head32.act")
    elif stage == "arm16":
        _arm(taps, P, dt, "cp.arm16", taps[f"{R}.layer3.1.out"], N, h16, w16, rten=taps["cp.conv_head32.act"])
    elif stage == "head16":
        _conv3("parse head conv3x3 upsample", "cp.conv_head16", P, "cp.conv_head16.conv", taps["cp.arm16.out"], N, h16, w16, taps["cp.conv_head16"],
               dt, upsample=True)
        _relu_in_place(taps, "cp.conv_head16", "cp.conv_head16.act")
    elif stage == "ffm":
        hw = h8 * w8
        cat = torch.cat([taps[f"{R}.layer2.1.out"].float(), taps["cp.conv_head16.act"].float()], 1)
        _eq(taps["ffm.cat"], cat, "ffm.cat == cat[layer2.1.out | relu(conv_head16)]")
        _window("parse 1x1", "ffm.convblk", P, "ffm.convblk.conv", cat, N, h8, w8, taps["ffm.convblk"], dt)
        _relu_in_place(taps, "ffm.convblk", "ffm.convblk.act")
        _mean(taps, "ffm.mean", taps["ffm.convblk.act"], N, hw)
        _pooled(taps, P, "ffm.conv1", taps["ffm.mean"][..., 0], "ffm.conv1", "relu")
        _pooled(taps, P, "ffm.conv2", taps["ffm.conv1"], "ffm.conv2", "sigmoid")
        _gate(taps, "ffm.out", taps["ffm.convblk.act"], taps["ffm.conv2"], hw, dt, add_x=True)
    elif stage == "out":
        M = N * h8 * w8
        _conv3("parse conv3x3", "conv_out.conv", P, "conv_out.conv.conv", taps["ffm.out"], N, h8, w8, taps["conv_out.conv"], dt)
        _relu_in_place(taps, "conv_out.conv", "conv_out.conv.act")
        lg = taps["logits"]
        assert lg.dtype == torch.float32 and tuple(lg.shape) == (M, 32), (lg.dtype, lg.shape)
        assert splits_of(M, 32, 256, _f32_flag()) == 1, "an fp32-output launch never splits K"
        _window("parse class head 1x1 f32", "logits", P, "conv_out.conv_out", taps["conv_out.conv.act"], N, h8, w8, lg, dt, out_f32=True)
        n = N_CLASSES
        _eq(lg[:, n:], torch.zeros(M, 32 - n), f"logits columns {n}..31 (zero weights) are zero")
    else:
        raise KeyError(stage)


_W = {}


def _weights(sd, dt):
    key = (id(sd), dt)
    if key not in _W:
        _W.clear()
        _W[key] = (sd, pm.weights(sd, dt))
    return _W[key][1]


def first_failing_stage(taps, sd, dt, stage_list=None):
    """The first stage that ``check_stage`` refuses, with its message; (None, None) if all pass."""
    for s in stage_list or stages():
        try:
            check_stage(taps, sd, dt, s)
        except AssertionError as e:
            return s, str(e)
    return None, None


# ------------------------------------------------------------------------------------------------ the cases of both test files
# wide: network input 96 x 64 -- maps 48 x 32, 24 x 16, 12 x 8, 6 x 4, 3 x 2: non-square, hw = 6 at layer 4; the stem's window budget
# holds 2.5 frames' window matrices (one is 48 * 32 * 392 * 2 bytes), so the stem runs as chunks of 2 + 1 frames.
# small: 64 x 64, the smallest input the engine accepts: layer 4 is 2 x 2 (M = 12), layer 2 is 8 x 8.
CASES = {"wide": dict(F=3, H=96, W=64, seeds=(51, 52, 53), budget=int(2.5 * 48 * 32 * 392 * 2)),
         "small": dict(F=3, H=64, W=64, seeds=(54, 55, 56), budget=None)}


def stem_step(case):
    """Frames per stem chunk, by ``ParseEngine.logits``'s rule."""
    c = CASES[case]
    if c["budget"] is None:
        return c["F"]
    return max(1, min(c["F"], c["budget"] // ((c["H"] // 2) * (c["W"] // 2) * 392 * 2)))


def base_sd():
    """test_parse_gpu.py's synthetic weights."""
    from vface_amd.pretrained.face_parsing import BiSeNet
    from vface_amd.utils import synth
    net = BiSeNet(n_classes=cp.N_CLASSES)
    synth.fill_parser_(net, seed=cp.WEIGHT_SEED)
    return net.state_dict()


def crops(case):
    """uint8 [F, 2H, 2W, 3]: ``cases_parse.crop`` with the case's three seeds."""
    c = CASES[case]
    return np.stack([cp.crop(c["H"], c["W"], s) for s in c["seeds"]])


class Taps(dict):
    """tap(name, tensor) -> a CPU clone under ``name``."""

    def __call__(self, name, t):
        self[name] = t.detach().cpu().clone()


def model_taps(case, sd, dt, defect=None):
    """tests/parse_model.py's ``engine_taps`` on a case (the stem chunked as the engine chunks it)."""
    return pm.engine_taps(sd, crops(case), dt, defect, step=stem_step(case))
