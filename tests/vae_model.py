"""CPU emulation of ``vface_amd.vae_engine.VAEEngine``: every stage restated in fp32 torch, rounded to the 16-bit compute type
exactly where the engine stores 16 bits -- the 8-channel input, every convolution output (after its residual add, which the epilogue
makes in fp32), every GroupNorm-apply output, q | k, V^T, the probabilities P, the attention output, the ``nin_shortcut`` output and
the 8-column ``post_quant`` output -- and kept in fp32 where the engine keeps fp32: the scores, the moments and the decoder's last
convolution.  The weights are the engine's own: ``vae_engine.pack_state_dict`` / ``Packer`` with the CPU as device (16-bit packed
weights, fp32 biases, the fp64 ``quant_conv o conv_out`` fold, the 8 x 8 ``post_quant``), unpacked here from the kernels' K order.
What it does not restate is the order of fp32 additions inside a GEMM, a convolution or a GroupNorm.

Its error against fp64 -- rel-L2 and the worst element's |err| / rms(ref) -- times ``MARGIN_L2`` / ``MARGIN_WORST`` is the tolerance
of test_vae_stages_gpu.py; ``defect`` seeds the one-line mistakes test_vae_bound_cpu.py must see past that tolerance.  ``STAGES``
are the stage cases both files run (same inputs, same weights, same fp64 reference).  Plain functions, nothing collected by pytest."""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import cases_vae as cv  # noqa: E402
from oracle import vae as ovae  # noqa: E402
from vface_amd import vae_engine as ve  # noqa: E402
from vface_amd.engine import _phase_form_pays  # noqa: E402
from vface_amd.utils import synth  # noqa: E402

MARGIN_L2 = 1.25      # rel-L2: the project's allowance over an emulation (test_clip_gpu.py) -- fp32 accumulation order, BLAS against MFMA
MARGIN_WORST = 2.0    # the worst element: an extreme-value statistic of the same distribution; which element the order hits moves it
DTS = (torch.float16, torch.bfloat16)
DEFECTS = ("attn_scale_n", "softmax_over_queries", "p_times_k", "value_bias_dropped", "downsample_leading_pad", "gn_eps_1e5",
           "fold_bias_term_dropped", "post_quant_bias_into_conv_in", "residual_after_norm1", "upsample_phases_swapped",
           "no_swish_before_conv_out")
SPECS = {"small": ovae.VAESpec(ch=32, resolution=32), "ffhq": ovae.FFHQ_VAE}


def rounder(dt):
    return (lambda t: t) if dt == torch.float32 else (lambda t: t.to(dt).float())


def figures(got, ref64):
    """``(rel-L2, worst |err| / rms(ref))`` of ``got`` against the fp64 reference."""
    e = got.double().flatten() - ref64.double().flatten()
    rms = float(ref64.double().flatten().norm()) / math.sqrt(ref64.numel())
    return float(e.norm()) / (rms * math.sqrt(ref64.numel())), float(e.abs().max()) / rms


# ------------------------------------------------------------------------------------------------ the kernels' K order, undone
def unpack_conv(wp, cinp, kh=3, kw=3):
    """``packing.pack_conv_window`` undone: ``[Cout, kh kw cinp]`` -> ``[Cout, cinp, kh, kw]``."""
    cout, t = wp.shape[0], kh * kw
    taps = wp.reshape(cout, cinp // 64, t, 64).permute(0, 2, 1, 3) if cinp % 64 == 0 else wp.reshape(cout, t, cinp)
    return taps.reshape(cout, kh, kw, cinp).permute(0, 3, 1, 2).contiguous()


def tokens(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()    # (one frame reshapes to a strided view otherwise)


def image(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ the stages
def gn(x, g, silu, r, defect=None):
    h = F.group_norm(x, 32, g[0], g[1], eps=1e-5 if defect == "gn_eps_1e5" else 1e-6)
    return r(h * torch.sigmoid(h) if silu else h)


def conv(x, p, r, *, stride=1, trailing=False, upsample=False, residual=None, out_f32=False, defect=None):
    if x.shape[1] < p["cinp"]:
        x = F.pad(x, (0, 0, 0, 0, 0, p["cinp"] - x.shape[1]))
    b = p["b"]
    if upsample and "phases" in p and (x.shape[2] * x.shape[3]) % 64 == 0 and _phase_form_pays(x.shape[2] * x.shape[3], p["cout"]):
        y = x.new_empty(x.shape[0], p["cout"], 2 * x.shape[2], 2 * x.shape[3])
        for py in (0, 1):
            for px in (0, 1):
                k = unpack_conv(p["phases"][2 * px + py if defect == "upsample_phases_swapped" else 2 * py + px].float(), p["cinp"], 2, 2)
                y[:, :, py::2, px::2] = F.conv2d(F.pad(x, (1 - px, px, 1 - py, py)), k, b)
    else:
        w = unpack_conv(p["w"].float(), p["cinp"])
        if upsample:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
        if trailing:
            y = F.conv2d(F.pad(x, (1, 0, 1, 0) if defect == "downsample_leading_pad" else (0, 1, 0, 1)), w, b, stride=stride)
        else:
            y = F.conv2d(x, w, b, stride=stride, padding=1)
    if residual is not None:
        y = y + residual
    return y if out_f32 else r(y)


def res(x, p, r, defect=None):
    h0 = gn(x, p["norm1"], True, r, defect)
    h = gn(conv(h0, p["conv1"], r), p["norm2"], True, r, defect)
    skip = h0 if defect == "residual_after_norm1" else x
    if "nin" in p:
        B, _, H, W = x.shape
        skip = image(r(tokens(skip) @ p["nin"]["w"].float().T + p["nin"]["b"]), B, H, W)
    return conv(h, p["conv2"], r, residual=skip)


def attn(x, p, r, defect=None):
    B, c, H, W = x.shape
    n = H * W
    g = tokens(gn(x, p["norm"], False, r, defect)).reshape(B, n, c)
    qk = r(g @ p["qk"]["w"].float().T + p["qk"]["b"])
    q, k = qk[..., :c], qk[..., c:]
    s = q @ k.transpose(1, 2)                                                       # fp32, never rounded
    if defect == "softmax_over_queries":
        s = s.transpose(1, 2)
    P = r(torch.softmax(s * (float(n) ** -0.5 if defect == "attn_scale_n" else float(int(c) ** -0.5)), -1))
    v = r(g @ p["wv"].float().T)                                                    # V^T as stored: no bias
    att = P @ (k if defect == "p_times_k" else v)
    att = r(att if defect == "value_bias_dropped" else att + p["bv"])               # the value bias as the column bias of P V^T
    out = r(att.reshape(B * n, c) @ p["proj"]["w"].float().T + p["proj"]["b"] + tokens(x))
    return image(out, B, H, W)


def post_quant_conv_in(z, P, r):
    B, _, h, w = z.shape
    zin = r(F.pad(z, (0, 0, 0, 0, 0, 8 - z.shape[1])))
    z8 = image(r(tokens(zin) @ P["dec.post_quant"]["w"].float().T + P["dec.post_quant"]["b"]), B, h, w)
    return conv(z8, P["dec.conv_in"], r)


def norm_out_conv(a, g, p, r, defect=None):
    return conv(gn(a, g, defect != "no_swish_before_conv_out", r, defect), p, r, out_f32=True)[:, :p["cout_true"]]


def pack(sd, spec, dt, defect=None):
    """The engine's packed weights on the CPU; the two packing defects are one-line changes of what ``Packer`` produces."""
    P = ve.pack_state_dict(sd, num_resolutions=len(spec.ch_mult), num_res_blocks=spec.num_res_blocks, z_channels=spec.z_channels,
                           embed_dim=spec.embed_dim, dtype=dt, device="cpu")
    return pack_defect(P, sd, defect)


def pack_defect(P, sd, defect, conv_in="decoder.conv_in", quant="quant_conv", post="post_quant_conv"):
    if defect == "fold_bias_term_dropped" and "enc.conv_out" in P:
        P["enc.conv_out"]["b"] = sd[quant + ".bias"].float().clone()
    if defect == "post_quant_bias_into_conv_in" and "dec.post_quant" in P:
        zc = sd[post + ".bias"].shape[0]
        P["dec.conv_in"]["b"] = (P["dec.conv_in"]["b"].double() + sd[conv_in + ".weight"].double().sum((2, 3)) @ sd[post + ".bias"].double()).float()
        P["dec.post_quant"]["b"] = torch.zeros_like(P["dec.post_quant"]["b"])
        assert zc <= 8
    return P


def encode(P, spec, x, dt, defect=None, taps=None):
    """``VAEEngine.encode`` up to the moments ``[F, 2 embed_dim, h, w]`` fp32."""
    r = rounder(dt)
    tap = (lambda k, a: a) if taps is None else (lambda k, a: taps.setdefault(k, a))
    nres = len(spec.ch_mult)
    a = tap("enc.conv_in", conv(r(F.pad(x, (0, 0, 0, 0, 0, 8 - x.shape[1]))), P["enc.conv_in"], r))
    for lvl in range(nres):
        for blk in range(spec.num_res_blocks):
            a = tap(f"enc.down.{lvl}.{blk}", res(a, P[f"enc.down.{lvl}.{blk}"], r, defect))
        if lvl != nres - 1:
            a = tap(f"enc.down.{lvl}.ds", conv(a, P[f"enc.down.{lvl}.ds"], r, stride=2, trailing=True, defect=defect))
    a = tap("enc.mid1", res(a, P["enc.mid1"], r, defect))
    a = tap("enc.attn", attn(a, P["enc.attn"], r, defect))
    a = tap("enc.mid2", res(a, P["enc.mid2"], r, defect))
    return norm_out_conv(a, P["enc.norm_out"], P["enc.conv_out"], r, defect)


def decode(P, spec, z, dt, defect=None, taps=None):
    """``VAEEngine.decode``: ``[F, out_ch, 8 h, 8 w]`` fp32."""
    r = rounder(dt)
    tap = (lambda k, a: a) if taps is None else (lambda k, a: taps.setdefault(k, a))
    a = tap("dec.conv_in", post_quant_conv_in(z, P, r))
    a = tap("dec.mid1", res(a, P["dec.mid1"], r, defect))
    a = tap("dec.attn", attn(a, P["dec.attn"], r, defect))
    a = tap("dec.mid2", res(a, P["dec.mid2"], r, defect))
    for lvl in reversed(range(len(spec.ch_mult))):
        for blk in range(spec.num_res_blocks + 1):
            a = tap(f"dec.up.{lvl}.{blk}", res(a, P[f"dec.up.{lvl}.{blk}"], r, defect))
        if lvl != 0:
            a = tap(f"dec.up.{lvl}.us", conv(a, P[f"dec.up.{lvl}.us"], r, upsample=True, defect=defect))
    return norm_out_conv(a, P["dec.norm_out"], P["dec.conv_out"], r, defect)


def state_dict(spec):
    return {k: synth.synth_tensor("vae." + k, tuple(s), 0) for k, s in ovae.param_shapes(spec).items()}


_RUNS = {}


def run_case(case, dt, golden):
    """The model on a fixture case (tests/golden/cases_vae.py): ``(outputs, taps)`` -- moments, z_mode, z_sample whole, ``dec`` on the
    fixture's elements; every stage's output.  Computed once per (case, type), shared, never changed."""
    if (case, dt) not in _RUNS:
        spec = SPECS[cv.CASES[case]["cfg"]]
        x, noise = cv.inputs(case)
        taps = {}
        with torch.no_grad():
            P = pack(state_dict(spec), spec, dt)
            mo = encode(P, spec, x, dt, taps=taps)
            dec = decode(P, spec, golden[f"{case}.z_sample"].float() / cv.SCALE, dt, taps=taps)
        _RUNS[(case, dt)] = ({"moments": mo, "z_mode": ovae.sample(mo, None, cv.SCALE), "z_sample": ovae.sample(mo, noise, cv.SCALE),
                              "dec": cv.take(case, "dec", dec, cv.K_DEC)}, taps)
    return _RUNS[(case, dt)]


def autocast_output(golden, case, k, tag):
    """The reference's own ``torch.autocast`` output ``k`` of a case, as fp32 (``dec`` is stored in its 16-bit type)."""
    if k == "dec" and tag == "bf16":
        return golden[f"{case}.dec_autocast_bf16_bits"].view(torch.int16).view(torch.bfloat16).float()
    return golden[f"{case}.{k}_autocast_{tag}"].float()


# ------------------------------------------------------------------------------------------------ the stage cases (CPU and GPU alike)
# name -> (kind, geometry, input family).  Spatial sizes: the smallest with a border, an odd extent and H != W (6 x 10: hw = 60, pixel
# statistics; 16 x 24 / 8 x 16 / 24 x 32: hw % 64 == 0, column statistics).  ``peaked``: q | k weights scaled so |q.k| c^-1/2 reaches
# about 30; ``lowvar``: input std 1e-2, where GroupNorm's eps decides the result.  Frame 1 is 3 x frame 0, plus a shift.
STAGES = {
    "attn.16x128": ("attn", dict(c=128, H=4, W=4, F=2), "plain"),
    "attn.120x128": ("attn", dict(c=128, H=10, W=12, F=2), "plain"),
    "attn.768x512": ("attn", dict(c=512, H=24, W=32, F=2), "plain"),
    "attn.16x128.peaked": ("attn", dict(c=128, H=4, W=4, F=2), "peaked"),
    "attn.120x128.peaked": ("attn", dict(c=128, H=10, W=12, F=2), "peaked"),
    "attn.768x512.peaked": ("attn", dict(c=512, H=24, W=32, F=2), "peaked"),
    "attn.4096x512.peaked": ("attn", dict(c=512, H=64, W=64, F=1), "peaked"),   # the production shape: fp16, GPU test only (LARGE)
    "res.128.128.6x10": ("res", dict(cin=128, cout=128, H=6, W=10, F=2), "plain"),
    "res.128.128.16x24": ("res", dict(cin=128, cout=128, H=16, W=24, F=2), "plain"),
    "res.128.128.6x10.lowvar": ("res", dict(cin=128, cout=128, H=6, W=10, F=2), "lowvar"),
    "res.128.256.6x10": ("res", dict(cin=128, cout=256, H=6, W=10, F=2), "plain"),
    "res.128.256.16x24": ("res", dict(cin=128, cout=256, H=16, W=24, F=2), "plain"),
    "res.256.512.6x10": ("res", dict(cin=256, cout=512, H=6, W=10, F=2), "plain"),
    "res.256.512.8x16": ("res", dict(cin=256, cout=512, H=8, W=16, F=2), "plain"),
    "down.128.6x10": ("down", dict(c=128, H=6, W=10, F=2), "plain"),
    "down.128.16x24": ("down", dict(c=128, H=16, W=24, F=2), "plain"),
    "up.128.6x10": ("up", dict(c=128, H=6, W=10, F=2), "plain"),            # nine taps on the upsampled grid (hw % 64)
    "up.512.16x24": ("up", dict(c=512, H=16, W=24, F=2), "plain"),          # four parity phases (_phase_form_pays)
    "dec_head.6x10": ("dec_head", dict(c=128, H=6, W=10, F=2), "plain"),
    "dec_head.16x24": ("dec_head", dict(c=128, H=16, W=24, F=2), "plain"),
    "enc_tail.6x10": ("enc_tail", dict(c=128, H=6, W=10, F=2), "plain"),
    "enc_tail.16x24": ("enc_tail", dict(c=128, H=16, W=24, F=2), "plain"),
    "dec_tail.6x10": ("dec_tail", dict(c=128, H=6, W=10, F=2), "plain"),
    "dec_tail.16x24": ("dec_tail", dict(c=128, H=16, W=24, F=2), "plain"),
}
LARGE = ("attn.4096x512.peaked",)             # a 35 GFLOP fp64 reference: one frame, one type, not part of the CPU suite
PHASE_FORM = {"up.128.6x10": False, "up.512.16x24": True}
# which stage cases a defect must fail (test_vae_bound_cpu.py asserts every pair, in both types)
OWNERS = {
    "attn_scale_n": ["attn.16x128.peaked", "attn.768x512.peaked"],
    "softmax_over_queries": ["attn.16x128.peaked", "attn.120x128.peaked", "attn.768x512.peaked"],
    "p_times_k": ["attn.16x128", "attn.120x128", "attn.768x512"],
    "value_bias_dropped": ["attn.16x128", "attn.120x128", "attn.768x512"],
    "downsample_leading_pad": ["down.128.6x10", "down.128.16x24"],
    "gn_eps_1e5": ["res.128.128.6x10.lowvar"],
    "fold_bias_term_dropped": ["enc_tail.6x10", "enc_tail.16x24"],
    "post_quant_bias_into_conv_in": ["dec_head.6x10", "dec_head.16x24"],
    "residual_after_norm1": ["res.128.128.6x10", "res.128.256.16x24", "res.256.512.6x10"],
    "upsample_phases_swapped": ["up.512.16x24"],
    "no_swish_before_conv_out": ["enc_tail.6x10", "dec_tail.16x24"],
}


def _conv_sd(sd, pre, cin, cout, k, gain=1.0):
    sd[pre + ".weight"] = synth.synth_tensor("vaestage." + pre + ".weight", (cout, cin, k, k), 0) * gain
    sd[pre + ".bias"] = synth.synth_tensor("vaestage." + pre + ".bias", (cout,), 0)


def _norm_sd(sd, pre, c):
    sd[pre + ".weight"] = synth.synth_tensor("vaestage." + pre + ".weight", (c,), 0)
    sd[pre + ".bias"] = synth.synth_tensor("vaestage." + pre + ".bias", (c,), 0)


def stage_weights(name):
    """The stage's fp32 state dict, keys as the reference names them under the prefix ``s``."""
    kind, g, family = STAGES[name]
    sd = {}
    if kind == "attn":
        c = g["c"]
        _norm_sd(sd, "s.norm", c)
        # peaked: after the GroupNorm g ~ N(0, 1), q.k c^-1/2 has std gain^2 (U(-1, 1) sqrt(3 / c) weights give unit-variance q, k):
        # gain 2.5 (std 6.25) puts the largest of the n^2 scores between 18 (n = 16) and 32 (n = 768)
        gain = 2.5 if family == "peaked" else 1.0
        for nme in ("q", "k"):
            _conv_sd(sd, f"s.{nme}", c, c, 1, gain)
        for nme in ("v", "proj_out"):
            _conv_sd(sd, f"s.{nme}", c, c, 1)
    elif kind == "res":
        _norm_sd(sd, "s.norm1", g["cin"]); _conv_sd(sd, "s.conv1", g["cin"], g["cout"], 3)
        _norm_sd(sd, "s.norm2", g["cout"]); _conv_sd(sd, "s.conv2", g["cout"], g["cout"], 3)
        if g["cin"] != g["cout"]:
            _conv_sd(sd, "s.nin_shortcut", g["cin"], g["cout"], 1)
    elif kind in ("down", "up"):
        _conv_sd(sd, "s.conv", g["c"], g["c"], 3)
    elif kind == "dec_head":
        _conv_sd(sd, "post_quant_conv", 4, 4, 1); _conv_sd(sd, "s.conv_in", 4, g["c"], 3)
        sd["post_quant_conv.bias"] = sd["post_quant_conv.bias"] * 10.0          # 0.5: a bias large enough to be seen at a border
    elif kind == "enc_tail":
        _norm_sd(sd, "s.norm_out", g["c"]); _conv_sd(sd, "s.conv_out", g["c"], 8, 3); _conv_sd(sd, "quant_conv", 8, 8, 1)
        sd["s.conv_out.bias"] = sd["s.conv_out.bias"] * 10.0
    elif kind == "dec_tail":
        _norm_sd(sd, "s.norm_out", g["c"]); _conv_sd(sd, "s.conv_out", g["c"], 3, 3)
    return sd


def stage_input(name, dt):
    """The stage's input ``[F, C, H, W]``, fp32 holding values of ``dt``."""
    kind, g, family = STAGES[name]
    C = 4 if kind == "dec_head" else g.get("cin", g.get("c"))
    x = synth.synth_normal("vaestage.x." + name, (g["F"], C, g["H"], g["W"]))
    x[1:] = 3.0 * x[1:] + 0.5                                                   # frames differ in scale: a frame-index slip shows
    if family == "lowvar":
        x = 1e-2 * x
    return rounder(dt)(x)


def stage_pack(name, sd, dt, device, defect=None):
    kind = STAGES[name][0]
    pk = ve.Packer(sd, dt, device)
    if kind == "attn":
        return pk.attn("s")
    if kind == "res":
        return pk.res("s")
    if kind == "down":
        return pk.conv3("s.conv")
    if kind == "up":
        return pk.upsample("s.conv")
    if kind == "dec_head":
        return pack_defect({"dec.post_quant": pk.post_quant(4, 4), "dec.conv_in": pk.conv3("s.conv_in")}, sd, defect, conv_in="s.conv_in")
    if kind == "enc_tail":
        return pack_defect({"enc.norm_out": pk.gn("s.norm_out"), "enc.conv_out": pk.folded_conv_out("s.conv_out")}, sd, defect)
    return {"dec.norm_out": pk.gn("s.norm_out"), "dec.conv_out": pk.conv3("s.conv_out", cout_pad=4)}


def stage_ref64(name, sd, x):
    """The matching ``oracle.vae`` function in fp64 on the 16-bit-rounded input with the UNROUNDED weights."""
    kind = STAGES[name][0]
    sd64, x64 = {k: v.double() for k, v in sd.items()}, x.double()
    if kind == "attn":
        return ovae.attn_block(sd64, "s", x64)
    if kind == "res":
        return ovae.resnet_block(sd64, "s", x64)
    if kind == "down":
        return ovae.downsample(sd64, "s", x64)
    if kind == "up":
        return ovae.upsample(sd64, "s", x64)
    if kind == "dec_head":
        return ovae._conv(sd64, "s.conv_in", ovae._conv(sd64, "post_quant_conv", x64, padding=0))
    if kind == "enc_tail":
        return ovae._conv(sd64, "quant_conv", ovae.norm_out_conv(sd64, "s", x64), padding=0)          # the unfolded two-step
    return ovae.norm_out_conv(sd64, "s", x64)


def stage_model(name, P, x, dt, defect=None):
    kind, r = STAGES[name][0], rounder(dt)
    if kind == "attn":
        return attn(x, P, r, defect)
    if kind == "res":
        return res(x, P, r, defect)
    if kind == "down":
        return conv(x, P, r, stride=2, trailing=True, defect=defect)
    if kind == "up":
        return conv(x, P, r, upsample=True, defect=defect)
    if kind == "dec_head":
        return post_quant_conv_in(x, P, r)
    if kind == "enc_tail":
        return norm_out_conv(x, P["enc.norm_out"], P["enc.conv_out"], r, defect)
    return norm_out_conv(x, P["dec.norm_out"], P["dec.conv_out"], r, defect)


_CLEAN = {}


def stage_clean(name, dt):
    """``(sd, x, ref64, (rel-L2, worst))`` of the clean model at a stage case: computed once, shared, never changed."""
    if (name, dt) not in _CLEAN:
        sd, x = stage_weights(name), stage_input(name, dt)
        with torch.no_grad():
            ref = stage_ref64(name, sd, x)
            got = stage_model(name, stage_pack(name, sd, dt, "cpu"), x, dt)
        _CLEAN[(name, dt)] = (sd, x, ref, figures(got, ref))
    return _CLEAN[(name, dt)]
