"""CPU emulation of ``vface_amd.clip.ClipEngine``: every kernel call replaced by its fp32 restatement in torch, with the rounding to
the 16-bit compute type at the engine's storage points -- the patch matrix, every LayerNorm output, q | k | v, the attention's
scaled query, probabilities and output, the MLP activations before and after the activation, the weights -- and the residual stream
in fp32 from ``pre_layrnorm`` to ``final_ln2``'s input.  What it does not restate is the order of fp32 additions inside a GEMM or a
LayerNorm.  Its error against the fixture's double run, times 1.25 (the margin smoke.py and the bf16 UNet test use over their
emulations), is the GPU test's tolerance; ``defect`` seeds the one-line mistakes test_clip_bound_cpu.py must see past that tolerance.
Plain functions, nothing collected by pytest."""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import cases_clip as cc  # noqa: E402

MARGIN = 1.25
PATCH, PROJ = 14, 768
DEFECTS = ("class_row_without_position", "erf_gelu_in_vit", "quick_gelu_in_mapper", "mapper_reads_q_third", "scale_dropped",
           "pool_token_1", "normalise_before_un_norm", "antialiased_resize")
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


def engine_cfg(name):
    c = cc.CONFIGS[name]
    return {k: c[k] for k in ("hidden", "heads", "layers", "mlp", "image")}


def synth_weights(name, keys=None):
    """The fp32 state dict the fixture's module was filled with, restricted to the engine's keys (``keys``: another key list)."""
    from vface_amd import clip
    from vface_amd.utils import synth
    shapes = clip.state_shapes(engine_cfg(name))
    return {k: synth.synth_tensor(k, shapes[k], cc.WEIGHT_SEED) for k in (keys or shapes)}


def prep32(frames, size, mask=None, defect=None):
    """ddpm.py:907-912 in torch fp32: un_norm, TF.normalize, TF.resize (bilinear, align_corners false, no antialias)."""
    x = frames.float()
    if mask is not None:
        x = x * (1.0 - mask.float().reshape(x.shape[0], 1, *x.shape[2:]))
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    t = (((x - mean) / std) + 1.0) / 2.0 if defect == "normalise_before_un_norm" else ((x + 1.0) / 2.0 - mean) / std
    return F.interpolate(t, size=(size, size), mode="bilinear", align_corners=False, antialias=defect == "antialiased_resize")


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def _attention(q, k, v, r, scale):
    """One head, ``[B, T, 64]`` each: the kernel's rounding points -- q scale log2(e) rounded once, base-2 scores in fp32,
    exponentials rounded to 16 bits for both the sum and the product with v, the normalised output rounded."""
    qs = r(q * (scale * math.log2(math.e)))
    s = qs @ k.transpose(1, 2)
    p = r(torch.exp2(s - s.max(dim=-1, keepdim=True).values))
    return r((p @ v) / p.sum(dim=-1, keepdim=True))


def encode(sd, cfg, dt, img, defect=None, taps=None):
    """``ClipEngine.encode`` on the CPU.  ``sd``: fp32 state dict (the engine's keys), ``img [B, 3, image, image]`` fp32."""
    r = lambda t: t.to(dt).float()
    C, heads, T = cfg["hidden"], cfg["heads"], (cfg["image"] // PATCH) ** 2 + 1
    B = img.shape[0]
    v_ = "model.vision_model."
    W = lambda name: r(sd[name + ".weight"])
    lin = lambda x, name: x @ W(name).T + sd[name + ".bias"]
    a0 = r(F.unfold(img, PATCH, stride=PATCH).transpose(1, 2))                                    # [B, P, 588]
    tok = a0 @ r(sd[v_ + "embeddings.patch_embedding.weight"].reshape(C, -1)).T
    pos = sd[v_ + "embeddings.position_embedding.weight"]
    x = torch.cat([sd[v_ + "embeddings.class_embedding"].view(1, 1, C).expand(B, 1, C), tok], 1) + pos[None]
    if defect == "class_row_without_position":
        x[:, 0] = sd[v_ + "embeddings.class_embedding"]
    if taps is not None:
        taps["embeddings"] = x.clone()
    x = _ln(x, sd[v_ + "pre_layrnorm.weight"], sd[v_ + "pre_layrnorm.bias"])                      # fp32: the stream starts unrounded
    scale = 1.0 if defect == "scale_dropped" else 0.125
    for i in range(cfg["layers"]):
        p = f"{v_}encoder.layers.{i}."
        h = r(_ln(x, sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"]))
        q, k, v = (r(lin(h, p + f"self_attn.{n}_proj")).view(B, T, heads, 64).transpose(1, 2).reshape(B * heads, T, 64) for n in "qkv")
        att = _attention(q, k, v, r, scale).view(B, heads, T, 64).transpose(1, 2).reshape(B, T, C)
        x = x + lin(att, p + "self_attn.out_proj")
        h = r(_ln(x, sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"]))
        m = r(lin(h, p + "mlp.fc1"))
        m = r(F.gelu(m) if defect == "erf_gelu_in_vit" else m * torch.sigmoid(1.702 * m))
        x = x + lin(m, p + "mlp.fc2")
        if taps is not None and i == 0:
            taps["layer0"] = x.clone()
    pooled = r(_ln(x[:, 1 if defect == "pool_token_1" else 0], sd[v_ + "post_layernorm.weight"], sd[v_ + "post_layernorm.bias"]))
    z = pooled @ r(sd["model.visual_projection.weight"]).T
    if taps is not None:
        taps["pooler_output"], taps["visual_projection"] = pooled.clone(), z.clone()
    third = 0 if defect == "mapper_reads_q_third" else 2
    for i in range(cc.MAPPER_LAYERS):
        p = f"mapper2.resblocks.{i}."
        g = r(_ln(z, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"]))
        wv, bv = sd[p + "attn.c_qkv.weight"][third * PROJ:(third + 1) * PROJ], sd[p + "attn.c_qkv.bias"][third * PROJ:(third + 1) * PROJ]
        vv = r(g @ r(wv).T + bv)
        z = z + lin(vv, p + "attn.c_proj")
        g = r(_ln(z, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"]))
        m = r(lin(g, p + "mlp.c_fc"))
        m = r(m * torch.sigmoid(1.702 * m) if defect == "quick_gelu_in_mapper" else F.gelu(m))
        z = z + lin(m, p + "mlp.c_proj")
        if taps is not None and i == 0:
            taps["mapper2_block0"] = z.clone()
    return r(_ln(z, sd["final_ln2.weight"], sd["final_ln2.bias"])).view(B, 1, PROJ)


def encode_from_frames(sd, cfg, dt, frames, mask=None, defect=None, taps=None):
    return encode(sd, cfg, dt, prep32(frames, cfg["image"], mask, defect), defect, taps)


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


# ---- the feature mix (ddpm.py:872-1045, shipped configuration), restated: ldm.models.diffusion.ddpm cannot be imported here ----
MIX_WEIGHTS = (1.0, 10.0, 0.05)                    # clip_weight, ID_weight, Landmarks_weight of configs/project_ffhq.yaml
MIX_LINEARS = {"proj_out_source": (768, 768), "proj_out_target": (768, 768), "ID_proj_out": (768, 512), "landmark_proj_out": (768, 136)}


def mix_weights(seed=cc.WEIGHT_SEED):
    from vface_amd.utils import synth
    sd = {}
    for name, shape in MIX_LINEARS.items():
        sd[name + ".weight"] = synth.synth_tensor(name + ".weight", shape, seed)
        sd[name + ".bias"] = synth.synth_tensor(name + ".bias", shape[:1], seed)
    return sd


def conditioning64(e_src, e_tar, id_feat, landmarks, sd):
    """``conditioning_with_feat`` in fp64 numpy-style arithmetic from E of the source ``[1 | B, 1, 768]`` and of the prepared target
    ``[B, 1, 768]``: c = proj_out_source(E(x)) + proj_out_target(E(prep(tar))), c2 = ID_proj_out(id_feat)[:, None],
    lm = landmark_proj_out(landmarks)[:, None], result = (c w_c + c2 w_id + lm w_lm) / (w_c + w_id + w_lm)."""
    d = lambda t: t.double()
    lin = lambda x, n: d(x) @ d(sd[n + ".weight"]).T + d(sd[n + ".bias"])
    c = lin(e_src, "proj_out_source") + lin(e_tar, "proj_out_target")
    c2 = lin(id_feat, "ID_proj_out")[:, None]
    lm = lin(landmarks, "landmark_proj_out")[:, None]
    wc, wi, wl = MIX_WEIGHTS
    return (c * wc + c2 * wi + lm * wl) / (wc + wi + wl)
