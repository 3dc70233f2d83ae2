"""The conditioning encoder on the GPU: the reference's ``FrozenCLIPEmbedder`` (REFace/ldm/modules/encoders/modules.py:211-264 -- HF
``CLIPVisionTransformer`` ViT-L/14, its pooled output, ``visual_projection``, ``mapper2`` of encoders/xf.py and ``final_ln2``) as a
sequence of HIP launches, eager on the caller's stream.  ``ClipEngine`` holds the packed weights; per batch of B images:

    patches   vface_clip_patches      [B P][640] 16-bit        P = (image / 14)^2 patches; optionally the whole of `prep`
    tokens    vface_gemm              [B P][C] fp32            the 14 x 14 stride-14 convolution, K = 588 padded to 640
    stream    vface_clip_embed        [B T][C] fp32            T = P + 1: class row, position table, pre_layrnorm
    per layer vface_layernorm, vface_gemm (q | k | v as one [3 C][C] weight), vface_attention (dh = C / heads = 64, on the three
              strided thirds of that buffer), vface_gemm (+ fp32 residual), vface_layernorm, vface_gemm, vface_act (quick_gelu),
              vface_gemm (+ fp32 residual)
    head      vface_layernorm on token 0 of every sample (post_layernorm), vface_gemm (visual_projection, fp32 out)
    mapper2   five blocks on [B][768]: with n_ctx = 1 the softmax over one key is exactly 1, so attn(x) = c_proj(v) and only the v
              third of c_qkv is packed; erf-GELU MLP; final_ln2 -> [B][768] in the compute type

The residual stream is fp32 from the embedding to the last block (``vface_stream32``); what is rounded to 16 bits are the GEMM
operands: LayerNorm outputs, q | k | v, attention outputs, MLP activations -- the points tests/clip_model.py restates.  No split-K
and no atomics: a sample's bits do not depend on the batch it is launched in.  No CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import hip

PATCH = hip.CLIP_PATCH
PROJ = 768                   # visual_projection's and mapper2's width, fixed by FrozenCLIPEmbedder.__init__
MAPPER_LAYERS = 5
VIT_L14 = dict(hidden=1024, heads=16, layers=24, mlp=4096, image=224)       # openai/clip-vit-large-patch14's vision_config

# state-dict prefixes FrozenCLIPEmbedder holds and its forward never reads (modules.py:215-233)
UNUSED_PREFIXES = ("model.text_model.", "model.text_projection.", "model.logit_scale", "mapper.", "final_ln.", "projection_back.",
                   "model.vision_model.embeddings.position_ids")


def state_shapes(cfg: dict) -> Dict[str, tuple]:
    """Key -> shape of every state-dict entry the engine reads, for a vision tower of ``cfg`` (hidden, heads, layers, mlp, image)."""
    C, I, T = cfg["hidden"], cfg["mlp"], (cfg["image"] // PATCH) ** 2 + 1
    v = "model.vision_model."
    s = {v + "embeddings.class_embedding": (C,), v + "embeddings.patch_embedding.weight": (C, 3, PATCH, PATCH),
         v + "embeddings.position_embedding.weight": (T, C)}

    def ln(name, n):
        s[name + ".weight"], s[name + ".bias"] = (n,), (n,)

    def lin(name, n, k):
        s[name + ".weight"], s[name + ".bias"] = (n, k), (n,)

    ln(v + "pre_layrnorm", C)
    for i in range(cfg["layers"]):
        p = f"{v}encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(p + "self_attn." + n, C, C)
        ln(p + "layer_norm1", C)
        lin(p + "mlp.fc1", I, C)
        lin(p + "mlp.fc2", C, I)
        ln(p + "layer_norm2", C)
    ln(v + "post_layernorm", C)
    s["model.visual_projection.weight"] = (PROJ, C)
    for i in range(MAPPER_LAYERS):
        p = f"mapper2.resblocks.{i}."
        lin(p + "attn.c_qkv", 3 * PROJ, PROJ)
        lin(p + "attn.c_proj", PROJ, PROJ)
        ln(p + "ln_1", PROJ)
        lin(p + "mlp.c_fc", 4 * PROJ, PROJ)
        lin(p + "mlp.c_proj", PROJ, 4 * PROJ)
        ln(p + "ln_2", PROJ)
    ln("final_ln2", PROJ)
    return s


def split_state_dict(sd, cfg: dict):
    """``(used, dropped)``: the entries the engine reads, and the names of those FrozenCLIPEmbedder holds without reading.  A key
    that is neither, a missing one, or a wrong shape raises."""
    want = state_shapes(cfg)
    used, dropped = {}, []
    for k, t in sd.items():
        if k in want:
            if tuple(t.shape) != want[k]:
                raise hip.VFaceHipError(f"{k}: shape {tuple(t.shape)}, expected {want[k]}")
            used[k] = t
        elif k.startswith(UNUSED_PREFIXES):
            dropped.append(k)
        else:
            raise hip.VFaceHipError(f"unexpected key {k!r} in a FrozenCLIPEmbedder state dict")
    missing = [k for k in want if k not in used]
    if missing:
        raise hip.VFaceHipError(f"{len(missing)} keys missing from the state dict, e.g. {missing[:3]}")
    return used, dropped


def pack_patch_weight(w: torch.Tensor) -> torch.Tensor:
    """``patch_embedding.weight [C, 3, 14, 14]`` -> ``[C, 640]``: its own flattening (column c 196 + ky 14 + kx, the order of
    vface_clip_patches), zero from 588 on."""
    C = w.shape[0]
    out = w.new_zeros(C, hip.CLIP_PATCH_KP)
    out[:, :hip.CLIP_PATCH_K] = w.reshape(C, hip.CLIP_PATCH_K)
    return out


def unpack_patch_weight(wp: torch.Tensor) -> torch.Tensor:
    return wp[:, :hip.CLIP_PATCH_K].reshape(wp.shape[0], 3, PATCH, PATCH)


class ClipEngine:
    """Executes ``FrozenCLIPEmbedder.forward`` on device buffers.  ``sd``: the reference's state dict (any float dtype, any device;
    unused keys are dropped, unknown ones refused); ``cfg``: hidden, heads, layers, mlp, image of the vision tower."""

    def __init__(self, sd, cfg: Optional[dict] = None, dtype: torch.dtype = torch.float16, device="cuda:0"):
        hip.load()      # no CPU fallback: fail here if the library is missing
        hip.dtype_code(dtype)
        self.cfg = dict(VIT_L14 if cfg is None else cfg)
        self.dtype, self.dev = dtype, torch.device(device)
        C, heads = self.cfg["hidden"], self.cfg["heads"]
        if self.cfg["image"] % PATCH or C % heads or C // heads != 64 or C % 64 or self.cfg["mlp"] % 64:
            raise hip.VFaceHipError("the image tower runs at patch 14, head dimension 64, widths that are multiples of 64")
        self.grid = self.cfg["image"] // PATCH
        self.P, self.T = self.grid ** 2, self.grid ** 2 + 1
        used, self.dropped = split_state_dict(sd, self.cfg)
        f = {k: t.detach().float().cpu() for k, t in used.items()}
        w16 = lambda t: t.to(self.dtype).contiguous().to(self.dev)
        f32 = lambda t: t.contiguous().to(self.dev)
        v = "model.vision_model."
        self.w_patch = w16(pack_patch_weight(f[v + "embeddings.patch_embedding.weight"]))
        self.cls, self.pos = f32(f[v + "embeddings.class_embedding"]), f32(f[v + "embeddings.position_embedding.weight"])
        ln = lambda name: (f32(f[name + ".weight"]), f32(f[name + ".bias"]))
        lin = lambda name: (w16(f[name + ".weight"]), f32(f[name + ".bias"]))
        self.pre_ln, self.post_ln, self.final_ln2 = ln(v + "pre_layrnorm"), ln(v + "post_layernorm"), ln("final_ln2")
        self.layers = []
        for i in range(self.cfg["layers"]):
            p = f"{v}encoder.layers.{i}."
            qkv = [f[p + f"self_attn.{n}_proj.{kind}"] for kind in ("weight", "bias") for n in ("q", "k", "v")]
            self.layers.append(dict(ln1=ln(p + "layer_norm1"), qkv=(w16(torch.cat(qkv[:3], 0)), f32(torch.cat(qkv[3:], 0))),
                                    out=lin(p + "self_attn.out_proj"), ln2=ln(p + "layer_norm2"), fc1=lin(p + "mlp.fc1"),
                                    fc2=lin(p + "mlp.fc2")))
        self.w_proj = w16(f["model.visual_projection.weight"])
        self.mapper = []
        for i in range(MAPPER_LAYERS):
            p = f"mapper2.resblocks.{i}."
            wv, bv = f[p + "attn.c_qkv.weight"][2 * PROJ:], f[p + "attn.c_qkv.bias"][2 * PROJ:]      # the v third: xf.py:70-71, one head
            self.mapper.append(dict(ln1=ln(p + "ln_1"), v=(w16(wv), f32(bv)), proj=lin(p + "attn.c_proj"), ln2=ln(p + "ln_2"),
                                    fc=lin(p + "mlp.c_fc"), cproj=lin(p + "mlp.c_proj")))

    # ---- building blocks -------------------------------------------------------------------------------------------------
    def _buf(self, rows, cols, dtype=None):
        return torch.empty(rows, cols, dtype=dtype or self.dtype, device=self.dev)

    def _linear(self, a, wb, *, M, out=None, residual32=None, out32=None, rows_per_sample=1):
        w, b = wb if isinstance(wb, tuple) else (wb, None)
        N, K = w.shape
        hip.gemm(a, w, out, M=M, N=N, K=K, lda=a.stride(0), ldc=out.stride(0) if out is not None else N, bias=b,
                 rows_per_sample=rows_per_sample, residual32=residual32, out32=out32, split_k=False)

    def _ln(self, x, gb, out, *, M, ldx=None):
        hip.layernorm(x, gb[0], gb[1], out, M=M, C_=out.shape[1], ldx=x.stride(0) if ldx is None else ldx, ldy=out.stride(0), eps=1e-5)

    # ---- the network -----------------------------------------------------------------------------------------------------
    def patches(self, img: torch.Tensor, *, prep: bool, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``img [B, 3, H, W]`` fp32 on the device -> the patch matrix ``[B P, 640]``.  ``prep``: frames in [-1, 1] of any size
        (``mask [B, 1, H, W]`` or ``[B, H, W]``: times (1 - mask) first); otherwise CLIP-normalised images of the tower's size."""
        if not img.is_cuda:
            raise hip.VFaceHipError("the engine runs on the GPU: images must be device tensors (no CPU fallback)")
        B, _, H, W = img.shape
        out = self._buf(B * self.P, hip.CLIP_PATCH_KP)
        mk = None if mask is None else mask.float().reshape(B, H, W).contiguous()
        hip.clip_patches(img.float().contiguous(), out, B=B, grid=self.grid, H=H, W=W, ldo=out.stride(0), prep=prep, mask=mk)
        return out

    def forward_patches(self, a0: torch.Tensor, taps: Optional[dict] = None) -> torch.Tensor:
        """The patch matrix ``[B P, 640]`` -> E ``[B, 1, 768]`` in the compute type.  ``taps``: a dict that receives clones of the
        intermediates the fixture records (one more launch for the embeddings: pre_layrnorm is fused behind them)."""
        C, I, T, P, heads = self.cfg["hidden"], self.cfg["mlp"], self.T, self.P, self.cfg["heads"]
        B = a0.shape[0] // P
        M = B * T
        tok = self._buf(B * P, C, torch.float32)
        self._linear(a0, self.w_patch, M=B * P, out32=tok, rows_per_sample=P)
        xa, xb = self._buf(M, C, torch.float32), self._buf(M, C, torch.float32)
        hip.clip_embed(tok, self.cls, self.pos, xa, B=B, patches=P, C_=C, ldt=C, ldo=C, gamma=self.pre_ln[0], beta=self.pre_ln[1])
        if taps is not None:                                                    # the sums in front of the fused pre_layrnorm
            hip.clip_embed(tok, self.cls, self.pos, xb, B=B, patches=P, C_=C, ldt=C, ldo=C)
            taps["embeddings"] = xb.view(B, T, C).clone()
        h, qkv, att, mid = self._buf(M, C), self._buf(M, 3 * C), self._buf(M, C), self._buf(M, I)
        flat = qkv.view(-1)
        for i, L in enumerate(self.layers):
            self._ln(xa, L["ln1"], h, M=M)
            self._linear(h, L["qkv"], M=M, out=qkv, rows_per_sample=T)
            hip.attention(flat, flat[C:], flat[2 * C:], att, B=B, heads=heads, n=T, nk=T, dh=64, ldq=3 * C, ldk=3 * C, ldv=3 * C,
                          bsq=T * 3 * C, bsk=T * 3 * C, bsv=T * 3 * C, ldo=C, bso=T * C, scale=0.125)
            self._linear(att, L["out"], M=M, residual32=xa, out32=xb, rows_per_sample=T)
            self._ln(xb, L["ln2"], h, M=M)
            self._linear(h, L["fc1"], M=M, out=mid, rows_per_sample=T)
            hip.act(mid, mid, rows=M, cols=I, ldx=I, ldy=I, kind=hip.ACT_QUICK_GELU)
            self._linear(mid, L["fc2"], M=M, residual32=xb, out32=xa, rows_per_sample=T)
            if taps is not None and i == 0:
                taps["layer0"] = xa.view(B, T, C).clone()
        pooled = self._buf(B, C)
        self._ln(xa, self.post_ln, pooled, M=B, ldx=T * C)                       # token 0 of every sample
        za, zb = self._buf(B, PROJ, torch.float32), self._buf(B, PROJ, torch.float32)
        self._linear(pooled, self.w_proj, M=B, out32=za)
        if taps is not None:
            taps["pooler_output"], taps["visual_projection"] = pooled.clone(), za.clone()
        g, vv, mm = self._buf(B, PROJ), self._buf(B, PROJ), self._buf(B, 4 * PROJ)
        for i, L in enumerate(self.mapper):
            self._ln(za, L["ln1"], g, M=B)
            self._linear(g, L["v"], M=B, out=vv)
            self._linear(vv, L["proj"], M=B, residual32=za, out32=zb)
            self._ln(zb, L["ln2"], g, M=B)
            self._linear(g, L["fc"], M=B, out=mm)
            hip.act(mm, mm, rows=B, cols=4 * PROJ, ldx=4 * PROJ, ldy=4 * PROJ, kind=hip.ACT_GELU_ERF)
            self._linear(mm, L["cproj"], M=B, residual32=zb, out32=za)
            if taps is not None and i == 0:
                taps["mapper2_block0"] = za.clone()
        out = self._buf(B, PROJ)
        self._ln(za, self.final_ln2, out, M=B)
        return out.view(B, 1, PROJ)

    def encode(self, img224: torch.Tensor, taps: Optional[dict] = None) -> torch.Tensor:
        """``FrozenCLIPEmbedder.forward``: CLIP-normalised images ``[B, 3, image, image]`` -> ``[B, 1, 768]``."""
        return self.forward_patches(self.patches(img224, prep=False), taps)

    def encode_from_frames(self, tar: torch.Tensor, mask: Optional[torch.Tensor] = None, taps: Optional[dict] = None) -> torch.Tensor:
        """E(prep(tar)) for frames ``[F, 3, H, W]`` in [-1, 1] (ddpm.py:907-913; with ``mask`` = inpaint_mask the input of
        scripts/VFace_inference_batch.py:493-496): the resize happens inside the patch gather, the 224 x 224 image never exists."""
        return self.forward_patches(self.patches(tar, prep=True, mask=mask), taps)
