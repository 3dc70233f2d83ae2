"""Stand-alone ``forward`` of the container modules of the drop-in surface (SURVEY 8b "module surface"):
``ResBlock`` / ``Downsample`` / ``Upsample`` / ``TimestepEmbedSequential`` (openaimodel.py:74-160, 255-275),
``SpatialTransformer`` / ``BasicTransformerBlock`` / ``CrossAttention`` / ``FeedForward`` / ``GEGLU`` (attention.py:37-64, 179-221,
239-243, 278-289).

Inside ``UNetModel.forward`` these layers are executed by ``UNetEngine`` as one fused kernel sequence (stacked
embedding projections, in-place concatenation, ...); a caller that invokes a sub-module directly gets the same
per-layer kernel sequence through the same engine methods, on tensors in the reference's layouts: ``[N, C, H, W]``
images, ``[B, n, d]`` token matrices, ``[N, emb]`` embeddings.  Results come back in the input's floating-point type.
There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import hip
from .engine import Act, HookCfg, UNetEngine, plan_fusion


def _engine_for(module, x: torch.Tensor) -> UNetEngine:
    """One parameter-version-checked engine + packed weights per module instance."""
    if not x.is_cuda:
        raise hip.VFaceHipError(f"{type(module).__name__}.forward needs CUDA tensors: no CPU fallback on the VFace path")
    dt = x.dtype if x.dtype in (torch.float16, torch.bfloat16) else torch.float16
    ver = tuple(p._version for p in module.parameters()) + (dt, str(x.device))
    cache = module.__dict__.get("_vface_exec")
    if cache is None or cache["ver"] != ver:
        cache = {"ver": ver, "eng": UNetEngine(None, dt, device=x.device), "packed": {}}
        module.__dict__["_vface_exec"] = cache
    return cache["eng"], cache["packed"]


def _sd(module):
    return {k: v.detach() for k, v in module.state_dict().items()}


def _to_act(eng: UNetEngine, x: torch.Tensor) -> Act:
    """NCHW -> NHWC 16-bit (+ the fp32 carrier when the input is fp32 and the residual stream is on)."""
    N, C, H, W = x.shape
    cpad = (C + 7) // 8 * 8
    t = eng._new(N * H * W, cpad)
    hip.nchw_to_nhwc(x.float().contiguous(), t, N=N, C_=C, hw=H * W, cpad=cpad)
    t32 = None
    if eng.stream32 and x.dtype == torch.float32 and C % 8 == 0:
        t32 = x.permute(0, 2, 3, 1).reshape(N * H * W, C).contiguous()
    return Act(t, N, H, W, None, t32)


def _from_act(a: Act, like: torch.Tensor) -> torch.Tensor:
    src = a.t32 if a.t32 is not None else a.t
    C = src.shape[1]
    return src.reshape(a.N, a.H, a.W, C).permute(0, 3, 1, 2).to(like.dtype).contiguous()


def _emb_rowbias(eng: UNetEngine, sd, emb: torch.Tensor) -> torch.Tensor:
    """emb_layers = SiLU -> Linear (openaimodel.py:218-224): fp32 [N, cout] row bias for the first conv's epilogue."""
    N = emb.shape[0]
    e16 = eng._new(N, emb.shape[1])
    hip.silu(emb.float().contiguous(), e16)
    w = eng.pack_lin(sd, "emb_layers.1")   # (small; re-packed per call)
    out = eng._new(N, w["w"].shape[0], torch.float32)
    eng._gemm(e16, w, out, flags=hip.EPI_OUT_F32)
    return out


def resblock_forward(mod, x: torch.Tensor, emb: torch.Tensor) -> torch.Tensor:
    eng, P = _engine_for(mod, x)
    sd = _sd(mod)
    if "res" not in P:
        P["res"] = eng.pack_res({("." + k): v for k, v in sd.items()}, "")
    p = dict(P["res"])
    rb = _emb_rowbias(eng, sd, emb)
    p["emb_slice"] = (0, rb.shape[1])
    y = eng._res(_to_act(eng, x), p, rb, None)
    return _from_act(y, x)


def conv_forward(mod, x: torch.Tensor, which: str) -> torch.Tensor:
    """Downsample.op (stride 2) / Upsample.conv (after nearest x2)."""
    eng, P = _engine_for(mod, x)
    if "conv" not in P:
        sd = {("." + k): v for k, v in _sd(mod).items()}
        P["conv"] = eng.pack_up(sd, ".conv") if which == "up" else eng.pack_conv3(sd, ".op")
    a = _to_act(eng, x)
    y = eng._conv(a, P["conv"], None, stride=2 if which == "down" else 1, upsample=which == "up")
    return _from_act(y, x)


def _a2vec(eng: UNetEngine, sd, t: str, context: Optional[torch.Tensor], N: int, c: int, P: dict) -> torch.Tensor:
    """The single-token cross-attention's contribution to_out(to_v(ctx)) as an fp32 [N, c] row bias."""
    if context is None:
        raise ValueError("context (cross-attention conditioning) is required: the reference's attn2 with context=None is "
                         "self-attention, which is not part of the VFace configuration")
    ctx = context.reshape(context.shape[0], -1)
    if context.dim() != 3 or context.shape[1] != 1:
        raise hip.VFaceHipError(f"context must be [N, tokens, context_dim]; got {tuple(context.shape)}")
    c16 = eng._new(N, ctx.shape[1])
    hip.cast_f32(ctx.float().contiguous(), c16)
    v = eng._new(N, c)
    if "a2" not in P:
        P["a2"] = (eng.pack_lin(sd, t + ".attn2.to_v", bias=False), eng.pack_lin(sd, t + ".attn2.to_out.0"))
    eng._gemm(c16, P["a2"][0], v)
    out = eng._new(N, c, torch.float32)
    eng._gemm(v, P["a2"][1], out, flags=hip.EPI_OUT_F32)
    return out


def _several_tokens(context: Optional[torch.Tensor]) -> bool:
    return context is not None and context.dim() == 3 and context.shape[1] > 1


def _block_several_tokens(eng: UNetEngine, blk, sd, t: str, p: dict, t0: torch.Tensor, context: torch.Tensor, B: int, n: int,
                          P: dict, want32: bool = False):
    """``UNetEngine._block`` for a context of SEVERAL tokens (attention.py:239-243 as written): the engine folds the single-token
    attn2 of the VFace configuration into attn1's epilogue as a row bias; with more tokens attn2 is a real
    cross-attention between attn1 and the FeedForward -- norm2, to_q of the tokens, to_k / to_v of the context, ``vface_attention``
    with nk = the context length, to_out into the block's running sum.  ``t0``: that sum ``[B*n, c]``, fp32 or 16-bit."""
    c, M, a2m = p["c"], t0.shape[0], blk.attn2
    ln = eng._new(M, c)
    hip.layernorm(t0, p["ln1"][0], p["ln1"][1], ln, M=M, C_=c, ldx=c, ldy=c)
    no_bias = torch.zeros(B, c, dtype=torch.float32, device=t0.device)
    t1 = eng._attn1(ln, t0, p, eng._hook_plan(blk.attn1, B, n), no_bias, B, n, blk.attn1.heads)
    if "x2" not in P:
        P["x2"] = {"ln2": (eng._f32(sd[t + ".norm2.weight"]), eng._f32(sd[t + ".norm2.bias"])),
                   "wq": eng.pack_lin(sd, t + ".attn2.to_q", bias=False), "wk": eng.pack_lin(sd, t + ".attn2.to_k", bias=False),
                   "wv": eng.pack_lin(sd, t + ".attn2.to_v", bias=False), "wo": eng.pack_lin(sd, t + ".attn2.to_out.0")}
    x2 = P["x2"]
    hip.layernorm(t1, x2["ln2"][0], x2["ln2"][1], ln, M=M, C_=c, ldx=c, ldy=c)
    m, d2 = context.shape[1], a2m.heads * a2m.dim_head
    c16 = eng._new(B * m, context.shape[2])
    hip.cast_f32(context.reshape(B * m, -1).float().contiguous(), c16)
    q, k, v, att = eng._new(M, d2), eng._new(B * m, d2), eng._new(B * m, d2), eng._new(M, d2)
    eng._gemm(ln, x2["wq"], q)
    eng._gemm(c16, x2["wk"], k)
    eng._gemm(c16, x2["wv"], v)
    hip.attention(q, k, v, att, B=B, heads=a2m.heads, n=n, nk=m, dh=a2m.dim_head, ldq=d2, ldk=d2, ldv=d2, bsq=n * d2, bsk=m * d2,
                  bsv=m * d2, ldo=d2, bso=n * d2, scale=a2m.scale)
    if t1.dtype == torch.float32:
        t1b = eng._new(M, c, torch.float32)
        eng._gemm(att, x2["wo"], None, hw=n, residual32=t1, out32=t1b)
    else:
        t1b = eng._new(M, c)
        eng._gemm(att, x2["wo"], t1b, hw=n, residual=t1, ldr=t1.stride(0))
    return eng._ffn(t1b, p, n, want32)


def spatial_transformer_forward(mod, x: torch.Tensor, context: Optional[torch.Tensor]) -> torch.Tensor:
    eng, P = _engine_for(mod, x)
    sd = {("." + k): v for k, v in _sd(mod).items()}
    if "st" not in P:
        P["st"] = eng.pack_st(sd, "")
    p = dict(P["st"])
    a = _to_act(eng, x)
    if _several_tokens(context):
        # (GroupNorm, proj_in and proj_out + x as the separate launches of UNetEngine._st)
        c, hw = p["c"], a.H * a.W
        g = eng._gn(a, p["gn"], 1e-6, False)
        s32 = eng.stream32 and c % 8 == 0
        t0 = eng._new(a.M, c, torch.float32 if s32 else None)
        eng._gemm(g.t, p["proj_in"], None if s32 else t0, hw=hw, **({"out32": t0} if s32 else {}))
        t2 = _block_several_tokens(eng, mod.transformer_blocks[0], sd, ".transformer_blocks.0", p, t0, context, a.N, hw, P)
        out, cs, o32 = eng._new_target(a.M, c, hw)
        eng._gemm(t2, p["proj_out"], out, colstats=cs, hw=hw, out32=o32, **eng._resid(a))
        return _from_act(Act(out, a.N, a.H, a.W, cs, o32), x)
    a2 = _a2vec(eng, sd, ".transformer_blocks.0", context, a.N, p["c"], P)
    p["a2_slice"] = (0, p["c"])
    y = eng._st(a, p, mod, a2, None)
    return _from_act(y, x)


def transformer_block_forward(mod, x: torch.Tensor, context: Optional[torch.Tensor]) -> torch.Tensor:
    """``x`` [B, n, d] tokens."""
    eng, P = _engine_for(mod, x)
    sd = {("." + k): v for k, v in _sd(mod).items()}
    if "blk" not in P:
        P["blk"] = eng.pack_block(sd, "")
    p = P["blk"]
    B, n, d = x.shape
    if eng.stream32 and d % 8 == 0:
        t0 = x.reshape(B * n, d).float().contiguous()
    else:
        t0 = eng._new(B * n, d)
        hip.cast_f32(x.reshape(B * n, d).float().contiguous(), t0)
    if _several_tokens(context):
        return _block_several_tokens(eng, mod, sd, "", p, t0, context, B, n, P, want32=True)[1].reshape(B, n, d).to(x.dtype)
    a2 = _a2vec(eng, sd, "", context, B, d, P)
    t2, t2_32 = eng._block(t0, p, eng._hook_plan(mod.attn1, B, n), mod.attn1.heads, a2, B, n, want32=True)
    return t2_32.reshape(B, n, d).to(x.dtype)


def cross_attention_forward(mod, x: torch.Tensor, context: Optional[torch.Tensor], cfg: Optional[HookCfg]) -> torch.Tensor:
    """``CrossAttention.forward`` / the hooked closure on ``[B, n, d]`` tokens (attention.py:179-221, pnp_utils.py:94-287): self-attention
    (``context=None``) is the engine's hooked attn1 sequence without a row bias or a residual; a context of any length is three
    projections, ``vface_attention`` with nk = its length and to_out.  Returns the 16-bit result, as autocast does."""
    eng, _ = _engine_for(mod, x)
    pk = mod._packed(eng.dtype)
    B, n, d_in = x.shape
    d = mod.heads * mod.dim_head

    def to16(t):
        t = t.contiguous()
        if t.dtype == eng.dtype:
            return t
        o = torch.empty(t.shape, dtype=eng.dtype, device=eng.device)
        hip.cast_f32(t.float(), o)
        return o

    x16 = to16(x).reshape(B * n, d_in)
    out = eng._new(B * n, mod.to_out[0].weight.shape[0])
    if context is None:
        p = {"c": d, "wqkv": pk["wqkv"], "wo": {"w": pk["wo"], "b": pk["bo"]}, "wlin": pk["wlin"],
             "qk_src": (mod.to_q.weight, mod.to_k.weight)}
        eng._attn1(x16, None, p, plan_fusion(cfg, B, n), None, B, n, mod.heads, out=out)
    else:
        m = context.shape[1]
        c16 = to16(context).reshape(B * m, context.shape[2])
        q, k, v, att = eng._new(B * n, d), eng._new(B * m, d), eng._new(B * m, d), eng._new(B * n, d)
        hip.gemm(x16, pk["wq"], q, M=B * n, N=d, K=d_in, lda=d_in, ldc=d)
        hip.gemm(c16, pk["wk"], k, M=B * m, N=d, K=c16.shape[1], lda=c16.shape[1], ldc=d)
        hip.gemm(c16, pk["wv"], v, M=B * m, N=d, K=c16.shape[1], lda=c16.shape[1], ldc=d)
        hip.attention(q, k, v, att, B=B, heads=mod.heads, n=n, nk=m, dh=mod.dim_head, ldq=d, ldk=d, ldv=d, bsq=n * d,
                      bsk=m * d, bsv=m * d, ldo=d, bso=n * d, scale=mod.scale)
        hip.gemm(att, pk["wo"], out, M=B * n, N=out.shape[1], K=d, lda=d, ldc=out.shape[1], bias=pk["bo"])
    return out.reshape(B, n, -1)


def feedforward_forward(mod, x: torch.Tensor) -> torch.Tensor:
    """FeedForward (GEGLU -> Dropout(0) -> Linear), ``x`` [..., d]."""
    from . import packing
    eng, P = _engine_for(mod, x)
    if "ff" not in P:
        sd = _sd(mod)
        w, b = packing.pack_geglu(sd["net.0.proj.weight"].float().cpu(), sd["net.0.proj.bias"].float().cpu())
        P["ff"] = ({"w": eng._w16(w), "b": eng._f32(b)}, eng.pack_lin(sd, "net.2"))
    ff1, ff2 = P["ff"]
    d = x.shape[-1]
    x16 = eng._new(x.numel() // d, d)
    hip.cast_f32(x.reshape(-1, d).float().contiguous(), x16)
    hmid = eng._new(x16.shape[0], ff1["w"].shape[0] // 2)
    hip.gemm(x16, ff1["w"], hmid, M=x16.shape[0], N=ff1["w"].shape[0], K=d, lda=d, ldc=hmid.shape[1], bias=ff1["b"],
             flags=hip.EPI_GEGLU)
    out = eng._new(x16.shape[0], ff2["w"].shape[0], torch.float32)
    eng._gemm(hmid, ff2, out, flags=hip.EPI_OUT_F32)
    return out.reshape(*x.shape[:-1], out.shape[1]).to(x.dtype)


def geglu_forward(mod, x: torch.Tensor) -> torch.Tensor:
    from . import packing
    eng, P = _engine_for(mod, x)
    if "g" not in P:
        sd = _sd(mod)
        w, b = packing.pack_geglu(sd["proj.weight"].float().cpu(), sd["proj.bias"].float().cpu())
        P["g"] = {"w": eng._w16(w), "b": eng._f32(b)}
    g = P["g"]
    d = x.shape[-1]
    x16 = eng._new(x.numel() // d, d)
    hip.cast_f32(x.reshape(-1, d).float().contiguous(), x16)
    out = eng._new(x16.shape[0], g["w"].shape[0] // 2)
    hip.gemm(x16, g["w"], out, M=x16.shape[0], N=g["w"].shape[0], K=d, lda=d, ldc=out.shape[1], bias=g["b"], flags=hip.EPI_GEGLU)
    return out.reshape(*x.shape[:-1], out.shape[1]).to(x.dtype)
