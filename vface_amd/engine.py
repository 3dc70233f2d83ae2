"""Device-resident execution of the hooked ldm UNet on MI355X.

The nn.Modules in ``vface_amd.ldm`` only own parameters (with the reference's state-dict names); this
engine walks them and issues hand-written HIP kernels (``vface_amd/hip.py`` -> ``libvface_hip.so``):

* activations live in HBM as token-major / NHWC 16-bit matrices ``[N*H*W, C]`` -- the layout in which the
  reference's ``b c h w <-> b (h w) c`` rearranges (attention.py:284,287) are no-ops, every conv is an
  implicit GEMM over contiguous channels, and ``th.cat([h, hs.pop()], 1)`` (openaimodel.py:898) is two
  producers writing disjoint column ranges of one buffer;
* per-sample additive terms (the time-embedding projection of every ResBlock, and the single-token
  cross-attention, which reduces to ``to_out(to_v(ctx))`` broadcast over tokens -- SURVEY F11) are computed
  once per forward as small GEMMs and folded into GEMM epilogues as a row bias;
* the attn1 hook (pnp_utils.py:94-287) is executed from its configuration, not from the closure: "replace"
  is an index map inside the attention kernel, FSAI / mix are folded into the q,k projection weights, and
  the flow warp is one gather kernel on chunk 1's fused q|k.

There is no CPU path here.
"""
from __future__ import annotations

import os

import numpy as np
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch

from . import hip, packing
from .replay import _StepReplay, _between_events


@dataclass
class HookCfg:
    """Captured arguments of ``register_spa_attn_injection`` (pnp_utils.py:57) for one attn1 module."""
    switch_on: bool = True
    chunks: int = 3
    fusion: str = "replace"
    flow: Optional[torch.Tensor] = None  # [F-1, 2, h, w] fp32 on the device, or None
    split_ratio_fft: float = 0.8
    alpha: float = 0.8
    # which attention maps the flow smoothing applies to: "reference" = exactly pnp_utils.py:201 (`q.shape[1] == 4096`,
    # reshaped to 64 x 64: the 512 x 512 level-0 maps and nothing else -- at any other resolution the reference silently
    # skips the warp); "flow_hw" = the level whose token count equals h*w of the supplied flow field (identical at
    # 512 x 512; what a 768 x 768 clip -- BASELINE config 5 -- needs for the module to act at all)
    flow_gate: str = "reference"


class Act:
    """A 2-D view ``[rows, C]`` (stride ``(ld, 1)``) of a 16-bit device buffer, with its image geometry and,
    when its producer emitted them, the per-64-row-slice column statistics ``cs`` ``[rows/64, C, 2]`` (fp32 view)
    from which a following GroupNorm takes mean / rstd without re-reading the tensor.

    ``t32`` (optional) is the same activation as the fp32 residual-stream carrier: the un-rounded sum its producer's
    epilogue formed.  Residual adds and normalisations read it; only matrix-core operands read the 16-bit ``t``,
    which may then be absent (None) when no consumer needs it."""
    __slots__ = ("t", "N", "H", "W", "cs", "t32")

    def __init__(self, t: Optional[torch.Tensor], N: int, H: int, W: int, cs: Optional[torch.Tensor] = None,
                 t32: Optional[torch.Tensor] = None):
        for v in (t, t32):
            assert v is None or (v.dim() == 2 and v.stride(1) == 1)
        assert t is not None or t32 is not None
        self.t, self.N, self.H, self.W, self.cs, self.t32 = t, N, H, W, cs, t32

    @property
    def any(self):
        return self.t if self.t is not None else self.t32

    @property
    def C(self):
        return self.any.shape[1]

    @property
    def ld(self):
        return self.t.stride(0)

    @property
    def M(self):
        return self.any.shape[0]

    @property
    def src(self):
        """What a normalisation reads: the fp32 carrier when there is one."""
        return self.t32 if self.t32 is not None else self.t

    @property
    def hw(self):
        return self.H * self.W


def _dev_flow(flow, device) -> Optional[torch.Tensor]:
    """Accept the reference's ``list of [1,2,h,w]`` or a stacked tensor; return [F-1,2,h,w] fp32 on device."""
    if flow is None:
        return None
    if isinstance(flow, (list, tuple)):
        if len(flow) == 0:
            return None
        flow = torch.cat([f.reshape(1, 2, f.shape[-2], f.shape[-1]) for f in flow], 0)
    return flow.to(device=device, dtype=torch.float32).contiguous()


def flow_gate_hw(cfg: HookCfg, n: int, flow_hw):
    """The (h, w) of the maps to warp if the flow smoothing fires for an attention over ``n`` tokens, else None.
    ``flow_hw``: spatial size of the flow field in use (the local fields, or the clip's when frames are sharded)."""
    if flow_hw is None:
        return None
    h, w = int(flow_hw[0]), int(flow_hw[1])
    if cfg.flow_gate == "reference":
        if n != 4096:
            return None
        if (h, w) != (64, 64):   # the reference reshapes to 64 x 64 and adds the flow to a 64 x 64 grid (temporal_flow.py:43)
            raise RuntimeError(f"The size of the flow field ({h}, {w}) must match the 64 x 64 attention map "
                               "(pnp_utils.py:201-207, temporal_flow.py:43)")
        return 64, 64
    if cfg.flow_gate != "flow_hw":
        raise ValueError(f"flow_gate must be 'reference' or 'flow_hw', not {cfg.flow_gate!r}")
    return (h, w) if n == h * w else None


def plan_fusion(cfg: Optional[HookCfg], N: int, n: int, clip_flow_hw=None, live: Optional[int] = None) -> dict:
    """Map a hook configuration onto the kernels' mechanisms (pnp_utils.py:129-262).
    Returns fusion code, chunks, which folded weight to use, and the flow / v-broadcast options.  ``clip_flow_hw``: the
    flow field's (h, w) when frames are sharded (a one-frame shard has no local field but still takes part in the
    boundary exchange): ``warp_hw`` is then set even when ``flow`` is None.
    ``live``: the batch holds only the first ``live`` of the hook's ``chunks`` chunks (the sampler left the recon third out:
    every hook mode edits chunk k >= 1 from chunk 0 and chunk k alone, pnp_utils.py:133-262, so the chunks that ARE there
    compute exactly what they compute in the full batch); the plan's ``chunks`` is then ``live``, its fusion still the one the
    hook's own ``chunks`` selects."""
    pl = {"fusion": hip.FUSION_NONE, "chunks": 1, "wlin": None, "flow": None, "alpha": 0.8, "v_fixed": False,
          "staged": None, "warp_hw": None, "hook_chunks": 1}
    if cfg is None or not cfg.switch_on:
        return pl
    chunks = cfg.chunks
    if chunks not in (2, 3):
        return pl  # the reference edits nothing for other values
    there = chunks if live is None else live
    if not 1 <= there <= chunks:
        raise hip.VFaceHipError(f"hooked attn1: {there} live chunks of chunks={chunks}")
    if N % there:
        raise hip.VFaceHipError(f"hooked attn1: batch {N} is not divisible by its {there} chunk(s) (hook chunks={chunks})")
    pl["chunks"], pl["hook_chunks"] = there, chunks
    f = cfg.fusion
    if chunks == 2 or f == "replace":
        pl["fusion"] = hip.FUSION_REPLACE
    elif f in ("fft", "flow_fix", "fft_vfixed"):
        pl["fusion"] = hip.FUSION_LINEAR
        pl["wlin"] = ("fsai", 0.8 if f == "fft_vfixed" else cfg.split_ratio_fft)
        pl["v_fixed"] = f == "fft_vfixed"
        if f == "flow_fix":
            fhw = tuple(cfg.flow.shape[-2:]) if cfg.flow is not None else clip_flow_hw
            hw = flow_gate_hw(cfg, n, fhw)
            if hw is not None:
                nf = cfg.flow.shape[0] if cfg.flow is not None else 0
                if nf != N // there - 1:
                    raise RuntimeError(f"flow has {nf} fields for {N // there} frames "
                                       "(align_by_flow needs F-1, temporal_flow.py:231-233)")
                pl["flow"], pl["alpha"], pl["warp_hw"] = cfg.flow, cfg.alpha, hw
    elif f == "mix":
        pl["fusion"], pl["wlin"] = hip.FUSION_LINEAR, ("mix", 0.5)
    elif f in ("temporal", "adaIn"):
        pl["staged"] = f  # edits that are not a sample map or a folded weight: separate kernels on the qkv buffer
    else:
        pl["chunks"] = 1  # unknown fusion strings edit nothing in the reference
    if pl["chunks"] == 1 and pl["fusion"] != hip.FUSION_NONE:
        pl["fusion"], pl["wlin"], pl["flow"], pl["warp_hw"], pl["v_fixed"] = hip.FUSION_NONE, None, None, None, False   # chunk 0 alone: unedited
    return pl


def sample_map(kind: str, B: int, c: int) -> torch.Tensor:
    """The attention kernel's per-sample source map (int32 on the CPU) for a batch of B samples in chunks of c frames."""
    idx = torch.arange(B, dtype=torch.int32)
    if kind == "qk_replace":
        return idx % c
    if kind in ("share_qk", "share_v"):
        # the shared rows with a warp (UNetEngine._rows): slot 0 = chunk 1's warped q|k, slot 1 = chunk 0's q|k and the v of chunks 0, 1
        m = torch.where(idx < c, idx + c, idx)            # chunk 0 reads slot 1 (q|k and v)
        if kind == "share_qk":
            m = torch.where((idx >= c) & (idx < 2 * c), idx - c, m)      # chunk 1's q|k: slot 0 (its v stays in slot 1 = itself)
        return m
    if kind == "v_fixed":  # chunk 0 identity, chunk k >= 1 -> its first frame
        return torch.where(idx < c, idx, (idx // c) * c)
    raise ValueError(kind)


def fold_qk(kind: str, param: float, wq: torch.Tensor, wk: torch.Tensor) -> torch.Tensor:
    """The folded ``[2d, 2d]`` q|k weight of a linear hook fusion (``plan_fusion``'s ``wlin``: FSAI or mix), fp32 on the CPU."""
    wq, wk = wq.detach().float().cpu(), wk.detach().float().cpu()
    return packing.fold_fsai(wq, wk, param) if kind == "fsai" else packing.fold_mix(wq, wk, param)


def qkv_attention(qkv: torch.Tensor, att: torch.Tensor, *, B: int, n: int, d: int, heads: int, **maps):
    """Self-attention over a ``[rows, 3d]`` q|k|v buffer of n-token samples into ``att`` ``[rows, d]``: q, k and v are the column
    thirds of one buffer, the softmax scale is ``dh ** -0.5`` formed in fp32; ``maps``: ``hip.attention``'s sample maps / value sets."""
    dh = d // heads
    hip.attention(qkv, qkv[:, d:], qkv[:, 2 * d:], att, B=B, heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d, ldv=3 * d,
                  bsq=n * 3 * d, bsk=n * 3 * d, bsv=n * 3 * d, ldo=d, bso=n * d,
                  scale=float(np.float32(1.0) / np.sqrt(np.float32(dh))), **maps)   # (fp32 arithmetic: it fixes the bits)


@dataclass(frozen=True)
class _Rows:
    """Where a SpatialTransformer pass keeps its chunks: the whole batch, chunk after chunk, or the ``[A ; C]`` rows of
    ``UNetEngine._shared_block`` (A stands for chunks 0 AND 1).  Row numbers; built in one place, ``UNetEngine._rows``."""
    own: tuple       # per chunk: the first of its own rows in the LayerNorm output and in the projections' q|k|v rows
    qk: tuple        # per chunk: the first row of the attention's q|k|v buffer its fused q|k goes to; None: not needed
    lead: int        # rows of that buffer in front of the projections' (the slot of a warped chunk 1 that has no rows of its own)
    maps: tuple      # the attention's sample maps (q|k, v) as ``sample_map`` kinds, None: identity
    tail: tuple      # per tail launch: (first output row, rows, first attention-output row, first row-bias sample)


def _phase_form_pays(hw_in: int, cout: int) -> bool:
    """The four parity-phase launches of an upsampling conv each cover hw_in rows per sample: below ~200 tiles per launch the
    9-tap form on the upsampled grid fills the chip better.  The tile count is taken at a NOMINAL batch, so the choice -- and the
    bits -- do not depend on the batch: 48 samples since round 6 (one launch stream's half of the 32-frame headline, a rank's 16-frame
    share at N > 1), like the convolution kernels' own rules.  At 48 the 8x8 -> 16x16 upsampling at 1280 channels takes the phase form
    too (measured, profiles/r05_m / r06_j: 369 vs 434 us at 48 samples, 399 vs 829 at 96 -- and 369 vs 224 at 24, which the 8-frame
    clip pays); same-box A/B on the headline: 76.00 -> 75.42 ms/step.  VFACE_PHASE_NOMINAL24=1: the rule of rounds 2-5 (A/B)."""
    if os.environ.get("VFACE_NO_PHASE_UPSAMPLE") == "1":   # A/B switch for measurements
        return False
    if os.environ.get("VFACE_PHASE_NOMINAL24") == "1":
        return (24 * hw_in // 128) * (cout // 128) >= 400
    return (48 * hw_in // 128) * (cout // 128) >= 200


class UNetEngine(_StepReplay):
    """Packed weights + kernel sequencing for one ``UNetModel``; how a DDIM step's forward is launched: ``replay._StepReplay``."""

    def __init__(self, unet, dtype: torch.dtype = torch.float16, device=None):
        """``unet=None``: an engine for stand-alone sub-modules (``vface_amd.module_exec``); ``device`` is then required."""
        self.unet = unet
        self.dtype = dtype
        self._device = torch.device(device) if device is not None else None
        self._packed: Dict[str, dict] = {}
        self._maps: Dict[tuple, torch.Tensor] = {}
        self._version = None
        # the boundary exchange: a parallel.Exchange (ranks, batches of a clip or stream halves), set by parallel.set_boundary
        self.halo_exchange = None
        self.halo_flow: Optional[torch.Tensor] = None  # flow from the previous rank's last frame into our frame 0
        self.halo_hw = None                            # (h, w) of the clip's flow fields (set with halo_exchange)
        self.exchange_events = None                    # a list: (start, end) HIP events around every finish_exchange (bench.py)
        # norm3 + FeedForward of the level-0 transformer blocks (C = 320; also the 64- / 128-channel test models) as one
        # activation-stationary kernel (csrc/ffn.hip).  VFACE_FUSE_FFN=0: the three-kernel path (A/B switch).
        self.fuse_ffn = os.environ.get("VFACE_FUSE_FFN", "1") != "0"
        # GroupNorm-apply -> proj_in -> LayerNorm -> attn1 projection of the level-0 SpatialTransformers (C = 320; also the 64- /
        # 128-channel test models) as one activation-stationary kernel (csrc/stfront.hip): four launches and four HBM round trips
        # of the token matrix less per block.  VFACE_FUSE_FRONT=0: the separate launches (A/B switch).
        self.fuse_front = os.environ.get("VFACE_FUSE_FRONT", "1") != "0"
        # attn1's out-projection (+ attn2's row bias + residual) in front of the fused FeedForward, one launch: the block's running
        # sum after attention never exists in HBM (csrc/ffn.hip, PRE form).  VFACE_FUSE_TAIL=0: GEMM + fused FeedForward (A/B).
        self.fuse_tail = os.environ.get("VFACE_FUSE_TAIL", "1") != "0"
        # ... and the SpatialTransformer's proj_out + x_in + column statistics behind it, still one launch (ffn.hip POST form)
        self.fuse_post = os.environ.get("VFACE_FUSE_POST", "1") != "0"
        # the time-embedding chain (timestep embedding, time_embed, every ResBlock's emb_layers) as three few-row launches
        self.fuse_temb = os.environ.get("VFACE_FUSE_TEMB", "1") != "0"
        # the UNet's `out` layer (GroupNorm -> SiLU -> conv3x3 to 4 channels) as one launch (csrc/outconv.hip).  VFACE_FUSE_OUT=0: A/B
        self.fuse_out = os.environ.get("VFACE_FUSE_OUT", "1") != "0"
        # the concat buffers' fp32 carrier over all columns, read by the output blocks' GroupNorm (the layout up to round 4); default: the
        # carrier covers the skip columns only and the concat GroupNorm reads the 16-bit copy (forward_nhwc).  VFACE_CONCAT32=1: A/B
        self.concat32 = os.environ.get("VFACE_CONCAT32", "0") == "1"
        self.interior16 = os.environ.get("VFACE_INTERIOR16", "1") != "0"      # (see _st; VFACE_INTERIOR16=0: fp32 interior sums, A/B)
        self._shape_ok: Dict[tuple, bool] = {}         # (_supported)
        # the batch holds only the first `live_chunks` chunks of the hooks' three (the sampler's dead-branch elimination leaves
        # the recon third out: DDIMSampler.drop_dead_branches); None = every chunk is there
        self.live_chunks: Optional[int] = None
        # The batch is the sampler's own [x ; x ; inv_t] with t repeated (ddim_w_inv.py:632-655): chunks 0 and 1 enter the UNet
        # with IDENTICAL inputs and diverge only where attn2's row bias (the context) is first added.  The sampler states it per
        # call (DDIMSampler.p_sample_ddim_with_inverse; never true for a batch handed in through apply_model): the first
        # ResBlock and the first SpatialTransformer's front -- and, where the hook leaves chunk 1's q,k equal to chunk 0's
        # (no hook, `replace`, `fft`), its attention -- then run on 2F samples, chunk 0 reading chunk 1's rows (_shared_block).
        self.share_prefix = False
        # fp32 residual stream: residual sums are carried between kernels in fp32, 16-bit copies exist only
        # where a matrix-core operand needs them.  VFACE_STREAM32=0 restores the all-16-bit activations (A/B switch).
        self.stream32 = os.environ.get("VFACE_STREAM32", "1") != "0"
        # GroupNorm-apply + SiLU of a ResBlock fused into the patch-staged convolution's operand path (openaimodel.py:201-205,
        # 225-232 `GroupNorm32 -> SiLU -> conv`): "both" = in_layers and out_layers; "out" = out_layers only (the in_layers
        # normalisation then reads the fp32 carrier in its own pass instead of the 16-bit copy); "off" (default) = separate
        # gn_apply passes.  Exact (bit-identical to the separate pass on the same input) but MEASURED SLOWER on this kernel:
        # the ~70 vector instructions per 1-KiB patch piece sit in the K-tile period's critical path -- 28.22 vs 27.49 ms per
        # DDIM step (conv 9.46 vs 7.77 ms, gn_apply 0 vs 1.0 ms), DESIGN 4 -- so it is opt-in.
        self.fuse_gn = os.environ.get("VFACE_FUSE_GN", "off")
        self._halo_k = 0                               # ordinal of the next boundary exchange of this forward (_halo_start)
        self._a2_lru: Dict[int, tuple] = {}            # (context_projections: a few contexts, most recently used last)
        self._a2_cache: Optional[tuple] = None         # the entry a graph capture pins in front of them (replay._capture)
        self._init_replay()
        hip.load()

    # ------------------------------------------------------------------ weights
    @property
    def device(self):
        return self._device if self._device is not None else next(self.unet.parameters()).device

    def _w16(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.device, dtype=self.dtype).contiguous()

    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def pack(self):
        """(Re)build every packed device weight from the module parameters."""
        u = self.unet
        if not next(u.parameters()).is_cuda:
            raise hip.VFaceHipError("UNetModel parameters are not on the GPU: the VFace path has no CPU fallback")
        P = self._packed = {}
        sd = {k: v.detach() for k, v in u.state_dict().items()}
        cpu = lambda k: sd[k].float().cpu()

        conv3 = lambda prefix: self.pack_conv3(sd, prefix)
        lin = lambda prefix, bias=True, conv=False: self.pack_lin(sd, prefix, bias, conv)

        P["time_embed.0"] = lin("time_embed.0")
        P["time_embed.2"] = lin("time_embed.2")
        emb_w, emb_b, off = [], [], 0
        vcat_w, voff = [], 0
        for kind, prefix, mod in u.layer_table():
            if kind == "conv":
                P[prefix] = conv3(prefix)
            elif kind == "down":
                P[prefix] = conv3(prefix + ".op")
            elif kind == "up":
                P[prefix] = self.pack_up(sd, prefix + ".conv")
            elif kind == "res":
                d = self.pack_res(sd, prefix)
                cout = d["conv1"]["cout"]
                emb_w.append(sd[prefix + ".emb_layers.1.weight"].float())
                emb_b.append(sd[prefix + ".emb_layers.1.bias"].float())
                d["emb_slice"] = (off, off + cout)
                off += cout
                P[prefix] = d
            elif kind == "st":
                d = self.pack_st(sd, prefix)
                d["a2_slice"] = (voff, voff + d["c"])
                vcat_w.append(sd[prefix + ".transformer_blocks.0.attn2.to_v.weight"].float())
                voff += d["c"]
                P[prefix] = d
        P["emb_all"] = {"w": self._w16(torch.cat(emb_w, 0)), "b": self._f32(torch.cat(emb_b, 0)), "n": off}
        P["a2_v_all"] = {"w": self._w16(torch.cat(vcat_w, 0)), "n": voff}
        P["out.gn"] = (self._f32(sd["out.0.weight"]), self._f32(sd["out.0.bias"]))
        P["out.conv"] = conv3("out.2")
        self._version = self._param_version()

    # ---- per-layer packers (also used for stand-alone sub-modules, vface_amd/module_exec.py); `sd`: name -> tensor
    def pack_conv3(self, sd, prefix):
        w = sd[prefix + ".weight"]
        d = {"w": self._w16(packing.pack_conv3x3(w.detach().float().cpu())), "b": self._f32(sd[prefix + ".bias"]),
             "cin": w.shape[1], "cinp": (w.shape[1] + 7) // 8 * 8, "cout": w.shape[0]}
        return d

    def pack_up(self, sd, prefix):
        d = self.pack_conv3(sd, prefix)
        # nearest x2 + conv3x3 = four parity-phase 2x2 convs with pre-summed taps (4/9 of the multiply-adds)
        d["phases"] = self._w16(packing.pack_upsample_phases(sd[prefix + ".weight"].detach().float().cpu()))
        return d

    def pack_lin(self, sd, prefix, bias=True, conv=False):
        w = sd[prefix + ".weight"]
        w = w.reshape(w.shape[0], w.shape[1]) if conv else w
        return {"w": self._w16(w), "b": self._f32(sd[prefix + ".bias"]) if bias else None}

    def pack_res(self, sd, prefix):
        d = {"in_gn": (self._f32(sd[prefix + ".in_layers.0.weight"]), self._f32(sd[prefix + ".in_layers.0.bias"])),
             "conv1": self.pack_conv3(sd, prefix + ".in_layers.2"),
             "out_gn": (self._f32(sd[prefix + ".out_layers.0.weight"]), self._f32(sd[prefix + ".out_layers.0.bias"])),
             "conv2": self.pack_conv3(sd, prefix + ".out_layers.3")}
        if (prefix + ".skip_connection.weight") in sd:
            d["skip"] = self.pack_lin(sd, prefix + ".skip_connection", conv=True)
            wsk = sd[prefix + ".skip_connection.weight"]
            if d["conv2"]["cinp"] % 64 == 0 and wsk.shape[1] % 64 == 0:
                # second conv + 1x1 shortcut in one K loop (vface_conv3x3_plus_1x1): weights side by side, biases summed
                d["conv2_skip"] = dict(d["conv2"], c2=wsk.shape[1],
                                       w=torch.cat([d["conv2"]["w"], d["skip"]["w"]], 1).contiguous(),
                                       b=(d["conv2"]["b"] + d["skip"]["b"]).contiguous())
        return d

    def pack_block(self, sd, t):
        """BasicTransformerBlock at state-dict prefix ``t``: attn1 / ff / norms (+ attn2's out projection; its to_v is
        stacked with the other blocks' by the UNet packer)."""
        cpu = lambda k: sd[k].detach().float().cpu()
        ffw, ffb = packing.pack_geglu(cpu(t + ".ff.net.0.proj.weight"), cpu(t + ".ff.net.0.proj.bias"))
        return {"ln1": (self._f32(sd[t + ".norm1.weight"]), self._f32(sd[t + ".norm1.bias"])),
                "ln3": (self._f32(sd[t + ".norm3.weight"]), self._f32(sd[t + ".norm3.bias"])),
                "wqkv": self._w16(packing.pack_qkv(sd[t + ".attn1.to_q.weight"], sd[t + ".attn1.to_k.weight"],
                                                  sd[t + ".attn1.to_v.weight"])),
                "wo": self.pack_lin(sd, t + ".attn1.to_out.0"),
                "ff1": {"w": self._w16(ffw), "b": self._f32(ffb)}, "ff2": self.pack_lin(sd, t + ".ff.net.2"),
                # fused FeedForward (csrc/ffn.hip): ff.net[2] in the order GEMM 1's accumulators hand the hidden units over --
                # packed only for the widths that kernel takes (a C = 1280 block would hold 13 MB of dead copy)
                "ff2p": (self._w16(packing.pack_ffn_w2(cpu(t + ".ff.net.2.weight")))
                         if self.fuse_ffn and hip.ffn_fused_width_supported(sd[t + ".norm1.weight"].shape[0]) else None),
                # the same kernel with attn1's out-projection in front (vface_attn_out_ffn_fused): [to_out ; ff.net[0] (k permuted)]
                "tail_w": (self._w16(packing.pack_attn_out_ffn(cpu(t + ".attn1.to_out.0.weight"), ffw))
                           if self.fuse_ffn and self.fuse_tail and hip.ffn_fused_width_supported(sd[t + ".norm1.weight"].shape[0])
                           else None),
                "a2_out": self.pack_lin(sd, t + ".attn2.to_out.0"), "c": sd[t + ".norm1.weight"].shape[0],
                "wlin": {}, "attn1_name": t + ".attn1",
                "qk_src": (sd[t + ".attn1.to_q.weight"], sd[t + ".attn1.to_k.weight"])}

    def pack_st(self, sd, prefix):
        d = self.pack_block(sd, prefix + ".transformer_blocks.0")
        d.update({"gn": (self._f32(sd[prefix + ".norm.weight"]), self._f32(sd[prefix + ".norm.bias"])),
                  "proj_in": self.pack_lin(sd, prefix + ".proj_in", conv=True),
                  "proj_out": self.pack_lin(sd, prefix + ".proj_out", conv=True)})
        c = d["c"]
        d["front_w"] = None
        if self.fuse_front and hip.st_front_supported(128, c, 128):      # (the widths csrc/stfront.hip takes)
            t = prefix + ".transformer_blocks.0.attn1"
            w_in = sd[prefix + ".proj_in.weight"].detach().float().cpu().reshape(c, c)
            w_p = packing.pack_qkv(sd[t + ".to_q.weight"], sd[t + ".to_k.weight"], sd[t + ".to_v.weight"]).detach().float().cpu()
            d["front_w"] = self._w16(packing.pack_st_front(w_in, w_p))
        d["tail_post"] = False
        if d.get("tail_w") is not None and self.fuse_post:
            # proj_out's rows behind the tail's weight stream (vface_attn_out_ffn_proj_fused), k columns in the stream's order
            w_po = sd[prefix + ".proj_out.weight"].detach().float().cpu().reshape(c, c)
            d["tail_w"] = torch.cat([d["tail_w"], self._w16(w_po[:, packing.ffn_w2_perm(c)])], 0).contiguous()
            d["tail_post"] = True
        return d

    def _param_version(self):
        return tuple(p._version for p in self.unet.parameters())

    def _ensure_packed(self):
        if not self._packed or self._version != self._param_version():
            self.pack()

    def _wlin(self, st: dict, kind: str, param: float) -> torch.Tensor:
        key = (kind, round(float(param), 9))
        if key not in st["wlin"]:
            st["wlin"][key] = self._w16(fold_qk(kind, param, *st["qk_src"]))
        return st["wlin"][key]

    def _map(self, kind: str, B: int, c: int) -> torch.Tensor:
        key = (kind, B, c)
        if key not in self._maps:
            self._maps[key] = sample_map(kind, B, c).to(self.device)
        return self._maps[key]

    # ------------------------------------------------------------------ primitive steps
    def _new(self, rows: int, cols: int, dtype=None) -> torch.Tensor:
        return torch.empty(rows, cols, dtype=dtype or self.dtype, device=self.device)

    def _new_target(self, rows: int, cols: int, hw: int, need16: bool = True):
        """A fresh output ``(16-bit buffer | None, column statistics | None, fp32 carrier | None)``: statistics when the
        image size allows (hw % 64 == 0); the carrier when the fp32 residual stream is on (and then the 16-bit copy only
        if a matrix-core operand will read it)."""
        s32 = self.stream32 and cols % 8 == 0
        return (self._new(rows, cols) if (need16 or not s32) else None, self._new_cs(rows, cols, hw),
                self._new(rows, cols, torch.float32) if s32 else None)

    def _new_cs(self, rows: int, cols: int, hw: int) -> Optional[torch.Tensor]:
        if hw % 64 or cols % 4:
            return None
        return torch.empty(rows // 64, cols, 2, dtype=torch.float32, device=self.device)

    def _gemm(self, a: torch.Tensor, w: dict, out: Optional[torch.Tensor], hw: int = 0, **kw):
        K = a.shape[1]
        if hw > 1 and "rowbias" not in kw:
            kw["rows_per_sample"] = hw   # split-K decided per sample: a frame's bits do not depend on its batch
        hip.gemm(a, w["w"], out, M=a.shape[0], N=w["w"].shape[0], K=K, lda=a.stride(0),
                 ldc=out.stride(0) if out is not None else 0, ldw=w["w"].shape[1], bias=w.get("b"), **kw)

    @staticmethod
    def _resid(x) -> dict:
        """Residual operand of an epilogue: the fp32 carrier when the tensor has one."""
        if isinstance(x, Act):
            if x.t32 is not None:
                return {"residual32": x.t32}
            return {"residual": x.t, "ldr": x.t.stride(0)}
        if x.dtype == torch.float32:
            return {"residual32": x}
        return {"residual": x, "ldr": x.stride(0)}

    def _gn(self, x: Act, gn, eps: float, silu: bool) -> Act:
        # (the fp32 carrier where there is one.  Reading the 16-bit copy in EVERY ResBlock -- 2 B per element instead of 4 -- was
        #  measured in round 5: -0.1 ms of an 83 ms step for +0.6 % of the error budget, profiles/r05_h: not taken; the concat
        #  GroupNorms, whose carrier had no other reader, do read 16 bits: forward_nhwc)
        src = x.src
        if x.cs is not None:
            st = hip.groupnorm_stats_from_cols(x.cs, nimg=x.N, hw=x.hw, C_=x.C, eps=eps)
        else:
            st = hip.groupnorm_stats(src, nimg=x.N, hw=x.hw, C_=x.C, ldx=src.stride(0), eps=eps)
        y = self._new(x.M, x.C)
        hip.groupnorm_apply(src, st, gn[0], gn[1], y, nimg=x.N, hw=x.hw, C_=x.C, ldx=src.stride(0), ldy=x.C, silu=silu)
        return Act(y, x.N, x.H, x.W)

    def _conv(self, x: Act, w: dict, tgt, stride=1, upsample=False, rowbias=None, residual=None, out_f32=False,
              stream=True, gn_ab=None) -> Act:
        """``tgt``: None (allocate) or ``(16-bit out view | None, colstats view | None, fp32 carrier view | None)``.
        ``residual``: an ``Act`` / tensor added in the epilogue.  ``stream=False``: a branch activation (consumed by one
        GEMM / GroupNorm only): 16-bit output, no fp32 carrier."""
        VH, VW = (2 * x.H, 2 * x.W) if upsample else (x.H, x.W)
        OH, OW = (VH - 1) // stride + 1, (VW - 1) // stride + 1
        if tgt is None:
            if out_f32:
                out, cs, o32 = self._new(x.N * OH * OW, w["cout"], torch.float32), None, None
            elif not stream:
                out, cs, o32 = self._new(x.N * OH * OW, w["cout"]), self._new_cs(x.N * OH * OW, w["cout"], OH * OW), None
            else:
                out, cs, o32 = self._new_target(x.N * OH * OW, w["cout"], OH * OW)
        else:
            out, cs, o32 = tgt
        assert x.C == w["cinp"], (x.C, w["cinp"])
        ldy = out.stride(0) if out is not None else 0
        if upsample and "phases" in w and _phase_form_pays(x.H * x.W, w["cout"]) and residual is None and not out_f32 \
                and (cs is None or (x.H * x.W) % 64 == 0):
            hip.upsample2x_conv3x3(x.t, w["phases"], out, nimg=x.N, H=x.H, W=x.W, cin=w["cinp"], cout=w["cout"], ldx=x.ld,
                                   ldy=ldy, bias=w["b"], rowbias=rowbias, colstats=cs, out32=o32)
            return Act(out, x.N, OH, OW, cs, o32)
        hip.conv3x3(x.t, w["w"], out, nimg=x.N, H=x.H, W=x.W, cin=w["cinp"], cout=w["cout"], ldx=x.ld,
                    ldy=ldy, stride=stride, upsample=upsample, bias=w["b"], rowbias=rowbias,
                    flags=hip.EPI_OUT_F32 if out_f32 else 0, colstats=cs, out32=o32, gn_ab=gn_ab, gn_silu=gn_ab is not None,
                    **(self._resid(residual) if residual is not None else {}))
        return Act(out, x.N, OH, OW, cs, o32)

    def _gn_fusable(self, x: Act, w: dict, which: str) -> bool:
        """Can GroupNorm-apply + SiLU of ``x`` ride in the operand path of the 3x3 convolution ``w``?  Needs producer-side
        column statistics, a 16-bit copy of ``x`` and a launch that runs the patch-staged kernel."""
        mode = self.fuse_gn
        if w["cout"] % 128:               # the fused form exists in the 128-wide tile only (the 160-wide one spilled: not built since round 6)
            return False
        if mode.endswith("128"):          # (the spelling of rounds 4-5, when "out" / "both" also took the spilled 160-wide form)
            mode = mode[:-3]
        if mode == "off" or (which == "in" and mode != "both"):
            return False
        return x.cs is not None and x.t is not None and x.C == w["cinp"] and \
            hip.conv_uses_patch_kernel(x.H, x.W, w["cinp"], w["cout"], 3, 1, False) == 1

    def _res(self, x: Act, p: dict, emb_all: torch.Tensor, out) -> Act:
        """ResBlock._forward (openaimodel.py:255-275), non-updown, no scale-shift."""
        a, b = p["emb_slice"]
        if self._gn_fusable(x, p["conv1"], "in"):
            ab = hip.groupnorm_coeffs_from_cols(x.cs, p["in_gn"][0], p["in_gn"][1], nimg=x.N, hw=x.hw, C_=x.C, eps=1e-5)
            h = self._conv(x, p["conv1"], None, rowbias=emb_all[:, a:b], stream=False, gn_ab=ab)
        else:
            h = self._gn(x, p["in_gn"], 1e-5, True)
            h = self._conv(h, p["conv1"], None, rowbias=emb_all[:, a:b], stream=False)
        gn2 = None
        if self._gn_fusable(h, p["conv2"], "out"):
            gn2 = hip.groupnorm_coeffs_from_cols(h.cs, p["out_gn"][0], p["out_gn"][1], nimg=h.N, hw=h.hw, C_=h.C, eps=1e-5)
        else:
            h = self._gn(h, p["out_gn"], 1e-5, True)
        if "conv2_skip" in p and os.environ.get("VFACE_NO_SKIP_FUSION") != "1":   # (env: A/B switch for measurements)
            w = p["conv2_skip"]
            o, cs, o32 = self._new_target(x.M, w["cout"], x.hw) if out is None else out
            hip.conv3x3_plus_1x1(h.t, x.t, w["w"], o, nimg=x.N, H=x.H, W=x.W, cin=w["cinp"], c2=w["c2"], cout=w["cout"],
                                 ldx=h.ld, ldx2=x.ld, ldy=o.stride(0) if o is not None else 0, bias=w["b"], colstats=cs,
                                 out32=o32, gn_ab=gn2, gn_silu=gn2 is not None)
            return Act(o, x.N, x.H, x.W, cs, o32)
        if "skip" in p:
            if self.stream32 and p["conv2"]["cout"] % 8 == 0:
                skip = self._new(x.M, p["conv2"]["cout"], torch.float32)
                self._gemm(x.t, p["skip"], None, hw=x.H * x.W, out32=skip)
            else:
                skip = self._new(x.M, p["conv2"]["cout"])
                self._gemm(x.t, p["skip"], skip, hw=x.H * x.W)
        else:
            skip = x
        return self._conv(h, p["conv2"], out, residual=skip, gn_ab=gn2)

    def _hook_plan(self, attn1, N: int, n: int) -> dict:
        """``plan_fusion`` of the hook registered on ``attn1`` for N samples of n tokens on this engine (its frame shard, its live chunks)."""
        fw = attn1.__dict__.get("forward")
        if fw is not None and not getattr(fw, "_vface", False):
            raise hip.VFaceHipError("attn1.forward was replaced by a closure this engine does not know; use "
                                    "vface_amd.ldm.models.pnp_utils.register_spa_attn_injection")
        return plan_fusion(getattr(attn1, "_vface_cfg", None), N, n, self.halo_hw if self.halo_exchange is not None else None,
                           self.live_chunks)

    def _attn1(self, xln: torch.Tensor, resid: Optional[torch.Tensor], p: dict, pl: dict, a2vec: Optional[torch.Tensor], N: int,
               n: int, heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A hooked attn1 behind the separate launches, every plan ``pl`` (``_hook_plan``): ``_attn1_att``, then ``_attn1_out``.
        ``resid`` 16-bit -> 16-bit result; ``resid`` fp32 (the residual stream) -> fp32 result, no 16-bit copy; ``resid`` None: a
        stand-alone attention (``module_exec``), no residual, into the 16-bit ``out``."""
        d = p["c"]
        res_kw = {}
        if resid is not None and resid.dtype == torch.float32:
            res_kw = {"residual32": resid, "out32": self._new(N * n, d, torch.float32)}
        elif resid is not None:
            out, res_kw = self._new(N * n, d), {"residual": resid, "ldr": resid.stride(0)}
        att = self._attn1_att(xln, self._new(N * n, 3 * d), p, pl, N // pl["chunks"], n, heads)
        self._attn1_out(att, p, pl, a2vec, n, out, **res_kw)
        return res_kw.get("out32", out)

    def _attn1_out(self, att: torch.Tensor, p: dict, pl: dict, a2vec: Optional[torch.Tensor], n: int, out: Optional[torch.Tensor],
                   **res_kw):
        """The end of a hooked attn1: its out-projection + bias + attn2's row bias + residual as one GEMM.  ``out`` 16-bit, or None
        with ``residual32`` / ``out32`` (the fp32 residual stream).  Split-K belongs to the plan: the staged modes ("temporal",
        "adaIn") launch with it allowed (and do split at d = 1280, n = 64), every other plan without a workspace."""
        d = p["c"]
        o = out if out is not None else res_kw["out32"]
        hip.gemm(att, p["wo"]["w"], out, M=att.shape[0], N=o.shape[1], K=d, lda=d, ldc=out.stride(0) if out is not None else 0, ldw=d,
                 bias=p["wo"]["b"], rowbias=a2vec, rows_per_sample=n, split_k=pl["staged"] is not None, **res_kw)

    def _fused_qk(self, own: torch.Tensor, first: torch.Tensor, wlin: torch.Tensor, dst: torch.Tensor, rows: int, d: int):
        """The dual-source q|k projection of a linear hook fusion: ``[own | first]`` (K = 2d; ``first``: chunk 0's rows
        of the same LayerNorm output) times the folded weight ``_wlin``."""
        hip.gemm(own, wlin, dst, M=rows, N=2 * d, K=2 * d, lda=own.stride(0), ldc=dst.stride(0), ldw=2 * d, a2=first,
                 lda2=first.stride(0), k1=d, split_k=False)

    def _warp(self, T: torch.Tensor, dst: torch.Tensor, pl: dict, F_: int, n: int, d: int, halo: Optional[torch.Tensor]):
        """The flow warp of chunk 1's fused q|k ``T`` ``[F n, 2d]`` into its rows of a qkv buffer; ``halo``: the previous rank's last
        frame of ``T`` when frames are sharded (None on the first rank and on an unsharded clip)."""
        h, w = pl["warp_hw"]
        hip.flow_warp(T, dst, pl["flow"], F=F_, h=h, w=w, C_=2 * d, ld_src=2 * d, fs_src=n * 2 * d, ld_dst=3 * d,
                      fs_dst=n * 3 * d, alpha=pl["alpha"], prev=halo, ld_prev=2 * d,
                      flow_prev=self.halo_flow if halo is not None else None)

    def _rows(self, pl: dict, F_: int, n: int, L: Optional[int] = None) -> _Rows:
        """The row layout of a pass under plan ``pl`` with F_ frames of n tokens per chunk: the whole batch, or (``L``: its chunks)
        the ``[A ; C]`` rows of ``_shared_block``.  Shared, the attention runs over [A ; C] as it stands -- chunk 1's FSAI(q0, q0)
        is q0 -- unless the flow warp makes chunk 1's q|k differ from chunk 0's: then over three sample slots -- slot 0 = the warped
        q|k of chunk 1, slot 1 = A (q|k of chunk 0, v of chunks 0 and 1), slot 2 = C -- addressed through the sample maps.  Its
        tail, where attn2's row bias separates chunk 0 from chunk 1, is two launches: rows A with chunk 0's bias -> chunk 0, rows
        [A ; C] with chunk 1's and 2's -> chunks 1, 2."""
        Fn = F_ * n
        qk_map = "qk_replace" if pl["fusion"] == hip.FUSION_REPLACE else None
        if L is None:
            own = tuple(ch * Fn for ch in range(pl["chunks"]))
            return _Rows(own, own, 0, (qk_map, "v_fixed" if pl["v_fixed"] else None), ((0, pl["chunks"] * Fn, 0, 0),))
        warp = pl["warp_hw"] is not None
        assert (L == 3 or not warp) and not pl["v_fixed"]
        lead = Fn if warp else 0
        return _Rows((0, 0, Fn)[:L], (None, 0 if warp else None, lead + Fn)[:L], lead,
                     ("share_qk", "share_v") if warp else (qk_map, None), ((0, Fn, 0, 0), (Fn, (L - 1) * Fn, lead, F_)))

    def _attn1_att(self, ln: Optional[torch.Tensor], buf: torch.Tensor, p: dict, pl: dict, F_: int, n: int, heads: int,
                   lay: Optional[_Rows] = None, projected: bool = False) -> torch.Tensor:
        """A hooked attn1 (pnp_utils.py:94-287) from the LayerNorm output ``ln`` through the q|k|v buffer ``buf`` to the attention
        output -- the one launch sequence of every plan, on the whole batch and on the shared rows (``lay``: ``_rows``, default the
        whole batch of F_ frames per chunk); ``_attn1_out`` or a fused tail ends it:
          no hook      one q|k|v projection over the batch, attention;
          replace      chunk 0's q|k|v and the other chunks' v, attention with every chunk reading chunk 0's q, k (scores once per
                       frame where the kernel has that form, else through the q|k sample map);
          linear       (fft / flow_fix / fft_vfixed / mix) the same two projections, then chunk k >= 1's q|k as ONE dual-source GEMM
                       ``[own | chunk 0] @ wlin`` (``_fused_qk``); flow_fix warps chunk 1's along the flow on the way into ``buf``
                       (``_warp``); fft_vfixed reads v through the first-frame map;
          staged       (temporal / adaIn, pnp_utils.py:145-160: edits that are neither a sample map nor a folded weight) the full
                       projection with split-K allowed, the edit of chunk k >= 1's q, k by its own kernels (``_staged_edit``), attention.
        ``projected``: the fused front already wrote chunk 0's q|k|v and the other chunks' v (``_st``; ``ln`` is then only needed by
        the linear fusions); otherwise those GEMMs (one over the whole batch when no hook edits it) are issued here, K = ``ln``'s width.
        Frames sharded across ranks and a flow warp: the one-neighbour boundary exchange sits between chunk 1's
        fused projection and the warp, and the launches that do not depend on it are issued behind its start.  This order decides
        whether the ranks' calls pair up and where the hipGraph segments are cut (``replay._GraphSegments``)."""
        d = p["c"]
        fusion, chunks = pl["fusion"], pl["chunks"]
        Fn = F_ * n
        lay = lay or self._rows(pl, F_, n)
        qkv = buf[lay.lead:]

        def project(split_k=False):
            if projected:
                return
            M, K = qkv.shape[0], ln.shape[1]
            g = lambda a, w, o, rows, cols: hip.gemm(a, w, o, M=rows, N=cols, K=K, lda=ln.stride(0), ldc=3 * d, ldw=K, split_k=split_k)
            if fusion == hip.FUSION_NONE:
                g(ln, p["wqkv"], qkv, M, 3 * d)
            else:
                g(ln, p["wqkv"], qkv, Fn, 3 * d)                                         # chunk 0: q, k, v as projected
                g(ln[Fn:], p["wqkv"][2 * d:], qkv[Fn:, 2 * d:], M - Fn, d)              # other chunks: v only, the fusion writes their q, k

        if pl["staged"]:
            project(split_k=True)
            self._staged_edit(pl["staged"], qkv, F_, n, d, chunks)
        elif fusion != hip.FUSION_LINEAR:
            project()
        else:
            wlin = self._wlin(p, *pl["wlin"])
            warp = pl["warp_hw"] is not None
            # every rank of a sharded clip takes part in the boundary exchange, a one-frame shard (no local field) too
            sharded = warp and self.halo_exchange is not None
            T = self._new(Fn, 2 * d) if warp else None

            def fused(ch):          # (own rows, then the structure rows = chunk 0's LayerNorm output)
                if lay.qk[ch] is not None:
                    dst = T if (warp and ch == 1) else buf[lay.qk[ch]:lay.qk[ch] + Fn, :2 * d]
                    self._fused_qk(ln[lay.own[ch]:], ln, wlin, dst, Fn, d)

            halo = None
            if sharded:
                fused(1)
                # my last frame's fused q|k goes to the next rank; the previous rank's arrives while chunk 0 / chunk 2 /
                # the v projections below are computed
                handle = self._halo_start(T[(F_ - 1) * n:])
            project()
            for ch in range(2 if sharded else 1, chunks):
                fused(ch)
            if sharded:
                halo = self._halo_finish(handle)
            if warp:
                self._warp(T, buf[lay.qk[1]:lay.qk[1] + Fn, :2 * d], pl, F_, n, d, halo)
        att = self._new(buf.shape[0], d)
        S, hc = buf.shape[0] // n, pl["hook_chunks"]
        qk_map, v_map = (self._map(kind, S, F_) if kind else None for kind in lay.maps)
        if fusion == hip.FUSION_REPLACE and S > F_ and hip.load().vface_attention_shared_scores_supported(d // heads, hc):
            # every chunk attends with q,k of chunk 0 (pnp_utils.py:136-142): softmax once per frame, one value set per chunk there
            qkv_attention(buf, att, B=F_, n=n, d=d, heads=heads, v_map=v_map, v_sets=hc, v_sets_live=S // F_, set_stride=F_)
        else:
            qkv_attention(buf, att, B=S, n=n, d=d, heads=heads, qk_map=qk_map, v_map=v_map)
        return att

    def _block(self, t0: torch.Tensor, p: dict, pl: dict, heads: int, a2vec: torch.Tensor, N: int, n: int, want32: bool = False):
        """BasicTransformerBlock._forward (attention.py:239-243) on the block's running sum ``t0`` ``[N*n, c]`` (fp32 when the
        residual stream is on, else 16-bit): returns its last value as the 16-bit operand of the next projection (and, if
        ``want32``, as fp32 too).  ``pl``: ``_hook_plan``; ``a2vec``: the single-token cross-attention's contribution, fp32 ``[N, c]``."""
        c, M = p["c"], t0.shape[0]
        ln = self._new(M, c)
        hip.layernorm(t0, p["ln1"][0], p["ln1"][1], ln, M=M, C_=c, ldx=c, ldy=c)
        return self._ffn(self._attn1(ln, t0, p, pl, a2vec, N, n, heads), p, n, want32)

    def _ffn(self, t1: torch.Tensor, p: dict, n: int, want32: bool = False):
        """``x + ff(norm3(x))`` (attention.py:243) on the block's running sum ``t1`` (fp32 with the residual stream, else 16-bit)."""
        c, M = p["c"], t1.shape[0]
        t2 = self._new(M, c)
        t2_32 = self._new(M, c, torch.float32) if want32 else None
        if self.fuse_ffn and t1.dtype == torch.float32 and p["ff2p"] is not None and self._ffn_ok(M, c):
            # norm3 -> ff.net[0] (GEGLU) -> ff.net[2] -> + x in ONE launch (csrc/ffn.hip): the [M, 4c] hidden matrix never exists
            hip.ffn_fused(t1, p["ln3"][0], p["ln3"][1], p["ff1"]["w"], p["ff1"]["b"], p["ff2p"], p["ff2"]["b"], t2, M=M, C_=c,
                          out32=t2_32)
            return (t2, t2_32) if want32 else t2
        ln = self._new(M, c)
        hip.layernorm(t1, p["ln3"][0], p["ln3"][1], ln, M=M, C_=c, ldx=c, ldy=c)
        ff = self._new(M, 4 * c)
        hip.gemm(ln, p["ff1"]["w"], ff, M=M, N=8 * c, K=c, lda=c, ldc=4 * c, bias=p["ff1"]["b"], flags=hip.EPI_GEGLU)
        self._gemm(ff, p["ff2"], t2, hw=n, out32=t2_32, **self._resid(t1))
        return (t2, t2_32) if want32 else t2

    # ------------------------------------------------------------------ chunks 0 and 1 of the sampler's batch share their prefix
    def _share_ok(self, block, h: Act, pl: dict) -> bool:
        """Can input block 1 -- ``[ResBlock, SpatialTransformer]`` -- of a ``[x ; x ; inv_t]`` batch run its chunk-0 / chunk-1
        prefix once (``_shared_block``)?  ``pl``: the ``_hook_plan`` of its attn1 over the whole batch.  Needs the whole batch (no dead-branch elimination), the fused front and the fused
        tail with ``proj_out`` behind it (the launches whose operands can be handed over as row ranges), and a hook mode whose
        chunk-1 edit is either the identity on identical inputs (none, ``replace``, ``fft``, ``mix``) or the flow warp."""
        L = 3 if self.live_chunks is None else self.live_chunks      # chunks in the batch: 3, or 2 = [uncond ; cond] (dead-branch elimination)
        if len(block) != 2 or block[0][0] != "res" or block[1][0] != "st" or L not in (2, 3):
            return False
        if h.N % L or h.t32 is None or h.cs is None or h.hw % 128 or not self.stream32:
            return False
        P = self._packed
        pr, p = P[block[0][1]], P[block[1][1]]
        c, n, F_ = p["c"], h.hw, h.N // L
        if pr["conv2"]["cout"] != c or c % 8:
            return False
        if not (self.fuse_front and self.fuse_ffn and self.fuse_tail and self.fuse_post) or p.get("front_w") is None or \
                p.get("tail_w") is None or not p.get("tail_post"):
            return False
        if not self._front_ok((L - 1) * F_ * n, c, n) or not self._ffn_ok(F_ * n, c) or not self._ffn_ok((L - 1) * F_ * n, c):
            return False
        attn1 = block[1][2].transformer_blocks[0].attn1
        cfg = getattr(attn1, "_vface_cfg", None)
        if cfg is not None and cfg.switch_on and cfg.chunks != 3:
            return False
        if pl["staged"] or pl["v_fixed"]:
            return False
        if L == 2:
            # [uncond ; cond] alone: shared only where chunk 1 IS chunk 0 at this layer (no hook, fft, mix) -- the one case whose
            # chunk-1 bits the three-chunk shared form changes, so that dropping the recon third keeps ITS bits; replace / flow_fix
            # are bit-identical shared or not, and stay on the whole-batch launches here
            return pl["fusion"] == hip.FUSION_NONE or (pl["fusion"] == hip.FUSION_LINEAR and pl["warp_hw"] is None)
        return pl["fusion"] in (hip.FUSION_NONE, hip.FUSION_REPLACE, hip.FUSION_LINEAR)

    def _shared_block(self, block, h: Act, out, emb_all: torch.Tensor, a2_all: torch.Tensor, pl: Optional[dict] = None) -> Act:
        """Input block 1 of the sampler's ``[uncond ; cond ; recon]`` batch (ddim_w_inv.py:632-655: ``x_in = cat([x, x, inv_t])``,
        ``t_in = cat([t] * 3)``): the ResBlock and everything of the SpatialTransformer in front of attn2's row bias see the same
        numbers for chunks 0 and 1, and every kernel here is batch-invariant -- so they run on the LAST 2F samples (a contiguous
        row range of the 3F-sample buffers) and chunk 0 reads chunk 1's rows: ``_st`` on the ``[A ; C]`` row layout (``_rows``).
        ``h``: input block 0's output over all 3F samples (the skip connection needs it whole); ``pl``: the plan ``_share_ok`` was
        asked with.  Chunks 0 and 2 come out bit-identical to the whole-batch launches; chunk 1 too
        under ``flow_fix`` / ``replace`` / no hook; under ``fft`` / ``mix`` its q,k ARE chunk 0's (what the reference's
        ``combine_fft_high_low(q0, q1)`` returns for q1 = q0 up to its FFT's fp32 rounding, face_swap_utils.py:425-464) instead of
        the folded-weight projection of the same rows.  With two live chunks the batch is [uncond ; cond] alone and the rows are A
        only (``_share_ok`` admits the hook modes that leave chunk 1 equal to chunk 0 here)."""
        P = self._packed
        (_, pre_r, _), (_, pre_s, mod) = block
        L = 3 if self.live_chunks is None else self.live_chunks
        F_ = h.N // L
        Fn = F_ * h.hw
        hv = Act(h.t[Fn:] if h.t is not None else None, (L - 1) * F_, h.H, h.W, h.cs[Fn // 64:], h.t32[Fn:])
        co = P[pre_r]["conv2"]["cout"]
        r = self._res(hv, P[pre_r], emb_all[F_:], self._new_target(hv.M, co, hv.hw, need16=False))
        self._st(r, P[pre_s], mod, a2_all, out, pl, shared=L)
        return Act(out[0], h.N, h.H, h.W, out[1], out[2])

    def _halo_start(self, tail: torch.Tensor, kind: str = "exchange"):
        """``halo_exchange.start_exchange`` (``kind`` "temporal" / "gather": ``start_temporal`` / ``start_gather``) with the
        exchange's ordinal inside this forward stated first (Exchange.set_index)."""
        ex = self.halo_exchange
        ex.set_index(self._halo_k)
        self._halo_k += 1
        return getattr(ex, "start_" + kind)(tail)

    def _halo_finish(self, handle):
        """``halo_exchange.finish_exchange``, timed with HIP events when ``exchange_events`` asks for it (an exchange that issues
        its host calls itself, ``times_itself``, also times them)."""
        ex = self.halo_exchange
        return _between_events(None if ex.times_itself else self.exchange_events, lambda: ex.finish_exchange(handle))

    def _staged_edit(self, mode: str, qkv: torch.Tensor, F_: int, n: int, d: int, chunks: int):
        """The q|k edit of the staged hook modes in the projected ``qkv`` buffer ``[chunks F_ n, 3d]`` (pnp_utils.py:145-160): chunk
        k >= 1's q, k from chunk 0's and its own (``chunks`` < 3: the batch came without its last chunk(s), ``plan_fusion`` ``live``).
        temporal: a 5-tap Gaussian over the frames; adaIn: per-token AdaIN with the global unbiased std, q then k.
        On a frame shard (``halo_exchange``: this rank holds global frames [first, first + F_) of ``total``) the same kernels run on
        the same numbers, with an exchange in front of the edit -- hence the unsharded rows, bit for bit:
        temporal: chunk 0's first two and last two frames go to the other ranks, the two frames before and after the shard come
          back (``start_temporal``), and the halo form of the Gaussian reads them (``vface_temporal_gauss_halo``).
        adaIn: every (q | k, chunk) pair's row partials (``vface_adain_rows``) are gathered over the ranks in ONE exchange
          (``start_gather``: global row order), then each pair's global std and scale (``vface_adain_reduce_scale``)."""
        if mode not in ("temporal", "adaIn"):
            raise ValueError(mode)
        Fn, ex = F_ * n, self.halo_exchange
        pairs = [(col, ch) for col in (0, d) for ch in range(1, chunks)] if mode == "adaIn" else []     # q then k
        own = lambda col, ch: qkv[ch * Fn:(ch + 1) * Fn, col:col + d]
        if chunks < 2:
            return                                  # (chunk 0 alone: nothing to edit, nothing to exchange -- on every rank)
        if mode == "temporal" and ex is None:
            hip.temporal_gauss(qkv, qkv[Fn:], qkv[2 * Fn:] if chunks > 2 else None, F=F_, n=n, C_=2 * d, ld_src=3 * d, fs_src=n * 3 * d,
                               ld_dst=3 * d, fs_dst=n * 3 * d)
        elif mode == "temporal":
            lo = min(F_, 2)
            edges = self._new(4 * n, 2 * d)
            hip.copy2d(qkv, edges, rows=lo * n, cols=2 * d, ld_src=3 * d, ld_dst=2 * d)
            hip.copy2d(qkv[(F_ - lo) * n:], edges[(4 - lo) * n:], rows=lo * n, cols=2 * d, ld_src=3 * d, ld_dst=2 * d)
            halo = self._halo_finish(self._halo_start(edges.view(4, n, 2 * d), "temporal")).reshape(4 * n, 2 * d)
            hip.temporal_gauss_halo(qkv, halo if ex.first > 0 else None, halo[2 * n:] if ex.first + F_ < ex.total else None, qkv[Fn:],
                                    qkv[2 * Fn:] if chunks > 2 else None, F=F_, first=ex.first, F_total=ex.total, n=n, C_=2 * d,
                                    ld_src=3 * d, fs_src=n * 3 * d, ld_dst=3 * d, fs_dst=n * 3 * d, ld_halo=2 * d, fs_halo=n * 2 * d)
        elif ex is None:
            for col, ch in pairs:
                hip.adain_fusion(qkv[:Fn, col:col + d], own(col, ch), own(col, ch), rows=Fn, C_=d, lda=3 * d, ldb=3 * d, ldd=3 * d)
        else:
            part = torch.empty(len(pairs), Fn, 2, dtype=torch.float64, device=qkv.device)
            ws = [torch.empty(hip.adain_rows_workspace_bytes(Fn, d), dtype=torch.uint8, device=qkv.device) for _ in pairs]
            for i, (col, ch) in enumerate(pairs):
                hip.adain_rows(qkv[:Fn, col:col + d], own(col, ch), part[i], ws[i], rows=Fn, C_=d, lda=3 * d, ldb=3 * d)
            glob = self._halo_finish(self._halo_start(part, "gather"))
            for i, (col, ch) in enumerate(pairs):
                hip.adain_reduce_scale(glob[i], ws[i], own(col, ch), partial_rows=glob.shape[1], rows=Fn, C_=d, ldd=3 * d)

    def _supported(self, rule, *shape) -> bool:
        """A host-side shape rule of the library (``hip.*_supported``) per shape, asked once (a ctypes call per block per forward
        otherwise)."""
        key = (rule,) + shape
        ok = self._shape_ok.get(key)
        if ok is None:
            ok = self._shape_ok[key] = bool(rule(*shape))
        return ok

    def _ffn_ok(self, M: int, c: int) -> bool:
        return self._supported(hip.ffn_fused_supported, M, c)

    def _front_ok(self, M: int, c: int, n: int) -> bool:
        return self._supported(hip.st_front_supported, M, c, n)

    def _st(self, x: Act, p: dict, mod, a2_all: torch.Tensor, tgt, pl: Optional[dict] = None, shared: Optional[int] = None) -> Act:
        """SpatialTransformer.forward + BasicTransformerBlock._forward (attention.py:278-289, 239-243): the one walk of the layer.
        With the fp32 residual stream the block's running sum (``x`` after proj_in, after attn1 + attn2) exists in fp32
        only -- LayerNorm and the next residual add read that; its last value feeds proj_out as a 16-bit operand.
        The FRONT -- GroupNorm-apply, proj_in, LayerNorm (norm1) and attn1's projection -- is ONE launch (csrc/stfront.hip) where
        ``x`` has the fp32 carrier and its producer's column statistics, the kernel takes the width and the hook plan is not a
        staged one (those edit a full q,k,v buffer); else the separate launches and ``_block``.  Behind the fused front come the
        hooked attn1 behind its projections (``_attn1_att``; the dual-source projections of the hook's linear fusions read the
        LayerNorm output the front also writes then) and one of three tails: attn1's out-projection + norm3 + FeedForward +
        proj_out + ``x`` in one launch, the same without proj_out, or ``_attn1_out`` + ``_ffn``.
        ``pl``: the layer's ``_hook_plan`` where the caller has it already.  ``shared``: ``x`` holds the [A ; C] rows of a
        ``_shared_block`` of that many chunks, ``a2_all`` / ``tgt`` cover all of them (``_share_ok`` has said that the fused front
        and the one-launch tail apply)."""
        attn1 = mod.transformer_blocks[0].attn1
        n, c, M = x.hw, p["c"], x.M
        N = x.N if shared is None else x.N // (shared - 1) * shared
        pl = pl or self._hook_plan(attn1, N, n)
        F_ = N // (shared or pl["chunks"])
        lay = self._rows(pl, F_, n, shared)
        a, b = p["a2_slice"]
        a2vec = a2_all[:, a:b]
        s32 = self.stream32 and c % 8 == 0
        out, cs, o32 = self._new_target(M, c, n) if tgt is None else tgt
        fusion = pl["fusion"]
        if s32 and self.fuse_front and p.get("front_w") is not None and x.t32 is not None and x.cs is not None and \
                self._front_ok(M, c, n) and not pl["staged"]:
            ab = hip.groupnorm_coeffs_from_cols(x.cs, p["gn"][0], p["gn"][1], nimg=x.N, hw=n, C_=c, eps=1e-6)
            t0 = self._new(M, c, torch.float32)
            buf = self._new(lay.lead + M, 3 * c)
            ln = self._new(M, c) if fusion == hip.FUSION_LINEAR and any(r is not None for r in lay.qk[1:]) else None
            hip.st_front(x.t32, ab, p["front_w"], p["proj_in"]["b"], p["ln1"][0], p["ln1"][1], t0, buf[lay.lead:], M=M, C_=c, hw=n,
                         NQ=3 * c, rows_full=M if fusion == hip.FUSION_NONE else F_ * n, nq_lo=0 if fusion == hip.FUSION_NONE else 2 * c,
                         ln=ln)
            att = self._attn1_att(ln, buf, p, pl, F_, n, attn1.heads, lay, projected=True)
            t2 = None
            if self.fuse_tail and p.get("tail_w") is not None and n % 128 == 0 and self._ffn_ok(M, c):
                # to_out + bias + attn2's row bias + residual -> norm3 -> FeedForward -> + x in ONE launch: t1 never exists in HBM
                if self.fuse_post and p.get("tail_post") and (out is not None or o32 is not None):
                    for r0, rows, at0, s0 in lay.tail:
                        hip.attn_out_ffn_proj_fused(att[at0:], t0, a2vec[s0:], p["tail_w"], p["wo"]["b"], p["ln3"][0], p["ln3"][1],
                                                    p["ff1"]["b"], p["ff2p"], p["ff2"]["b"], p["proj_out"]["b"], x.t32,
                                                    out[r0:] if out is not None else None, o32[r0:] if o32 is not None else None,
                                                    cs[r0 // 64:] if cs is not None else None, M=rows, C_=c, rows_per_sample=n)
                    return Act(out, N, x.H, x.W, cs, o32)
                t2 = self._new(M, c)
                hip.attn_out_ffn_fused(att, t0, a2vec, p["tail_w"], p["wo"]["b"], p["ln3"][0], p["ln3"][1], p["ff1"]["b"], p["ff2p"],
                                       p["ff2"]["b"], t2, M=M, C_=c, rows_per_sample=n)
            else:
                t1 = self._new(M, c, torch.float32)
                self._attn1_out(att, p, pl, a2vec, n, None, residual32=t0, out32=t1)
                t2 = self._ffn(t1, p, n)
        else:
            g = self._gn(x, p["gn"], 1e-6, False)
            # interior16: the block's INTERIOR running sums (t0 after proj_in, t1 after attention) of the 640- / 1280-channel blocks in 16
            # bits -- 12 B per element less through HBM per block (proj_in, two LayerNorms, to_out's residual in and out, ff.net[2]'s
            # residual); the main residual stream (x_in + proj_out) stays fp32.  Emulated cost on the whole UNet: 1.2400e-3 vs 1.2236e-3
            # (tests/precision_budget.py `si_min_c`; the level-0 blocks, where it would cost 4x that, keep t1 in registers anyway)
            wide = s32 and not (self.interior16 and c >= 640)
            t0 = self._new(M, c, torch.float32 if wide else None)
            if wide:
                self._gemm(g.t, p["proj_in"], None, hw=n, out32=t0)
            else:
                self._gemm(g.t, p["proj_in"], t0, hw=n)
            t2 = self._block(t0, p, pl, attn1.heads, a2vec, N, n)
        assert not shared, "_share_ok admits only the layers whose tail launch includes proj_out"
        self._gemm(t2, p["proj_out"], out, colstats=cs, hw=n, out32=o32, **self._resid(x))
        return Act(out, x.N, x.H, x.W, cs, o32)

    # ------------------------------------------------------------------ the forward
    def embeddings(self, timesteps: torch.Tensor, context: torch.Tensor):
        """time_embed -> every ResBlock's emb_layers (openaimodel.py:874-875,264-271), and every attn2's
        ``to_out(to_v(ctx))``, as fp32 row-bias matrices."""
        P, N = self._packed, timesteps.shape[0]
        mc = self.unet.model_channels
        temb = self._new(N, mc)
        hip.timestep_embedding(timesteps.to(device=self.device, dtype=torch.int64).contiguous(), temb, mc)
        e0, emb = self._new(N, 4 * mc), self._new(N, 4 * mc)
        emb_all = self._new(N, P["emb_all"]["n"], torch.float32)
        if self.fuse_temb and hip.linear_small_supported(N, 4 * mc, mc) and hip.linear_small_supported(N, P["emb_all"]["n"], 4 * mc):
            # three launches of the few-row kernel (csrc/linear_small.hip) instead of three GEMMs + two SiLUs; each SiLU acts on its
            # layer's fp32 sum
            hip.linear_small(temb, P["time_embed.0"]["w"], P["time_embed.0"]["b"], e0, M=N, N=4 * mc, K=mc, silu=True)
            hip.linear_small(e0, P["time_embed.2"]["w"], P["time_embed.2"]["b"], emb, M=N, N=4 * mc, K=4 * mc, silu=True)
            hip.linear_small(emb, P["emb_all"]["w"], P["emb_all"].get("b"), emb_all, M=N, N=P["emb_all"]["n"], K=4 * mc)
        else:
            self._gemm(temb, P["time_embed.0"], e0)
            hip.silu(e0, e0)
            self._gemm(e0, P["time_embed.2"], emb)
            hip.silu(emb, emb)
            self._gemm(emb, P["emb_all"], emb_all, flags=hip.EPI_OUT_F32)
        return emb_all, self.context_projections(context, N)

    def context_projections(self, context: torch.Tensor, N: int) -> torch.Tensor:
        """Every attn2's ``to_out(to_v(ctx))`` as one fp32 [N, sum c] matrix.  They depend on the context only: the DDIM loop
        hands the same tensor object every step, so they are computed once per clip (the cache holds the tensor itself --
        its storage cannot be recycled under us -- and its version counter, so an in-place edit invalidates it)."""
        P = self._packed
        # (one entry per context OBJECT, a few of them: two loops interleaved through one engine -- this batch's sampling and the
        #  next batch's inversion, DDIMSampler.sample_while_inverting -- alternate two contexts and would evict a single entry at
        #  every step of the eager path)
        cache = self._a2_lru
        cached = self._a2_cache or cache.get(id(context))
        if cached is not None and cached[0] is context and cached[1] == context._version and cached[2] is P:
            return cached[3]
        ctx = context.reshape(N, -1)
        if ctx.shape[1] != self.unet.context_dim:
            raise hip.VFaceHipError(f"context must be [N, 1, {self.unet.context_dim}] (single token, SURVEY F11); "
                                    f"got {tuple(context.shape)}")
        ctx16 = self._new(N, ctx.shape[1])
        hip.cast_f32(ctx.to(device=self.device, dtype=torch.float32).contiguous(), ctx16)
        v_all = self._new(N, P["a2_v_all"]["n"])
        self._gemm(ctx16, {"w": P["a2_v_all"]["w"]}, v_all)
        a2_all = self._new(N, P["a2_v_all"]["n"], torch.float32)
        for kind, prefix, _ in self.unet.layer_table():
            if kind == "st":
                a, b = P[prefix]["a2_slice"]
                self._gemm(v_all[:, a:b], P[prefix]["a2_out"], a2_all[:, a:b], flags=hip.EPI_OUT_F32)
        cache.pop(id(context), None)
        cache[id(context)] = (context, context._version, P, a2_all)      # most recently used last; the entry keeps its tensor alive
        while len(cache) > 4:
            cache.pop(next(iter(cache)))
        return a2_all

    def forward_nhwc(self, x: Act, timesteps: torch.Tensor, context: torch.Tensor) -> torch.Tensor:
        """UNetModel.forward (openaimodel.py:860-907) on an NHWC 16-bit input (channels padded to 8k).
        Returns eps as fp32 NHWC ``[N*H*W, out_channels]``."""
        self._ensure_packed()
        self._halo_k = 0             # ordinal of the next boundary exchange of this forward (_halo_start)
        P, u = self._packed, self.unet
        emb_all, a2_all = self.embeddings(timesteps, context)
        blocks_in, mid, blocks_out = u.block_table()

        def run(block, h: Act, out) -> Act:
            for i, (kind, prefix, mod) in enumerate(block):
                last = i == len(block) - 1
                tgt = out if last else None
                if tgt is None and kind in ("res", "st"):
                    # inside a block: the 16-bit copy exists only if the next layer reads it as a matrix-core operand
                    # (a down / up convolution); a SpatialTransformer reads the fp32 carrier only
                    need16 = last or block[i + 1][0] != "st"
                    co = P[prefix]["conv2"]["cout"] if kind == "res" else P[prefix]["c"]
                    tgt = self._new_target(h.M, co, h.hw, need16=need16)
                if kind == "conv":
                    h = self._conv(h, P[prefix], tgt)
                elif kind == "res":
                    h = self._res(h, P[prefix], emb_all, tgt)
                elif kind == "st":
                    h = self._st(h, P[prefix], mod, a2_all, tgt)
                elif kind == "down":
                    h = self._conv(h, P[prefix], tgt, stride=2)
                elif kind == "up":
                    h = self._conv(h, P[prefix], tgt, upsample=True)
            return h

        # geometry pass: output shape of every input block, to size the concat buffers
        shapes = []
        H, W = x.H, x.W
        for block in blocks_in:
            for kind, prefix, _ in block:
                if kind == "down":
                    H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            shapes.append((H, W, u.block_out_channels(block)))
        nb = len(blocks_in)
        h_ch = [u.block_out_channels(mid)] + [u.block_out_channels(b) for b in blocks_out[:-1]]
        # The concat buffers.  An output block reads cat([h, skip]) twice: its ResBlock's in_layers GroupNorm and the 1x1 shortcut
        # fused into its second convolution -- BOTH from the 16-bit copy (the statistics are the producers' column sums; rounding the
        # GroupNorm's input costs nothing measurable: tests/precision_budget.py `gn_in16`, 1.2236e-3 vs 1.2273e-3 whole-UNet).  So the
        # fp32 carrier exists for the SKIP columns only -- there it is the input path's residual stream, read by the next input
        # block -- and the `h` columns (the previous output block's result, consumed by nothing else) are written once, 16-bit:
        # 4 B per element less from their producers and 2 B less into every concat GroupNorm (6.5 GB per 96-sample step).
        cats, cats_cs, cats32 = [], [], []
        for j in range(nb):  # output block j consumes cat([h_{j}, skip_{nb-1-j}])
            sh, sw, sc = shapes[nb - 1 - j]
            rows = x.N * sh * sw
            cats.append(self._new(rows, h_ch[j] + sc))
            cats_cs.append(self._new_cs(rows, h_ch[j] + sc, sh * sw))
            wide = self.concat32                 # (VFACE_CONCAT32=1, A/B: the carrier over ALL columns, read by the concat GroupNorm)
            cats32.append(self._new(rows, (h_ch[j] + sc) if wide else sc, torch.float32) if (self.stream32 and sc % 8 == 0) else None)

        def part(j, a, b):  # columns [a, b) of concat buffer j, of its statistics and (skip columns only) of its fp32 carrier
            cs, b32, hc = cats_cs[j], cats32[j], (0 if self.concat32 else h_ch[j])
            return (cats[j][:, a:b], (cs[:, a:b] if cs is not None else None),
                    (b32[:, a - hc:b - hc] if (b32 is not None and a >= hc) else None))

        h = x
        for i, block in enumerate(blocks_in):
            j = nb - 1 - i
            if i == 1 and self.share_prefix and block[-1][0] == "st":
                pl = self._hook_plan(block[-1][2].transformer_blocks[0].attn1, h.N, h.hw)
                if self._share_ok(block, h, pl):
                    h = self._shared_block(block, h, part(j, h_ch[j], cats[j].shape[1]), emb_all, a2_all, pl)
                    continue
            h = run(block, h, part(j, h_ch[j], cats[j].shape[1]))
        h = run(mid, h, part(0, 0, h_ch[0]))
        for j, block in enumerate(blocks_out):
            sh, sw, _ = shapes[nb - 1 - j]
            inp = Act(cats[j], x.N, sh, sw, cats_cs[j], cats32[j] if self.concat32 else None)
            tgt = part(j + 1, 0, h_ch[j + 1]) if j + 1 < nb else None
            h = run(block, inp, tgt)
        oc = P["out.conv"]
        if self.fuse_out and h.cs is not None and oc["cinp"] % 64 == 0 and oc["cinp"] <= 640 and oc["cout"] in (3, 4) and h.C == oc["cinp"]:
            # out = normalization -> SiLU -> conv3x3 (openaimodel.py:712-716) in ONE launch (csrc/outconv.hip)
            ab = hip.groupnorm_coeffs_from_cols(h.cs, P["out.gn"][0], P["out.gn"][1], nimg=h.N, hw=h.hw, C_=h.C, eps=1e-5)
            eps = self._new(h.M, oc["cout"], torch.float32)
            hip.gn_silu_conv3x3_small(h.src, ab, oc["w"], oc["b"], eps, nimg=h.N, H=h.H, W=h.W, cin=oc["cinp"], cout=oc["cout"])
            return eps
        h = self._gn(h, P["out.gn"], 1e-5, True)
        return self._conv(h, P["out.conv"], None, out_f32=True).t


    def forward(self, x: torch.Tensor, timesteps: torch.Tensor, context: torch.Tensor) -> torch.Tensor:
        """NCHW fp32 in, NCHW fp32 out -- the signature of the reference's ``UNetModel.forward``."""
        if not x.is_cuda:
            raise hip.VFaceHipError("UNetModel.forward needs CUDA tensors: the VFace path has no CPU fallback")
        N, C, H, W = x.shape
        cpad = (C + 7) // 8 * 8
        xin = self._new(N * H * W, cpad)
        hip.nchw_to_nhwc(x.float().contiguous(), xin, N=N, C_=C, hw=H * W, cpad=cpad)
        eps = self.forward_nhwc(Act(xin, N, H, W), timesteps, context)
        out = torch.empty(N, eps.shape[1], H, W, dtype=torch.float32, device=x.device)
        hip.nhwc_to_nchw_f32(eps, out, N=N, C_=eps.shape[1], hw=H * W, ldx=eps.stride(0))
        return out
