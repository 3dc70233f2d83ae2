"""Kernel sequencing for the first-stage KL-VAE: ``AutoencoderKL.encode / decode``
(``REFace/ldm/models/autoencoder.py:323-333``) over ``Encoder`` / ``Decoder``
(``ldm/modules/diffusionmodules/model.py:368-568``) with the kernels of the UNet path:

* every 3x3 convolution is ``vface_conv3x3`` (``Downsample`` :72-77 = trailing zero padding + stride 2, ``Upsample`` :55-58 =
  the fused nearest x2), with the producer-side column statistics feeding the next GroupNorm (eps 1e-6, swish);
* ``AttnBlock`` (:176-202) has ONE head of all 512 channels, beyond what the streaming attention kernel keeps in LDS, and
  runs once per frame, not per step: scores = ``vface_gemm`` (fp32 out) per image, ``vface_softmax_rows``, then
  ``P @ V`` as a GEMM against V^T, which is produced directly as ``Wv @ h^T`` (the value bias moves to the output column
  bias: the rows of P sum to one);
* ``quant_conv`` (1x1 after ``conv_out``, no nonlinearity between) is folded into ``conv_out`` in fp64; ``post_quant_conv``
  keeps its own tiny GEMM (its bias does not commute with ``conv_in``'s zero padding); ``1/scale_factor`` is not applied
  here (``decode_first_stage`` does that, ddpm.py:1284).

Activations are NHWC 16-bit ``[F*H*W, C]`` as in the UNet engine; frames are processed in chunks so every tensor view
stays below the 4 GiB the buffer descriptors address (``frames_per_chunk``), and a size the mid attention's launches would refuse
is refused before the first of them (``check_attention_tokens``).  No CPU path."""
from __future__ import annotations

from typing import Optional

import torch

from . import hip, packing
from .engine import Act, _phase_form_pays
from .ldm.modules.distributions.distributions import DiagonalGaussianDistribution


def check_attention_tokens(h: int, w: int, what: str):
    """The mid ``AttnBlock`` at a latent of ``h x w``: its ``P V^T`` GEMM has K = lda = n = h w and its probabilities are rows of
    ``vface_softmax_rows``, so n must be a multiple of ``hip.GEMM_K_MULTIPLE`` and at most ``hip.SOFTMAX_MAX_COLS``.  Raised before
    anything is allocated or launched."""
    n = h * w
    if n % hip.GEMM_K_MULTIPLE or n > hip.SOFTMAX_MAX_COLS:
        raise hip.VFaceHipError(f"{what}: the latent is {h} x {w}, n = {n} attention tokens per frame; the mid AttnBlock's P V^T GEMM "
                                f"(K = lda = n) and its row softmax need n to be a multiple of {hip.GEMM_K_MULTIPLE} and at most "
                                f"{hip.SOFTMAX_MAX_COLS}")


def frames_per_chunk(H: int, W: int, channels, dtype: torch.dtype, max_frames: int = 8) -> int:
    """How many frames of ``H x W`` pixels go through the network at once: the most, up to ``max_frames``, at which every
    activation ``[frames * (H >> l) * (W >> l), channels[l]]`` of ``dtype`` stays below ``hip.OPERAND_BYTES_LIMIT``, the extent
    csrc/dispatch.cpp allows one operand view.  ``channels``: the widest row of each level, level 0 (full resolution) first; an
    int is level 0 alone.  Depends on nothing but its arguments (frames are independent, so the chunk does not change a bit)."""
    widths = [channels] if isinstance(channels, int) else list(channels)
    per_frame = max((H >> l) * (W >> l) * c for l, c in enumerate(widths)) * torch.empty(0, dtype=dtype).element_size()
    n = min(max_frames, (hip.OPERAND_BYTES_LIMIT - 1) // per_frame)
    if n < 1:
        raise hip.VFaceHipError(f"one {H} x {W} frame has an activation of {per_frame} bytes; an operand view must stay below "
                                f"{hip.OPERAND_BYTES_LIMIT}")
    return n


def level_widths(net) -> list:
    """The widest activation row of each resolution level of an ``Encoder`` / ``Decoder`` (the mid attention's q | k buffer counts
    at the deepest one), for ``frames_per_chunk``."""
    levels = net.down if hasattr(net, "down") else net.up
    out = [max(max(b.in_channels, b.out_channels) for b in L.block) for L in levels]
    out[-1] = max(out[-1], 2 * net.mid.attn_1.in_channels)
    return out


class Packer:
    """A state dict with the reference's key names -> the operands one stage's kernels read, on ``device``: 16-bit packed weights,
    fp32 biases and GroupNorm parameters.  ``pack_state_dict`` walks the whole network with it; the stage tests pack one block."""

    def __init__(self, sd: dict, dtype: torch.dtype, device):
        self.sd = {k: v.detach().double().cpu() for k, v in sd.items()}
        self.dtype, self.device = dtype, device

    def w16(self, t):
        return t.detach().to(device=self.device, dtype=self.dtype).contiguous()

    def f32(self, t):
        return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def conv3(self, pre, w=None, b=None, cout_pad=None):
        w = self.sd[pre + ".weight"] if w is None else w
        b = self.sd[pre + ".bias"] if b is None else b
        cout, cin = w.shape[0], w.shape[1]
        if cout_pad is not None and cout_pad > cout:   # GEMM N must be a multiple of 4: zero output channels
            w = torch.cat([w, torch.zeros(cout_pad - cout, *w.shape[1:], dtype=w.dtype)], 0)
            b = torch.cat([b, torch.zeros(cout_pad - cout, dtype=b.dtype)])
        return {"w": self.w16(packing.pack_conv3x3(w.float())), "b": self.f32(b), "cin": cin,
                "cinp": (cin + 7) // 8 * 8, "cout": w.shape[0], "cout_true": cout}

    def upsample(self, pre):
        d = self.conv3(pre)
        d["phases"] = self.w16(packing.pack_upsample_phases(self.sd[pre + ".weight"].float()))
        return d

    def lin(self, pre, rows=slice(None)):
        w = self.sd[pre + ".weight"]
        return {"w": self.w16(w.reshape(w.shape[0], w.shape[1])[rows]), "b": self.f32(self.sd[pre + ".bias"][rows])}

    def gn(self, pre):
        return (self.f32(self.sd[pre + ".weight"]), self.f32(self.sd[pre + ".bias"]))

    def res(self, pre):
        d = {"norm1": self.gn(pre + ".norm1"), "conv1": self.conv3(pre + ".conv1"), "norm2": self.gn(pre + ".norm2"),
             "conv2": self.conv3(pre + ".conv2")}
        if pre + ".nin_shortcut.weight" in self.sd:
            d["nin"] = self.lin(pre + ".nin_shortcut")
        return d

    def attn(self, pre):
        sd = self.sd
        wq, wk = sd[pre + ".q.weight"], sd[pre + ".k.weight"]
        c = wq.shape[0]
        return {"norm": self.gn(pre + ".norm"), "c": c,
                "qk": {"w": self.w16(torch.cat([wq.reshape(c, c), wk.reshape(c, c)], 0)),
                       "b": self.f32(torch.cat([sd[pre + ".q.bias"], sd[pre + ".k.bias"]]))},
                "wv": self.w16(sd[pre + ".v.weight"].reshape(c, c)), "bv": self.f32(sd[pre + ".v.bias"]),
                "proj": self.lin(pre + ".proj_out")}

    def folded_conv_out(self, pre="encoder.conv_out", quant="quant_conv"):
        """quant_conv o conv_out, folded in fp64 (both linear, nothing between them: autoencoder.py:324-325)."""
        sd = self.sd
        wq = sd[quant + ".weight"].reshape(sd[quant + ".weight"].shape[0], -1)
        wc, bc = sd[pre + ".weight"], sd[pre + ".bias"]
        return self.conv3("", w=torch.einsum("om,mikl->oikl", wq, wc), b=wq @ bc + sd[quant + ".bias"])

    def post_quant(self, zc, ed, pre="post_quant_conv"):
        """post_quant_conv as an 8 x 8 GEMM (zero rows and columns past zc, ed).  It stays a launch of its own: its bias does not
        commute with conv_in's zero padding (a border pixel's missing taps would still receive it)."""
        wpq = torch.zeros(8, 8, dtype=torch.float64); wpq[:zc, :ed] = self.sd[pre + ".weight"].reshape(zc, ed)
        bpq = torch.zeros(8, dtype=torch.float64); bpq[:zc] = self.sd[pre + ".bias"]
        return {"w": self.w16(wpq), "b": self.f32(bpq)}


def pack_state_dict(sd: dict, *, num_resolutions: int, num_res_blocks: int, z_channels: int, embed_dim: int, dtype: torch.dtype,
                    device) -> dict:
    """``AutoencoderKL``'s whole state dict through ``Packer``, under the stage names ``VAEEngine`` sequences.
    (tests/vae_model.py calls it with the CPU as device.)"""
    pk = Packer(sd, dtype, device)
    conv3, res, attn, gn = pk.conv3, pk.res, pk.attn, pk.gn
    P = {}
    P["enc.conv_in"] = conv3("encoder.conv_in")
    for lvl in range(num_resolutions):
        for blk in range(num_res_blocks):
            P[f"enc.down.{lvl}.{blk}"] = res(f"encoder.down.{lvl}.block.{blk}")
        if lvl != num_resolutions - 1:
            P[f"enc.down.{lvl}.ds"] = conv3(f"encoder.down.{lvl}.downsample.conv")
    P["enc.mid1"], P["enc.attn"], P["enc.mid2"] = res("encoder.mid.block_1"), attn("encoder.mid.attn_1"), res("encoder.mid.block_2")
    P["enc.norm_out"] = gn("encoder.norm_out")
    P["enc.conv_out"] = pk.folded_conv_out()
    P["dec.post_quant"] = pk.post_quant(z_channels, embed_dim)
    P["dec.conv_in"] = conv3("decoder.conv_in")
    P["dec.mid1"], P["dec.attn"], P["dec.mid2"] = res("decoder.mid.block_1"), attn("decoder.mid.attn_1"), res("decoder.mid.block_2")
    for lvl in range(num_resolutions):
        for blk in range(num_res_blocks + 1):
            P[f"dec.up.{lvl}.{blk}"] = res(f"decoder.up.{lvl}.block.{blk}")
        if lvl != 0:
            P[f"dec.up.{lvl}.us"] = pk.upsample(f"decoder.up.{lvl}.upsample.conv")
    P["dec.norm_out"] = gn("decoder.norm_out")
    P["dec.conv_out"] = conv3("decoder.conv_out", cout_pad=4)
    return P


class VAEEngine:
    def __init__(self, vae, dtype: torch.dtype = torch.float16, max_frames: int = 8):
        self.vae = vae
        self.dtype = dtype
        self.max_frames = max_frames
        self._packed = None
        hip.load()

    @property
    def device(self):
        return next(self.vae.parameters()).device

    # ------------------------------------------------------------------ weights
    def pack(self):
        if not next(self.vae.parameters()).is_cuda:
            raise hip.VFaceHipError("AutoencoderKL parameters are not on the GPU: the VFace path has no CPU fallback")
        enc = self.vae.encoder
        self._packed = pack_state_dict(self.vae.state_dict(), num_resolutions=enc.num_resolutions, num_res_blocks=enc.num_res_blocks,
                                       z_channels=self.vae.decoder.z_channels, embed_dim=self.vae.embed_dim, dtype=self.dtype,
                                       device=self.device)

    def _ensure_packed(self):
        if self._packed is None:
            self.pack()

    # ------------------------------------------------------------------ building blocks
    def _new(self, rows, cols, dtype=None):
        return torch.empty(rows, cols, dtype=dtype or self.dtype, device=self.device)

    def _cs(self, rows, cols, hw):
        if hw % 64 or cols % 8:
            return None
        return torch.empty(rows // 64, cols, 2, dtype=torch.float32, device=self.device)

    def _gn(self, x: Act, gn, silu: bool) -> Act:
        if x.cs is not None:
            st = hip.groupnorm_stats_from_cols(x.cs, nimg=x.N, hw=x.hw, C_=x.C, eps=1e-6)
        else:
            st = hip.groupnorm_stats(x.t, nimg=x.N, hw=x.hw, C_=x.C, ldx=x.ld, eps=1e-6)
        y = self._new(x.M, x.C)
        hip.groupnorm_apply(x.t, st, gn[0], gn[1], y, nimg=x.N, hw=x.hw, C_=x.C, ldx=x.ld, ldy=x.C, silu=silu)
        return Act(y, x.N, x.H, x.W)

    def _conv(self, x: Act, w: dict, stride=1, upsample=False, trailing_pad=False, residual=None, out_f32=False) -> Act:
        VH, VW = (2 * x.H, 2 * x.W) if upsample else (x.H, x.W)
        OH, OW = (VH - 1) // stride + 1, (VW - 1) // stride + 1
        rows = x.N * OH * OW
        out = self._new(rows, w["cout"], torch.float32 if out_f32 else None)
        cs = None if out_f32 else self._cs(rows, w["cout"], OH * OW)
        assert x.C == w["cinp"], (x.C, w["cinp"])
        flags = (hip.EPI_OUT_F32 if out_f32 else 0) | (hip.CONV_PAD_TRAILING if trailing_pad else 0)
        if upsample and "phases" in w and residual is None and not out_f32 and (x.H * x.W) % 64 == 0 \
                and _phase_form_pays(x.H * x.W, w["cout"]):
            # Upsample (model.py:55-58) as four parity-phase 2x2 convs with pre-summed taps: 4/9 of the multiply-adds
            hip.upsample2x_conv3x3(x.t, w["phases"], out, nimg=x.N, H=x.H, W=x.W, cin=w["cinp"], cout=w["cout"], ldx=x.ld,
                                   ldy=out.stride(0), bias=w["b"], colstats=cs)
            return Act(out, x.N, OH, OW, cs)
        hip.conv3x3(x.t, w["w"], out, nimg=x.N, H=x.H, W=x.W, cin=w["cinp"], cout=w["cout"], ldx=x.ld, ldy=out.stride(0),
                    stride=stride, upsample=upsample, bias=w["b"], residual=residual,
                    ldr=residual.stride(0) if residual is not None else 0, flags=flags, colstats=cs)
        return Act(out, x.N, OH, OW, cs)

    def _res(self, x: Act, p: dict) -> Act:
        """ResnetBlock.forward (model.py:118-141), temb None."""
        h = self._conv(self._gn(x, p["norm1"], True), p["conv1"])
        h = self._gn(h, p["norm2"], True)
        if "nin" in p:
            skip = self._new(x.M, p["conv2"]["cout"])
            hip.gemm(x.t, p["nin"]["w"], skip, M=x.M, N=skip.shape[1], K=x.C, lda=x.ld, ldc=skip.shape[1], bias=p["nin"]["b"],
                     rows_per_sample=x.hw)
        else:
            skip = x.t
        return self._conv(h, p["conv2"], residual=skip)

    def _attn(self, x: Act, p: dict) -> Act:
        """AttnBlock.forward (model.py:176-202)."""
        c, n = p["c"], x.hw
        g = self._gn(x, p["norm"], False)
        qk = self._new(x.M, 2 * c)
        hip.gemm(g.t, p["qk"]["w"], qk, M=x.M, N=2 * c, K=c, lda=c, ldc=2 * c, bias=p["qk"]["b"])
        att = self._new(x.M, c)
        scores = torch.empty(n, n, dtype=torch.float32, device=self.device)
        prob = self._new(n, n)
        vt = self._new(c, n)
        for b in range(x.N):
            rows = slice(b * n, (b + 1) * n)
            hip.gemm(qk[rows], qk[rows, c:], scores, M=n, N=n, K=c, lda=2 * c, ldw=2 * c, ldc=n, flags=hip.EPI_OUT_F32)
            hip.softmax_rows(scores, prob, M=n, N=n, scale=float(int(c) ** -0.5))
            hip.gemm(p["wv"], g.t[rows], vt, M=c, N=n, K=c, lda=c, ldw=c, ldc=n)              # V^T = Wv h^T
            hip.gemm(prob, vt, att[rows], M=n, N=c, K=n, lda=n, ldw=n, ldc=c, bias=p["bv"])   # P V + bv (rows of P sum to 1)
        out = self._new(x.M, c)
        cs = self._cs(x.M, c, n)
        hip.gemm(att, p["proj"]["w"], out, M=x.M, N=c, K=c, lda=c, ldc=c, bias=p["proj"]["b"], residual=x.t, ldr=x.ld,
                 colstats=cs, rows_per_sample=n)
        return Act(out, x.N, x.H, x.W, cs)

    # ------------------------------------------------------------------ encode / decode
    def _chunks(self, F, H, W, net):
        """Frame ranges of one pass each, for ``H x W`` pixels at level 0 of ``net``: ``frames_per_chunk`` frames at a time."""
        per = frames_per_chunk(H, W, level_widths(net), self.dtype, self.max_frames)
        return [(f0, min(F, f0 + per)) for f0 in range(0, F, per)]

    def _input(self, x: torch.Tensor) -> Act:
        """``[n, C, H, W]`` of any float type and stride -> the 16-bit NHWC activation of 8 stored channels."""
        n, C, H, W = x.shape
        xin = self._new(n * H * W, 8)
        hip.nchw_to_nhwc(x.float().contiguous(), xin, N=n, C_=C, hw=H * W, cpad=8)
        return Act(xin, n, H, W)

    def _post_quant_conv_in(self, zin: Act, P: dict) -> Act:
        """post_quant_conv (a launch of its own, see ``Packer.post_quant``) and the decoder's conv_in."""
        z8 = self._new(zin.M, 8)
        hip.gemm(zin.t, P["dec.post_quant"]["w"], z8, M=zin.M, N=8, K=8, lda=8, ldc=8, bias=P["dec.post_quant"]["b"])
        return self._conv(Act(z8, zin.N, zin.H, zin.W), P["dec.conv_in"])

    def _norm_out_conv(self, a: Act, gn, conv: dict) -> Act:
        """norm_out, swish and the last convolution of either network, fp32 out (the encoder's carries quant_conv folded in)."""
        return self._conv(self._gn(a, gn, True), conv, out_f32=True)

    def encode(self, x: torch.Tensor, taps: Optional[dict] = None) -> DiagonalGaussianDistribution:
        """``taps`` (tests): receives every stage's output ``Act`` under its packed-weight key; one chunk only."""
        if not x.is_cuda:
            raise hip.VFaceHipError("input is not on the GPU: the VFace path has no CPU fallback")
        enc = self.vae.encoder
        F, C, H, W = x.shape
        if C != enc.in_channels or H % (1 << (enc.num_resolutions - 1)) or W % (1 << (enc.num_resolutions - 1)):
            raise hip.VFaceHipError(f"encode expects [F, {enc.in_channels}, H, W] with H, W multiples of "
                                    f"{1 << (enc.num_resolutions - 1)}; got {tuple(x.shape)}")
        zc = enc.z_channels
        h, w = H >> (enc.num_resolutions - 1), W >> (enc.num_resolutions - 1)
        check_attention_tokens(h, w, f"encode of {tuple(x.shape)}")
        chunks = self._chunks(F, H, W, enc)
        self._ensure_packed()
        P = self._packed
        moments = torch.empty(F * h * w, P["enc.conv_out"]["cout"], dtype=torch.float32, device=self.device)
        assert taps is None or len(chunks) == 1
        tap = (lambda k, a: a) if taps is None else (lambda k, a: taps.setdefault(k, a))
        for f0, f1 in chunks:
            a = tap("enc.conv_in", self._conv(self._input(x[f0:f1]), P["enc.conv_in"]))
            for lvl in range(enc.num_resolutions):
                for blk in range(enc.num_res_blocks):
                    a = tap(f"enc.down.{lvl}.{blk}", self._res(a, P[f"enc.down.{lvl}.{blk}"]))
                if lvl != enc.num_resolutions - 1:
                    a = tap(f"enc.down.{lvl}.ds", self._conv(a, P[f"enc.down.{lvl}.ds"], stride=2, trailing_pad=True))
            a = tap("enc.mid1", self._res(a, P["enc.mid1"]))
            a = tap("enc.attn", self._attn(a, P["enc.attn"]))
            a = tap("enc.mid2", self._res(a, P["enc.mid2"]))
            a = self._norm_out_conv(a, P["enc.norm_out"], P["enc.conv_out"])
            moments[f0 * h * w:f1 * h * w] = a.t
        return DiagonalGaussianDistribution(moments, F, h, w, zc)

    def decode(self, z: torch.Tensor, taps: Optional[dict] = None) -> torch.Tensor:
        if not z.is_cuda:
            raise hip.VFaceHipError("latents are not on the GPU: the VFace path has no CPU fallback")
        dec = self.vae.decoder
        F, C, h, w = z.shape
        if C != self.vae.embed_dim:
            raise hip.VFaceHipError(f"decode expects [F, {self.vae.embed_dim}, h, w]; got {tuple(z.shape)}")
        up = 1 << (dec.num_resolutions - 1)
        check_attention_tokens(h, w, f"decode of {tuple(z.shape)}")
        chunks = self._chunks(F, h * up, w * up, dec)
        self._ensure_packed()
        P = self._packed
        out = torch.empty(F, dec.out_ch, h * up, w * up, dtype=torch.float32, device=self.device)
        assert taps is None or len(chunks) == 1
        tap = (lambda k, a: a) if taps is None else (lambda k, a: taps.setdefault(k, a))
        for f0, f1 in chunks:
            a = tap("dec.conv_in", self._post_quant_conv_in(self._input(z[f0:f1]), P))
            a = tap("dec.mid1", self._res(a, P["dec.mid1"]))
            a = tap("dec.attn", self._attn(a, P["dec.attn"]))
            a = tap("dec.mid2", self._res(a, P["dec.mid2"]))
            for lvl in reversed(range(dec.num_resolutions)):
                for blk in range(dec.num_res_blocks + 1):
                    a = tap(f"dec.up.{lvl}.{blk}", self._res(a, P[f"dec.up.{lvl}.{blk}"]))
                if lvl != 0:
                    a = tap(f"dec.up.{lvl}.us", self._conv(a, P[f"dec.up.{lvl}.us"], upsample=True))
            a = self._norm_out_conv(a, P["dec.norm_out"], P["dec.conv_out"])
            hip.nhwc_to_nchw_f32(a.t, out[f0:f1], N=f1 - f0, C_=dec.out_ch, hw=a.H * a.W, ldx=a.t.stride(0))
        return out
