"""The identity network on the HIP kernels: ``IDLoss.extract_feats`` (``REFace/ldm/models/diffusion/ddpm.py:91-124``) -- a pooling
and crop chain in front of ArcFace ``Backbone(112, 50, 'ir_se')`` (``REFace/src/Face_models/encoders/{model_irse,helpers}.py``) --
without leaving the GPU.  ``ArcFaceEngine`` runs it for a batch of images on ``convnet.ConvNetEngine`` as ``ParseEngine`` does:

    rows      vface_id_prep                    [B 112 112][8] 16-bit   un_norm_clip, (x - .5) / .5, pool 256, crop, pool 112
    stem      vface_conv3x3 (Cin 8, bn folded) -> vface_prelu: y and z = the first unit's leading BatchNorm of the unrounded y
    24 units  vface_conv3x3 (z, stride 1) -> vface_prelu (in place) -> vface_conv3x3 (stride s, trailing bn folded)
              -> vface_channel_stats -> vface_pooled_linear (fc1, ReLU) -> vface_pooled_linear (fc2, sigmoid)
              -> vface_se_gate_add: y = res * gate + shortcut, z = the next unit's leading BatchNorm of the unrounded sum.
              The shortcut is the unit's input subsampled (MaxPool2d(1, s)) or vface_im2col + vface_gemm (1x1 stride s, bn folded)
    head      vface_gemm M = B, K = 25088, fp32 out: BatchNorm2d(512), Flatten, Linear and BatchNorm1d as one matrix
    norm      vface_l2norm_rows                -> fp32 [B, 512]

What is folded, on the host in fp64: the stem's BatchNorm, every unit's trailing BatchNorm and the shortcut's into the convolution in
front of each; ``output_layer``'s BatchNorm2d into the columns of its Linear (exact: nothing is padded there), those columns permuted
from the reference's NCHW flatten ``c 49 + p`` to the token rows' ``p 512 + c``, and its BatchNorm1d into the rows and the bias.  A
unit's LEADING BatchNorm sits in front of a zero-padded convolution: folded, the padding would carry its shift, so it stays a
per-channel ``(a, b)`` pair applied by the kernel that writes the unit's input.  Dropout in eval is the identity.

No launch splits K by batch size and no kernel uses atomics, so an image's features do not depend on the images sharing its batch.
No CPU fallback: without the HIP library every call raises.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import hip
from .convnet import ConvNetEngine

BN_EPS = 1e-5
# (in_channel, depth, stride) of the 24 units of IR-50: get_blocks(50) of helpers.py:29-36
UNITS = tuple((cin, d, 2 if i == 0 else 1)
              for n, c0, d in ((3, 64, 64), (4, 64, 128), (14, 128, 256), (3, 256, 512))
              for i, cin in enumerate([c0] + [d] * (n - 1)))
FEAT, FINAL_HW, SE_REDUCTION = 512, 7, 16
SHIPPED = "Backbone(input_size=112, num_layers=50, mode='ir_se'), single scale"


def check_config(input_size: int = 112, num_layers: int = 50, mode: str = "ir_se", multi_scale: bool = False):
    if input_size != 112 or num_layers != 50 or mode != "ir_se" or multi_scale:
        raise NotImplementedError(f"the identity network is built for {SHIPPED} only; got input_size={input_size}, "
                                  f"num_layers={num_layers}, mode={mode!r}, multi_scale={multi_scale}")


def bn_pair(sd, name: str, eps: float = BN_EPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval-mode BatchNorm ``name`` as ``y = a x + b``, in the dtype of ``sd``; an absent affine ``weight`` / ``bias`` is 1 / 0."""
    mean, var = sd[name + ".running_mean"], sd[name + ".running_var"]
    a = 1.0 / torch.sqrt(var + eps)
    if name + ".weight" in sd:
        a = a * sd[name + ".weight"]
    b = -mean * a
    if name + ".bias" in sd:
        b = b + sd[name + ".bias"]
    return a, b


def fold_head(sd, prefix: str = "output_layer", hw: int = FINAL_HW * FINAL_HW) -> Tuple[torch.Tensor, torch.Tensor]:
    """``BatchNorm1d(Linear(Flatten(BatchNorm2d(x))))`` as ``W' t + b'`` on the token rows ``t[p C + c] = x[c][p]``, in the dtype of
    ``sd``: BatchNorm2d into the columns, the columns from ``c hw + p`` to ``p C + c``, BatchNorm1d into the rows and the bias."""
    w, b = sd[f"{prefix}.3.weight"], sd[f"{prefix}.3.bias"]
    N, K = w.shape
    C_ = K // hw
    a2, b2 = bn_pair(sd, f"{prefix}.0")
    w3 = w.reshape(N, C_, hw)
    b = b + (w3 * b2.reshape(1, C_, 1)).sum((1, 2))
    w3 = (w3 * a2.reshape(1, C_, 1)).permute(0, 2, 1).reshape(N, K)
    a1, b1 = bn_pair(sd, f"{prefix}.4")
    return w3 * a1.reshape(N, 1), b * a1 + b1


class ArcFaceEngine(ConvNetEngine):
    """Executes the IR-SE50 ``Backbone`` on device buffers.  ``sd``: its state dict (any float dtype, any device), or None for an
    engine that holds only the units added with ``add_unit``."""
    split_k = False      # an image's features must not depend on its batch (see ConvNetEngine.split_k)

    def __init__(self, sd: Optional[Dict[str, torch.Tensor]], dtype: torch.dtype = torch.float16, device="cuda:0"):
        super().__init__(dtype, device)
        self.lead: Dict[str, tuple] = {}       # unit -> (a, b) of its leading BatchNorm, fp32 on the device
        self.slope: Dict[str, torch.Tensor] = {}
        self.units = []
        if sd is None:
            return
        sd = {k: v.detach().double().cpu() for k, v in sd.items() if torch.is_floating_point(v)}      # everything is folded in fp64
        self.add_conv(sd, "input_layer.0", "input_layer.1", cin_pad=8)
        self.slope["input_layer"] = self._vec(sd["input_layer.2.weight"])
        for i, (cin, depth, stride) in enumerate(UNITS):
            self.add_unit(sd, f"body.{i}", cin, depth, stride)
        w, b = fold_head(sd)
        if tuple(w.shape) != (FEAT, FEAT * FINAL_HW * FINAL_HW):
            raise NotImplementedError(f"the identity network is built for {SHIPPED} only; got an output layer {tuple(w.shape)}")
        self.head_w, self.head_b = w.float().to(self.dtype).to(self.dev), self._vec(b)

    def _vec(self, v):
        return v.float().contiguous().to(self.dev)

    def add_unit(self, sd, u: str, cin: int, depth: int, stride: int):
        """One ``bottleneck_IR_SE``: ``sd`` holds its tensors under ``u + '.'`` in fp64."""
        r = f"{u}.res_layer"
        a, b = bn_pair(sd, f"{r}.0")
        self.lead[u] = (self._vec(a), self._vec(b))
        self.add_conv(sd, f"{r}.1")
        self.slope[u] = self._vec(sd[f"{r}.2.weight"])
        self.add_conv(sd, f"{r}.3", f"{r}.4")
        self.add_conv(sd, f"{r}.5.fc1", pooled=True)
        self.add_conv(sd, f"{r}.5.fc2", pooled=True)
        if f"{u}.shortcut_layer.0.weight" in sd:
            self.add_conv(sd, f"{u}.shortcut_layer.0", f"{u}.shortcut_layer.1")
        elif cin != depth:
            raise hip.VFaceHipError(f"{u}: {cin} -> {depth} channels needs a convolution shortcut")
        self.units.append((u, cin, depth, stride))

    # ---- building blocks -------------------------------------------------------------------------------------------------
    def lead_in(self, u: str, x: torch.Tensor, *, M: int, C_: int) -> torch.Tensor:
        """The leading BatchNorm of unit ``u`` on a stored tensor (inside the network the kernel that writes ``x`` writes this
        too, from the unrounded value): a PReLU of slope 1 with the ``z`` output."""
        z = self._buf(M, C_)
        one = torch.ones(C_, dtype=torch.float32, device=self.dev)
        hip.prelu(x, one, self._buf(M, C_), M=M, C_=C_, z=z, za=self.lead[u][0], zb=self.lead[u][1])
        return z

    def unit(self, u: str, x: torch.Tensor, z: torch.Tensor, *, nimg: int, H: int, W: int, cin: int, depth: int, stride: int,
             nxt: Optional[str] = None):
        """``x``: the unit's input [nimg H W, cin], ``z``: its leading BatchNorm of it -> (y, z of unit ``nxt`` | None, OH, OW)."""
        r = f"{u}.res_layer"
        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        M = nimg * OH * OW
        t = self._buf(nimg * H * W, depth)
        self.conv3(f"{r}.1", z, t, nimg=nimg, H=H, W=W, ldx=z.stride(0))
        hip.prelu(t, self.slope[u], t, M=nimg * H * W, C_=depth)
        res = self._buf(M, depth)
        self.conv3(f"{r}.3", t, res, nimg=nimg, H=H, W=W, ldx=depth, stride=stride)
        p1, p2 = self.P[f"{r}.5.fc1"], self.P[f"{r}.5.fc2"]
        means = hip.channel_stats(res, nimg=nimg, hw=OH * OW, C_=depth)
        h = torch.empty(nimg, p1["cout"], dtype=torch.float32, device=self.dev)
        hip.pooled_linear(means, p1["w"], p1["b"], h, nimg=nimg, N=p1["cout"], K=depth, lda=2 * depth, sa=2, act=hip.ACT_RELU)
        g = torch.empty(nimg, depth, dtype=torch.float32, device=self.dev)
        hip.pooled_linear(h, p2["w"], p2["b"], g, nimg=nimg, N=depth, K=p2["cin"], lda=h.stride(0), sa=1, act=hip.ACT_SIGMOID)
        y = self._buf(M, depth)
        zn = self._buf(M, depth) if nxt is not None else None
        za, zb = self.lead[nxt] if nxt is not None else (None, None)
        if f"{u}.shortcut_layer.0" in self.P:      # bn(conv1x1 stride s (x)), through the window matrix as the parser's downsample.0
            sc = self._buf(M, depth)
            self.window(f"{u}.shortcut_layer.0", x, sc, nimg=nimg, H=H, W=W, C_=cin, ldx=x.stride(0), stride=stride)
            hip.se_gate_add(res, g, sc, y, nimg=nimg, H=OH, W=OW, C_=depth, sc_stride=0, z=zn, za=za, zb=zb)
        else:                                      # MaxPool2d(1, s): the input, subsampled
            hip.se_gate_add(res, g, x, y, nimg=nimg, H=H, W=W, C_=depth, sc_stride=stride, z=zn, za=za, zb=zb)
        return y, zn, OH, OW

    # ---- the network -----------------------------------------------------------------------------------------------------
    def _need_net(self):
        if not hasattr(self, "head_w"):
            raise hip.VFaceHipError("this engine holds units only: it was built without the network's state dict")

    @torch.no_grad()
    def features(self, x8: torch.Tensor, B: int, taps: Optional[dict] = None) -> torch.Tensor:
        """Token rows [B 112 112, 8] of the network's input -> fp32 [B, 512], rows of unit length.  ``taps``: a dict that receives
        clones of the stem's and every unit's output (tests)."""
        self._need_net()
        S = hip.ID_SIZE
        if not x8.is_cuda:
            raise hip.VFaceHipError("the identity network runs on the GPU: its input must be a device tensor (no CPU fallback)")
        if x8.dtype != self.dtype or tuple(x8.shape) != (B * S * S, 8) or not x8.is_contiguous():
            raise hip.VFaceHipError(f"features: input must be contiguous {self.dtype} [{B * S * S}, 8]; got {x8.dtype} {tuple(x8.shape)}")
        M = B * S * S
        x, z = self._buf(M, 64), self._buf(M, 64)
        p = self.P["input_layer.0"]      # (its "cin" is the module's 3: the rows and the packed weight hold 8)
        hip.conv3x3(x8, p["w"], x, nimg=B, H=S, W=S, cin=8, cout=p["cout"], ldx=8, ldy=x.stride(0), bias=p["b"])
        first = self.units[0][0]
        hip.prelu(x, self.slope["input_layer"], x, M=M, C_=64, z=z, za=self.lead[first][0], zb=self.lead[first][1])
        if taps is not None:
            taps["input_layer"] = x.clone()
        H = W = S
        for i, (u, cin, depth, stride) in enumerate(self.units):
            nxt = self.units[i + 1][0] if i + 1 < len(self.units) else None
            x, z, H, W = self.unit(u, x, z, nimg=B, H=H, W=W, cin=cin, depth=depth, stride=stride, nxt=nxt)
            if taps is not None:
                taps[u] = x.clone()
        K = H * W * FEAT
        raw = torch.empty(B, FEAT, dtype=torch.float32, device=self.dev)
        hip.gemm(x, self.head_w, raw, M=B, N=FEAT, K=K, lda=K, ldc=FEAT, bias=self.head_b, flags=hip.EPI_OUT_F32, split_k=self.split_k)
        out = torch.empty(B, FEAT, dtype=torch.float32, device=self.dev)
        hip.l2norm_rows(raw, out, B=B, N=FEAT)
        return out

    @torch.no_grad()
    def prep(self, img: torch.Tensor, *, clip_img: bool = True, frames: bool = False, mask=None) -> torch.Tensor:
        """``extract_feats`` up to the network: fp32 [B, 3, H, W] on the device -> token rows [B 112 112, 8]."""
        if not img.is_cuda:
            raise hip.VFaceHipError("the identity network runs on the GPU: images must be device tensors (no CPU fallback)")
        B, _, H, W = img.shape
        out = self._buf(B * hip.ID_SIZE * hip.ID_SIZE, 8)
        mk = None if mask is None else mask.float().reshape(B, H, W).contiguous()
        hip.id_prep(img.float().contiguous(), out, clip_img=clip_img, prep=frames, mask=mk)
        return out

    def extract_feats(self, img: torch.Tensor, clip_img: bool = True) -> torch.Tensor:
        return self.features(self.prep(img, clip_img=clip_img), img.shape[0])

    def extract_feats_from_frames(self, frames: torch.Tensor, mask=None) -> torch.Tensor:
        return self.features(self.prep(frames, frames=True, mask=mask), frames.shape[0])
