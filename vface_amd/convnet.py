"""What the convolutional engines beside the UNet share (``raft.RaftEngine``, ``parsing.ParseEngine``): the packed-weight table, the
two convolution launches, the 8-column token rows, and the lazily built engine of their ``nn.Module`` parameter containers.  Nothing
here knows a network: each engine converts its own state dict, lists its own layers and walks them itself.  No CPU fallback: without
the HIP library every engine raises at construction.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import hip, packing


def fold_bn(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, eps: float = 1e-5,
            b: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``BatchNorm(eval)(conv(x, w) + b)`` == ``conv(x, w') + b'`` (an exact refactoring in real arithmetic); ``b=None`` is ``b = 0``.
    Computed in the dtype of the inputs: the caller chooses fp32 or fp64 by what it passes."""
    scale = gamma / torch.sqrt(var + eps)
    return w * scale.reshape(-1, *([1] * (w.dim() - 1))), ((0 if b is None else b) - mean) * scale + beta


class ConvNetEngine:
    """Packed convolutions ``self.P[name]`` on device buffers and the launches that run them."""

    # Whether ``window`` lets ``vface_gemm`` split K.  The split is chosen from M, so from the batch: the face parser promises that a
    # frame's labels do not depend on the frames sharing its batch and turns it off; the flow producer agrees across batch sizes to
    # rounding only, and keeps the launches it was measured with.  It decides the bits of either network: do not unify it.
    split_k = True

    def __init__(self, dtype: torch.dtype, device):
        hip.load()      # no CPU fallback: fail here if the library is missing
        hip.dtype_code(dtype)
        self.dtype, self.dev = dtype, torch.device(device)
        self.P: Dict[str, dict] = {}

    # ---- weights --------------------------------------------------------------------------------------------------------
    def add_conv(self, sd, name, bn: Optional[str] = None, cin_pad: Optional[int] = None, cout_pad: Optional[int] = None,
                 store: Optional[str] = None, pooled: bool = False):
        """``sd[name + ".weight"]`` (+ ``".bias"`` if present), eval-mode BatchNorm ``bn`` folded in the dtype of ``sd``, output
        channels zero-padded to ``cout_pad``, then fp32 and packed: 3x3 for ``vface_conv3x3``, any other window in the row order of
        ``vface_im2col``, both in the compute type; ``pooled`` (a 1x1 convolution on a pooled vector) as fp32 [N, K].  The bias is
        fp32, or None for a layer with neither a bias nor a BatchNorm."""
        w, b = sd[name + ".weight"], sd.get(name + ".bias")
        if bn is not None:
            w, b = fold_bn(w, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"], b=b)
        cout, cin, kh, kw = w.shape
        if cout_pad is not None and cout_pad > cout:
            w = torch.cat([w, w.new_zeros(cout_pad - cout, cin, kh, kw)], 0)
            b = b if b is None else torch.cat([b, b.new_zeros(cout_pad - cout)])
        w = w.float()
        if pooled:
            wp, kind = w.reshape(w.shape[0], cin).contiguous(), "pooled"
        elif (kh, kw) == (3, 3):
            wp, kind = packing.pack_conv3x3(w, cin_pad).to(self.dtype), "conv3"
        else:
            wp, kind = packing.pack_conv_im2col(w, cin_pad).to(self.dtype), "gemm"
        self.P[store or name] = {"w": wp.to(self.dev), "b": b if b is None else b.float().to(self.dev), "kh": kh, "kw": kw,
                                 "cout": w.shape[0], "cin": cin, "kind": kind}

    # ---- building blocks -------------------------------------------------------------------------------------------------
    def _buf(self, rows, cols, dtype=None):
        return torch.empty(rows, cols, dtype=dtype or self.dtype, device=self.dev)

    def conv3(self, name, x, out, *, nimg, H, W, ldx, stride=1, upsample=False, out32=False):
        p = self.P[name]
        hip.conv3x3(x, p["w"], out, nimg=nimg, H=H, W=W, cin=p["cin"], cout=p["cout"], ldx=ldx, ldy=out.stride(0), stride=stride,
                    upsample=upsample, bias=p["b"], flags=hip.EPI_OUT_F32 if out32 else 0)

    def window(self, name, x, out, *, nimg, H, W, C_, ldx, stride=1, out32=False):
        """kh x kw convolution, 'same' padding, through the explicit window matrix (a 1x1 stride-1 window needs none)."""
        p = self.P[name]
        kh, kw = p["kh"], p["kw"]
        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        M, K = nimg * OH * OW, kh * kw * C_
        if kh == kw == 1 and stride == 1:
            a, lda = x, ldx
        else:
            a = self._buf(M, K)
            hip.im2col(x, a, nimg=nimg, H=H, W=W, C_=C_, kh=kh, kw=kw, stride=stride, pad_y=(kh - 1) // 2, pad_x=(kw - 1) // 2, ldx=ldx)
            lda = K
        hip.gemm(a, p["w"], out, M=M, N=p["cout"], K=K, lda=lda, ldc=out.stride(0), bias=p["b"],
                 flags=hip.EPI_OUT_F32 if out32 else 0, split_k=self.split_k)

    def tokens8(self, img: torch.Tensor) -> torch.Tensor:
        """Images [N, C <= 8, H, W] (any float type) -> the 8-channel token rows a stem reads."""
        if not img.is_cuda:
            raise hip.VFaceHipError("the engine runs on the GPU: images must be device tensors (no CPU fallback)")
        N, C_, H, W = img.shape
        out = self._buf(N * H * W, 8)
        hip.nchw_to_nhwc(img.float().contiguous(), out, N=N, C_=C_, hw=H * W, cpad=8)
        return out


class EngineOwner:
    """Mixin of an ``nn.Module`` parameter container (listed before it): ``engine`` is built from the parameters on first use by
    ``_make_engine()`` and dropped whenever they are loaded, moved or cast."""
    _engine = None

    @property
    def engine(self):
        if self._engine is None:
            self._engine = self._make_engine()
        return self._engine

    def load_state_dict(self, *a, **k):
        self._engine = None
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)
