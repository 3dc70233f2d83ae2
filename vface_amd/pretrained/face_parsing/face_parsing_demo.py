"""``FaceParser`` / ``faceParsing_demo`` of ``REFace/pretrained/face_parsing/face_parsing_demo.py`` on the HIP kernels.

The reference parses one PIL image at a time: resize to 1024 x 1024 on the caller's side (VFace_inference_batch.py:292), the
factor-2 bicubic pre-filter and normalisation, BiSeNet in fp32, argmax, a copy to the host and the 19 -> 12 relabelling in numpy.
Here ``FaceParser.labels`` does the same for a batch of aligned crops that are already on the device and returns the label maps
there; ``faceParsing_demo`` keeps the reference's one-image surface on top of it.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch
from torch import nn

from ... import hip
from ...scripts.resample import resample_coeffs
from ...utils import synth
from .model import BiSeNet


class FaceParser(nn.Module):
    """``seg_ckpt``: a face-parsing state dict on disk (the 79999_iter.pth of the reference's README), or None for the name-keyed
    synthetic fill (``synth.fill_parser_``) every other network of this build runs on where checkpoints are absent.  ``size``: the
    side of the crops the pre-filter reads (twice the network's input)."""

    def __init__(self, seg_ckpt=None, size: int = 1024, device="cuda", dtype: torch.dtype = torch.float16, seed: int = 0):
        super().__init__()
        if size % 64 or size < 128:
            raise hip.VFaceHipError(f"FaceParser: size must be a multiple of 64 and at least 128 (the network's input is size / 2, "
                                    f"a multiple of 32); got {size}")
        self.seg_ckpt, self.size, self.device = seg_ckpt, size, torch.device(device)
        self.seg = BiSeNet(n_classes=19, compute_dtype=dtype)
        if seg_ckpt is None:
            synth.fill_parser_(self.seg, seed=seed)
        else:
            self.seg.load_state_dict(torch.load(seg_ckpt, map_location="cpu", weights_only=True))
        for p in self.seg.parameters():
            p.requires_grad = False
        self.seg.to(self.device).eval()
        self._tables: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}

    def _resize(self, crops: torch.Tensor) -> torch.Tensor:
        """``img.resize((size, size), Image.BILINEAR)`` (VFace_inference_batch.py:292): Pillow's x pass, then its y pass."""
        _, h, w, _ = crops.shape
        for axis, n in ((0, w), (1, h)):
            if n != self.size:
                if (n, self.size) not in self._tables:
                    b, k = resample_coeffs(n, self.size, "bilinear")
                    self._tables[(n, self.size)] = (torch.from_numpy(b).to(crops.device), torch.from_numpy(k).to(crops.device))
                crops = hip.resample_u8(crops, self.size, axis, *self._tables[(n, self.size)])
        return crops

    @torch.no_grad()
    def labels(self, crops_u8: torch.Tensor, convert_to_seg12: bool = True) -> torch.Tensor:
        """uint8 crops [F, S, S, 3] on the device -> uint8 label maps [F, size / 2, size / 2] on the device."""
        if not isinstance(crops_u8, torch.Tensor) or not crops_u8.is_cuda:
            raise hip.VFaceHipError("the face parser runs on the GPU: crops must be device tensors (no CPU fallback)")
        if crops_u8.dtype != torch.uint8 or crops_u8.dim() != 4 or crops_u8.shape[3] != 3:
            raise hip.VFaceHipError(f"labels: crops must be uint8 [F, S, S, 3]; got {crops_u8.dtype} {tuple(crops_u8.shape)}")
        return self.seg.engine.labels(self._resize(crops_u8.contiguous()), convert_to_seg12)

    def forward(self, img) -> torch.Tensor:
        """A PIL image -> its 19-class map as an int64 tensor [size / 2, size / 2] on the device (the reference's return)."""
        u8 = torch.from_numpy(np.array(img.convert("RGB"))).to(self.device)
        return self.labels(u8[None], convert_to_seg12=False)[0].long()


def init_faceParsing_pretrained_model(faceParser_name, ckpt_path, config_path=""):
    if faceParser_name == "default":
        return FaceParser(seg_ckpt=ckpt_path)
    if faceParser_name == "segnext":
        raise NotImplementedError("the segnext parser is mmseg's (third party); only the default BiSeNet parser is built here")
    raise ValueError(f"unknown face parser {faceParser_name!r} (default | segnext)")


def faceParsing_demo(model, img, convert_to_seg12=True, model_name="default"):
    """``model``: a ``FaceParser``; ``img``: a PIL image.  Returns the label map as a numpy uint8 array, 12 classes by default."""
    if model_name == "segnext":
        raise NotImplementedError("the segnext parser is mmseg's (third party); only the default BiSeNet parser is built here")
    if model_name != "default":
        raise ValueError(f"unknown face parser {model_name!r} (default | segnext)")
    u8 = torch.from_numpy(np.array(img.convert("RGB"))).to(model.device)
    return model.labels(u8[None], convert_to_seg12=convert_to_seg12)[0].cpu().numpy()
