"""``FrozenCLIPEmbedder`` of ``REFace/ldm/modules/encoders/modules.py:211-264``: same ``forward`` / ``encode`` surface and the same
state-dict keys for what its forward reads (``model.vision_model.*``, ``model.visual_projection.weight``, ``mapper2.*``,
``final_ln2.*``); the computation is ``vface_amd.clip.ClipEngine`` on the GPU.  What the reference's class holds without reading --
the text tower, ``text_projection``, ``logit_scale``, ``mapper``, ``final_ln``, ``projection_back`` -- has no parameters here: those
keys of a checkpoint are accepted and dropped; any other unknown key is refused.

Nothing is fetched: the reference builds the towers with ``CLIPModel.from_pretrained(version)``; this class takes the vision
tower's sizes as a dict (default: ``openai/clip-vit-large-patch14``'s) and its weights from ``load_state_dict``.  The other encoders
of the reference's file are out of scope."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .... import clip
from ....convnet import EngineOwner


def _register(root: nn.Module, key: str, shape) -> None:
    """A zero parameter under the dotted state-dict name ``key`` (plain ``nn.Module`` containers along the path)."""
    *path, leaf = key.split(".")
    mod = root
    for name in path:
        if name not in mod._modules:
            mod.add_module(name, nn.Module())
        mod = mod._modules[name]
    mod.register_parameter(leaf, nn.Parameter(torch.zeros(*shape), requires_grad=False))


class AbstractEncoder(nn.Module):
    def __init__(self):
        super().__init__()

    def encode(self, *args, **kwargs):
        raise NotImplementedError


class FrozenCLIPEmbedder(EngineOwner, nn.Module):
    def __init__(self, version: str = "openai/clip-vit-large-patch14", vision_config: Optional[dict] = None,
                 compute_dtype: torch.dtype = torch.float16):
        super().__init__()
        if vision_config is None and version != "openai/clip-vit-large-patch14":
            raise NotImplementedError(f"{version!r}: nothing is fetched by name; pass the vision tower's sizes as vision_config "
                                      "(hidden, heads, layers, mlp, image)")
        self.version = version
        self.vision_config = dict(clip.VIT_L14 if vision_config is None else vision_config)
        self.compute_dtype = compute_dtype
        for key, shape in clip.state_shapes(self.vision_config).items():
            _register(self, key, shape)

    def _make_engine(self) -> "clip.ClipEngine":
        return clip.ClipEngine(self.state_dict(), self.vision_config, self.compute_dtype, next(self.parameters()).device)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """The reference's state dict unchanged: unused keys dropped, unknown ones, missing ones and wrong shapes refused."""
        used, _ = clip.split_state_dict(state_dict, self.vision_config)
        return super().load_state_dict(used, strict=strict, **kw)

    def freeze(self):
        for param in self.parameters():
            param.requires_grad = False

    @torch.no_grad()
    def forward(self, image: torch.Tensor) -> torch.Tensor:
        """CLIP-normalised images ``[B, 3, 224, 224]`` on the GPU -> ``[B, 1, 768]`` in the compute type (modules.py:253-261)."""
        return self.engine.encode(image)

    def encode(self, image):
        return self(image)

    @torch.no_grad()
    def encode_from_frames(self, tar: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``encode(prep(tar))`` for frames in [-1, 1] of any size, the resize fused into the patch gather (ddpm.py:907-913)."""
        return self.engine.encode_from_frames(tar, mask)

    def forward_probabilities(self, text, image):
        raise NotImplementedError("forward_probabilities needs the text tower and a tokenizer (modules.py:266-285); the VFace path "
                                  "never calls it")


def _out_of_scope(name: str, why: str):
    class _Stub(AbstractEncoder):
        def __init__(self, *a, **k):
            raise NotImplementedError(f"{name}: {why}")
    _Stub.__name__ = _Stub.__qualname__ = name
    return _Stub


_WHY = "not used by the shipped configuration (project_ffhq.yaml:79-80 targets FrozenCLIPEmbedder)"
ClassEmbedder = _out_of_scope("ClassEmbedder", _WHY)
TransformerEmbedder = _out_of_scope("TransformerEmbedder", _WHY)
BERTTokenizer = _out_of_scope("BERTTokenizer", _WHY)
BERTEmbedder = _out_of_scope("BERTEmbedder", _WHY)
SpatialRescaler = _out_of_scope("SpatialRescaler", _WHY)
FrozenCLIPImageEmbedder = _out_of_scope("FrozenCLIPImageEmbedder", _WHY)
FrozenCLIPTextEmbedder = _out_of_scope("FrozenCLIPTextEmbedder", _WHY)
