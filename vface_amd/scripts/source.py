"""The clip-level source state: what ``REFace/scripts/VFace_inference_batch.py`` derives from the source image once per clip and
hands to every batch's DDIM inversion (:436-438, :462-468, :509-527).

    reference                                                                               here
    --------------------------------------------------------------------------------------  ---------------------------------
    cond_w_src = conditioning_with_feat(ref_image_tensor, landmarks_src, tar=ref_img_inv)   :437   SourceState.cond_w_src
    z_inpaint_src = get_first_stage_encoding(encode_first_stage(ref_img_inv_ori_inpaint))   :465-466   SourceState.z_inpaint
    inpaint_mask_src = Resize([h, w])(1 - reference_mask_tensor)                            :462, :468 SourceState.mask_latent
    z_ref = get_first_stage_encoding(encode_first_stage(ref_img_inv))                       :509-512   SourceState.z_ref
    z2 = cat([z2_tar, z_ref]); cond = cat([inverse_cond, cond_w_src]); inpaint_* = cat(..)  :513-525   inversion_operands

The reference repeats the source rows over the batch's frames before (:509) or after (:438, :522-523) computing them; here each
is computed once for the clip and broadcast.  ``landmarks_src`` (dlib, :436) stays an input, as the target landmarks are.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .intake import SourceTensors


@dataclass
class SourceState:
    z_ref: torch.Tensor                          # [1, 4, h, w]   :509-512
    z_inpaint: torch.Tensor                      # [1, 4, h, w]   :465-466
    mask_latent: torch.Tensor                    # [1, 1, h, w]   :462, :468
    e_source: Optional[torch.Tensor] = None      # E(ref_image_tensor), shared with every batch's `c` (:442)
    id_source: Optional[torch.Tensor] = None     # [1, 512] the source's identity features (:437, :442 -> ddpm.py:1010)
    cond_w_src: Optional[torch.Tensor] = None    # [1, 1, 768]    :437

    def inversion_operands(self, z2_tar: torch.Tensor, inverse_cond: torch.Tensor, z_inpaint_tar: torch.Tensor,
                           mask_latent_tar: torch.Tensor, cond_src: Optional[torch.Tensor] = None):
        """``x, cond, test_model_kwargs`` of the inversion of ``[target ; source]`` (:513-525, :531-540) for a batch of F frames:
        the target halves are the arguments, the source halves the clip's single row repeated F times.  ``cond_src``: the
        condition of the source half where the model has no conditioning stage (``cond_w_src`` is None then)."""
        F_ = z2_tar.shape[0]
        src = self.cond_w_src if cond_src is None else cond_src
        if src is None:
            raise ValueError("inversion_operands: the model has no conditioning stage, so the source half's condition must be given")
        rep = lambda t: t.expand(F_, *t.shape[1:]) if t.shape[0] == 1 else t
        x = torch.cat([z2_tar, rep(self.z_ref)])                                                   # :514
        cond = torch.cat([inverse_cond, rep(src)])                                                 # :515
        kw = {"inpaint_image": torch.cat([z_inpaint_tar, rep(self.z_inpaint)]),                    # :524
              "inpaint_mask": torch.cat([mask_latent_tar, rep(self.mask_latent)])}                 # :525
        return x, cond, kw


@torch.no_grad()
def prepare_source(model, src: SourceTensors, landmarks_src: Optional[torch.Tensor] = None,
                   id_feat: Optional[torch.Tensor] = None) -> SourceState:
    """``src``: ``FrameIntake.source`` of ONE source image.  ``model``: a ``LatentDiffusion`` with a first stage; with a conditioning
    stage it also needs ``landmarks_src`` [1, 136] and, unless the stage was built with ArcFace, the identity features ``id_feat``
    [1, 512]."""
    if src.masked.shape[0] != 1:
        raise ValueError(f"prepare_source: one source image per clip; got {src.masked.shape[0]}")
    z_ref = model.get_first_stage_encoding(model.encode_first_stage(src.masked)).detach()              # :509-512
    z_inpaint = model.get_first_stage_encoding(model.encode_first_stage(src.inpaint_image)).detach()   # :465-466
    state = SourceState(z_ref, z_inpaint, src.inpaint_mask_latent)
    if hasattr(model, "cond_stage_model"):
        state.e_source = model.get_learned_conditioning(src.clip_image)
        state.id_source = model.face_ID_model.extract_feats(src.clip_image)[0] if hasattr(model, "face_ID_model") else id_feat
        state.cond_w_src = model.conditioning_with_feat(                                               # :437
            None, landmarks=landmarks_src, id_feat=state.id_source, e_src=state.e_source,
            e_tar=model.cond_stage_model.encode_from_frames(src.masked))
    return state
