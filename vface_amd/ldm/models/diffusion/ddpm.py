"""The thin slice of ``REFace/ldm/models/diffusion/ddpm.py`` that sits on the hot path:
``LatentDiffusion.apply_model`` (ddpm.py:1519-1617) and ``DiffusionWrapper.forward`` (:2231-2257) for
``conditioning_key: crossattn``, plus the schedule buffers of ``DDPM.register_schedule`` the sampler reads.
The first-stage VAE is optional: ``first_stage_config`` builds ``AutoencoderKL`` under ``first_stage_model``
and ``encode_first_stage`` / ``get_first_stage_encoding`` / ``decode_first_stage`` (:1402, :850-857, :1277-1284) work as in
the reference.  The conditioning stage is optional too: ``cond_stage_config`` builds ``FrozenCLIPEmbedder`` under
``cond_stage_model`` with the projections of ddpm.py:695-733, and ``get_learned_conditioning`` (:859-870) /
``conditioning_with_feat`` (:872-1045, the shipped configuration) run on the GPU.  ``other_params.arcface`` adds ``IDLoss``
(:91-124) under ``face_ID_model`` -- ArcFace IR-SE50 behind the pooling and crop chain of ``extract_feats``, on the HIP kernels
(``vface_amd.arcface``) -- and ``conditioning_with_feat`` then computes ``id_feat`` itself; without it the features stay an input,
as the dlib landmarks always do.  Losses and training (the other ~2000 lines) are out of scope.

State-dict keys of the UNet are ``model.diffusion_model.*`` as in ``last.ckpt`` so
``load_state_dict(ckpt["state_dict"], strict=False)`` (VFace_inference_batch.py:118-135) fills it unchanged.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from ...modules.diffusionmodules.openaimodel import UNetModel
from ...modules.diffusionmodules.util import make_beta_schedule


class DiffusionWrapper(nn.Module):
    def __init__(self, unet: UNetModel, conditioning_key="crossattn"):
        super().__init__()
        if conditioning_key != "crossattn":
            raise NotImplementedError("the VFace configuration uses conditioning_key='crossattn' (project_ffhq.yaml:13)")
        self.diffusion_model = unet
        self.conditioning_key = conditioning_key

    def forward(self, x, t, c_concat=None, c_crossattn=None):
        cc = c_crossattn[0] if len(c_crossattn) == 1 else torch.cat(c_crossattn, 1)
        return self.diffusion_model(x, t, context=cc)


class IDLoss(nn.Module):
    """``IDLoss`` of ddpm.py:91-124 as far as inference uses it: ``facenet`` (``Backbone(112, 50, 'ir_se', drop_ratio=0.6)``, :98)
    and ``extract_feats``.  ``arcface_path``: a state-dict file for ``facenet`` (:101), read with ``weights_only=True``; None leaves
    the parameters to the caller (a checkpoint's ``face_ID_model.facenet.*`` keys, or a fill)."""

    def __init__(self, arcface_path=None, multiscale: bool = False, compute_dtype: torch.dtype = torch.float16):
        super().__init__()
        from ....arcface import check_config
        from ....src.Face_models.encoders.model_irse import Backbone
        check_config(multi_scale=multiscale)
        self.multiscale = False
        self.facenet = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode="ir_se", compute_dtype=compute_dtype)
        if arcface_path is not None:
            self.facenet.load_state_dict(torch.load(arcface_path, map_location="cpu", weights_only=True))
        self.eval()
        for p in self.parameters():
            p.requires_grad = False

    @torch.no_grad()
    def extract_feats(self, x, clip_img: bool = True):
        """:112-124: ``x [B, 3, H, W]`` on the device (CLIP-normalised with ``clip_img``) -> ``[features]``, fp32 [B, 512]."""
        return [self.facenet.engine.extract_feats(x, clip_img=clip_img)]

    @torch.no_grad()
    def extract_feats_from_frames(self, frames, mask=None):
        """``extract_feats(prep(frames * (1 - mask)))`` in one pass: ``frames [B, 3, H, W]`` in [-1, 1] at any size, ``prep`` the
        resize and CLIP normalisation ``FrozenCLIPEmbedder.encode_from_frames`` applies (the two see the same image)."""
        return [self.facenet.engine.extract_feats_from_frames(frames, mask)]

    def forward(self, *a, **k):
        raise NotImplementedError("IDLoss.forward is the training loss (ddpm.py:128-170); inference uses extract_feats only")


class LatentDiffusion(nn.Module):
    def __init__(self, unet_config: dict, timesteps=1000, linear_start=0.00085, linear_end=0.012,
                 beta_schedule="linear", scale_factor=0.18215, parameterization="eps", first_stage_config=None,
                 cond_stage_config=None):
        super().__init__()
        self.model = DiffusionWrapper(UNetModel(**unet_config))
        if first_stage_config is not None:
            from ..autoencoder import AutoencoderKL
            self.first_stage_model = AutoencoderKL(**first_stage_config)
        if cond_stage_config is not None:
            self._init_cond_stage(dict(cond_stage_config))
        self.parameterization = parameterization
        self.scale_factor = scale_factor
        self.num_timesteps = int(timesteps)
        betas = make_beta_schedule(beta_schedule, timesteps, linear_start=linear_start, linear_end=linear_end)
        ac = np.cumprod(1.0 - betas, axis=0)
        f32 = lambda a: torch.tensor(a, dtype=torch.float32)
        self.register_buffer("betas", f32(betas), persistent=False)
        self.register_buffer("alphas_cumprod", f32(ac), persistent=False)
        self.register_buffer("alphas_cumprod_prev", f32(np.append(1.0, ac[:-1])), persistent=False)

    @property
    def device(self):
        return self.betas.device

    @property
    def unet(self) -> UNetModel:
        return self.model.diffusion_model

    # ---- first stage (ddpm.py:1402-1420, 850-857, 1277-1300; the patch-split branches are not configured) ----
    def encode_first_stage(self, x):
        return self.first_stage_model.encode(x)

    def get_first_stage_encoding(self, encoder_posterior, noise=None):
        from ...modules.distributions.distributions import DiagonalGaussianDistribution
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            return encoder_posterior.sample(noise, scale=self.scale_factor)   # scale_factor * sample(), one kernel
        if isinstance(encoder_posterior, torch.Tensor):
            return self.scale_factor * encoder_posterior
        raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")

    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False):
        if predict_cids:
            raise NotImplementedError("predict_cids belongs to VQ first stages; the VFace configuration uses AutoencoderKL")
        return self.first_stage_model.decode(1. / self.scale_factor * z)

    # ---- conditioning stage (ddpm.py:598-733, 859-870, 872-1045; project_ffhq.yaml:79-99) ----
    def _init_cond_stage(self, cfg: dict):
        from ...modules.encoders.modules import FrozenCLIPEmbedder
        target = cfg.get("target", "ldm.modules.encoders.modules.FrozenCLIPEmbedder")
        if not target.endswith("encoders.modules.FrozenCLIPEmbedder"):
            raise NotImplementedError(f"cond_stage_config.target {target!r}: the shipped configuration uses FrozenCLIPEmbedder")
        op = {**FFHQ_COND_PARAMS, **cfg.get("other_params", {})}
        add = {**FFHQ_COND_PARAMS["Additional_config"], **op.get("Additional_config", {})}
        for flag in ("concat_feat", "land_mark_id_seperate_layers", "multi_scale_ID", "sep_head_att", "stack_feat", "normalize"):
            if op.get(flag, False):
                raise NotImplementedError(f"other_params.{flag} is false in the shipped configuration (project_ffhq.yaml:87-90)")
        if not (add["Source_CLIP_feat"] and add["Target_CLIP_feat"] and op["Landmark_cond"] and op["weight_division"]):
            raise NotImplementedError("the shipped configuration has Source_CLIP_feat, Target_CLIP_feat, Landmark_cond and weight_division on")
        if not (op["clip_weight"] > 0 and op["ID_weight"] > 0):
            raise NotImplementedError("the shipped configuration mixes CLIP and identity features (clip_weight 1.0, ID_weight 10.0)")
        self.clip_weight, self.ID_weight, self.Landmarks_weight = float(op["clip_weight"]), float(op["ID_weight"]), float(op["Landmarks_weight"])
        self.Landmark_cond, self.weight_division, self.normalize = True, True, False
        self.Source_CLIP_feat = self.Target_CLIP_feat = True
        self.cond_stage_model = FrozenCLIPEmbedder(**cfg.get("params", {}))
        self.learnable_vector = nn.Parameter(torch.randn((1, 1, 768)), requires_grad=False)
        self.proj_out_source, self.proj_out_target = nn.Linear(768, 768), nn.Linear(768, 768)
        self.proj_out = nn.Identity()
        self.ID_proj_out = nn.Linear(512, 768)
        self.landmark_proj_out = nn.Linear(136, 768)
        self._cond_packed = None
        arcface = op.get("arcface", False)
        if arcface:      # True: parameters come from the checkpoint (face_ID_model.facenet.*) or a fill; a str: other_params.arcface_path
            self.face_ID_model = IDLoss(arcface if isinstance(arcface, str) else None,
                                        compute_dtype=cfg.get("params", {}).get("compute_dtype", torch.float16))

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """With a conditioning stage, the checkpoint's ``cond_stage_model.*`` keys that FrozenCLIPEmbedder holds without reading
        (the text tower, ``mapper``, ``final_ln``, ``projection_back``) are dropped before loading."""
        if hasattr(self, "cond_stage_model"):
            from .... import clip
            pre = "cond_stage_model."
            state_dict = {k: v for k, v in state_dict.items()
                          if not (k.startswith(pre) and k[len(pre):].startswith(clip.UNUSED_PREFIXES))}
            self.cond_stage_model._engine = None
            self._cond_packed = None
            if hasattr(self, "face_ID_model"):
                self.face_ID_model.facenet._engine = None
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def _apply(self, fn, *a, **k):
        self._cond_packed = None
        return super()._apply(fn, *a, **k)

    def get_learned_conditioning(self, c):
        return self.cond_stage_model.encode(c)

    def _cond_weights(self):
        """The four projections in the compute type (landmark_proj_out's K = 136 zero-padded to 192), built on first use."""
        if self._cond_packed is None:
            dt = self.cond_stage_model.compute_dtype
            pk = {}
            for name in ("proj_out_source", "proj_out_target", "ID_proj_out", "landmark_proj_out"):
                lin = getattr(self, name)
                w = lin.weight.detach().float()
                if w.shape[1] % 64:
                    w = torch.cat([w, w.new_zeros(w.shape[0], -w.shape[1] % 64)], 1)
                pk[name] = (w.to(dt).contiguous(), lin.bias.detach().float().contiguous())
            self._cond_packed = pk
        return self._cond_packed

    @torch.no_grad()
    def conditioning_with_feat(self, x, landmarks=None, tar=None, id_feat=None, *, e_src=None, e_tar=None):
        """ddpm.py:872-1045 in the shipped configuration, ``[B, 1, 768]`` fp32:
            c  = proj_out_source(E(x)) + proj_out_target(E(prep(tar)))            x [1 | B, 3, 224, 224] CLIP-normalised
            c2 = ID_proj_out(id_feat)[:, None]                                    id_feat [1 | B, 512]: the ArcFace features; None:
                                                                                  face_ID_model.extract_feats(x)[0] (:1010), which
                                                                                  needs the stage built with other_params.arcface
            lm = landmark_proj_out(landmarks)[:, None]                            landmarks [B, 136]: dlib's, an input as in the reference
            (c clip_weight + c2 ID_weight + lm Landmarks_weight) / (clip_weight + ID_weight + Landmarks_weight)
        ``e_src`` / ``e_tar``: E(x) / E(prep(tar)) where the caller already has them -- a clip's source image is encoded once, and
        both conditions of a batch (scripts/VFace_inference_batch.py:442, :500) share E(prep(tar))."""
        from .... import hip
        if id_feat is None and x is not None and hasattr(self, "face_ID_model"):
            id_feat = self.face_ID_model.extract_feats(x)[0]
        if landmarks is None or id_feat is None or (tar is None and e_tar is None) or (x is None and e_src is None):
            raise NotImplementedError("the shipped configuration mixes CLIP (source and target), identity and landmark features: "
                                      "x, tar, landmarks and id_feat are all needed (id_feat = face_ID_model.extract_feats(x)[0], not computed here)")
        enc, pk = self.cond_stage_model, self._cond_weights()
        dt, dev = enc.compute_dtype, landmarks.device
        if e_tar is None:
            e_tar = enc.encode_from_frames(tar)
        if e_src is None:
            e_src = self.get_learned_conditioning(x)
        B, Bs = e_tar.shape[0], e_src.shape[0]
        if Bs not in (1, B):
            raise ValueError(f"{Bs} source images for {B} target frames")
        if id_feat.shape[0] not in (1, B):
            raise ValueError(f"{id_feat.shape[0]} identity features for {B} target frames")
        id_feat = id_feat.reshape(id_feat.shape[0], 512).expand(B, 512)      # one source for the batch: c2 is broadcast (:1038)
        f32 = lambda: torch.empty(B, 768, dtype=torch.float32, device=dev)

        def linear(a, name, M, out32, **kw):
            w, b = pk[name]
            hip.gemm(a, w, None, M=M, N=768, K=w.shape[1], lda=a.stride(0), ldc=768, bias=b, out32=out32, split_k=False, **kw)

        def staged(t, K):       # a [B, k] fp32 input as zero-padded 16-bit rows
            buf = torch.zeros(B, K, dtype=dt, device=dev)
            buf[:, :t.shape[-1]] = t.reshape(B, -1).to(device=dev, dtype=dt)
            return buf

        c_src = torch.empty(Bs, 768, dtype=torch.float32, device=dev)
        linear(e_src.view(Bs, 768), "proj_out_source", Bs, c_src)
        c, c2, lm = f32(), f32(), f32()
        linear(e_tar.view(B, 768), "proj_out_target", B, c, rowbias=c_src, rows_per_sample=B if Bs == 1 else 1)
        linear(staged(id_feat, 512), "ID_proj_out", B, c2)
        linear(staged(landmarks, pk["landmark_proj_out"][0].shape[1]), "landmark_proj_out", B, lm)
        out = f32()
        hip.cond_mix([(c, self.clip_weight), (c2, self.ID_weight), (lm, self.Landmarks_weight)], B=B, N=768, out32=out, ldo32=768)
        return out.view(B, 1, 768)

    def apply_model(self, x_noisy, t, cond):
        if isinstance(cond, dict):
            return self.model(x_noisy, t, **cond)
        if not isinstance(cond, list):
            cond = [cond]
        return self.model(x_noisy, t, c_crossattn=cond)


# project_ffhq.yaml:81-99 (+ the defaults of ddpm.py:644-647 for what the yaml leaves out)
FFHQ_COND_PARAMS = dict(clip_weight=1.0, ID_weight=10.0, Landmark_cond=True, Landmarks_weight=0.05, concat_feat=False,
                        land_mark_id_seperate_layers=False, multi_scale_ID=False, sep_head_att=False, weight_division=True,
                        Additional_config=dict(Target_CLIP_feat=True, Source_CLIP_feat=True))

# project_ffhq.yaml:33-56
FFHQ_UNET_CONFIG = dict(image_size=32, in_channels=9, out_channels=4, model_channels=320,
                        attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8,
                        use_spatial_transformer=True, transformer_depth=1, context_dim=768, use_checkpoint=True,
                        legacy=False, add_conv_in_front_of_unet=False)
