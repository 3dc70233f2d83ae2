"""Everything a run owns, built once from the normalised options before the first batch: the ``LatentDiffusion`` with its optional
stages, its weights (``--ckpt``, or the seeded fill), the sampler and its hook plan, the frame intake, the face parser, RAFT, the
paste-back and the clip-level source state.  Nothing here is inside a timed stage except the source intake, which times itself
(``source_seconds``, reported by batch 0)."""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Any, Optional

import torch

from ..utils import synth
from .checkpoint import load_checkpoint
from .intake import PRESERVE_MASK_SRC_FFHQ


@dataclass
class Run:
    opt: Any
    device: torch.device
    model: Any
    sampler: Any = None
    started: float = 0.0                    # the clock `total_seconds` counts from
    intake: Any = None                      # FrameIntake             --intake
    parser: Any = None                      # FaceParser              --parse
    raft: Any = None                        # RAFT                    --raft_flow
    paster: Any = None                      # PasteBack               --paste_back
    source_state: Any = None                # source.SourceState      --source_intake
    source_seconds: Optional[float] = None
    e_source: Optional[torch.Tensor] = None     # E(source image), once per clip (:437)    --clip_cond
    id_source: Optional[torch.Tensor] = None    # its identity features (ddpm.py:1010)     --arcface

    paste_noise: Optional[torch.Tensor] = None  # the next background round trip's posterior draw, where it was taken ahead
    plan: Any = None                            # [(first, count)] of the run's batches (inputs.batch_plan), set by the loop
    carry: Any = None                           # parallel.ClipCarry                       --whole_clip
    last_image: Optional[torch.Tensor] = None   # the previous batch's last target image, for the boundary flow field

    @property
    def latent(self):
        return self.opt.H // self.opt.f, self.opt.W // self.opt.f

    def background_round_trip(self, x):
        """The paste-back's background through the VAE (:615-617; ``PasteBack.vae_round_trip``).  Its posterior draw comes from
        torch's global generator, as every encoding's does, so WHEN it is drawn decides its value: ``paste_noise`` holds a draw the
        loop took ahead (pipeline.prepare_next), None draws here."""
        posterior = self.model.encode_first_stage(x)
        noise, self.paste_noise = self.paste_noise, None
        if noise is not None and tuple(noise.shape) != (posterior.F, posterior.zc, posterior.h, posterior.w):
            raise ValueError(f"background_round_trip: a draw of {tuple(noise.shape)} for a posterior of "
                             f"{(posterior.F, posterior.zc, posterior.h, posterior.w)}")
        return self.model.decode_first_stage(self.model.get_first_stage_encoding(posterior, noise))


def build_model(opt, inputs, cfg, dt):
    """The ``LatentDiffusion`` on the host, weights in: ``--ckpt``, or the seeded fill (UNet and VAE seed 0, conditioning seed 5)."""
    from ..ldm.models.diffusion.ddpm import LatentDiffusion
    cfg = dict(cfg, compute_dtype=dt)
    stage_kw = {}
    if opt.clip_cond:
        stage_kw["cond_stage_config"] = dict(params=dict(compute_dtype=dt), **(dict(other_params=dict(arcface=True)) if opt.arcface else {}))
    if opt.with_vae:
        from ..ldm.models.autoencoder import FFHQ_VAE_CONFIG
        stage_kw["first_stage_config"] = dict(FFHQ_VAE_CONFIG, compute_dtype=dt)
    model = LatentDiffusion(cfg, **stage_kw)
    if opt.ckpt:
        print(load_checkpoint(model, opt.ckpt, with_vae=opt.with_vae, stub_unknown_globals=opt.ckpt_stub_unknown_globals))
        return model
    synth.fill_module_(model.unet, seed=0)
    if opt.with_vae:
        synth.fill_module_(model.first_stage_model, seed=0, prefix="vae.")
    if opt.clip_cond:
        synth.fill_module_(model.cond_stage_model, seed=5)
        for name in ("proj_out_source", "proj_out_target", "ID_proj_out", "landmark_proj_out"):
            synth.fill_module_(getattr(model, name), seed=5, prefix=name + ".")
        if opt.arcface:
            synth.fill_arcface_(model.face_ID_model.facenet, seed=5, prefix="face_ID_model.facenet.")
        vector = inputs.learnable_vector()      # (read as `uc` by a run whose inputs draw none)
        if vector is not None:
            model.learnable_vector.data.copy_(vector)
    return model


def build_sampler(opt, model):
    from ..ldm.models.diffusion.ddim_w_inv import DDIMSampler, HookPlan
    sampler = DDIMSampler(model)
    sampler.hook_plan = HookPlan(fusion=opt.fusion, enabled=opt.fusion != "none")
    sampler.flow_gate = opt.flow_gate
    sampler.drop_dead_branches = bool(opt.drop_dead_branches)
    if opt.hip_graph:
        sampler.model.model.diffusion_model.engine.use_graph = True
    if opt.no_hip_graph:
        sampler.model.model.diffusion_model.engine.use_graph = False
    sampler.flow_resample = "area" if opt.flow_pixels or opt.raft_flow else None    # (RAFT's field is at pixel resolution)
    return sampler


def build_raft(opt, dt, dev):
    from ..raft import RAFT
    raft = RAFT(compute_dtype=dt)
    if opt.raft_ckpt:
        raft.load_state_dict(torch.load(opt.raft_ckpt, map_location="cpu", weights_only=True))
    else:
        synth.fill_module_(raft, seed=0, prefix="raft.")
    return raft.to(dev).eval()


def source_intake(run, inputs):
    """:254-355, :436-438, :462-468: the source image's side, once per clip.  Sets ``source_state`` and its wall seconds."""
    from .source import prepare_source
    frames, quads, labels, landmarks, id_feat = inputs.source()
    torch.cuda.synchronize()
    t0 = time.time()
    src = run.intake.source(frames, quads, labels_u8=None if run.parser is not None else labels, parser=run.parser,
                            preserve_labels=PRESERVE_MASK_SRC_FFHQ, convert_to_seg12=run.opt.seg12)
    run.source_state = prepare_source(run.model, src, landmarks_src=landmarks, id_feat=id_feat)
    torch.cuda.synchronize()
    run.source_seconds = time.time() - t0
    if run.opt.clip_cond:
        run.e_source, run.id_source = run.source_state.e_source, run.source_state.id_source


def build_run(opt, inputs, unet_config) -> Run:
    """``opt``: normalised and checked options; ``inputs``: the run's provider (scripts/inputs.py); ``unet_config``: the UNet's
    hyper-parameters.  The device is first touched by the model's move to it."""
    dev = inputs.device
    dt = torch.float16 if opt.compute_dtype == "fp16" else torch.bfloat16
    model = build_model(opt, inputs, unet_config, dt).to(dev).eval()
    run = Run(opt, dev, model)
    if opt.clip_cond and not opt.source_intake:     # :437: the source image, resized and CLIP-normalised, encoded once per clip
        source224 = inputs.source_clip_image()
        run.e_source = model.get_learned_conditioning(source224)
        if opt.arcface:     # :437 -> ddpm.py:1010: the source's identity, once per clip
            run.id_source = model.face_ID_model.extract_feats(source224)[0]
    run.sampler, run.started = build_sampler(opt, model), time.time()
    if opt.intake:
        from .intake import FrameIntake
        run.intake = FrameIntake(H=opt.H, W=opt.W, latent=run.latent, device=dev)
    if opt.parse:
        from ..pretrained.face_parsing import FaceParser
        run.parser = FaceParser(seg_ckpt=opt.faceParsing_ckpt, size=1024, device=dev, dtype=dt)
        run.parser.seg.engine      # fold and upload the weights now, not inside the first batch's `parse` stage
    if opt.source_intake:
        source_intake(run, inputs)
    if opt.raft_flow:
        run.raft = build_raft(opt, dt, dev)
    if opt.paste_back:
        from .paste_back import PasteBack
        # (--precision autocast, the reference's default: its decoded tensor is float16 and :597-608 quantise in float16)
        # (a clip from disk is rarely square: its background is resized to the frame's own (width, height), where :623
        #  swaps the two and Pillow then refuses to compose; on square frames the two are the same bits)
        run.paster = PasteBack(H=opt.H, W=opt.W, device=dev, encode_decode=run.background_round_trip,
                               half_arithmetic=opt.precision == "autocast", frame_size_order=inputs.frame_size_order)
    return run
