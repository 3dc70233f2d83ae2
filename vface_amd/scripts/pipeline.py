"""The stages of a batch and the loop over batches (``REFace/scripts/VFace_inference_batch.py:413-636``).

A stage is a function of ``(run, inputs, batch)``: ``run`` is what the run owns (``scripts/run_setup.py`` ``Run``), ``inputs`` the
provider it was handed (``scripts/inputs.py``), ``batch`` the state it reads and extends.  Which stages run is decided by what
``run`` holds and the options; none of them asks what kind of provider it has.  ``prepare`` is a batch up to, not including, its
DDIM inversion; ``run_batches`` inverts, samples (beside the next batch's inversion under ``--pipeline_inversion``), decodes,
pastes, hands the batch to the output sink and appends its record.

Which frames a batch holds is ``inputs.batch_plan(opt)``; a stage reads ``batch.first`` / ``batch.count``, never ``--n_samples``.
Under ``--whole_clip`` (an extension of the reference) the plan covers every frame, ``flow_fix`` is coupled across the
batch boundaries (``parallel.ClipCarry`` in ``run.carry``, the boundary field in ``batch.boundary_flow``) and every per-frame
random draw is ``frame_noise``'s -- so the frames written do not depend on ``--n_samples``."""
from __future__ import annotations

import contextlib
import time
from dataclasses import dataclass, field
from typing import Any, Optional

import torch

from .inputs import batch_plan
from .intake import REMOVE_MASK_TAR_FFHQ, inv_transforms


class StageTimer:
    """Wall seconds of a batch's stages: ``with timer("flow"): ...`` drains the GPU on both sides and adds to ``seconds["flow"]``."""

    def __init__(self):
        self.seconds = {}

    @contextlib.contextmanager
    def __call__(self, name):
        torch.cuda.synchronize()
        t0 = time.time()
        yield
        torch.cuda.synchronize()
        self.seconds[name] = self.seconds.get(name, 0.0) + time.time() - t0

    def take_as_next(self, other: "StageTimer"):
        """``--pipeline_inversion``: the next batch's preparation runs before this batch samples, so it is this batch's wall time."""
        for name, s in other.seconds.items():
            self.seconds["next_" + name] = s
        other.seconds = {}


@dataclass
class Batch:
    id: int
    frame_ids: Optional[list]
    first: int = 0                  # the batch's frames in the clip: [first, first + count) (inputs.batch_plan)
    count: int = 0
    timer: StageTimer = field(default_factory=StageTimer)
    c: Any = None                   # conditioning tokens [F, 1, 768]; uc, tc: unconditional, and the inversion's
    uc: Any = None
    tc: Any = None
    frames: Any = None              # uint8 [F, Hs, Ws, 3] the frames pasted into, and the inverse of their crops' cut
    inv_transforms: Any = None
    crops: Any = None               # uint8 [F, 1024, 1024, 3] aligned crops (kept where the parser reads them)
    labels: Any = None              # uint8 [F, H, W] label maps
    img: Any = None                 # fp32 [F, 3, H, W] the batch's target images: the intake's, or the stand-in
    inpaint_mask: Any = None        # fp32 [F, 1, H, W]
    z_inp: Any = None               # inpaint latents, and their mask on the latent grid
    mask: Any = None
    flow: Any = None
    boundary_flow: Any = None       # --whole_clip: the field from the previous batch's last frame into this batch's frame 0
    coupled: bool = False           # ... and whether the sampler coupled flow_fix across that boundary; the bytes handed on
    carry_bytes: int = 0
    inv_store: dict = field(default_factory=dict)      # timestep -> inverted latents
    invert_kw: Optional[dict] = None                    # arguments of ddim_invert; None: nothing to invert
    inverted: bool = False
    samples: Any = None
    decoded: Any = None             # decode_first_stage(samples), and the same in [0, 1]
    pixels: Any = None
    pasted: Any = None              # uint8 [F, Hs, Ws, 3]


DRAWS = ("inpaint", "z2_tar", "paste_back")     # the per-frame posterior draws of a batch (distributions.py:23-28)


def frame_noise(seed: int, frames, draw: str, shape) -> torch.Tensor:
    """``--whole_clip``: N(0, 1) ``[len(frames), *shape]`` on the host, row j from a ``torch.Generator`` seeded by ``(seed, frames[j],
    draw)`` alone -- a frame's draw is the same whichever batch holds it and wherever it stands in that batch."""
    rows = []
    for f in frames:
        gen = torch.Generator().manual_seed(((int(seed) * 1000003 + int(f)) * len(DRAWS) + DRAWS.index(draw)) % (1 << 63))
        rows.append(torch.randn(tuple(shape), generator=gen))
    return torch.stack(rows) if rows else torch.empty((0,) + tuple(shape))


def batch_noise(run, b, draw):
    """The posterior draw ``draw`` of batch ``b``: None = torch's global generator in batch order, as the reference draws."""
    if not run.opt.whole_clip:
        return None
    return frame_noise(run.opt.seed, range(b.first, b.first + b.count), draw, (run.opt.C,) + tuple(run.latent))


def encode(run, x, noise=None):
    return run.model.get_first_stage_encoding(run.model.encode_first_stage(x), noise).detach()  # :456-457


def target_images(inputs, b):
    if b.img is None:
        b.img = inputs.images(b.id)
    return b.img


def stage_intake(run, inputs, b):
    """Frames, quads and label maps -> crops, image, inpaint image and masks; with a parser the label maps are its own (:251,
    :292-294: it sees the aligned crop, the dataset reads its map).  Returns the pixels the VAE encodes."""
    b.frames, crop_frames, quads, labels = inputs.intake_frames(b.id)
    if run.parser is None:
        with b.timer("intake"):
            b.img, inpaint_image, b.inpaint_mask, b.mask, b.inv_transforms = run.intake(b.frames, quads, labels, REMOVE_MASK_TAR_FFHQ)
        b.labels = labels
        return inpaint_image
    with b.timer("intake"):
        b.crops = run.intake.crop(crop_frames, quads)
    with b.timer("parse"):      # (a frame without landmarks takes the label map of the frame before: the provider's business)
        b.labels = inputs.carry_labels(b.id, run.parser.labels(b.crops, convert_to_seg12=run.opt.seg12))
    with b.timer("intake"):
        b.img, inpaint_image, b.inpaint_mask, b.mask = run.intake.tensors(b.crops, b.labels, REMOVE_MASK_TAR_FFHQ)
        b.inv_transforms = inv_transforms(quads, run.intake.image_size)
    return inpaint_image


def stage_latents(run, inputs, b):
    """``z_inp`` and ``mask``: from the intake's pixels, from stand-in images (``--with_vae`` alone), or stand-ins themselves."""
    if run.intake is None:
        b.mask = inputs.latent_mask(b.id)
    if not run.opt.with_vae:
        b.z_inp = inputs.latents(b.id)
        return
    pixels = stage_intake(run, inputs, b) if run.intake is not None else target_images(inputs, b)
    with b.timer("vae_encode"):
        b.z_inp = encode(run, pixels, batch_noise(run, b, "inpaint"))


def stage_conditioning(run, inputs, b):
    """:442 c = conditioning_with_feat(source, landmarks, tar = the batch's frames); :491-500 the inversion's condition takes the
    masked frames in the source's place.  E(prep(tar)) is needed by both: once per batch."""
    model, enc = run.model, run.model.cond_stage_model
    tar = target_images(inputs, b)
    keep = b.inpaint_mask if b.inpaint_mask is not None else inputs.keep_mask(b.id)
    idf, idf_t = (run.id_source, None) if run.opt.arcface else inputs.id_feats(b.id)
    lmk = inputs.landmarks(b.id)
    with b.timer("clip_cond"):
        e_tar = enc.encode_from_frames(tar)
        if run.opt.arcface:     # :442 the source's features; :500 those of the batch's masked frames, the network once per frame
            idf_t = model.face_ID_model.extract_feats_from_frames(tar, keep)[0]
        b.c = model.conditioning_with_feat(None, landmarks=lmk, id_feat=idf, e_src=run.e_source, e_tar=e_tar)
        b.tc = model.conditioning_with_feat(None, landmarks=lmk, id_feat=idf_t, e_src=enc.encode_from_frames(tar, keep), e_tar=e_tar)


def stage_flow(run, inputs, b):
    """The batch's own F - 1 fields and, under ``--whole_clip`` with a batch in front of it, the boundary field: RAFT on [the
    previous batch's last image ; this batch's images] gives F fields, the first of which is the boundary's.  RAFT's fields are
    not bit-invariant to how many pairs one call holds, so under ``--whole_clip`` every pair is a call of its own."""
    whole = run.opt.whole_clip
    if whole and run.opt.fusion != "flow_fix":
        return                      # (no other hook mode reads a flow field: `sample_kwargs` hands none over)
    if run.raft is None:
        b.flow = inputs.flow(b.id)
        if whole and b.first > 0:
            with b.timer("boundary_flow"):
                b.boundary_flow = inputs.boundary_flow(b.id)
        return
    from . import temporal_flow as tflow
    video = target_images(inputs, b)
    if not whole:
        with b.timer("flow"):       # :550-553 flow = return_flow(target frames), pixel resolution
            b.flow = tflow.return_flow(video, run.raft)
        return
    if b.first > 0:
        with b.timer("boundary_flow"):
            b.boundary_flow = tflow.return_flow(torch.cat([run.last_image, video[:1]]), run.raft)[0]
    with b.timer("flow"):
        b.flow = [tflow.return_flow(video[i:i + 2], run.raft)[0] for i in range(video.shape[0] - 1)]
    run.last_image = video[-1:].clone()


def stage_inversion_operands(run, inputs, b):
    """:531-540: invert [target ; source] (2F), hooks off; the target half is cached per timestep.  ``--no_inversion``: a seeded
    cache instead."""
    opt, F_, (h, w) = run.opt, b.count, run.latent
    if opt.no_inversion:
        run.sampler.make_schedule(opt.ddim_steps, ddim_eta=opt.ddim_eta, verbose=False)
        b.inv_store, b.inverted = inputs.inversion_cache(b.id, run.sampler.ddim_timesteps), True
        return
    if run.source_state is not None:    # :488-490, :509-525: z2_tar = encode(prior), prior = the batch's image; the source's own half
        with b.timer("vae_encode"):
            z2_tar = encode(run, b.img, batch_noise(run, b, "z2_tar"))
        z2, cond2, kw2 = run.source_state.inversion_operands(z2_tar, b.tc, b.z_inp, b.mask, cond_src=None if opt.clip_cond else b.c)
    else:
        z2, cond2 = inputs.inversion_latents(b.id), torch.cat([b.tc, b.c])
        kw2 = {"inpaint_image": torch.cat([b.z_inp, b.z_inp]), "inpaint_mask": torch.cat([b.mask, b.mask])}
    b.invert_kw = dict(x=z2, cond=cond2, S=opt.ddim_steps, shape=[opt.C, h, w], eta=opt.ddim_eta,
                       unconditional_guidance_scale=opt.scale, unconditional_conditioning=None,
                       inverse_dir=b.inv_store, batch_size=F_, test_model_kwargs=kw2, max_steps=opt.max_steps)


def prepare(run, inputs, batch_id) -> Batch:
    """Everything of a batch up to (not including) its DDIM inversion: intake, parsing, VAE encoding, conditioning, flow."""
    # (a run too short for one batch still prepares batch 0, as it always did, and then writes nothing)
    plan = run.plan if run.plan is not None else batch_plan(run.opt)
    first, count = plan[batch_id] if batch_id < len(plan) else (batch_id * run.opt.n_samples, run.opt.n_samples)
    b = Batch(batch_id, inputs.frame_ids(batch_id), first, count)
    b.c, b.uc, b.tc = inputs.tokens(batch_id)
    if b.uc is None:    # :423 uc = learnable_vector per frame
        b.uc = run.model.learnable_vector.detach().float().repeat(b.count, 1, 1)
    stage_latents(run, inputs, b)
    b.timer.seconds.update(inputs.own_seconds(batch_id))       # (device work of the provider's own, under its own stage names)
    if run.opt.clip_cond:
        stage_conditioning(run, inputs, b)
    stage_flow(run, inputs, b)
    if run.source_state is not None and batch_id == 0:
        b.timer.seconds["source_intake"] = run.source_seconds
    stage_inversion_operands(run, inputs, b)
    return b


def prepare_next(run, inputs, cur) -> Batch:
    """``--pipeline_inversion``: the batch after ``cur``, prepared before ``cur`` samples; its stages count as ``cur``'s wall time.
    Every VAE encoding draws its posterior's noise from torch's global generator, so the values follow the order of the draws:
    the one draw ``cur`` has still to make -- its paste-back's background -- is taken first, where the sequential order has it,
    and the frames stay bit-identical to that order's."""
    if run.paster is not None:
        run.paste_noise = torch.randn(run.opt.n_samples, run.opt.C, *run.latent)
    nxt = prepare(run, inputs, cur.id + 1)
    cur.timer.take_as_next(nxt.timer)
    return nxt


def sample_kwargs(run, b):
    """:541 start code = the cached latent of the second-highest timestep ("ddim_latents_961.pt" at 50 steps)."""
    opt, sampler, (h, w) = run.opt, run.sampler, run.latent
    sampler.make_schedule(opt.ddim_steps, ddim_eta=opt.ddim_eta, verbose=False)
    ts = [int(s) for s in sampler.ddim_timesteps]
    start_t = ts[-2] if ts[-2] in b.inv_store else max(b.inv_store)
    x_T = b.inv_store[start_t]
    if opt.max_steps is not None:  # smoke runs: the remaining cache entries are never read
        for s in ts:
            b.inv_store.setdefault(s, x_T)
    kw = dict(S=opt.ddim_steps, conditioning=b.c, target_conditioning=b.tc, inverse_results_dir=b.inv_store, batch_size=b.count,
              shape=[opt.C, h, w], verbose=False, unconditional_guidance_scale=opt.scale, unconditional_conditioning=b.uc,
              eta=opt.ddim_eta, x_T=x_T, flow=b.flow if opt.fusion == "flow_fix" else None,
              test_model_kwargs={"inpaint_image": b.z_inp, "inpaint_mask": b.mask}, max_steps=opt.max_steps)
    if b.coupled:
        kw.update(carry=run.carry, boundary_flow=b.boundary_flow)
    return kw


def stage_invert(run, b):
    if not b.inverted:
        with b.timer("inversion"):
            run.sampler.ddim_invert(**b.invert_kw)
        b.inverted = True


def stage_sample(run, b, nxt):
    """Sampling; with ``nxt`` (a prepared batch) its inversion runs beside it (DDIMSampler.sample_while_inverting).  Returns the
    stage's wall seconds."""
    name = "sampling" if nxt is None else "sampling_beside_next_inversion"
    b.coupled = run.carry is not None and run.opt.fusion == "flow_fix" and run.carry.world > 1
    if b.coupled:
        run.carry.begin_batch(b.id)
    with b.timer(name):
        if nxt is None:
            b.samples, _ = run.sampler.sample(**sample_kwargs(run, b))
        else:
            (b.samples, _), _ = run.sampler.sample_while_inverting(sample_kwargs(run, b), nxt.invert_kw)
            nxt.inverted = True
    if b.coupled:
        b.carry_bytes = run.carry.carry_bytes()
        run.carry.end_batch()       # (the last batch lets go of the generation it read)
    return b.timer.seconds[name]


def stage_decode(run, b):
    with b.timer("vae_decode"):
        b.decoded = run.model.decode_first_stage(b.samples)                                    # :596
        b.pixels = torch.clamp((b.decoded + 1.0) / 2.0, min=0.0, max=1.0)                      # :597


def stage_paste_back(run, inputs, b):
    """:603-633, into the frames the crops were cut from with the inverse of that cut (:68-71, :625), or into stand-ins."""
    if b.frames is None:
        b.frames, b.inv_transforms = inputs.paste_target(b.id, run.paster.canvas)
    if run.opt.whole_clip:
        run.paste_noise = batch_noise(run, b, "paste_back")
    with b.timer("paste_back"):
        b.pasted = run.paster.paste(b.decoded, b.frames, b.inv_transforms)
    return b.timer.seconds["paste_back"]


def record(run, inputs, b, sample_seconds, paste_seconds, wall_seconds) -> dict:
    keep = run.opt.return_samples
    rec = {"batch": b.id, "frames": b.count, "sample_seconds": sample_seconds, "batch_wall_seconds": wall_seconds,
           "samples": b.samples if keep else None, "labels": b.labels if keep else None,
           "inversion_cache": dict(b.inv_store) if keep else None,
           "finite": bool(torch.isfinite(b.samples).all()) and (b.pixels is None or bool(torch.isfinite(b.pixels).all())),
           "pixels": None if b.pixels is None else list(b.pixels.shape),
           "pasted": None if b.pasted is None else list(b.pasted.shape), "paste_seconds": paste_seconds,
           "stage_seconds": dict(b.timer.seconds)}
    of_the_clip = {"frame_ids": b.frame_ids, "pasted_frames": b.pasted if keep else None, "crops": b.crops if keep else None,
                   "conditioning": b.c if keep else None}
    rec.update((key, of_the_clip[key]) for key in inputs.record_keys)
    if run.opt.whole_clip:      # what the run did at this batch's front boundary, and what it keeps for the next one's
        rec.update(coupled=b.coupled and b.first > 0, carry_bytes=b.carry_bytes)
    return rec


def run_batches(run, inputs, sink) -> dict:
    opt = run.opt
    run.plan = batch_plan(opt)      # DataLoader(batch_size=n_samples, drop_last=True) (:376-382), or every frame (--whole_clip)
    nbatches = len(run.plan)
    if opt.whole_clip:
        from ..parallel import ClipCarry
        if nbatches and (run.carry is None or run.carry.batches != run.plan):      # (kept across walks of one clip: its captures are too)
            run.carry = ClipCarry(run.plan)
    # --pipeline_inversion: the DDIM inversion of batch k + 1 runs beside the sampling of batch k (the batches are independent,
    # :413, :529-553); batch 0's inversion runs alone, the last batch's sampling too
    pipelined = opt.pipeline_inversion and not opt.no_inversion and nbatches > 1
    results = []
    cur = prepare(run, inputs, 0)
    torch.cuda.synchronize()
    t_batch = time.time()       # a batch's wall time = from the previous batch's last frame to its own (its preparation included)
    for batch_id in range(nbatches):
        stage_invert(run, cur)
        nxt = prepare_next(run, inputs, cur) if pipelined and batch_id + 1 < nbatches else None
        sample_seconds = stage_sample(run, cur, nxt)
        if opt.with_vae:
            stage_decode(run, cur)
        paste_seconds = stage_paste_back(run, inputs, cur) if opt.paste_back else None
        sink.write(cur)
        torch.cuda.synchronize()
        results.append(record(run, inputs, cur, sample_seconds, paste_seconds, time.time() - t_batch))
        print(f"batch {batch_id}: {cur.count} frames sampled in {sample_seconds:.2f} s")
        t_batch = time.time()
        if nxt is None and batch_id + 1 < nbatches:
            nxt = prepare(run, inputs, batch_id + 1)
        cur = nxt
    return {"batches": results, "total_seconds": time.time() - run.started}
