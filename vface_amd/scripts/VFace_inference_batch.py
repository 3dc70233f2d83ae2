"""Entry point of the VFace path with the reference's flags (``REFace/scripts/VFace_inference_batch.py:673-860``).

What runs here is the part of ``run_inference`` that is the hot path (``:529-594``): optional DDIM inversion of
the target latents into a latent cache, then ``sampler.sample`` over batches of ``--n_samples`` frames with the
shipped hook schedule.  ``--synthetic`` stands in for everything around it in the reference -- video decoding, dlib
crop/align, face parsing, CLIP/ArcFace/landmark conditioning, the KL-VAE and paste-back (``:193-528, 596-670``) -- with
seeded synthetic latents / conditioning / flow of the right shapes and writes the denoised latents.  The widening flags
(``--with_vae``, ``--raft_flow``, ``--intake``, ``--source_intake``, ``--parse``, ``--paste_back``, ``--clip_cond``, ``--arcface``) replace one
stand-in each by the stage itself on the GPU (synthetic weights unless ``--ckpt`` covers it).

    python -m vface_amd.scripts.VFace_inference_batch --synthetic --n_frames 24 --n_samples 8 --ddim_steps 50

Without ``--synthetic`` the run is a real clip's (``run_clip``): every one of those stages, on frames, a source image and a
landmarks file from disk (``scripts/clip_io.py``; dlib and the video decoder stay outside, so the ``{index}.png`` frames the
reference writes at ``:285`` and dlib's 68 points are inputs), the pasted frames out as PNG (``:636``) and, with ``--video_out``, as
a YUV4MPEG2 file in the reference's ``yuv420p`` / BT.709 / ``tv`` range at 10 fps (``:646-654``; ``scripts/mux.py``).  H.264 and
audio are not built.

    python -m vface_amd.scripts.VFace_inference_batch --target_frames clip/ --src_image src.png --landmarks clip.npz \\
        --ckpt last.ckpt --faceParsing_ckpt 79999_iter.pth --raft_ckpt raft_large.pth --video_out out.y4m
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    # flags of the reference (same names, defaults and meaning)
    p.add_argument("--prompt", type=str, nargs="?", default="a photograph of an astronaut riding a horse")
    p.add_argument("--data_config", type=str, nargs="?", default=None, help="yaml of (video dir, source image) pairs")
    p.add_argument("--Base_dir", type=str, nargs="?", default="results_video_new", help="dir to write results to")
    p.add_argument("--skip_grid", action="store_true")
    p.add_argument("--skip_save", action="store_true")
    p.add_argument("--ddim_steps", type=int, default=50, help="number of ddim sampling steps")
    p.add_argument("--plms", action="store_true")
    p.add_argument("--laion400m", action="store_true")
    p.add_argument("--fixed_code", action="store_true")
    p.add_argument("--Start_from_target", action="store_true", default=True)
    p.add_argument("--only_target_crop", action="store_true", default=True)
    p.add_argument("--target_start_noise_t", type=int, default=1000)
    p.add_argument("--ddim_eta", type=float, default=0.0)
    p.add_argument("--n_iter", type=int, default=2)
    p.add_argument("--H", type=int, default=512)
    p.add_argument("--W", type=int, default=512)
    p.add_argument("--C", type=int, default=4, help="latent channels")
    p.add_argument("--f", type=int, default=8, help="downsampling factor")
    p.add_argument("--n_samples", type=int, default=6, help="frames per sampler batch")
    p.add_argument("--n_frames", type=int, default=24)
    p.add_argument("--n_rows", type=int, default=0)
    p.add_argument("--scale", type=float, default=3.0, help="unconditional guidance scale")
    p.add_argument("--src_image_mask", type=str, default=None)
    p.add_argument("--from-file", type=str, default=None)
    p.add_argument("--config", type=str, default=None, help="project_ffhq.yaml (UNet hyper-parameters)")
    p.add_argument("--ckpt", type=str, default=None, help="last.ckpt; its model.diffusion_model.* keys are loaded")
    p.add_argument("--ckpt_stub_unknown_globals", action="store_true",
                   help="read a pytorch_lightning last.ckpt whose non-tensor entries (callbacks, hyper_parameters) the "
                        "weights-only loader rejects: tensors through torch's own allow-list, every other pickled global as an "
                        "inert placeholder (nothing outside the allow-list is ever called)")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--rank", type=int, default=0)
    p.add_argument("--precision", type=str, choices=["full", "autocast"], default="autocast")
    # additions of this build
    p.add_argument("--synthetic", action="store_true", help="synthetic latents/conditioning/flow instead of video I/O")
    p.add_argument("--target_frames", type=str, default=None,
                   help="real-clip run: folder of the target clip's frames, {index}.png (or .jpg) as the reference writes them (:285); "
                        "taken in the order of the integer index, the first --n_frames of them")
    p.add_argument("--src_image", type=str, default=None, help="real-clip run: the source image (the identity to put in)")
    p.add_argument("--landmarks", type=str, default=None,
                   help="real-clip run: .npz with dlib's 68 points, which this build does not compute -- frames [N, 68, 2] (a NaN row = "
                        "no face found), source [68, 2], optionally crops [N, 68, 2] and source_crop [68, 2] (scripts/clip_io.py)")
    p.add_argument("--video_out", type=str, default=None,
                   help="real-clip run: write the pasted frames as a YUV4MPEG2 file (yuv420p, BT.709, tv range, 10 fps: :646-654; "
                        "scripts/mux.py) -- the hand-off to an encoder; H.264 and audio are not built")
    p.add_argument("--synthetic_weights", action="store_true",
                   help="real-clip run on seeded weights for every model (the seeds of --synthetic) instead of --ckpt, "
                        "--faceParsing_ckpt and --raft_ckpt: for tests and smoke runs")
    p.add_argument("--raft_flow", action="store_true",
                   help="compute the optical flow from the (synthetic) target frames with the RAFT-shaped producer "
                        "(temporal_flow.return_flow, VFace_inference_batch.py:550-553) instead of a synthetic field; implies "
                        "--flow_pixels.  --raft_ckpt: a raft_large state dict (torchvision layout); default synthetic weights")
    p.add_argument("--raft_ckpt", type=str, default=None)
    p.add_argument("--paste_back", action="store_true",
                   help="with --with_vae: paste the decoded crops into (synthetic) original frames on the GPU, the block of "
                        "VFace_inference_batch.py:603-636 (scripts/paste_back.py); --only_target_crop is implied")
    p.add_argument("--frame_size", type=int, default=1024, help="side of the synthetic original frames of --paste_back / --intake")
    p.add_argument("--intake", action="store_true",
                   help="with --with_vae: start from (synthetic) video frames, one quad per frame and a label map, and make the "
                        "aligned crops, the images, inpaint images and the latent mask on the GPU -- crop_faces_by_quads "
                        "(alignmengt.py:255-263), VideoDataset.__getitem_gray__ (video_swap_dataset.py:135-240) and :459 "
                        "(scripts/intake.py); with --paste_back the same frames and their inv_transforms (:68-71) are pasted into")
    p.add_argument("--parse", action="store_true",
                   help="with --intake: the label maps come from the face parser on the GPU -- faceParsing_demo on the aligned "
                        "crops (:251, :292-294; pretrained/face_parsing, vface_amd/parsing.py) -- instead of synthetic rings; needs "
                        "--H 512 --W 512, the size of the reference's map (video_swap_dataset.py:139)")
    p.add_argument("--source_intake", action="store_true",
                   help="with --intake: the source image's side runs on the GPU too -- a (synthetic) source frame and quad go through "
                        "the aligned crop, the label map (the parser's with --parse), the preserve mask, the masked 512 x 512 image, "
                        "its latents and the CLIP-normalised 224 x 224 image (:254-355, :462-468; scripts/intake.py FrameIntake.source, "
                        "scripts/source.py) once per clip, and every batch's inversion takes [target ; source] as the reference "
                        "builds it (:509-527); with --clip_cond the source's CLIP / identity features come from that image")
    p.add_argument("--faceParsing_ckpt", type=str, default=None,
                   help="face-parsing state dict (Other_dependencies/face_parsing/79999_iter.pth); default synthetic weights")
    p.add_argument("--faceParser_name", type=str, default="default", help="default (BiSeNet) | segnext (mmseg: not built)")
    p.add_argument("--seg12", default=True, action="store_true", help="12-class label maps (the reference's default)")
    p.add_argument("--with_vae", action="store_true",
                   help="synthetic run through the first-stage KL-VAE too: the inpaint latents come from encode_first_stage of "
                        "synthetic images (:456-457) and the samples are decoded to pixels (:596-600)")
    p.add_argument("--clip_cond", action="store_true",
                   help="the conditioning tokens come from the conditioning stage on the GPU -- FrozenCLIPEmbedder (ViT-L/14, mapper2) "
                        "and conditioning_with_feat (:437-442, :491-500; vface_amd/clip.py) on the batch's frames: the intake's image "
                        "and mask with --intake, seeded images otherwise -- instead of seeded N(0, 1); the ArcFace features and the "
                        "landmarks stay seeded inputs, and so does the source image unless --source_intake makes it")
    p.add_argument("--arcface", action="store_true",
                   help="with --clip_cond: the identity features of the mix come from ArcFace IR-SE50 on the GPU (IDLoss.extract_feats, "
                        "ddpm.py:91-124, :1010; vface_amd/arcface.py) -- once for the source image, once per batch for the masked "
                        "frames -- instead of seeded N(0, 1)")
    p.add_argument("--fusion", type=str, default="flow_fix", help="hook mode on the input-block attn1 modules")
    p.add_argument("--no_inversion", action="store_true", help="use random recon latents instead of DDIM inversion")
    p.add_argument("--flow_pixels", action="store_true",
                   help="hand the sampler the flow at PIXEL resolution, as the reference's return_flow produces it "
                        "(temporal_flow.py:163-188), and let it be resampled to the latent map (area mean / 8, vface_flow_to_latent) "
                        "instead of failing like the reference does (SURVEY F8)")
    p.add_argument("--flow_gate", choices=["reference", "flow_hw"], default="reference",
                   help="which attention maps the flow smoothing touches: 'reference' = exactly pnp_utils.py:201 (the 4096-token "
                        "maps of a 512x512 clip, nothing at any other resolution); 'flow_hw' = the level whose token count equals "
                        "h*w of the flow field (needed for the module to act at e.g. 768x768)")
    p.add_argument("--compute_dtype", choices=["fp16", "bf16"], default="fp16")
    p.add_argument("--hip_graph", action="store_true",
                   help="(default since round 3; kept for older command lines) replay each DDIM step's UNet forward from a "
                        "hipGraph: one capture per clip shape and hook plan, bit-equal to kernel-by-kernel launches")
    p.add_argument("--no_hip_graph", action="store_true", help="launch every kernel of a step from the host (VFACE_GRAPH=0)")
    p.add_argument("--drop_dead_branches", action="store_true",
                   help="exact dead-branch elimination (results bit-identical): sampling runs the UNet on [uncond ; cond] without "
                        "the recon third -- its x_prev is dropped by the sampler and no hook mode reads chunk 2 (ddim_w_inv.py:"
                        "667,703-707,738; pnp_utils.py:136-142,195-199,255-256) -- and the inversion runs on the target half only "
                        "(only nosie[:batch_size] is saved, ddim_w_inv.py:464-486): -33 %% / -50 %% of the UNet work")
    p.add_argument("--max_steps", type=int, default=None, help="stop after this many DDIM steps (smoke runs)")
    p.add_argument("--pipeline_inversion", action="store_true",
                   help="run the DDIM inversion of batch k + 1 beside the sampling of batch k, on two HIP streams (the batches are "
                        "independent: VFace_inference_batch.py:413, 529-553); frames bit-identical to the sequential order")
    return p


def load_unet_config(path):
    from ..ldm.models.diffusion.ddpm import FFHQ_UNET_CONFIG
    if path is None:
        return dict(FFHQ_UNET_CONFIG)
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    return dict(cfg["model"]["params"]["unet_config"]["params"])


class _StubUnpickler:
    """``pickle_module`` for ``torch.load`` of a checkpoint written by the reference's pytorch_lightning==1.4.2
    (``REFace/environment.yml``): its ``callbacks`` / ``hyper_parameters`` entries pickle CLASS objects (the ModelCheckpoint
    class as a dict key) and omegaconf containers, which ``weights_only=True`` rejects and which are not importable here.

    ``find_class`` resolves EXACTLY the (module, name) pairs of torch's own ``weights_only`` allow-list
    (``torch._weights_only_unpickler._get_allowed_globals``: the ``_rebuild_*`` helpers, storages, dtypes, ``torch.Size``,
    ``collections.OrderedDict`` ..) plus the numpy scalar / dtype reconstructors -- never a whole package: every other global,
    including every other ``torch.*`` / ``numpy.*`` / ``builtins`` name (``torch.utils.collect_env.run``, ``torch.hub.load``,
    ``numpy.load``, ``os.system`` ..), becomes an inert placeholder class whose construction, call and ``__setstate__`` do
    nothing.  No callable outside the allow-list is ever invoked (``tests/test_host_cpu.py`` feeds it hostile pickles).
    It is used only when the caller asks for it (``load_checkpoint(.., stub_unknown_globals=True)`` /
    ``--ckpt_stub_unknown_globals``), never as a silent fallback."""
    import pickle as _pickle

    _NUMPY_OK = frozenset({("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
                           ("numpy", "dtype"), ("numpy.core.multiarray", "_reconstruct"),
                           ("numpy._core.multiarray", "_reconstruct"), ("numpy", "ndarray")})
    _allowed = None

    @classmethod
    def allowed(cls) -> dict:
        if cls._allowed is None:
            from torch._weights_only_unpickler import _get_allowed_globals
            cls._allowed = dict(_get_allowed_globals())
        return cls._allowed

    class Unpickler(_pickle.Unpickler):
        _stubs: dict = {}

        def find_class(self, module, name):
            hit = _StubUnpickler.allowed().get(f"{module}.{name}")
            if hit is not None:
                return hit
            if (module, name) in _StubUnpickler._NUMPY_OK:
                return super().find_class(module, name)
            key = (module, name)
            if key not in self._stubs:
                def _new(cls, *a, **k):
                    return object.__new__(cls)
                self._stubs[key] = type(name, (), {"__module__": module, "__new__": _new, "__init__": lambda self, *a, **k: None,
                                                   "__setstate__": lambda self, st: None, "__call__": lambda self, *a, **k: None,
                                                   "append": lambda self, *a: None, "extend": lambda self, *a: None,
                                                   "__setitem__": lambda self, *a: None})
            return self._stubs[key]

    @staticmethod
    def load(f, **kw):
        return _StubUnpickler.Unpickler(f, **kw).load()

    @staticmethod
    def loads(b, **kw):
        import io
        return _StubUnpickler.Unpickler(io.BytesIO(b), **kw).load()

    __name__ = "vface_stub_pickle"


def load_checkpoint(model, path: str, with_vae: bool = False, stub_unknown_globals: bool = False) -> str:
    """Load ``last.ckpt`` of the reference (``VFace_inference_batch.py:118-135``: ``torch.load`` -> ``["state_dict"]`` ->
    ``load_state_dict(strict=False)``) into ``model``.  Only the keys of what this build runs are taken:
    ``model.diffusion_model.*`` always, ``first_stage_model.*`` when the first stage was built (``with_vae``),
    ``cond_stage_model.*`` and the projections of ``conditioning_with_feat`` when the conditioning stage was built (the text tower
    and the other entries FrozenCLIPEmbedder holds without reading are dropped); the ArcFace weights of a full LDM checkpoint
    (``face_ID_model.facenet.*``) when the identity network was built (``--arcface``), otherwise they are outside the path and ignored.  Unlike the reference's
    non-strict load, a checkpoint that does not cover every parameter of the path raises instead of silently running on
    default-initialised weights.

    The load is ``weights_only=True``.  A pytorch_lightning checkpoint carries class-keyed callback state that the safe loader
    rejects: pass ``stub_unknown_globals=True`` (``--ckpt_stub_unknown_globals``) to read it through ``_StubUnpickler`` (exact
    allow-list, inert placeholders for everything else).  There is no automatic fallback: a file that fails the safe loader
    raises, naming the flag."""
    import pickle
    if stub_unknown_globals:
        ck = torch.load(path, map_location="cpu", weights_only=False, pickle_module=_StubUnpickler)
    else:
        try:
            ck = torch.load(path, map_location="cpu", weights_only=True)
        except pickle.UnpicklingError as e:
            raise RuntimeError(
                f"{path}: the weights-only loader rejected this checkpoint ({str(e).splitlines()[0][:200]}).  If it is a "
                "pytorch_lightning checkpoint (callbacks / hyper_parameters pickle class objects), pass "
                "--ckpt_stub_unknown_globals (load_checkpoint(.., stub_unknown_globals=True)): tensors load through torch's own "
                "allow-list and every other global becomes an inert placeholder") from e
    sd = ck.get("state_dict", ck) if isinstance(ck, dict) else ck
    prefixes = ("model.diffusion_model.",) + (("first_stage_model.",) if with_vae else ())
    if hasattr(model, "cond_stage_model"):      # the conditioning stage was built: its encoder and the four projections load too
        prefixes += ("cond_stage_model.", "proj_out_source.", "proj_out_target.", "ID_proj_out.", "landmark_proj_out.", "learnable_vector")
    if hasattr(model, "face_ID_model"):
        prefixes += ("face_ID_model.facenet.",)
    taken = {k: v for k, v in sd.items() if k.startswith(prefixes) and torch.is_tensor(v)}
    if not taken:
        raise RuntimeError(f"{path}: no key starts with {prefixes} -- not an LDM checkpoint of this model "
                           f"(first keys: {list(sd)[:5]})")
    missing, unexpected = model.load_state_dict(taken, strict=False)
    hot = [k for k in missing if k.startswith(prefixes)]
    if hot or unexpected:
        raise RuntimeError(f"{path}: {len(hot)} parameter(s) of the denoising path missing (first: {hot[:5]}), "
                           f"{len(unexpected)} unexpected key(s) (first: {list(unexpected)[:5]})")
    return (f"loaded {path}: {len(taken)} tensors under {', '.join(prefixes)} matched every parameter of the path "
            f"({len(sd) - len(taken)} checkpoint entries outside it ignored)")


def _quad_coeffs(size, quad):
    """Eight PIL perspective coefficients (output pixel -> crop coordinates) that land the ``size`` x ``size`` crop on ``quad``
    (four frame-space corners, clockwise from top-left) -- what ``crop_and_align_face`` (:58-73) stores per frame."""
    import numpy as np
    src = [(0, 0), (size, 0), (size, size), (0, size)]
    A, B = [], []
    for (x, y), (u, v) in zip(quad, src):
        A += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        B += [u, v]
    return np.linalg.solve(np.array(A, float), np.array(B, float))


REMOVE_MASK_TAR_FFHQ = (1, 2, 3, 5, 6, 7, 9)      # models/REFace/configs/project_ffhq.yaml: remove_mask_tar_FFHQ
PRESERVE_MASK_SRC_FFHQ = (1, 2, 3, 5, 6, 7, 9)    # project_ffhq.yaml:217-224: preserve_mask_src_FFHQ (the source's face region)


def synthetic_intake_inputs(F_: int, S_: int, H: int, W: int, seed: int):
    """Stand-ins for what video decoding, landmark detection and face parsing hand to the intake: seeded uint8 frames
    [F, S, S, 3], one quad [4, 2] per frame (NW, SW, SE, NE; half the frame wide, rotating and drifting from frame to frame, the
    first one partly outside the frame) and a label map [F, H, W] with the parser's values 0..18 in rings round the centre."""
    import numpy as np
    gen = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (F_, S_, S_, 3), dtype=torch.uint8, generator=gen)
    quads = np.empty((F_, 4, 2), np.float64)
    for f in range(F_):
        c = np.array([S_ * (0.15 if f == 0 else 0.5) + 3.0 * f, S_ * 0.5 + 2.0 * f])
        th = 0.05 * (f + 1)
        x = S_ / 4.0 * np.array([np.cos(th), np.sin(th)])
        y = np.flipud(x) * [-1, 1]
        quads[f] = np.stack([c - x - y, c - x + y, c + x + y, c + x - y])
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    r = torch.hypot((ys - (H - 1) / 2) / (0.5 * H), (xs - (W - 1) / 2) / (0.5 * W))
    labels = torch.stack([((r * 12).long() + f) % 19 for f in range(F_)]).to(torch.uint8)
    return frames, quads, labels


def check_parse_options(opt):
    """--parse feeds the intake, and the map it makes is the parser's 512 x 512 one, which the intake takes at the sampler's size."""
    if not getattr(opt, "parse", False):
        return
    if not getattr(opt, "intake", False):
        raise SystemExit("--parse makes the label maps the intake reads: it needs --intake")
    if (opt.H, opt.W) != (512, 512):
        raise SystemExit(f"--parse needs --H 512 --W 512: the parser's label map is 512 x 512 by construction; got {opt.H} x {opt.W}")
    if opt.faceParser_name == "segnext":
        raise NotImplementedError("--faceParser_name segnext is mmseg's parser (third party); only the default BiSeNet parser is built")
    if opt.faceParser_name != "default":
        raise SystemExit(f"--faceParser_name: default | segnext; got {opt.faceParser_name!r}")


def check_source_options(opt):
    """--source_intake runs the source image through the intake's kernels and sizes."""
    if getattr(opt, "source_intake", False) and not getattr(opt, "intake", False):
        raise SystemExit("--source_intake makes the source's tensors with the frame intake: it needs --intake")


def run_synthetic(opt) -> dict:
    return _run_pipeline(opt, None)


CLIP_STAGES = ("with_vae", "intake", "parse", "paste_back", "clip_cond", "arcface", "source_intake", "raft_flow")


def run_clip(opt) -> dict:
    """The reference's whole chain on a clip from disk (``--target_frames``, ``--src_image``, ``--landmarks``): the stages of
    ``run_synthetic`` with every widening flag on (``CLIP_STAGES``; ``--fusion`` as given), fed by ``scripts/clip_io.ClipInputs``
    instead of the seeded stand-ins -- decoded frames, quads from dlib's landmarks (``quad_from_landmarks``), the source image, the
    conditioning landmarks and ``uc = learnable_vector`` (:423).  A frame without landmarks takes the crop, label map and inverse
    transform of the frame before it and zero conditioning landmarks, and is pasted into its own frame (:297-303).  Pasted
    frames go to ``Base_dir/results/{index}.png`` (:636) unless ``--skip_save``, and to ``--video_out`` as YUV4MPEG2
    (scripts/mux.py).  Where the landmarks file has no ``crops``, the conditioning landmarks are derived from the frame points;
    that stands in for the reference's second detection on the crop and is not equal to it (scripts/clip_io.py).
    Returns the record of ``run_synthetic``; every batch also carries ``frame_ids`` and, with ``opt.return_samples``,
    ``pasted_frames``, ``crops`` and ``conditioning``."""
    from .clip_io import ClipInputs
    check_clip_options(opt)
    clip = ClipInputs(opt.target_frames, opt.src_image, opt.landmarks, opt.n_frames, opt.H, opt.W)
    return _run_pipeline(opt, clip)


def check_clip_options(opt):
    """What a real-clip run needs on its command line, checked without a GPU; switches every stage of ``CLIP_STAGES`` on."""
    for flag in ("target_frames", "src_image", "landmarks"):
        if not getattr(opt, flag, None):
            raise SystemExit(f"a real-clip run needs --{flag} (frames, source image and landmarks come from disk; dlib and the "
                             "video decoder are outside this build, INTEGRATION.md), or run the seeded stand-ins with --synthetic")
    ckpts = ("ckpt", "faceParsing_ckpt", "raft_ckpt")
    if getattr(opt, "synthetic_weights", False):
        given = [f for f in ckpts if getattr(opt, f, None)]
        if given:
            raise SystemExit(f"--synthetic_weights seeds every model: drop --{given[0]}")
    else:
        for flag in ckpts:
            if not getattr(opt, flag, None):
                raise SystemExit(f"a real-clip run needs --{flag} (or --synthetic_weights for a run on seeded weights)")
    for name in CLIP_STAGES:
        setattr(opt, name, True)
    check_parse_options(opt)        # H x W other than 512 x 512 is refused: the parser's map


def _run_pipeline(opt, clip) -> dict:
    """``clip``: None = the seeded stand-ins of ``--synthetic``; a ``clip_io.ClipInputs`` = frames, quads, landmarks and source from
    disk.  The stages are the same code either way."""
    from ..ldm.models.diffusion.ddim_w_inv import DDIMSampler, HookPlan
    from ..ldm.models.diffusion.ddpm import LatentDiffusion
    from ..utils import synth

    if getattr(opt, "intake", False) and not opt.with_vae:
        raise SystemExit("--intake makes the pixels the VAE encodes: it needs --with_vae")
    check_parse_options(opt)
    check_source_options(opt)
    source_intake = bool(getattr(opt, "source_intake", False))
    dev = torch.device("cuda", 0)
    dt = torch.float16 if opt.compute_dtype == "fp16" else torch.bfloat16
    cfg = load_unet_config(opt.config)
    cfg["compute_dtype"] = dt
    clip_cond = bool(getattr(opt, "clip_cond", False))
    arcface = bool(getattr(opt, "arcface", False))
    if arcface and not clip_cond:
        raise SystemExit("--arcface computes the identity features of the conditioning mix: it needs --clip_cond")
    stage_kw = dict(cond_stage_config=dict(params=dict(compute_dtype=dt), **(dict(other_params=dict(arcface=True)) if arcface else {}))) \
        if clip_cond else {}
    if opt.with_vae:
        from ..ldm.models.autoencoder import FFHQ_VAE_CONFIG
        model = LatentDiffusion(cfg, first_stage_config=dict(FFHQ_VAE_CONFIG, compute_dtype=dt), **stage_kw)
    else:
        model = LatentDiffusion(cfg, **stage_kw)
    if opt.ckpt:
        print(load_checkpoint(model, opt.ckpt, with_vae=opt.with_vae, stub_unknown_globals=opt.ckpt_stub_unknown_globals))
    else:
        synth.fill_module_(model.unet, seed=0)
        if opt.with_vae:
            synth.fill_module_(model.first_stage_model, seed=0, prefix="vae.")
    if clip_cond and not opt.ckpt:
        synth.fill_module_(model.cond_stage_model, seed=5)
        for name in ("proj_out_source", "proj_out_target", "ID_proj_out", "landmark_proj_out"):
            synth.fill_module_(getattr(model, name), seed=5, prefix=name + ".")
        if arcface:
            synth.fill_arcface_(model.face_ID_model.facenet, seed=5, prefix="face_ID_model.facenet.")
        if clip is not None:    # (read as `uc` below; a --synthetic run draws its `uc` per batch and leaves the module's own draw)
            model.learnable_vector.data.copy_(synth.synth_normal("cli.learnable_vector", (1, 1, 768)))
    model = model.to(dev).eval()
    e_source, id_source = None, None
    if clip_cond and not source_intake:       # :437: the source image, resized and CLIP-normalised, is encoded once per clip and broadcast
        source224 = synth.synth_normal("cli.source224", (1, 3, 224, 224)).to(dev)
        e_source = model.get_learned_conditioning(source224)
        if arcface:     # :437 -> ddpm.py:1010: the source's identity, once per clip
            id_source = model.face_ID_model.extract_feats(source224)[0]
    sampler = DDIMSampler(model)
    sampler.hook_plan = HookPlan(fusion=opt.fusion, enabled=opt.fusion != "none")
    sampler.flow_gate = opt.flow_gate
    sampler.drop_dead_branches = bool(opt.drop_dead_branches)
    if opt.hip_graph:
        sampler.model.model.diffusion_model.engine.use_graph = True
    if opt.no_hip_graph:
        sampler.model.model.diffusion_model.engine.use_graph = False
    sampler.flow_resample = "area" if opt.flow_pixels else None
    h, w = opt.H // opt.f, opt.W // opt.f
    F_ = opt.n_samples
    os.makedirs(opt.Base_dir, exist_ok=True)
    results, t_all = [], time.time()
    paster, raft, writer = None, None, None
    intake = None
    if getattr(opt, "intake", False):
        from .intake import FrameIntake
        intake = FrameIntake(H=opt.H, W=opt.W, latent=(h, w), device=dev)
    parser = None
    if getattr(opt, "parse", False):
        from ..pretrained.face_parsing import FaceParser
        parser = FaceParser(seg_ckpt=opt.faceParsing_ckpt, size=1024, device=dev, dtype=dt)
        parser.seg.engine      # fold and upload the weights now, not inside the first batch's `parse` stage
    source_state, source_seconds = None, None
    if source_intake:       # :254-355, :436-438, :462-468: once per clip; a seeded frame and quad stand in for the photo and dlib
        from .source import prepare_source
        if clip is not None:    # the photo, its quad from dlib's points, its landmarks on the crop; the label map is the parser's
            src_frames, src_quads, src_labels = clip.source_u8, clip.source_quad, None
            src_lmk = torch.from_numpy(clip.source_landmarks).to(dev)
        else:
            src_frames, src_quads, src_labels = synthetic_intake_inputs(1, opt.frame_size, opt.H, opt.W, opt.seed + 500)
            src_lmk = synth.synth_normal("cli.landmarks_src", (1, 136)).to(dev) * 0.1 + 0.5
        src_id = None if arcface else synth.synth_normal("cli.id_feat_src", (1, 512)).to(dev)
        src_frames, src_labels = src_frames.to(dev), None if src_labels is None else src_labels.to(dev)
        torch.cuda.synchronize()
        ts_ = time.time()
        src = intake.source(src_frames, src_quads, labels_u8=None if parser is not None else src_labels, parser=parser,
                            preserve_labels=PRESERVE_MASK_SRC_FFHQ, convert_to_seg12=opt.seg12)
        source_state = prepare_source(model, src, landmarks_src=src_lmk, id_feat=src_id)
        torch.cuda.synchronize()
        source_seconds = time.time() - ts_
        if clip_cond:
            e_source, id_source = source_state.e_source, source_state.id_source
    nbatches = opt.n_frames // F_       # DataLoader(batch_size=n_samples, drop_last=True) (:376-382)
    # --pipeline_inversion: the DDIM inversion of batch k + 1 runs beside the sampling of batch k (DDIMSampler.sample_while_inverting:
    # the batches are independent, :413, :529-553); batch 0's inversion runs alone, the last batch's sampling too
    pipelined = bool(getattr(opt, "pipeline_inversion", False)) and not opt.no_inversion and nbatches > 1

    def stage(stages, name, t_start):      # wall seconds of a pipeline stage, GPU drained on both sides
        torch.cuda.synchronize()
        stages[name] = stages.get(name, 0.0) + time.time() - t_start
        return time.time()

    carried = {}        # what a clip's batch hands to the next: the last frame's label map

    def prepare(batch_id):
        """Everything of a batch up to (not including) its DDIM inversion: conditioning, VAE encoding, flow."""
        nonlocal raft
        tag = lambda s: f"cli.{s}.{batch_id}"
        d = lambda t: t.to(dev)
        stages = {}
        img, frames, inv_tf, labels, inpaint_mask, crops, given = None, None, None, None, None, None, None
        if clip is not None:    # :423 uc = learnable_vector per frame; c and tc come from the conditioning stage below
            given = clip.batch(batch_id, F_)
            uc = model.learnable_vector.detach().float().repeat(F_, 1, 1)
            c = tc = None
        else:
            c, uc, tc = (d(synth.synth_normal(tag(k), (F_, 1, 768))) for k in ("c", "uc", "tc"))
        if intake is not None:
            if given is not None:       # a frame without landmarks is cut with the quad, and from the pixels, of the frame it takes
                frames, crop_frames, quads, labels = d(given["frames"]), d(given["crop_frames"]), given["quads"], None
            else:
                frames, quads, labels = synthetic_intake_inputs(F_, opt.frame_size, opt.H, opt.W, opt.seed + 1000 + batch_id)
                frames, labels = d(frames), d(labels)
                crop_frames = frames
            ts_ = stage(stages, "_", time.time())
            if parser is not None:      # :251, :292-294: the parser sees the aligned crop, the dataset reads its map
                from .intake import inv_transforms
                crops = intake.crop(crop_frames, quads)
                ts_ = stage(stages, "intake", ts_)
                labels = parser.labels(crops, convert_to_seg12=opt.seg12)
                if given is not None:   # :297-303: no landmarks = the label map of the frame before, across a batch boundary too
                    for f in range(F_):
                        if not given["found"][f]:
                            labels[f] = labels[f - 1] if f else carried["labels"]
                    carried["labels"] = labels[-1].clone()
                ts_ = stage(stages, "parse", ts_)
                img, inpaint_image, inpaint_mask, mask = intake.tensors(crops, labels, REMOVE_MASK_TAR_FFHQ)
                inv_tf = inv_transforms(quads, intake.image_size)
            else:
                img, inpaint_image, inpaint_mask, mask, inv_tf = intake(frames, quads, labels, REMOVE_MASK_TAR_FFHQ)
            ts_ = stage(stages, "intake", ts_)
            z_inp = model.get_first_stage_encoding(model.encode_first_stage(inpaint_image)).detach()     # :456-457
            stage(stages, "vae_encode", ts_)
        elif opt.with_vae:
            img = d(torch.stack([synth.synth_normal(tag(f"img{f}"), (3, opt.H, opt.W)).clamp(-1, 1) for f in range(F_)]))
            ts_ = stage(stages, "_", time.time())
            z_inp = model.get_first_stage_encoding(model.encode_first_stage(img)).detach()       # :456-457
            stage(stages, "vae_encode", ts_)
        else:
            z_inp = d(synth.synth_normal(tag("inp"), (F_, opt.C, h, w)) * 0.18215)
        if intake is None:
            mask = d(synth.synth_mask(F_, h, w))
        if clip_cond:
            # :442 c = conditioning_with_feat(source, landmarks, tar = the batch's frames); :491-500 the inversion's condition takes
            # the masked frames in the source's place.  E(prep(tar)) is needed by both: once per batch
            tar = img if img is not None else d(torch.stack([synth.synth_normal(tag(f"img{f}"), (3, opt.H, opt.W)).clamp(-1, 1)
                                                             for f in range(F_)]))
            keep = inpaint_mask if inpaint_mask is not None else d(synth.synth_mask(F_, opt.H, opt.W))
            idf, idf_t = (d(synth.synth_normal(tag(k), (F_, 512))) for k in ("id_feat", "id_feat_tar"))
            lmk = d(synth.synth_normal(tag("landmarks"), (F_, 136)) * 0.1 + 0.5)
            if given is not None:       # ddpm.py:1068-1099: the points on the crop, in pixels; zeros where no face was found
                lmk = d(torch.from_numpy(given["landmarks"]))
            ts_ = stage(stages, "_", time.time())
            enc = model.cond_stage_model
            e_tar = enc.encode_from_frames(tar)
            if arcface:     # :442 the source's features; :500 those of the batch's masked frames, the network once per frame
                idf, idf_t = id_source, model.face_ID_model.extract_feats_from_frames(tar, keep)[0]
            c = model.conditioning_with_feat(None, landmarks=lmk, id_feat=idf, e_src=e_source, e_tar=e_tar)
            tc = model.conditioning_with_feat(None, landmarks=lmk, id_feat=idf_t, e_src=enc.encode_from_frames(tar, keep), e_tar=e_tar)
            stage(stages, "clip_cond", ts_)
        if opt.raft_flow:     # :550-553 flow = return_flow(target frames), pixel resolution
            from . import temporal_flow as tflow
            if raft is None:
                from ..raft import RAFT
                raft = RAFT(compute_dtype=dt)
                if opt.raft_ckpt:
                    raft.load_state_dict(torch.load(opt.raft_ckpt, map_location="cpu", weights_only=True))
                else:
                    synth.fill_module_(raft, seed=0, prefix="raft.")
                raft = raft.to(dev).eval()
            video = img if opt.with_vae else d(torch.stack([synth.synth_normal(tag(f"img{f}"), (3, opt.H, opt.W)).clamp(-1, 1)
                                                            for f in range(F_)]))
            ts_ = stage(stages, "_", time.time())
            flow = tflow.return_flow(video, raft)
            stage(stages, "flow", ts_)
            sampler.flow_resample = "area"
        elif opt.flow_pixels:   # a pixel-resolution field whose latent resample is a +-2-cell motion
            flow = [f[None] * opt.f for f in synth.synth_flow(F_ - 1, opt.H, opt.W, seed=opt.seed + batch_id)]
        else:
            flow = [f[None] for f in synth.synth_flow(F_ - 1, h, w, seed=opt.seed + batch_id)]
        inv_store = {}
        invert_kw = None
        if source_state is not None and batch_id == 0:
            stages["source_intake"] = source_seconds
        if opt.no_inversion:
            sampler.make_schedule(opt.ddim_steps, ddim_eta=opt.ddim_eta, verbose=False)
            for s in sampler.ddim_timesteps:
                inv_store[int(s)] = d(synth.synth_normal(tag(f"inv{int(s)}"), (F_, opt.C, h, w)))
        else:
            # :531-540: invert [target ; source] (2F), hooks off; the target half is cached per timestep
            if source_state is not None:    # :488-490, :509-525: z2_tar = encode(prior), prior = the batch's image; the source's own half
                ts_ = stage(stages, "_", time.time())
                z2_tar = model.get_first_stage_encoding(model.encode_first_stage(img)).detach()
                stage(stages, "vae_encode", ts_)
                z2, cond2, kw2 = source_state.inversion_operands(z2_tar, tc, z_inp, mask, cond_src=None if clip_cond else c)
            else:
                z2 = d(synth.synth_normal(tag("z2"), (2 * F_, opt.C, h, w)))
                cond2 = torch.cat([tc, c])
                kw2 = {"inpaint_image": torch.cat([z_inp, z_inp]), "inpaint_mask": torch.cat([mask, mask])}
            invert_kw = dict(x=z2, cond=cond2, S=opt.ddim_steps, shape=[opt.C, h, w], eta=opt.ddim_eta,
                             unconditional_guidance_scale=opt.scale, unconditional_conditioning=None,
                             inverse_dir=inv_store, batch_size=F_, test_model_kwargs=kw2, max_steps=opt.max_steps)
        return {"id": batch_id, "c": c, "uc": uc, "tc": tc, "z_inp": z_inp, "mask": mask, "flow": flow, "inv_store": inv_store,
                "invert_kw": invert_kw, "inverted": invert_kw is None, "stages": stages, "frames": frames, "inv_transforms": inv_tf,
                "labels": labels, "crops": crops, "frame_ids": None if given is None else given["frame_ids"]}

    def sample_kwargs(b):
        # :541 start code = the cached latent of the second-highest timestep ("ddim_latents_961.pt" at 50 steps)
        sampler.make_schedule(opt.ddim_steps, ddim_eta=opt.ddim_eta, verbose=False)
        ts = [int(s) for s in sampler.ddim_timesteps]
        inv_store = b["inv_store"]
        start_t = ts[-2] if ts[-2] in inv_store else max(inv_store)
        x_T = inv_store[start_t]
        if opt.max_steps is not None:  # smoke runs: the remaining cache entries are never read
            for s in ts:
                inv_store.setdefault(s, x_T)
        return dict(S=opt.ddim_steps, conditioning=b["c"], target_conditioning=b["tc"], inverse_results_dir=inv_store, batch_size=F_,
                    shape=[opt.C, h, w], verbose=False, unconditional_guidance_scale=opt.scale, unconditional_conditioning=b["uc"],
                    eta=opt.ddim_eta, x_T=x_T, flow=b["flow"] if opt.fusion == "flow_fix" else None,
                    test_model_kwargs={"inpaint_image": b["z_inp"], "inpaint_mask": b["mask"]}, max_steps=opt.max_steps)

    cur = prepare(0)
    torch.cuda.synchronize()
    t_batch = time.time()       # a batch's wall time = from the previous batch's last frame to its own (its preparation included)
    for batch_id in range(nbatches):
        stages = cur["stages"]
        if not cur["inverted"]:
            ts_ = stage(stages, "_", time.time())
            sampler.ddim_invert(**cur["invert_kw"])
            stage(stages, "inversion", ts_)
            cur["inverted"] = True
        nxt = prepare(batch_id + 1) if (pipelined and batch_id + 1 < nbatches) else None
        if nxt is not None:                      # (its encoding / flow are this batch's wall time: they run before this batch samples)
            for k, v in nxt["stages"].items():
                if k != "_":
                    stages["next_" + k] = v
            nxt["stages"] = {}
        torch.cuda.synchronize()
        t0 = time.time()
        if nxt is not None:
            (samples, _), _ = sampler.sample_while_inverting(sample_kwargs(cur), nxt["invert_kw"])
            nxt["inverted"] = True
        else:
            samples, _ = sampler.sample(**sample_kwargs(cur))
        torch.cuda.synchronize()
        dt_s = time.time() - t0
        stages["sampling" if nxt is None else "sampling_beside_next_inversion"] = dt_s
        pixels = None
        if opt.with_vae:
            ts_ = time.time()
            x_samples = model.decode_first_stage(samples)                                          # :596
            pixels = torch.clamp((x_samples + 1.0) / 2.0, min=0.0, max=1.0)                       # :597
            stage(stages, "vae_decode", ts_)
        pasted, paste_s = None, None
        if opt.paste_back:
            if not opt.with_vae:
                raise SystemExit("--paste_back pastes decoded pixels: it needs --with_vae")
            from .paste_back import PasteBack
            if paster is None:
                # (--precision autocast, the reference's default: its decoded tensor is float16 and :597-608 quantise in float16)
                # (a clip from disk is rarely square: its background is resized to the frame's own (width, height), where :623
                #  swaps the two and Pillow then refuses to compose; on square frames the two are the same bits)
                paster = PasteBack(H=opt.H, W=opt.W, device=dev, encode_decode=PasteBack.vae_round_trip(model),
                                   half_arithmetic=opt.precision == "autocast",
                                   frame_size_order="reference" if clip is None else "width_height")
            if intake is not None:      # the frames the crops were cut from and the inverse of that cut (:68-71, :625)
                frames, co = cur["frames"], cur["inv_transforms"]
            else:
                S_ = opt.frame_size
                gen = torch.Generator().manual_seed(opt.seed + 1000 + batch_id)
                frames = torch.randint(0, 256, (F_, S_, S_, 3), dtype=torch.uint8, generator=gen).to(dev)
                # inv_transforms_all rows (:625): here the 1024 canvas lands on the central half of the frame, slightly sheared
                q = S_ / 4.0
                co = [_quad_coeffs(paster.canvas, [(q + 3 * f, q), (3 * q, q + f), (3 * q - f, 3 * q), (q, 3 * q - 2 * f)])
                      for f in range(F_)]
            torch.cuda.synchronize()
            t1 = time.time()
            pasted = paster.paste(x_samples, frames, co)                                           # :603-633
            torch.cuda.synchronize()
            paste_s = time.time() - t1
            stages["paste_back"] = paste_s
        if clip is not None:
            if getattr(opt, "video_out", None):      # :646-654: yuv420p, BT.709, tv range, 10 fps; in frame order
                if writer is None:
                    from .mux import Y4MWriter
                    writer = Y4MWriter(opt.video_out, pasted.shape[2], pasted.shape[1])
                ts_ = stage(stages, "_", time.time())
                writer.write(pasted)
                stage(stages, "video_out", ts_)
            if not opt.skip_save:
                from PIL import Image
                os.makedirs(os.path.join(opt.Base_dir, "results"), exist_ok=True)
                for f, index in enumerate(cur["frame_ids"]):                                       # :636
                    Image.fromarray(pasted[f].cpu().numpy()).save(os.path.join(opt.Base_dir, "results", f"{index}.png"))
        elif not opt.skip_save:
            if pasted is not None:
                from PIL import Image
                for f in range(F_):                                                                # :636
                    Image.fromarray(pasted[f].cpu().numpy()).save(os.path.join(opt.Base_dir, f"pasted_b{batch_id}_f{f}.png"))
            torch.save(samples.cpu(), os.path.join(opt.Base_dir, f"samples_batch{batch_id}.pt"))
            if pixels is not None:
                torch.save(pixels.cpu(), os.path.join(opt.Base_dir, f"pixels_batch{batch_id}.pt"))
        torch.cuda.synchronize()
        results.append({"batch": batch_id, "frames": F_, "sample_seconds": dt_s, "batch_wall_seconds": time.time() - t_batch,
                        "samples": samples if getattr(opt, "return_samples", False) else None,
                        "labels": cur["labels"] if getattr(opt, "return_samples", False) else None,
                        "inversion_cache": dict(cur["inv_store"]) if getattr(opt, "return_samples", False) else None,
                        "finite": bool(torch.isfinite(samples).all()) and (pixels is None or bool(torch.isfinite(pixels).all())),
                        "pixels": None if pixels is None else list(pixels.shape),
                        "pasted": None if pasted is None else list(pasted.shape), "paste_seconds": paste_s,
                        "stage_seconds": {k: v for k, v in stages.items() if k != "_"}})
        if clip is not None:
            keep = bool(getattr(opt, "return_samples", False))
            results[-1].update(frame_ids=list(cur["frame_ids"]), pasted_frames=pasted if keep else None,
                               crops=cur["crops"] if keep else None, conditioning=cur["c"] if keep else None)
        print(f"batch {batch_id}: {F_} frames sampled in {dt_s:.2f} s")
        t_batch = time.time()
        cur = nxt if nxt is not None else (prepare(batch_id + 1) if batch_id + 1 < nbatches else None)
    if writer is not None:
        writer.close()
    return {"batches": results, "total_seconds": time.time() - t_all}


def main(argv=None):
    opt = build_parser().parse_args(argv)
    torch.manual_seed(opt.seed)  # seed_everything(42) (:862)
    if opt.plms:
        raise NotImplementedError("--plms selects PLMSSampler, which is outside the VFace hot path (SURVEY §2)")
    if not opt.synthetic:       # a clip from disk; its arguments are checked before the GPU is asked for
        check_clip_options(opt)
        if not torch.cuda.is_available():
            sys.exit("An MI355X is required: the VFace hot path has no CPU fallback.")
        return run_clip(opt)
    check_parse_options(opt)
    check_source_options(opt)
    if not torch.cuda.is_available():
        sys.exit("An MI355X is required: the VFace hot path has no CPU fallback.")
    return run_synthetic(opt)


if __name__ == "__main__":
    main()
