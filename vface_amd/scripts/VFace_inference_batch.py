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
landmarks file from disk (``scripts/clip_io.py``; dlib and the H.264 decoder stay outside, so dlib's 68 points and the decoded clip
are inputs: the ``{index}.png`` frames the reference writes at ``:285`` (read by Pillow on the host or, with ``--png_decoder gpu``,
inflated and unfiltered on the GPU: ``scripts/png_in.py``, csrc/png_in.hip), or -- ``--target_video`` -- the YUV4MPEG2 file any decoder
writes, whose I420 planes are uploaded and converted to RGB on the GPU, ``scripts/demux.py``, csrc/demux.hip), the pasted frames out
as PNG (``:636``; by Pillow on the host or, with ``--png_encoder gpu``, filtered and deflated on the GPU: ``scripts/png.py``,
csrc/png.hip) and, with ``--video_out``, as a YUV4MPEG2 file in the reference's ``yuv420p`` / BT.709 / ``tv`` range at 10 fps
(``:646-654``; ``scripts/mux.py``) or, with ``--video_codec mjpeg``, as Motion-JPEG in an AVI: a baseline JPEG encoder on the GPU
(``scripts/mjpeg.py``, csrc/mjpeg.hip), a compressed file every player opens.  H.264 and audio are not built.

    python -m vface_amd.scripts.VFace_inference_batch --target_frames clip/ --src_image src.png --landmarks clip.npz \\
        --ckpt last.ckpt --faceParsing_ckpt 79999_iter.pth --raft_ckpt raft_large.pth --video_out out.y4m

    ffmpeg -i in.mp4 -pix_fmt yuv420p clip.y4m
    python -m vface_amd.scripts.VFace_inference_batch --target_video clip.y4m --src_image src.png --landmarks clip.npz \\
        --ckpt last.ckpt --faceParsing_ckpt 79999_iter.pth --raft_ckpt raft_large.pth --video_out out.y4m

    python -m vface_amd.scripts.VFace_inference_batch --target_video clip.y4m --src_image src.png --landmarks clip.npz \\
        --ckpt last.ckpt --faceParsing_ckpt 79999_iter.pth --raft_ckpt raft_large.pth --video_out out.avi --video_codec mjpeg

    ffmpeg -i in.mp4 -c:v mjpeg -pix_fmt yuvj420p clip.avi
    python -m vface_amd.scripts.VFace_inference_batch --target_video clip.avi --src_image src.png --landmarks clip.npz \\
        --ckpt last.ckpt --faceParsing_ckpt 79999_iter.pth --raft_ckpt raft_large.pth --video_out out.avi --video_codec mjpeg

This module is the command line and nothing else: the flags (``build_parser``), their normalisation and every dependency between
them (``normalise_options``, ``check_options``), and ``run_synthetic`` / ``run_clip`` / ``main``, which put a run together from
parts that meet at plain data:

    scripts/inputs.py       what a batch is fed: ``SeededInputs`` (``--synthetic``) or ``ClipRunInputs`` (a clip), one interface
    scripts/run_setup.py    everything a run owns, built once: model and weights, sampler, intake, parser, RAFT, paste-back, source
    scripts/pipeline.py     the stages of a batch, their wall timing, the loop (``--pipeline_inversion``, ``--whole_clip``), the record
    scripts/outputs.py      the sinks: ``.pt`` / PNG of a seeded run, PNG / YUV4MPEG2 / Motion-JPEG of a clip
    scripts/checkpoint.py   reading ``last.ckpt``
"""
from __future__ import annotations

import argparse
import sys

import torch

from .checkpoint import _StubUnpickler, load_checkpoint                     # noqa: F401  (importable from here, as they always were)
from .inputs import _quad_coeffs, synthetic_intake_inputs                   # noqa: F401
from .intake import PRESERVE_MASK_SRC_FFHQ, REMOVE_MASK_TAR_FFHQ            # noqa: F401


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
    p.add_argument("--target_video", type=str, default=None,
                   help="real-clip run: the target clip as a YUV4MPEG2 file instead of --target_frames (`ffmpeg -i in.mp4 -pix_fmt yuv420p "
                        "clip.y4m`; 8-bit progressive 4:2:0, scripts/demux.py): the I420 planes are uploaded, 1.5 bytes per pixel, and "
                        "converted to RGB on the GPU (csrc/demux.hip); or as Motion-JPEG in an AVI (`ffmpeg -i in.mp4 -c:v mjpeg -pix_fmt "
                        "yuvj420p clip.avi`, or what --video_codec mjpeg wrote; baseline 4:2:0, scripts/mjpeg_in.py): the compressed scans "
                        "are uploaded and decoded on the GPU (csrc/mjpeg_in.hip).  The file's first bytes say which, not its name; frame "
                        "ids 0 .. --n_frames - 1")
    p.add_argument("--video_in_matrix", choices=["bt709", "bt601"], default=None,
                   help="with --target_video FILE.y4m: the matrix of the file, which Y4M cannot tag.  Default bt709: what --video_out writes "
                        "and HD material carries; bt601 is what an untagged swscale conversion uses.  Refused with an AVI: JFIF fixes "
                        "full-range BT.601")
    p.add_argument("--chroma_upsample", choices=["sited", "nearest"], default=None,
                   help="with --target_video: sited (default) = interpolate the chroma where the header says its samples sit "
                        "(C420jpeg: centre; C420mpeg2: left); nearest = repeat each sample over its 2 x 2 block")
    p.add_argument("--video_in_entropy", choices=["auto", "serial", "parallel"], default=None,
                   help="with --target_video FILE.avi: how the Huffman decoder spreads a frame over lanes.  serial = one lane per "
                        "restart interval; parallel = many lanes inside an interval, stitched by self-synchronisation "
                        "(csrc/jpeg_subseq.hpp); auto (default) = parallel where a restart interval is long -- files without restart markers "
                        "(ffmpeg's, Pillow's, most cameras') above all -- serial otherwise (scripts/mjpeg_in.entropy_path).  The frames "
                        "are the same bit for bit.  Refused with a .y4m")
    p.add_argument("--src_image", type=str, default=None, help="real-clip run: the source image (the identity to put in)")
    p.add_argument("--landmarks", type=str, default=None,
                   help="real-clip run: .npz with dlib's 68 points, which this build does not compute -- frames [N, 68, 2] (a NaN row = "
                        "no face found), source [68, 2], optionally crops [N, 68, 2] and source_crop [68, 2] (scripts/clip_io.py)")
    p.add_argument("--video_out", type=str, default=None,
                   help="real-clip run: write the pasted frames as a YUV4MPEG2 file (yuv420p, BT.709, tv range, 10 fps: :646-654; "
                        "scripts/mux.py) -- the hand-off to an encoder; H.264 and audio are not built -- or, with --video_codec "
                        "mjpeg, as Motion-JPEG in an AVI")
    p.add_argument("--video_codec", choices=["y4m", "mjpeg"], default=None,
                   help="with --video_out: y4m (default) = raw YUV4MPEG2; mjpeg = one baseline 4:2:0 JPEG per frame, encoded on the GPU "
                        "(csrc/mjpeg.hip), in a RIFF AVI with an index (scripts/mjpeg.py): full-range BT.601 as every MJPEG decoder "
                        "assumes, 10 fps, no audio")
    p.add_argument("--video_quality", type=int, default=None,
                   help="with --video_codec mjpeg: libjpeg's quality scale, 1..100 (default 90): the tables Pillow's quality= yields")
    p.add_argument("--png_decoder", choices=["pillow", "gpu"], default="pillow",
                   help="how the {index}.png files of --target_frames are decoded: pillow (default) = Pillow on the host, frame by "
                        "frame; gpu = the host checks each file's chunks and uploads the compressed bytes, inflate and unfilter run on "
                        "the GPU (csrc/png_in.hip, scripts/png_in.py; 8-bit RGB, RGBA and grey, not interlaced, at most 8192 pixels "
                        "wide), timed with the host's reading and checking as the batch's png_in stage.  The frames are the same bit "
                        "for bit.  Not with --target_video or --synthetic")
    p.add_argument("--png_in_inflate", choices=["auto", "serial", "parallel"], default="serial",
                   help="with --png_decoder gpu: how a file's deflate stream is inflated: serial (default) = one wave per file; parallel "
                        "= many waves per file, one per stretch of blocks that starts in a chunk of 16 KiB (csrc/png_in_par.hip), a file "
                        "whose stretches do not chain up exactly is decoded serially in the same call; auto = parallel where the mean "
                        "compressed frame exceeds scripts/png_in.PARALLEL_MIN_BODY_BYTES.  The frames are the same bit for bit")
    p.add_argument("--png_encoder", choices=["pillow", "gpu"], default="pillow",
                   help="how the pasted frames' PNGs (:636) are compressed: pillow (default) = Pillow on the host, frame by frame; gpu = "
                        "filter and deflate on the GPU (csrc/png.hip, scripts/png.py; distance-1 matches only), timed as the batch's "
                        "png_out stage.  Both are lossless and decode to the same pixels")
    p.add_argument("--gif_out", type=str, default=None,
                   help="real-clip run: write the pasted frames as an animated GIF89a (:658; 10 fps, looping, a palette of 256 per "
                        "frame), quantised and LZW-coded on the GPU (csrc/gif.hip, scripts/gif.py), timed as the batch's gif_out stage; "
                        "beside --video_out and --png_encoder, and independent of both")
    p.add_argument("--gif_seg_pixels", type=int, default=None,
                   help="with --gif_out: indices of a frame coded from an empty LZW table by one wave, 1..65535 (default "
                        "hip.GIF_SEG_PIXELS)")
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
    p.add_argument("--whole_clip", action="store_true",
                   help="process EVERY frame (a last, shorter batch where --n_frames is no multiple of --n_samples) and make "
                        "--n_samples a memory knob only: flow_fix is coupled across the batch boundaries (batch k keeps its last "
                        "frame's q|k of every step, batch k + 1 smooths its first frame with them, parallel.ClipCarry) and every "
                        "per-frame random draw is seeded by (--seed, frame, draw), so the frames written are the same for every "
                        "--n_samples.  An extension of the reference, which drops the tail frames and leaves a seam at every batch")
    return p


def load_unet_config(path):
    from ..ldm.models.diffusion.ddpm import FFHQ_UNET_CONFIG
    if path is None:
        return dict(FFHQ_UNET_CONFIG)
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    return dict(cfg["model"]["params"]["unet_config"]["params"])


def normalise_options(opt) -> argparse.Namespace:
    """A copy of ``opt`` with every attribute of ``build_parser()`` and ``return_samples`` (keep each batch's tensors in its
    record; off) present: what ``opt`` lacks -- a namespace from an older parser, or one a caller deleted from -- takes the
    parser's own default.  Everything past this function reads plain attributes."""
    full = build_parser().parse_args([])
    full.return_samples = False
    vars(full).update(vars(opt))
    return full


CLIP_STAGES = ("with_vae", "intake", "parse", "paste_back", "clip_cond", "arcface", "source_intake", "raft_flow")


def check_parse_options(opt):
    """--parse feeds the intake, and the map it makes is the parser's 512 x 512 one, which the intake takes at the sampler's size."""
    opt = normalise_options(opt)
    if not opt.parse:
        return
    if not opt.intake:
        raise SystemExit("--parse makes the label maps the intake reads: it needs --intake")
    if (opt.H, opt.W) != (512, 512):
        raise SystemExit(f"--parse needs --H 512 --W 512: the parser's label map is 512 x 512 by construction; got {opt.H} x {opt.W}")
    if opt.faceParser_name == "segnext":
        raise NotImplementedError("--faceParser_name segnext is mmseg's parser (third party); only the default BiSeNet parser is built")
    if opt.faceParser_name != "default":
        raise SystemExit(f"--faceParser_name: default | segnext; got {opt.faceParser_name!r}")


def check_source_options(opt):
    """--source_intake runs the source image through the intake's kernels and sizes."""
    opt = normalise_options(opt)
    if opt.source_intake and not opt.intake:
        raise SystemExit("--source_intake makes the source's tensors with the frame intake: it needs --intake")


def check_clip_options(opt):
    """What a real-clip run needs on its command line, checked without a GPU; switches every stage of ``CLIP_STAGES`` on (in
    ``opt`` itself)."""
    given = normalise_options(opt)
    check_video_in_options(given)
    if given.target_video and given.target_frames:
        raise SystemExit("--target_video and --target_frames both name the target clip: give one of them")
    for flag in ("target_frames", "src_image", "landmarks"):
        if not vars(given)[flag] and not (flag == "target_frames" and given.target_video):
            raise SystemExit(f"a real-clip run needs --{flag} (frames, source image and landmarks come from disk; dlib and the "
                             "video decoder are outside this build, INTEGRATION.md), or run the seeded stand-ins with --synthetic")
    for flag in ("ckpt", "faceParsing_ckpt", "raft_ckpt"):
        if given.synthetic_weights and vars(given)[flag]:
            raise SystemExit(f"--synthetic_weights seeds every model: drop --{flag}")
        if not given.synthetic_weights and not vars(given)[flag]:
            raise SystemExit(f"a real-clip run needs --{flag} (or --synthetic_weights for a run on seeded weights)")
    for name in CLIP_STAGES:
        setattr(opt, name, True)
    check_parse_options(opt)        # H x W other than 512 x 512 is refused: the parser's map


def check_video_in_options(opt):
    """--video_in_matrix, --chroma_upsample and --video_in_entropy say how --target_video is read: without it they would be ignored, so
    they are refused."""
    opt = normalise_options(opt)
    for flag in ("video_in_matrix", "chroma_upsample"):
        if vars(opt)[flag] is not None and not opt.target_video:
            raise SystemExit(f"--{flag} says how --target_video is converted: it needs --target_video FILE.y4m")
    if opt.video_in_entropy is not None and not opt.target_video:
        raise SystemExit("--video_in_entropy says how --target_video is decoded: it needs --target_video FILE.avi")


def check_video_in_reader(opt, video):
    """The flags that belong to ONE of the two readers of --target_video, once the file's first bytes have said which it is."""
    if video.fixed_matrix and opt.video_in_matrix:
        raise SystemExit(f"--video_in_matrix names the matrix of a file that cannot tag it; {opt.target_video} is Motion-JPEG, and "
                         f"JFIF fixes full-range BT.601: leave the flag out")
    if not video.fixed_matrix and opt.video_in_entropy:
        raise SystemExit(f"--video_in_entropy chooses the Huffman decoder of Motion-JPEG; {opt.target_video} is YUV4MPEG2, which has "
                         f"no entropy coding: leave the flag out")


def check_png_decoder_options(opt):
    """--png_decoder gpu says how the folder of --target_frames is read: a run that reads no such folder refuses it."""
    opt = normalise_options(opt)
    if opt.png_decoder != "gpu":
        if getattr(opt, "png_in_inflate", "serial") != "serial":
            raise SystemExit(f"--png_in_inflate {opt.png_in_inflate} says how the GPU decoder inflates: it needs --png_decoder gpu")
        return
    if opt.synthetic:
        raise SystemExit("--png_decoder gpu decodes the PNG files of --target_frames: --synthetic reads no frames from disk")
    if opt.target_video:
        raise SystemExit("--png_decoder gpu decodes the PNG files of --target_frames: --target_video reads the clip from a video file")


def check_video_out_options(opt):
    """--video_codec says how --video_out is written and --video_quality how the mjpeg codec quantises: alone they would be
    ignored, so they are refused."""
    opt = normalise_options(opt)
    if opt.video_codec is not None and not opt.video_out:
        raise SystemExit("--video_codec says how --video_out is written: it needs --video_out FILE")
    if opt.video_quality is not None:
        if opt.video_codec != "mjpeg":
            raise SystemExit("--video_quality is the quantiser of the JPEG encoder: it needs --video_codec mjpeg (y4m is lossless)")
        if not 1 <= opt.video_quality <= 100:
            raise SystemExit(f"--video_quality is libjpeg's scale, 1..100; got {opt.video_quality}")


def check_gif_out_options(opt):
    """--gif_out writes the frames of a clip; --gif_seg_pixels says how it cuts them: alone it would be ignored, so it is refused."""
    opt = normalise_options(opt)
    if opt.gif_seg_pixels is not None:
        if not opt.gif_out:
            raise SystemExit("--gif_seg_pixels says how --gif_out cuts a frame's indices: it needs --gif_out FILE")
        if not 1 <= opt.gif_seg_pixels <= 65535:
            raise SystemExit(f"--gif_seg_pixels is 1..65535 indices; got {opt.gif_seg_pixels}")
    if opt.gif_out and opt.synthetic:
        raise SystemExit("--gif_out writes the pasted frames of a real clip: --synthetic writes no clip (its sink saves tensors and "
                         "single frames)")


def check_options(opt):
    """Every dependency between flags, on normalised options, before anything is built.  Without ``--synthetic`` the run is a
    clip's: its files and checkpoints are asked for and every stage is switched on."""
    check_video_in_options(opt)
    check_video_out_options(opt)
    check_png_decoder_options(opt)
    check_gif_out_options(opt)
    if not opt.synthetic:
        check_clip_options(opt)
    if opt.intake and not opt.with_vae:
        raise SystemExit("--intake makes the pixels the VAE encodes: it needs --with_vae")
    check_parse_options(opt)
    check_source_options(opt)
    if opt.arcface and not opt.clip_cond:
        raise SystemExit("--arcface computes the identity features of the conditioning mix: it needs --clip_cond")
    if opt.paste_back and not opt.with_vae:
        raise SystemExit("--paste_back pastes decoded pixels: it needs --with_vae")
    check_whole_clip_options(opt)


def check_whole_clip_options(opt):
    """--whole_clip promises the same frames for every --n_samples: what cannot keep that promise is refused."""
    opt = normalise_options(opt)
    if not opt.whole_clip:
        return
    if opt.fusion in ("temporal", "adaIn"):
        needs = "the NEXT batch's first two frames" if opt.fusion == "temporal" else "a standard deviation over every frame of the clip"
        raise SystemExit(f"--whole_clip walks the batches one after another and --fusion {opt.fusion} needs {needs}: its frames would "
                         "still depend on --n_samples (coupled across batches: flow_fix; uncoupled modes: none, fft, replace, mix ..)")
    if opt.pipeline_inversion:
        raise SystemExit("--whole_clip and --pipeline_inversion together are not built: the carry is installed on the engine for one "
                         "loop's forwards, and --pipeline_inversion runs two loops on it at once")
    if opt.ddim_eta != 0.0:
        raise SystemExit(f"--whole_clip needs --ddim_eta 0: the sampler's noise is drawn per batch, so at --ddim_eta {opt.ddim_eta:g} "
                         "the frames would depend on --n_samples")


def _checked(opt, synthetic: bool) -> argparse.Namespace:
    opt = normalise_options(opt)
    opt.synthetic = synthetic
    check_options(opt)
    return opt


def _run(opt) -> dict:
    """``opt``: normalised and checked.  The providers, the set-up, the loop and the sinks meet here and nowhere else."""
    from . import inputs as providers, outputs
    from .pipeline import run_batches
    from .run_setup import build_run
    dev = torch.device("cuda", 0)
    if opt.synthetic:
        inputs, sink_type = providers.SeededInputs(opt, dev), outputs.SeededOutputs
    else:
        from .clip_io import ClipInputs
        if opt.target_video:
            from .mjpeg_in import open_video
            video = open_video(opt.target_video)            # by the file's first bytes: a YUV4MPEG2 file, or an AVI with an MJPG stream
            check_video_in_reader(opt, video)
            clip = ClipInputs.from_video(video, opt.src_image, opt.landmarks, opt.n_frames, opt.H, opt.W)
        elif opt.png_decoder == "gpu":
            clip = ClipInputs.from_png_folder(opt.target_frames, opt.src_image, opt.landmarks, opt.n_frames, opt.H, opt.W)
            clip.video.inflate = opt.png_in_inflate
        else:
            clip = ClipInputs(opt.target_frames, opt.src_image, opt.landmarks, opt.n_frames, opt.H, opt.W)
        inputs, sink_type = providers.ClipRunInputs(clip, opt, dev), outputs.ClipOutputs
    run = build_run(opt, inputs, load_unet_config(opt.config))
    sink = sink_type(opt)
    try:
        return run_batches(run, inputs, sink)
    finally:
        sink.close()


def run_synthetic(opt) -> dict:
    """The seeded stand-ins of ``--synthetic`` (``scripts/inputs.SeededInputs``) through the stages the flags of ``opt`` switch on.
    Returns ``{"batches": [one record per batch], "total_seconds"}``."""
    return _run(_checked(opt, synthetic=True))


def run_clip(opt) -> dict:
    """The reference's whole chain on a clip from disk (``--target_frames``, ``--src_image``, ``--landmarks``): the stages of
    ``run_synthetic`` with every widening flag on (``CLIP_STAGES``; ``--fusion`` as given), fed by ``scripts/clip_io.ClipInputs``
    instead of the seeded stand-ins -- decoded frames, quads from dlib's landmarks (``quad_from_landmarks``), the source image, the
    conditioning landmarks and ``uc = learnable_vector`` (:423).  A frame without landmarks takes the crop, label map and inverse
    transform of the frame before it and zero conditioning landmarks, and is pasted into its own frame (:297-303).  Pasted
    frames go to ``Base_dir/results/{index}.png`` (:636) unless ``--skip_save``, and to ``--video_out`` as YUV4MPEG2
    (scripts/mux.py) or, with ``--video_codec mjpeg``, as Motion-JPEG in an AVI (scripts/mjpeg.py).  Where the landmarks file has no ``crops``, the conditioning landmarks are derived from the frame points;
    that stands in for the reference's second detection on the crop and is not equal to it (scripts/clip_io.py).
    Returns the record of ``run_synthetic``; every batch also carries ``frame_ids`` and, with ``opt.return_samples``,
    ``pasted_frames``, ``crops`` and ``conditioning``."""
    return _run(_checked(opt, synthetic=False))


def main(argv=None):
    opt = build_parser().parse_args(argv)
    torch.manual_seed(opt.seed)  # seed_everything(42) (:862)
    if opt.plms:
        raise NotImplementedError("--plms selects PLMSSampler, which is outside the VFace hot path (SURVEY §2)")
    opt = _checked(opt, opt.synthetic)      # a run's arguments are checked before the GPU is asked for
    if not torch.cuda.is_available():
        sys.exit("An MI355X is required: the VFace hot path has no CPU fallback.")
    return _run(opt)


if __name__ == "__main__":
    main()


