"""The command line's parts that need no GPU: options normalised once, every flag dependency in `check_options`, and the two input
providers of vface_amd/scripts/inputs.py behind their one interface."""
import argparse

import numpy as np
import pytest
import torch
from PIL import Image

from test_clip_io_cpu import landmark_file, write_frames
from vface_amd.scripts import VFace_inference_batch as cli
from vface_amd.scripts import clip_io
from vface_amd.scripts.inputs import ClipRunInputs, SeededInputs, _quad_coeffs, synthetic_intake_inputs
from vface_amd.utils import synth


def options(*args):
    return cli.normalise_options(cli.build_parser().parse_args(list(args)))


def test_normalising_fills_what_is_missing_from_the_parsers_defaults():
    defaults = cli.build_parser().parse_args([])
    opt = cli.build_parser().parse_args(["--synthetic", "--n_frames", "7", "--fusion", "none"])
    gone = ("intake", "source_intake", "pipeline_inversion", "video_out", "frame_size", "seg12", "faceParser_name")
    for name in gone:
        delattr(opt, name)
    full = cli.normalise_options(opt)
    assert set(vars(full)) == set(vars(defaults)) | {"return_samples"} and full.return_samples is False
    for name in gone:
        assert getattr(full, name) == getattr(defaults, name), name
    assert full is not opt and not hasattr(opt, "intake")                   # a copy: the caller's namespace is as it was
    assert vars(cli.normalise_options(argparse.Namespace())) == dict(vars(defaults), return_samples=False)


def test_normalising_leaves_given_values_alone():
    opt = cli.build_parser().parse_args(["--synthetic", "--intake", "--frame_size", "320", "--n_samples", "3", "--video_out", "o.y4m",
                                         "--compute_dtype", "bf16", "--max_steps", "2"])
    opt.return_samples = True
    assert vars(cli.normalise_options(opt)) == vars(opt)
    del opt.parse
    full = cli.normalise_options(opt)
    assert (full.intake, full.frame_size, full.n_samples, full.video_out, full.compute_dtype, full.max_steps, full.return_samples,
            full.parse) == (True, 320, 3, "o.y4m", "bf16", 2, True, False)


CLIP = ("--target_frames", "d", "--src_image", "s.png", "--landmarks", "l.npz")


@pytest.mark.parametrize("args, error, message", [
    (("--synthetic", "--with_vae", "--parse"), SystemExit, "--parse makes the label maps the intake reads: it needs --intake"),
    (("--synthetic", "--with_vae", "--intake", "--parse", "--H", "256", "--W", "256"), SystemExit,
     "--parse needs --H 512 --W 512: the parser's label map is 512 x 512 by construction; got 256 x 256"),
    (("--synthetic", "--with_vae", "--intake", "--parse", "--faceParser_name", "segnext"), NotImplementedError, "segnext is mmseg's parser"),
    (("--synthetic", "--with_vae", "--intake", "--parse", "--faceParser_name", "other"), SystemExit, "--faceParser_name: default | segnext; got 'other'"),
    (("--synthetic", "--with_vae", "--source_intake"), SystemExit,
     "--source_intake makes the source's tensors with the frame intake: it needs --intake"),
    (("--synthetic", "--intake"), SystemExit, "--intake makes the pixels the VAE encodes: it needs --with_vae"),
    (("--synthetic", "--arcface"), SystemExit, "--arcface computes the identity features of the conditioning mix: it needs --clip_cond"),
    (("--synthetic", "--paste_back"), SystemExit, "--paste_back pastes decoded pixels: it needs --with_vae"),
    ((), SystemExit, "a real-clip run needs --target_frames (frames, source image and landmarks come from disk"),
    (CLIP[:2] + CLIP[4:], SystemExit, "a real-clip run needs --src_image"),
    (CLIP[:4], SystemExit, "a real-clip run needs --landmarks"),
    (CLIP, SystemExit, "a real-clip run needs --ckpt (or --synthetic_weights for a run on seeded weights)"),
    (CLIP + ("--ckpt", "a.ckpt", "--raft_ckpt", "r.pth"), SystemExit, "a real-clip run needs --faceParsing_ckpt"),
    (CLIP + ("--ckpt", "a.ckpt", "--faceParsing_ckpt", "p.pth"), SystemExit, "a real-clip run needs --raft_ckpt"),
    (CLIP + ("--synthetic_weights", "--raft_ckpt", "r.pth"), SystemExit, "--synthetic_weights seeds every model: drop --raft_ckpt"),
    (CLIP + ("--synthetic_weights", "--H", "256", "--W", "256"), SystemExit, "--parse needs --H 512 --W 512"),
])
def test_check_options_raises_each_dependency(args, error, message):
    with pytest.raises(error) as e:
        cli.check_options(options(*args))
    assert message in str(e.value)


def test_check_options_passes_and_switches_a_clips_stages_on():
    for args in (("--synthetic",), ("--synthetic", "--with_vae", "--intake", "--parse", "--source_intake", "--clip_cond", "--arcface",
                                    "--raft_flow", "--paste_back")):
        cli.check_options(options(*args))
    opt = options(*CLIP, "--synthetic_weights")
    cli.check_options(opt)
    assert all(getattr(opt, name) for name in cli.CLIP_STAGES)
    with pytest.raises(SystemExit, match="--paste_back pastes decoded pixels"):      # before anything is built: no GPU is asked for
        cli.run_synthetic(cli.build_parser().parse_args(["--synthetic", "--paste_back"]))


@pytest.mark.parametrize("k", [0, 3])
def test_seeded_provider_equals_the_expressions_it_replaced(k):
    """Batch k of 2 frames at 64 x 64 (8 x 8 latents), 96 x 96 original frames: every tag, seed offset and host-side expression."""
    F_, H, W, h, w, S_, seed = 2, 64, 64, 8, 8, 96, 7
    opt = options("--synthetic", "--n_samples", "2", "--H", "64", "--W", "64", "--frame_size", "96", "--seed", "7", "--ddim_steps", "4")
    p = SeededInputs(opt, "cpu")
    tag = lambda s: f"cli.{s}.{k}"
    eq = lambda got, want: got.dtype == want.dtype and torch.equal(got, want)
    assert p.frame_ids(k) is None and p.inherits(k) == [False, False] and p.learnable_vector() is None and p.record_keys == ()
    for got, name in zip(p.tokens(k), ("c", "uc", "tc")):
        assert eq(got, synth.synth_normal(tag(name), (F_, 1, 768))), name
    frames, quads, labels = synthetic_intake_inputs(F_, S_, H, W, seed + 1000 + k)
    got = p.intake_frames(k)
    assert eq(got[0], frames) and got[1] is got[0] and np.array_equal(got[2], quads) and eq(got[3], labels)
    assert p.carry_labels(k, labels) is labels
    img = torch.stack([synth.synth_normal(tag(f"img{f}"), (3, H, W)).clamp(-1, 1) for f in range(F_)])
    assert eq(p.images(k), img)
    assert eq(p.latents(k), synth.synth_normal(tag("inp"), (F_, 4, h, w)) * 0.18215)
    assert eq(p.latent_mask(k), synth.synth_mask(F_, h, w)) and eq(p.keep_mask(k), synth.synth_mask(F_, H, W))
    for got, name in zip(p.id_feats(k), ("id_feat", "id_feat_tar")):
        assert eq(got, synth.synth_normal(tag(name), (F_, 512))), name
    assert eq(p.landmarks(k), synth.synth_normal(tag("landmarks"), (F_, 136)) * 0.1 + 0.5)
    assert all(eq(a, b[None]) for a, b in zip(p.flow(k), synth.synth_flow(F_ - 1, h, w, seed=seed + k))) and len(p.flow(k)) == F_ - 1
    opt.flow_pixels = True
    assert all(eq(a, b[None] * 8) for a, b in zip(p.flow(k), synth.synth_flow(F_ - 1, H, W, seed=seed + k)))
    cache = p.inversion_cache(k, torch.tensor([1, 251, 501, 751]))
    assert sorted(cache) == [1, 251, 501, 751] and all(eq(cache[s], synth.synth_normal(tag(f"inv{s}"), (F_, 4, h, w))) for s in cache)
    assert eq(p.inversion_latents(k), synth.synth_normal(tag("z2"), (2 * F_, 4, h, w)))
    got_frames, got_co = p.paste_target(k, 1024)
    q = S_ / 4.0
    assert eq(got_frames, torch.randint(0, 256, (F_, S_, S_, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed + 1000 + k)))
    for f in range(F_):
        assert np.array_equal(got_co[f], _quad_coeffs(1024, [(q + 3 * f, q), (3 * q, q + f), (3 * q - f, 3 * q), (q, 3 * q - 2 * f)]))
    src = p.source()
    frames, quads, labels = synthetic_intake_inputs(1, S_, H, W, seed + 500)
    assert eq(src[0], frames) and np.array_equal(src[1], quads) and eq(src[2], labels)
    assert eq(src[3], synth.synth_normal("cli.landmarks_src", (1, 136)) * 0.1 + 0.5) and eq(src[4], synth.synth_normal("cli.id_feat_src", (1, 512)))
    opt.arcface = True
    assert p.source()[4] is None
    assert eq(p.source_clip_image(), synth.synth_normal("cli.source224", (1, 3, 224, 224)))


@pytest.mark.parametrize("order", ["prepared_ahead", "prepared_after"])
def test_clip_provider_carries_the_label_map_across_the_batch_boundary(tmp_path, order):
    """4 frames in batches of 2, frame 2 -- the FIRST of batch 1 -- without landmarks: it takes the label map batch 0 ended with,
    whether batch 1 is prepared before batch 0's results are consumed (--pipeline_inversion) or after."""
    frames = write_frames(tmp_path / "f", 4, size=(320, 240))
    Image.fromarray(frames[0, :100, :90]).save(tmp_path / "src.png")
    _, arrays = landmark_file(str(tmp_path / "lm.npz"))
    clip = clip_io.ClipInputs(str(tmp_path / "f"), str(tmp_path / "src.png"), str(tmp_path / "lm.npz"), 4, 512, 512)
    opt = options("--target_frames", str(tmp_path / "f"), "--n_samples", "2", "--n_frames", "4")
    p = ClipRunInputs(clip, opt, "cpu")
    maps = lambda k: torch.stack([torch.full((8, 8), 10 * k + f, dtype=torch.uint8) for f in range(2)])
    assert p.inherits(0) == [False, False] and p.inherits(1) == [True, False]
    l0 = p.carry_labels(0, maps(0))
    assert torch.equal(l0, maps(0))
    if order == "prepared_after":       # batch 0 is sampled, written and let go of before batch 1 is looked at
        assert p.frame_ids(0) == [0, 1]
        l0.fill_(255)
    l1 = p.carry_labels(1, maps(1))
    assert torch.equal(l1[0], maps(0)[1]) and torch.equal(l1[1], maps(1)[1])
    # the rest of the interface, for the batch with the inherited frame
    assert p.frame_ids(1) == [2, 3] and p.tokens(1) == (None, None, None) and p.record_keys == ("frame_ids", "pasted_frames", "crops", "conditioning")
    paste_into, crop_from, quads, labels = p.intake_frames(1)
    assert labels is None and np.array_equal(paste_into.numpy(), frames[2:4]) and np.array_equal(crop_from.numpy(), frames[[1, 3]])
    assert np.array_equal(quads, clip.quads[2:])
    lmk = p.landmarks(1)
    assert lmk.dtype == torch.float32 and not lmk[0].any() and np.array_equal(lmk[1].numpy(), arrays["crops"][3].reshape(136).astype(np.float32))
    src = p.source()
    assert tuple(src[0].shape) == (1, 100, 90, 3) and src[2] is None and src[4] is None and tuple(src[3].shape) == (1, 136)
    assert torch.equal(p.learnable_vector(), synth.synth_normal("cli.learnable_vector", (1, 1, 768)))
