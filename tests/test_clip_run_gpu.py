"""The real-clip run of the command line (`run_clip`): frames, source image and landmarks from disk, seeded weights, one DDIM
step -- through intake, parser, conditioning, flow, inversion, sampling, decode, paste-back, PNG and YUV4MPEG2 output."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import mux_model as mm
from test_clip_io_cpu import square, template_landmarks

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N, FW, FH = 4, 320, 240         # frames of the clip; non-square, so a W / H swap anywhere shows


def small_cfg():
    """The small UNet of the other command-line tests, at the 64 x 64 latents of a 512 x 512 run (as test_cli_parse sets it)."""
    from test_source_gpu import small_cfg as cfg
    return dict(cfg(), image_size=64)


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """The clip on disk (written once) and four runs of it: twice as it is, once with a landmarks file without `crops`, once with
    `--pipeline_inversion`."""
    import yaml
    from vface_amd.scripts import VFace_inference_batch as cli
    root = tmp_path_factory.mktemp("clip")
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (N, FH, FW, 3), dtype=np.uint8)
    (root / "frames").mkdir()
    for i in range(N):
        Image.fromarray(frames[i]).save(root / "frames" / f"{i}.png")
    source = rng.integers(0, 256, (180, 200, 3), dtype=np.uint8)
    Image.fromarray(source).save(root / "src.png")
    quads = np.stack([square(160 + 4 * i, 120 - 3 * i, 60 + 2 * i, 0.06 * i) for i in range(N)])
    lm = np.stack([template_landmarks(q) for q in quads])
    lm[2] = np.nan                                  # frame 2: no face found; it is the FIRST frame of batch 1
    src_lm = template_landmarks(square(100, 90, 50, -0.1))
    crops = rng.integers(100, 412, (N, 68, 2)).astype(np.float64)
    np.savez(root / "lm.npz", frames=lm, source=src_lm, crops=crops, source_crop=rng.integers(100, 412, (68, 2)).astype(np.float64))
    np.savez(root / "lm_nocrops.npz", frames=lm, source=src_lm)
    (root / "small.yaml").write_text(yaml.safe_dump({"model": {"params": {"unet_config": {"params": small_cfg()}}}}))

    def run(tag, landmarks="lm.npz", more=()):
        args = ["--target_frames", str(root / "frames"), "--src_image", str(root / "src.png"), "--landmarks", str(root / landmarks),
                "--video_out", str(root / f"{tag}.y4m"), "--synthetic_weights", "--config", str(root / "small.yaml"),
                "--H", "512", "--W", "512", "--max_steps", "1", "--ddim_steps", "50", "--n_frames", str(N), "--n_samples", "2",
                "--Base_dir", str(root / tag), *more]
        opt = cli.build_parser().parse_args(args)
        opt.return_samples = True
        torch.manual_seed(opt.seed)
        return cli.run_clip(opt)["batches"]

    return {"root": root, "frames": frames, "quads": quads, "a": run("a"), "b": run("b"), "nocrops": run("c", "lm_nocrops.npz"),
            "pipelined": run("d", more=["--pipeline_inversion"])}


def cat(batches, key):
    return torch.cat([b[key] for b in batches])


def test_clip_run_is_complete_and_repeatable(clip):
    a, b = clip["a"], clip["b"]
    assert len(a) == 2 and [x["frame_ids"] for x in a] == [[0, 1], [2, 3]]
    for x in a:
        assert x["finite"] and x["pixels"] == [2, 3, 512, 512] and x["pasted"] == [2, FH, FW, 3]
        for stage in ("intake", "parse", "clip_cond", "flow", "inversion", "vae_encode", "vae_decode", "paste_back", "video_out"):
            assert x["stage_seconds"][stage] > 0, stage
    assert a[0]["stage_seconds"]["source_intake"] > 0
    for key in ("samples", "pasted_frames", "crops", "conditioning", "labels"):
        assert torch.equal(cat(a, key), cat(b, key)), key
    pasted = cat(a, "pasted_frames")
    assert pasted.dtype == torch.uint8 and tuple(pasted.shape) == (N, FH, FW, 3)
    assert not torch.equal(pasted, torch.from_numpy(clip["frames"]).to(DEV))


def test_pipelined_inversion_gives_the_same_clip(clip):
    """Two batches with the frame without landmarks on the boundary: batch 1 is prepared -- its label map inherited -- before batch
    0 is sampled, and every tensor equals the sequential run's."""
    a, p = clip["a"], clip["pipelined"]
    assert ["sampling_beside_next_inversion" in x["stage_seconds"] for x in p] == [True, False] and "next_parse" in p[0]["stage_seconds"]
    for key in ("samples", "pasted_frames", "crops", "labels", "conditioning"):
        assert torch.equal(cat(a, key), cat(p, key)), key


def test_outputs_on_disk_are_the_pasted_frames(clip):
    from vface_amd import hip
    pasted = cat(clip["a"], "pasted_frames")
    results = clip["root"] / "a" / "results"
    assert sorted(os.listdir(results), key=lambda s: int(s.split(".")[0])) == [f"{i}.png" for i in range(N)]
    for i in range(N):
        assert np.array_equal(np.array(Image.open(results / f"{i}.png")), pasted[i].cpu().numpy()), i
    tags, payload = mm.read_y4m(str(clip["root"] / "a.y4m"))
    assert (tags["W"], tags["H"], tags["F"]) == (str(FW), str(FH), "10:1") and payload.shape == (N, mm.frame_bytes(FW, FH))
    assert np.array_equal(payload, hip.rgb_to_yuv420(pasted).cpu().numpy())
    mm.check_i420(payload, pasted.cpu().numpy(), "video_out")


def test_crops_are_the_intakes_and_a_frame_without_landmarks_takes_the_one_before(clip):
    from vface_amd.scripts.intake import FrameIntake, quad_from_landmarks
    crops = cat(clip["a"], "crops")
    assert tuple(crops.shape) == (N, 1024, 1024, 3)
    decoded = torch.stack([torch.from_numpy(np.array(Image.open(clip["root"] / "frames" / f"{i}.png").convert("RGB")))
                           for i in range(N)]).to(DEV)
    take = [0, 1, 1, 3]
    quads = np.stack([quad_from_landmarks(template_landmarks(clip["quads"][t])) for t in take])
    by_hand = FrameIntake(H=512, W=512, latent=(64, 64), device=DEV).crop(decoded[take].contiguous(), quads)
    assert torch.equal(crops, by_hand)
    assert torch.equal(crops[2], crops[1]) and not torch.equal(crops[3], crops[1])
    labels = cat(clip["a"], "labels")
    assert torch.equal(labels[2], labels[1])
    pasted = cat(clip["a"], "pasted_frames")
    # pasted into its own frame: outside the quad, the background is frame 2's (after its VAE round trip), not frame 1's
    assert not torch.equal(pasted[2], pasted[1]) and not torch.equal(pasted[2, 0], pasted[1, 0])


def test_without_crop_landmarks_the_conditioning_is_derived(clip):
    a, c = clip["a"], clip["nocrops"]
    assert torch.equal(cat(a, "crops"), cat(c, "crops"))
    ca, cc = cat(a, "conditioning"), cat(c, "conditioning")
    assert tuple(ca.shape) == (N, 1, 768) and bool(torch.isfinite(cc).all())
    for f in (0, 1, 3):
        assert not torch.equal(ca[f], cc[f]), f


def test_synthetic_path_is_untouched(tmp_path):
    """tests/test_parse_gpu.py test_cli_parse's run again: the `--synthetic` record has the keys it had and none of the clip's."""
    import yaml
    from vface_amd.scripts import VFace_inference_batch as cli
    ypath = tmp_path / "small.yaml"
    ypath.write_text(yaml.safe_dump({"model": {"params": {"unet_config": {"params": small_cfg()}}}}))
    args = ["--synthetic", "--with_vae", "--intake", "--parse", "--paste_back", "--frame_size", "640", "--config", str(ypath),
            "--n_frames", "2", "--n_samples", "2", "--H", "512", "--W", "512", "--max_steps", "1", "--ddim_steps", "50", "--skip_save",
            "--Base_dir", str(tmp_path / "a")]
    opt = cli.build_parser().parse_args(args)
    opt.return_samples = True
    torch.manual_seed(opt.seed)
    b = cli.run_synthetic(opt)["batches"][0]
    assert sorted(b) == sorted(["batch", "frames", "sample_seconds", "batch_wall_seconds", "samples", "labels", "inversion_cache", "finite",
                                "pixels", "pasted", "paste_seconds", "stage_seconds"])
    assert b["finite"] and b["pixels"] == [2, 3, 512, 512] and b["pasted"] == [2, 640, 640, 3]
    assert b["stage_seconds"]["parse"] > 0 and "video_out" not in b["stage_seconds"]
    labels = b["labels"]
    assert labels.shape == (2, 512, 512) and int(labels.max()) < 12
    assert not torch.equal(labels.cpu(), cli.synthetic_intake_inputs(2, 640, 512, 512, opt.seed + 1000)[2])
