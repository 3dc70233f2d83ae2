"""The real-clip run fed from a YUV4MPEG2 file (`--target_video`): the clip of tests/test_clip_run_gpu.py written as a .y4m, against
the same planes decoded by the model, saved as PNG and run with `--target_frames`."""
import numpy as np
import pytest
import torch
from PIL import Image

import demux_model as dm
import mux_model as mm
from test_clip_io_cpu import square, template_landmarks
from test_clip_run_gpu import FH, FW, N, cat, small_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The clip on disk both ways (written once) and its three runs: from the video file, from the folder, and from the video file
    read as BT.601.  4 frames of 320 x 240, 2 per batch, frame 2 -- the first of batch 1 -- without landmarks, so its crop is cut
    from frame 1, read again by seek."""
    import yaml
    from vface_amd.scripts import VFace_inference_batch as cli
    from vface_amd.scripts import mux
    root = tmp_path_factory.mktemp("video_in")
    rng = np.random.default_rng(11)
    i420 = mm.rgb_to_i420(rng.integers(0, 256, (N, FH, FW, 3), dtype=np.uint8))
    with open(root / "clip.y4m", "wb") as f:
        f.write(mux.y4m_header(FW, FH) + mux.y4m_frames(i420, FW, FH))
    decoded = dm.i420_to_rgb(i420, FW, FH)              # BT.709, limited, centre: what the header and the defaults say
    (root / "frames").mkdir()
    for i in range(N):
        Image.fromarray(decoded[i]).save(root / "frames" / f"{i}.png")
    Image.fromarray(rng.integers(0, 256, (180, 200, 3), dtype=np.uint8)).save(root / "src.png")
    quads = np.stack([square(160 + 4 * i, 120 - 3 * i, 60 + 2 * i, 0.06 * i) for i in range(N)])
    lm = np.stack([template_landmarks(q) for q in quads])
    lm[2] = np.nan
    np.savez(root / "lm.npz", frames=lm, source=template_landmarks(square(100, 90, 50, -0.1)),
             crops=rng.integers(100, 412, (N, 68, 2)).astype(np.float64), source_crop=rng.integers(100, 412, (68, 2)).astype(np.float64))
    (root / "small.yaml").write_text(yaml.safe_dump({"model": {"params": {"unet_config": {"params": small_cfg()}}}}))

    def run(tag, source):
        args = [*source, "--src_image", str(root / "src.png"), "--landmarks", str(root / "lm.npz"), "--synthetic_weights",
                "--config", str(root / "small.yaml"), "--H", "512", "--W", "512", "--max_steps", "1", "--ddim_steps", "50",
                "--n_frames", str(N), "--n_samples", "2", "--skip_save", "--Base_dir", str(root / tag)]
        opt = cli.build_parser().parse_args(args)
        opt.return_samples = True
        torch.manual_seed(opt.seed)
        return cli.run_clip(opt)["batches"]

    video = ["--target_video", str(root / "clip.y4m")]
    return {"decoded": decoded, "video": run("v", video), "folder": run("f", ["--target_frames", str(root / "frames")]),
            "bt601": run("m", video + ["--video_in_matrix", "bt601"])}


def test_video_file_and_folder_of_its_decoded_frames_give_the_same_clip(runs):
    v, f = runs["video"], runs["folder"]
    assert len(v) == len(f) == 2 and [x["frame_ids"] for x in v] == [x["frame_ids"] for x in f] == [[0, 1], [2, 3]]
    for key in ("samples", "crops", "labels", "conditioning", "pasted_frames"):
        assert torch.equal(cat(v, key), cat(f, key)), key
    assert all(x["finite"] and x["pasted"] == [2, FH, FW, 3] for x in v)
    crops = cat(v, "crops")
    assert torch.equal(crops[2], crops[1]) and not torch.equal(crops[3], crops[1])       # frame 2 was cut from frame 1


def test_video_in_is_timed_for_video_runs_only(runs):
    for x in runs["video"] + runs["bt601"]:
        assert x["stage_seconds"]["video_in"] > 0
        for stage in ("intake", "parse", "clip_cond", "flow", "inversion", "vae_encode", "vae_decode", "paste_back"):
            assert x["stage_seconds"][stage] > 0, stage
    for x, y in zip(runs["folder"], runs["video"]):
        assert "video_in" not in x["stage_seconds"]
        assert set(y["stage_seconds"]) - set(x["stage_seconds"]) == {"video_in"} and set(x) == set(y)


def test_the_matrix_flag_reaches_the_frames(runs):
    assert not torch.equal(cat(runs["bt601"], "crops"), cat(runs["video"], "crops"))
    assert not torch.equal(cat(runs["bt601"], "pasted_frames"), cat(runs["video"], "pasted_frames"))
