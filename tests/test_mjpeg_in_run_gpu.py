"""The real-clip run fed from a Motion-JPEG AVI (`--target_video clip.avi`): the fixture of tests/test_demux_run_gpu.py with the
clip written as an AVI of frames Pillow encoded with one restart interval per MCU row, against the same frames decoded by the model
(tests/jpeg_decode_model.py), saved as PNG and run with `--target_frames`."""
import numpy as np
import pytest
import torch
from PIL import Image

import demux_model as dm
import jpeg_decode_model as jdm
import jpeg_model as jm
import mjpeg_in_cases as cases
from test_clip_io_cpu import square, template_landmarks
from test_clip_run_gpu import FH, FW, N, cat, small_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """The clip on disk both ways, written once: 4 frames of 320 x 240, frame 2 -- the first of batch 1 -- without landmarks, so
    its crop is cut from frame 1, whose record is read again by seek."""
    import yaml
    from vface_amd.scripts import VFace_inference_batch as cli
    root = tmp_path_factory.mktemp("mjpeg_in")
    rng = np.random.default_rng(11)
    source = jm.patterns(N, FW, FH, seed=17)["smooth"]
    jpegs = [cases.pillow_jpeg(source[i], quality=90, restart_marker_rows=1) for i in range(N)]
    (root / "clip.avi").write_bytes(jm.avi_file(jpegs, FW, FH))
    decoded = []
    for jpeg in jpegs:
        coef, status, quant, W, H = jdm.decode_frame(jpeg)
        assert status == 0 and (W, H) == (FW, FH)
        decoded.append(dm.i420_to_rgb(jdm.planes(coef[None], quant[None], W, H), W, H, "bt601", True, "centre")[0])
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
    # frame 3 with the second half of its scan gone
    broken = jpegs[:3] + [jpegs[3][:len(jpegs[3]) // 2]]
    (root / "broken.avi").write_bytes(jm.avi_file(broken, FW, FH))

    def run(tag, source):
        args = [*source, "--src_image", str(root / "src.png"), "--landmarks", str(root / "lm.npz"), "--synthetic_weights",
                "--config", str(root / "small.yaml"), "--H", "512", "--W", "512", "--max_steps", "1", "--ddim_steps", "50",
                "--n_frames", str(N), "--n_samples", "2", "--skip_save", "--Base_dir", str(root / tag)]
        opt = cli.build_parser().parse_args(args)
        opt.return_samples = True
        torch.manual_seed(opt.seed)
        return cli.run_clip(opt)["batches"]
    return {"root": root, "run": run}


@pytest.fixture(scope="module")
def runs(clip):
    root, run = clip["root"], clip["run"]
    return {"video": run("v", ["--target_video", str(root / "clip.avi")]), "folder": run("f", ["--target_frames", str(root / "frames")])}


def test_avi_and_folder_of_its_decoded_frames_give_the_same_clip(runs):
    v, f = runs["video"], runs["folder"]
    assert len(v) == len(f) == 2 and [x["frame_ids"] for x in v] == [x["frame_ids"] for x in f] == [[0, 1], [2, 3]]
    for key in ("samples", "crops", "labels", "conditioning", "pasted_frames"):
        assert torch.equal(cat(v, key), cat(f, key)), key
    assert all(x["finite"] and x["pasted"] == [2, FH, FW, 3] for x in v)
    crops = cat(v, "crops")
    assert torch.equal(crops[2], crops[1]) and not torch.equal(crops[3], crops[1])       # frame 2 was cut from frame 1


def test_video_in_is_timed(runs):
    for x, y in zip(runs["folder"], runs["video"]):
        assert y["stage_seconds"]["video_in"] > 0 and "video_in" not in x["stage_seconds"]
        assert set(y["stage_seconds"]) - set(x["stage_seconds"]) == {"video_in"} and set(x) == set(y)


def test_the_matrix_flag_is_refused_with_an_avi(clip):
    with pytest.raises(SystemExit, match="--video_in_matrix names the matrix of a file that cannot tag it; .*clip.avi is Motion-JPEG"):
        clip["run"]("m", ["--target_video", str(clip["root"] / "clip.avi"), "--video_in_matrix", "bt601"])


def test_a_corrupt_frame_ends_the_run_by_name(clip):
    with pytest.raises(SystemExit, match="broken.avi: frame 3 does not decode: the scan does not hold the RST markers its DRI promises"):
        clip["run"]("b", ["--target_video", str(clip["root"] / "broken.avi")])
