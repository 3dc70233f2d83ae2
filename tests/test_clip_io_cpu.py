"""What a real-clip run reads from disk (vface_amd/scripts/clip_io.py) and the command line that starts it -- without a GPU."""
import numpy as np
import pytest
import torch
from PIL import Image

from vface_amd.scripts import VFace_inference_batch as cli
from vface_amd.scripts import clip_io
from vface_amd.scripts.intake import inv_transforms, quad_from_landmarks


def write_frames(folder, n, size=(6, 4), ext="png", seed=0):
    folder.mkdir(exist_ok=True)
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (n, size[1], size[0], 3), dtype=np.uint8)
    for i in range(n):
        Image.fromarray(frames[i]).save(folder / f"{i}.{ext}")
    return frames


def template_landmarks(quad):
    """68 points whose ``quad_from_landmarks`` is ``quad`` [4, 2] (NW, SW, SE, NE of a square, any rotation and size): the eyes
    and the mouth are placed where compute_transform (alignmengt.py:152-178) reads them, every other point at the centre."""
    quad = np.asarray(quad, dtype=np.float64)
    centre = quad.mean(0)
    x = (quad[3] - quad[0]) / 2.0                   # half the top edge: the crop's x axis
    y = (quad[1] - quad[0]) / 2.0                   # half the left edge: its y axis
    e2e = x / 2.0                                   # eye to eye: 2 |e2e| = |x|, the larger of the two candidate sizes
    e2m = y * 0.5                                   # eyes to mouth: 1.8 |e2m| = 0.9 |x|; perpendicular to e2e, so x keeps its direction
    eye_avg = centre - e2m * 0.1
    lm = np.tile(centre, (68, 1))
    lm[36:42] = eye_avg - e2e / 2.0
    lm[42:48] = eye_avg + e2e / 2.0
    lm[48:60] = eye_avg + e2m
    return lm


def square(cx, cy, half, theta=0.0):
    c, s = np.cos(theta), np.sin(theta)
    x, y = half * np.array([c, s]), half * np.array([-s, c])
    o = np.array([cx, cy], dtype=np.float64)
    return np.stack([o - x - y, o - x + y, o + x + y, o + x - y])


def test_template_landmarks_give_back_their_quad():
    for q in (square(160, 120, 60), square(100.5, 90.25, 40, 0.3)):
        assert np.allclose(quad_from_landmarks(template_landmarks(q)), q, atol=1e-9)


def test_frames_are_listed_in_numeric_order(tmp_path):
    frames = write_frames(tmp_path / "f", 12)
    listed = clip_io.list_frames(str(tmp_path / "f"))
    assert [i for i, _ in listed] == list(range(12))                    # 2 before 10: not the order of the names
    assert sorted(p.name for p in (tmp_path / "f").iterdir())[:3] == ["0.png", "1.png", "10.png"]
    got = clip_io.load_frames([p for _, p in listed])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (12, 4, 6, 3) and np.array_equal(got.numpy(), frames)
    Image.fromarray(frames[0]).save(tmp_path / "f" / "12.jpg")          # .jpg is a frame name too
    assert [i for i, _ in clip_io.list_frames(str(tmp_path / "f"))] == list(range(13))
    grey = tmp_path / "g"
    grey.mkdir()
    Image.fromarray(frames[0, :, :, 0]).save(grey / "0.png")           # an 8-bit grey file decodes to RGB
    assert tuple(clip_io.load_frames([str(grey / "0.png")]).shape) == (1, 4, 6, 3)


def test_stray_names_and_mixed_sizes_are_refused(tmp_path):
    write_frames(tmp_path / "f", 3)
    (tmp_path / "f" / "notes.txt").write_text("x")
    with pytest.raises(SystemExit, match="notes.txt"):
        clip_io.list_frames(str(tmp_path / "f"))
    (tmp_path / "f" / "notes.txt").unlink()
    Image.fromarray(np.zeros((4, 6, 3), np.uint8)).save(tmp_path / "f" / "frame_3.png")
    with pytest.raises(SystemExit, match="frame_3.png"):
        clip_io.list_frames(str(tmp_path / "f"))
    (tmp_path / "f" / "frame_3.png").unlink()
    Image.fromarray(np.zeros((4, 6, 3), np.uint8)).save(tmp_path / "f" / "02.png")       # the index 2 a second time
    with pytest.raises(SystemExit, match="twice"):
        clip_io.list_frames(str(tmp_path / "f"))
    (tmp_path / "f" / "02.png").unlink()
    Image.fromarray(np.zeros((5, 6, 3), np.uint8)).save(tmp_path / "f" / "3.png")
    with pytest.raises(SystemExit, match="one size"):
        clip_io.load_frames([p for _, p in clip_io.list_frames(str(tmp_path / "f"))])
    with pytest.raises(SystemExit, match="not a directory"):
        clip_io.list_frames(str(tmp_path / "nowhere"))


def landmark_file(path, n=4, nan=(2,), with_crops=True, **extra):
    quads = [square(160 + 3 * i, 120 + 2 * i, 60, 0.05 * i) for i in range(n)]
    frames = np.stack([template_landmarks(q) for q in quads])
    for i in nan:
        frames[i] = np.nan
    arrays = {"frames": frames, "source": template_landmarks(square(100, 100, 50, -0.1))}
    if with_crops:
        rng = np.random.default_rng(1)
        arrays["crops"] = rng.integers(0, 512, (n, 68, 2)).astype(np.float64)
        arrays["source_crop"] = rng.integers(0, 512, (68, 2)).astype(np.float64)
    arrays.update(extra)
    np.savez(path, **arrays)
    return quads, arrays


def test_landmarks_file_shapes_and_fallback(tmp_path):
    path = str(tmp_path / "lm.npz")
    quads, arrays = landmark_file(path, n=5, nan=(2, 3))
    lm = clip_io.load_landmarks(path, 5)
    assert lm.frames.shape == (5, 68, 2) and lm.source.shape == (68, 2) and lm.crops.shape == (5, 68, 2) and lm.source_crop.shape == (68, 2)
    found, take = clip_io.fallback_indices(lm.frames)
    assert list(found) == [True, True, False, False, True] and list(take) == [0, 1, 1, 1, 4]
    with pytest.raises(SystemExit, match="needs 6"):
        clip_io.load_landmarks(path, 6)
    landmark_file(path, nan=(0,))
    with pytest.raises(SystemExit, match="frame 0"):
        clip_io.fallback_indices(clip_io.load_landmarks(path).frames)
    for bad, word in ((dict(frames=np.zeros((4, 67, 2))), "frames"), (dict(source=np.zeros((68, 3))), "source"),
                      (dict(crops=np.zeros((3, 68, 2))), "crops"), (dict(source_crop=np.zeros(136)), "source_crop"),
                      (dict(quads=np.zeros((4, 4, 2))), "quads")):
        landmark_file(path, **bad)
        with pytest.raises(SystemExit, match=word):
            clip_io.load_landmarks(path, 4)
    np.savez(path, frames=np.zeros((4, 68, 2)))
    with pytest.raises(SystemExit, match="source"):
        clip_io.load_landmarks(path)


def test_clip_inputs(tmp_path):
    """The batches of a 4-frame clip whose frame 2 has no landmarks: it takes frame 1's quad, coefficients and PIXELS for the crop
    (read again: frame 1 is in the batch before), keeps its own frame for the paste, and its conditioning landmarks are zeros."""
    frames = write_frames(tmp_path / "f", 5, size=(320, 240))
    Image.fromarray(frames[0, :100, :90]).save(tmp_path / "src.png")
    path = str(tmp_path / "lm.npz")
    quads, arrays = landmark_file(path)
    clip = clip_io.ClipInputs(str(tmp_path / "f"), str(tmp_path / "src.png"), path, 4, 512, 512)
    assert clip.frame_ids == [0, 1, 2, 3] and tuple(clip.source_u8.shape) == (1, 100, 90, 3)
    assert np.allclose(clip.quads, np.stack([quads[0], quads[1], quads[1], quads[3]]), atol=1e-9)
    assert np.array_equal(clip.coeffs, inv_transforms(clip.quads, 1024)) and clip.coeffs.shape == (4, 8)
    assert np.array_equal(clip.landmarks[[0, 1, 3]], arrays["crops"][[0, 1, 3]].reshape(3, 136).astype(np.float32))
    assert clip.landmarks.dtype == np.float32 and not clip.landmarks[2].any()
    assert np.array_equal(clip.source_landmarks, arrays["source_crop"].reshape(1, 136).astype(np.float32))
    b0, b1 = clip.batch(0, 2), clip.batch(1, 2)
    assert b0["frame_ids"] == [0, 1] and b1["frame_ids"] == [2, 3] and list(b1["found"]) == [False, True]
    assert np.array_equal(b0["frames"].numpy(), frames[:2]) and b0["crop_frames"] is b0["frames"]
    assert np.array_equal(b1["frames"].numpy(), frames[2:4])
    assert np.array_equal(b1["crop_frames"].numpy(), frames[[1, 3]])
    assert np.array_equal(b1["quads"], clip.quads[2:]) and np.array_equal(b1["landmarks"], clip.landmarks[2:])
    one = clip.batch(0, 4)        # the same fallback inside one batch
    assert np.array_equal(one["crop_frames"].numpy(), frames[[0, 1, 1, 3]]) and np.array_equal(one["frames"].numpy(), frames[:4])
    with pytest.raises(SystemExit, match="--n_frames asks for 6"):
        clip_io.ClipInputs(str(tmp_path / "f"), str(tmp_path / "src.png"), path, 6, 512, 512)


def test_derived_crop_landmarks_put_a_quad_corner_on_the_crops_corner(tmp_path):
    """Without `crops` the conditioning landmarks are the frame points pushed through the crop's projective map: a point exactly on
    a corner of the quad lands on the matching corner of the H x W crop, within one pixel, and the centre on the centre."""
    H, W = 512, 384
    for q in (square(160, 120, 60), square(100.5, 90.25, 40, 0.3)):
        co = inv_transforms(q[None], 1024)[0]
        pts = np.tile(q.mean(0), (68, 1))
        pts[:4] = q                                             # NW, SW, SE, NE
        got = clip_io.derive_crop_landmarks(pts, co, 1024, H, W)
        assert got.shape == (68, 2) and np.array_equal(got, np.rint(got))
        for p, corner in zip(got[:4], ([0, 0], [0, H], [W, H], [W, 0])):
            assert np.abs(p - corner).max() <= 1.0, (p, corner)
        assert np.abs(got[4] - [W / 2, H / 2]).max() <= 1.0
    path = str(tmp_path / "lm.npz")
    quads, arrays = landmark_file(path, with_crops=False)
    lm = clip_io.load_landmarks(path, 4)
    assert lm.crops is None and lm.source_crop is None
    write_frames(tmp_path / "f", 4, size=(320, 240))
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "src.png")
    clip = clip_io.ClipInputs(str(tmp_path / "f"), str(tmp_path / "src.png"), path, 4, 512, 512)
    want = clip_io.derive_crop_landmarks(arrays["frames"][1], clip.coeffs[1], 1024, 512, 512).reshape(136)
    assert np.array_equal(clip.landmarks[1], want.astype(np.float32)) and not clip.landmarks[2].any() and clip.landmarks[3].any()
    # the template's eyes lie on the crop's horizontal midline region, inside the crop
    assert (clip.landmarks[1] >= 0).all() and (clip.landmarks[1] <= 512).all()
    assert clip.source_landmarks.shape == (1, 136) and clip.source_landmarks.any()


def test_new_flags_parse_and_missing_ones_are_named(tmp_path):
    p = cli.build_parser()
    opt = p.parse_args(["--target_frames", "d", "--src_image", "s.png", "--landmarks", "l.npz", "--video_out", "o.y4m", "--synthetic_weights"])
    assert (opt.target_frames, opt.src_image, opt.landmarks, opt.video_out, opt.synthetic_weights) == ("d", "s.png", "l.npz", "o.y4m", True)
    none = p.parse_args([])
    assert (none.target_frames, none.src_image, none.landmarks, none.video_out, none.synthetic_weights) == (None, None, None, None, False)
    with pytest.raises(SystemExit, match="--target_frames"):
        cli.main([])
    base = ["--target_frames", "d", "--src_image", "s.png", "--landmarks", "l.npz"]
    with pytest.raises(SystemExit, match="--src_image"):
        cli.main(base[:2] + base[4:])
    with pytest.raises(SystemExit, match="--landmarks"):
        cli.main(base[:4])
    with pytest.raises(SystemExit, match="--ckpt"):
        cli.main(base)
    with pytest.raises(SystemExit, match="--faceParsing_ckpt"):
        cli.main(base + ["--ckpt", "a.ckpt", "--raft_ckpt", "r.pth"])
    with pytest.raises(SystemExit, match="--raft_ckpt"):
        cli.main(base + ["--ckpt", "a.ckpt", "--faceParsing_ckpt", "p.pth"])
    with pytest.raises(SystemExit, match="drop --ckpt"):
        cli.main(base + ["--synthetic_weights", "--ckpt", "a.ckpt"])
    with pytest.raises(SystemExit, match="--parse needs --H 512 --W 512"):
        cli.main(base + ["--synthetic_weights", "--H", "256", "--W", "256"])
    opt = p.parse_args(base + ["--synthetic_weights"])
    cli.check_clip_options(opt)
    assert all(getattr(opt, name) for name in cli.CLIP_STAGES) and opt.fusion == "flow_fix"
