"""The video intake without a GPU: the integer model of the I420 -> RGB conversion (tests/demux_model.py) against its fp64
definition and against the mux's model, the coefficient tables of csrc/demux.hip, the seeded defects, the YUV4MPEG2 reader
(vface_amd/scripts/demux.py), the command line's new flags and ``ClipInputs`` over a reader."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import demux_model as dm
import mux_model as mm
from conftest import ROOT
from test_clip_io_cpu import landmark_file
from vface_amd.scripts import VFace_inference_batch as cli
from vface_amd.scripts import clip_io, demux, mux


# ---- the model
@pytest.mark.parametrize("matrix,full_range", dm.TABLES)
def test_model_against_the_fp64_definition(matrix, full_range):
    """All 2^24 (Y, Cb, Cr) triples in `nearest` mode (chroma sixteenths = 16 x the sample): the integer result against the clamped
    definition.  The bound is derived from the coefficients' rounding residues (dm.definition_bound), not picked."""
    coeff, off = dm.coefficients(matrix, full_range)
    bound = dm.definition_bound(matrix, full_range)
    assert 0.5 < bound < 0.51
    cb, cr = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = 0.0
    for y in range(256):
        got = dm.rgb_from_sixteenths(y, 16 * cb, 16 * cr, coeff, off)
        want = np.clip(dm.fp64_definition(float(y), cb, cr, matrix, full_range), 0.0, 255.0)
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"{matrix} {'full' if full_range else 'limited'}: worst |model - definition| = {worst:.5f}, derived bound {bound:.5f}")
    assert worst <= bound, (worst, bound)
    assert worst > 0.49          # (the half level of the rounding is reached: the comparison is not vacuous)


def test_bt709_limited_coefficients_are_the_published_ones():
    coeff, off = dm.coefficients("bt709", False)
    assert coeff.tolist() == [76309, 117489, -34925, -13975, 138438] and off == 16
    assert dm.coefficients("bt709", True)[0][0] == 65536 and dm.coefficients("bt601", True)[1] == 0


def test_every_intermediate_fits_int32():
    ranges = dm.value_ranges()
    assert set(ranges) == set(dm.TABLES)
    for table, rec in ranges.items():
        assert rec["peak"] < 2 ** 31, (table, rec)
        for ch in "rgb":
            lo, hi = rec[ch]
            assert -2 ** 31 <= lo < 0 and 255 << 20 < hi < 2 ** 31, (table, ch, lo, hi)      # both clamp ends are reachable
    assert abs(ranges[("bt709", False)]["peak"] - 5.8e8) < 0.1e8
    # the extremes are reached: the corners of the box through the model itself
    for (matrix, full), rec in ranges.items():
        coeff, off = dm.coefficients(matrix, full)
        y, u, v = np.meshgrid([0, 255], [0, 4080], [0, 4080], indexing="ij")
        raw = (dm.rgb_from_sixteenths(y, u, v, coeff, off, clamp=False).astype(np.int64))
        for k, ch in enumerate("rgb"):
            assert raw[..., k].min() == rec[ch][0] >> 20 and raw[..., k].max() == rec[ch][1] >> 20, (matrix, full, ch)


@pytest.mark.parametrize("mode", dm.CHROMA_MODES)
def test_chroma_weights_sum_to_sixteen_everywhere(mode):
    """At every pixel of every size -- edges and odd sides included -- the four weights are non-negative and sum to 16, and every
    neighbour index lies inside the plane: a plane of ones comes back as 16, and the sixteenths of any plane stay in 0..4080."""
    for W, H in mm.SIZES:
        cw, ch = (W + 1) // 2, (H + 1) // 2
        for horizontal, n, cn in ((True, W, cw), (False, H, ch)):
            ia, wa, ib, wb = dm.chroma_taps(n, cn, mode, horizontal)
            assert ((wa + wb) == 4).all() and (wa >= 0).all() and (wb >= 0).all()
            assert (ia >= 0).all() and (ia < cn).all() and (ib >= 0).all() and (ib < cn).all()
        assert (dm.chroma_sixteenths(np.ones((1, ch, cw), np.uint8), W, H, mode) == 16).all()
        assert (dm.chroma_sixteenths(np.full((1, ch, cw), 255, np.uint8), W, H, mode) == 4080).all()


def test_chroma_modes_place_a_single_sample_where_they_should():
    """One bright sample at (row 1, column 1) of a 3 x 3 chroma plane under 6 x 6 luma: the weights every mode spreads around it."""
    c = np.zeros((1, 3, 3), np.uint8)
    c[0, 1, 1] = 1
    near = dm.chroma_sixteenths(c, 6, 6, "nearest")[0]
    assert near[2:4, 2:4].tolist() == [[16, 16], [16, 16]] and near.sum() == 64
    centre = dm.chroma_sixteenths(c, 6, 6, "centre")[0]
    assert centre[1:5, 1:5].tolist() == [[1, 3, 3, 1], [3, 9, 9, 3], [3, 9, 9, 3], [1, 3, 3, 1]] and centre.sum() == 64
    left = dm.chroma_sixteenths(c, 6, 6, "left")[0]
    assert left[1:5, 1:4].tolist() == [[2, 4, 2], [6, 12, 6], [6, 12, 6], [2, 4, 2]] and left.sum() == 64


def test_tables_of_the_kernel_are_the_models():
    src = open(os.path.join(ROOT, "vface_amd", "csrc", "demux.hip")).read()
    for name, matrix in (("kBt709", "bt709"), ("kBt601", "bt601")):
        m = re.search(r"constexpr int " + name + r"\[2\]\[5\] = \{\{([^}]*)\}, \{([^}]*)\}\};", src)
        assert m, name
        for full, row in enumerate(m.groups()):
            assert [int(v) for v in row.split(",")] == dm.coefficients(matrix, bool(full))[0].tolist(), (name, full)
    assert "full_range ? 0 : 16" in src
    from vface_amd import hip
    assert hip.YUV_MATRICES == {"bt709": 0, "bt601": 1} and hip.YUV_CHROMA == {m: i for i, m in enumerate(dm.CHROMA_MODES)}
    assert re.search(r"enum \{ kNearest = 0, kCentre = 1, kLeft = 2 \}", src)


@pytest.mark.parametrize("defect", dm.DEFECTS)
def test_every_defect_is_seen(defect):
    """Each seeded wrong conversion differs from the model BY VALUE (i420_to_rgb asserts that its bytes stay bytes) and check_rgb
    says so: on the noise at both sizes, and on the pattern made for it."""
    made_for = {"nearest": "checker", "edge_wrap": "checker", "odd_row_off": "checker", "no_clamp": "noise", "full_range": "corners",
                "truncate": "noise", "bt601": "corners", "swap_uv": "corners", "swap_rb": "corners"}
    for W, H in ((7, 5), (66, 34)):
        pats = dm.patterns(2, W, H)
        for name in ("noise", made_for[defect]):
            bad = dm.i420_to_rgb(pats[name], W, H, defect=defect)
            with pytest.raises(AssertionError, match="first at frame"):
                dm.check_rgb(bad, pats[name], W, H, what=defect)
    for name, p in dm.patterns(2, 7, 5).items():
        dm.check_rgb(dm.i420_to_rgb(p, 7, 5), p, 7, 5, what=name)          # and the model passes its own check


def test_patterns_reach_both_clamp_ends_and_separate_the_chroma_modes():
    W, H = 66, 34
    pats = dm.patterns(1, W, H)
    assert set(pats) == {"noise", "corners", "checker"}
    for p in pats.values():
        assert p.dtype == np.uint8 and p.shape == (1, mm.frame_bytes(W, H))
    coeff, off = dm.coefficients()
    y, cb, cr = mm.planes(pats["noise"], W, H)
    raw = dm.rgb_from_sixteenths(y, dm.chroma_sixteenths(cb, W, H, "centre"), dm.chroma_sixteenths(cr, W, H, "centre"), coeff, off,
                                 clamp=False)
    assert raw.min() < 0 and raw.max() > 255
    assert {16, 235, 240, 128, 0, 255} <= set(np.unique(pats["corners"]))
    out = {m: dm.i420_to_rgb(pats["checker"], W, H, chroma=m) for m in dm.CHROMA_MODES}
    assert not np.array_equal(out["nearest"], out["centre"]) and not np.array_equal(out["centre"], out["left"])
    assert not np.array_equal(out["nearest"], out["left"])


# ---- round trip with the mux's model
def test_round_trip_with_the_mux_model_over_all_colours():
    """rgb -> mux_model -> demux_model on FLAT frames, for all 2^24 colours: every channel back within 2 levels (BT.709 limited,
    what the mux writes).  A flat frame's chroma sample is the pixel's own (the mean of equal pixels), and every chroma mode
    interpolates equal samples to themselves, so the frame reduces to one pixel -- which the second half checks on real frames."""
    coeff, off = dm.coefficients()
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = np.zeros(3, np.int64)
    for r in range(256):
        y = mm.luma_from_rgb(r, g, b)
        u = mm.chroma_from_sums(r, g, b, 0, mm.CB)
        v = mm.chroma_from_sums(r, g, b, 0, mm.CR)
        back = dm.rgb_from_sixteenths(y, 16 * u, 16 * v, coeff, off)
        err = np.abs(back - np.stack([np.full_like(g, r), g, b], axis=-1)).reshape(-1, 3).max(axis=0)
        worst = np.maximum(worst, err)
    print("worst round-trip error (R, G, B):", worst.tolist())
    assert (worst <= 2).all(), worst
    rng = np.random.default_rng(3)
    for W, H in ((7, 5), (2, 2), (1, 1)):
        colours = rng.integers(0, 256, (40, 3), dtype=np.uint8)
        flat = np.broadcast_to(colours[:, None, None, :], (40, H, W, 3)).copy()
        i420 = mm.rgb_to_i420(flat)
        near = dm.i420_to_rgb(i420, W, H, chroma="nearest")
        assert np.array_equal(dm.i420_to_rgb(i420, W, H, chroma="centre"), near)
        assert np.array_equal(dm.i420_to_rgb(i420, W, H, chroma="left"), near)
        assert np.abs(near.astype(int) - flat).max() <= 2
        one = dm.rgb_from_sixteenths(mm.luma_from_rgb(*colours.T.astype(np.int64)),
                                     16 * mm.chroma_from_sums(*colours.T.astype(np.int64), 0, mm.CB),
                                     16 * mm.chroma_from_sums(*colours.T.astype(np.int64), 0, mm.CR), coeff, off)
        assert np.array_equal(near[:, 0, 0], one)


# ---- the reader
def write_y4m(path, i420, W, H, header=None, marker=b"FRAME\n"):
    with open(path, "wb") as f:
        f.write(mux.y4m_header(W, H) if header is None else header)
        for row in i420:
            f.write(marker + row.tobytes())


@pytest.mark.parametrize("W,H", [(66, 34), (7, 5), (1, 1)])
def test_reader_round_trips_what_the_mux_writes(tmp_path, W, H):
    i420 = dm.patterns(5, W, H)["noise"]
    path = str(tmp_path / "clip.y4m")
    with open(path, "wb") as f:
        f.write(mux.y4m_header(W, H))
        f.write(mux.y4m_frames(i420[:2], W, H))
        f.write(mux.y4m_frames(i420[2:], W, H))
    with demux.Y4MReader(path) as r:
        head = r.header
        assert (r.W, r.H, len(r), r.frame_bytes) == (W, H, 5, mm.frame_bytes(W, H))
        assert (head.fps, head.interlace, head.aspect, head.siting, head.full_range) == ((10, 1), "p", "1:1", "centre", False)
        assert head.x_tags == {"COLORRANGE": "LIMITED"}
        got = r.read(range(5))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (5, mm.frame_bytes(W, H)) and np.array_equal(got.numpy(), i420)
        assert np.array_equal(r.read([4, 0, 2, 2]).numpy(), i420[[4, 0, 2, 2]])          # random order, by seek
        assert tuple(r.read([]).shape) == (0, mm.frame_bytes(W, H))
        with pytest.raises(IndexError):
            r.read([5])
    tags, frames = mm.read_y4m(path)                                                      # the other reader agrees
    assert np.array_equal(frames, i420)


def test_reader_finds_frames_behind_frame_parameters_and_never_reads_planes_to_count(tmp_path, monkeypatch):
    W, H = 6, 4
    i420 = dm.patterns(3, W, H)["noise"]
    path = str(tmp_path / "p.y4m")
    head = b"YUV4MPEG2 W6 H4 F30000:1001 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL\n"
    with open(path, "wb") as f:
        f.write(head)
        for k, row in enumerate(i420):
            f.write((b"FRAME\n", b"FRAME Ip\n", b"FRAME Xabc=1 It\n")[k] + row.tobytes())
    r = demux.Y4MReader(path)
    assert len(r) == 3 and np.array_equal(r.read([2, 1, 0]).numpy(), i420[::-1])
    assert r.header.fps == (30000, 1001) and r.header.siting == "left" and r.header.full_range and r.header.interlace == "p"
    assert r.header.x_tags == {"YSCSS": "420MPEG2", "COLORRANGE": "FULL"} and r.header.aspect == ""
    assert r.offsets == [len(head) + 6, len(head) + 6 + 36 + 9, len(head) + 6 + 36 + 9 + 36 + 16]
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.read([0])
    # indexing reads lines only: with `read` / `readinto` of the file forbidden, a file opens and counts its frames
    class LinesOnly:
        def __init__(self, f):
            self.f = f

        def __getattr__(self, name):
            if name in ("read", "readinto", "readall"):
                raise AssertionError(f"the index called {name}")
            return getattr(self.f, name)

    monkeypatch.setattr(demux, "open", lambda *a, **k: LinesOnly(open(*a, **k)), raising=False)
    assert len(demux.Y4MReader(path)) == 3


def test_header_forms():
    h = demux.parse_y4m_header("YUV4MPEG2 W320 H240 F25:1\n")
    assert (h.W, h.H, h.fps, h.interlace, h.siting, h.full_range, h.x_tags) == (320, 240, (25, 1), "p", "centre", False, {})
    assert demux.parse_y4m_header(b"YUV4MPEG2 W2 H2 I? C420 F0:0").interlace == "?"
    assert demux.parse_y4m_header("YUV4MPEG2 H3 W5 Ip A4:3 C420jpeg").aspect == "4:3"
    assert demux.parse_y4m_header("YUV4MPEG2 W5 H3 C420mpeg2").siting == "left"
    assert demux.parse_y4m_header("YUV4MPEG2 W5 H3 XCOLORRANGE=FULL").full_range
    for tag in ("It", "Ib", "Im"):
        with pytest.raises(SystemExit, match=f"a.y4m: tag {tag}: interlaced"):
            demux.parse_y4m_header(f"YUV4MPEG2 W4 H4 {tag} C420jpeg", "a.y4m")
    for tag in ("C420paldv", "C422", "C444", "Cmono", "C420p10", "C420p12", "C422p10", "C444p16", "C444alpha", "Cmono16"):
        with pytest.raises(SystemExit, match=f"b.y4m: tag {tag}: only 8-bit 4:2:0"):
            demux.parse_y4m_header(f"YUV4MPEG2 W4 H4 Ip {tag}", "b.y4m")
    with pytest.raises(SystemExit, match="c.y4m: tag XCOLORRANGE=WIDE"):
        demux.parse_y4m_header("YUV4MPEG2 W4 H4 XCOLORRANGE=WIDE", "c.y4m")
    with pytest.raises(SystemExit, match="no frame size"):
        demux.parse_y4m_header("YUV4MPEG2 W4 F25:1", "d.y4m")
    with pytest.raises(SystemExit, match="'Wx' does not parse"):
        demux.parse_y4m_header("YUV4MPEG2 Wx H4", "e.y4m")
    with pytest.raises(SystemExit, match="not a YUV4MPEG2 stream"):
        demux.parse_y4m_header("RIFF W4 H4", "f.y4m")


def test_reader_refusals_name_the_frame(tmp_path):
    W, H = 6, 4
    i420 = dm.patterns(3, W, H)["noise"]
    path = str(tmp_path / "t.y4m")
    write_y4m(path, i420, W, H)
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) - 5)
    with pytest.raises(SystemExit, match=r"t.y4m: frame 2 is truncated: 31 of 36 bytes \(6 x 4"):
        demux.Y4MReader(path)
    write_y4m(path, i420, W, H, marker=b"FRAMF\n")
    with pytest.raises(SystemExit, match="t.y4m: frame 0: no FRAME marker at byte"):
        demux.Y4MReader(path)
    with open(path, "wb") as f:
        f.write(mux.y4m_header(W, H) + b"FRAME\n" + i420[0].tobytes() + b"junk" + b"FRAME\n" + i420[1].tobytes())
    with pytest.raises(SystemExit, match="frame 1: no FRAME marker"):
        demux.Y4MReader(path)
    with open(path, "wb") as f:
        f.write(b"\x00\x00\x00\x20ftypisom\x00\x00\x02\x00isomiso2avc1mp41" + bytes(5000))
    with pytest.raises(SystemExit) as e:
        demux.Y4MReader(path)
    assert "does not start with 'YUV4MPEG2'" in str(e.value) and "container" in str(e.value)
    assert "ffmpeg -i in.mp4 -pix_fmt yuv420p clip.y4m" in str(e.value)
    write_y4m(path, i420, W, H, header=b"YUV4MPEG2 W6 H4 It C420jpeg\n")
    with pytest.raises(SystemExit, match="t.y4m: tag It: interlaced"):
        demux.Y4MReader(path)
    write_y4m(path, i420, W, H, header=b"YUV4MPEG2 W6 H4 Ip C420p10\n")
    with pytest.raises(SystemExit, match="t.y4m: tag C420p10"):
        demux.Y4MReader(path)
    with pytest.raises(SystemExit, match="no such file"):
        demux.Y4MReader(str(tmp_path / "nowhere.y4m"))
    write_y4m(path, i420[:0], W, H)                     # a header and nothing else: an empty clip, not an error
    assert len(demux.Y4MReader(path)) == 0


# ---- the command line
BASE = ["--src_image", "s.png", "--landmarks", "l.npz", "--synthetic_weights"]


def test_new_flags_parse_and_depend_on_each_other():
    p = cli.build_parser()
    none = p.parse_args([])
    assert (none.target_video, none.video_in_matrix, none.chroma_upsample) == (None, None, None)
    opt = p.parse_args(["--target_video", "c.y4m", "--video_in_matrix", "bt601", "--chroma_upsample", "nearest"] + BASE)
    assert (opt.target_video, opt.video_in_matrix, opt.chroma_upsample) == ("c.y4m", "bt601", "nearest")
    cli.check_clip_options(opt)
    assert all(getattr(opt, name) for name in cli.CLIP_STAGES)
    opt = cli.normalise_options(p.parse_args(["--target_video", "c.y4m"] + BASE))
    cli.check_options(opt)
    with pytest.raises(SystemExit):
        p.parse_args(["--video_in_matrix", "bt2020"])
    with pytest.raises(SystemExit):
        p.parse_args(["--chroma_upsample", "bicubic"])
    with pytest.raises(SystemExit) as e:
        cli.main(["--target_video", "c.y4m", "--target_frames", "d"] + BASE)
    assert str(e.value) == "--target_video and --target_frames both name the target clip: give one of them"
    for flag, value in (("video_in_matrix", "bt709"), ("chroma_upsample", "sited")):
        for more in (["--target_frames", "d"] + BASE, ["--synthetic"]):
            with pytest.raises(SystemExit) as e:
                cli.main([f"--{flag}", value] + more)
            assert str(e.value) == f"--{flag} says how --target_video is converted: it needs --target_video FILE.y4m"
        with pytest.raises(SystemExit, match=f"--{flag} says how --target_video is converted"):
            cli.check_clip_options(p.parse_args([f"--{flag}", value, "--target_frames", "d"] + BASE))
    with pytest.raises(SystemExit, match="a real-clip run needs --src_image"):
        cli.main(["--target_video", "c.y4m", "--landmarks", "l.npz"])
    with pytest.raises(SystemExit, match="a real-clip run needs --ckpt"):
        cli.main(["--target_video", "c.y4m", "--src_image", "s.png", "--landmarks", "l.npz"])


def test_neither_source_keeps_its_message_byte_for_byte():
    with pytest.raises(SystemExit) as e:
        cli.main([])
    assert str(e.value) == ("a real-clip run needs --target_frames (frames, source image and landmarks come from disk; dlib and the "
                            "video decoder are outside this build, INTEGRATION.md), or run the seeded stand-ins with --synthetic")


# ---- ClipInputs over a reader
def test_clip_inputs_over_a_reader_equal_the_folder_form(tmp_path):
    """The same 5-frame clip as a .y4m and as the PNG files of its decoded frames: ids, quads, coeffs, landmarks, found and source
    are equal, the batches carry the file's I420 rows, and frame 2 -- without landmarks, first of batch 1 -- is cut from frame 1,
    which is read AGAIN by seek (it lies in batch 0)."""
    W, H = 320, 240
    rng = np.random.default_rng(0)
    i420 = mm.rgb_to_i420(rng.integers(0, 256, (5, H, W, 3), dtype=np.uint8))
    vpath = str(tmp_path / "clip.y4m")
    write_y4m(vpath, i420, W, H)
    rgb = dm.i420_to_rgb(i420, W, H)
    (tmp_path / "f").mkdir()
    for i in range(5):
        Image.fromarray(rgb[i]).save(tmp_path / "f" / f"{i}.png")
    Image.fromarray(rgb[0, :100, :90]).save(tmp_path / "src.png")
    lpath = str(tmp_path / "lm.npz")
    landmark_file(lpath)
    folder = clip_io.ClipInputs(str(tmp_path / "f"), str(tmp_path / "src.png"), lpath, 4, 512, 512)
    reader = demux.Y4MReader(vpath)
    reads = []
    real_read = reader.read
    reader.read = lambda idx: reads.append(list(idx)) or real_read(idx)
    video = clip_io.ClipInputs.from_video(reader, str(tmp_path / "src.png"), lpath, 4, 512, 512)
    assert folder.video is None and video.video is reader and video.size == (H, W)
    assert video.frame_ids == folder.frame_ids == [0, 1, 2, 3]
    for name in ("quads", "coeffs", "landmarks", "found", "take", "source_quad", "source_landmarks"):
        assert np.array_equal(getattr(video, name), getattr(folder, name)), name
    assert torch.equal(video.source_u8, folder.source_u8)
    for k in range(2):
        bv, bf = video.batch(k, 2), folder.batch(k, 2)
        assert bv["frame_ids"] == bf["frame_ids"]
        for name in ("quads", "coeffs", "landmarks", "found"):
            assert np.array_equal(bv[name], bf[name]), name
        assert bv["frames"].dtype == torch.uint8 and np.array_equal(bv["frames"].numpy(), i420[2 * k:2 * k + 2])
        assert np.array_equal(dm.i420_to_rgb(bv["frames"].numpy(), W, H), bf["frames"].numpy())
        assert np.array_equal(dm.i420_to_rgb(bv["crop_frames"].numpy(), W, H), bf["crop_frames"].numpy())
    assert reads == [[0, 1], [2, 3], [1]]
    assert np.array_equal(video.batch(1, 2)["crop_frames"].numpy(), i420[[1, 3]])
    one = video.batch(0, 4)       # the same fallback inside one batch: nothing is read twice
    assert np.array_equal(one["crop_frames"].numpy(), i420[[0, 1, 1, 3]]) and reads[-1] == [0, 1, 2, 3]
    with pytest.raises(SystemExit) as e:
        clip_io.ClipInputs.from_video(reader, str(tmp_path / "src.png"), lpath, 6, 512, 512)
    assert "5 frame(s), --n_frames asks for 6" in str(e.value) and "--target_video" in str(e.value)
