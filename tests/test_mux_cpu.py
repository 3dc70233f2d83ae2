"""The mux's integer colour model (tests/mux_model.py) against its fp64 definition, its seeded defects against the assertion the
GPU test uses, and the YUV4MPEG2 framing of vface_amd/scripts/mux.py -- all without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import mux_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_colours():
    """Every 8-bit colour, one red level at a time: (r, g [65536], b [65536])."""
    g, b = (v.reshape(-1) for v in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    for r in range(256):
        yield np.full_like(g, r), g, b


def test_coefficients_are_the_rounded_bt709_limited_range_rows():
    assert list(mm.LUMA) == [11966, 40254, 4064] and mm.Y_OFFSET == 16       # the plainly rounded luma row
    assert mm.CB.sum() == 0 and mm.CR.sum() == 0
    one = 65536.0
    for got, exact in ((mm.LUMA, 219 / 255 * np.array([0.2126, 0.7152, 0.0722])),
                       (mm.CB, 224 / 255 * np.array([-0.2126, -0.7152, 0.9278]) / 1.8556),
                       (mm.CR, 224 / 255 * np.array([0.7874, -0.7152, -0.0722]) / 1.5748)):
        assert np.abs(got - one * exact).max() < 1.0        # (0.5 from rounding; the zero-sum residual moves one entry further)


def test_kernel_source_carries_the_models_tables():
    src = open(os.path.join(ROOT, "vface_amd", "csrc", "mux.hip")).read()
    for name, row in (("kLuma", mm.LUMA), ("kCb", mm.CB), ("kCr", mm.CR)):
        m = re.search(r"constexpr int %s\[3\] = \{(-?\d+), (-?\d+), (-?\d+)\};" % name, src)
        assert m and [int(v) for v in m.groups()] == list(row), name


def test_model_stays_within_a_level_of_fp64_over_all_colours():
    """All 2^24 colours: single pixels for luma, uniform 2 x 2 blocks (sums of four equal pixels) for chroma.  The integer result is
    never a full level away from the unrounded fp64 definition; greys have no chroma; the extremes need no clamp."""
    worst = {"y": 0.0, "cb": 0.0, "cr": 0.0}
    lo = {"y": 255, "cb": 255, "cr": 255}
    hi = {"y": 0, "cb": 0, "cr": 0}
    for r, g, b in _all_colours():
        ey, ecb, ecr = mm.fp64_definition(r, g, b)
        got = {"y": mm.luma_from_rgb(r, g, b), "cb": mm.chroma_from_sums(4 * r, 4 * g, 4 * b, 2, mm.CB),
               "cr": mm.chroma_from_sums(4 * r, 4 * g, 4 * b, 2, mm.CR)}
        for k, e in (("y", ey), ("cb", ecb), ("cr", ecr)):
            worst[k] = max(worst[k], float(np.abs(got[k] - e).max()))
            lo[k], hi[k] = min(lo[k], int(got[k].min())), max(hi[k], int(got[k].max()))
        grey = (g == r) & (b == r)
        assert (got["cb"][grey] == 128).all() and (got["cr"][grey] == 128).all()
        # blocks of 2 and of 1 scale every term of the sum alike: the same sample
        assert np.array_equal(mm.chroma_from_sums(2 * r, 2 * g, 2 * b, 1, mm.CB), got["cb"])
        assert np.array_equal(mm.chroma_from_sums(r, g, b, 0, mm.CR), got["cr"])
    print("worst |integer - fp64|:", worst, "ranges:", lo, hi)
    assert max(worst.values()) < 1.0, worst
    assert (lo["y"], hi["y"]) == (16, 235) and lo["cb"] >= 16 and hi["cb"] <= 240 and lo["cr"] >= 16 and hi["cr"] <= 240
    rng = mm.value_ranges()
    assert rng["y"] == (lo["y"], hi["y"]) and rng["cb"] == (lo["cb"], hi["cb"]) and rng["cr"] == (lo["cr"], hi["cr"])
    assert max(rng["y_peak"], rng["cb_peak"], rng["cr_peak"]) < 2 ** 31


def test_black_white_and_greys():
    px = lambda v: np.full((1, 2, 2, 3), v, np.uint8)
    assert list(mm.rgb_to_i420(px(0))[0]) == [16, 16, 16, 16, 128, 128]
    assert list(mm.rgb_to_i420(px(255))[0]) == [235, 235, 235, 235, 128, 128]
    for v in range(256):
        assert tuple(mm.rgb_to_i420(px(v)[:, :1, :1])[0][1:]) == (128, 128)


def test_block_mean_uses_the_pixels_that_exist():
    """3 x 3: a full block, a 2-pixel block on the last column, one on the last row, the single corner pixel."""
    rgb = np.random.default_rng(3).integers(0, 256, (1, 3, 3, 3), dtype=np.uint8)
    y, cb, cr = mm.planes(mm.rgb_to_i420(rgb), 3, 3)
    assert y.shape == (1, 3, 3) and cb.shape == cr.shape == (1, 2, 2)
    for (by, bx), (ys, xs) in {(0, 0): (slice(0, 2), slice(0, 2)), (0, 1): (slice(0, 2), slice(2, 3)),
                               (1, 0): (slice(2, 3), slice(0, 2)), (1, 1): (slice(2, 3), slice(2, 3))}.items():
        mean = rgb[0, ys, xs].reshape(-1, 3).astype(np.float64).mean(0)
        _, ecb, ecr = mm.fp64_definition(*mean)
        assert abs(cb[0, by, bx] - ecb) < 1.0 and abs(cr[0, by, bx] - ecr) < 1.0


@pytest.mark.parametrize("defect", mm.DEFECTS)
def test_seeded_defects_are_seen_by_the_kernel_tests_assertion(defect):
    """The GPU test asserts ``check_i420(kernel output, input)`` over ``SIZES`` x ``patterns``.  A conversion with one of the seeded
    defects in place of the kernel must fail that same assertion on those same inputs (and the model itself must pass it)."""
    seen = 0
    for W, H in mm.SIZES:
        for name, rgb in mm.patterns(3, W, H).items():
            mm.check_i420(mm.rgb_to_i420(rgb), rgb, name)
            try:
                mm.check_i420(mm.rgb_to_i420(rgb, defect=defect), rgb, name)
            except AssertionError:
                seen += 1
    assert seen > 0, defect
    if defect == "edge_div4":       # only sizes with an odd side have edge blocks; every one of those must show it
        for W, H in [s for s in mm.SIZES if s[0] % 2 or s[1] % 2]:
            rgb = mm.patterns(1, W, H)["noise"]
            with pytest.raises(AssertionError):
                mm.check_i420(mm.rgb_to_i420(rgb, defect=defect), rgb)


@pytest.mark.parametrize("W,H", [(66, 34), (7, 5), (1, 1)])
def test_y4m_file_round_trips(tmp_path, W, H):
    from vface_amd.scripts import mux
    rgb = mm.patterns(3, W, H)["noise"]
    i420 = mm.rgb_to_i420(rgb)
    header = mux.y4m_header(W, H)
    assert header == f"YUV4MPEG2 W{W} H{H} F10:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n".encode()
    body = mux.y4m_frames(torch.from_numpy(i420), W, H)
    n = mm.frame_bytes(W, H)
    assert len(body) == 3 * (6 + n) and body.count(b"FRAME\n") >= 3 and body[:6] == b"FRAME\n" and body[6 + n:12 + n] == b"FRAME\n"
    assert mux.y4m_frames(i420, W, H) == body
    path = tmp_path / "a.y4m"
    path.write_bytes(header + body)
    tags, frames = mm.read_y4m(str(path))
    assert tags == {"W": str(W), "H": str(H), "F": "10:1", "I": "p", "A": "1:1", "C": "420jpeg", "COLORRANGE": "LIMITED"}
    assert np.array_equal(frames, i420)
    assert mux.y4m_header(W, H, fps=25).split()[3] == b"F25:1"
    with pytest.raises(ValueError):
        mux.y4m_frames(i420[:, :-1], W, H)
    with pytest.raises(ValueError):
        mux.y4m_header(0, H)


def test_writer_refuses_cpu_frames(tmp_path):
    from vface_amd import hip
    from vface_amd.scripts import mux
    with mux.Y4MWriter(str(tmp_path / "b.y4m"), 4, 2) as w:
        with pytest.raises(hip.VFaceHipError):
            w.write(torch.zeros(1, 2, 4, 3, dtype=torch.uint8))
    assert (tmp_path / "b.y4m").read_bytes() == mux.y4m_header(4, 2)
    assert mux.Y4MWriter.__init__.__defaults__ == (10,) and hip.i420_frame_bytes(7, 5) == mm.frame_bytes(7, 5) == 35 + 2 * 12


def test_launcher_refuses_bad_arguments_before_any_hip_call():
    from vface_amd import hip
    lib = hip.load()
    buf = (hip.C.c_ubyte * 64)()
    p = hip.C.cast(buf, hip.C.c_void_p)
    call = lib.vface_rgb_to_yuv420
    assert call(None, 2, 2, p, 6, 1, None) == -1 and call(p, 2, 2, None, 6, 1, None) == -1       # VFACE_ERR_ARG
    assert call(p, 0, 2, p, 6, 1, None) == -1 and call(p, 2, 0, p, 6, 1, None) == -1 and call(p, 2, 2, p, 6, 0, None) == -1
    assert call(p, 2, 2, p, 5, 1, None) == -3 and call(p, 3, 3, p, 16, 1, None) == -3              # VFACE_ERR_SHAPE: 6 and 17 needed
