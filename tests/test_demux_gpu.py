"""vface_yuv420_to_rgb (csrc/demux.hip) against its integer model (tests/demux_model.py), bit for bit, and the YUV4MPEG2 reader of
vface_amd/scripts/demux.py feeding it."""
import numpy as np
import pytest
import torch

import demux_model as dm
import mux_model as mm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL, POISON = 0xA5, 0x5A
GRID_CAP = 2048         # kDemuxGridCap of csrc/demux.hip: workgroups of 256 strips (2 rows x 16 pixels each) before the grid loops


def convert_between_poison_and_sentinel(i420: np.ndarray, W: int, H: int, gap: int, lead: int, **how):
    """The kernel's output for ``i420`` [F, frame_bytes]: the frames lie ``frame_bytes + gap`` apart from byte ``lead`` of a buffer
    of POISON bytes, the dense RGB output is a view at byte ``lead`` of a buffer of SENTINEL bytes.  Returns (rgb [F, H, W, 3], the
    whole output buffer) on the host."""
    from vface_amd import hip
    F, n = i420.shape[0], mm.frame_bytes(W, H)
    stride = n + gap
    src = torch.full((lead + F * stride + 64,), POISON, dtype=torch.uint8, device=DEV)
    rows = src[lead:lead + F * stride].view(F, stride)[:, :n]
    rows.copy_(torch.from_numpy(i420[:, :n]))
    nout = F * H * W * 3
    buf = torch.full((lead + nout + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = buf[lead:lead + nout].view(F, H, W, 3)
    out = hip.yuv420_to_rgb(rows, W, H, out=view, **how)
    assert out.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    return whole[lead:lead + nout].reshape(F, H, W, 3), whole


def untouched(whole, lead, nout):
    return (whole[:lead] == SENTINEL).all() and (whole[lead + nout:] == SENTINEL).all()


@pytest.mark.parametrize("W,H", mm.SIZES)
@pytest.mark.parametrize("F", [1, 3])
def test_kernel_equals_model(W, H, F):
    """Every size of the mux's list (odd sides, tails of the 16-pixel strip, more than one strip and row pair), 1 and 3 frames, every
    pattern, all three chroma modes.  Poison between and around the input frames never reaches an output (the model knows nothing
    of it); nothing outside the output view is written.  ``lead`` walks both buffers through the alignments the accesses choose
    between."""
    for i, (name, i420) in enumerate(dm.patterns(F, W, H).items()):
        gap, lead = (0, 0) if i == 0 else (5 + 8 * i, i)
        for chroma in dm.CHROMA_MODES:
            got, whole = convert_between_poison_and_sentinel(i420, W, H, gap, lead, chroma=chroma)
            dm.check_rgb(got, i420, W, H, chroma=chroma, what=f"{name} F={F}")
            assert untouched(whole, lead, F * H * W * 3), f"{name} {chroma}: bytes outside the frames were written"


@pytest.mark.parametrize("W,H", [(7, 5), (66, 34)])
@pytest.mark.parametrize("matrix,full_range", dm.TABLES)
def test_all_four_tables(W, H, matrix, full_range):
    i420 = dm.patterns(2, W, H, seed=3)["noise"]
    for chroma in dm.CHROMA_MODES:
        got, whole = convert_between_poison_and_sentinel(i420, W, H, 7, 3, matrix=matrix, full_range=full_range, chroma=chroma)
        dm.check_rgb(got, i420, W, H, matrix, full_range, chroma, what="tables")
        assert untouched(whole, 3, 2 * H * W * 3)


@pytest.mark.parametrize("W", [16, 17, 18, 19, 33, 48])
def test_rows_at_every_alignment(W):
    """W * 3 % 4 != 0 for W = 17, 18, 19, 33: with 9 rows the output rows start on every residue mod 4 (and mod 16), the Y rows on
    every residue of W, the chroma rows on those of (W + 1) / 2; W = 16 and 48 are the all-wide case.  Dense default output."""
    from vface_amd import hip
    H = 9
    i420 = dm.patterns(2, W, H, seed=7)["noise"]
    if W in (17, 18, 19, 33):
        assert (W * 3) % 4 != 0 and len({(y * W * 3) % 4 for y in range(H)}) > 1
    for chroma in dm.CHROMA_MODES:
        got = hip.yuv420_to_rgb(torch.from_numpy(i420).to(DEV), W, H, chroma=chroma)
        assert got.shape == (2, H, W, 3) and got.is_contiguous() and got.dtype == torch.uint8
        dm.check_rgb(got.cpu().numpy(), i420, W, H, chroma=chroma, what=f"W={W}")


def test_past_the_grid_cap():
    """More strips than GRID_CAP * 256 threads, so the first threads loop: 3 pixels wide (one strip per row pair) and tall."""
    items = GRID_CAP * 256 + 101
    W, H = 3, 2 * items - 1
    rng = np.random.default_rng(5)
    i420 = rng.integers(0, 256, (1, mm.frame_bytes(W, H)), dtype=np.uint8)
    got, whole = convert_between_poison_and_sentinel(i420, W, H, 0, 0)
    dm.check_rgb(got, i420, W, H, what="past the cap")
    assert untouched(whole, 0, H * W * 3)


def test_wrapper_refuses_what_it_cannot_run():
    from vface_amd import hip
    W, H = 6, 4
    n = mm.frame_bytes(W, H)
    ok = torch.zeros(2, n, dtype=torch.uint8, device=DEV)
    assert tuple(hip.yuv420_to_rgb(ok, W, H).shape) == (2, H, W, 3)
    assert tuple(hip.yuv420_to_rgb(torch.zeros(2, 2 * n, dtype=torch.uint8, device=DEV)[:, :n + 3], W, H).shape) == (2, H, W, 3)
    for bad in (ok.cpu(), ok.float(), ok.to(torch.int8), ok[:, :n - 1], ok.view(2, n, 1), ok[0],
                torch.zeros(2, 2 * n, dtype=torch.uint8, device=DEV)[:, ::2], torch.zeros(n, 2, dtype=torch.uint8, device=DEV).t(),
                ok[:0]):
        with pytest.raises(hip.VFaceHipError):
            hip.yuv420_to_rgb(bad, W, H)
    for bad_out in (torch.zeros(2, H, W, 3, dtype=torch.uint8), torch.zeros(2, W, H, 3, dtype=torch.uint8, device=DEV),
                    torch.zeros(2, H, W, 4, dtype=torch.uint8, device=DEV)[..., :3], torch.zeros(2, H, W, 3, device=DEV),
                    torch.zeros(2, H, 2 * W, 3, dtype=torch.uint8, device=DEV)[:, :, ::2]):
        with pytest.raises(hip.VFaceHipError):
            hip.yuv420_to_rgb(ok, W, H, out=bad_out)
    for how in (dict(matrix="bt2020"), dict(chroma="bicubic"), dict(matrix=0), dict(chroma="sited")):
        with pytest.raises(hip.VFaceHipError):
            hip.yuv420_to_rgb(ok, W, H, **how)
    for W_, H_ in ((0, 4), (6, 0), (6, 5)):        # (6 x 5 needs more bytes than the rows have)
        with pytest.raises(hip.VFaceHipError):
            hip.yuv420_to_rgb(ok, W_, H_)
    # the C entry point itself: a stride below frame_bytes is VFACE_ERR_SHAPE, an unknown code VFACE_ERR_ARG; nothing is launched
    lib, out = hip.load(), torch.zeros(2, H, W, 3, dtype=torch.uint8, device=DEV)
    assert lib.vface_yuv420_to_rgb(ok.data_ptr(), n - 1, W, H, 2, out.data_ptr(), 0, 0, 1, None) == -3
    assert lib.vface_yuv420_to_rgb(ok.data_ptr(), n, W, H, 2, out.data_ptr(), 2, 0, 1, None) == -1
    assert lib.vface_yuv420_to_rgb(ok.data_ptr(), n, W, H, 2, out.data_ptr(), 0, 0, 3, None) == -1


def test_device_round_trip_with_the_mux():
    """rgb -> hip.rgb_to_yuv420 -> hip.yuv420_to_rgb on an image that is constant on every 2 x 2 block (so `nearest` puts every
    pixel's own chroma back): within the 2 levels the two models' round trip allows (tests/test_demux_cpu.py)."""
    from vface_amd import hip
    rng = np.random.default_rng(2)
    blocks = rng.integers(0, 256, (2, 17, 33, 3), dtype=np.uint8)
    rgb = torch.from_numpy(np.repeat(np.repeat(blocks, 2, axis=1), 2, axis=2)).to(DEV)
    H, W = rgb.shape[1:3]
    back = hip.yuv420_to_rgb(hip.rgb_to_yuv420(rgb), W, H, chroma="nearest")
    assert int((back.int() - rgb.int()).abs().max()) <= 2


def test_reader_plus_kernel(tmp_path):
    """A file as scripts/mux.py frames it, read by Y4MReader in another order, converted as its header says: the model of its planes."""
    from vface_amd import hip
    from vface_amd.scripts import demux, mux
    W, H = 66, 34
    i420 = dm.patterns(3, W, H, seed=9)["noise"]
    path = str(tmp_path / "clip.y4m")
    with open(path, "wb") as f:
        f.write(mux.y4m_header(W, H) + mux.y4m_frames(i420, W, H))
    with demux.Y4MReader(path) as r:
        rows = r.read([2, 0, 1])
        got = hip.yuv420_to_rgb(rows.to(DEV), r.W, r.H, full_range=r.header.full_range, chroma=r.header.siting)
    dm.check_rgb(got.cpu().numpy(), i420[[2, 0, 1]], W, H, what="file")
