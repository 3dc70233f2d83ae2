"""vface_rgb_to_yuv420 (csrc/mux.hip) against its integer model (tests/mux_model.py), bit for bit in all three planes, and the
YUV4MPEG2 writer of vface_amd/scripts/mux.py on the device."""
import numpy as np
import pytest
import torch

import mux_model as mm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = 0xA5
GRID_CAP = 2048         # kMuxGridCap of csrc/mux.hip: workgroups of 256 strips (2 rows x 16 pixels each) before the grid loops


def convert_in_sentinel(rgb: np.ndarray, gap: int, lead: int = 0):
    """The kernel's output for ``rgb`` written at byte ``lead`` of a buffer of SENTINEL bytes, frames ``frame_bytes + gap`` apart.
    Returns (planes uint8 [F, frame_bytes], the whole buffer) on the host."""
    from vface_amd import hip
    F, H, W, _ = rgb.shape
    n = mm.frame_bytes(W, H)
    stride = n + gap
    buf = torch.full((lead + F * stride + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = buf[lead:lead + F * stride].view(F, stride)[:, :n]
    out = hip.rgb_to_yuv420(torch.from_numpy(rgb).to(DEV), out=view)
    assert out.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    return whole[lead:lead + F * stride].reshape(F, stride)[:, :n], whole, stride


@pytest.mark.parametrize("W,H", mm.SIZES)
@pytest.mark.parametrize("F", [1, 3])
def test_kernel_equals_model(W, H, F):
    """Every size of the issue (odd sides, tails of the 16-pixel strip, more than one strip and row pair), 1 and 3 frames, every
    input pattern; the frames lie inside a sentinel buffer with a gap between them, and nothing outside the planes is written.
    ``lead`` walks the output through every byte alignment the stores choose between."""
    for i, (name, rgb) in enumerate(mm.patterns(F, W, H).items()):
        gap, lead = (0, 0) if i == 0 else (5 + 8 * i, i)
        got, whole, stride = convert_in_sentinel(rgb, gap, lead)
        mm.check_i420(got, rgb, f"{name} F={F}")
        n = mm.frame_bytes(W, H)
        mask = np.ones(whole.shape, bool)
        for f in range(F):
            mask[lead + f * stride:lead + f * stride + n] = False
        assert (whole[mask] == SENTINEL).all(), f"{name}: bytes outside the frames were written"


@pytest.mark.parametrize("W", [16, 17, 18, 19, 33, 48])
def test_rows_at_every_alignment(W):
    """W * 3 % 4 != 0 for W = 17, 18, 19, 33: with 9 rows the rows of the input start on every residue mod 4 (and mod 16), those of
    Y on every residue of W; W = 16 and 48 are the all-wide case.  Dense output (the default `out`)."""
    from vface_amd import hip
    H = 9
    rgb = mm.patterns(2, W, H, seed=7)["noise"]
    if W in (17, 18, 19, 33):
        assert (W * 3) % 4 != 0 and len({(y * W * 3) % 4 for y in range(H)}) > 1
    got = hip.rgb_to_yuv420(torch.from_numpy(rgb).to(DEV))
    assert got.shape == (2, mm.frame_bytes(W, H)) and got.is_contiguous()
    mm.check_i420(got.cpu().numpy(), rgb, f"W={W}")


def test_past_the_grid_cap():
    """More strips than GRID_CAP * 256 threads, so the first threads loop: 3 pixels wide (one strip per row pair) and tall."""
    items = GRID_CAP * 256 + 101
    W, H = 3, 2 * items - 1
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    got, whole, _ = convert_in_sentinel(rgb, 0)
    mm.check_i420(got, rgb, "past the cap")
    assert (whole[mm.frame_bytes(W, H):] == SENTINEL).all()


def test_wrapper_refuses_what_it_cannot_run():
    from vface_amd import hip
    ok = torch.zeros(2, 4, 6, 3, dtype=torch.uint8, device=DEV)
    n = mm.frame_bytes(6, 4)
    for bad in (ok.cpu(), ok.float(), ok[..., :2], ok.permute(0, 2, 1, 3)):
        with pytest.raises(hip.VFaceHipError):
            hip.rgb_to_yuv420(bad)
    for bad_out in (torch.zeros(2, n - 1, dtype=torch.uint8, device=DEV), torch.zeros(2, n, dtype=torch.uint8),
                    torch.zeros(2, 2 * n, dtype=torch.uint8, device=DEV)[:, ::2], torch.zeros(n, 2, dtype=torch.uint8, device=DEV).t()):
        with pytest.raises(hip.VFaceHipError):
            hip.rgb_to_yuv420(ok, out=bad_out)


def test_y4m_writer_writes_what_the_kernel_makes(tmp_path):
    from vface_amd import hip
    from vface_amd.scripts import mux
    W, H = 66, 34
    rgb = torch.from_numpy(mm.patterns(3, W, H, seed=9)["noise"]).to(DEV)
    path = str(tmp_path / "clip.y4m")
    with mux.Y4MWriter(path, W, H) as w:
        assert w.write(rgb[:2]) == 2 and w.write(rgb[2:]) == 1 and w.frames == 3
        with pytest.raises(hip.VFaceHipError):
            w.write(rgb[:, :, :-1])
        with pytest.raises(hip.VFaceHipError):
            w.write(rgb.cpu())
    tags, frames = mm.read_y4m(path)
    assert (tags["W"], tags["H"], tags["F"], tags["C"], tags["COLORRANGE"]) == ("66", "34", "10:1", "420jpeg", "LIMITED")
    assert np.array_equal(frames, hip.rgb_to_yuv420(rgb).cpu().numpy())
    mm.check_i420(frames, rgb.cpu().numpy(), "file")
