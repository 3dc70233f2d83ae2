"""A CPU model (torch fp32) of the rounding points of ``vface_flow_warp`` (csrc/pointwise.hip) on the flat buffers the kernel is
given -- element offsets, leading dimensions and frame strides as the launcher takes them -- plus seeded DEFECTS of one line each
and the flow families of the warp tests.  It restates the kernel in torch: it is not a reference (that is the fp64 warp of
``kernel_bounds.flow_warp_ref_and_bound``) -- it shows that the bound admits a correct kernel and refuses a subtly wrong one
(test_hook_bound_cpu.py).  Plain module, nothing collected by pytest.

What is modelled: the coordinate in the reference's fp32 operation order (x + dx; 2 v / max(W - 1, 1) - 1 as a true division or
as a product with the fp32 reciprocal; ((g + 1) / 2) (W - 1); clamp; floor), the neighbour index min(x0 + 1, W - 1), four fp32
weights, the fp32 sum of four products, alpha * x rounded to the storage type, fp32(1 - alpha) * warp added in fp32, one rounding.
An element index past the end of a buffer reads NaN, like the poison the GPU tests lay behind every frame.
Not modelled: the contraction of products and sums into fused multiply-adds."""
import torch

DEFECTS = ("xy_swapped", "neighbour_unclamped", "ax_unrounded", "frame_f", "ld_prev_as_ld_src", "recip_for_true")
FAMILIES = ("smooth", "integer", "outside_left", "outside_right", "outside_up", "outside_down", "on_edge")


def _coord(pos, d, size, recip):
    v = pos + d
    den = torch.tensor(float(max(size - 1, 1)), dtype=torch.float32)
    qn = (2.0 * v) * (torch.tensor(1.0, dtype=torch.float32) / den) if recip else (2.0 * v) / den
    return torch.clamp(((qn - 1.0) + 1.0) * 0.5 * float(size - 1), 0.0, float(size - 1))


def _rows(buf, base, ld, pix, C):
    idx = base + pix.reshape(-1, 1).long() * ld + torch.arange(C)
    ok = (idx >= 0) & (idx < buf.numel())
    got = buf[idx.clamp(0, buf.numel() - 1)].float()
    return torch.where(ok, got, torch.full_like(got, float("nan")))


def flow_warp_model(src, src_off, ld_src, fs_src, flow, *, F, h, w, C, alpha, prev=None, prev_off=0, ld_prev=0, flow_prev=None,
                    recip=False, defect=None):
    """``src``, ``prev``: flat 16-bit CPU buffers; ``flow [F - 1, 2, h, w]``, ``flow_prev [2, h, w]`` fp32.  Returns ``(out [F, h w, C]``
    of the storage type, ``x0, y0 [F - 1, h, w]`` int32): what the kernel stores and what it reports through dbg_x0 / dbg_y0."""
    assert defect is None or defect in DEFECTS
    dt = src.dtype
    hw = h * w
    pix = torch.arange(hw)
    py, px = pix // w, pix % w
    a32, oma32 = torch.tensor(alpha, dtype=torch.float32), torch.tensor(1.0 - alpha, dtype=torch.float32)
    if defect == "recip_for_true":
        recip = True
    pitch = h if defect == "xy_swapped" else w
    out, X0, Y0 = [], [], []
    for f in range(F):
        cur = _rows(src, src_off + f * fs_src, ld_src, pix, C)
        if f > 0:
            buf, base, ld, fl = src, src_off + (f if defect == "frame_f" else f - 1) * fs_src, ld_src, flow[f - 1]
        elif prev is not None:
            buf, base, ld, fl = prev, prev_off, (ld_src if defect == "ld_prev_as_ld_src" else ld_prev), flow_prev
        else:
            out.append(cur.to(dt))
            continue
        ix, iy = _coord(px.float(), fl[0].reshape(-1), w, recip), _coord(py.float(), fl[1].reshape(-1), h, recip)
        fx0, fy0 = torch.floor(ix), torch.floor(iy)
        x0, y0 = fx0.long(), fy0.long()
        if f > 0:
            X0.append(x0.int().reshape(h, w))
            Y0.append(y0.int().reshape(h, w))
        wx1, wy1 = ix - fx0, iy - fy0
        wx0, wy0 = 1.0 - wx1, 1.0 - wy1
        x1, y1 = (x0 + 1, y0 + 1) if defect == "neighbour_unclamped" else (torch.clamp(x0 + 1, max=w - 1), torch.clamp(y0 + 1, max=h - 1))
        wv = _rows(buf, base, ld, y0 * pitch + x0, C) * (wx0 * wy0)[:, None]
        wv = wv + _rows(buf, base, ld, y0 * pitch + x1, C) * (wx1 * wy0)[:, None]
        wv = wv + _rows(buf, base, ld, y1 * pitch + x0, C) * (wx0 * wy1)[:, None]
        wv = wv + _rows(buf, base, ld, y1 * pitch + x1, C) * (wx1 * wy1)[:, None]
        ax = a32 * cur
        if defect != "ax_unrounded":
            ax = ax.to(dt).float()
        out.append((ax + oma32 * wv).to(dt))
    idx = (torch.stack(X0), torch.stack(Y0)) if X0 else (None, None)
    return (torch.stack(out),) + idx


def make_flow(family, nf, h, w, seed=0):
    """``[nf, 2, h, w]`` fp32 flow fields of one family:
    smooth -- sub-pixel, slowly varying; integer -- whole cells in -3 .. 3 (the coordinate sits on the floor() boundary);
    outside_left / right / up / down -- every pixel points past that side by 2 .. 4 cells, the other component sub-pixel: the
    border clamp, and on the right / bottom the neighbour min(x0 + 1, w - 1) with weight zero; on_edge -- ix exactly w - 1 for
    every pixel, iy exactly h - 1 in the lower half of the map."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * h + w)
    xs = torch.arange(w, dtype=torch.float32).view(1, 1, w).expand(nf, h, w)
    ys = torch.arange(h, dtype=torch.float32).view(1, h, 1).expand(nf, h, w)
    ph = torch.rand((nf, 1, 1), generator=g) * 6.28
    sx = 0.45 * torch.sin(xs * 0.31 + ys * 0.17 + ph) + 0.3 * torch.rand((nf, h, w), generator=g)
    sy = 0.45 * torch.cos(xs * 0.13 - ys * 0.29 + ph) - 0.3 * torch.rand((nf, h, w), generator=g)
    far = 2.0 + 2.0 * torch.rand((nf, h, w), generator=g)
    if family == "smooth":
        dx, dy = sx, sy
    elif family == "integer":
        dx = torch.randint(-3, 4, (nf, h, w), generator=g).float()
        dy = torch.randint(-3, 4, (nf, h, w), generator=g).float()
    elif family == "outside_left":
        dx, dy = -(xs + far), sy
    elif family == "outside_right":
        dx, dy = (w - 1 - xs) + far, sy
    elif family == "outside_up":
        dx, dy = sx, -(ys + far)
    elif family == "outside_down":
        dx, dy = sx, (h - 1 - ys) + far
    elif family == "on_edge":
        dx = (w - 1) - xs
        dy = torch.where(ys >= h // 2, (h - 1) - ys, sy)
    else:
        raise ValueError(family)
    return torch.stack([dx, dy], 1).contiguous()


def make_frames(nf, hw, C, dt, seed):
    """``[nf, hw, C]`` of type ``dt``, every frame drawn with its own scale and offset: a warp from another frame than the previous
    one lands far outside the bound."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((nf, hw, C), generator=g)
    sc = (0.6 + 0.45 * torch.arange(nf, dtype=torch.float32)).view(nf, 1, 1)
    return (x * sc + 0.25 * (torch.arange(nf, dtype=torch.float32).view(nf, 1, 1) - 1.0)).to(dt)


def lay_frames(x, ld, gap_rows, off, fill=float("nan")):
    """``x [nf, rows, C]`` laid into a flat buffer filled with ``fill``: ``(buffer, off, ld, frame stride)``; ``gap_rows`` rows of
    fill lie right behind every frame, ``ld - C`` elements of it behind every row."""
    nf, rows, C = x.shape
    fs = (rows + gap_rows) * ld
    buf = torch.full((off + nf * fs + 8,), fill, dtype=x.dtype)
    buf[off:off + nf * fs].as_strided((nf, rows, C), (fs, ld, 1)).copy_(x)
    return buf, off, ld, fs
