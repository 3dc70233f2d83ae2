"""The colour conversion of the mux, stated once in integers: 8-bit RGB frames -> I420 (``yuv420p``), BT.709, limited (``tv``)
range -- what the reference asks ffmpeg for (``REFace/scripts/VFace_inference_batch.py:646-654``).  ``vface_rgb_to_yuv420``
(csrc/mux.hip) equals ``rgb_to_i420`` bit for bit; this file is also the reader of the YUV4MPEG2 files ``scripts/mux.py`` writes.

Definition (fp64, ITU-R BT.709 with Kr = 0.2126, Kb = 0.0722, 8-bit limited range)::

    Y' = 16  + 219/255 (0.2126 R + 0.7152 G + 0.0722 B)
    Cb = 128 + 224/255 (B - Y'_full) / 1.8556          Y'_full = 0.2126 R + 0.7152 G + 0.0722 B
    Cr = 128 + 224/255 (R - Y'_full) / 1.5748

Integers: every coefficient is the fp64 one times 2^16, rounded to nearest.  A chroma row must sum to zero (a grey has no
chroma); where plain rounding leaves a residual, the coefficient that moves least from its fp64 value takes it.  Results are rounded
half-up: ``(sum + offset << 16 + 1 << 15) >> 16``.  Luma is per pixel.  A chroma sample is the mean of the pixels of its 2 x 2 block
that exist (4; 2 on an odd last column or row; 1 in the odd corner), centre-sited: the R, G, B of those pixels are summed first and
the shift grows by log2 of their number.

No clamp: ``value_ranges()`` bounds every result from the signs of the coefficients -- Y' in [16, 235], Cb and Cr in [16, 240] --
and every intermediate stays inside int32.
"""
from __future__ import annotations

import numpy as np

SHIFT = 16
KR, KB = 0.2126, 0.0722
DEFECTS = ("swap_rb", "full_range", "truncate", "edge_div4", "swap_planes")


def _zero_sum(x):
    r = np.rint(x)
    d = -r.sum()
    if d:
        i = int(np.argmin(np.abs(r + d - x)))
        r[i] += d
    return r


def coefficients(full_range: bool = False):
    """``(luma, cb, cr, y_offset)``: int64 [3] rows over (R, G, B).  ``full_range`` is the seeded defect (scale 1, offset 0)."""
    one = float(1 << SHIFT)
    ys, cs, off = (1.0, 1.0, 0) if full_range else (219.0 / 255.0, 224.0 / 255.0, 16)
    kg = 1.0 - KR - KB
    luma = np.rint(one * ys * np.array([KR, kg, KB]))
    cb = _zero_sum(one * cs * np.array([-KR, -kg, 1.0 - KB]) / (2.0 * (1.0 - KB)))
    cr = _zero_sum(one * cs * np.array([1.0 - KR, -kg, -KB]) / (2.0 * (1.0 - KR)))
    return luma.astype(np.int64), cb.astype(np.int64), cr.astype(np.int64), off


LUMA, CB, CR, Y_OFFSET = coefficients()


def luma_from_rgb(r, g, b, coeff=LUMA, offset=Y_OFFSET, rounding=True):
    r, g, b = (np.asarray(v, dtype=np.int64) for v in (r, g, b))
    return (coeff[0] * r + coeff[1] * g + coeff[2] * b + (offset << SHIFT) + ((1 << (SHIFT - 1)) if rounding else 0)) >> SHIFT


def chroma_from_sums(sr, sg, sb, log2n, coeff, rounding=True):
    """One chroma sample from the R, G, B sums of the ``2 ** log2n`` pixels of its block."""
    sr, sg, sb = (np.asarray(v, dtype=np.int64) for v in (sr, sg, sb))
    sh = SHIFT + np.asarray(log2n, dtype=np.int64)
    return (coeff[0] * sr + coeff[1] * sg + coeff[2] * sb + (128 << sh) + ((1 << (sh - 1)) if rounding else 0)) >> sh


def value_ranges():
    """Extremes of every result over all inputs, from the coefficients' signs (a linear form peaks at a corner of the cube), and
    the largest intermediate magnitude.  Shows that no clamp is needed and that int32 holds every sum."""
    out = {}
    for name, c, off in (("y", LUMA, Y_OFFSET), ("cb", CB, 128), ("cr", CR, 128)):
        lo, hi = int(np.minimum(c, 0).sum()) * 255, int(np.maximum(c, 0).sum()) * 255
        half = 1 << (SHIFT - 1)
        out[name] = ((lo + (off << SHIFT) + half) >> SHIFT, (hi + (off << SHIFT) + half) >> SHIFT)
        # a block of 4 scales sums, offset and rounding term by 4
        out[name + "_peak"] = 4 * (max(-lo, hi) + (off << SHIFT) + half)
    return out


def frame_bytes(W: int, H: int) -> int:
    return W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)


def rgb_to_i420(rgb, defect=None) -> np.ndarray:
    """uint8 [F, H, W, 3] -> uint8 [F, frame_bytes(W, H)]: Y [H][W], Cb [ch][cw], Cr [ch][cw] per frame.  ``defect``: one of
    ``DEFECTS``, a wrong conversion the checks must see."""
    assert defect is None or defect in DEFECTS, defect
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3, (rgb.dtype, rgb.shape)
    F, H, W, _ = rgb.shape
    cw, ch = (W + 1) // 2, (H + 1) // 2
    luma, cb, cr, off = coefficients(full_range=defect == "full_range")
    rounding = defect != "truncate"
    x = rgb.astype(np.int64)
    if defect == "swap_rb":
        x = x[..., ::-1]
    y = luma_from_rgb(x[..., 0], x[..., 1], x[..., 2], luma, off, rounding)
    pad = np.zeros((F, 2 * ch, 2 * cw, 3), np.int64)
    pad[:, :H, :W] = x
    sums = pad.reshape(F, ch, 2, cw, 2, 3).sum(axis=(2, 4))
    ones = np.zeros((2 * ch, 2 * cw), np.int64)
    ones[:H, :W] = 1
    count = ones.reshape(ch, 2, cw, 2).sum(axis=(1, 3))            # 4, 2 or 1
    log2n = np.log2(count).astype(np.int64)
    if defect == "edge_div4":
        log2n = np.full_like(log2n, 2)
    u = chroma_from_sums(sums[..., 0], sums[..., 1], sums[..., 2], log2n, cb, rounding)
    v = chroma_from_sums(sums[..., 0], sums[..., 1], sums[..., 2], log2n, cr, rounding)
    if defect == "swap_planes":
        u, v = v, u
    for p in (y, u, v):
        assert p.min() >= 0 and p.max() <= 255      # (the defects stay inside a byte too: they must be seen by value, not by overflow)
    return np.concatenate([y.reshape(F, -1), u.reshape(F, -1), v.reshape(F, -1)], axis=1).astype(np.uint8)


def planes(buf, W: int, H: int):
    """uint8 [F, >= frame_bytes] -> (Y [F, H, W], Cb [F, ch, cw], Cr [F, ch, cw])."""
    buf = np.asarray(buf)
    F = buf.shape[0]
    cw, ch = (W + 1) // 2, (H + 1) // 2
    n, c = W * H, cw * ch
    return buf[:, :n].reshape(F, H, W), buf[:, n:n + c].reshape(F, ch, cw), buf[:, n + c:n + 2 * c].reshape(F, ch, cw)


def fp64_definition(r, g, b):
    """The definition at the top of this file, in float64, unrounded: (Y', Cb, Cr)."""
    r, g, b = (np.asarray(v, dtype=np.float64) for v in (r, g, b))
    yf = KR * r + (1.0 - KR - KB) * g + KB * b
    return (16.0 + 219.0 / 255.0 * yf, 128.0 + 224.0 / 255.0 * (b - yf) / (2.0 * (1.0 - KB)),
            128.0 + 224.0 / 255.0 * (r - yf) / (2.0 * (1.0 - KR)))


def check_i420(got, rgb, what=""):
    """THE assertion of the kernel tests: ``got`` uint8 [F, frame_bytes] equals the model of ``rgb`` in all three planes, bit for
    bit.  Named planes, so a failure says where."""
    rgb = np.asarray(rgb)
    F, H, W, _ = rgb.shape
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == (F, frame_bytes(W, H)), (what, got.dtype, got.shape)
    for name, g, e in zip(("Y", "Cb", "Cr"), planes(got, W, H), planes(rgb_to_i420(rgb), W, H)):
        bad = np.argwhere(g != e)
        assert bad.size == 0, (f"{what} {W}x{H} plane {name}: {len(bad)} of {e.size} differ, first at (frame, row, col) "
                               f"{tuple(bad[0])}: got {g[tuple(bad[0])]}, model {e[tuple(bad[0])]}")


SIZES = ((1, 1), (2, 2), (1, 5), (5, 1), (3, 3), (7, 5), (66, 34), (130, 98))       # (W, H)


def patterns(F: int, W: int, H: int, seed: int = 0):
    """The inputs of the kernel tests, name -> uint8 [F, H, W, 3]: seeded noise; the primaries, secondaries and extremes cycling
    over the pixels (so every one lands on every block position and edge); a checker of black and white whose cell is one pixel
    (every full block averages two blacks and two whites)."""
    rng = np.random.default_rng(seed + 1000 * W + H)
    noise = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    colours = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255],
                        [1, 1, 1], [254, 254, 254], [128, 128, 128]], np.uint8)
    idx = (np.arange(F)[:, None, None] * 5 + np.arange(H)[None, :, None] * 3 + np.arange(W)[None, None, :]) % len(colours)
    checker = (((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2) * 255).astype(np.uint8)
    checker = np.broadcast_to(checker[None, :, :, None], (F, H, W, 3)).copy()
    checker[1::2] = 255 - checker[1::2]
    return {"noise": noise, "colours": colours[idx], "checker": checker}


# ---- YUV4MPEG2 reader (the inverse of scripts/mux.py `y4m_header` / `y4m_frames`)
def read_y4m(path):
    """-> (tags: dict of the header's fields by first letter, ``X`` tags by name; frames: uint8 [F, frame_bytes])."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"\n")
    words = data[:end].decode("ascii").split(" ")
    assert words[0] == "YUV4MPEG2", words
    tags = {}
    for w in words[1:]:
        if w[0] == "X":
            k, _, v = w[1:].partition("=")
            tags[k] = v
        else:
            tags[w[0]] = w[1:]
    W, H = int(tags["W"]), int(tags["H"])
    n = frame_bytes(W, H)
    pos, frames = end + 1, []
    while pos < len(data):
        assert data[pos:pos + 6] == b"FRAME\n", (pos, data[pos:pos + 6])
        pos += 6
        assert pos + n <= len(data), "truncated frame"
        frames.append(np.frombuffer(data, np.uint8, n, pos))
        pos += n
    return tags, (np.stack(frames) if frames else np.zeros((0, n), np.uint8))
