"""The colour conversion of the video intake, stated once in integers: I420 (``yuv420p``) frames -> 8-bit RGB, the counterpart of
``tests/mux_model.py``.  ``vface_yuv420_to_rgb`` (csrc/demux.hip) equals ``i420_to_rgb`` bit for bit.

Definition (fp64; Kr, Kb of the matrix, Kg = 1 - Kr - Kb; limited range: off = 16, ys = 255/219, cs = 255/224; full range: off = 0,
ys = cs = 1)::

    R = ys (Y - off) + cs 2(1 - Kr) (Cr - 128)
    G = ys (Y - off) - cs 2(1 - Kr) Kr/Kg (Cr - 128) - cs 2(1 - Kb) Kb/Kg (Cb - 128)
    B = ys (Y - off) + cs 2(1 - Kb) (Cb - 128)

Integers: the five coefficients (cY, cRV, cGV, cGU, cBU) are the fp64 ones times 2^16, rounded to nearest.  The chroma of a pixel is
an integer in SIXTEENTHS, ``u16`` / ``v16`` in 0..4080: the four neighbouring chroma samples with integer weights that sum to 16
(``chroma_taps``), every neighbour index clamped into the plane:

    nearest   16 c[y >> 1][x >> 1]
    centre    (C420jpeg; what scripts/mux.py writes) weights (3, 1) / 4 between sample i = x >> 1 and i - 1 (even x) or i + 1 (odd x),
              the same for rows: 9, 3, 3, 1
    left      (C420mpeg2) horizontally co-sited: (4, 0) on even x, (2, 2) between i and i + 1 on odd x; rows as in centre

One rounding, then the clamp (arithmetic shift)::

    R = clamp((16 cY (Y - off) + cRV (v16 - 2048)                      + 2^19) >> 20, 0, 255)
    G = clamp((16 cY (Y - off) + cGV (v16 - 2048) + cGU (u16 - 2048) + 2^19) >> 20, 0, 255)
    B = clamp((16 cY (Y - off) + cBU (u16 - 2048)                      + 2^19) >> 20, 0, 255)

``value_ranges()`` shows that int32 holds every sum for all four tables.
"""
from __future__ import annotations

import numpy as np

from mux_model import SIZES, frame_bytes, planes  # noqa: F401  (one frame layout, one list of sizes for both directions)

SHIFT = 16
MATRICES = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}        # name -> (Kr, Kb)
CHROMA_MODES = ("nearest", "centre", "left")
TABLES = tuple((m, fr) for m in ("bt709", "bt601") for fr in (False, True))
DEFECTS = ("swap_uv", "swap_rb", "full_range", "bt601", "truncate", "nearest", "edge_wrap", "odd_row_off", "no_clamp")


def range_scales(full_range: bool):
    """``(luma scale, chroma scale, Y offset)``."""
    return (1.0, 1.0, 0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16)


def fp64_coefficients(matrix: str = "bt709", full_range: bool = False) -> np.ndarray:
    """float64 [5]: (cY, cRV, cGV, cGU, cBU) of the definition, unscaled."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    ys, cs, _ = range_scales(full_range)
    return np.array([ys, cs * 2.0 * (1.0 - kr), -cs * 2.0 * (1.0 - kr) * kr / kg, -cs * 2.0 * (1.0 - kb) * kb / kg,
                     cs * 2.0 * (1.0 - kb)])


def coefficients(matrix: str = "bt709", full_range: bool = False):
    """``(int64 [5]: cY, cRV, cGV, cGU, cBU; Y offset)``: the fp64 values times 2^16, rounded to nearest."""
    return np.rint(fp64_coefficients(matrix, full_range) * float(1 << SHIFT)).astype(np.int64), range_scales(full_range)[2]


def rgb_from_sixteenths(y, u16, v16, coeff, off, rounding=True, clamp=True):
    """The three formulas of the module docstring on arrays of Y (0..255) and chroma sixteenths (0..4080) -> int64 [..., 3]."""
    y, u16, v16 = (np.asarray(v, dtype=np.int64) for v in (y, u16, v16))
    cy, crv, cgv, cgu, cbu = (int(c) for c in coeff)
    luma = 16 * cy * (y - off) + ((1 << (SHIFT + 3)) if rounding else 0)
    u, v = u16 - 2048, v16 - 2048
    out = np.stack(np.broadcast_arrays(luma + crv * v, luma + cgv * v + cgu * u, luma + cbu * u), axis=-1) >> (SHIFT + 4)
    return np.clip(out, 0, 255) if clamp else out


def fp64_definition(y, cb, cr, matrix: str = "bt709", full_range: bool = False):
    """The definition at the top of this file in float64, unrounded and unclamped: [..., 3]."""
    y, cb, cr = (np.asarray(v, dtype=np.float64) for v in (y, cb, cr))
    cy, crv, cgv, cgu, cbu = fp64_coefficients(matrix, full_range)
    luma = cy * (y - range_scales(full_range)[2])
    return np.stack(np.broadcast_arrays(luma + crv * (cr - 128.0), luma + cgv * (cr - 128.0) + cgu * (cb - 128.0),
                                        luma + cbu * (cb - 128.0)), axis=-1)


def definition_bound(matrix: str, full_range: bool) -> float:
    """How far the integer result may lie from the (clamped) definition, from the coefficients' rounding residues alone: half a
    level of the one rounding, the luma residue times the largest |Y - off|, and the chroma residues of the channel that has the
    most of them times the largest |C - 128| = 128."""
    c, off = coefficients(matrix, full_range)
    res = np.abs(c / float(1 << SHIFT) - fp64_coefficients(matrix, full_range))
    return 0.5 + res[0] * (255 - off) + max(res[1], res[2] + res[3], res[4]) * 128.0


def chroma_taps(n: int, cn: int, mode: str, horizontal: bool, defect=None):
    """For the ``n`` luma positions of one axis over ``cn`` chroma samples: ``(ia, wa, ib, wb)``, int64 [n] each -- two sample
    indices, clamped into the plane, and their weights in quarters (wa + wb = 4)."""
    x = np.arange(n, dtype=np.int64)
    i, odd = x >> 1, (x & 1) == 1
    if defect == "odd_row_off" and not horizontal:
        i = np.minimum((x + 1) >> 1, cn - 1)
    if mode == "nearest":
        return i, np.full(n, 4, np.int64), i, np.zeros(n, np.int64)
    if mode == "left" and horizontal:
        return i, np.where(odd, 2, 4), np.minimum(i + 1, cn - 1), np.where(odd, 2, 0)
    assert mode in ("centre", "left"), mode
    other = i + np.where(odd, 1, -1)
    if not (defect == "edge_wrap" and horizontal):
        other = np.clip(other, 0, cn - 1)
    return i, np.full(n, 3, np.int64), other, np.full(n, 1, np.int64)


def chroma_sixteenths(c, W: int, H: int, mode: str, defect=None) -> np.ndarray:
    """A chroma plane [F, ch, cw] -> its value at every pixel in sixteenths, int64 [F, H, W]."""
    F, ch, cw = c.shape
    ia, wa, ib, wb = chroma_taps(W, cw, mode, True, defect)
    ja, va, jb, vb = chroma_taps(H, ch, mode, False, defect)
    flat = np.asarray(c, dtype=np.int64).reshape(F, ch * cw)

    def at(j, i):       # (edge_wrap: an unclamped column index walks into the row before / after; the plane's two ends hold)
        return flat[:, np.clip(j[:, None] * cw + i[None, :], 0, ch * cw - 1)]

    return ((va[:, None] * wa[None, :]) * at(ja, ia) + (va[:, None] * wb[None, :]) * at(ja, ib)
            + (vb[:, None] * wa[None, :]) * at(jb, ia) + (vb[:, None] * wb[None, :]) * at(jb, ib))


def i420_to_rgb(i420, W: int, H: int, matrix: str = "bt709", full_range: bool = False, chroma: str = "centre", defect=None) -> np.ndarray:
    """uint8 [F, >= frame_bytes(W, H)] -> uint8 [F, H, W, 3].  ``defect``: one of ``DEFECTS``, a wrong conversion the checks must
    see."""
    assert defect is None or defect in DEFECTS, defect
    assert matrix in MATRICES and chroma in CHROMA_MODES, (matrix, chroma)
    i420 = np.asarray(i420)
    assert i420.dtype == np.uint8 and i420.ndim == 2 and i420.shape[1] >= frame_bytes(W, H), (i420.dtype, i420.shape)
    y, cb, cr = planes(i420, W, H)
    if defect == "swap_uv":
        cb, cr = cr, cb
    if defect == "full_range":
        full_range = not full_range
    if defect == "bt601":
        matrix = "bt601" if matrix == "bt709" else "bt709"
    if defect == "nearest":
        chroma = "nearest" if chroma != "nearest" else "centre"
    coeff, off = coefficients(matrix, full_range)
    u16, v16 = (chroma_sixteenths(c, W, H, chroma, defect) for c in (cb, cr))
    assert 0 <= min(u16.min(), v16.min()) and max(u16.max(), v16.max()) <= 4080
    out = rgb_from_sixteenths(y, u16, v16, coeff, off, rounding=defect != "truncate", clamp=defect != "no_clamp")
    if defect == "no_clamp":
        out = out & 255
    if defect == "swap_rb":
        out = out[..., ::-1]
    assert out.min() >= 0 and out.max() <= 255       # (the defects stay inside a byte: they must be seen by value, not by overflow)
    return out.astype(np.uint8)


def value_ranges():
    """For each of the four tables: the extremes of the three sums before the shift (a linear form peaks at a corner of its box:
    Y - off in [-off, 255 - off], u16 - 2048 and v16 - 2048 in [-2048, 2032]) and the largest magnitude of any intermediate.  The
    chroma sixteenths are sums of bytes with non-negative weights that add up to 16 in every mode, so 0..4080 holds for all
    three."""
    out = {}
    for matrix, full in TABLES:
        c, off = coefficients(matrix, full)
        cy, crv, cgv, cgu, cbu = (int(v) for v in c)
        ylo, yhi, half = 16 * cy * (0 - off), 16 * cy * (255 - off), 1 << (SHIFT + 3)

        def span(*cs):
            return (sum(min(k * -2048, k * 2032) for k in cs), sum(max(k * -2048, k * 2032) for k in cs))

        rows = {"r": span(crv), "g": span(cgv, cgu), "b": span(cbu)}
        rec = {name: (ylo + lo + half, yhi + hi + half) for name, (lo, hi) in rows.items()}
        # every partial sum is bounded by the sum of the magnitudes of its terms
        rec["peak"] = max(max(abs(ylo), abs(yhi)) + sum(abs(k) * 2048 for k in cs) + half for cs in ((crv,), (cgv, cgu), (cbu,)))
        out[(matrix, full)] = rec
    return out


def check_rgb(got, i420, W: int, H: int, matrix: str = "bt709", full_range: bool = False, chroma: str = "centre", what=""):
    """THE assertion of the kernel tests: ``got`` uint8 [F, H, W, 3] equals the model of ``i420`` bit for bit.  A failure names the
    frame, row, column and channel of the first mismatch."""
    got, i420 = np.asarray(got), np.asarray(i420)
    F = i420.shape[0]
    assert got.dtype == np.uint8 and got.shape == (F, H, W, 3), (what, got.dtype, got.shape)
    want = i420_to_rgb(i420, W, H, matrix, full_range, chroma)
    bad = np.argwhere(got != want)
    if bad.size:
        f, r, c, k = (int(v) for v in bad[0])
        raise AssertionError(f"{what} {W}x{H} {matrix} {'full' if full_range else 'limited'} {chroma}: {len(bad)} of {want.size} bytes "
                             f"differ, first at frame {f}, row {r}, column {c}, channel {'RGB'[k]}: got {got[f, r, c, k]}, "
                             f"model {want[f, r, c, k]}")


def patterns(F: int, W: int, H: int, seed: int = 0):
    """The inputs of the kernel tests, name -> uint8 [F, frame_bytes(W, H)]: seeded noise over the whole byte range in all three
    planes (out-of-range codes and both clamp ends occur); the extremes and the limited-range corners cycling over the positions of
    every plane at strides of their own; a chroma checker whose cell is one SAMPLE under a luma ramp -- what separates the three
    chroma modes."""
    cw, ch = (W + 1) // 2, (H + 1) // 2
    n = frame_bytes(W, H)
    rng = np.random.default_rng(seed + 1000 * W + H)
    noise = rng.integers(0, 256, (F, n), dtype=np.uint8)
    codes = np.array([0, 255, 16, 235, 240, 128, 1, 254], np.uint8)

    def cycle(h, w, a, b, c):
        return codes[(np.arange(F)[:, None, None] * a + np.arange(h)[None, :, None] * b + np.arange(w)[None, None, :] * c) % len(codes)]

    corners = np.concatenate([cycle(H, W, 5, 3, 1).reshape(F, -1), cycle(ch, cw, 3, 1, 3).reshape(F, -1),
                              cycle(ch, cw, 1, 5, 7).reshape(F, -1)], axis=1)
    cell = (np.arange(ch)[:, None] + np.arange(cw)[None, :]) % 2
    stripe = np.broadcast_to(np.arange(cw)[None, :] % 2, (ch, cw))     # (Cr in one-sample columns: a row's two ends differ where
    ramp = ((np.arange(H)[:, None] * 7 + np.arange(W)[None, :] * 3) % 256).astype(np.uint8)     # the checker's do not, cw even)
    checker = np.empty((F, n), np.uint8)
    for f in range(F):
        k, s = (cell, stripe) if f % 2 == 0 else (1 - cell, 1 - stripe)
        checker[f] = np.concatenate([ramp.reshape(-1), np.where(k, 240, 16).reshape(-1), np.where(s, 16, 240).reshape(-1)])
    return {"noise": noise, "corners": corners, "checker": checker}
