"""The Motion-JPEG way IN, stated once in plain Python and integers: the scan of a baseline 4:2:0 JPEG frame -> restart intervals
(``vface_jpeg_scan_index``, csrc/mjpeg_in.hip, equals ``split_intervals``) -> quantised coefficients (``vface_jpeg_decode_entropy``
and the shared routine of csrc/jpeg_interval.hpp equal ``decode_scan``, statuses included) -> I420 planes (``vface_jpeg_planes``
equals ``planes`` bit for bit).  The header parse is ``vface_amd/scripts/mjpeg_in.parse_jpeg``; everything behind it is this file's
own.  The mirror image of ``tests/jpeg_model.py``, whose coefficient layout it shares: [mcus][6][64], blocks Y00 Y01 Y10 Y11 Cb Cr,
zigzag order.

Arithmetic of the planes.  ``q`` a coefficient, ``Q`` its quantiser (by component, row-major)::

    d = clamp(q Q, -2048, 2047)
    C[k][n] = rint(2^15 a_k cos((2n + 1) k pi / 16)),  a_0 = sqrt(1/8), a_k = 1/2
    columns: t[m][u] = clamp((sum_v C[v][m] d[v][u] + (1 << 10)) >> 11, -16384, 16383)        t carries 4 fraction bits
    rows:    p[m][n] = clamp(((sum_u C[u][n] t[m][u] + (1 << 18)) >> 19) + 128, 0, 255)

``value_ranges()`` shows that every sum fits int32 for EVERY int16 coefficient and every Q in 1..255 -- a hostile file can hold
any value, which is what the two inner clamps are for -- and that neither clamp is within reach of coefficients an encoder can
produce.  ``definition_bound()`` derives, from the table's rounding residues, how far ``p`` before its last rounding can lie from
the fp64 definition (dequantise, exact inverse DCT, + 128) for such coefficients: eps = 0.1471, so a pixel is within 0.5 + eps.
15 table bits and 4 fraction bits are what int32 allows: 2.642 x 2^15 x 2^14 < 2^31 (13 table bits give eps = 0.39).

Status codes are those of csrc/jpeg_interval.hpp (``STATUS``); a frame's status is the largest of its intervals' codes.
"""
from __future__ import annotations

import numpy as np

import jpeg_model as jm

DEFECTS = ("zigzag", "sign_extend", "dc_no_reset", "one_predictor", "no_unstuff", "zrl15", "eob_ignored", "chroma_tables", "wrong_quant",
           "no_level_shift", "transpose", "interval_off_by_one")
OK, MARKER_COUNT, MARKER_ORDER, SHORT, BAD_CODE, DC_CATEGORY, AC_SIZE, RUN, RANGE = range(9)
STATUS = ("ok", "marker_count", "marker_order", "short", "bad_code", "dc_category", "ac_size", "run", "range")

TABLE_BITS, PASS1_SHIFT, PASS2_SHIFT = 15, 11, 19
D_MIN, D_MAX = -2048, 2047
T_MIN, T_MAX = -16384, 16383
C = np.rint((1 << TABLE_BITS) * jm.C_EXACT).astype(np.int64)      # C[k][n]
C_EXACT = jm.C_EXACT
Q_MAX = 255
LEGAL_NOISE = Q_MAX / 2.0 + 1.0     # a legal coefficient times Q lies this close to a true DCT coefficient: half a step, and 1 for the encoder's own arithmetic


def interval_count(mcus: int, restart: int) -> int:
    return 1 if restart <= 0 or restart >= mcus else -(-mcus // restart)


# ---- markers
def split_intervals(scan: bytes, mcus: int, restart: int, defect=None):
    """-> ([(begin, end), ...], status): the byte ranges of the restart intervals of one frame's scan, the RST markers in neither.
    A wrong marker count or order gives its status and no ranges."""
    want = interval_count(mcus, restart)
    at = [i for i in range(len(scan) - 1) if scan[i] == 0xFF and (scan[i + 1] & 0xF8) == 0xD0]
    if len(at) != want - 1:
        return [], MARKER_COUNT
    if any((scan[i + 1] & 7) != (j & 7) for j, i in enumerate(at)):
        return [], MARKER_ORDER
    edges = [0] + [v for i in at for v in (i, i + 2)] + [len(scan)]
    return [(edges[2 * j], edges[2 * j + 1]) for j in range(want)], OK


# ---- Huffman decoding
def code_book(table):
    """(BITS, HUFFVAL) -> {(length, code): symbol}, T.81 Annex C."""
    bits, vals = table
    out, code, i = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            if i < len(vals):
                out[(length, code)] = vals[i]
            code += 1
            i += 1
        code <<= 1
    return out


class Bits:
    """The bits of bytes[begin:end] with the stuffed 00 bytes taken out; an FF before anything but 00 ends the data."""

    def __init__(self, data: bytes, begin: int, end: int, defect=None):
        out, pos = bytearray(), begin
        while pos < end:
            b = data[pos]
            if b == 0xFF and defect != "no_unstuff":
                if pos + 1 < end and data[pos + 1] == 0:
                    pos += 2
                else:
                    break
            else:
                pos += 1
            out.append(b)
        self.n, self.value, self.at = 8 * len(out), int.from_bytes(bytes(out), "big"), 0

    def left(self):
        return self.n - self.at

    def peek(self, length):
        """the next ``length`` bits, zeros where the data has run out"""
        have = min(length, self.left())
        v = (self.value >> (self.n - self.at - have)) & ((1 << have) - 1) if have else 0
        return v << (length - have)

    def symbol(self, book):
        for length in range(1, 17):
            s = book.get((length, self.peek(length)))
            if s is not None:
                if length > self.left():
                    return -SHORT
                self.at += length
                return s
        return -SHORT if self.left() < 16 else -BAD_CODE

    def receive_extend(self, s, defect=None):
        if s > self.left():
            return None
        v = self.peek(s)
        self.at += s
        if defect == "sign_extend":
            return v - (1 << s) if v < (1 << (s - 1)) else v
        return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def decode_interval(data: bytes, begin: int, end: int, books, blocks: int, defect=None, pred=None):
    """-> (int16 [blocks, 64] zigzag, status).  ``books``: ([dc book of Y, Cb, Cr], [ac book of Y, Cb, Cr]).  What was decoded before
    a fault stays, the rest is zero."""
    out = np.zeros((blocks, 64), np.int16)
    bits = Bits(data, begin, max(begin, end), defect)
    pred = [0, 0, 0] if pred is None else pred
    for blk in range(blocks):
        slot = blk % 6
        comp = 0 if slot < 4 else slot - 3
        tab = 1 if (defect == "chroma_tables" and comp == 0) else comp
        p = 0 if defect == "one_predictor" else comp
        s = bits.symbol(books[0][tab])
        if s < 0:
            return out, -s
        if s > 11:
            return out, DC_CATEGORY
        if s:
            diff = bits.receive_extend(s, defect)
            if diff is None:
                return out, SHORT
            pred[p] += diff
        if not -32768 <= pred[p] <= 32767:
            return out, RANGE
        out[blk, 0] = pred[p]
        k = 1
        for _ in range(63):
            if k >= 64:
                break
            rs = bits.symbol(books[1][tab])
            if rs < 0:
                return out, -rs
            r, sz = rs >> 4, rs & 15
            if sz == 0:
                if r != 15:
                    if defect == "eob_ignored":
                        k += 1
                        continue
                    break
                k += 15 if defect == "zrl15" else 16
                continue
            if sz > 10:
                return out, AC_SIZE
            k += r
            if k > 63:
                return out, RUN
            v = bits.receive_extend(sz, defect)
            if v is None:
                return out, SHORT
            out[blk, k] = v
            k += 1
    return out, OK


def decode_scan(scan: bytes, mcus: int, restart: int, huffman, defect=None):
    """One frame: -> (int16 [mcus, 6, 64], status).  ``huffman``: ([(BITS, HUFFVAL) of the DC table of Y, Cb, Cr], [.. AC ..])."""
    out = np.zeros((mcus, 6, 64), np.int16)
    ranges, status = split_intervals(scan, mcus, restart, defect)
    if status:
        return out, status
    books = ([code_book(t) for t in huffman[0]], [code_book(t) for t in huffman[1]])
    step = mcus if restart <= 0 or restart >= mcus else restart
    pred = [0, 0, 0]
    for i, (begin, end) in enumerate(ranges):
        m0 = i * step + (1 if defect == "interval_off_by_one" and i else 0)
        m1 = min(i * step + step, mcus)
        if m0 >= m1:
            continue
        got, code = decode_interval(scan, begin, end, books, (m1 - m0) * 6, defect, pred if defect == "dc_no_reset" else None)
        out[m0:m1] = got.reshape(-1, 6, 64)
        status = max(status, code)
    return out, status


def frame_tables(frame):
    """A ``mjpeg_in.JpegFrame`` -> (huffman by component as ``decode_scan`` takes it, quant uint8 [3, 64] by component)."""
    huffman = ([frame.huffman[(0, c[4])] for c in frame.components], [frame.huffman[(1, c[5])] for c in frame.components])
    return huffman, np.stack([frame.quant[c[3]] for c in frame.components])


def decode_frame(jpeg: bytes, defect=None):
    """A complete JPEG -> (coefficients int16 [mcus, 6, 64], status, quant [3, 64], W, H); the header parse is mjpeg_in's."""
    from vface_amd.scripts import mjpeg_in
    frame = mjpeg_in.parse_jpeg(jpeg)
    huffman, quant = frame_tables(frame)
    mcus = mjpeg_in.mcu_count(frame.W, frame.H)
    coef, status = decode_scan(jpeg[frame.scan[0]:frame.scan[1]], mcus, frame.restart, huffman, defect)
    return coef, status, quant, frame.W, frame.H


# ---- coefficients -> planes
def dequantise(coef, quant, defect=None):
    """int16 [..., mcus, 6, 64] zigzag, quant [..., 3, 64] row-major by component -> d int64 [..., mcus, 6, 8 (v), 8 (u)], clamped."""
    coef, quant = np.asarray(coef, np.int64), np.asarray(quant, np.int64)
    comp = np.array([0, 0, 0, 0, 1, 2] if defect != "wrong_quant" else [1, 1, 1, 1, 0, 0])
    q = quant[..., comp, :][..., None, :, :]                       # [..., 1, 6, 64] row-major
    rows = np.zeros_like(coef)
    if defect == "zigzag":
        rows[:] = coef
    else:
        rows[..., jm.ZIGZAG] = coef
    return np.clip(rows * q, D_MIN, D_MAX).reshape(coef.shape[:-1] + (8, 8))


def inverse_dct(d, defect=None):
    """d int64 [..., 8 (v), 8 (u)] -> pixels int64 [..., 8 (m), 8 (n)] in 0..255."""
    if defect == "transpose":
        d = np.swapaxes(d, -1, -2)
    t = np.clip((np.einsum("vm,...vu->...mu", C, d) + (1 << (PASS1_SHIFT - 1))) >> PASS1_SHIFT, T_MIN, T_MAX)
    p = (np.einsum("un,...mu->...mn", C, t) + (1 << (PASS2_SHIFT - 1))) >> PASS2_SHIFT
    return np.clip(p + (0 if defect == "no_level_shift" else 128), 0, 255)


def assemble(px, W: int, H: int):
    """block pixels [F, mcus, 6, 8, 8] -> (Y [F, H, W], Cb, Cr [F, ch, cw]), cropped out of the whole MCUs."""
    F = px.shape[0]
    mr, mc = jm.mcu_grid(W, H)
    px = px.reshape(F, mr, mc, 6, 8, 8)
    y = px[:, :, :, :4].reshape(F, mr, mc, 2, 2, 8, 8).transpose(0, 1, 3, 5, 2, 4, 6).reshape(F, 16 * mr, 16 * mc)
    cb = px[:, :, :, 4].transpose(0, 1, 3, 2, 4).reshape(F, 8 * mr, 8 * mc)
    cr = px[:, :, :, 5].transpose(0, 1, 3, 2, 4).reshape(F, 8 * mr, 8 * mc)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return y[:, :H, :W], cb[:, :ch, :cw], cr[:, :ch, :cw]


def planes(coef, quant, W: int, H: int, defect=None) -> np.ndarray:
    """int16 [F, mcus, 6, 64], quant [F, 3, 64] -> uint8 [F, frame_bytes] I420 rows: what ``vface_jpeg_planes`` writes."""
    coef = np.asarray(coef)
    F = coef.shape[0]
    y, cb, cr = assemble(inverse_dct(dequantise(coef.reshape(F, -1, 6, 64), quant, defect), defect), W, H)
    return np.concatenate([y.reshape(F, -1), cb.reshape(F, -1), cr.reshape(F, -1)], axis=1).astype(np.uint8)


def fp64_pixels(coef, quant):
    """The definition: dequantise, exact inverse DCT, + 128; no rounding, no clamp.  -> float64 [..., mcus, 6, 8, 8]."""
    coef, quant = np.asarray(coef, np.float64), np.asarray(quant, np.float64)
    rows = np.zeros_like(coef)
    rows[..., jm.ZIGZAG] = coef
    d = (rows * quant[..., np.array([0, 0, 0, 0, 1, 2]), :][..., None, :, :]).reshape(coef.shape[:-1] + (8, 8))
    return np.einsum("vm,...vu,un->...mn", C_EXACT, d, C_EXACT) + 128.0


def model_pixels_unrounded(coef, quant):
    """``inverse_dct`` before its last shift, as a float: what ``definition_bound`` bounds against ``fp64_pixels``."""
    d = dequantise(coef, quant)
    t = np.clip((np.einsum("vm,...vu->...mu", C, d) + (1 << (PASS1_SHIFT - 1))) >> PASS1_SHIFT, T_MIN, T_MAX)
    return np.einsum("un,...mu->...mn", C, t) / float(1 << PASS2_SHIFT) + 128.0


def libjpeg_upsample(c, W: int, H: int):
    """[F, ch, cw] integers -> int64 [F, H, W]: the same (3, 1)/4 weights per axis with the ROUNDING of libjpeg's h2v2 "fancy"
    upsampling (jdsample.c): exact column sums 3 near + far, then (3 s + left + 8) >> 4 on even and (3 s + right + 7) >> 4 on odd
    columns, neighbours clamped into the plane.  What a libjpeg decoder's full-size chroma planes are made of."""
    c = np.asarray(c, np.int64)
    out = np.zeros(c.shape[:1] + (2 * c.shape[1], 2 * c.shape[2]), np.int64)
    for v in range(2):
        far = np.concatenate([c[:, :1], c[:, :-1]], axis=1) if v == 0 else np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        s = 3 * c + far
        left, right = np.concatenate([s[..., :1], s[..., :-1]], axis=2), np.concatenate([s[..., 1:], s[..., -1:]], axis=2)
        out[:, v::2, 0::2] = (3 * s + left + 8) >> 4
        out[:, v::2, 1::2] = (3 * s + right + 7) >> 4
    return out[:, :H, :W]


# ---- the proofs
def value_ranges():
    """Extremes of every intermediate over ALL int16 coefficients and all Q in 1..255 (a linear form peaks at a corner of the box),
    and over the coefficients an encoder can produce.  Asserts what the kernel relies on; returns the numbers."""
    out = {}
    column_weight = int(np.abs(C).sum(axis=0).max())              # max over the output index of sum_k |C[k][.]|
    out["product_peak"] = 32768 * Q_MAX
    out["pass1_peak"] = column_weight * max(-D_MIN, D_MAX) + (1 << (PASS1_SHIFT - 1))
    out["pass1_out"] = (out["pass1_peak"]) >> PASS1_SHIFT        # before the clamp of t
    out["pass2_peak"] = column_weight * max(-T_MIN, T_MAX) + (1 << (PASS2_SHIFT - 1))
    for name in ("product_peak", "pass1_peak", "pass2_peak"):
        assert out[name] < 2 ** 31, (name, out[name])
    # what an encoder can produce: q Q = T + e, T the DCT of a block of pixels in [-128, 127] (|T| <= 1024, reached by DC), |e| <= Q / 2 + 1
    exact_weight = float(np.abs(C_EXACT).sum(axis=0).max())
    out["legal_d"] = 1024 + LEGAL_NOISE
    # t / 16 = sum_v C'[v][m] (T + e)[v][u]: the exact part of T is a 1-D transform of a row of pixels (<= sum_n |c_u[n]| 128 <=
    # sqrt(8) 128), the table's residues add <= 8 x 2^-16 x 1024, the noise passes with the column's weight; + 1 for the rounding
    assert exact_weight <= column_weight / 32768.0 + 8 * 2.0 ** -16
    out["legal_t"] = 16.0 * (np.sqrt(8.0) * 128.0 + 8 * 2.0 ** -16 * 1024 + column_weight / 32768.0 * LEGAL_NOISE) + 1
    assert out["legal_d"] < D_MAX and out["legal_t"] < T_MAX, out
    return out


def definition_bound() -> float:
    """eps: how far ``model_pixels_unrounded`` may lie from ``fp64_pixels`` for coefficients an encoder can produce, from the
    table's residues alone.  With C' = C / 2^15 and R[v, u; m, n] = C'[v][m] C'[u][n] - c[v][m] c[u][n] the table's part of the
    error at pixel (m, n) is sum R d, d = T + e: |sum R T| <= ||R||_2 ||T||_2 with ||T||_2 = ||pixels||_2 <= 8 x 128 (the DCT is
    orthonormal), |sum R e| <= sum |R| (Q / 2 + 1) with Q = 255.  The rounding of t (half a unit of 1/16) passes through the row
    transform: sum_u |C'[u][n]| / 32."""
    Cn = C / float(1 << TABLE_BITS)
    R = np.einsum("vm,un->vumn", Cn, Cn) - np.einsum("vm,un->vumn", C_EXACT, C_EXACT)
    table = (np.sqrt((R ** 2).sum(axis=(0, 1))) * 1024.0 + np.abs(R).sum(axis=(0, 1)) * LEGAL_NOISE).max()
    rounding = np.abs(Cn).sum(axis=0).max() / float(1 << (TABLE_BITS - PASS1_SHIFT + 1))
    return float(table + rounding)


def legal_coefficients(rng, quality: int, blocks: int):
    """Random coefficients an encoder can produce at ``quality``: the quantised exact DCT of random pixel blocks (flat, noisy,
    saturated) -> (int16 [1, blocks / 6, 6, 64], quant [1, 3, 64]).  ``blocks`` a multiple of 6."""
    qy, qc = jm.quant_tables(quality)
    kinds = rng.integers(0, 3, blocks)
    px = np.where(kinds[:, None, None] == 0, rng.integers(0, 256, (blocks, 8, 8)),
                  np.where(kinds[:, None, None] == 1, rng.choice([0, 255], (blocks, 8, 8)),
                           np.clip(rng.integers(0, 256, (blocks, 1, 1)) + rng.integers(-6, 7, (blocks, 8, 8)), 0, 255))).astype(np.float64)
    T = np.einsum("vm,bmn,un->bvu", C_EXACT, px - 128.0, C_EXACT).reshape(-1, 6, 64)
    Q = np.stack([qy] * 4 + [qc] * 2).astype(np.float64)
    q = np.rint(T / Q).astype(np.int64)[..., jm.ZIGZAG]
    return q.astype(np.int16)[None], np.stack([qy, qc, qc]).astype(np.uint8)[None]
