"""The Motion-JPEG path, stated once in integers: 8-bit RGB frames -> quantised 8 x 8 DCT coefficients of a baseline 4:2:0 JPEG
(``vface_jpeg_coefficients``, csrc/mjpeg.hip, equals ``coefficients`` bit for bit), their Huffman coding with restart intervals
(``vface_jpeg_entropy`` equals ``scan_bytes``), and the frame and AVI assembly of ``vface_amd/scripts/mjpeg.py`` written a second
time, independently, with a RIFF walker to take such a file apart again.

Arithmetic.  An MCU is 16 x 16 pixels; a frame is extended to whole MCUs by replicating its last column and row.  The colour
matrix is **full-range BT.601 (JFIF)** -- what every MJPEG decoder assumes, not the BT.709 ``tv`` range of the ``.y4m`` path::

    Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16                                   per pixel
    Cb = min(255, (-11059 SR - 21709 SG + 32768 SB + (128 << 18) + (1 << 17)) >> 18)  S over the 2 x 2 block
    Cr = min(255, ( 32768 SR - 27439 SG -  5329 SB + (128 << 18) + (1 << 17)) >> 18)
    C[k][n] = rint(8192 a_k cos((2n + 1) k pi / 16)),  a_0 = sqrt(1/8), a_k = 1/2
    rows:    t = (C . (x - 128) + (1 << 10)) >> 11
    columns: c = C . t                                  (c carries a scale of 2^15)
    q = sign(c) ((|c| + (d >> 1)) / d),  d = Q << 15

Blocks of an MCU in the order Y00 Y01 Y10 Y11 Cb Cr, 64 coefficients each in zigzag order.  ``value_ranges()`` bounds every
intermediate (int32 holds all of them), shows |DC| <= 1024 and |AC| <= 1023, and that ``(|c| + (d >> 1)) / d`` equals
``(n * RECIP(Q)) >> RECIP_SHIFT`` with ``n = (|c| + (Q << 14)) >> 15`` -- the form the kernel divides in.
"""
from __future__ import annotations

import struct

import numpy as np

DEFECTS = ("zigzag", "transpose", "no_level_shift", "truncate_quant", "chroma3", "dc_no_reset", "no_stuffing", "zrl15",
           "eob_after_63", "rst_no_wrap")

LUMA = np.array([19595, 38470, 7471], np.int64)
CB = np.array([-11059, -21709, 32768], np.int64)
CR = np.array([32768, -27439, -5329], np.int64)
RECIP_SHIFT = 20


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order, np.int64)


ZIGZAG = _zigzag()          # ZIGZAG[k] = row-major index (8 v + u) of the k-th coefficient of the scan


def dct_table():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    a = np.where(k == 0, np.sqrt(1.0 / 8.0), 0.5)
    exact = a * np.cos((2 * n + 1) * k * np.pi / 16.0)
    return np.rint(8192.0 * exact).astype(np.int64), exact


C, C_EXACT = dct_table()

# ---- Annex K of ITU-T T.81: quantisation base tables (row-major) and the four Huffman tables (BITS, HUFFVAL)
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
            0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
            0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
            0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
            0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
            0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
            0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
            0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
              0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
              0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
              0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
              0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
              0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
              0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
              0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
              0xF9, 0xFA])


def huffman_codes(table):
    """(BITS, HUFFVAL) -> {symbol: (code, length)}, the canonical assignment of T.81 Annex C."""
    bits, vals = table
    assert sum(bits) == len(vals)
    out, code, i = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[i]] = (code, length)
            code += 1
            i += 1
        code <<= 1
    return out


HUFF = {"dc": (huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA)), "ac": (huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA))}


def quant_tables(quality: int):
    """libjpeg's ``jpeg_set_quality`` (baseline): (luma, chroma) int64 [64], row-major."""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def reciprocal(Q):
    return ((1 << RECIP_SHIFT) + np.asarray(Q, np.int64) - 1) // np.asarray(Q, np.int64)


def mcu_grid(W: int, H: int):
    return (H + 15) // 16, (W + 15) // 16          # (mcu_rows, mcu_cols)


def value_ranges():
    """Extremes of every intermediate over all inputs, from the signs of the tables (a linear form peaks at a corner of the cube).
    Asserts what the kernel relies on; returns the numbers."""
    out = {}
    half = 1 << 15
    out["y"] = (half >> 16, (int(LUMA.sum()) * 255 + half) >> 16)
    for name, c in (("cb", CB), ("cr", CR)):
        off = (128 << 18) + (1 << 17)
        lo, hi = int(np.minimum(c, 0).sum()) * 1020 + off, int(np.maximum(c, 0).sum()) * 1020 + off
        out[name] = (lo >> 18, hi >> 18)                       # before the min(255, .)
        out[name + "_peak"] = max(abs(lo), abs(hi))
    assert out["y"] == (0, 255) and out["cb"] == (1, 256) == out["cr"] and int(CB.sum()) == 0 == int(CR.sum())
    # interval arithmetic over x - 128 in [-128, 127]: P and N are the sums of a row's positive and (negated) negative entries
    P, N = np.maximum(C, 0).sum(axis=1), np.maximum(-C, 0).sum(axis=1)
    t_lo, t_hi = (-128 * P - 127 * N + 1024) >> 11, (127 * P + 128 * N + 1024) >> 11      # per horizontal frequency u
    out["row_sum_peak"] = int((128 * P + 127 * N).max()) + 1024
    c_lo = P[:, None] * t_lo[None, :] - N[:, None] * t_hi[None, :]                         # [v][u]
    c_hi = P[:, None] * t_hi[None, :] - N[:, None] * t_lo[None, :]
    c_peak = np.maximum(-c_lo, c_hi)
    out["c_peak"] = int(c_peak.max())
    out["quant_peak"] = out["c_peak"] + (255 << 14)
    # x = -128 everywhere is the extreme of DC: -1024 at Q = 1.  An AC row sums to zero (+-1 from rounding), so half its weight
    # meets 127 and half 128: every AC stays at or under 1023 after the rounding, also at (4, 0), (0, 4), (4, 4), whose rows weigh
    # as much as DC's
    out["dc"] = -int((c_peak[0, 0] + (1 << 14)) >> 15)
    ac = c_peak.copy()
    ac[0, 0] = 0
    out["ac"] = int((ac.max() + (1 << 14)) >> 15)
    out["n_peak"] = (out["c_peak"] + (255 << 14)) >> 15       # the dividend of the reciprocal multiply
    for v in ("cb_peak", "cr_peak", "row_sum_peak", "c_peak", "quant_peak"):
        assert out[v] < 2 ** 31, (v, out[v])
    assert out["dc"] == -1024 and out["ac"] <= 1023, out
    assert out["n_peak"] * int(reciprocal(1)) < 2 ** 32, out
    return out


def replicate(rgb):
    """uint8 [F, H, W, 3] -> int64 [F, 16 mr, 16 mc, 3], last column and row repeated."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3, (rgb.dtype, rgb.shape)
    F, H, W, _ = rgb.shape
    mr, mc = mcu_grid(W, H)
    return np.pad(rgb.astype(np.int64), ((0, 0), (0, 16 * mr - H), (0, 16 * mc - W), (0, 0)), mode="edge")


def ycc(x, defect=None):
    """int64 [F, Hp, Wp, 3] (whole MCUs) -> (Y [F, Hp, Wp], Cb, Cr [F, Hp/2, Wp/2])."""
    F, Hp, Wp, _ = x.shape
    y = (x @ LUMA + (1 << 15)) >> 16
    blocks = x.reshape(F, Hp // 2, 2, Wp // 2, 2, 3)
    s = blocks.sum(axis=(2, 4))
    if defect == "chroma3":
        s = s - blocks[:, :, 1, :, 1]
    cb = np.minimum(255, (s @ CB + (128 << 18) + (1 << 17)) >> 18)
    cr = np.minimum(255, (s @ CR + (128 << 18) + (1 << 17)) >> 18)
    return y, cb, cr


def mcu_blocks(y, cb, cr):
    """-> int64 [F, mr, mc, 6, 8, 8]: Y00 Y01 Y10 Y11 Cb Cr of every MCU, pixel values."""
    F, Hp, Wp = y.shape
    mr, mc = Hp // 16, Wp // 16
    yb = y.reshape(F, mr, 2, 8, mc, 2, 8).transpose(0, 1, 4, 2, 5, 3, 6).reshape(F, mr, mc, 4, 8, 8)
    cbb = cb.reshape(F, mr, 8, mc, 8).transpose(0, 1, 3, 2, 4)[:, :, :, None]
    crb = cr.reshape(F, mr, 8, mc, 8).transpose(0, 1, 3, 2, 4)[:, :, :, None]
    return np.concatenate([yb, cbb, crb], axis=3)


def forward_dct(px, defect=None):
    """pixel blocks int64 [..., 8, 8] -> c int64 [..., 8 (v), 8 (u)] at a scale of 2^15."""
    x = px - (0 if defect == "no_level_shift" else 128)
    t = (np.einsum("kn,...rn->...rk", C, x) + (1 << 10)) >> 11
    c = np.einsum("vm,...mk->...vk", C, t)
    if defect == "transpose":
        c = np.swapaxes(c, -1, -2)
    return c


def quantise(c, Q, defect=None):
    """c int64 [..., 64] row-major at 2^15, Q int64 [64] -> q in the form the kernel divides in (``value_ranges``)."""
    n = (np.abs(c) + (0 if defect == "truncate_quant" else (Q << 14))) >> 15
    q = (n * reciprocal(Q)) >> RECIP_SHIFT
    assert np.array_equal(q, n // Q)
    return np.sign(c) * q


def coefficients(rgb, qy, qc, defect=None):
    """uint8 [F, H, W, 3], (luma, chroma) tables row-major -> int16 [F, mr, mc, 6, 64] in zigzag order."""
    assert defect is None or defect in DEFECTS, defect
    blocks = mcu_blocks(*ycc(replicate(rgb), defect))
    c = forward_dct(blocks, defect).reshape(blocks.shape[:4] + (64,))
    Q = np.stack([np.asarray(qy, np.int64)] * 4 + [np.asarray(qc, np.int64)] * 2)
    q = quantise(c, Q, defect)
    zz = ZIGZAG.copy()
    if defect == "zigzag":
        zz[[9, 10]] = zz[[10, 9]]
    q = q[..., zz]
    assert np.abs(q[..., 1:]).max(initial=0) <= 1023 and np.abs(q[..., 0]).max(initial=0) <= 1024
    return q.astype(np.int16)


# ---- entropy coding
class BitWriter:
    def __init__(self, stuffing=True):
        self.out, self.acc, self.n, self.stuffing = bytearray(), 0, 0, stuffing

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 255
            self.out.append(b)
            if b == 255 and self.stuffing:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _magnitude(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v - 1) & ((1 << s) - 1)


def encode_block(w, blk, pred, comp, defect=None):
    """One block of 64 zigzag coefficients into BitWriter ``w``; returns its DC (the next predictor)."""
    dc, ac = HUFF["dc"][comp], HUFF["ac"][comp]
    s, bits = _magnitude(int(blk[0]) - pred)
    w.put(*dc[s])
    w.put(bits, s)
    run = 0
    limit = 15 if defect == "zrl15" else 16
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run >= limit:
            w.put(*ac[0xF0])
            run -= limit
        s, bits = _magnitude(v)
        w.put(*ac[(run << 4) | s])
        w.put(bits, s)
        run = 0
    if run or defect == "eob_after_63":
        w.put(*ac[0x00])
    return int(blk[0])


def interval_bytes(mcus, defect=None, pred=None):
    """MCUs int16 [R, 6, 64] -> the byte-aligned, stuffed bytes of one restart interval."""
    w = BitWriter(stuffing=defect != "no_stuffing")
    pred = [0, 0, 0] if pred is None else pred
    for m in mcus:
        for b in range(6):
            comp = max(0, b - 3)
            pred[comp] = encode_block(w, m[b], pred[comp], min(comp, 1), defect)
    w.flush()
    return bytes(w.out)


def scan_intervals(coef, restart: int, defect=None):
    """One frame's coefficients int16 [mr, mc, 6, 64] (or [M, 6, 64]) -> list of interval byte strings."""
    mcus = np.asarray(coef).reshape(-1, 6, 64)
    pred = [0, 0, 0]
    return [interval_bytes(mcus[i:i + restart], defect, pred if defect == "dc_no_reset" else None)
            for i in range(0, len(mcus), restart)]


def scan_bytes(coef, restart: int, defect=None) -> bytes:
    """The entropy-coded segment of one frame: the intervals with RSTm (m = index mod 8) between them; no EOI."""
    out = bytearray()
    for i, iv in enumerate(scan_intervals(coef, restart, defect)):
        if i:
            m = (i - 1) if defect == "rst_no_wrap" else (i - 1) % 8
            out += bytes([0xFF, (0xD0 + m) & 255])
        out += iv
    return bytes(out)


# ---- frame and file assembly (independent of vface_amd/scripts/mjpeg.py; the tests compare the two)
def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_frame(W, H, qy, qc, restart, scan) -> bytes:
    out = bytearray(b"\xFF\xD8")
    out += _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, q in enumerate((qy, qc)):
        out += _segment(0xDB, bytes([i]) + bytes(int(v) for v in np.asarray(q)[ZIGZAG]))
    out += _segment(0xC0, bytes([8]) + struct.pack(">HH", H, W) + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls_id, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([cls_id]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", restart))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return bytes(out) + bytes(scan) + b"\xFF\xD9"


def encode_frames(rgb, quality: int, restart: int, defect=None):
    """uint8 [F, H, W, 3] -> list of complete JPEG frames, the whole model in one call."""
    F, H, W, _ = np.asarray(rgb).shape
    qy, qc = quant_tables(quality)
    coef = coefficients(rgb, qy, qc, defect)
    return [jpeg_frame(W, H, qy, qc, restart, scan_bytes(coef[f], restart, defect)) for f in range(F)]


def _chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def avi_file(frames, W, H, fps=10) -> bytes:
    """JPEG frames -> a RIFF 'AVI ' with one MJPG video stream, an index, sizes and counts filled in."""
    n, biggest = len(frames), max((len(f) for f in frames), default=0)
    avih = struct.pack("<14I", 1000000 // fps, min(biggest * fps, 0xFFFFFFFF), 0, 0x10, n, 0, 1, biggest, W, H, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIiI4H", 0, 0, 0, 0, 1, fps, 0, n, biggest, -1, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = _chunk(b"LIST", b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)))
    movi, idx = bytearray(b"movi"), bytearray()
    for f in frames:
        idx += b"00dc" + struct.pack("<III", 0x10, len(movi), len(f))
        movi += _chunk(b"00dc", f)
    body = b"AVI " + hdrl + _chunk(b"LIST", bytes(movi)) + _chunk(b"idx1", bytes(idx))
    return b"RIFF" + struct.pack("<I", len(body)) + body


def walk_riff(data: bytes):
    """Takes a RIFF 'AVI ' apart and asserts its structure: every size field adds up, chunks are even-padded, the index points at
    ``00dc`` chunks of the sizes it names.  -> {"avih": 14 ints, "strh": dict, "strf": dict, "frames": [bytes], "index": [...]}"""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI ", data[:12]
    assert struct.unpack_from("<I", data, 4)[0] == len(data) - 8, "RIFF size"
    out = {"frames": [], "index": []}

    def walk(lo, hi, depth):
        pos = lo
        while pos < hi:
            fourcc, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
            body = pos + 8
            assert body + size <= hi, (fourcc, pos, size, hi)
            if fourcc == b"LIST":
                kind = data[body:body + 4]
                if kind == b"movi":
                    out["movi"] = body
                walk(body + 4, body + size, depth + 1)
            elif fourcc == b"avih":
                assert size == 56
                out["avih"] = struct.unpack_from("<14I", data, body)
            elif fourcc == b"strh":
                assert size == 56
                v = struct.unpack_from("<4s4sIHHIIIIIIiI4H", data, body)
                out["strh"] = dict(type=v[0], handler=v[1], scale=v[6], rate=v[7], length=v[9], buffer=v[10], frame=v[13:17])
            elif fourcc == b"strf":
                assert size == 40
                v = struct.unpack_from("<IiiHH4sIiiII", data, body)
                out["strf"] = dict(size=v[0], W=v[1], H=v[2], planes=v[3], bits=v[4], compression=v[5], image=v[6])
            elif fourcc == b"00dc":
                out["frames"].append(data[body:body + size])
            elif fourcc == b"idx1":
                assert size % 16 == 0
                out["index"] = [struct.unpack_from("<4sIII", data, body + 16 * i) for i in range(size // 16)]
            else:
                raise AssertionError(f"unexpected chunk {fourcc!r} at {pos}")
            pos = body + size + (size & 1)
            if size & 1:
                assert data[pos - 1] == 0, "pad byte"
        assert pos == hi, (pos, hi)

    walk(12, len(data), 0)
    assert len(out["index"]) == len(out["frames"]) == out["avih"][4] == out["strh"]["length"]
    for (fourcc, flags, off, size), frame in zip(out["index"], out["frames"]):
        at = out["movi"] + off
        assert fourcc == b"00dc" and flags == 0x10 and data[at:at + 4] == b"00dc", (fourcc, off)
        assert struct.unpack_from("<I", data, at + 4)[0] == size == len(frame)
    return out


# ---- the fp64 definition, for the CPU test of the model
def fp64_coefficients(rgb):
    """The unquantised DCT coefficients of the fp64 JFIF Y'CbCr of the replicated frames: float64 [F, mr, mc, 6, 64] row-major."""
    x = replicate(rgb).astype(np.float64)
    kr, kb = 0.299, 0.114
    y = kr * x[..., 0] + (1 - kr - kb) * x[..., 1] + kb * x[..., 2]
    F, Hp, Wp = y.shape
    m = x.reshape(F, Hp // 2, 2, Wp // 2, 2, 3).mean(axis=(2, 4))
    ym = kr * m[..., 0] + (1 - kr - kb) * m[..., 1] + kb * m[..., 2]
    cb = 128.0 + (m[..., 2] - ym) / (2.0 * (1.0 - kb))
    cr = 128.0 + (m[..., 0] - ym) / (2.0 * (1.0 - kr))
    blocks = mcu_blocks(y, cb, cr) - 128.0
    c = np.einsum("vm,...mn,un->...vu", C_EXACT, blocks, C_EXACT)
    return c.reshape(c.shape[:4] + (64,))


SIZES = ((1, 1), (8, 8), (16, 16), (9, 17), (130, 50), (250, 136))         # (W, H)


def patterns(F: int, W: int, H: int, seed: int = 0):
    """name -> uint8 [F, H, W, 3]: smooth (sinusoids + ramp + sigma = 4 noise), noise, edges (hard stripes of period 3, 5 and 8),
    saturated primaries cycling over the pixels, a constant."""
    rng = np.random.default_rng(seed + 1000 * W + H)
    f, y, x = np.meshgrid(np.arange(F), np.arange(H), np.arange(W), indexing="ij")
    smooth = np.stack([128 + 60 * np.sin(x / 11.0 + f) + 40 * np.cos(y / 7.0) + 0.2 * x,
                       128 + 70 * np.sin((x + y) / 17.0 + 0.5 * f) + 0.3 * y,
                       100 + 50 * np.cos(x / 5.0) * np.sin(y / 13.0 + f) + 0.25 * (x + y)], axis=-1)
    smooth = np.clip(np.rint(smooth + rng.normal(0.0, 4.0, smooth.shape)), 0, 255).astype(np.uint8)
    noise = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    edges = np.stack([((x + f) % 3 == 0) * 255, ((y + f) % 5 < 2) * 255, ((x + y) % 8 < 4) * 255], axis=-1).astype(np.uint8)
    colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0], [255, 255, 255]], np.uint8)
    primaries = colours[(5 * f + 3 * y + x) % len(colours)]
    constant = np.broadcast_to(np.array([37, 201, 118], np.uint8), (F, H, W, 3)).copy()
    return {"smooth": smooth, "noise": noise, "edges": edges, "primaries": primaries, "constant": constant}
