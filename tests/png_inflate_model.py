"""The PNG decoder of csrc/png_in.hip and vface_amd/scripts/png_in.py, stated in plain Python: inflate (RFC 1951) with the status of
csrc/png_inflate.hpp, and the five PNG filter types undone.  The kernels and the header's serial routine equal it bit for bit
(tests/test_png_in_gpu.py, tests/png_inflate_probe.cpp); zlib and Pillow are the yardsticks it is held to (tests/test_png_in_cpu.py).

``inflate(body, expect) -> (status, produced, consumed, bytes)``.  ``body`` is a raw deflate stream (no zlib header, no Adler-32).
The status is the FIRST condition met in stream order; inside a dynamic header in the order of the list:

    0   the final block ended with exactly ``expect`` bytes
    1   a bit was needed past the stream's end (a stored block whose LEN bytes are not all there is this, before anything is copied)
    2   block type 3
    3   stored block: LEN != ~NLEN
    4   more than 286 literal/length codes or more than 30 distance codes
    5   the code-length code is over-subscribed or incomplete
    6   repeat 16 with no previous length, or a repeat past HLIT + HDIST
    7   no code for symbol 256
    8   the literal/length set is over-subscribed, or incomplete and not a single 1-bit code
    9   the same for the distance set (a set with no code at all is legal: literals only)
    10  bits that are no literal/length code (15 of them were there), or symbol 286 / 287
    11  bits that are no distance code, or symbol 30 / 31
    12  a distance greater than the bytes produced so far
    13  more than ``expect`` bytes: the token (literal, match, stored block) that would pass ``expect`` is not written
    14  the final block ended with fewer than ``expect`` bytes

A symbol is found by the canonical walk, one bit at a time up to 15; where the stream ends inside the walk the status is 1.  A failed
symbol has taken no bits.  ``consumed``: whole bytes of the body behind the last bit taken (``len(body)`` for status 1); bytes behind
the final block are accepted and not counted.  ``produced``: ``len(bytes)``.

``unfilter(rows, W, H, bpp) -> (status, rgb)``: rows uint8 [H, 1 + bpp W] -> uint8 [H, W, 3]; bytes mod 256, zeros above row 0, bpp
bytes to the left, Paeth ties a, b, c; bpp 4 drops alpha, bpp 1 replicates grey.  status: 0, or 1 + the first row whose filter byte
is above 4 (rgb is then zeros).

``defect`` names a seeded one-line mistake (DEFECTS); tests/test_png_in_cpu.py shows that each is seen."""
import numpy as np

HCLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LITLEN = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 8
FIXED_DIST = (5,) * 32
WINDOW = 32768
STATUS = {0: "decoded", 1: "the stream ends early", 2: "block type 3", 3: "stored block: LEN != ~NLEN", 4: "too many length or distance codes",
          5: "bad code-length code", 6: "bad repeat in the code lengths", 7: "no end-of-block code", 8: "bad literal/length code set",
          9: "bad distance code set", 10: "invalid literal/length code", 11: "invalid distance code", 12: "distance too far back",
          13: "more bytes than the image holds", 14: "fewer bytes than the image holds"}
DEFECTS = ("dist_base_off_by_one", "no_mod_d", "ring_wrap", "repeat16_source", "len_258", "hclen_order", "stored_nlen_unchecked",
           "paeth_tie_order", "average_floor", "sub_bpp_1", "up_row_0")


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    def __init__(self, data):
        self.data, self.at, self.total = bytes(data), 0, 8 * len(data)

    def take(self, k):
        if self.at + k > self.total:
            raise _Stop(1)
        v = 0
        for i in range(k):
            v |= ((self.data[(self.at + i) >> 3] >> ((self.at + i) & 7)) & 1) << i
        self.at += k
        return v


class _Code:
    """count[l] codes of length l and the symbols by (length, symbol); ``left`` = what remains of the code space in units of 2^-15."""

    def __init__(self, lens):
        self.count = [0] * 16
        for l in lens:
            self.count[l] += 1
        self.count[0] = 0
        self.left = (1 << 15) - sum(self.count[l] << (15 - l) for l in range(1, 16))
        self.single = sum(self.count) == 1 and self.count[1] == 1
        self.none = sum(self.count) == 0
        self.sym = [i for l in range(1, 16) for i, x in enumerate(lens) if x == l]

    def symbol(self, bits, miss):
        """The canonical walk; ``miss``: the status of 15 bits that are no code.  Takes the code's bits, or none."""
        code = first = index = 0
        for l in range(1, 16):
            if bits.at + l > bits.total:
                raise _Stop(1)
            code |= (bits.data[(bits.at + l - 1) >> 3] >> ((bits.at + l - 1) & 7)) & 1
            cnt = self.count[l]
            if code - cnt < first:
                bits.at += l
                return self.sym[index + code - first]
            index += cnt
            first = (first + cnt) << 1
            code <<= 1
        raise _Stop(miss)


def _dynamic(bits, defect):
    hlit, hdist, hclen = bits.take(5), bits.take(5), bits.take(4)
    nlen, ndist = hlit + 257, hdist + 1
    if nlen > 286 or ndist > 30:
        raise _Stop(4)
    cl = [0] * 19
    order = HCLEN_ORDER if defect != "hclen_order" else tuple(range(16, 19)) + tuple(range(16))
    for i in range(hclen + 4):
        cl[order[i]] = bits.take(3)
    code = _Code(cl)
    if code.left != 0:
        raise _Stop(5)
    lens = []
    while len(lens) < nlen + ndist:
        s = code.symbol(bits, 1)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise _Stop(6)
            fill, times = (lens[-1] if defect != "repeat16_source" else lens[0]), 3 + bits.take(2)
        else:
            fill, times = 0, (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
        if len(lens) + times > nlen + ndist:
            raise _Stop(6)
        lens += [fill] * times
    if lens[256] == 0:
        raise _Stop(7)
    lit, dist = _Code(lens[:nlen]), _Code(lens[nlen:])
    if lit.left < 0 or (lit.left > 0 and not lit.single):
        raise _Stop(8)
    if dist.left < 0 or (dist.left > 0 and not dist.single and not dist.none):
        raise _Stop(9)
    return lit, dist


def inflate(body, expect, defect=None):
    assert defect is None or defect in DEFECTS, defect
    body = bytes(body)
    bits, out = _Bits(body), bytearray()
    try:
        final = 0
        while not final:
            final, kind = bits.take(1), bits.take(2)
            if kind == 3:
                raise _Stop(2)
            if kind == 0:
                bits.at = (bits.at + 7) & ~7
                n, nn = bits.take(16), bits.take(16)
                if n != (~nn & 0xFFFF) and defect != "stored_nlen_unchecked":
                    raise _Stop(3)
                if bits.at + 8 * n > bits.total:
                    raise _Stop(1)
                if len(out) + n > expect:
                    raise _Stop(13)
                out += body[bits.at >> 3:(bits.at >> 3) + n]
                bits.at += 8 * n
                continue
            lit, dist = (_Code(FIXED_LITLEN), _Code(FIXED_DIST)) if kind == 1 else _dynamic(bits, defect)
            while True:
                s = lit.symbol(bits, 10)
                if s < 256:
                    if len(out) + 1 > expect:
                        raise _Stop(13)
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise _Stop(10)
                length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                if defect == "len_258" and s == 285:
                    length = 227 + 31 + 1
                d = dist.symbol(bits, 11)
                if d > 29:
                    raise _Stop(11)
                distance = DIST_BASE[d] + bits.take(DIST_EXTRA[d]) + (1 if defect == "dist_base_off_by_one" and d >= 4 else 0)
                p = len(out)
                if distance > p:
                    raise _Stop(12)
                if p + length > expect:
                    raise _Stop(13)
                for i in range(length):
                    q = p - distance + (i % distance if defect != "no_mod_d" else min(i, distance - 1))
                    if defect == "ring_wrap" and (q // WINDOW) != ((p - distance) // WINDOW):
                        q -= 1                      # (a ring whose wrap loses a byte)
                    out.append(out[q])
        status = 0 if len(out) == expect else 14
    except _Stop as stop:
        status = stop.status
    consumed = len(body) if status == 1 else (bits.at + 7) >> 3
    return status, len(out), consumed, bytes(out)


def unfilter(rows, W, H, bpp, defect=None):
    assert defect is None or defect in DEFECTS, defect
    rows = np.asarray(rows, np.uint8).reshape(H, 1 + bpp * W)
    for y in range(H):
        if rows[y, 0] > 4:
            return 1 + y, np.zeros((H, W, 3), np.uint8)
    n = bpp * W
    left = bpp if defect != "sub_bpp_1" else 1
    above = [0] * n
    out = np.zeros((H, n), np.uint8)
    for y in range(H):
        ft, raw = int(rows[y, 0]), rows[y, 1:].tolist()
        if y == 0 and defect == "up_row_0":
            above = raw
        cur = [0] * n
        for i in range(n):
            a = cur[i - left] if i >= left else 0
            b = above[i]
            c = above[i - left] if i >= left else 0
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) >> 1 if defect != "average_floor" else (a + b + 1) >> 1
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                if defect == "paeth_tie_order":
                    pred = a if (pa <= pb and pa <= pc) else (b if pb < pc else c)
                else:
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            cur[i] = (raw[i] + pred) & 255
        out[y] = cur
        above = cur
    px = out.reshape(H, W, bpp)
    rgb = np.repeat(px, 3, axis=2) if bpp == 1 else px[:, :, :3]
    return 0, np.ascontiguousarray(rgb)


def adler_halves(data):
    """(s1, s2) of Adler-32 over ``data``, as vface_png_inflate returns them."""
    import zlib
    v = zlib.adler32(bytes(data))
    return v & 0xFFFF, v >> 16
