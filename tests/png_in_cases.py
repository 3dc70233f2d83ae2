"""Constructed deflate streams and PNG files for the PNG decoder: tests/test_png_in_cpu.py puts them through the model, zlib and the
sanitizer probe, tests/test_png_in_gpu.py through vface_png_inflate and vface_png_unfilter.

A small bit writer makes the streams: fixed blocks from tokens (a literal is an int 0..255, a match a ``(length, distance)`` pair; a
bare symbol number >= 256 in ``("sym", n)`` / ``("dsym", n)`` places that code as it is), dynamic blocks from given code lengths, and
stored blocks."""
import functools
import io
import struct
import zlib

import numpy as np

import png_inflate_model as im

# a complete code-length code for constructed dynamic headers: 13 codes of 4 bits and 6 of 5
DEFAULT_CL = (4,) * 13 + (5,) * 6


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        """n bits of value, least significant first (header fields, extra bits)."""
        self.bits += [(value >> i) & 1 for i in range(n)]
        return self

    def code(self, code, n):
        """A Huffman code: most significant bit first."""
        self.bits += [(code >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)
        return self

    def raw(self, data):
        assert len(self.bits) % 8 == 0
        for v in bytes(data):
            self.put(v, 8)
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def canonical(lens):
    """Code lengths -> (code, length) per symbol, RFC 1951 3.2.2."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        out.append((nxt[l], l))
        if l:
            nxt[l] += 1
    return out


def _index(base, value):
    i = len(base) - 1
    while base[i] > value:
        i -= 1
    return i


def put_tokens(w, tokens, lit_lens, dist_lens):
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "sym":
            w.code(*lit[t[1]])
        elif t[0] == "dsym":
            w.code(*dist[t[1]])
        else:
            length, distance = t
            i = 28 if length == 258 else _index(im.LEN_BASE[:28], length)
            w.code(*lit[257 + i]).put(length - im.LEN_BASE[i], im.LEN_EXTRA[i])
            j = _index(im.DIST_BASE, distance)
            w.code(*dist[j]).put(distance - im.DIST_BASE[j], im.DIST_EXTRA[j])
    return w


def fixed_block(w, tokens, final=1, end=True):
    w.put(final, 1).put(1, 2)
    put_tokens(w, tokens, im.FIXED_LITLEN, im.FIXED_DIST)
    if end:
        w.code(*canonical(im.FIXED_LITLEN)[256])
    return w


def stored_block(w, data, final=1, nlen=None):
    w.put(final, 1).put(0, 2).align()
    w.put(len(data), 16).put((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
    return w.raw(data)


def plain_sequence(lens):
    """Every length written as itself: no repeat symbols."""
    return [(l, 0) for l in lens]


def dynamic_block(w, lit_lens, dist_lens, tokens, final=1, cl_lens=DEFAULT_CL, seq=None, hclen=19, hlit=None, hdist=None, end=True):
    """``seq``: the code-length symbols as ``(symbol, extra value)``; by default every length as itself."""
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    w.put(final, 1).put(2, 2)
    w.put(len(lit_lens) - 257 if hlit is None else hlit, 5).put(len(dist_lens) - 1 if hdist is None else hdist, 5).put(hclen - 4, 4)
    for s in im.HCLEN_ORDER[:hclen]:
        w.put(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for s, extra in (plain_sequence(lit_lens + dist_lens) if seq is None else seq):
        w.code(*cl[s])
        if s >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[s])
    put_tokens(w, tokens, lit_lens, dist_lens)
    if end and lit_lens[256]:
        w.code(*canonical(lit_lens)[256])
    return w


def run_tokens(n, byte=0x5A):
    """Tokens that make n >= 1 bytes: a literal and distance-1 matches."""
    out, left = [byte], n - 1
    while left >= 258 + 3 or left == 258:
        out.append((258, 1))
        left -= 258
    if left > 258:
        out.append((left - 3, 1))
        left = 3
    if left >= 3:
        out.append((left, 1))
        left = 0
    return out + [byte] * left


def lens_for(used, n):
    """n lengths, zero but for ``used``: {symbol: length}."""
    out = [0] * n
    for s, l in used.items():
        out[s] = l
    return out


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def constructed():
    """name -> body: valid streams, each built for one corner of the format.  ``expect`` is the model's (or zlib's) output length."""
    c = {}
    c["length_3_and_258"] = fixed_block(BitWriter(), [1, 2, 3, (3, 3), (258, 2), (258, 1), (3, 1)]).bytes()
    for d in (1, 2, 3, 63, 64, 65, 257, 32768):
        w = stored_block(BitWriter(), _noise(max(d, 300), d), final=0)
        lengths = sorted({l for l in (3, d - 1, d, d + 1, 2 * d + 1, 258) if 3 <= l <= 258})
        fixed_block(w, [t for l in lengths for t in ((l, d), 7)])
        c[f"distance_{d}"] = w.bytes()
    # matches whose destination and whose source cross byte 32768 of the output, where the ring wraps
    w = stored_block(BitWriter(), _noise(32700, 1), final=0)
    fixed_block(w, [(100, 50), (258, 100), (258, 32768), (150, 200), 9, (258, 300), (200, 32767)])
    c["ring_wrap"] = w.bytes()
    # a 15-bit code: literals 0..13 take 1..14 bits, literal 14 and the end of block 15
    deep = lens_for({**{i: i + 1 for i in range(14)}, 14: 15, 256: 15}, 257)
    c["code_of_15_bits"] = dynamic_block(BitWriter(), deep, [0], [14, 13, 0, 12, 11, 10, 9, 14, 1]).bytes()
    # 16 repeats 'the 2 before it' over symbol 257 and all four distance codes: across the HLIT / HDIST boundary
    lit = lens_for({97: 2, 98: 2, 256: 2, 257: 2}, 258)
    seq = [(18, 97 - 11), (2, 0), (2, 0), (18, 138 - 11), (18, 19 - 11), (2, 0), (16, 5 - 3)]
    c["repeat_across_boundary"] = dynamic_block(BitWriter(), lit, [2, 2, 2, 2], [97, 98, (3, 2), (3, 1), (3, 3), 97], seq=seq).bytes()
    # zero runs by 17 and 18 that also cross it: symbols 258.. and the first distance lengths are zeros
    lit = lens_for({97: 1, 256: 2, 257: 2}, 262)
    seq = [(18, 97 - 11), (1, 0), (18, 138 - 11), (18, 20 - 11), (2, 0), (2, 0), (17, 6 - 3), (1, 0), (1, 0)]
    c["zero_run_across_boundary"] = dynamic_block(BitWriter(), lit, [0, 0, 1, 1], [97, 97, 97, 97, (3, 3), (3, 4)], seq=seq).bytes()
    one = lens_for({65: 2, 66: 2, 256: 2, 258: 2}, 259)
    c["single_distance_code"] = dynamic_block(BitWriter(), one, [1], [65, 66, (4, 1), 65, (4, 1)]).bytes()
    c["no_distance_code"] = dynamic_block(BitWriter(), lens_for({65: 1, 66: 2, 256: 2}, 257), [0], [65, 66, 66, 65]).bytes()
    c["only_end_of_block"] = dynamic_block(BitWriter(), lens_for({256: 1}, 257), [0], []).bytes()       # a single 1-bit literal/length code
    w = fixed_block(BitWriter(), [1, 2, 3], final=0)
    stored_block(w, b"", final=0)
    fixed_block(w, [(3, 3), 4], final=0)                 # (this block starts and ends inside a byte)
    stored_block(w, b"stored", final=0)
    c["empty_stored_block_and_boundaries"] = fixed_block(w, [(6, 6)]).bytes()
    c["bytes_after_the_final_block"] = fixed_block(BitWriter(), [9, 8, 7]).bytes() + b"\xAA\x55\x00\xFF"
    c["stored_only"] = stored_block(stored_block(BitWriter(), _noise(70000, 3)[:65535], final=0), _noise(4465, 4)).bytes()
    return c


def status_streams(expect):
    """status -> a stream that yields exactly that status for ``expect`` >= 16, one per status 1..14."""
    assert expect >= 16
    s = {}
    s[1] = fixed_block(BitWriter(), [1, 2, 3, 4], end=False).bytes()[:-1]
    s[2] = BitWriter().put(1, 1).put(3, 2).put(0, 13).bytes()
    s[3] = stored_block(BitWriter(), b"abcde", nlen=0x1234).bytes()
    s[4] = dynamic_block(BitWriter(), lens_for({256: 1}, 257), [0], [], hlit=30).bytes()
    s[5] = dynamic_block(BitWriter(), lens_for({256: 1}, 257), [0], [], cl_lens=lens_for({0: 1, 1: 2}, 19)).bytes()
    s[6] = dynamic_block(BitWriter(), lens_for({256: 1}, 257), [0], [], seq=[(16, 0)] + [(0, 0)] * 258).bytes()
    s[7] = dynamic_block(BitWriter(), lens_for({65: 1, 66: 1}, 257), [0], []).bytes()
    s[8] = dynamic_block(BitWriter(), lens_for({65: 2, 256: 2}, 257), [0], [65]).bytes()
    s[9] = dynamic_block(BitWriter(), lens_for({65: 1, 256: 1}, 257), [2, 2], [65]).bytes()
    s[10] = fixed_block(BitWriter(), [1, ("sym", 286), 2]).bytes()
    s[11] = fixed_block(BitWriter(), [1, 2, 3, ("sym", 257), ("dsym", 30), 4]).bytes()
    s[12] = fixed_block(BitWriter(), [1, (3, 5), 4]).bytes()
    s[13] = fixed_block(BitWriter(), run_tokens(expect) + [1]).bytes()
    s[14] = fixed_block(BitWriter(), run_tokens(expect - 1)).bytes()
    return s


def more_status_streams(expect):
    """Further ways to the same statuses: name -> (status, stream)."""
    s = {}
    s["empty"] = (1, b"")
    s["stored_short"] = (1, stored_block(BitWriter(), b"abcdefgh").bytes()[:-3])
    s["stored_header_short"] = (1, stored_block(BitWriter(), b"").bytes()[:3])
    s["dynamic_header_short"] = (1, dynamic_block(BitWriter(), lens_for({65: 1, 256: 1}, 257), [0], [65]).bytes()[:20])
    s["too_many_distance_codes"] = (4, dynamic_block(BitWriter(), lens_for({256: 1}, 257), [0], [], hdist=30).bytes())
    s["code_lengths_over_subscribed"] = (5, dynamic_block(BitWriter(), lens_for({256: 1}, 257), [0], [], cl_lens=lens_for({0: 1, 1: 1, 2: 1}, 19)).bytes())
    s["repeat_past_the_end"] = (6, dynamic_block(BitWriter(), lens_for({256: 1}, 257), [0], [], seq=[(18, 127)] * 2).bytes())
    s["litlen_over_subscribed"] = (8, dynamic_block(BitWriter(), lens_for({65: 1, 66: 1, 256: 1}, 257), [0], []).bytes())
    s["distance_over_subscribed"] = (9, dynamic_block(BitWriter(), lens_for({65: 1, 256: 1}, 257), [1, 1, 1], []).bytes())
    s["single_litlen_code_other_bit"] = (10, dynamic_block(BitWriter(), lens_for({256: 1}, 257), [0], [], end=False).put(0xFFFF, 16).bytes())
    s["no_distance_code_but_a_match"] = (11, dynamic_block(BitWriter(), lens_for({65: 2, 256: 2, 257: 1}, 258), [0], [65, ("sym", 257)], end=False).put(0, 16).bytes())
    s["stored_too_long"] = (13, stored_block(BitWriter(), bytes(expect + 1)).bytes())
    s["match_too_long"] = (13, fixed_block(BitWriter(), run_tokens(expect - 2) + [(3, 1)]).bytes())
    s["stored_too_few"] = (14, stored_block(BitWriter(), bytes(expect - 1)).bytes())
    return s


# ---- PNG files
def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(payload, zlib.crc32(kind)))


def png_bytes(W, H, colour_type, rows, depth=8, interlace=0, split=None, extra=(), level=6, stream=None):
    """A PNG of the filtered ``rows`` (bytes): IHDR, ``extra`` chunks, IDAT chunks of ``split`` payload bytes (None = one chunk; 0 =
    an empty chunk between 1-byte chunks), IEND.  ``stream``: the zlib stream instead of ``zlib.compress(rows, level)``."""
    z = zlib.compress(bytes(rows), level) if stream is None else stream
    if split is None:
        parts = [z]
    elif split == 0:
        parts = [p for i in range(len(z)) for p in (z[i:i + 1], b"")]
    else:
        parts = [z[i:i + split] for i in range(0, len(z), split)]
    out = im_signature() + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour_type, 0, 0, interlace))
    out += b"".join(chunk(k, p) for k, p in extra)
    return out + b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b"")


def im_signature():
    return b"\x89PNG\r\n\x1a\n"


def pillow_png(array, **save):
    """uint8 [H, W] (L), [H, W, 3] (RGB) or [H, W, 4] (RGBA) -> the file Pillow writes."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(array).save(buf, "PNG", **save)
    return buf.getvalue()


def resplit(data, split, extra=()):
    """A PNG file with its IDAT payloads joined and cut again (``png_bytes``'s ``split``), ``extra`` chunks put behind IHDR."""
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack_from(">I4s", data, pos)
        if kind == b"IHDR":
            head = data[pos + 8:pos + 8 + n]
        elif kind == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    W, H, depth, colour, _, _, lace = struct.unpack(">IIBBBBB", head)
    return png_bytes(W, H, colour, b"", depth, lace, split, extra, stream=idat)


# ---- streams that zlib wrote, and seeded mutations of small ones
def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(bytes(data)) + c.flush()


def _texture(n, seed):
    """Bytes with repeats at many distances: words drawn from a small dictionary, some noise between them."""
    rng = np.random.default_rng(seed)
    words = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(2, 40, 24)]
    out = b""
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] if rng.random() < 0.8 else rng.integers(0, 256, 3, dtype=np.uint8).tobytes()
    return out[:n]


@functools.lru_cache(maxsize=None)
def zlib_streams():
    """name -> (body, data): what ``zlib.compressobj`` writes at the levels and strategies a PNG writer may use."""
    s = {"level0_stored_past_65535": (raw_deflate(_noise(70001, 5), 0), _noise(70001, 5))}
    data = _texture(40000, 6)
    for name, (level, strategy) in {"fixed": (6, zlib.Z_FIXED), "rle": (6, zlib.Z_RLE), "huffman_only": (6, zlib.Z_HUFFMAN_ONLY),
                                    "level1": (1, 0), "level6": (6, 0), "level9": (9, 0)}.items():
        s[name] = (raw_deflate(data, level, strategy), data)
    return s


@functools.lru_cache(maxsize=None)
def mutation_bases():
    """Small valid bodies of every block type: [(body, expect)]."""
    out = []
    for seed in range(6):
        data = _texture(160 + 37 * seed, 40 + seed)
        for level, strategy in ((6, 0), (9, 0), (1, 0), (6, zlib.Z_FIXED), (6, zlib.Z_RLE), (6, zlib.Z_HUFFMAN_ONLY), (0, 0)):
            out.append((raw_deflate(data, level, strategy), len(data)))
    for name in ("repeat_across_boundary", "zero_run_across_boundary", "single_distance_code", "code_of_15_bits",
                 "empty_stored_block_and_boundaries", "distance_63", "length_3_and_258"):
        body = constructed()[name]
        out.append((body, len(zlib.decompressobj(-15).decompress(body))))
    return out


def mutations(count, seed):
    """``count`` bodies, each a base with ONE bit flipped, byte changed, byte inserted or tail cut off: [(body, expect)]."""
    rng = np.random.default_rng(seed)
    bases, out = mutation_bases(), []
    for k in range(count):
        body, expect = bases[k % len(bases)]
        b = bytearray(body)
        kind, at = k // len(bases) % 4, int(rng.integers(0, len(b)))
        if kind == 0:
            b[at] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            b[at] = int(rng.integers(0, 256))
        elif kind == 2:
            del b[at:]
        else:
            b.insert(at, int(rng.integers(0, 256)))
        out.append((bytes(b), expect))
    return out


def zlib_accepts(body, expect):
    """(accepted, bytes): zlib reaches the end of the stream with exactly ``expect`` bytes (bytes behind the end are allowed)."""
    d = zlib.decompressobj(-15)
    try:
        data = d.decompress(bytes(body))
    except zlib.error:
        return False, b""
    return d.eof and len(data) == expect, data
