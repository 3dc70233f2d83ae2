"""The PNG encoder of csrc/png.hip and vface_amd/scripts/png.py, stated in numpy and plain Python: filter, tokens, code lengths, block,
stripes, stream, file.  The kernels equal it byte for byte (tests/test_png_gpu.py); zlib and Pillow read what it writes
(tests/test_png_cpu.py).

Format.  8-bit RGB, colour type 2, no interlace: signature, IHDR, one IDAT, IEND.  Every row takes the filter type (0 None, 1 Sub,
2 Up, 3 Average, 4 Paeth; bpp 3; zeros above row 0) whose filtered bytes, read as signed, have the smallest sum of absolute values,
ties to the lowest type; predictions read the source pixels.  The zlib stream is 78 01, the body, Adler-32.  The body is cut into
stripes of ``stripe_rows`` rows, each coded on its own: one dynamic-Huffman block (BFINAL 0) of literals and distance-1 matches
ended by symbol 256, then an empty stored block that byte-aligns it -- or, if that is not smaller, stored blocks of at most 65535
bytes.  ``03 00`` (an empty final fixed block) ends the body.

The two choices the format leaves open are those of csrc/png_huffman.hpp, restated here:
  1. lengths: used symbols sorted by (count, symbol); two-queue Huffman merge, a leaf before a node of equal weight; leaves per depth
     folded into the limit and repaired (one code of the longest shorter length l becomes two of l + 1 for every unit the Kraft sum
     is too large); lengths handed out by rank, most frequent first, the higher symbol first among equal counts;
  2. header: HLIT 29 (286 codes), HDIST 0 (one distance code of length 1); zero runs of the 287 lengths as 18 (11..138, greedy),
     then 17 (3..10), then literal zeros; symbol 16 is never used.
``defect`` names a seeded one-line mistake (DEFECTS); tests/test_png_cpu.py shows that each is seen."""
import struct
import zlib

import numpy as np

LITLEN, CODELEN, SEQ = 286, 19, 287
LITLEN_BITS, CODELEN_BITS = 15, 7
HCLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
MAX_HEADER_BITS = 3 + 14 + CODELEN * 3 + SEQ * CODELEN_BITS            # kPngMaxHeaderBits
# what a stripe can cost beyond its tokens: the largest header, the end-of-block code, and the sync: 3 bits, padding, 00 00 FF FF
STRIPE_OVERHEAD_BYTES = (MAX_HEADER_BITS + LITLEN_BITS + 3 + 7) // 8 + 4
STORED_MAX = 65535
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
ADLER = 65521
DEFECTS = ("paeth_tie_order", "remainder_2_as_match", "codes_not_reversed", "no_end_of_block", "length_16", "hclen_untrimmed",
           "hclen_order", "adler_65536", "match_over_stripe_start", "stored_nlen")
_LEN_INDEX = np.zeros(259, np.int64)
for _i, _b in enumerate(LEN_BASE):
    _LEN_INDEX[_b:] = _i


# ---- filter
def filter_candidates(frame, defect=None):
    """frame uint8 [H, W, 3] -> uint8 [5, H, 3 W]: the filtered bytes of every row under each of the five types."""
    H, W, _ = frame.shape
    x = frame.reshape(H, 3 * W).astype(np.int64)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if defect == "paeth_tie_order":
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb < pc, b, c))
    else:
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)


def filter_rows(frame, defect=None):
    """frame uint8 [H, W, 3] -> uint8 [H, 1 + 3 W]: every row's filter byte and filtered bytes."""
    cand = filter_candidates(frame, defect)
    cost = np.abs(cand.astype(np.int8).astype(np.int64)).sum(axis=2)        # [5, H]
    best = np.argmin(cost, axis=0)                                           # the first minimum: ties to the lowest type
    H = frame.shape[0]
    rows = np.empty((H, 1 + cand.shape[2]), np.uint8)
    rows[:, 0] = best
    rows[:, 1:] = cand[best, np.arange(H)]
    return rows


# ---- tokens
def tokens(data, defect=None, lead=0):
    """uint8 [n] -> (symbol, extra value, extra bits), int64 arrays, one entry per token, without the end of block.  Greedy: a run's
    first byte is a literal, the rest is cut into matches of 258, a remainder of 3 or more is one match, of 1 or 2 literals.
    ``lead``: bytes in front of ``data`` that equal data[0] (only the match_over_stripe_start defect passes it)."""
    data = np.asarray(data, np.uint8)
    n = len(data)
    starts = np.flatnonzero(np.concatenate([[True], data[1:] != data[:-1]]))
    length = np.diff(np.concatenate([starts, [n]]))
    body = length - 1
    if lead:
        body[0] += 1                      # the first byte joins the run in front of it: no literal of its own
    nfull, rem = body // 258, body % 258
    as_match = rem >= (2 if defect == "remainder_2_as_match" else 3)
    first = np.ones(len(starts), np.int64)
    if lead:
        first[0] = 0
    count = first + nfull + np.where(as_match, 1, rem)
    run = np.repeat(np.arange(len(starts)), count)
    k = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count) + (1 - first[run])
    byte = data[starts][run].astype(np.int64)
    match = (k >= 1) & ((k <= nfull[run]) | as_match[run])
    mlen = np.where(k <= nfull[run], 258, np.maximum(rem[run], 3))
    idx = _LEN_INDEX[mlen]
    sym = np.where(match, 257 + idx, byte)
    extra = np.where(match, mlen - np.asarray(LEN_BASE)[idx], 0)
    ebits = np.where(match, np.asarray(LEN_EXTRA)[idx], 0)
    return sym, extra, ebits


# ---- code lengths
def huffman_lengths(count, maxbits):
    """count [n] -> code lengths [n], none above maxbits: csrc/png_huffman.hpp's construction (see the module docstring)."""
    n = len(count)
    order = sorted((int(c), i) for i, c in enumerate(count) if c)
    length = [0] * n
    used = len(order)
    if used == 0:
        return length
    if used == 1:
        length[order[0][1]] = 1
        return length
    leaf = [c for c, _ in order]
    node, leaf_parent, node_parent = [0] * (used - 1), [0] * used, [0] * (used - 1)
    li = ni = 0
    for k in range(used - 1):
        w = 0
        for _ in range(2):
            if li < used and (ni >= k or leaf[li] <= node[ni]):
                w += leaf[li]
                leaf_parent[li] = k
                li += 1
            else:
                w += node[ni]
                node_parent[ni] = k
                ni += 1
        node[k] = w
    depth = [0] * (used - 1)
    for k in range(used - 3, -1, -1):
        depth[k] = depth[node_parent[k]] + 1
    per_len = [0] * (max(maxbits, used) + 2)
    for i in range(used):
        per_len[depth[leaf_parent[i]] + 1] += 1
    for d in range(maxbits + 1, len(per_len)):
        per_len[maxbits] += per_len[d]
        per_len[d] = 0
    kraft = sum(per_len[d] << (maxbits - d) for d in range(1, maxbits + 1))
    while kraft > 1 << maxbits:
        per_len[maxbits] -= 1
        for d in range(maxbits - 1, 0, -1):
            if per_len[d]:
                per_len[d] -= 1
                per_len[d + 1] += 2
                break
        kraft -= 1
    r = used
    for d in range(1, maxbits + 1):
        for _ in range(per_len[d]):
            r -= 1
            length[order[r][1]] = d
    return length


def canonical_codes(length, reverse=True):
    """lengths -> the canonical codes of RFC 1951 3.2.2, bit-reversed for the LSB-first stream."""
    top = max(max(length), 1)
    cnt = [0] * (top + 2)
    for d in length:
        cnt[d] += 1
    cnt[0] = 0
    nxt, c = [0] * (top + 2), 0
    for d in range(1, top + 1):
        c = (c + cnt[d - 1]) << 1
        nxt[d] = c
    code = []
    for d in length:
        v = 0
        if d:
            v = nxt[d]
            nxt[d] += 1
            if reverse:
                v = int(format(v, f"0{d}b")[::-1], 2)
        code.append(v)
    return code


def code_length_symbols(seq):
    """The lengths a header carries -> [(symbol, extra value, extra bits)] of the code-length alphabet."""
    out, i, n = [], 0, len(seq)
    while i < n:
        if seq[i]:
            out.append((seq[i], 0, 0))
            i += 1
            continue
        run = 1
        while i + run < n and seq[i + run] == 0:
            run += 1
        i += run
        while run >= 11:
            take = min(run, 138)
            out.append((18, take - 11, 7))
            run -= take
        if run >= 3:
            out.append((17, run - 3, 3))
            run = 0
        out.extend([(0, 0, 0)] * run)
    return out


# ---- bits
def pack_bits(values, nbits):
    """(value, bit count) per item, int64 arrays -> (bytes, bit count): the values LSB-first, back to back, the last byte zero-padded."""
    values, nbits = np.asarray(values, np.int64), np.asarray(nbits, np.int64)
    total = int(nbits.sum())
    item = np.repeat(np.arange(len(nbits)), nbits)
    off = np.arange(total) - np.repeat(np.cumsum(nbits) - nbits, nbits)
    bits = ((values[item] >> off) & 1).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes(), total


# ---- blocks
def stored_bytes(n):
    return n + 5 * ((n + STORED_MAX - 1) // STORED_MAX)


def stored_blocks(data, defect=None):
    out = bytearray()
    for at in range(0, len(data), STORED_MAX):
        piece = bytes(data[at:at + STORED_MAX])
        nlen = len(piece) if defect == "stored_nlen" else len(piece) ^ 0xFFFF
        out += b"\0" + struct.pack("<HH", len(piece), nlen) + piece
    return bytes(out)


def dynamic_block(data, defect=None, lead=0):
    """One stripe as a dynamic-Huffman block and the empty stored block behind it -> (bytes, details)."""
    sym, extra, ebits = tokens(data, defect, lead)
    count = np.bincount(sym, minlength=LITLEN)
    count[256] = 1
    length = huffman_lengths(count, 16 if defect == "length_16" else LITLEN_BITS)
    if defect == "length_16":
        length[256] = 16                                # what an unlimited construction gives a rare symbol
    code = canonical_codes(length, reverse=defect != "codes_not_reversed")
    seq = length + [1]                                  # the single distance code takes one bit
    cl = code_length_symbols(seq)
    cl_count = [0] * CODELEN
    for s, _, _ in cl:
        cl_count[s] += 1
    cl_len = huffman_lengths(cl_count, CODELEN_BITS)
    cl_code = canonical_codes(cl_len)
    order = HCLEN_ORDER if defect != "hclen_order" else tuple(range(CODELEN))
    hclen = CODELEN
    while hclen > 4 and cl_len[order[hclen - 1]] == 0:
        hclen -= 1
    sent = CODELEN if defect == "hclen_untrimmed" else hclen       # the defect: all 19 are written, the field says hclen
    head = [(0, 1), (2, 2), (LITLEN - 257, 5), (0, 5), (hclen - 4, 4)]
    head += [(cl_len[order[i]], 3) for i in range(sent)]
    for s, e, eb in cl:
        head += [(cl_code[s], cl_len[s]), (e, eb)]
    hv, hb = np.array([v for v, _ in head], np.int64), np.array([b for _, b in head], np.int64)
    length_a, code_a = np.asarray(length, np.int64), np.asarray(code, np.int64)
    is_match = sym > 256
    tv = code_a[sym] | (extra << length_a[sym])        # the distance code, one 0 bit, sits above the extra bits
    tb = length_a[sym] + ebits + is_match
    tail = [] if defect == "no_end_of_block" else [(code[256], length[256])]
    tail += [(0, 3)]                                    # the empty stored block: BFINAL 0, BTYPE 00
    values = np.concatenate([hv, tv, np.array([v for v, _ in tail], np.int64)])
    nbits = np.concatenate([hb, tb, np.array([b for _, b in tail], np.int64)])
    packed, total = pack_bits(values, nbits)
    details = {"lengths": length, "cl_lengths": cl_len, "hclen": hclen, "header_bits": int(hb.sum()), "count": count,
               "dynamic_bits": total - 3}
    return packed + b"\x00\x00\xFF\xFF", details


def stripe_block(data, defect=None, lead=0):
    """One stripe -> (bytes, 'dynamic' or 'stored', details): dynamic only where it is SMALLER than the stored form."""
    dyn, details = dynamic_block(data, defect, lead)
    if len(dyn) < stored_bytes(len(data)):
        return dyn, "dynamic", details
    return stored_blocks(data, defect), "stored", details


def adler_pair(data, modulus=ADLER):
    """(s1, s2) of Adler-32 over ``data`` alone, starting from (1, 0)."""
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    n = len(d)
    s1 = (1 + int(d.sum())) % modulus
    s2 = (n + int((d * np.arange(n, 0, -1)).sum())) % modulus
    return s1, s2


def adler_combine(parts, modulus=ADLER):
    """[(s1, s2, length)] of consecutive pieces -> Adler-32 of their concatenation."""
    s1, s2 = 1, 0
    for p1, p2, n in parts:
        s2 = (s2 + p2 + (n % modulus) * ((s1 - 1) % modulus)) % modulus
        s1 = (s1 + p1 - 1) % modulus
    return (s2 << 16) | s1


def deflate_bound(row_bytes, rows, stripe_rows):
    """Bytes that always hold a body: every stripe stored, and the final 03 00."""
    full, last = divmod(rows, stripe_rows)
    return full * stored_bytes(stripe_rows * row_bytes) + (stored_bytes(last * row_bytes) if last else 0) + 2


def deflate_rows(rows, stripe_rows, defect=None):
    """rows uint8 [H, row_bytes] of any bytes -> {'body', 'stripes': [bytes], 'kinds', 'adler': [(s1, s2)], 'details'}."""
    rows = np.ascontiguousarray(rows, np.uint8)
    H = rows.shape[0]
    stripes, kinds, adler, details = [], [], [], []
    for r0 in range(0, H, stripe_rows):
        data = rows[r0:r0 + stripe_rows].reshape(-1)
        lead = 0
        if defect == "match_over_stripe_start" and r0 and rows[r0 - 1, -1] == data[0]:
            lead = 1
        blk, kind, det = stripe_block(data, defect, lead)
        stripes.append(blk)
        kinds.append(kind)
        details.append(det)
        adler.append(adler_pair(data, 65536 if defect == "adler_65536" else ADLER))
    return {"body": b"".join(stripes) + b"\x03\x00", "stripes": stripes, "kinds": kinds, "adler": adler, "details": details}


def zlib_stream(rows, stripe_rows, defect=None):
    rows = np.ascontiguousarray(rows, np.uint8)
    d = deflate_rows(rows, stripe_rows, defect)
    H, rb = rows.shape
    lens = [min(stripe_rows, H - r0) * rb for r0 in range(0, H, stripe_rows)]
    modulus = 65536 if defect == "adler_65536" else ADLER
    value = adler_combine([(s1, s2, n) for (s1, s2), n in zip(d["adler"], lens)], modulus)
    return b"\x78\x01" + d["body"] + struct.pack(">I", value), d


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def png_file(W, H, stream):
    """The file around a zlib stream: signature, IHDR (8-bit RGB, no interlace), one IDAT, IEND."""
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", stream)
            + _chunk(b"IEND", b""))


def encode(frame, stripe_rows, defect=None):
    """uint8 [H, W, 3] -> the PNG file."""
    H, W, _ = frame.shape
    return png_file(W, H, zlib_stream(filter_rows(frame, defect), stripe_rows, defect)[0])


# ---- test content
def patterns(F, W, H, seed=0):
    """name -> uint8 [F, H, W, 3]: the five patterns of the filter tests."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = {}
    out["noise"] = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    smooth = np.stack([(xx * 3 + yy * 2 + 7 * f) % 256 for f in range(F)])
    out["smooth"] = np.stack([smooth, (smooth * 2) % 256, 255 - smooth], axis=-1).astype(np.uint8)
    out["flat"] = np.broadcast_to(rng.integers(0, 256, (F, 1, 1, 3), dtype=np.uint8), (F, H, W, 3)).copy()
    out["extremes"] = rng.choice(np.array([0, 255, 128, 127], np.uint8), (F, H, W, 3))
    out["blocks"] = np.repeat(np.repeat(rng.integers(0, 256, (F, (H + 3) // 4, (W + 3) // 4, 3), dtype=np.uint8), 4, axis=1), 4, axis=2)[:, :H, :W]
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def content(kind, W, H, seed=0):
    """The three content kinds of the measurements: 'smooth' (synthetic gradient), 'noisy' (smooth + Gaussian noise, sigma 2: the
    closest to decoded video), 'noise' (uniform).  -> uint8 [H, W, 3]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(xx / 97.0 + yy / 131.0), 128 + 90 * np.cos(xx / 61.0) * np.sin(yy / 83.0),
                     (xx + yy) * 255.0 / (W + H)], axis=-1)
    if kind == "smooth":
        img = base
    elif kind == "noisy":
        img = base + rng.normal(0.0, 2.0, base.shape)
    elif kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    else:
        raise ValueError(kind)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
