"""Inflate of ONE stream on many waves, block by block: the protocol of csrc/png_inflate_par.hpp and csrc/png_in_par.hip
(``vface_png_inflate_parallel``) stated in plain Python on top of tests/png_inflate_model.py.  The kernels and the header's host
routine equal it in the candidate list, in which files fall back and why, and in everything ``vface_png_inflate`` returns.

``inflate_parallel(body, expect, chunk_bytes) -> Result``:

1. **Find.**  The body is cut into chunks of ``chunk_bytes`` bytes.  Chunk 0's segment starts at bit 0.  For chunk c >= 1 the candidate
   is the smallest bit position p in ``[8 c chunk_bytes, 8 (c + 1) chunk_bytes)`` (and inside the body) at which a block start
   passes: BTYPE = 2 (either BFINAL) and the dynamic header behind it read to the end with status 0 (``passes``).  ``quick`` is the
   cheap necessary condition every position is put to first.  A chunk without a candidate starts no segment.
2. **Count.**  A segment is decoded block after block from its start, writing nothing, and stops behind the first block that ends
   at a bit position >= the next segment's start, or behind a final block (``decode_segment``).
3. **Validate.**  The file takes the parallel path only if, in this order of precedence: no segment reports a status (else reason
   2); every segment but the last ends exactly on the next one's start without having seen BFINAL, and the last saw BFINAL (else
   reason 1); the produced counts sum to ``expect`` (else reason 3).  A status here is one of 1..11: statuses 12, 13 and 14 depend on
   the bytes in front of a segment and are reasons 4, 3 and 3.
4. **Place.**  The exclusive prefix sum of the produced counts is every segment's offset.
5. **Write.**  Each segment becomes 16-bit elements: below 256 a byte, ``0x8000 | k`` "the byte k positions into the 32 768 bytes in
   front of this segment's first byte"; a match that copies from such an element copies the element.  A distance greater than
   offset + bytes produced so far flags the file (reason 4).
6. **Resolve.**  Segments in order: an element becomes a byte, a marker reads the output at a position that an earlier segment has
   finished.  The Adler halves are summed in stream order.  ``consumed`` = ceil(end bit of the last segment / 8).
7. **Fall back.**  A flagged file is ``png_inflate_model.inflate``'s, whole.

By induction from bit 0 an accepted chain is the serial decode's own block sequence: a false candidate costs a fallback, never a byte.

``Result``: status, produced, consumed, data -- ``png_inflate_model.inflate``'s four --, ``adler`` (s1, s2), ``info`` (segments decoded
in parallel and accepted or 0, the fallback reason, candidates found, 0), ``candidates`` (the bit positions, in order), ``far`` (how
many matches reached in front of their own segment) and ``hops`` (the most segments a marker was followed through).

``defect`` names a seeded one-line mistake (DEFECTS); tests/test_png_in_parallel_cpu.py shows that each is seen."""
import functools
from typing import NamedTuple

import numpy as np

import png_inflate_model as im

MARK = 0x8000
REASONS = {0: "none", 1: "the chain did not close", 2: "a segment reported a status", 3: "the byte count is not expect",
           4: "a reference reaches in front of the file", 5: "the file's range lies outside the buffer"}
DEFECTS = ("end_rule_gt", "marker_base_off_by_one", "marker_as_byte", "chain_on_bytes", "bfinal_not_required", "candidate_past_chunk",
           "adler_completion_order")
_W7 = np.array([0, 64, 32, 16, 8, 4, 2, 1], np.int64)           # 2^(7 - l): the code-length code's Kraft sum in 128ths


class Segment(NamedTuple):
    start: int          # bit
    status: int
    end: int            # bit behind the last block decoded
    final: bool         # the last block decoded was a final one
    elements: list
    far: int            # the most any match reached in front of the segment's first byte
    far_matches: int


class Result(NamedTuple):
    status: int
    produced: int
    consumed: int
    data: bytes
    adler: tuple
    info: tuple
    candidates: tuple
    far: int
    hops: int


def _bits(body):
    return np.unpackbits(np.frombuffer(bytes(body), np.uint8), bitorder="little").astype(np.int64)


def quick(body):
    """The bit positions that pass the cheap test, ascending: BTYPE 2, HLIT <= 29, HDIST <= 29, 17 + 3 (HCLEN + 4) bits inside the
    body, and the code-length code exactly complete.  Every position that ``passes`` is among them."""
    n = 8 * len(body)
    if n < 17:
        return np.zeros(0, np.int64)
    b = np.concatenate([_bits(body), np.zeros(80, np.int64)])
    p = np.arange(n)
    p = p[(b[p + 1] == 0) & (b[p + 2] == 1)]

    def field(at, k):
        return sum(b[p + at + i] << i for i in range(k))
    p = p[(field(3, 5) <= 29)]
    p = p[(field(8, 5) <= 29)]
    ncode = field(13, 4) + 4
    p, ncode = p[p + 17 + 3 * ncode <= n], ncode[p + 17 + 3 * ncode <= n]
    kraft = np.zeros(len(p), np.int64)
    for i in range(19):
        kraft += np.where(i < ncode, _W7[field(17 + 3 * i, 3)], 0)
    return p[kraft == 128]


def passes(body, p):
    """A block start passes at bit p: BTYPE 2 and a dynamic header that reads with status 0 within the body."""
    bits = im._Bits(body)
    bits.at = p
    try:
        bits.take(1)
        if bits.take(2) != 2:
            return False
        im._dynamic(bits, None)
        return True
    except im._Stop:
        return False


@functools.lru_cache(maxsize=64)
def block_starts(body):
    """Every bit position of the body at which a block start passes (whatever the chunks)."""
    return tuple(int(p) for p in quick(body) if passes(body, int(p)))


def find(body, chunk_bytes, defect=None):
    """{chunk: candidate bit}, chunks c >= 1."""
    found, starts, n = {}, block_starts(bytes(body)), len(body)
    for c in range(1, (n + chunk_bytes - 1) // chunk_bytes):
        lo, hi = 8 * c * chunk_bytes, min(8 * (c + 1) * chunk_bytes, 8 * n)
        if defect == "candidate_past_chunk":
            hi = 8 * n
        first = next((p for p in starts if lo <= p < hi), None)
        if first is not None:
            found[c] = first
    return found


def decode_segment(body, start, stop_at, defect=None):
    """Blocks from bit ``start`` until one ends at a bit >= ``stop_at`` (None: no next segment) or was final."""
    bits, out = im._Bits(body), []
    bits.at = start
    final, far, far_matches, end = 0, 0, 0, start
    try:
        while True:
            final, kind = bits.take(1), bits.take(2)
            if kind == 3:
                raise im._Stop(2)
            if kind == 0:
                bits.at = (bits.at + 7) & ~7
                n, nn = bits.take(16), bits.take(16)
                if n != (~nn & 0xFFFF):
                    raise im._Stop(3)
                if bits.at + 8 * n > bits.total:
                    raise im._Stop(1)
                out += body[bits.at >> 3:(bits.at >> 3) + n]
                bits.at += 8 * n
            else:
                lit, dist = (im._Code(im.FIXED_LITLEN), im._Code(im.FIXED_DIST)) if kind == 1 else im._dynamic(bits, None)
                while True:
                    s = lit.symbol(bits, 10)
                    if s < 256:
                        out.append(s)
                        continue
                    if s == 256:
                        break
                    if s > 285:
                        raise im._Stop(10)
                    length = im.LEN_BASE[s - 257] + bits.take(im.LEN_EXTRA[s - 257])
                    d = dist.symbol(bits, 11)
                    if d > 29:
                        raise im._Stop(11)
                    distance = im.DIST_BASE[d] + bits.take(im.DIST_EXTRA[d])
                    q = len(out)
                    if distance > q:
                        far, far_matches = max(far, distance - q), far_matches + 1
                    for i in range(length):
                        at = q - distance + i % distance
                        if at >= 0:
                            out.append(out[at])
                        else:
                            out.append(MARK | (im.WINDOW + at + (1 if defect == "marker_base_off_by_one" else 0)) & 0x7FFF)
            end = bits.at
            if final or (stop_at is not None and (end > stop_at if defect == "end_rule_gt" else end >= stop_at)):
                break
        status = 0
    except im._Stop as stop:
        status, end = stop.status, bits.at
    return Segment(start, status, end, bool(final) and status == 0, out, far, far_matches)


def validate(segments, expect, defect=None):
    """The fallback reason of step 3 from the counted segments (their ``start``, ``status``, ``end``, ``final`` and element count)."""
    if any(s.status for s in segments):
        return 2
    for i, s in enumerate(segments):
        last = i + 1 == len(segments)
        if last:
            if not s.final:
                return 1
            continue
        nxt = segments[i + 1].start
        closes = (s.end >> 3) == (nxt >> 3) if defect == "chain_on_bytes" else s.end == nxt
        if not closes or (s.final and defect != "bfinal_not_required"):
            return 1
    if sum(len(s.elements) for s in segments) != expect:
        return 3
    return 0


def adler_add(s1, s2, data):
    """(s1, s2) of Adler-32 continued over ``data``."""
    for v in data:
        s1 = (s1 + v) % 65521
        s2 = (s2 + s1) % 65521
    return s1, s2


@functools.lru_cache(maxsize=8)
def _serial(body, expect):
    return im.inflate(body, expect)


def inflate_parallel(body, expect, chunk_bytes, defect=None):
    assert defect is None or defect in DEFECTS, defect
    assert 64 <= chunk_bytes <= 1 << 20 and chunk_bytes % 4 == 0, chunk_bytes
    body = bytes(body)
    found = find(body, chunk_bytes, defect)
    starts = [0] + [found[c] for c in sorted(found)]
    segments = [decode_segment(body, p, starts[i + 1] if i + 1 < len(starts) else None, defect) for i, p in enumerate(starts)]
    reason = validate(segments, expect, defect)
    offsets = np.concatenate([[0], np.cumsum([len(s.elements) for s in segments])]).tolist()
    if reason == 0 and any(s.far > off for s, off in zip(segments, offsets)):
        reason = 4
    candidates = tuple(starts[1:])
    if reason:
        status, produced, consumed, data = _serial(body, expect)
        return Result(status, produced, consumed, data, adler_add(1, 0, data), (0, reason, len(candidates), 0), candidates, 0, 0)
    out, depth, hops, pieces = bytearray(), [], 0, []
    for s, off in zip(segments, offsets):
        for e in s.elements:
            if e < 256 or defect == "marker_as_byte":
                out.append(e & 255)
                depth.append(0)
            else:
                at = off - im.WINDOW + (e & 0x7FFF)
                inside = 0 <= at < off                  # (always: write has refused every distance that would not be)
                out.append(out[at] if inside else 0)
                depth.append(depth[at] + 1 if inside else 0)          # (at < off: a byte that an earlier segment finished)
        pieces.append(bytes(out[off:]))
    hops = max(depth, default=0)
    order = sorted(range(len(pieces)), key=lambda i: len(pieces[i])) if defect == "adler_completion_order" else range(len(pieces))
    s1, s2 = 1, 0
    for i in order:
        s1, s2 = adler_add(s1, s2, pieces[i])
    consumed = (segments[-1].end + 7) >> 3
    return Result(0, len(out), consumed, bytes(out), (s1, s2), (len(segments), 0, len(candidates), 0), candidates,
                  sum(s.far_matches for s in segments), hops)

