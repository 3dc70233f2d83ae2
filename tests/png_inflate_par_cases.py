"""Deflate streams for the parallel inflate (tests/png_inflate_par_model.py; csrc/png_inflate_par.hpp, csrc/png_in_par.hip), made with
the bit writer and block builders of tests/png_in_cases.py: the two zlib-written families that show the parallel path is taken, and
constructed streams for the protocol's corners.  tests/test_png_in_parallel_cpu.py puts them through the model and the sanitizer
probe, tests/test_png_in_parallel_gpu.py through ``vface_png_inflate_parallel``.

``corners()``: name -> ``Case``: the body, ``expect``, the status the serial routine gives and the fallback reason per chunk size."""
import functools
import zlib
from typing import NamedTuple

import numpy as np

import png_in_cases as cases

CHUNKS = (64, 256, 4096)
# A complete literal/length code with every symbol 0..285 (literals 9 bits, the end of block 3, lengths 6 and 7) and a complete
# distance code with all 30: the dynamic blocks below carry literals AND matches at any distance.  Its header is 1338 bits.
LIT = [9] * 256 + [3] + [6] * 19 + [7] * 10
DIST = [4, 4] + [5] * 28
HEADER_BITS = 3 + 14 + 19 * 3 + 316 * 4


class Case(NamedTuple):
    body: bytes
    expect: int
    status: int
    reason: dict            # chunk_bytes -> the fallback reason
    candidates: dict        # chunk_bytes -> the candidate bits, where the case pins them


def walk(n, seed):
    """n bytes of a random walk: the cumulative sum of integers in [-3, 3], halved, mod 256."""
    return ((np.cumsum(np.random.default_rng(seed).integers(-3, 4, n)) // 2) % 256).astype(np.uint8).tobytes()


def deflate_small_blocks(data):
    """memLevel 1: zlib starts a new block every 127 tokens."""
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 1)
    return c.compress(bytes(data)) + c.flush()


@functools.lru_cache(maxsize=None)
def family_a():
    """(body, data): 20 000 bytes of a random walk, a block every 127 tokens."""
    data = walk(20000, 1)
    return deflate_small_blocks(data), data


@functools.lru_cache(maxsize=None)
def family_b():
    """(body, data): the same kind of bytes with two long repeats -- 30 000 bytes, 500 fresh, the first 20 000 again, 300 fresh, bytes
    10 000 .. 30 000 again: references far in front of their own segment, through more than one earlier segment."""
    base = walk(30000, 2)
    data = base + walk(500, 3) + base[:20000] + walk(300, 4) + base[10000:30000]
    return deflate_small_blocks(data), data


def lits(n, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 256, n)]


def dyn(w, tokens, final=0):
    return cases.dynamic_block(w, LIT, DIST, tokens, final=final)


def pad_to(w, bit, seed=0):
    """A fixed block (not final) of literals that ends exactly on ``bit``: 3 + 7 bits of header and end, literals of 9 and of 8 bits."""
    need = bit - len(w.bits) - 10
    nine = need % 8
    eight = (need - 9 * nine) // 8
    assert need >= 0 and eight >= 0 and 9 * nine + 8 * eight == need, (bit, len(w.bits))
    rng = np.random.default_rng(seed)
    tokens = [int(v) for v in rng.integers(144, 256, nine)] + [int(v) for v in rng.integers(0, 144, eight)]
    cases.fixed_block(w, tokens, final=0)
    assert len(w.bits) == bit
    w.padded = getattr(w, "padded", 0) + len(tokens)             # (the bytes the padding makes)
    return w


def _expect(body):
    d = zlib.decompressobj(-15)
    return len(d.decompress(bytes(body)))


def _ok(w, reason=0, candidates=None):
    body = w.bytes() if isinstance(w, cases.BitWriter) else w
    reason = reason if isinstance(reason, dict) else {c: reason for c in CHUNKS}
    return Case(body, _expect(body), 0, reason, candidates or {})


@functools.lru_cache(maxsize=None)
def corners():
    c = {}
    # a candidate exactly on a chunk's first bit (byte 256) and one on a chunk's last (bit 7 of byte 767), for chunks of 64 and 256
    w = dyn(cases.BitWriter(), lits(20, 1))
    dyn(pad_to(w, 8 * 256, 2), lits(20, 3))
    dyn(pad_to(w, 8 * 768 - 1, 4), lits(20, 5), final=1)
    c["candidate_on_first_and_last_bit"] = _ok(w, candidates={64: (2048, 6143), 256: (2048, 6143), 4096: ()})
    # a block longer than three chunks (of 64 and of 256): chunks without a candidate
    w = dyn(cases.BitWriter(), lits(1000, 6))
    at = len(w.bits)
    dyn(w, lits(10, 7), final=1)
    c["block_longer_than_three_chunks"] = _ok(w, candidates={64: (at,), 256: (at,), 4096: ()})
    assert at > 8 * 256 * 4
    c["shorter_than_one_chunk"] = _ok(cases.fixed_block(cases.BitWriter(), [1, 2, 3, (3, 3), 4]), candidates={k: () for k in CHUNKS})
    # a final block that ends inside a byte, in a second segment; and the same stream with bytes behind it
    w = dyn(cases.BitWriter(), lits(40, 8))
    at = len(w.bits)
    dyn(w, lits(12, 9), final=1)
    assert len(w.bits) % 8 != 0 and at > 8 * 64
    c["final_block_ends_inside_a_byte"] = _ok(w, candidates={64: (at,)})
    body = w.bytes() + cases._noise(100, 10)
    c["bytes_behind_the_final_block"] = Case(body, 52, 0, {k: 0 for k in CHUNKS}, {64: (at,)})
    # fixed, stored and dynamic blocks that one segment runs through (chunk 0 is not searched: the dynamic block starts no segment)
    w = cases.fixed_block(cases.BitWriter(), lits(5, 11), final=0)
    cases.stored_block(w, cases._noise(10, 12), final=0)
    assert len(w.bits) < 8 * 64
    dyn(w, lits(30, 13) + [(5, 12), (258, 40)])
    at = len(w.bits)
    dyn(w, [(4, 300), 7], final=1)
    c["stored_fixed_and_dynamic_in_one_segment"] = _ok(w, candidates={64: (at,)})
    # a distance of exactly 32768 from a segment's first byte (marker 0) and of 32768 from its last bytes
    w = cases.stored_block(cases.BitWriter(), cases._noise(32768, 14), final=0)
    at = len(w.bits)
    dyn(w, [(258, 32768)] + lits(20, 15) + [(3, 32768)], final=1)
    c["distance_32768_from_a_segments_ends"] = _ok(w, candidates={k: (at,) for k in CHUNKS})
    # a match that overlaps itself across marker elements: distance 7 < length 50, the source in front of the segment
    w = cases.stored_block(cases.BitWriter(), cases._noise(100, 16), final=0)
    pad_to(w, 8 * 256, 17)
    dyn(w, [(50, 7)] + lits(9, 18) + [(258, 1), (40, 60)], final=1)
    c["overlapping_match_across_markers"] = _ok(w, candidates={64: (2048,), 256: (2048,), 4096: ()})
    # a planted false candidate: a stored block whose payload is a complete dynamic block (11 literals: it ends on a byte), the first
    # candidate of its chunk, with BFINAL 0 and with BFINAL 1.  The chain does not close on it: reason 1, the serial routine's bytes
    for final in (0, 1):
        planted = dyn(cases.BitWriter(), lits(11, 19), final=final)
        assert len(planted.bits) % 8 == 0
        w = dyn(cases.BitWriter(), lits(100, 20))
        cases.stored_block(w, planted.bytes(), final=0)
        at = len(w.bits) - len(planted.bits)
        dyn(w, lits(10, 21), final=1)
        c[f"planted_false_candidate_bfinal_{final}"] = _ok(w, reason={64: 1, 256: 1, 4096: 0},
                                                        candidates={64: (at, at + len(planted.bits)), 256: (at,), 4096: ()})
    # a final block with another block start exactly behind it: the segment before the second one saw BFINAL
    w = dyn(cases.BitWriter(), lits(40, 22), final=1)
    at = len(w.bits)
    dyn(w, [], final=1)
    c["block_start_behind_the_final_block"] = Case(w.bytes(), 40, 0, {64: 1, 256: 0, 4096: 0}, {64: (at,)})
    # a reference in front of the file's first byte from a later segment: reason 4, status 12
    w = dyn(cases.BitWriter(), lits(100, 23))
    pad_to(w, 8 * 512, 24)
    dyn(w, [5, (3, 5000)], final=1)
    total = 100 + w.padded + 1 + 3
    c["reference_in_front_of_the_file"] = Case(w.bytes(), total, 12, {k: 4 for k in CHUNKS}, {64: (4096,), 256: (4096,)})
    # a total one byte short of expect and one byte over: reason 3, statuses 14 and 13
    good = c["candidate_on_first_and_last_bit"]
    c["one_byte_short_of_expect"] = Case(good.body, good.expect + 1, 14, {k: 3 for k in CHUNKS}, {})
    c["one_byte_over_expect"] = Case(good.body, good.expect - 1, 13, {k: 3 for k in CHUNKS}, {})
    # every status 1 .. 14 in a segment other than the first: 4200 stored bytes, a dynamic block that starts the segment, an empty
    # stored block to reach a byte boundary, then the stream of tests/png_in_cases.py that yields the status.  Statuses 1 .. 11 are
    # a segment's own to see (reason 2); 12 is seen against the bytes in front (4), 13 and 14 against the file's count (3)
    for status, tail in cases.status_streams(16).items():
        w = cases.stored_block(cases.BitWriter(), cases._noise(4200, 25), final=0)
        dyn(w, lits(6, 26))
        cases.stored_block(w, b"", final=0)
        if status == 12:
            tail = cases.fixed_block(cases.BitWriter(), [1, (3, 32768), 2]).bytes()
        body = w.bytes() + tail
        reason = 4 if status == 12 else 3 if status in (13, 14) else 2
        expect = 4206 + (5 if status == 12 else 16)
        c[f"status_{status}_in_a_later_segment"] = Case(body, expect, status, {k: reason for k in CHUNKS}, {})
    return c
