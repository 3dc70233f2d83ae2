"""The GIF writer of csrc/gif.hip and vface_amd/scripts/gif.py (REFace/scripts/VFace_inference_batch.py:658), stated in numpy and plain
Python: histogram, boxes, palette, index map, LZW, image data, file.  The kernels equal it bit for bit (tests/test_gif_gpu.py);
Pillow reads what it writes (tests/test_gif_cpu.py).

1. Histogram.  cell(r, g, b) = (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3); 32768 counts per frame.
2. Boxes: median cut on the counts, every choice an integer rule.  Box 0 holds every non-empty cell.  Up to 255 times:
   - a box is splittable if it holds at least two non-empty cells; its key is population x longest side in cells (hi - lo + 1 of
     the non-empty cells along the axis); the splittable box with the largest key is split, the lowest box number on a tie; if
     none is splittable the cut ends;
   - the axis is the longest side, ties in R, G, B order;
   - with m[v] the population of the box at coordinate v of that axis, the cut c is the smallest v with 2 (m[lo] + .. + m[v]) >=
     population, but at most hi - 1: both sides are non-empty because lo and hi are tight;
   - the cells above c go to a new box with the next free number; the box keeps its number and the cells up to c.
   Result: a label per cell (0 for an empty cell) and ncolors = the number of boxes = min(256, non-empty cells).
3. Palette.  Entry i is the mean of the PIXELS whose cell lies in box i, each channel (2 sum + n) // (2 n); entries from ncolors on are 0.
4. Index map.  Every pixel takes the entry with the smallest squared RGB distance among the first ncolors, the lowest index on a tie.
5. LZW.  Minimum code size 8, Clear 256, end of information 257, first free code 258, 9 to 12 bits, LSB first.  The index stream
   is cut into segments of ``seg_pixels`` indices.  Stream: Clear at 9 bits; per segment its greedy codes from an empty table, then
   its terminator: Clear if another segment follows, end of information after the last.  The k-th code behind a Clear (k = 0, 1, ..)
   has width(k) = 9 for k = 0, else min(12, max(9, bit length of 257 + k)): the decoder's table lags the encoder's by one entry, and the
   decoder widens when ITS next free code reaches 2^width.  Every data code emitted assigns the next free code; when none is free
   (4095 is assigned: 3839 codes behind the Clear) the encoder emits Clear -- at 12 bits -- and goes on with an empty table.  A
   terminator is the k-th code of its table like any other.
6. Image data: 08, the bits padded to a byte in sub-blocks of at most 255 bytes behind their length byte, 00.
``defect`` names a seeded one-line mistake (DEFECTS); tests/test_gif_cpu.py shows that each is seen."""
import functools
import struct

import numpy as np

CELLS, CLEAR, EOI, FIRST, TABLE = 32768, 256, 257, 258, 4096
PERIOD = TABLE - FIRST + 2           # codes between two forced Clears, the Clear included: 3839 data codes and the Clear
DELAY_CS = 10                        # the reference's fps=10 (:247)
DEFECTS = ("cell_shift_2", "empty_side", "mean_floor", "tie_high", "bump_early", "bump_late", "terminator_width", "no_forced_clear",
           "subblock_256", "no_zero_end")


# ---- 1. histogram
def cells(frame, defect=None):
    f = frame.reshape(-1, 3).astype(np.int64)
    s = 2 if defect == "cell_shift_2" else 3
    return ((f[:, 0] >> s) << 10 | (f[:, 1] >> s) << 5 | (f[:, 2] >> s)) & (CELLS - 1)


def histogram(frame, defect=None):
    """uint8 [H, W, 3] -> int64 [32768]"""
    return np.bincount(cells(frame, defect), minlength=CELLS).astype(np.int64)


# ---- 2. boxes
_COORD = np.stack([np.arange(CELLS) >> 10, (np.arange(CELLS) >> 5) & 31, np.arange(CELLS) & 31])


def box_key(pop, lo, hi, ncells, i):
    """0 for a box that cannot be split; otherwise larger = split first."""
    if ncells < 2:
        return 0
    return (int(pop) * (max(h - l for l, h in zip(lo, hi)) + 1)) << 8 | (255 - i)


def box_axis(lo, hi):
    side = [h - l for l, h in zip(lo, hi)]
    return side.index(max(side))                 # the first maximum: R, G, B order


def box_cut(marg, lo, hi, pop, defect=None):
    """marg[v]: population at coordinate v -> the last coordinate of the lower side."""
    run = 0
    for v in range(lo, hi + 1):
        run += int(marg[v])
        if 2 * run >= pop:
            break
    return v if defect == "empty_side" else min(v, hi - 1)


def _stats(n, co, mask):
    idx = np.flatnonzero(mask)
    if not idx.size:
        return {"pop": 0, "lo": [0, 0, 0], "hi": [0, 0, 0], "ncells": 0}
    return {"pop": int(n[idx].sum()), "lo": [int(c[idx].min()) for c in co], "hi": [int(c[idx].max()) for c in co], "ncells": int(idx.size)}


def boxes(counts, defect=None):
    """int64 [32768] -> (labels uint8 [32768], ncolors, [box stats]).  Works on the non-empty cells alone."""
    counts = np.asarray(counts, np.int64)
    used = np.flatnonzero(counts > 0)
    n, co = counts[used], _COORD[:, used]
    lab = np.zeros(len(used), np.int64)
    info = [_stats(n, co, lab == 0)]
    while len(info) < 256:
        keys = [box_key(b["pop"], b["lo"], b["hi"], b["ncells"], i) for i, b in enumerate(info)]
        if max(keys) == 0:
            break
        i = keys.index(max(keys))                # keys are distinct: 255 - i is part of them
        b = info[i]
        ax = box_axis(b["lo"], b["hi"])
        mine = lab == i
        marg = np.bincount(co[ax][mine], weights=n[mine], minlength=32).astype(np.int64)
        c = box_cut(marg, b["lo"][ax], b["hi"][ax], b["pop"], defect)
        upper = mine & (co[ax] > c)
        lab[upper] = len(info)
        info[i] = _stats(n, co, mine & ~upper)
        info.append(_stats(n, co, upper))
    labels = np.zeros(CELLS, np.uint8)
    labels[used] = lab
    return labels, len(info), info


# ---- 3. palette
def palette(frame, labels, ncolors, defect=None):
    """-> uint8 [256, 3], zeros from ncolors on"""
    lab = labels[cells(frame)]
    px = frame.reshape(-1, 3).astype(np.int64)
    pal = np.zeros((256, 3), np.uint8)
    n = np.bincount(lab, minlength=256)
    for ch in range(3):
        s = np.bincount(lab, weights=px[:, ch], minlength=256).astype(np.int64)
        for i in range(ncolors):
            pal[i, ch] = s[i] // n[i] if defect == "mean_floor" else (2 * s[i] + n[i]) // (2 * n[i])
    return pal


# ---- 4. index map
def index_map(frame, pal, ncolors, defect=None):
    """-> uint8 [H * W]"""
    px = frame.reshape(-1, 3).astype(np.int32)
    p = pal[:ncolors].astype(np.int32)
    out = np.empty(len(px), np.uint8)
    for at in range(0, len(px), 1 << 14):
        d = ((px[at:at + (1 << 14), None, :] - p[None]) ** 2).sum(axis=2)
        if defect == "tie_high":
            out[at:at + (1 << 14)] = ncolors - 1 - np.argmin(d[:, ::-1], axis=1)
        else:
            out[at:at + (1 << 14)] = np.argmin(d, axis=1)     # the first minimum: the lowest index
    return out


def quantise(frame, defect=None):
    """-> dict: counts, labels, ncolors, palette [256, 3], indices [H * W]"""
    counts = histogram(frame, defect)
    labels, ncolors, info = boxes(counts, defect)
    pal = palette(frame, labels, ncolors, defect)
    return {"counts": counts, "labels": labels, "ncolors": ncolors, "boxes": info, "palette": pal,
            "indices": index_map(frame, pal, ncolors, defect)}


# ---- 5. LZW
def width(k, defect=None):
    if defect == "bump_early":
        return min(12, max(9, (258 + k).bit_length()))
    if defect == "bump_late":
        return min(12, max(9, (256 + k).bit_length())) if k else 9
    return min(12, max(9, (257 + k).bit_length())) if k else 9


def lzw_segment(seg, last, defect=None):
    """indices of ONE segment -> dict: codes [(code, width)], bits, forced (Clears inside), next (the next free code at the terminator)"""
    codes, k, table, nxt, forced = [], 0, {}, FIRST, 0
    prefix = int(seg[0])
    for ch in map(int, seg[1:]):
        hit = table.get((prefix, ch))
        if hit is not None:
            prefix = hit
            continue
        codes.append((prefix, width(k, defect)))
        k += 1
        if nxt < TABLE:
            table[(prefix, ch)] = nxt
            nxt += 1
        elif defect != "no_forced_clear":
            codes.append((CLEAR, width(k, defect)))
            k, table, nxt, forced = 0, {}, FIRST, forced + 1
        prefix = ch
    codes.append((prefix, width(k, defect)))
    k += 1
    codes.append((EOI if last else CLEAR, width(k - 1 if defect == "terminator_width" else k, defect)))
    return {"codes": codes, "bits": sum(w for _, w in codes), "forced": forced, "next": nxt}


def lzw(indices, seg_pixels, defect=None):
    """uint8 [n] -> dict: data (the padded bit stream, bytes), segments [lzw_segment's dicts]"""
    n = len(indices)
    segs = [lzw_segment(indices[at:at + seg_pixels], at + seg_pixels >= n, defect) for at in range(0, n, seg_pixels)]
    acc, nbits, out = CLEAR, 9, bytearray()
    for s in segs:
        for code, w in s["codes"]:
            acc |= code << nbits
            nbits += w
        while nbits >= 8:
            out.append(acc & 255)
            acc >>= 8
            nbits -= 8
    if nbits:
        out.append(acc & 255)
    return {"data": bytes(out), "segments": segs}


# ---- 6. image data
def sub_blocks(data, defect=None):
    size = 256 if defect == "subblock_256" else 255
    out = bytearray([8])
    for at in range(0, len(data), size):
        blk = data[at:at + size]
        out.append(len(blk) & 255)
        out += blk
    if defect != "no_zero_end":
        out.append(0)
    return bytes(out)


def image_data(indices, seg_pixels, defect=None):
    return sub_blocks(lzw(indices, seg_pixels, defect)["data"], defect)


def image_data_bytes(nbytes):
    return 1 + nbytes + (nbytes + 254) // 255 + 1


def code_bits(j):
    """Bits of the first j codes of a segment: periods of PERIOD codes, each from width 9."""
    def cum(k):
        return 9 * k + max(0, k - 255) + max(0, k - 767) + max(0, k - 1791)
    return (j // PERIOD) * cum(PERIOD) + cum(j % PERIOD)


def max_codes(m):
    """The most codes a segment of m indices can make: m data codes, a forced Clear behind every 3839 of them, the terminator."""
    return m + m // (PERIOD - 1) + 1


def lzw_bound(npix, seg_pixels):
    """vface_gif_lzw_bound: bytes that always hold a frame's image data."""
    full, last = divmod(npix, seg_pixels)
    bits = 9 + full * code_bits(max_codes(seg_pixels)) + (code_bits(max_codes(last)) if last else 0)
    return image_data_bytes((bits + 7) // 8)


# ---- the file
def header(W, H):
    return b"GIF89a" + struct.pack("<HHBBB", W, H, 0x70, 0, 0) + b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\x00\x00\x00"


def frame_header(W, H):
    """graphic control extension (disposal 1, no transparency, the delay) and image descriptor with a local table of 256"""
    return b"\x21\xF9\x04\x04" + struct.pack("<H", DELAY_CS) + b"\x00\x00" + b"\x2C" + struct.pack("<HHHH", 0, 0, W, H) + b"\x87"


def gif_file(frames, seg_pixels, defect=None, qs=None):
    """uint8 [F, H, W, 3] -> (bytes, [quantise's dicts]); ``qs``: the frames' quantise() where the caller has it already"""
    F, H, W, _ = frames.shape
    out, qs = bytearray(header(W, H)), [quantise(frame, defect) for frame in frames] if qs is None else qs
    for q in qs:
        out += frame_header(W, H) + q["palette"].tobytes() + image_data(q["indices"], seg_pixels, defect)
    return bytes(out + b"\x3B"), qs


# ---- the inverse
def decode_image_data(data, npix):
    """image data -> (uint8 [npix] indices, bytes consumed): the decoder GIF readers apply, written from the format alone"""
    assert data[0] == 8
    at, raw = 1, bytearray()
    while data[at]:
        raw += data[at + 1:at + 1 + data[at]]
        at += 1 + data[at]
    acc = int.from_bytes(raw, "little")
    out, pos, w, table, prev = [], 0, 9, None, None
    while True:
        code = (acc >> pos) & ((1 << w) - 1)
        pos += w
        assert pos <= 8 * len(raw), "ran off the stream"
        if code == CLEAR:
            table, w, prev = [[i] for i in range(256)] + [None, None], 9, None
            continue
        if code == EOI:
            break
        if prev is None:
            entry = table[code]
        else:
            assert code <= len(table), "code ahead of the table"
            entry = table[code] if code < len(table) else prev + [prev[0]]
            if len(table) < TABLE:
                table.append(prev + [entry[0]])
                if len(table) == 1 << w and w < 12:
                    w += 1
        out += entry
        prev = entry
    assert len(out) == npix and 8 * len(raw) - pos < 8, (len(out), npix)
    return np.array(out, np.uint8), at + 1


@functools.lru_cache(maxsize=None)
def stream_with_next(target):
    """A noise index stream whose ONE segment ends with the next free code == target (binary search over the length)."""
    noise = np.random.default_rng(target).integers(0, 256, 5000, dtype=np.uint8)
    lo, hi = 1, 5000
    while lo < hi:                                           # next is monotone in the length: greedy codes of a prefix are a prefix
        mid = (lo + hi) // 2
        seg = lzw_segment(noise[:mid], True)
        if (seg["forced"], seg["next"]) < (0, target):          # behind a forced Clear the count starts again
            lo = mid + 1
        else:
            hi = mid
    assert lzw_segment(noise[:lo], True)["next"] == target and lzw_segment(noise[:lo], True)["forced"] == 0
    return noise[:lo].copy()


@functools.lru_cache(maxsize=None)
def stream_with_bytes(target):
    """(an index stream over four values, seg_pixels) whose bit stream is ``target`` bytes long.  In one segment the lengths that
    can be reached are fixed by the widths alone, so the search is over the segment length too."""
    s = np.random.default_rng(1000 + target).integers(0, 4, 6000, dtype=np.uint8)
    for seg_pixels in (65535,) + tuple(range(200, 264)):
        lo, hi = 1, 6000
        while lo < hi:
            mid = (lo + hi) // 2
            if len(lzw(s[:mid], seg_pixels)["data"]) < target:
                lo = mid + 1
            else:
                hi = mid
        if len(lzw(s[:lo], seg_pixels)["data"]) == target:
            return s[:lo].copy(), seg_pixels
    raise AssertionError(target)
