"""The streams the Motion-JPEG decoder is tested on, built once and shared by tests/test_mjpeg_in_cpu.py and
tests/test_mjpeg_in_gpu.py: the encoder model's own scans (``round_trip_streams``), frames Pillow (libjpeg-turbo) encoded in every
form the parser promises to read (``pillow_frames``), and scans corrupted by hand (``corruption_cases``).  Each builder is cached:
the model decodes a stream once per process."""
from __future__ import annotations

import functools
import io
import struct

import numpy as np
from PIL import Image

import jpeg_decode_model as jdm
import jpeg_model as jm
from test_mjpeg_gpu import SIZES, entropy_cases

ANNEX_K = ([jm.DC_LUMA, jm.DC_CHROMA, jm.DC_CHROMA], [jm.AC_LUMA, jm.AC_CHROMA, jm.AC_CHROMA])
PILLOW_SIZES = ((1, 1), (9, 17), (130, 50), (250, 136))
PILLOW_PATTERNS = ("noise", "smooth", "edges")          # (smooth = the gradient: sinusoids and a ramp)


@functools.lru_cache(maxsize=None)
def round_trip_streams():
    """[(name, coefficients int16 [M, 6, 64], restart, scan bytes)]: every SIZES entry of test_mjpeg_gpu.py with restart intervals of 1,
    of one MCU row and of more than the frame's MCUs, and every frame of every constructed case of ``entropy_cases()`` (+-2047 DC
    differences, zero runs of 15 / 16 / 17 / 32 / 62, FF at the end of an interval, wrapping RST numbers)."""
    out = []
    for i, (W, H) in enumerate(SIZES):
        mr, mc = jm.mcu_grid(W, H)
        pats = jm.patterns(1, W, H, seed=21)
        rgb = pats[sorted(pats)[i % len(pats)]]
        coef = jm.coefficients(rgb, *jm.quant_tables((50, 90, 100)[i % 3]))[0].reshape(-1, 6, 64)
        for restart in (1, mc, mr * mc + 3):
            out.append((f"{W}x{H}_r{restart}", coef, restart, jm.scan_bytes(coef, restart)))
    for name, (coef, restart) in sorted(entropy_cases().items()):
        for f in range(coef.shape[0]):
            out.append((f"{name}_{f}", coef[f], restart, jm.scan_bytes(coef[f], restart)))
    return out


def segments(jpeg: bytes):
    """[(marker, start, end)] of the header segments of a frame up to and including SOS; SOI is not listed."""
    out, pos = [], 2
    while True:
        marker, size = jpeg[pos + 1], struct.unpack_from(">H", jpeg, pos + 2)[0]
        out.append((marker, pos, pos + 2 + size))
        pos += 2 + size
        if marker == 0xDA:
            return out


def without(jpeg: bytes, marker: int) -> bytes:
    keep = bytearray(jpeg[:2])
    segs = segments(jpeg)
    for m, lo, hi in segs:
        if m != marker:
            keep += jpeg[lo:hi]
    return bytes(keep) + jpeg[segs[-1][2]:]


def merged(jpeg: bytes, marker: int) -> bytes:
    """All segments of ``marker`` (DQT or DHT) as ONE segment holding their tables, where the first of them stood."""
    segs = segments(jpeg)
    payload = b"".join(jpeg[lo + 4:hi] for m, lo, hi in segs if m == marker)
    one = bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload
    out, done = bytearray(jpeg[:2]), False
    for m, lo, hi in segs:
        if m != marker:
            out += jpeg[lo:hi]
        elif not done:
            out += one
            done = True
    return bytes(out) + jpeg[segs[-1][2]:]


def with_extra_segments(jpeg: bytes) -> bytes:
    com = b"\xFF\xFE" + struct.pack(">H", 2 + 11) + b"hello world"
    app1 = b"\xFF\xE1" + struct.pack(">H", 2 + 6) + b"Exif\0\0"
    first = segments(jpeg)[0][2]            # COM in front of the first segment (APP0), APP1 behind it
    return jpeg[:2] + com + jpeg[2:first] + app1 + jpeg[first:]


def pillow_jpeg(rgb, **how) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", subsampling=2, **how)
    return buf.getvalue()


OWN_QTABLES = [[min(255, 3 + 2 * ((i * 7) % 23) + i // 2) for i in range(64)], [min(255, 5 + 3 * ((i * 5) % 17) + i) for i in range(64)]]
VARIANTS = (("q30", dict(quality=30), None), ("q90", dict(quality=90), None), ("q100", dict(quality=100), None),
            ("optimize", dict(quality=75, optimize=True), None), ("restart_blocks", dict(quality=85, restart_marker_blocks=3), None),
            ("restart_rows", dict(quality=85, restart_marker_rows=1), None), ("qtables", dict(qtables=OWN_QTABLES), None),
            ("no_dht", dict(quality=80), lambda j: without(j, 0xC4)), ("merged_tables", dict(quality=60, optimize=True), lambda j: merged(merged(j, 0xDB), 0xC4)),
            ("com_app1", dict(quality=70), with_extra_segments))


@functools.lru_cache(maxsize=None)
def pillow_frames():
    """[(name, W, H, jpeg bytes)]: every variant at every size of PILLOW_SIZES, the patterns taken in turn so that every
    pattern meets every size."""
    out = []
    for v, (name, how, edit) in enumerate(VARIANTS):
        for s, (W, H) in enumerate(PILLOW_SIZES):
            pattern = PILLOW_PATTERNS[(v + s) % 3]
            jpeg = pillow_jpeg(jm.patterns(1, W, H, seed=33)[pattern][0], **how)
            out.append((f"{name}_{W}x{H}_{pattern}", W, H, edit(jpeg) if edit else jpeg))
    return out


@functools.lru_cache(maxsize=None)
def decoded_pillow_frames():
    """name -> (coefficients [mcus, 6, 64], status, quant [3, 64], W, H) of every Pillow frame, by the model."""
    return {name: jdm.decode_frame(jpeg) for name, W, H, jpeg in pillow_frames()}


def _code(table, symbol):
    code, length = jm.huffman_codes(table)[symbol]
    return format(code, f"0{length}b")


def _bits(text: str) -> bytes:
    text += "1" * (-len(text) % 8)
    raw = int(text, 2).to_bytes(len(text) // 8, "big")
    return raw.replace(b"\xFF", b"\xFF\x00")


@functools.lru_cache(maxsize=None)
def corruption_cases():
    """name -> (scan bytes, mcus, restart, the status the decoder must give): one frame each, Annex-K tables.  Bad bytes are
    refused; nothing here is meant to do anything but be refused."""
    good = jm.coefficients(jm.patterns(1, 48, 32, seed=5)["smooth"], *jm.quant_tables(90))[0].reshape(-1, 6, 64)      # 6 MCUs
    scan = jm.scan_bytes(good, 3)
    eob_y, eob_c = _code(jm.AC_LUMA, 0x00), _code(jm.AC_CHROMA, 0x00)
    dc0_y, dc0_c = _code(jm.DC_LUMA, 0), _code(jm.DC_CHROMA, 0)
    empty_mcu = (dc0_y + eob_y) * 4 + (dc0_c + eob_c) * 2
    cases = {
        "cut_short": (scan[:len(scan) // 3], 6, 6, jdm.SHORT),
        # sixteen 1 bits are no code of the Annex-K luma DC table (its longest code is 9 bits: 111111110)
        "no_such_code": (_bits("1" * 16 + "0" * 64), 1, 0, jdm.BAD_CODE),
        # DC 0, then run 15 / size 1 four times: 1 + 4 x 16 = 65 > 63
        "run_past_63": (_bits(dc0_y + (_code(jm.AC_LUMA, 0xF1) + "1") * 4 + eob_y + empty_mcu), 1, 0, jdm.RUN),
        "only_ff": (b"\xFF" * 40, 1, 0, jdm.SHORT),
        "zero_length": (b"", 1, 0, jdm.SHORT),
        "marker_count": (scan.replace(b"\xFF\xD0", b"\x12\x34"), 6, 3, jdm.MARKER_COUNT),
        "marker_order": (scan.replace(b"\xFF\xD0", b"\xFF\xD3"), 6, 3, jdm.MARKER_ORDER),
    }
    assert b"\xFF\xD0" in scan
    return cases


def category12_tables():
    """Huffman tables whose luma DC table holds a symbol 12 (a legal DHT: the categories 0..12 at 4 bits each), and a scan that
    uses it: a category-12 DC difference is outside baseline JPEG and must be refused, not decoded."""
    dc12 = ([0, 0, 0, 13] + [0] * 12, list(range(13)))
    huffman = ([dc12, jm.DC_CHROMA, jm.DC_CHROMA], ANNEX_K[1])
    scan = _bits(format(12, "04b") + "1" * 12 + _code(jm.AC_LUMA, 0x00) * 1 + "0" * 64)
    return scan, huffman
