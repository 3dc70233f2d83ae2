"""The reference's compressed video out, as Motion-JPEG in an AVI: a baseline JPEG encoder on the GPU and the writer of its file.

The reference ends in a playable compressed file (``REFace/scripts/VFace_inference_batch.py:646-658``: ffmpeg makes an mp4 and a
gif of the PNG frames).  H.264 is not built here; baseline JPEG is: ``hip.jpeg_coefficients`` (colour matrix, 2 x 2 chroma mean,
8 x 8 DCT, quantisation) and ``hip.jpeg_entropy`` (Huffman coding in restart intervals, one wave each) of csrc/mjpeg.hip turn
the pasted frames into the scan bytes of one 4:2:0 JPEG per frame where the frames are, the host receives the compressed bytes
only -- roughly a tenth of the I420 planes of ``scripts/mux.py`` at quality 90 -- and ``MJPEGWriter`` frames them: SOI, JFIF
APP0, two DQT, SOF0, four DHT (the typical tables of T.81 Annex K), DRI, SOS, the scan, EOI, one ``00dc`` chunk per frame in a
RIFF ``AVI `` with an ``idx1`` index.  ffmpeg, VLC, mpv and OpenCV open the file; every frame is a ``.jpg`` of its own.

- The matrix is **full-range BT.601 (JFIF)**: what every MJPEG decoder assumes.  It is not the BT.709 ``tv`` range of the
  ``.y4m`` path (``scripts/mux.py``), which stays the lossless hand-off to an H.264 encoder.
- The quantisation tables are libjpeg's: the Annex-K base tables scaled by ``quality`` (``quant_tables``), the tables Pillow's
  ``quality=`` yields.  The integer arithmetic is stated in ``tests/jpeg_model.py`` and the kernels equal it bit for bit; its error
  against the source is that of libjpeg's own encoder.
- The restart interval is one MCU row: the rows of a frame are coded independently, by one wave each.
- **Audio, H.264 and OpenDML are not built**: a file that would pass 4 GiB is refused before the frame that would break it.
"""
from __future__ import annotations

import struct

import torch

from .. import hip
from .mux import REFERENCE_FPS

# T.81 Annex K: the quantisation base tables, row-major, and the typical Huffman tables as (BITS, HUFFVAL)
BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
             100, 103, 99)
BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
               99) + (99,) * 32
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
          56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
DHT = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D),
     (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
      0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A,
      0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53,
      0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
      0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
      0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9,
      0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2,
      0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
     (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
      0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17,
      0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A,
      0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
      0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
      0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7,
      0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2,
      0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA)),
)
DEFAULT_QUALITY = 90
RIFF_LIMIT = 0xFFFFFFFF         # the RIFF size field; OpenDML (AVI 2.0) is not built


def quant_tables(quality: int):
    """libjpeg's scaling of the Annex-K base tables (``jpeg_set_quality``, baseline): 5000 / q below 50, 200 - 2 q from 50 up,
    results clamped to 1..255 -- the tables Pillow's ``quality=`` yields.  -> (luma, chroma), tuples of 64 ints, row-major."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quant_tables: quality is 1..100; got {quality}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(255, max(1, (b * scale + 50) // 100)) for b in base) for base in (BASE_LUMA, BASE_CHROMA))


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes((0xFF, marker)) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_header(W: int, H: int, tables, restart: int) -> bytes:
    """Everything of a frame in front of its scan: SOI, JFIF APP0, two DQT (zigzag order), SOF0 (Y 2 x 2, Cb and Cr 1 x 1), the four
    DHT, DRI, SOS."""
    W, H, restart = int(W), int(H), int(restart)
    if not (1 <= W <= 65535 and 1 <= H <= 65535 and 1 <= restart <= 65535):
        raise ValueError(f"jpeg_header: W, H and restart are 1..65535; got {W}, {H}, {restart}")
    out = bytearray(b"\xFF\xD8")
    out += _segment(0xE0, b"JFIF\0" + bytes((1, 1, 0, 0, 1, 0, 1, 0, 0)))
    for i, table in enumerate(tables):
        out += _segment(0xDB, bytes((i,)) + bytes(int(table[z]) for z in ZIGZAG))
    out += _segment(0xC0, bytes((8,)) + struct.pack(">HH", H, W) + bytes((3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for cls_id, bits, vals in DHT:
        out += _segment(0xC4, bytes((cls_id,)) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", restart))
    out += _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))
    return bytes(out)


def jpeg_frame(W: int, H: int, tables, restart: int, scan: bytes) -> bytes:
    """One complete JPEG: the header, the scan as ``hip.jpeg_entropy`` makes it, EOI.  No GPU."""
    return jpeg_header(W, H, tables, restart) + bytes(scan) + b"\xFF\xD9"


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def avi_header(W: int, H: int, fps: int, frames: int, biggest: int, movi_bytes: int) -> bytes:
    """RIFF header, ``hdrl`` (``avih``; one ``strl``: ``strh`` vids / MJPG, ``strf`` a BITMAPINFOHEADER with biCompression MJPG) and
    the head of the ``movi`` list, for a file of ``frames`` frames whose largest is ``biggest`` bytes and whose ``movi`` list holds
    ``movi_bytes`` (the fourcc and the padded chunks).  Its length does not depend on the counts: ``close()`` writes it again."""
    avih = struct.pack("<14I", 1000000 // fps, min(biggest * fps, 0xFFFFFFFF), 0, 0x10, frames, 0, 1, biggest, W, H, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIiI4H", 0, 0, 0, 0, 1, fps, 0, frames, biggest, -1, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = _chunk(b"LIST", b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)))
    riff = 4 + len(hdrl) + 8 + movi_bytes + 8 + 16 * frames
    return b"RIFF" + struct.pack("<I", riff) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_bytes) + b"movi"


class MJPEGWriter:
    """``with MJPEGWriter(path, W, H, quality=90) as w: w.write(pasted)`` -- ``pasted``: uint8 device frames [F, H, W, 3] as
    ``PasteBack.paste`` returns them.  Each call encodes on the GPU, copies the lengths and then ONLY the compressed bytes to the
    host, and appends one ``00dc`` chunk per frame; ``close()`` writes the index and patches the sizes and counts.  Frames of
    another size, and CPU tensors, are refused (``VFaceHipError``): there is no host encoder."""

    def __init__(self, path: str, W: int, H: int, fps: int = REFERENCE_FPS, quality: int = DEFAULT_QUALITY):
        self.path, self.W, self.H, self.fps, self.quality = path, int(W), int(H), int(fps), int(quality)
        if self.fps <= 0:
            raise ValueError(f"MJPEGWriter: fps must be positive; got {fps}")
        self.tables = quant_tables(self.quality)
        self.restart = hip.jpeg_mcu_grid(self.W, self.H)[1]             # one MCU row
        self._header = jpeg_header(self.W, self.H, self.tables, self.restart)
        self.frames, self._index, self._biggest, self._q = 0, [], 0, None
        self._f = open(path, "wb")
        self._f.write(avi_header(self.W, self.H, self.fps, 0, 0, 4))
        self._movi = self._f.tell() - 4                                 # where the 'movi' fourcc stands: idx1 offsets count from it
        self._pos = self._f.tell()

    def write(self, frames_u8: torch.Tensor) -> int:
        if self._f is None:
            raise ValueError(f"{self.path} is closed")
        if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda:
            raise hip.VFaceHipError("MJPEGWriter.write: the encoder runs on the GPU; frames must be device tensors (no CPU fallback)")
        if frames_u8.dim() != 4 or tuple(frames_u8.shape[1:]) != (self.H, self.W, 3):
            raise hip.VFaceHipError(f"MJPEGWriter.write: {self.path} holds {self.W} x {self.H} frames, uint8 [F, {self.H}, {self.W}, 3]; "
                                    f"got {tuple(frames_u8.shape)}")
        if self._q is None or self._q[0].device != frames_u8.device:
            self._q = tuple(torch.tensor(t, dtype=torch.uint8, device=frames_u8.device) for t in self.tables)
        coef = hip.jpeg_coefficients(frames_u8.contiguous(), *self._q)
        scans, lengths = hip.jpeg_entropy(coef, self.restart)
        lengths = lengths.cpu().tolist()
        data = scans[:sum(lengths)].cpu().numpy().tobytes()
        at = 0
        for n in lengths:
            self._append(self._header + data[at:at + n] + b"\xFF\xD9")
            at += n
        self._f.flush()
        return len(lengths)

    def _append(self, jpeg: bytes):
        """One complete JPEG as the next ``00dc`` chunk, even-padded, and its index entry; refused if the finished file (this
        chunk, the index with it, the patched headers) would pass the 4 GiB a RIFF size field holds."""
        size = len(jpeg)
        end = self._pos + 8 + size + (size & 1) + 8 + 16 * (self.frames + 1)
        if end > RIFF_LIMIT + 8:
            raise ValueError(f"{self.path}: frame {self.frames} would take the file past 4 GiB; OpenDML is not built "
                             f"(the {self.frames} frames written so far stay valid: close() finishes the file)")
        self._f.write(_chunk(b"00dc", jpeg))
        self._index.append((self._pos - self._movi, size))
        self._pos += 8 + size + (size & 1)
        self._biggest = max(self._biggest, size)
        self.frames += 1

    def close(self):
        if self._f is None:
            return
        self._f.write(_chunk(b"idx1", b"".join(b"00dc" + struct.pack("<III", 0x10, off, size) for off, size in self._index)))
        self._f.seek(0)
        self._f.write(avi_header(self.W, self.H, self.fps, self.frames, self._biggest, self._pos - self._movi))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
