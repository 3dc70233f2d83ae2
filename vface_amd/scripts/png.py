"""The reference's main output, one PNG per pasted frame (``REFace/scripts/VFace_inference_batch.py:636``), encoded on the GPU.

PNG compression is a filter per row followed by zlib.  ``hip.png_filter`` picks every row's filter by the minimum sum of absolute
values and ``hip.png_deflate`` codes the filtered rows in independent stripes of ``stripe_rows`` rows -- one dynamic-Huffman block of
literals and distance-1 matches each, zlib's ``Z_RLE`` token set -- where the frames are (csrc/png.hip).  The host receives the
compressed bytes and O(stripes) scalars: per frame a length, per stripe the two halves of Adler-32.  It combines the checksums
(``adler32_combine``), and adds ``78 01``, the chunk framing and the chunk CRC (``png_file``).  There is no host compressor on this
path, and no LZ77 beyond distance 1: a noise-free synthetic gradient comes out larger than Pillow's level 6, decoded video smaller
(DESIGN §9).  The format is stated in ``tests/png_model.py``; the files equal the model's byte for byte.
"""
from __future__ import annotations

import struct
import zlib

import torch

from .. import hip

ADLER_MODULUS = 65521
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def adler32_combine(parts) -> int:
    """``[(s1, s2, length)]`` of consecutive pieces, each the Adler-32 halves of the piece alone (started from 1, 0) -> Adler-32 of
    their concatenation.  O(pieces) scalar work: s1 adds up less the extra 1s; a piece's s2 grows by its length times what s1 was
    in front of it."""
    s1, s2 = 1, 0
    for p1, p2, n in parts:
        s2 = (s2 + int(p2) + (int(n) % ADLER_MODULUS) * ((s1 - 1) % ADLER_MODULUS)) % ADLER_MODULUS
        s1 = (s1 + int(p1) - 1) % ADLER_MODULUS
    return (s2 << 16) | s1


def _chunk(kind: bytes, payload: bytes) -> bytes:
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(payload, zlib.crc32(kind)))


def png_file(W: int, H: int, body: bytes, adler: int) -> bytes:
    """One complete PNG: signature, IHDR (8-bit RGB, colour type 2, no interlace), one IDAT -- ``78 01``, the deflate body as
    ``hip.png_deflate`` makes it, Adler-32 of the filtered bytes -- and IEND.  No GPU."""
    W, H = int(W), int(H)
    if not (1 <= W < 1 << 31 and 1 <= H < 1 << 31):
        raise ValueError(f"png_file: W and H are 1..2^31 - 1; got {W}, {H}")
    stream = b"\x78\x01" + bytes(body) + struct.pack(">I", int(adler))
    return SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", stream) + _chunk(b"IEND", b"")


class PNGEncoder:
    """``PNGEncoder(W, H).encode(pasted)`` -- ``pasted``: uint8 device frames [F, H, W, 3] as ``PasteBack.paste`` returns them -> a list
    of F complete PNG files as ``bytes``.  A call filters and deflates the whole batch on the GPU, copies the lengths and the
    checksum halves in one small copy and then ONLY the compressed bytes in one more.  Frames of another size, and CPU tensors, are
    refused (``VFaceHipError``): there is no host encoder."""

    def __init__(self, W: int, H: int, stripe_rows: int = hip.PNG_STRIPE_ROWS):
        self.W, self.H, self.stripe_rows = int(W), int(H), int(stripe_rows)
        if min(self.W, self.H, self.stripe_rows) <= 0:
            raise ValueError(f"PNGEncoder: W, H and stripe_rows must be positive; got {W}, {H}, {stripe_rows}")
        self.row_bytes = 1 + 3 * self.W
        self.stripes = (self.H + self.stripe_rows - 1) // self.stripe_rows
        self._stripe_bytes = [min(self.stripe_rows, self.H - r) * self.row_bytes for r in range(0, self.H, self.stripe_rows)]
        self._rows = self._out = None

    def encode(self, frames_u8: torch.Tensor):
        if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda:
            raise hip.VFaceHipError("PNGEncoder.encode: the encoder runs on the GPU; frames must be device tensors (no CPU fallback)")
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or tuple(frames_u8.shape[1:]) != (self.H, self.W, 3):
            raise hip.VFaceHipError(f"PNGEncoder.encode: this encoder takes {self.W} x {self.H} frames, uint8 [F, {self.H}, {self.W}, 3]; "
                                    f"got {tuple(frames_u8.shape)}")
        F_ = frames_u8.shape[0]
        if F_ == 0:
            return []
        if self._rows is None or self._rows.shape[0] != F_ or self._rows.device != frames_u8.device:
            self._rows = torch.empty((F_, self.H, self.row_bytes), dtype=torch.uint8, device=frames_u8.device)
            self._out = torch.empty(F_ * hip.png_deflate_bound(self.row_bytes, self.H, self.stripe_rows), dtype=torch.uint8,
                                    device=frames_u8.device)
        rows = hip.png_filter(frames_u8.contiguous(), out=self._rows)
        out, meta, _ = hip.png_deflate(rows, self.stripe_rows, out=self._out)
        meta = meta.cpu().tolist()                                  # the lengths and the checksum halves: one copy
        lengths, halves = meta[:F_], meta[F_:]
        data = out[:sum(lengths)].cpu().numpy().tobytes()          # the compressed bytes: one copy
        files, at = [], 0
        for f, n in enumerate(lengths):
            h = halves[2 * f * self.stripes:2 * (f + 1) * self.stripes]
            adler = adler32_combine([(h[2 * s], h[2 * s + 1], self._stripe_bytes[s]) for s in range(self.stripes)])
            files.append(png_file(self.W, self.H, data[at:at + n], adler))
            at += n
        return files
