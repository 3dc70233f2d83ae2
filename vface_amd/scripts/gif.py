"""The GIF the reference ends a run with (``clips.write_gif(...)``, ``REFace/scripts/VFace_inference_batch.py:658``), encoded on the GPU.

A GIF frame is a palette of at most 256 colours, an index per pixel and the LZW code stream of the indices.  Every stage runs where
the frames are (csrc/gif.hip): ``hip.gif_histogram`` counts the pixels in cells of 8 x 8 x 8, ``hip.gif_boxes`` cuts the counts into
up to 256 boxes (median cut), ``hip.gif_palette`` takes each box's mean colour, ``hip.gif_map`` gives every pixel its nearest entry
by exact search, and ``hip.gif_lzw`` codes the indices in independent segments of ``seg_pixels`` -- a Clear code resets the
decoder's table, so one wave codes a segment -- and frames the bits into sub-blocks.  The host adds the fixed headers below and the
768 palette bytes; it does no quantising, no LZW and no sub-block framing.  Palettes are per frame (local colour tables), so batches
are independent and the file is appended batch by batch.  No dithering, no clip-wide palette, no inter-frame transparency or cropping
(DESIGN §9).  The format is stated in ``tests/gif_model.py``; the files equal the model's byte for byte.
"""
from __future__ import annotations

import struct

import torch

from .. import hip

DELAY_CS = 10                      # hundredths of a second per frame: the reference's hard-coded fps=10 (:247)
TRAILER = b"\x3B"


def gif_header(W: int, H: int) -> bytes:
    """Signature, logical screen descriptor (no global colour table, 8 bits of colour resolution) and the NETSCAPE2.0 application
    extension with loop count 0 (forever).  No GPU."""
    W, H = int(W), int(H)
    if not (1 <= W <= hip.GIF_MAX_SIDE and 1 <= H <= hip.GIF_MAX_SIDE):
        raise ValueError(f"gif_header: a GIF's W and H are 1..{hip.GIF_MAX_SIDE}; got {W}, {H}")
    return b"GIF89a" + struct.pack("<HHBBB", W, H, 0x70, 0, 0) + b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", 0) + b"\x00"


def frame_header(W: int, H: int, delay_cs: int = DELAY_CS) -> bytes:
    """Graphic control extension (disposal 1: leave in place; no transparency; the delay) and the image descriptor of a frame that
    covers the screen, with a local colour table of 256 entries, not interlaced.  The palette and the image data follow."""
    return (b"\x21\xF9\x04\x04" + struct.pack("<H", int(delay_cs)) + b"\x00\x00"
            + b"\x2C" + struct.pack("<HHHH", 0, 0, int(W), int(H)) + b"\x87")


class GIFWriter:
    """``with GIFWriter(path, W, H) as w: w.write(pasted)`` -- ``pasted``: uint8 device frames [F, H, W, 3] as ``PasteBack.paste``
    returns them.  Each call quantises and codes the batch on the GPU, copies the palettes and the offsets in two small copies and
    then ONLY the image data that exists, and appends the frames; ``close()`` writes the trailer.  Frames of another size, and CPU
    tensors, are refused (``VFaceHipError``): there is no host encoder."""

    def __init__(self, path: str, W: int, H: int, seg_pixels: int = hip.GIF_SEG_PIXELS):
        self.path, self.W, self.H, self.seg_pixels = path, int(W), int(H), int(seg_pixels)
        if not (1 <= self.W <= hip.GIF_MAX_SIDE and 1 <= self.H <= hip.GIF_MAX_SIDE):
            raise ValueError(f"GIFWriter: a GIF's W and H are 1..{hip.GIF_MAX_SIDE}; got {W}, {H}")
        if self.W * self.H > hip.GIF_MAX_PIXELS:
            raise ValueError(f"GIFWriter: W * H stays at or below 2^24 pixels: a colour box sums up to 255 per pixel in 32 bits; got {W} x {H}")
        if not 1 <= self.seg_pixels <= hip.GIF_MAX_SEG_PIXELS:
            raise ValueError(f"GIFWriter: seg_pixels is 1..{hip.GIF_MAX_SEG_PIXELS}; got {seg_pixels}")
        self.frames, self._buf = 0, None
        self._frame_header = frame_header(self.W, self.H)
        self._f = open(path, "wb")
        self._f.write(gif_header(self.W, self.H))

    def encode(self, frames_u8: torch.Tensor):
        """-> ``(palettes, data)``: F x 768 palette bytes and the F image-data byte strings."""
        if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda:
            raise hip.VFaceHipError("GIFWriter.write: the encoder runs on the GPU; frames must be device tensors (no CPU fallback)")
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or tuple(frames_u8.shape[1:]) != (self.H, self.W, 3):
            raise hip.VFaceHipError(f"GIFWriter.write: {self.path} holds {self.W} x {self.H} frames, uint8 [F, {self.H}, {self.W}, 3]; "
                                    f"got {tuple(frames_u8.shape)}")
        F_ = frames_u8.shape[0]
        if F_ == 0:
            return [], []
        frames_u8 = frames_u8.contiguous()
        if self._buf is None or self._buf["F"] != F_ or self._buf["out"].device != frames_u8.device:
            dev, npix = frames_u8.device, self.W * self.H
            self._buf = {"F": F_, "counts": torch.empty((F_, hip.GIF_CELLS), dtype=torch.int32, device=dev),
                         "labels": torch.empty((F_, hip.GIF_CELLS), dtype=torch.uint8, device=dev),
                         "ncolors": torch.empty((F_,), dtype=torch.int32, device=dev),
                         "palette": torch.empty((F_, hip.GIF_COLORS, 3), dtype=torch.uint8, device=dev),
                         "indices": torch.empty((F_, npix), dtype=torch.uint8, device=dev),
                         "out": torch.empty(F_ * hip.gif_lzw_bound(npix, self.seg_pixels), dtype=torch.uint8, device=dev)}
        b = self._buf
        counts = hip.gif_histogram(frames_u8, out=b["counts"])
        labels, ncolors = hip.gif_boxes(counts, labels=b["labels"], ncolors=b["ncolors"])
        palette = hip.gif_palette(frames_u8, labels, out=b["palette"])
        indices = hip.gif_map(frames_u8, palette, ncolors, out=b["indices"])
        out, offsets = hip.gif_lzw(indices, self.seg_pixels, out=b["out"])
        offsets = offsets.cpu().tolist()                              # F + 1 scalars: one copy
        palettes = palette.cpu().numpy().tobytes()                    # 768 bytes per frame: one copy
        data = out[:offsets[-1]].cpu().numpy().tobytes()              # the image data that exists: one copy
        return ([palettes[768 * f:768 * (f + 1)] for f in range(F_)], [data[offsets[f]:offsets[f + 1]] for f in range(F_)])

    def write(self, frames_u8: torch.Tensor) -> int:
        if self._f is None:
            raise ValueError(f"{self.path} is closed")
        palettes, data = self.encode(frames_u8)
        for pal, image in zip(palettes, data):
            self._f.write(self._frame_header + pal + image)
        self._f.flush()
        self.frames += len(data)
        return len(data)

    def close(self):
        if self._f is None:
            return
        self._f.write(TRAILER)
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
