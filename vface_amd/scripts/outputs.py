"""Where a finished batch goes: one object per run with ``write(batch)`` and ``close()``.  ``batch`` is the loop's state of the
batch (``scripts/pipeline.py`` ``Batch``): ``samples``, ``pixels``, ``pasted``, ``frame_ids`` and its stage timer."""
from __future__ import annotations

import os

import torch


def _save_png(frame_u8, path):
    from PIL import Image
    Image.fromarray(frame_u8.cpu().numpy()).save(path)                                             # :636


class _PNGSink:
    """``--png_encoder``: ``pillow`` saves frame by frame on the host, untimed, as before; ``gpu`` encodes a batch's frames in one
    call of ``scripts/png.py``'s ``PNGEncoder`` (made for the first batch's size) under the batch's ``png_out`` stage."""

    def __init__(self, opt):
        self.gpu, self.encoder = getattr(opt, "png_encoder", "pillow") == "gpu", None

    def save(self, b, paths):
        if not self.gpu:
            for f, path in enumerate(paths):
                _save_png(b.pasted[f], path)
            return
        with b.timer("png_out"):
            H, W = b.pasted.shape[1], b.pasted.shape[2]
            if self.encoder is None or (self.encoder.W, self.encoder.H) != (W, H):
                from .png import PNGEncoder
                self.encoder = PNGEncoder(W, H)
            for path, data in zip(paths, self.encoder.encode(b.pasted)):
                with open(path, "wb") as f:
                    f.write(data)


class SeededOutputs:
    """``--synthetic``: ``samples_batch{k}.pt``, ``pixels_batch{k}.pt`` and ``pasted_b{k}_f{f}.png`` under ``--Base_dir``,
    nothing with ``--skip_save``."""

    def __init__(self, opt):
        self.dir, self.save, self.png = opt.Base_dir, not opt.skip_save, _PNGSink(opt)
        os.makedirs(self.dir, exist_ok=True)

    def write(self, b):
        if not self.save:
            return
        if b.pasted is not None:
            self.png.save(b, [os.path.join(self.dir, f"pasted_b{b.id}_f{f}.png") for f in range(b.pasted.shape[0])])
        torch.save(b.samples.cpu(), os.path.join(self.dir, f"samples_batch{b.id}.pt"))
        if b.pixels is not None:
            torch.save(b.pixels.cpu(), os.path.join(self.dir, f"pixels_batch{b.id}.pt"))

    def close(self):
        pass


class ClipOutputs:
    """A clip from disk: the pasted frames as ``Base_dir/results/{index}.png`` (:636; ``--png_encoder``) unless ``--skip_save`` and, with
    ``--video_out``, as YUV4MPEG2 in frame order (:646-654: yuv420p, BT.709, tv range, 10 fps; scripts/mux.py), the batch's
    ``video_out`` stage -- or, with ``--video_codec mjpeg``, as Motion-JPEG in an AVI at ``--video_quality`` (default 90;
    scripts/mjpeg.py), the same stage -- and, with ``--gif_out``, as an animated GIF (:658; scripts/gif.py), the batch's ``gif_out``
    stage, whether or not ``--skip_save`` is given.  Each file is opened by the first batch, whose frames give its size."""

    def __init__(self, opt):
        self.dir, self.save, self.video_out, self.writer = opt.Base_dir, not opt.skip_save, opt.video_out, None
        self.codec, self.quality, self.png = opt.video_codec or "y4m", opt.video_quality, _PNGSink(opt)
        self.gif_out, self.gif_seg_pixels, self.gif = getattr(opt, "gif_out", None), getattr(opt, "gif_seg_pixels", None), None
        os.makedirs(self.dir, exist_ok=True)

    def write(self, b):
        if self.video_out:
            if self.writer is None:
                W, H = b.pasted.shape[2], b.pasted.shape[1]
                if self.codec == "mjpeg":
                    from .mjpeg import DEFAULT_QUALITY, MJPEGWriter
                    self.writer = MJPEGWriter(self.video_out, W, H, quality=DEFAULT_QUALITY if self.quality is None else self.quality)
                else:
                    from .mux import Y4MWriter
                    self.writer = Y4MWriter(self.video_out, W, H)
            with b.timer("video_out"):
                self.writer.write(b.pasted)
        if self.gif_out:
            if self.gif is None:
                from .gif import GIFWriter
                kw = {} if self.gif_seg_pixels is None else {"seg_pixels": self.gif_seg_pixels}
                self.gif = GIFWriter(self.gif_out, b.pasted.shape[2], b.pasted.shape[1], **kw)
            with b.timer("gif_out"):
                self.gif.write(b.pasted)
        if self.save:
            os.makedirs(os.path.join(self.dir, "results"), exist_ok=True)
            self.png.save(b, [os.path.join(self.dir, "results", f"{index}.png") for index in b.frame_ids])

    def close(self):
        if self.writer is not None:
            self.writer.close()
        if self.gif is not None:
            self.gif.close()
