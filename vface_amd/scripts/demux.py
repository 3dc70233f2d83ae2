"""The way in for a target clip: a YUV4MPEG2 reader, the inverse of ``scripts/mux.py`` ``y4m_header`` / ``y4m_frames``.  Host only.

The reference decodes the target video itself (``REFace/scripts/VFace_inference_batch.py:240-285``: ``cv2.VideoCapture``, BGR ->
RGB, one PNG per frame).  The H.264 decoder is not built here; what is read is the lossless hand-off every decoder can write::

    ffmpeg -i in.mp4 -pix_fmt yuv420p clip.y4m

``Y4MReader`` hands out the I420 planes as they lie in the file -- 1.5 bytes per pixel, which is what crosses to the device -- and
``hip.yuv420_to_rgb`` (csrc/demux.hip) makes the RGB frames there.

- **8-bit progressive 4:2:0 only**: ``C420jpeg`` / ``C420`` / no ``C`` tag (chroma centre-sited) and ``C420mpeg2`` (horizontally
  co-sited); ``C420paldv``, 4:2:2, 4:4:4, mono, every high-bit-depth form and interlaced streams are refused by name.
- **Y4M cannot tag the matrix.**  ``XCOLORRANGE=FULL|LIMITED`` is read (limited where absent); BT.709 or BT.601 is the caller's
  to say (``--video_in_matrix``).
- **Files only**: frames are found by reading the ``FRAME`` lines on open and read by ``seek``; a pipe cannot be indexed.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple

import numpy as np
import torch

MAGIC = b"YUV4MPEG2"
CHROMA_SITING = {"420jpeg": "centre", "420": "centre", "420mpeg2": "left"}
FFMPEG_LINE = "ffmpeg -i in.mp4 -pix_fmt yuv420p clip.y4m"
MAX_LINE = 4096         # a header or FRAME line longer than this is not one


class Y4MHeader(NamedTuple):
    W: int
    H: int
    fps: tuple              # (numerator, denominator); (0, 0) = unknown
    interlace: str          # "p" | "?"
    aspect: str             # "n:d" as written, "" where absent
    siting: str             # "centre" | "left": where the header says the chroma samples sit
    full_range: bool
    x_tags: dict


def frame_bytes(W: int, H: int) -> int:
    return W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)


def parse_y4m_header(line, path: str = "<y4m>") -> Y4MHeader:
    """The stream header line (bytes or str, with or without its newline).  Unsupported streams raise ``SystemExit`` naming the tag
    and ``path``."""
    if isinstance(line, bytes):
        line = line.decode("ascii", errors="replace")
    words = line.rstrip("\n").split(" ")
    if words[0] != MAGIC.decode():
        raise SystemExit(f"{path}: not a YUV4MPEG2 stream (the header starts with {words[0][:16]!r})")
    W = H = None
    fps, interlace, aspect, colour, x_tags = (0, 0), "p", "", "420jpeg", {}
    for w in filter(None, words[1:]):
        key, val = w[0], w[1:]
        try:
            if key == "W":
                W = int(val)
            elif key == "H":
                H = int(val)
            elif key == "F":
                n, _, d = val.partition(":")
                fps = (int(n), int(d))
            elif key == "I":
                interlace = val
            elif key == "A":
                aspect = val
            elif key == "C":
                colour = val
            elif key == "X":
                k, _, v = val.partition("=")
                x_tags[k] = v
            else:
                raise SystemExit(f"{path}: unknown header tag {w!r}")
        except ValueError:
            raise SystemExit(f"{path}: header tag {w!r} does not parse") from None
    if W is None or H is None or W <= 0 or H <= 0:
        raise SystemExit(f"{path}: the header gives no frame size (W{W} H{H})")
    if interlace not in ("p", "?"):
        raise SystemExit(f"{path}: tag I{interlace}: interlaced streams are not read; deinterlace first ({FFMPEG_LINE} -vf yadif)")
    if colour not in CHROMA_SITING:
        raise SystemExit(f"{path}: tag C{colour}: only 8-bit 4:2:0 is read (C420jpeg, C420mpeg2, C420); convert with `{FFMPEG_LINE}`")
    rng = x_tags.get("COLORRANGE", "LIMITED")
    if rng not in ("FULL", "LIMITED"):
        raise SystemExit(f"{path}: tag XCOLORRANGE={rng}: FULL or LIMITED")
    return Y4MHeader(W, H, fps, interlace, aspect, CHROMA_SITING[colour], rng == "FULL", x_tags)


class Y4MReader:
    """``Y4MReader(path)``: the header (``.header``, ``.W``, ``.H``), ``len()`` = the frame count, ``read(indices)`` = host uint8
    ``[F, frame_bytes]`` in the order asked for.  The frames are indexed on open from their ``FRAME...\\n`` lines alone (parameters
    after ``FRAME`` are allowed, so offsets are found, not computed); the planes are only ever read by ``read``.
    ``to_rgb`` is the surface it shares with ``mjpeg_in.MJPEGReader``: what ``read`` returned -> RGB frames on the device."""
    fixed_matrix = None             # Y4M cannot tag the matrix: --video_in_matrix says it

    def __init__(self, path: str):
        self.path = path
        if not os.path.isfile(path):
            raise SystemExit(f"{path}: no such file (a YUV4MPEG2 file is read by seek; a pipe cannot be)")
        self._f = open(path, "rb")
        try:
            self._index()
        except BaseException:
            self.close()
            raise

    def _index(self):
        path = self.path
        size = os.fstat(self._f.fileno()).st_size
        first = self._f.readline(MAX_LINE)
        if not first.startswith(MAGIC + b" ") or not first.endswith(b"\n"):
            raise SystemExit(f"{path}: does not start with {MAGIC.decode()!r}: this looks like a container or another format, not Y4M; "
                             f"decode it first: `{FFMPEG_LINE}`")
        self.header = parse_y4m_header(first, path)
        self.W, self.H = self.header.W, self.header.H
        self.frame_bytes = frame_bytes(self.W, self.H)
        self.offsets: List[int] = []
        pos = len(first)
        while pos < size:
            self._f.seek(pos)
            line = self._f.readline(MAX_LINE)
            k = len(self.offsets)
            if not line.startswith(b"FRAME") or not line.endswith(b"\n") or line[5:6] not in (b"\n", b" "):
                raise SystemExit(f"{path}: frame {k}: no FRAME marker at byte {pos} (found {line[:8]!r})")
            pos += len(line)
            if pos + self.frame_bytes > size:
                raise SystemExit(f"{path}: frame {k} is truncated: {size - pos} of {self.frame_bytes} bytes "
                                 f"({self.W} x {self.H}, 4:2:0)")
            self.offsets.append(pos)
            pos += self.frame_bytes

    def __len__(self):
        return len(self.offsets)

    def read(self, indices) -> torch.Tensor:
        if self._f is None:
            raise ValueError(f"{self.path} is closed")
        indices = [int(i) for i in indices]
        out = np.empty((len(indices), self.frame_bytes), np.uint8)
        for row, i in enumerate(indices):
            if not 0 <= i < len(self.offsets):
                raise IndexError(f"{self.path}: frame {i} of {len(self.offsets)}")
            self._f.seek(self.offsets[i])
            if self._f.readinto(memoryview(out[row])) != self.frame_bytes:
                raise SystemExit(f"{self.path}: frame {i} is truncated (the file changed while it was read)")
        return torch.from_numpy(out)

    def to_rgb(self, i420: torch.Tensor, device, matrix: str = "bt709", chroma_upsample: str = "sited") -> torch.Tensor:
        """I420 rows as ``read`` returns them -> device uint8 [F, H, W, 3]: the rows are uploaded as they are (1.5 bytes per pixel)
        and ``hip.yuv420_to_rgb`` converts them there; range and chroma siting from the file's header."""
        from .. import hip
        head = self.header
        return hip.yuv420_to_rgb(i420.to(device), head.W, head.H, matrix=matrix, full_range=head.full_range,
                                 chroma="nearest" if chroma_upsample == "nearest" else head.siting)

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
