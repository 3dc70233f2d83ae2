"""The colour half of the reference's video mux, on the GPU, and a YUV4MPEG2 writer for its result.

The reference writes every pasted frame as PNG (``REFace/scripts/VFace_inference_batch.py:636``) and then runs ffmpeg over the
folder (``:646-654``): 10 fps (``:247``), ``-pix_fmt yuv420p -colorspace bt709 -color_range tv``, libx264, plus the audio of the
target clip.  Here the RGB -> Y'CbCr conversion and the 4:2:0 subsampling are one kernel (``hip.rgb_to_yuv420``, csrc/mux.hip)
on the pasted frames where they are, and the host receives 1.5 bytes per pixel instead of 3.

- The matrix is **BT.709, limited (``tv``) range** (``:654``), chroma centre-sited; the integer arithmetic is stated in
  ``tests/mux_model.py`` and the kernel equals it bit for bit.
- **Y4M cannot tag the matrix.**  The header says ``C420jpeg`` (centre-sited 4:2:0) and ``XCOLORRANGE=LIMITED``, nothing more; an
  encoder therefore has to be told, as the reference tells it::

      ffmpeg -i out.y4m -c:v libx264 -pix_fmt yuv420p -colorspace bt709 -color_range tv out.mp4

- **Audio and H.264 are not built.**  The ``.y4m`` file is the lossless hand-off to an H.264 encoder; the compressed file this
  project writes itself is Motion-JPEG in an AVI (``scripts/mjpeg.py``, ``--video_codec mjpeg``), a different product: full-range
  BT.601, lossy, playable as it is.
"""
from __future__ import annotations

import torch

from .. import hip

REFERENCE_FPS = 10      # VFace_inference_batch.py:247, hard-coded there


def y4m_header(W: int, H: int, fps: int = REFERENCE_FPS) -> bytes:
    if min(int(W), int(H), int(fps)) <= 0:
        raise ValueError(f"y4m_header: W, H and fps must be positive; got {W}, {H}, {fps}")
    return f"YUV4MPEG2 W{int(W)} H{int(H)} F{int(fps)}:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n".encode("ascii")


def y4m_frames(i420, W: int, H: int) -> bytes:
    """The framing of I420 frames (host uint8 [F, frame_bytes], tensor or array): ``FRAME\\n`` + the planes, per frame.  No GPU."""
    n = hip.i420_frame_bytes(int(W), int(H))
    if isinstance(i420, torch.Tensor):
        if i420.is_cuda:
            raise ValueError("y4m_frames takes host bytes: copy the planes to the host first (Y4MWriter.write does)")
        i420 = i420.numpy()
    if i420.dtype.name != "uint8" or i420.ndim != 2 or i420.shape[1] != n:
        raise ValueError(f"y4m_frames: I420 frames of {W} x {H} are uint8 [F, {n}]; got {i420.dtype} {tuple(i420.shape)}")
    return b"".join(b"FRAME\n" + row.tobytes() for row in i420)


class Y4MWriter:
    """``with Y4MWriter(path, W, H) as w: w.write(pasted)`` -- ``pasted``: uint8 device frames [F, H, W, 3] as ``PasteBack.paste``
    returns them.  Each call converts on the GPU, makes ONE device-to-host copy of the I420 bytes (half the bytes of the RGB
    frames) and appends the frames to the file.  Frames of another size, and CPU tensors, are refused (``VFaceHipError``): there
    is no host conversion."""

    def __init__(self, path: str, W: int, H: int, fps: int = REFERENCE_FPS):
        self.path, self.W, self.H, self.fps = path, int(W), int(H), int(fps)
        header = y4m_header(self.W, self.H, self.fps)
        self.frames = 0
        self._f = open(path, "wb")
        self._f.write(header)

    def write(self, frames_u8: torch.Tensor) -> int:
        if self._f is None:
            raise ValueError(f"{self.path} is closed")
        if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda:
            raise hip.VFaceHipError("Y4MWriter.write: the conversion runs on the GPU; frames must be device tensors (no CPU fallback)")
        if frames_u8.dim() != 4 or tuple(frames_u8.shape[1:]) != (self.H, self.W, 3):
            raise hip.VFaceHipError(f"Y4MWriter.write: {self.path} holds {self.W} x {self.H} frames, uint8 [F, {self.H}, {self.W}, 3]; "
                                    f"got {tuple(frames_u8.shape)}")
        i420 = hip.rgb_to_yuv420(frames_u8.contiguous()).cpu()
        self._f.write(y4m_frames(i420, self.W, self.H))
        self._f.flush()
        self.frames += i420.shape[0]
        return i420.shape[0]

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
