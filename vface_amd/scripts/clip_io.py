"""What a real-clip run reads from disk: the target frames, the source image and the landmarks file.  Host only (Pillow, numpy).

The target clip comes as the folder of ``{index}.png`` files the reference's own decoding writes, or as a YUV4MPEG2 file
(``ClipInputs.from_video`` over a ``scripts/demux.Y4MReader``: the batches then carry the file's I420 rows, which
``inputs.ClipRunInputs`` uploads and converts on the device); the H.264 decoder itself stays outside either way.

The reference decodes the target video into ``{index}.png`` files (``REFace/scripts/VFace_inference_batch.py:285``) and runs dlib
on every frame and, a second time, on every aligned crop (``ddpm.py:1068-1099`` ``get_landmarks``).  dlib is outside this build
(``scripts/intake.py:21-22``), so the landmarks are an input file, ``--landmarks FILE.npz``:

    frames        float [N, 68, 2]   dlib's 68 points of every target frame, in frame coordinates (x, y); a row of NaN = no face found
    source        float [68, 2]      the same for the source image
    crops         float [N, 68, 2]   optional: the points dlib returns on the H x W aligned crop of each frame -- what
                                     ``get_landmarks`` feeds ``landmark_proj_out``; NaN rows = no face on the crop (zeros, ddpm.py:1082)
    source_crop   float [68, 2]      optional: the same for the source's crop

Where ``crops`` / ``source_crop`` are absent they are DERIVED (``derive_crop_landmarks``): the frame points are pushed through the
projective map of the frame's aligned crop.  That stands in for the reference's second detection on the crop and is NOT equal to
it -- a detector run on the resampled crop does not return the projected points of its run on the frame.
"""
from __future__ import annotations

import os
import re
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from ..parallel import clip_batches

FRAME_NAME = re.compile(r"^(\d+)\.(png|jpg)$")


def list_frames(directory: str) -> List[Tuple[int, str]]:
    """``(index, path)`` of every ``{index}.png`` / ``{index}.jpg`` in ``directory``, by integer index (2 before 10).  Any other
    name, or an index present twice, raises ``SystemExit`` naming it."""
    if not os.path.isdir(directory):
        raise SystemExit(f"--target_frames {directory}: not a directory")
    found = {}
    for name in sorted(os.listdir(directory)):
        m = FRAME_NAME.match(name)
        if m is None:
            raise SystemExit(f"--target_frames {directory}: {name!r} is not a frame file ({{index}}.png or {{index}}.jpg)")
        idx = int(m.group(1))
        if idx in found:
            raise SystemExit(f"--target_frames {directory}: frame {idx} is there twice ({os.path.basename(found[idx])!r} and {name!r})")
        found[idx] = os.path.join(directory, name)
    return sorted(found.items())


def load_image(path: str) -> torch.Tensor:
    """``Image.open(path).convert("RGB")`` -> uint8 [H, W, 3] (host)."""
    from PIL import Image
    with Image.open(path) as im:
        return torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8))


def load_frames(paths) -> torch.Tensor:
    """The frames of ``paths`` as one uint8 [F, H, W, 3] host tensor; a frame of another size than the first raises ``SystemExit``."""
    frames = [load_image(p) for p in paths]
    for p, f in zip(paths, frames):
        if f.shape != frames[0].shape:
            raise SystemExit(f"--target_frames: {p} is {f.shape[1]} x {f.shape[0]}, {paths[0]} is {frames[0].shape[1]} x "
                             f"{frames[0].shape[0]}: the frames of a clip must all be one size")
    return torch.stack(frames)


class Landmarks(NamedTuple):
    frames: np.ndarray                      # float64 [N, 68, 2]
    source: np.ndarray                      # float64 [68, 2]
    crops: Optional[np.ndarray]             # float64 [N, 68, 2] | None
    source_crop: Optional[np.ndarray]       # float64 [68, 2] | None


def load_landmarks(path: str, n_frames: Optional[int] = None) -> Landmarks:
    """Read and check ``--landmarks FILE.npz`` (layout: this module's docstring).  ``n_frames``: the frames the run will use; a file
    with fewer rows raises ``SystemExit``."""
    with np.load(path) as z:
        have = {k: np.asarray(z[k], dtype=np.float64) for k in z.files}
    for key in ("frames", "source"):
        if key not in have:
            raise SystemExit(f"--landmarks {path}: no array {key!r} (has {sorted(have)})")
    unknown = set(have) - {"frames", "source", "crops", "source_crop"}
    if unknown:
        raise SystemExit(f"--landmarks {path}: unknown array(s) {sorted(unknown)}")
    fr, src = have["frames"], have["source"]
    if fr.ndim != 3 or fr.shape[1:] != (68, 2):
        raise SystemExit(f"--landmarks {path}: 'frames' must be [N, 68, 2]; got {list(fr.shape)}")
    if n_frames is not None and fr.shape[0] < n_frames:
        raise SystemExit(f"--landmarks {path}: 'frames' has {fr.shape[0]} rows, the run needs {n_frames}")
    if src.shape != (68, 2) or not np.isfinite(src).all():
        raise SystemExit(f"--landmarks {path}: 'source' must be a finite [68, 2]; got {list(src.shape)}")
    crops, src_crop = have.get("crops"), have.get("source_crop")
    if crops is not None and crops.shape != fr.shape:
        raise SystemExit(f"--landmarks {path}: 'crops' must be {list(fr.shape)} like 'frames'; got {list(crops.shape)}")
    if src_crop is not None and src_crop.shape != (68, 2):
        raise SystemExit(f"--landmarks {path}: 'source_crop' must be [68, 2]; got {list(src_crop.shape)}")
    return Landmarks(fr, src, crops, src_crop)


def fallback_indices(frames_lm: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``(found [N] bool, take [N] int)``: ``found[i]`` = frame i has landmarks (no NaN in its row); ``take[i]`` = the frame whose
    aligned crop, label map and inverse transform frame i uses -- itself, or the last frame before it that has landmarks (the
    reference's ``except`` branch, VFace_inference_batch.py:297-303).  Frame 0 without landmarks raises ``SystemExit``: there is
    nothing before it."""
    found = np.isfinite(frames_lm).all(axis=(1, 2))
    if found.size == 0 or not found[0]:
        raise SystemExit("--landmarks: frame 0 has no landmarks (NaN row) and no frame before it to take the crop from")
    take = np.maximum.accumulate(np.where(found, np.arange(found.size), 0))
    return found, take


def derive_crop_landmarks(points, coeffs, image_size: int, H: int, W: int) -> np.ndarray:
    """Frame points [68, 2] -> their place on the H x W aligned crop: ``(p + 0.5)`` through the frame's ``inv_transforms`` row
    ``coeffs`` [8] (frame -> ``image_size`` canvas, projective), scaled to H x W, minus 0.5, ``np.rint``.  A stand-in for dlib on
    the crop, not equal to it (module docstring)."""
    p = np.asarray(points, dtype=np.float64) + 0.5
    a = np.asarray(coeffs, dtype=np.float64)
    den = a[6] * p[:, 0] + a[7] * p[:, 1] + 1.0
    x = (a[0] * p[:, 0] + a[1] * p[:, 1] + a[2]) / den
    y = (a[3] * p[:, 0] + a[4] * p[:, 1] + a[5]) / den
    return np.rint(np.stack([x * (W / float(image_size)) - 0.5, y * (H / float(image_size)) - 0.5], axis=1))


def conditioning_landmarks(lm: Landmarks, found, take, coeffs, ids, image_size: int, H: int, W: int) -> np.ndarray:
    """float32 [len(ids), 136]: what ``landmark_proj_out`` sees for the frames ``ids`` -- ``crops`` flattened where the file has
    them, derived from ``frames`` and each frame's OWN ``coeffs`` row otherwise; zeros where no face was found (ddpm.py:1082)."""
    out = np.zeros((len(ids), 136), np.float32)
    for row, i in enumerate(ids):
        if not found[i]:
            continue
        if lm.crops is not None:
            pts = lm.crops[i]
            if not np.isfinite(pts).all():
                continue
        else:
            pts = derive_crop_landmarks(lm.frames[i], coeffs[row], image_size, H, W)
        out[row] = pts.reshape(136)
    return out


def source_conditioning_landmarks(lm: Landmarks, coeffs, image_size: int, H: int, W: int) -> np.ndarray:
    pts = lm.source_crop if lm.source_crop is not None else derive_crop_landmarks(lm.source, coeffs, image_size, H, W)
    return (pts if np.isfinite(pts).all() else np.zeros((68, 2))).reshape(1, 136).astype(np.float32)


class ClipInputs:
    """The inputs of a real-clip run, as the pipeline of ``VFace_inference_batch.py`` asks for them batch by batch: what
    ``synthetic_intake_inputs`` and the seeded landmarks stand in for in a ``--synthetic`` run.  Host only.

    ``quads`` / ``coeffs`` hold, for every frame, the quad (``quad_from_landmarks``) and the ``inv_transforms(.., image_size)`` row
    of the frame it TAKES its crop from (``fallback_indices``); ``landmarks`` the conditioning rows [n, 136]."""

    def __init__(self, target_frames: str, src_image: str, landmarks: str, n_frames: int, H: int, W: int, image_size: int = 1024):
        listed = list_frames(target_frames)
        if len(listed) < n_frames:
            raise SystemExit(f"--target_frames {target_frames}: {len(listed)} frame file(s), --n_frames asks for {n_frames}")
        listed = listed[:n_frames]
        self.video = None           # (a folder of frame files)
        self.frame_ids = [i for i, _ in listed]
        self.paths = [p for _, p in listed]
        self.size = None            # (H, W) of the clip's frames, known after the first batch
        self._set_up(src_image, landmarks, n_frames, H, W, image_size)

    @classmethod
    def from_video(cls, video, src_image: str, landmarks: str, n_frames: int, H: int, W: int, image_size: int = 1024):
        """The same inputs over a ``scripts/demux.Y4MReader`` or a ``scripts/mjpeg_in.MJPEGReader`` instead of a folder: frame ids
        0 .. n_frames - 1, and ``batch`` hands out what the reader's ``read`` returns -- the I420 rows of the file, uint8
        [F, frame_bytes], or an ``MJPEGFrames`` of compressed scans -- where the folder form hands out RGB frames (the conversion
        is the device's: the reader's ``to_rgb``, called by ``inputs.ClipRunInputs``).  One frame size by construction."""
        if len(video) < n_frames:
            raise SystemExit(f"--target_video {video.path}: {len(video)} frame(s), --n_frames asks for {n_frames}")
        self = cls.__new__(cls)
        self.video = video
        self.frame_ids = list(range(n_frames))
        self.paths = None
        self.size = (video.H, video.W)
        self._set_up(src_image, landmarks, n_frames, H, W, image_size)
        return self

    @classmethod
    def from_png_folder(cls, target_frames: str, src_image: str, landmarks: str, n_frames: int, H: int, W: int, image_size: int = 1024):
        """The folder form with the frames decoded on the device (``--png_decoder gpu``): the folder's own ``frame_ids`` and
        ``paths`` as ``__init__`` keeps them, and ``batch`` hands out the ``PNGFrames`` that a ``scripts/png_in.PNGFolderReader``
        over those paths read -- parsed files, not pixels; the reader's ``to_rgb`` decodes them (``inputs.ClipRunInputs``).  The
        clip's size is the first file's IHDR; a ``.jpg`` in the folder is refused by name."""
        from .png_in import PNGFolderReader
        listed = list_frames(target_frames)
        if len(listed) < n_frames:
            raise SystemExit(f"--target_frames {target_frames}: {len(listed)} frame file(s), --n_frames asks for {n_frames}")
        listed = listed[:n_frames]
        self = cls.__new__(cls)
        self.frame_ids = [i for i, _ in listed]
        self.paths = [p for _, p in listed]
        self.video = PNGFolderReader(self.paths, f"--target_frames {target_frames}")
        self.size = (self.video.H, self.video.W)
        self._set_up(src_image, landmarks, n_frames, H, W, image_size)
        return self

    def _set_up(self, src_image, landmarks, n_frames, H, W, image_size):
        from .intake import inv_transforms, quad_from_landmarks
        self.source_u8 = load_image(src_image)[None]                 # [1, Hs, Ws, 3]
        lm = load_landmarks(landmarks, n_frames)
        self.found, self.take = fallback_indices(lm.frames[:n_frames])
        self.quads = np.stack([quad_from_landmarks(lm.frames[t]) for t in self.take])
        self.coeffs = inv_transforms(self.quads, image_size)
        self.landmarks = conditioning_landmarks(lm, self.found, self.take, self.coeffs, range(n_frames), image_size, H, W)
        self.source_quad = quad_from_landmarks(lm.source)[None]
        self.source_landmarks = source_conditioning_landmarks(lm, inv_transforms(self.source_quad, image_size)[0], image_size, H, W)

    def _read(self, indices) -> torch.Tensor:
        """Frames ``indices`` of the clip: RGB [n, Hs, Ws, 3] from a folder (checked against the clip's size), I420 rows
        [n, frame_bytes] from a video file."""
        if self.video is not None:
            return self.video.read(indices)
        frames = load_frames([self.paths[i] for i in indices])
        if self.size is None:
            self.size = tuple(frames.shape[1:3])
        if tuple(frames.shape[1:3]) != self.size:
            raise SystemExit(f"--target_frames: {self.paths[indices[0]]} is {frames.shape[2]} x {frames.shape[1]}, the clip's first frames "
                             f"are {self.size[1]} x {self.size[0]}: the frames of a clip must all be one size")
        return frames

    def batch(self, batch_id: int, F: int, whole_clip: bool = False) -> dict:
        """Frames ``[batch_id * F, (batch_id + 1) * F)`` of the clip -- ``whole_clip``: batch ``batch_id`` of the plan that covers
        every frame (``parallel.clip_batches``: the last batch may be shorter than F) --: ``frames`` uint8 [F, Hs, Ws, 3], each frame itself (pasted
        into); ``crop_frames``: the frames the crops are cut from (a frame without landmarks: the one it takes, read again);
        ``quads`` [F, 4, 2], ``coeffs`` [F, 8], ``landmarks`` float32 [F, 136], ``found`` bool [F], ``frame_ids``.  Over a video file
        ``frames`` and ``crop_frames`` are I420 rows [F, frame_bytes] (``from_video``)."""
        first, count = clip_batches(len(self.frame_ids), F)[batch_id] if whole_clip else (batch_id * F, F)
        sl = slice(first, first + count)
        own = list(range(sl.start, sl.stop))
        frames = self._read(own)
        crop_frames = frames
        if any(self.take[i] != i for i in own):
            crop_frames = frames.clone()
            for row, i in enumerate(own):
                t = int(self.take[i])
                if t != i:
                    # (a frame of an earlier batch passed the size check when its own batch was read)
                    crop_frames[row] = frames[t - sl.start] if t >= sl.start else self._read_again(t)
        return {"frames": frames, "crop_frames": crop_frames, "quads": self.quads[sl], "coeffs": self.coeffs[sl],
                "landmarks": self.landmarks[sl], "found": self.found[sl], "frame_ids": [self.frame_ids[i] for i in own]}

    def _read_again(self, t: int) -> torch.Tensor:
        return self.video.read([t])[0] if self.video is not None else load_image(self.paths[t])
