"""Frame intake on the GPU: decoded video frame -> 1024 x 1024 aligned crop -> the tensors the sampler consumes.

The mirror image of ``paste_back.py``.  The reference runs this front end on the host, frame by frame, with Pillow and numpy:
``crop_image`` (``REFace/src/utils/alignmengt.py:99-145``, reached from ``crop_faces_by_quads :255-263``),
``VideoDataset.__getitem_gray__`` (``REFace/ldm/data/video_swap_dataset.py:135-240``) and the mask resize of
``REFace/scripts/VFace_inference_batch.py:459``.  Here a batch of frames stays in HBM and each step is one launch of
``csrc/intake.hip`` / ``csrc/paste.hip`` (8-bit results bit-identical to Pillow's):

    reference (per frame)                                                              here (whole batch)
    ---------------------------------------------------------------------------------  -------------------------------------------
    shrink = floor(qsize / size / 2); img.resize(rsize, ANTIALIAS)      alignmengt :108-114   hip.resample_u8, Lanczos tables
    border, crop window, img.crop(crop); quad -= crop[0:2]                         :115-123   host: O(F) scalars (crop_plan)
    img.transform((size, size), QUAD, (quad + 0.5).flatten(), BILINEAR)            :142       hip.quad_crop
    Image.open(..).convert('RGB').resize((512, 512))             video_swap_dataset :139      hip.resample_u8, bicubic tables
    get_tensor()(img_p)                                                            :214       hip.dataset_tensors -> image
    1 - ToTensor(255 * isin(label, remove))                                  :157-163, :219   hip.dataset_tensors -> inpaint_mask
    image_tensor * mask_tensor                                                     :221       hip.dataset_tensors -> inpaint_image
    Resize([h, w])(inpaint_mask)                               VFace_inference_batch :459      hip.dataset_tensors -> mask_latent
    calc_alignment_coefficients(quad + 0.5, square)                 :68-71, alignmengt :266-276 host: inv_transforms (8 x 8 solve)

Landmark detection (dlib) and face parsing (BiSeNet) stay outside: their outputs -- landmarks or quads, and label maps -- are
the inputs here.  Host work is limited to O(F) scalars and the per-size tap tables; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from .resample import linear_taps_u8, resample_coeffs

REMOVE_MASK_TAR_FFHQ = (1, 2, 3, 5, 6, 7, 9)      # models/REFace/configs/project_ffhq.yaml: remove_mask_tar_FFHQ
PRESERVE_MASK_SRC_FFHQ = (1, 2, 3, 5, 6, 7, 9)    # project_ffhq.yaml:217-224: preserve_mask_src_FFHQ (the source's face region)


class SourceTensors(NamedTuple):
    """What ``FrameIntake.source`` makes of the source image(s) (VFace_inference_batch.py:254-355, :462, :468)."""
    crop: torch.Tensor                   # uint8 [n, S, S, 3]        the aligned crop (:254-258)
    labels: torch.Tensor                 # uint8 [n, H, W]           the parser's map (:263), or the one given
    clip_image: torch.Tensor             # fp32 [n, 3, c, c]         ref_image_tensor (:343-347)
    mask: torch.Tensor                   # fp32 [n, 1, H, W]         reference_mask_tensor (:341)
    masked: torch.Tensor                 # fp32 [n, 3, H, W]         ref_img_inv_ori (:350-352)
    inpaint_image: torch.Tensor          # fp32 [n, 3, H, W]         ref_img_inv_ori_inpaint (:354-355), zero as in the reference
    inpaint_mask_latent: torch.Tensor    # fp32 [n, 1, h, w]         inpaint_mask_src (:462, :468)


def quad_from_landmarks(lm) -> np.ndarray:
    """68 facial landmarks [68, 2] -> the oriented crop quad [4, 2] (NW, SW, SE, NE): ``compute_transform`` (alignmengt.py:152-178,
    scale = 1) and the stacking of ``crop_faces`` (:211), the same float64 operations in the same order."""
    lm = np.asarray(lm)
    if lm.shape != (68, 2):
        raise ValueError(f"quad_from_landmarks: landmarks must be [68, 2]; got {lm.shape}")
    lm_eye_left, lm_eye_right, lm_mouth_outer = lm[36:42], lm[42:48], lm[48:60]
    eye_left = np.mean(lm_eye_left, axis=0)
    eye_right = np.mean(lm_eye_right, axis=0)
    eye_avg = (eye_left + eye_right) * 0.5
    eye_to_eye = eye_right - eye_left
    mouth_avg = (lm_mouth_outer[0] + lm_mouth_outer[6]) * 0.5
    eye_to_mouth = mouth_avg - eye_avg
    x = eye_to_eye - np.flipud(eye_to_mouth) * [-1, 1]
    x /= np.hypot(*x)
    x *= max(np.hypot(*eye_to_eye) * 2.0, np.hypot(*eye_to_mouth) * 1.8)
    x *= 1.0
    y = np.flipud(x) * [-1, 1]
    c = eye_avg + eye_to_mouth * 0.1
    return np.stack([c - x - y, c - x + y, c + x + y, c + x - y])


def inv_transforms(quads, image_size: int) -> np.ndarray:
    """``inv_transforms_all`` (VFace_inference_batch.py:68-71): per quad the eight PIL PERSPECTIVE coefficients of
    ``calc_alignment_coefficients(quad + 0.5, [[0, 0], [0, S], [S, S], [S, 0]])`` (alignmengt.py:266-276), float64, through the
    same normal equations ``inv(A^T A) A^T b`` -- what ``PasteBack.paste`` takes.  Returns [F, 8]."""
    quads = np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2)
    S = image_size
    pb = [[0, 0], [0, S], [S, S], [S, 0]]
    out = np.empty((quads.shape[0], 8), np.float64)
    for f, quad in enumerate(quads):
        rows = []
        for p1, p2 in zip(quad + 0.5, pb):
            rows.append([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]])
            rows.append([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]])
        a = np.array(rows, dtype=float)
        b = np.array(pb).reshape(8)
        out[f] = np.dot(np.dot(np.linalg.inv(np.dot(a.T, a)), a.T), b)
    return out


def crop_plan(quad, width: int, height: int, output_size: int, enable_padding: bool = False):
    """The host scalars of ``crop_image`` (alignmengt.py:100-123, :142) for one ``width`` x ``height`` frame: returns
    ``(shrink, (rw, rh), window, coeffs)`` -- the integer shrink factor (<= 1: none), the frame's size after the shrink, the
    crop window (x0, y0, x1, y1) inside the (shrunk) frame and the eight coefficients Pillow's ``Image.__transformer`` derives
    for ``QUAD`` from ``quad - window origin + 0.5`` and the output size."""
    if enable_padding:
        raise NotImplementedError("crop_image(enable_padding=True) is not built: the reference never passes it")
    quad = np.array(quad, dtype=np.float64).reshape(4, 2)
    x = (quad[3] - quad[1]) / 2
    qsize = np.hypot(*x) * 2
    size = (int(width), int(height))
    shrink = int(np.floor(qsize / output_size * 0.5))                                           # :109
    if shrink > 1:
        size = (int(np.rint(float(size[0]) / shrink)), int(np.rint(float(size[1]) / shrink)))   # :111
        quad /= shrink
        qsize /= shrink
    border = max(int(np.rint(qsize * 0.1)), 3)                                                  # :116
    crop = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))),
            int(np.ceil(max(quad[:, 1]))))
    crop = (max(crop[0] - border, 0), max(crop[1] - border, 0), min(crop[2] + border, size[0]), min(crop[3] + border, size[1]))
    if crop[2] <= crop[0] or crop[3] <= crop[1]:
        raise ValueError(f"crop window {crop} is empty: the quad lies outside the {size[0]} x {size[1]} frame")
    # (:121 skips a crop that is the whole frame; then the window is the frame and its origin (0, 0))
    quad -= crop[0:2]                                                                           # :123
    data = (quad + 0.5).flatten()                                                               # :142
    nw, sw, se, ne = data[:2], data[2:4], data[4:6], data[6:8]
    x0, y0 = nw
    As = 1.0 / output_size
    At = 1.0 / output_size
    coeffs = (x0, (ne[0] - x0) * As, (sw[0] - x0) * At, (se[0] - sw[0] - ne[0] + x0) * As * At,
              y0, (ne[1] - y0) * As, (sw[1] - y0) * At, (se[1] - sw[1] - ne[1] + y0) * As * At)
    return shrink, size, crop, np.array(coeffs, dtype=np.float64)


class FrameIntake:
    """Batch intake on one device.  ``image_size``: side of the aligned crop (the reference's 1024); ``H, W``: the sampler's
    pixel size; ``latent``: (h, w) of the latent grid the mask is resized to."""

    def __init__(self, image_size: int = 1024, H: int = 512, W: int = 512, latent: Tuple[int, int] = (64, 64), device="cuda:0"):
        self.image_size, self.H, self.W, self.latent = image_size, H, W, (int(latent[0]), int(latent[1]))
        self.device = torch.device(device)
        self._tables: Dict[Tuple[int, int, str], Tuple[torch.Tensor, torch.Tensor]] = {}
        self._members: Dict[Tuple[int, ...], torch.Tensor] = {}
        self._linear: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}

    def _table(self, in_size: int, out_size: int, filter: str):
        key = (in_size, out_size, filter)
        if key not in self._tables:
            b, k = resample_coeffs(in_size, out_size, filter)
            self._tables[key] = (torch.from_numpy(b).to(self.device), torch.from_numpy(k).to(self.device))
        return self._tables[key]

    def _check(self, t: torch.Tensor, what: str):
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise hip.VFaceHipError(f"the intake runs on the GPU: {what} must be tensors on {self.device}")

    def resize_u8(self, frames: torch.Tensor, out_w: int, out_h: int, filter: str = "bicubic") -> torch.Tensor:
        """``Image.resize((out_w, out_h), filter)`` of uint8 [F, H, W, 3] frames: x pass, then y pass (each skipped when that size
        is unchanged, as Pillow does).  The default is Pillow's own default for RGB, bicubic."""
        _, h, w, _ = frames.shape
        if out_w != w:
            frames = hip.resample_u8(frames, out_w, 0, *self._table(w, out_w, filter))
        if out_h != h:
            frames = hip.resample_u8(frames, out_h, 1, *self._table(h, out_h, filter))
        return frames

    def crop(self, frames_u8: torch.Tensor, quads, enable_padding: bool = False) -> torch.Tensor:
        """``crop_faces_by_quads`` (alignmengt.py:255-263): uint8 frames [F, Hs, Ws, 3] (device) and one quad [4, 2] per frame ->
        the aligned crops uint8 [F, image_size, image_size, 3].  Frames whose face is so large that ``crop_image`` shrinks them
        first (:108-114) go through the Lanczos resize, grouped by resulting size; every group is one ``quad_crop`` launch."""
        self._check(frames_u8, "frames")
        quads = np.asarray(quads, dtype=np.float64)
        F_, Hs, Ws, _ = frames_u8.shape
        if quads.shape != (F_, 4, 2):
            raise ValueError(f"crop: one quad [4, 2] per frame; got {quads.shape} for {F_} frames")
        S = self.image_size
        plans = [crop_plan(quads[f], Ws, Hs, S, enable_padding) for f in range(F_)]
        groups: Dict[Tuple[int, int], List[int]] = {}
        for f, (shrink, size, _, _) in enumerate(plans):
            groups.setdefault(size if shrink > 1 else (Ws, Hs), []).append(f)
        out = None
        for (rw, rh), idx in groups.items():
            src = frames_u8 if len(idx) == F_ else frames_u8[torch.as_tensor(idx, device=self.device)]
            src = self.resize_u8(src.contiguous(), rw, rh, "lanczos")
            co = torch.from_numpy(np.stack([plans[f][3] for f in idx])).to(self.device)
            win = torch.tensor([plans[f][2] for f in idx], dtype=torch.int32)
            res = hip.quad_crop(src, co, win, S)
            if len(idx) == F_:
                return res
            if out is None:
                out = torch.empty(F_, S, S, 3, dtype=torch.uint8, device=self.device)
            out[torch.as_tensor(idx, device=self.device)] = res
        return out

    def tensors(self, crops_u8: torch.Tensor, labels_u8: torch.Tensor, remove_labels: Sequence[int]):
        """``VideoDataset.__getitem_gray__`` for a batch: crops uint8 [F, S, S, 3], label maps uint8 [F, H, W] (the parser's
        output at the sampler's size), ``remove_labels`` the ``remove_mask_tar_FFHQ`` list.  Returns fp32
        ``image [F, 3, H, W], inpaint_image [F, 3, H, W], inpaint_mask [F, 1, H, W], mask_latent [F, 1, h, w]``."""
        self._check(crops_u8, "crops")
        self._check(labels_u8, "label maps")
        key = tuple(sorted(int(v) for v in remove_labels))
        if key not in self._members:
            self._members[key] = hip.label_membership(key, self.device)
        img = self.resize_u8(crops_u8.contiguous(), self.W, self.H, "bicubic")                  # :139
        return hip.dataset_tensors(img, labels_u8.contiguous(), self._members[key], self.latent)

    def _member(self, labels: Sequence[int]) -> torch.Tensor:
        key = tuple(sorted(int(v) for v in labels))
        if key not in self._members:
            self._members[key] = hip.label_membership(key, self.device)
        return self._members[key]

    def source(self, frames_u8: torch.Tensor, quads, labels_u8: Optional[torch.Tensor] = None, parser=None,
               preserve_labels: Sequence[int] = PRESERVE_MASK_SRC_FFHQ, clip_size: int = 224,
               convert_to_seg12: bool = True) -> SourceTensors:
        """The source image's side of ``VFace_inference_batch.py`` (:254-355, :462, :468): uint8 frames [n, Hs, Ws, 3] (device),
        one quad [4, 2] each, and either the label maps uint8 [n, H, W] or a ``FaceParser`` that makes them from the aligned crop
        (:263) -> ``SourceTensors``.  ``crop`` (:254-258), the parser, ``resize((W, H), Image.BILINEAR)`` (:350; Pillow's
        bilinear, not the bicubic default the target frames get) and one ``hip.source_tensors`` launch.  The 224 x 224 resize of
        :343 (albumentations ``A.Resize``, ``cv2.INTER_LINEAR``) is OpenCV's 11-bit fixed-point form as DESIGN §9 states it;
        parity with ``cv2.resize`` is not pinned."""
        if labels_u8 is None and parser is None:
            raise ValueError("source: give the label maps (labels_u8) or the face parser that makes them (parser)")
        crop = self.crop(frames_u8, quads)
        if labels_u8 is None:
            labels_u8 = parser.labels(crop, convert_to_seg12=convert_to_seg12)
        self._check(labels_u8, "label maps")
        S, c = self.image_size, int(clip_size)
        if (S, c) not in self._linear:
            taps, weights = linear_taps_u8(S, c)
            self._linear[(S, c)] = (torch.from_numpy(taps).to(self.device), torch.from_numpy(weights).to(self.device))
        taps, weights = self._linear[(S, c)]
        img = self.resize_u8(crop, self.W, self.H, "bilinear")                                  # :350
        mask, masked, inpaint, mlat, clip_image = hip.source_tensors(crop, img, labels_u8.contiguous(), self._member(preserve_labels),
                                                                     (taps, weights, taps, weights), self.latent, c)
        return SourceTensors(crop, labels_u8, clip_image, mask, masked, inpaint, mlat)

    def __call__(self, frames_u8: torch.Tensor, quads, labels_u8: torch.Tensor, remove_labels: Sequence[int]):
        """Frames + quads + label maps -> ``image, inpaint_image, inpaint_mask, mask_latent, inv_transforms``; the last is the
        float64 [F, 8] array ``PasteBack.paste`` takes for the same frames."""
        image, inpaint, mask, mlat = self.tensors(self.crop(frames_u8, quads), labels_u8, remove_labels)
        return image, inpaint, mask, mlat, inv_transforms(quads, self.image_size)
