"""What a run's stages are fed, batch by batch: two providers with one interface (``scripts/pipeline.py`` asks, never looks at
which of the two it was handed).

``SeededInputs`` is the ``--synthetic`` run: seeded stand-ins for everything a stage that is switched off would have made, and for
what video decoding, dlib and the source photo hand to the stages that are on.  ``ClipRunInputs`` is a clip from disk
(``clip_io.ClipInputs``): frames, quads, landmarks and source from files; every stage is on, so it has no stand-ins.

The questions, for batch ``k`` of ``F = --n_samples`` frames (tensors on the provider's device unless stated):

    frame_ids(k)            the clip's frame indices, or None (the record and the PNG names)
    tokens(k)               c, uc, tc [F, 1, 768]; None = made by the conditioning stage (uc: the model's learnable_vector)
    intake_frames(k)        frames to paste into, frames to crop from, quads [F, 4, 2] (host), label maps or None = ask the parser
    inherits(k)             per frame: does it take the label map of the frame before (no landmarks, :297-303)?
    carry_labels(k, maps)   the label maps with the inherited ones put in; remembers batch k's last map for batch k + 1
    own_seconds(k)          stage name -> wall seconds of device work the provider did itself for batch k (``video_in``: the upload
                            and colour conversion of a clip read from a video file; ``png_in``: reading and parsing a folder's PNG
                            files on the host, their upload and decoding, under ``--png_decoder gpu``); asked once, after ``intake_frames``
    landmarks(k)            conditioning landmarks [F, 136]
    source()                source frame [1, Hs, Ws, 3], quad (host), label map or None, landmarks [1, 136], identity features or None
    learnable_vector()      a seeded value for the model's learnable_vector on seeded weights, or None = leave the module's own

and, where a stage is off (seeded only): ``images`` ``latents`` ``latent_mask`` ``keep_mask`` ``id_feats`` ``flow``
``boundary_flow`` ``inversion_cache`` ``inversion_latents`` ``paste_target`` ``source_clip_image``.

Which frames batch ``k`` holds is ``batch_plan(opt)[k]``, ``(first, count)``: ``--n_samples`` frames each and the tail dropped, or under
``--whole_clip`` every frame (``parallel.clip_batches``: a last batch may be shorter).  Under ``--whole_clip`` the seeded stand-ins
are drawn per CLIP and cut by frame, so that what a frame is fed does not depend on the batch that holds it.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from ..parallel import clip_batches
from ..utils import synth


def batch_plan(opt):
    """``[(first, count), ...]`` of a run: the reference's ``DataLoader(batch_size=n_samples, drop_last=True)`` (:376-382), or
    under ``--whole_clip`` every frame of the clip (``parallel.clip_batches``).  The loop, the providers and ``clip_io`` read it
    from here."""
    if getattr(opt, "whole_clip", False):
        return clip_batches(opt.n_frames, opt.n_samples)
    return [(k * opt.n_samples, opt.n_samples) for k in range(opt.n_frames // opt.n_samples)]


def _quad_coeffs(size, quad):
    """Eight PIL perspective coefficients (output pixel -> crop coordinates) that land the ``size`` x ``size`` crop on ``quad``
    (four frame-space corners, clockwise from top-left) -- what ``crop_and_align_face`` (:58-73) stores per frame."""
    src = [(0, 0), (size, 0), (size, size), (0, size)]
    A, B = [], []
    for (x, y), (u, v) in zip(quad, src):
        A += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        B += [u, v]
    return np.linalg.solve(np.array(A, float), np.array(B, float))


def synthetic_intake_inputs(F_: int, S_: int, H: int, W: int, seed: int):
    """Stand-ins for what video decoding, landmark detection and face parsing hand to the intake: seeded uint8 frames
    [F, S, S, 3], one quad [4, 2] per frame (NW, SW, SE, NE; half the frame wide, rotating and drifting from frame to frame, the
    first one partly outside the frame) and a label map [F, H, W] with the parser's values 0..18 in rings round the centre."""
    gen = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (F_, S_, S_, 3), dtype=torch.uint8, generator=gen)
    quads = np.empty((F_, 4, 2), np.float64)
    for f in range(F_):
        c = np.array([S_ * (0.15 if f == 0 else 0.5) + 3.0 * f, S_ * 0.5 + 2.0 * f])
        th = 0.05 * (f + 1)
        x = S_ / 4.0 * np.array([np.cos(th), np.sin(th)])
        y = np.flipud(x) * [-1, 1]
        quads[f] = np.stack([c - x - y, c - x + y, c + x + y, c + x - y])
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    r = torch.hypot((ys - (H - 1) / 2) / (0.5 * H), (xs - (W - 1) / 2) / (0.5 * W))
    labels = torch.stack([((r * 12).long() + f) % 19 for f in range(F_)]).to(torch.uint8)
    return frames, quads, labels


class SeededInputs:
    """The stand-ins of ``--synthetic``.  Every draw is a function of its tag (``cli.{name}.{k}``) or seed alone, so the order in
    which a run asks is free.  A stand-in is drawn over a SCOPE and the batch takes its rows of it (``_scope``): the batch's own
    ``--n_samples`` frames, tagged and seeded by the batch -- or, under ``--whole_clip``, the clip's ``--n_frames``, tagged ``clip``,
    drawn once per provider and cut by frame."""
    frame_size_order = "reference"      # (PasteBack: :623 as written; the seeded frames are square)
    record_keys = ()                    # a batch's record carries no key beyond the common ones

    def __init__(self, opt, device):
        self.opt, self.device, self.F = opt, torch.device(device), opt.n_samples
        self.h, self.w = opt.H // opt.f, opt.W // opt.f
        self.whole = bool(getattr(opt, "whole_clip", False))
        self.plan = batch_plan(opt)
        self._clip = {}                 # --whole_clip: what was drawn over the clip, by name

    def _scope(self, k):
        """``(tag, seed offset, frames, rows)`` of batch k's stand-ins: what they are drawn over, and the batch's rows of it."""
        if self.whole:
            first, count = self.plan[k]
            return "clip", 0, self.opt.n_frames, slice(first, first + count)
        return k, k, self.F, slice(0, self.F)

    def _drawn(self, k, name, make):
        """``make(tag, seed offset, frames)`` over batch k's scope; a clip-long draw is made once."""
        tag, offset, n, _ = self._scope(k)
        if not self.whole:
            return make(tag, offset, n)
        if name not in self._clip:
            self._clip[name] = make(tag, offset, n)
        return self._clip[name]

    def count(self, k):
        rows = self._scope(k)[3]
        return rows.stop - rows.start

    def _host(self, k, name, shape, groups=1):
        """Batch k's rows of N(0, 1) ``[groups * frames, *shape]`` tagged ``cli.{name}.{scope}`` (``groups`` blocks of frames each)."""
        rows = self._scope(k)[3]
        full = self._drawn(k, name, lambda tag, _, n: synth.synth_normal(f"cli.{name}.{tag}", (groups * n,) + tuple(shape)))
        return full.reshape((groups, -1) + tuple(shape))[:, rows].reshape((-1,) + tuple(shape))

    def _normal(self, k, name, shape, groups=1):
        return self._host(k, name, shape, groups).to(self.device)

    def frame_ids(self, k):
        return None

    def tokens(self, k):
        return tuple(self._normal(k, name, (1, 768)) for name in ("c", "uc", "tc"))

    def intake_frames(self, k):
        o, rows = self.opt, self._scope(k)[3]
        frames, quads, labels = (v[rows] for v in self._drawn(k, "intake", lambda _, offset, n: synthetic_intake_inputs(
            n, o.frame_size, o.H, o.W, o.seed + 1000 + offset)))
        frames = frames.to(self.device)
        return frames, frames, quads, labels.to(self.device)

    def inherits(self, k):
        return [False] * self.count(k)

    def carry_labels(self, k, labels):
        return labels

    def own_seconds(self, k):
        return {}

    def landmarks(self, k):
        return (self._host(k, "landmarks", (136,)) * 0.1 + 0.5).to(self.device)

    def source(self):
        o = self.opt
        frames, quads, labels = synthetic_intake_inputs(1, o.frame_size, o.H, o.W, o.seed + 500)
        lmk = synth.synth_normal("cli.landmarks_src", (1, 136)).to(self.device) * 0.1 + 0.5
        idf = None if o.arcface else synth.synth_normal("cli.id_feat_src", (1, 512)).to(self.device)
        return frames.to(self.device), quads, labels.to(self.device), lmk, idf

    def learnable_vector(self):
        return None     # (a seeded run draws its `uc` per batch)

    # ---- stand-ins for the products of stages that are off
    def images(self, k):
        o, (tag, _, n, rows) = self.opt, self._scope(k)
        return torch.stack([synth.synth_normal(f"cli.img{f}.{tag}", (3, o.H, o.W)).clamp(-1, 1) for f in range(n)[rows]]).to(self.device)

    def latents(self, k):
        return (self._host(k, "inp", (self.opt.C, self.h, self.w)) * 0.18215).to(self.device)

    def latent_mask(self, k):
        return synth.synth_mask(self.count(k), self.h, self.w).to(self.device)

    def keep_mask(self, k):
        return synth.synth_mask(self.count(k), self.opt.H, self.opt.W).to(self.device)

    def id_feats(self, k):
        return tuple(self._normal(k, name, (512,)) for name in ("id_feat", "id_feat_tar"))

    def _fields(self, k):
        """The scope's frames - 1 host fields; with ``--flow_pixels`` at pixel resolution, their latent resample a +-2-cell motion."""
        o = self.opt
        if o.flow_pixels:
            return self._drawn(k, "flow", lambda _, offset, n: [f[None] * o.f for f in synth.synth_flow(n - 1, o.H, o.W, seed=o.seed + offset)])
        return self._drawn(k, "flow", lambda _, offset, n: [f[None] for f in synth.synth_flow(n - 1, self.h, self.w, seed=o.seed + offset)])

    def flow(self, k):
        """The fields between the batch's own frames."""
        rows = self._scope(k)[3]
        return self._fields(k)[rows.start:rows.stop - 1]

    def boundary_flow(self, k):
        """``--whole_clip``: the field from the last frame of batch k - 1 into the first frame of batch k; None for batch 0."""
        first = self._scope(k)[3].start
        return self._fields(k)[first - 1] if first else None

    def inversion_cache(self, k, timesteps):
        return {int(s): self._normal(k, f"inv{int(s)}", (self.opt.C, self.h, self.w)) for s in timesteps}

    def inversion_latents(self, k):
        return self._normal(k, "z2", (self.opt.C, self.h, self.w), groups=2)       # [target ; source]

    def paste_target(self, k, canvas):
        """Original frames and ``inv_transforms_all`` rows (:625) where no intake made them: the ``canvas`` lands on the central
        half of the frame, slightly sheared."""
        S_, (_, _, n, rows) = self.opt.frame_size, self._scope(k)
        frames = self._drawn(k, "paste", lambda _, offset, n: torch.randint(
            0, 256, (n, S_, S_, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(self.opt.seed + 1000 + offset)))
        q = S_ / 4.0
        return frames[rows].to(self.device), [_quad_coeffs(canvas, [(q + 3 * f, q), (3 * q, q + f), (3 * q - f, 3 * q), (q, 3 * q - 2 * f)])
                                              for f in range(n)[rows]]

    def source_clip_image(self):
        return synth.synth_normal("cli.source224", (1, 3, 224, 224)).to(self.device)


class ClipRunInputs:
    """A ``clip_io.ClipInputs`` behind the same questions.  A frame without landmarks is cut with the quad, and from the pixels, of
    the frame it takes (``clip_io.fallback_indices``), inherits that frame's label map -- across a batch boundary too, which is
    the one thing this object carries from batch to batch -- and has zero conditioning landmarks.  Over a video file
    (``ClipInputs.from_video``) the clip hands out what the file's reader read -- I420 rows of a Y4M file, the compressed scans of
    an AVI's JPEG frames -- and the reader's ``to_rgb`` makes the RGB frames on the device (``hip.yuv420_to_rgb``; matrix and chroma
    siting from ``--video_in_matrix``, ``--chroma_upsample`` and the file's header; for an AVI the decoder of ``scripts/mjpeg_in.py``
    in front of it), timed as stage ``video_in``.  Over a folder read with ``--png_decoder gpu`` (``ClipInputs.from_png_folder``) it
    hands out parsed PNG files and ``scripts/png_in.py`` decodes them on the device; reading and parsing on the host and the decode are
    timed together as stage ``png_in``."""
    frame_size_order = "width_height"   # (a clip is rarely square: paste_back.PasteBack)
    record_keys = ("frame_ids", "pasted_frames", "crops", "conditioning")

    def __init__(self, clip, opt, device):
        self.clip, self.device, self.F = clip, torch.device(device), opt.n_samples
        self.whole = bool(getattr(opt, "whole_clip", False))
        self.plan = batch_plan(opt)
        self._last_labels = {}      # batch id -> its last frame's label map, for the first frame of the batch after it
        self.matrix, self.chroma_upsample = opt.video_in_matrix or "bt709", opt.chroma_upsample or "sited"
        self.entropy = getattr(opt, "video_in_entropy", None) or "auto"     # (an AVI's Huffman decoder: scripts/mjpeg_in.entropy_path)
        self._seconds = {}          # batch id -> wall seconds of what this provider did on the device for it (`own_seconds`)

    def _rows(self, k):
        first, count = self.plan[k] if self.whole else (k * self.F, self.F)
        return slice(first, first + count)

    def frame_ids(self, k):
        return list(self.clip.frame_ids[self._rows(k)])

    def tokens(self, k):
        return None, None, None     # :423 uc = learnable_vector; c and tc come from the conditioning stage

    def intake_frames(self, k):
        t_read = time.time()
        given = self.clip.batch(k, self.F, whole_clip=self.whole)
        t_read = time.time() - t_read
        if self.clip.video is None:
            return given["frames"].to(self.device), given["crop_frames"].to(self.device), given["quads"], None
        # a video file: what its reader hands out crosses to the device (I420 rows, or JPEG scans) and becomes RGB frames there
        torch.cuda.synchronize(self.device)
        t0 = time.time()
        frames = self._rgb(given["frames"])
        crop_frames = frames if given["crop_frames"] is given["frames"] else self._rgb(given["crop_frames"])
        torch.cuda.synchronize(self.device)
        stage = getattr(self.clip.video, "stage", "video_in")
        # png_in also holds the host's half, which ran inside clip.batch: reading the files, every chunk's CRC, joining the IDATs
        self._seconds[k] = {stage: time.time() - t0 + (t_read if stage == "png_in" else 0.0)}
        return frames, crop_frames, given["quads"], None

    def _rgb(self, read):
        """What the clip's reader handed out (I420 rows of a Y4M file, the scans of an AVI's JPEG frames, the parsed files of a
        folder of PNGs under ``--png_decoder gpu``: stage ``png_in``) -> device RGB frames."""
        if getattr(self.clip.video, "stage", None) == "png_in":     # scripts/png_in.PNGFolderReader: no matrix, no chroma
            return self.clip.video.to_rgb(read, self.device)
        if self.clip.video.fixed_matrix:            # Motion-JPEG: --video_in_entropy is its reader's alone
            return self.clip.video.to_rgb(read, self.device, self.matrix, self.chroma_upsample, entropy=self.entropy)
        return self.clip.video.to_rgb(read, self.device, self.matrix, self.chroma_upsample)

    def own_seconds(self, k):
        return self._seconds.pop(k, {})

    def inherits(self, k):
        return [not bool(found) for found in self.clip.found[self._rows(k)]]

    def carry_labels(self, k, labels):
        for f, inherited in enumerate(self.inherits(k)):
            if inherited:
                labels[f] = labels[f - 1] if f else self._last_labels[k - 1]
        self._last_labels = {k: labels[-1].clone()}
        return labels

    def landmarks(self, k):     # ddpm.py:1068-1099: the points on the crop, in pixels; zeros where no face was found
        return torch.from_numpy(self.clip.landmarks[self._rows(k)]).to(self.device)

    def source(self):           # the photo, its quad from dlib's points, its landmarks on the crop; the label map is the parser's
        c = self.clip
        return c.source_u8.to(self.device), c.source_quad, None, torch.from_numpy(c.source_landmarks).to(self.device), None

    def learnable_vector(self):
        return synth.synth_normal("cli.learnable_vector", (1, 1, 768))

    def _no_stand_in(self, *a):
        raise RuntimeError("a clip from disk runs every stage (CLIP_STAGES): there is no stand-in for a stage's product")

    images = latents = latent_mask = keep_mask = id_feats = flow = boundary_flow = _no_stand_in
    inversion_cache = inversion_latents = paste_target = source_clip_image = _no_stand_in
