"""Tap tables of Pillow's 8-bit separable resampling (Resample.c), shared by the paste-back and the frame intake: host work, a
few KB per (in, out) size pair, consumed by ``hip.resample_u8``."""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2      # Pillow Resample.c: 8-bit samples, 2 guard bits -> 22 fractional bits


def _bilinear(a: np.ndarray) -> np.ndarray:
    a = np.abs(a)
    return np.where(a < 1.0, 1.0 - a, 0.0)


def _bicubic(x: np.ndarray) -> np.ndarray:
    """Resample.c bicubic_filter, a = -0.5 (Keys), each product rounded in the C expression's order."""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _lanczos(x: np.ndarray) -> np.ndarray:
    """Resample.c lanczos_filter: sinc(x) * sinc(x / 3) on [-3, 3).  ``math.sin`` is the C library's ``sin`` that Pillow calls;
    numpy's vectorised one may differ from it in the last bit."""
    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    out = np.zeros(x.shape, np.float64)
    for i, v in enumerate(x.tolist()):
        if -3.0 <= v < 3.0:
            out[i] = sinc(v) * sinc(v / 3)
    return out


FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def resample_coeffs(in_size: int, out_size: int, filter: str = "bilinear") -> Tuple[np.ndarray, np.ndarray]:
    """Tap tables of ``Image.resize(.., filter)`` on 8-bit images from ``in_size`` to ``out_size`` samples: ``bounds`` int32
    [out_size, 2] = (first input sample, taps) and ``kk`` int32 [out_size, ksize] = 22-bit fixed-point weights, as Pillow's
    ``precompute_coeffs`` (support = filter support * max(scale, 1), window centred on (o + 0.5) * scale, weights normalised to
    sum 1 in double) and ``normalize_coeffs_8bpc`` (round half away from zero) produce them.

    ``filter``: ``"bilinear"`` (triangle, support 1: ``Image.BILINEAR``, the paste-back's resizes), ``"bicubic"`` (a = -0.5,
    support 2: ``Image.BICUBIC``, which is the DEFAULT of ``Image.resize(size)`` for an RGB image and so what
    ``video_swap_dataset.py:139`` runs) or ``"lanczos"`` (support 3: ``Image.LANCZOS``; ``alignmengt.py:112`` names it
    ``PIL.Image.ANTIALIAS``, an alias that Pillow 10 removed).  The last two have negative lobes: sums can leave 0..255 and the
    kernel's clip matters."""
    if in_size <= 0 or out_size <= 0:
        raise ValueError("resample_coeffs: sizes must be positive")
    if filter not in FILTERS:
        raise ValueError(f"resample_coeffs: filter must be one of {sorted(FILTERS)}; got {filter!r}")
    fn, filter_support = FILTERS[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filter_support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, ksize), np.float64)
    total = np.zeros(out_size, np.float64)
    for x in range(ksize):           # sequential accumulation, tap by tap, as the C loop sums it
        col = np.where(x < xmax, fn((x + xmin - center + 0.5) * inv), 0.0)
        w[:, x] = col
        total = total + col
    nz = total != 0.0
    w[nz] = w[nz] / total[nz, None]
    w[np.arange(ksize)[None, :] >= xmax[:, None]] = 0.0
    fixed = w * float(1 << PRECISION_BITS)
    kk = np.where(w < 0, np.trunc(-0.5 + fixed), np.trunc(0.5 + fixed)).astype(np.int32)
    return np.stack([xmin, xmax], 1).astype(np.int32), kk


LINEAR_COEF_BITS = 11            # OpenCV resize: INTER_RESIZE_COEF_BITS, weights are 11-bit fixed point


def linear_taps_u8(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Tap tables of the 8-bit 2-tap linear resize ``hip.source_tensors`` runs for ``A.Resize`` (albumentations' default,
    ``cv2.INTER_LINEAR``) from ``in_size`` to ``out_size`` samples: ``taps`` int32 [out_size, 2] = the two source samples and
    ``weights`` int16 [out_size, 2] = their 11-bit fixed-point weights.  Half-pixel centres, no antialias: for output ``d``,
    ``f = (d + 0.5) * in / out - 0.5`` in double, ``s = floor(f)``, ``t = f - s``; below the first sample and from the last one
    on, the tap is that sample with weight 2048; ``w1 = rint(2048 t)``, ``w0 = rint(2048 (1 - t))``, round half to even.  This is
    OpenCV's long-standing fixed-point form as DESIGN §9 states it; parity with ``cv2.resize`` is not pinned (OpenCV is not
    available to the tests)."""
    if in_size <= 0 or out_size <= 0:
        raise ValueError("linear_taps_u8: sizes must be positive")
    f = (np.arange(out_size, dtype=np.float64) + 0.5) * float(in_size) / float(out_size) - 0.5
    s = np.floor(f)
    t = f - s
    low, high = s < 0, s >= in_size - 1
    s = np.where(low, 0, np.where(high, in_size - 1, s)).astype(np.int64)
    t = np.where(low | high, 0.0, t)
    one = float(1 << LINEAR_COEF_BITS)
    taps = np.stack([s, np.minimum(s + 1, in_size - 1)], 1).astype(np.int32)
    weights = np.stack([np.rint(one * (1.0 - t)), np.rint(one * t)], 1).astype(np.int16)
    return taps, weights
