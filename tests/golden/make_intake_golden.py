#!/usr/bin/env python3
"""Writes tests/golden/intake.npz: the REFERENCE's own outputs for the frame intake's host chain, recorded by running its
``src/utils/alignmengt.py`` -- ``crop_image`` on the quad cases of cases_intake.py, ``calc_alignment_coefficients`` on the same
quads and ``compute_transform`` on fixed landmark sets.  Only arrays are written.

Runs where a checkout of the reference is at hand (it is not needed to run the tests):

    python tests/golden/make_intake_golden.py /path/to/REFace

The reference imports dlib, cv2, skimage.io and face_alignment at module level without using them on these paths; empty
stand-in modules take their place when they are not installed.  ``Image.ANTIALIAS`` (alignmengt.py:112), removed in Pillow 10,
is the Lanczos filter.
"""
import os
import sys
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases_intake as ci  # noqa: E402


def load_reference(root: str):
    for name in ("dlib", "cv2", "skimage", "skimage.io", "face_alignment"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            if "." in name:
                parent, child = name.rsplit(".", 1)
                setattr(sys.modules[parent], child, sys.modules[name])
    if not hasattr(Image, "ANTIALIAS"):
        Image.ANTIALIAS = Image.LANCZOS
    sys.path.insert(0, root)
    from src.utils import alignmengt
    return alignmengt


def main():
    ref = load_reference(sys.argv[1])
    out = {"frame": ci.frame(), "pillow_version": np.array(Image.__version__)}
    for name, c, x, size, _ in ci.CASES:
        q = ci.quad(c, x)
        out[f"{name}.quad"] = q
        out[f"{name}.crop"] = np.asarray(ref.crop_image(Image.fromarray(out["frame"]), size, q.copy()))      # :259
        square = [[0, 0], [0, size], [size, size], [size, 0]]
        out[f"{name}.inv"] = ref.calc_alignment_coefficients(q + 0.5, square)                                # :68-71
    for seed, integer in ci.LANDMARK_SETS:
        lm = ci.landmarks(seed, integer)
        ref.get_landmark = lambda *a, _lm=lm, **k: _lm
        c, x, y = ref.compute_transform(None, None)
        out[f"lm{seed}.lm"], out[f"lm{seed}.c"], out[f"lm{seed}.x"], out[f"lm{seed}.y"] = lm, c, x, y
    path = os.path.join(HERE, "intake.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
