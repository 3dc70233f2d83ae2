"""The quad cases of the frame intake, shared by the fixture generator (make_intake_golden.py) and the tests: a 90 x 120 frame
(height x width), quads given as centre ``c`` and half-axis ``x`` with ``y = flipud(x) * [-1, 1]`` (alignmengt.py:176), stacked
NW, SW, SE, NE (:211)."""
import numpy as np

FRAME_H, FRAME_W, FRAME_SEED = 90, 120, 20260
# name, c, x, output size, partly outside the frame
CASES = [("inside", (60.3, 40.2), (14.1, 3.2), 32, False),
         ("rot45", (60.0, 45.0), (12.0, 12.0), 32, False),
         ("partly_out", (100.0, 20.0), (20.0, -9.0), 32, True),
         ("corner", (5.0, 85.0), (9.0, 2.0), 24, True),
         ("shrink6", (60.0, 45.0), (70.0, 10.0), 16, True),
         ("shrink2", (60.0, 45.0), (33.0, -4.0), 16, False)]


def frame() -> np.ndarray:
    return np.random.default_rng(FRAME_SEED).integers(0, 256, (FRAME_H, FRAME_W, 3), dtype=np.uint8)


def quad(c, x) -> np.ndarray:
    c, x = np.array(c, np.float64), np.array(x, np.float64)
    y = np.flipud(x) * [-1, 1]
    return np.stack([c - x - y, c - x + y, c + x + y, c + x - y])


def landmarks(seed: int, integer: bool) -> np.ndarray:
    """A fixed 68-point set: a rough face (eyes above mouth, tilted) plus seeded jitter; dlib hands back integers, face_alignment
    floats."""
    rng = np.random.default_rng(seed)
    lm = rng.uniform(100, 400, (68, 2))
    tilt = np.array([[np.cos(0.2 * seed), -np.sin(0.2 * seed)], [np.sin(0.2 * seed), np.cos(0.2 * seed)]])
    base = np.array([250.0, 240.0])
    lm[36:42] = base + (np.array([-45.0, -30.0]) + rng.uniform(-6, 6, (6, 2))) @ tilt.T
    lm[42:48] = base + (np.array([45.0, -30.0]) + rng.uniform(-6, 6, (6, 2))) @ tilt.T
    lm[48:60] = base + (np.array([0.0, 55.0]) + rng.uniform(-25, 25, (12, 2)) * [1.0, 0.2]) @ tilt.T
    return np.rint(lm).astype(np.int64) if integer else lm


LANDMARK_SETS = [(1, True), (2, False), (5, False)]
