"""Configurations and inputs of the identity fixture (tests/golden/arcface.npz), by seed.  Weights are the name-keyed fill
``vface_amd.utils.synth.fill_arcface_(module, seed=WEIGHT_SEED)`` on both sides, so only results are stored.  The network's input
is ``cases_clip.frames("wide")`` -- two 512 x 512 frames in [-1, 1] -- through the chain of ``extract_feats``."""
import numpy as np

WEIGHT_SEED = 11
BATCH = 2
FRAMES = "wide"                # cases_clip.frames(FRAMES)
# name -> (in_channel, depth, stride, H, W, images, seed) of one bottleneck_IR_SE on a small odd map
UNIT_CASES = {
    "id_s1": (64, 64, 1, 7, 5, 2, 1),            # MaxPool2d(1, 1): the input itself
    "id_s2": (64, 64, 2, 14, 10, 2, 2),          # MaxPool2d(1, 2): 14 x 10 -> 7 x 5
    "conv_s2": (64, 128, 2, 14, 10, 2, 3),       # 1x1 stride-2 convolution shortcut
    "id_s2_odd": (64, 64, 2, 7, 5, 3, 4),        # 7 x 5 -> 4 x 3: OH = (H - 1) / s + 1 at odd sizes
}


def unit_input(name: str) -> np.ndarray:
    """float32 [images, in_channel, H, W], standard normal: what a unit sees inside the network (std 0.45 .. 1.8)."""
    cin, _, _, H, W, n, seed = UNIT_CASES[name]
    g = np.random.Generator(np.random.PCG64([seed, H, W]))
    return g.standard_normal((n, cin, H, W)).astype(np.float32)


def unit_prefix(name: str) -> str:
    """The fill's key prefix: every case has weights of its own."""
    return f"unit.{name}."
