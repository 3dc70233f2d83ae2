"""Inputs of the face-parsing fixture (tests/golden/parse.npz), by seed: smooth colour fields plus noise.  (Uniform noise alone
is a constant to a network that pools down by 32: its logits hardly vary.)"""
import numpy as np

# network input sizes (H, W); the crops the pre-filter reads are twice as large
NET_SIZES = ((64, 64), (96, 64), (512, 512))
# the recorded frame of each size.  Chosen on the reference alone: the share of pixels whose double-precision margin (top logit -
# runner-up) lies under 32 E_ref, the bf16 label rule's exclusion, must stay under that rule's 5 % cap (seed 0 gives 6.5 % at
# 64 x 64; these give 3.1 %, 4.2 % and 2.8 %)
SEEDS = {(64, 64): 3, (96, 64): 0, (512, 512): 0}
N_CLASSES = 19
WEIGHT_SEED = 11


def crop(net_h: int, net_w: int, seed: int = 0) -> np.ndarray:
    """uint8 [2 net_h, 2 net_w, 3]: a few low-frequency waves per channel, a soft blob, and +-24 levels of noise."""
    H, W = 2 * net_h, 2 * net_w
    g = np.random.Generator(np.random.PCG64([seed, H, W]))
    y, x = np.meshgrid(np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W), indexing="ij")
    img = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(4):
            fy, fx = g.uniform(0.5, 6.0, 2)
            img[..., c] += g.uniform(0.1, 0.3) * np.sin(2 * np.pi * (fy * y + fx * x) + g.uniform(0, 2 * np.pi))
        cy, cx, r = g.uniform(0.3, 0.7), g.uniform(0.3, 0.7), g.uniform(0.1, 0.3)
        img[..., c] += g.uniform(-0.4, 0.4) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    img = 0.5 + img + g.uniform(-24.0, 24.0, (H, W, 3)) / 255.0
    return np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)
