"""Configurations and inputs of the conditioning fixture (tests/golden/clip.npz), by seed: the image tower's sizes, the frames the
target branch of ``conditioning_with_feat`` resizes, and the seeded side inputs of the mix.  Weights are the name-keyed fill
``vface_amd.utils.synth.fill_module_(module, seed=WEIGHT_SEED)`` on both sides, so only results are stored."""
import numpy as np

WEIGHT_SEED = 5
BATCH = 2
PROJ = 768                     # visual_projection's width = mapper2's width (fixed by FrozenCLIPEmbedder itself)
MAPPER_LAYERS = 5
# name -> the vision tower's size (patch 14, hidden_act quick_gelu) and the frames' (H, W) before the resize to `image`
CONFIGS = {
    "tiny": dict(hidden=128, heads=2, layers=2, mlp=512, image=42, frame=(64, 48), seed=3),
    "wide": dict(hidden=1024, heads=16, layers=4, mlp=4096, image=224, frame=(512, 512), seed=1),
    "full": dict(hidden=1024, heads=16, layers=24, mlp=4096, image=224, frame=(512, 512), seed=1),
}
# what the text tower is built with: never run, only present in the state dict (its keys are accepted and dropped)
TEXT = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, vocab_size=64, max_position_embeddings=8,
            bos_token_id=1, eos_token_id=2)
INTERMEDIATES = ("embeddings", "layer0", "pooler_output", "visual_projection", "mapper2_block0")


def vision_config(name: str) -> dict:
    c = CONFIGS[name]
    return dict(hidden_size=c["hidden"], num_attention_heads=c["heads"], num_hidden_layers=c["layers"], intermediate_size=c["mlp"],
                image_size=c["image"], patch_size=14, hidden_act="quick_gelu", layer_norm_eps=1e-5)


def frames(name: str) -> np.ndarray:
    """float32 [BATCH, 3, H, W] in [-1, 1]: a few low-frequency waves per channel, a soft blob, and noise (cases_parse.crop's
    recipe on a float image)."""
    c = CONFIGS[name]
    H, W = c["frame"]
    g = np.random.Generator(np.random.PCG64([c["seed"], H, W]))
    y, x = np.meshgrid(np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W), indexing="ij")
    out = np.zeros((BATCH, 3, H, W))
    for b in range(BATCH):
        for ch in range(3):
            for _ in range(4):
                fy, fx = g.uniform(0.5, 6.0, 2)
                out[b, ch] += g.uniform(0.2, 0.6) * np.sin(2 * np.pi * (fy * y + fx * x) + g.uniform(0, 2 * np.pi))
            cy, cx, r = g.uniform(0.3, 0.7), g.uniform(0.3, 0.7), g.uniform(0.1, 0.3)
            out[b, ch] += g.uniform(-0.8, 0.8) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    out += g.uniform(-0.2, 0.2, out.shape)
    return np.clip(out, -1.0, 1.0).astype(np.float32)


def side_inputs(batch: int = BATCH):
    """``(id_feat [batch, 512], landmarks [batch, 136])`` float32: the ArcFace features and dlib landmarks the mix takes as inputs."""
    g = np.random.Generator(np.random.PCG64([7, batch]))
    return g.standard_normal((batch, 512)).astype(np.float32), g.uniform(0.0, 1.0, (batch, 136)).astype(np.float32)
