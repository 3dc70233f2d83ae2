"""Constructed index streams for the LZW half of the GIF writer, shared by tests/test_gif_cpu.py (the model, Pillow, the host
program) and tests/test_gif_gpu.py (vface_gif_lzw); the model's answer to each is computed once."""
import functools

import numpy as np

import gif_model as gm

NEXT_TARGETS = (511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4094, 4095)
BYTE_TARGETS = (254, 255, 256, 509, 510, 511)


@functools.lru_cache(maxsize=None)
def lzw_cases():
    """name -> (uint8 [F, npix], seg_pixels)"""
    rng = np.random.default_rng(23)
    out = {}
    out["one_value"] = (np.full((1, 3000), 7, np.uint8), 65535)                       # runs that grow: codes for 2, 3, 4, .. sevens
    out["two_values"] = ((np.arange(2500) % 2 * 200).astype(np.uint8)[None], 65535)
    out["all_values"] = (np.tile(np.arange(256, dtype=np.uint8), 3)[None], 65535)
    out["noise_fills_table"] = (rng.integers(0, 256, (1, 12000), dtype=np.uint8), 12001)
    out["noise_three_tables_in_segments"] = (rng.integers(0, 256, (1, 17000), dtype=np.uint8), 8000)
    for t in NEXT_TARGETS:
        s = gm.stream_with_next(t)
        # the FIRST segment ends on the table size t and is closed by a Clear; three more indices make the last segment
        out[f"next_{t}"] = (np.concatenate([s, np.array([5, 5, 9], np.uint8)])[None], len(s))
        out[f"next_{t}_last"] = (s[None].copy(), len(s) + 1)
    for b in BYTE_TARGETS:
        s, seg = gm.stream_with_bytes(b)
        out[f"bytes_{b}"] = (s[None].copy(), seg)
    three = np.stack([np.zeros(2000, np.uint8), (np.arange(2000) % 3).astype(np.uint8), rng.integers(0, 256, 2000, dtype=np.uint8)])
    out["three_frames"] = (three, 512)
    out["seg_1"] = (rng.integers(0, 256, (2, 300), dtype=np.uint8), 1)
    out["seg_above_npix"] = (rng.integers(0, 16, (2, 300), dtype=np.uint8), 301)
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    """-> [per frame: {"image": image data bytes, "lzw": gif_model.lzw's dict}]"""
    frames, seg = lzw_cases()[name]
    out = []
    for idx in frames:
        d = gm.lzw(idx, seg)
        out.append({"image": gm.sub_blocks(d["data"]), "lzw": d})
    return out


def palette_frame(values):
    """A frame [1, n, 3] of the given RGB triples."""
    return np.array(values, np.uint8).reshape(1, -1, 3)
