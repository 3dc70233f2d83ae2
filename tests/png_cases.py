"""Constructed row buffers for the deflate half of the PNG encoder: tests/test_png_cpu.py puts them through the model and zlib,
tests/test_png_gpu.py through vface_png_deflate.  name -> (uint8 [F, H, row_bytes], stripe_rows)."""
import functools

import numpy as np

import png_model as pm

RUN_LENGTHS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517)
LANE_WIDTHS = (63, 64, 65, 255, 256, 257)


def runs_buffer(lengths, values=None):
    """Runs of the given lengths, neighbours with different byte values."""
    out = []
    for i, n in enumerate(lengths):
        v = (values[i] if values is not None else 1 + i % 7)
        out.append(np.full(n, v, np.uint8))
    return np.concatenate(out)


def fibonacci_bytes(k=18):
    """Byte v (1..k) occurs fib(v + 1) times (1, 2, 3, 5, ...) and never twice in a row: with the end of block's count of 1 the
    counts ARE the Fibonacci numbers 1, 1, 2, 3, 5, ..., so an unlimited Huffman code would be k bits deep.  k = 18: 10943 bytes."""
    fib = [1, 1]
    while len(fib) < k + 1:
        fib.append(fib[-1] + fib[-2])
    ordered = np.concatenate([np.full(fib[v + 1], v + 1, np.uint8) for v in range(k - 1, -1, -1)])
    n = len(ordered)
    out = np.zeros(n, np.uint8)
    out[0::2] = ordered[:(n + 1) // 2]
    out[1::2] = ordered[(n + 1) // 2:]
    assert (out[1:] != out[:-1]).all()
    return out


def every_symbol():
    """All 256 literals and all 29 length codes: a run of base + 1 bytes per length code, then every byte value once."""
    lengths = [b + 1 for b in pm.LEN_BASE]
    values = [(37 * i + 11) % 251 for i in range(len(lengths))]
    for i in range(1, len(values)):
        if values[i] == values[i - 1]:
            values[i] += 1
    return np.concatenate([runs_buffer(lengths, values), np.arange(256, dtype=np.uint8)[::-1], np.arange(256, dtype=np.uint8)])


def random_runs(rng, n, choices):
    out, at = np.zeros(n, np.uint8), 0
    v = 0
    while at < n:
        length = int(rng.choice(choices))
        v = (v + 1 + int(rng.integers(0, 5))) % 256
        out[at:at + length] = v
        at += length
    return out


@functools.lru_cache(maxsize=None)
def deflate_cases():
    rng = np.random.default_rng(23)
    cases = {}
    cases["constant"] = (np.full((1, 40, 64), 7, np.uint8), 16)
    cases["constant_one_stripe"] = (np.zeros((1, 3, 1000), np.uint8), 3)
    cases["one_byte"] = (np.full((1, 1, 1), 200, np.uint8), 16)
    runs = runs_buffer(RUN_LENGTHS + RUN_LENGTHS[::-1])
    cases["runs"] = (runs.reshape(1, 1, -1), 1)
    cases["runs_in_rows"] = (np.concatenate([runs, runs[:len(runs) % 2]]).reshape(1, 2, -1), 1)
    # a run from byte 100 to byte 160 of a buffer whose stripes are 128 bytes: it meets the stripe boundary and is cut there
    meet = (np.arange(256) * 5 % 251).astype(np.uint8)
    meet[100:160] = 9
    cases["run_meets_stripe"] = (meet.reshape(1, 4, 64), 2)
    cases["two_values"] = ((rng.random((1, 8, 257)) < 0.3).astype(np.uint8), 4)
    cases["every_symbol"] = (every_symbol().reshape(1, 1, -1), 1)
    cases["fibonacci"] = (fibonacci_bytes().reshape(1, 1, -1), 16)
    cases["noise"] = (rng.integers(0, 256, (1, 4, 20000), dtype=np.uint8), 4)            # one stripe of 80000 bytes: two stored blocks
    cases["noise_small_stripes"] = (rng.integers(0, 256, (2, 5, 33), dtype=np.uint8), 2)
    for rb in LANE_WIDTHS:
        data = random_runs(rng, 6 * rb, (1, 1, 2, 3, 4, 5, 62, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 258, 259, 260, 300))
        cases[f"lanes_{rb}"] = (data.reshape(1, 6, rb), 3)
    three = np.zeros((3, 20, 100), np.uint8)
    three[1] = random_runs(rng, 2000, (1, 2, 3, 7, 40)).reshape(20, 100)
    three[2] = rng.integers(0, 256, (20, 100), dtype=np.uint8)
    cases["three_frames"] = (three, 8)                                                  # 20 rows: stripes of 8, 8 and 4
    cases["past_the_grid_cap"] = (rng.integers(0, 3, (2, 2060, 3), dtype=np.uint8), 1)   # 4120 stripes
    return cases


def model(name):
    """-> per frame, ``pm.deflate_rows`` of the case."""
    return _model(name)


@functools.lru_cache(maxsize=None)
def _model(name):
    rows, stripe_rows = deflate_cases()[name]
    return [pm.deflate_rows(rows[f], stripe_rows) for f in range(rows.shape[0])]
