"""The PNG encoder without a GPU: the format of tests/png_model.py read back by zlib and Pillow, the constructed buffers of
tests/png_cases.py through its deflate half, csrc/png_huffman.hpp as a host program under sanitizers against the model's lengths,
seeded defects of the model that must be seen, the size of the model's streams against zlib's Z_RLE, the host half of
vface_amd/scripts/png.py, the flag and the binding."""
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases as cases
import png_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vface_amd", "csrc")
SIZES = ((1, 1), (2, 1), (1, 2), (3, 5), (21, 5), (85, 2), (86, 2), (250, 136))      # (W, H); row_bytes 64, 256 and 259 among them
STRIPES = (1, 2, 16)
# Size condition ("Frames out, PNG").  Reference: zlib Z_RLE, level 6, ONE stream over the same filtered bytes.  Allowed on
# top: per stripe pm.STRIPE_OVERHEAD_BYTES (the largest header the layout can emit, the end of block, the sync), and a proportional
# term for block boundaries: measured on these frames, stripe overheads included, at +0.0702 % (smooth), -0.0774 % (noisy) and
# -0.0105 % (noise) -- the model is SMALLER than zlib on two of three -- and asserted as the measured worst case plus one percentage point.
MEASURED_WORST = 0.000702
PROPORTIONAL = MEASURED_WORST + 0.01


def inflate_stripes(d):
    """Every stripe's bytes through a FRESH raw inflater: a match that reaches back over the stripe's first byte cannot decode."""
    out = []
    for blk in d["stripes"]:
        z = zlib.decompressobj(-15)
        out.append(z.decompress(blk) + z.flush())
    return out


def seen(frame, stripe_rows, defect):
    """True if the defect shows: zlib or Pillow refuses the file, a stripe does not decode on its own, or the pixels differ."""
    try:
        rows = pm.filter_rows(frame, defect)
        stream, d = pm.zlib_stream(rows, stripe_rows, defect)
        if zlib.decompress(stream) != rows.tobytes():
            return True
        if b"".join(inflate_stripes(d)) != rows.tobytes():
            return True
        im = Image.open(io.BytesIO(pm.png_file(frame.shape[1], frame.shape[0], stream)))
        im.load()
        return not np.array_equal(np.asarray(im), frame)
    except Exception:                                   # zlib.error, Pillow's OSError / SyntaxError
        return True


@pytest.mark.parametrize("W,H", SIZES)
def test_files_decode_to_the_frames(W, H):
    """Model file -> Image.open equals the frame; zlib.decompress(stream) equals the filtered rows; every stripe decodes alone."""
    for name, frames in pm.patterns(2, W, H, seed=W + H).items():
        for stripe_rows in STRIPES + (3,):              # 5 and 136 are no multiples of 3 and 16
            for frame in frames:
                rows = pm.filter_rows(frame)
                stream, d = pm.zlib_stream(rows, stripe_rows)
                assert zlib.decompress(stream) == rows.tobytes(), (name, stripe_rows)
                assert len(d["body"]) <= pm.deflate_bound(1 + 3 * W, H, stripe_rows)
                lens = [min(stripe_rows, H - r) * (1 + 3 * W) for r in range(0, H, stripe_rows)]
                assert [len(b) for b in inflate_stripes(d)] == lens
                im = Image.open(io.BytesIO(pm.encode(frame, stripe_rows)))
                assert im.mode == "RGB" and im.size == (W, H) and np.array_equal(np.asarray(im), frame), (name, stripe_rows)


def test_container_is_four_chunks():
    data = pm.encode(pm.patterns(1, 21, 5)["smooth"][0], 2)
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, kinds = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        assert zlib.crc32(data[at + 4:at + 8 + n]) == struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]
        kinds.append(kind)
        at += 12 + n
    assert kinds == [b"IHDR", b"IDAT", b"IEND"] and data[16:29] == struct.pack(">IIBBBBB", 21, 5, 8, 2, 0, 0, 0)


@pytest.mark.parametrize("name", sorted(cases.deflate_cases()))
def test_constructed_buffers_decode(name):
    rows, stripe_rows = cases.deflate_cases()[name]
    for f, d in enumerate(cases.model(name)):
        H, rb = rows[f].shape
        value = pm.adler_combine([(s1, s2, min(stripe_rows, H - r) * rb) for (s1, s2), r in zip(d["adler"], range(0, H, stripe_rows))])
        assert value == zlib.adler32(rows[f].tobytes())
        assert zlib.decompress(b"\x78\x01" + d["body"] + struct.pack(">I", value)) == rows[f].tobytes()
        assert b"".join(inflate_stripes(d)) == rows[f].tobytes()
        assert len(d["body"]) <= pm.deflate_bound(rb, H, stripe_rows)


def test_the_cases_hold_what_they_promise():
    c, m = cases.deflate_cases(), cases.model
    sym = pm.tokens(c["runs"][0].reshape(-1))[0]
    # runs of 1, 2, 3: literals only; 4: one match of 3; 258: one of 257; 259: one of 258; 260, 261: 258 and literals; 262: 258 and 3;
    # 517: two of 258
    assert (sym == 285).sum() == 2 * (1 + 1 + 1 + 1 + 2) and (sym == 284).sum() == 2 and (sym == 257).sum() == 2 * 2
    assert pm.tokens(np.full(261, 5, np.uint8))[0].tolist() == [5, 285, 5, 5] and pm.tokens(np.full(262, 5, np.uint8))[0].tolist() == [5, 285, 257]
    assert pm.tokens(np.full(3, 5, np.uint8))[0].tolist() == [5, 5, 5] and pm.tokens(np.full(4, 5, np.uint8))[0].tolist() == [5, 257]
    count = m("every_symbol")[0]["details"][0]["count"]
    assert (count[:256] > 0).all() and (count[257:286] > 0).all() and m("every_symbol")[0]["kinds"] == ["dynamic"]
    fib = m("fibonacci")[0]["details"][0]
    assert max(pm.huffman_lengths(fib["count"], 64)) > 15 and max(fib["lengths"]) == 15 and m("fibonacci")[0]["kinds"] == ["dynamic"]
    sr = c["noise"][1]
    noise = m("noise")[0]
    assert noise["kinds"] == ["stored"] and len(noise["body"]) == pm.deflate_bound(20000, 4, sr) == 80000 + 2 * 5 + 2
    assert noise["stripes"][0][:5] == b"\x00\xff\xff\x00\x00" and noise["stripes"][0][65540:65545] == b"\x00" + struct.pack("<HH", 14465, 14465 ^ 0xFFFF)
    assert set(m("noise_small_stripes")[0]["kinds"]) == {"stored"}
    assert m("constant")[0]["kinds"] == ["dynamic"] * 3 and len({len(d["body"]) for d in m("three_frames")}) == 3
    two = m("two_values")[0]["details"][0]["count"]
    assert (two[:256] > 0).sum() == 2
    # the run 100..160 is cut at byte 128: a literal and a match on either side
    stripes = m("run_meets_stripe")[0]
    assert pm.tokens(c["run_meets_stripe"][0].reshape(-1)[128:256])[0][:2].tolist() == [9, 257 + 15] and len(stripes["stripes"]) == 2


def test_each_filter_type_is_chosen_and_ties_go_low():
    W = 32
    rng = np.random.default_rng(1)
    ramp = (np.arange(W * 3).reshape(W, 3) * 5 % 256).astype(np.uint8)
    noise = rng.integers(0, 256, (W, 3), dtype=np.uint8)
    prev = rng.integers(0, 200, (W, 3)).astype(np.int64)
    avg = np.zeros((W, 3), np.int64)
    for i in range(W):
        avg[i] = ((avg[i - 1] if i else 0) + prev[i]) >> 1
    # zeros on top: every type gives zeros, a five-way tie -> None.  A ramp: Sub.  Noise under a ramp: None.  The row above again:
    # Up.  Under a noise row, x = (left + above) >> 1: Average
    frame = np.stack([np.zeros((W, 3), np.uint8), ramp, noise, noise, prev.astype(np.uint8), avg.astype(np.uint8)])
    best = pm.filter_rows(frame)[:, 0].tolist()
    assert best[:4] == [0, 1, 0, 2] and best[5] == 3
    cost = np.abs(pm.filter_candidates(frame).astype(np.int8).astype(np.int64)).sum(axis=2)
    assert (cost[:, 0] == 0).all()
    # steps along the row and down the rows: Paeth follows whichever neighbour did not step
    steps = np.zeros((8, W, 3), np.uint8)
    for r in range(8):
        for i in range(W):
            steps[r, i] = 40 * ((r + 1) // 2 % 2) + 90 * ((i + r) // 3 % 2) + (r * 7 + i * 3) % 5
    assert pm.filter_rows(steps)[:, 0].tolist() == [1, 1, 4, 1, 2, 1, 3, 1]
    # ties: a constant row under the same constant row: Up and Paeth both give zeros, Up is the lower type; on a frame's first row Sub
    # and Paeth are the same bytes (Paeth of (a, 0, 0) is a) and Sub is the lower type
    flat = np.full((2, W, 3), 77, np.uint8)
    assert pm.filter_rows(flat)[:, 0].tolist() == [1, 2]
    cost = np.abs(pm.filter_candidates(flat).astype(np.int8).astype(np.int64)).sum(axis=2)
    assert cost[2, 1] == cost[4, 1] == 0 and cost[1, 0] == cost[4, 0] < cost[0, 0]


def test_adler_combine_across_the_modulus():
    from vface_amd.scripts import png
    rng = np.random.default_rng(9)
    for sizes in ((1,), (5, 7), (70000, 3, 66000), (300000, 300000), (1, 65521, 65520, 2)):
        pieces = [rng.integers(200, 256, n, dtype=np.uint8).tobytes() for n in sizes]     # large bytes: the sums wrap 65521 many times
        parts = [pm.adler_pair(p) + (len(p),) for p in pieces]
        assert all((s2 << 16 | s1) == zlib.adler32(p) for (s1, s2, _), p in zip(parts, pieces))
        want = zlib.adler32(b"".join(pieces))
        assert pm.adler_combine(parts) == want and png.adler32_combine(parts) == want
    ff = [b"\xff" * 65521, b"\xff" * 65522]
    assert png.adler32_combine([pm.adler_pair(p) + (len(p),) for p in ff]) == zlib.adler32(b"".join(ff))


@pytest.mark.parametrize("defect", pm.DEFECTS)
def test_seeded_defects_are_seen(defect):
    """Each one-line mistake of the model shows on a frame built for it; the same frame without the defect is clean."""
    rng = np.random.default_rng(17)
    if defect == "match_over_stripe_start":
        # a noise row plus 2 per row: Up leaves rows of 2s under the filter byte 2, so a run crosses every stripe's first byte
        frame = ((rng.integers(0, 256, (1, 40, 3)) + 2 * np.arange(8)[:, None, None]) % 256).astype(np.uint8)
        assert (pm.filter_rows(frame)[1:4] == 2).all()     # rows 1..3: the stripe that starts at row 2 continues row 1's run
        frames = [(frame, 2)]
    elif defect == "stored_nlen":
        frames = [(rng.integers(0, 256, (8, 40, 3), dtype=np.uint8), 4)]
    elif defect == "remainder_2_as_match":
        frame = np.zeros((8, 40, 3), np.uint8)
        frame[:, ::4] = 90                              # runs of 3 equal bytes: a literal and a remainder of 2
        frames = [(frame, 2), (np.full((8, 40, 3), 55, np.uint8), 2)]
    else:
        frames = [(pm.content("noisy", 64, 48, seed=2), 16), (pm.patterns(1, 40, 24)["blocks"][0], 8)]
    assert not any(seen(frame, sr, None) for frame, sr in frames)
    assert any(seen(frame, sr, defect) for frame, sr in frames), defect


def host_compiler():
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    return cxx


def probe_histograms():
    """(counts, maxbits): one and two symbols used, all 286, Fibonacci counts that force depths above 15 and above 7 before the limit,
    flat and steep shapes, and 20 000 seeded random ones."""
    rng = np.random.default_rng(31)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    out = []
    for n, maxbits in ((pm.LITLEN, pm.LITLEN_BITS), (pm.CODELEN, pm.CODELEN_BITS)):
        one = np.zeros(n, np.uint32)
        one[n // 2] = 9
        two = one.copy()
        two[0] = 1
        out += [(one, maxbits), (two, maxbits), (np.ones(n, np.uint32), maxbits), (np.arange(1, n + 1, dtype=np.uint32), maxbits),
                (np.full(n, 0x7FFFFF, np.uint32), maxbits)]
        for k in (maxbits + 2, min(n, 40), min(n, 19)):
            f = np.zeros(n, np.uint32)
            f[rng.permutation(n)[:k]] = fib[:k]
            out.append((f, maxbits))
    out.append((np.array(fib[:19], np.uint32), pm.CODELEN_BITS))
    for i in range(20000):
        n, maxbits = ((pm.LITLEN, pm.LITLEN_BITS), (pm.CODELEN, pm.CODELEN_BITS))[i % 4 == 0]
        shape = i % 5
        if shape == 0:
            c = rng.integers(0, 1 << int(rng.integers(1, 24)), n)
        elif shape == 1:
            c = rng.geometric(0.3, n) - 1
        elif shape == 2:
            c = (2.0 ** rng.uniform(0, 22, n)).astype(np.int64) * (rng.random(n) < rng.random())
        elif shape == 3:
            c = rng.integers(0, 3, n)
        else:
            c = np.rint(rng.exponential(1.0, n) ** 6).astype(np.int64) % (1 << 24)
        out.append((c.astype(np.uint32), maxbits))
    return out


def test_huffman_routine_under_sanitizers(tmp_path):
    """csrc/png_huffman.hpp as a host program with -fsanitize=address,undefined: Kraft sum 1, the limits, the kernel's ranked way
    equal to the serial one (checked by the program), and every record's lengths equal to the model's."""
    exe = str(tmp_path / "png_huffman_probe")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "png_huffman_probe.cpp"), "-o", exe], check=True)
    hists = probe_histograms()
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for c, maxbits in hists:
            f.write(struct.pack("<ii", len(c), maxbits) + np.ascontiguousarray(c, np.uint32).tobytes())
    done = subprocess.run([exe, path], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    lines = done.stdout.splitlines()
    assert lines[-1] == f"records {len(hists)}" and len(lines) == len(hists) + 1
    deep15 = deep7 = 0
    for (c, maxbits), line in zip(hists, lines):
        want = pm.huffman_lengths(c.tolist(), maxbits)
        assert line == "lengths " + " ".join(map(str, want)), (c.tolist(), maxbits, line)
        used = [x for x in want if x]
        if len(used) >= 2:
            assert sum(2.0 ** -x for x in used) == 1.0 and max(used) <= maxbits
        if max(pm.huffman_lengths(c.tolist(), 64), default=0) > maxbits:
            deep15 += maxbits == 15
            deep7 += maxbits == 7
    assert deep15 >= 3 and deep7 >= 3, (deep15, deep7)


@pytest.fixture(scope="module")
def size_frames():
    return {kind: pm.content(kind, 512, 512, seed=4) for kind in ("smooth", "noisy", "noise")}


def test_size_against_zlib_rle(size_frames):
    """The model's stream at the default stripe height against zlib Z_RLE, level 6, one stream over the same filtered bytes (see the
    derivation at the top of this file); Pillow's level 6 is recorded, not asserted: LZ77 beyond distance 1 pays on the noise-free
    gradient, which comes out larger here."""
    from vface_amd import hip
    sr = hip.PNG_STRIPE_ROWS
    for kind, frame in size_frames.items():
        rows = pm.filter_rows(frame)
        stream, d = pm.zlib_stream(rows, sr)
        z = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        ref = z.compress(rows.tobytes()) + z.flush()
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, "PNG")
        allowed = len(ref) * (1 + PROPORTIONAL) + len(d["stripes"]) * pm.STRIPE_OVERHEAD_BYTES
        print(f"{kind}: model {len(stream)}  Z_RLE {len(ref)} ({len(stream) / len(ref) - 1:+.4%})  allowed {allowed:.0f}  "
              f"Pillow file {len(buf.getvalue())}  model file {len(pm.png_file(512, 512, stream))}")
        assert len(stream) <= allowed, kind
        assert zlib.decompress(stream) == rows.tobytes()
        assert max(det["header_bits"] for det in d["details"]) <= pm.MAX_HEADER_BITS


def test_host_half_and_flag():
    """png_file frames a body the way the model does; PNGEncoder refuses CPU tensors; the flag parses and defaults to pillow; the
    binding lists the entry points."""
    import torch
    from vface_amd import hip
    from vface_amd.scripts import VFace_inference_batch as cli
    from vface_amd.scripts import png
    frame = pm.patterns(1, 21, 5)["smooth"][0]
    rows = pm.filter_rows(frame)
    stream, d = pm.zlib_stream(rows, 2)
    value = zlib.adler32(rows.tobytes())
    assert png.png_file(21, 5, d["body"], value) == pm.png_file(21, 5, stream) == pm.encode(frame, 2)
    enc = png.PNGEncoder(21, 5)
    assert enc.stripe_rows == hip.PNG_STRIPE_ROWS
    for bad in (torch.from_numpy(frame)[None], "frames"):
        with pytest.raises(hip.VFaceHipError):
            enc.encode(bad)
    opt = cli.build_parser().parse_args([])
    assert opt.png_encoder == "pillow"
    assert cli.build_parser().parse_args(["--png_encoder", "gpu"]).png_encoder == "gpu"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--png_encoder", "zlib"])
    lib = hip.load()
    for name in ("vface_png_filter", "vface_png_deflate", "vface_png_deflate_workspace_bytes", "vface_png_deflate_bound"):
        assert hasattr(lib, name)
    for rb, H, sr in ((1, 1, 1), (64, 5, 2), (20000, 4, 4), (65535, 3, 1), (65536, 2, 2), (5761, 1080, 16)):
        assert hip.png_deflate_bound(rb, H, sr) == pm.deflate_bound(rb, H, sr)
    assert lib.vface_png_deflate_workspace_bytes(0, 1, 1, 1) == 0 and lib.vface_png_deflate_workspace_bytes(64, 5, 2, 2) > 2 * 5 * 64
