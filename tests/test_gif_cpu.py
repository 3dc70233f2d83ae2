"""The GIF writer without a GPU: the format of tests/gif_model.py read back by Pillow and by the model's own decoder, the constructed
index streams of tests/gif_cases.py, the median cut's corner cases, quality and size against Pillow, seeded defects of the model that
must be seen, csrc/gif_palette.hpp and csrc/gif_lzw.hpp as a host program under sanitizers against the model, the host half of
vface_amd/scripts/gif.py, the flags and the binding."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import gif_cases as cases
import gif_model as gm
import png_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vface_amd", "csrc")
SIZES = ((1, 1), (2, 1), (1, 2), (3, 5), (21, 5), (85, 2), (250, 136))                  # (W, H)
# Quality ("Video out, GIF").  Reference: Pillow's quantize(256, MEDIANCUT, dither=NONE) on the same frame; the figure is
# the model's mean squared error against the source divided by Pillow's.  Both are deterministic; the bound is the measured ratio
# rounded up to two decimals.  (W, H, content) -> bound; the measured ratios stand in DESIGN.
QUALITY_BOUND = {(250, 136, "smooth"): 0.73, (250, 136, "noisy"): 0.90, (250, 136, "noise"): 0.34,
                 (512, 512, "smooth"): 0.62, (512, 512, "noisy"): 0.72, (512, 512, "noise"): 0.66}
# Size.  Reference: the image data of Pillow's own GIF save of the same P image (same palette, same indices): one LZW stream, the
# table cleared when it fills.  The figure is the model's image-data bytes at hip.GIF_SEG_PIXELS divided by Pillow's, pinned the same way.
SIZE_BOUND = {(250, 136, "smooth"): 0.84, (250, 136, "noisy"): 0.83, (250, 136, "noise"): 1.00,
              (512, 512, "smooth"): 0.78, (512, 512, "noisy"): 0.83, (512, 512, "noise"): 1.00}


def test_frames(F, W, H, seed):
    p = pm.patterns(F, W, H, seed=seed)
    return np.stack([p[k][f] for f, k in zip(range(F), ("noise", "smooth", "blocks"))])


test_frames.__test__ = False


def grey_file(indices, image):
    """A one-frame GIF around ``image`` (image data): npix x 1, palette entry i = (i, i, i): Pillow's decoder on an index stream."""
    pal = np.repeat(np.arange(256, dtype=np.uint8), 3).tobytes()
    return gm.header(len(indices), 1) + gm.frame_header(len(indices), 1) + pal + image + b"\x3B"


def pillow_indices(data, frame=0):
    im = Image.open(io.BytesIO(data))
    im.seek(frame)
    return np.asarray(im.convert("RGB"))[..., 0].reshape(-1)


def image_data_of(data):
    """The image data of the FIRST frame of any GIF file, walked block by block."""
    packed = data[10]
    at = 13 + ((3 << ((packed & 7) + 1)) if packed & 0x80 else 0)
    while data[at] == 0x21:
        at += 2
        while data[at]:
            at += 1 + data[at]
        at += 1
    assert data[at] == 0x2C
    packed = data[at + 9]
    at += 10 + ((3 << ((packed & 7) + 1)) if packed & 0x80 else 0)
    start = at
    at += 1
    while data[at]:
        at += 1 + data[at]
    return data[start:at + 1]


# ---- Pillow opens the model's file
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("F", [1, 3])
def test_pillow_opens_the_models_file(W, H, F):
    frames = test_frames(F, W, H, seed=W + 2 * H)
    qs = [gm.quantise(frame) for frame in frames]                          # the quantiser does not depend on the segments
    for seg in (1, 7, 64, 4096, W * H + 1):
        data, _ = gm.gif_file(frames, seg, qs=qs)
        im = Image.open(io.BytesIO(data))
        assert im.format == "GIF" and im.size == (W, H) and getattr(im, "n_frames", 1) == F, seg
        at = len(gm.header(W, H))
        for f in range(F):
            im.seek(f)
            assert im.info["duration"] == 100 and im.info["loop"] == 0, (seg, f, im.info)
            want = qs[f]["palette"][qs[f]["indices"]].reshape(H, W, 3)
            assert np.array_equal(np.asarray(im.convert("RGB")), want), (seg, f)
            # the model's own decoder inverts its encoder, and the length formula holds
            at += len(gm.frame_header(W, H)) + 768
            idx, used = gm.decode_image_data(data[at:], W * H)
            assert np.array_equal(idx, qs[f]["indices"]), (seg, f)
            assert used == gm.image_data_bytes(len(gm.lzw(qs[f]["indices"], seg)["data"])) <= gm.lzw_bound(W * H, seg), (seg, f)
            at += used
        assert data[at:] == b"\x3B"


def test_container_layout():
    W, H = 21, 5
    data, qs = gm.gif_file(test_frames(2, W, H, seed=1), 64)
    assert data[:6] == b"GIF89a" and struct.unpack("<HH", data[6:10]) == (W, H) and data[10] & 0x80 == 0          # no global colour table
    assert data[13:32] == b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\x00\x00\x00" and len(gm.header(W, H)) == 32
    fh = data[32:32 + 18]
    assert fh[:4] == b"\x21\xF9\x04\x04" and struct.unpack("<H", fh[4:6]) == (10,) and fh[6:8] == b"\x00\x00"      # disposal 1, no transparency
    assert fh[8:9] == b"\x2C" and struct.unpack("<HHHH", fh[9:17]) == (0, 0, W, H) and fh[17] == 0x87               # local table of 256
    assert data[50:50 + 768] == qs[0]["palette"].tobytes() and data[50 + 768] == 8


# ---- constructed index streams
@pytest.mark.parametrize("name", sorted(cases.lzw_cases()))
def test_constructed_streams_decode(name):
    frames, seg = cases.lzw_cases()[name]
    for idx, m in zip(frames, cases.model(name)):
        got, used = gm.decode_image_data(m["image"], len(idx))
        assert np.array_equal(got, idx) and used == len(m["image"]) == gm.image_data_bytes(len(m["lzw"]["data"])), name
        assert len(m["image"]) <= gm.lzw_bound(len(idx), seg), name
        assert np.array_equal(pillow_indices(grey_file(idx, m["image"])), idx), name
        for s in m["lzw"]["segments"]:
            assert s["bits"] == gm.code_bits(len(s["codes"])) and len(s["codes"]) <= gm.max_codes(seg), name
            assert all(code < 1 << w for code, w in s["codes"]), name


def test_the_cases_hold_what_they_promise():
    m = cases.model
    one = m("one_value")[0]["lzw"]["segments"][0]["codes"]
    assert [c for c, _ in one[:4]] == [7, 258, 259, 260]                                  # 7, 77, 777, ..: every code one seven longer
    assert len({c for c, _ in m("two_values")[0]["lzw"]["segments"][0]["codes"]} & {0, 200}) == 2
    assert {c for c, _ in m("all_values")[0]["lzw"]["segments"][0]["codes"]} >= set(range(256))
    fill = m("noise_fills_table")[0]["lzw"]["segments"]
    assert len(fill) == 1 and fill[0]["forced"] >= 1
    at = [j for j, (c, _) in enumerate(fill[0]["codes"]) if c == gm.CLEAR]
    assert at[0] == gm.PERIOD - 1 and fill[0]["codes"][at[0]][1] == 12 and fill[0]["codes"][at[0] + 1][1] == 9
    assert sum(s["forced"] for s in m("noise_three_tables_in_segments")[0]["lzw"]["segments"]) >= 2
    for t in cases.NEXT_TARGETS:
        first = m(f"next_{t}")[0]["lzw"]["segments"]
        assert len(first) == 2 and first[0]["next"] == t and first[0]["codes"][-1][0] == gm.CLEAR
        last = m(f"next_{t}_last")[0]["lzw"]["segments"]
        assert len(last) == 1 and last[0]["next"] == t and last[0]["codes"][-1] == (gm.EOI, max(9, min(12, t.bit_length())))
    # the terminator's width follows the table size it falls on: the decoder widens when its next free code is 512, before it reads on
    assert [m(f"next_{t}_last")[0]["lzw"]["segments"][0]["codes"][-1][1] for t in (511, 512, 513)] == [9, 10, 10]
    for b in cases.BYTE_TARGETS:
        assert len(m(f"bytes_{b}")[0]["lzw"]["data"]) == b
        assert len(m(f"bytes_{b}")[0]["image"]) == 1 + b + (2 if b <= 255 else 3 if b <= 510 else 4)
    assert len({len(x["image"]) for x in m("three_frames")}) == 3
    assert len(m("seg_1")[0]["lzw"]["segments"]) == 300 and len(m("seg_above_npix")[0]["lzw"]["segments"]) == 1


# ---- boxes and palette
def frame_of_cells(cells, counts=None):
    """A frame [1, n, 3] with counts[i] pixels at the centre of every cell (r, g, b in cells)."""
    counts = [1] * len(cells) if counts is None else counts
    px = [[8 * r + 4, 8 * g + 4, 8 * b + 4] for (r, g, b), n in zip(cells, counts) for _ in range(n)]
    return np.array(px, np.uint8).reshape(1, -1, 3)


def test_one_colour_and_zero_padding():
    q = gm.quantise(np.full((4, 6, 3), (9, 200, 77), np.uint8))
    assert q["ncolors"] == 1 and q["palette"][0].tolist() == [9, 200, 77] and not q["palette"][1:].any() and not q["indices"].any()
    q = gm.quantise(frame_of_cells([(0, 0, 0), (5, 5, 5), (31, 0, 9)], [3, 1, 2]))
    assert q["ncolors"] == 3 and not q["palette"][3:].any() and sorted(map(tuple, q["palette"][:3].tolist())) == [(4, 4, 4), (44, 44, 44), (252, 4, 76)]


def test_up_to_256_colours_in_distinct_cells_come_back_exactly():
    rng = np.random.default_rng(3)
    cells = rng.permutation(32768)[:256]
    frame = np.stack([(cells >> 10) * 8 + rng.integers(0, 8, 256), ((cells >> 5) & 31) * 8 + rng.integers(0, 8, 256),
                      (cells & 31) * 8 + rng.integers(0, 8, 256)], axis=1).astype(np.uint8)
    frame = np.concatenate([frame, frame[:100], frame[:7]]).reshape(1, -1, 3)          # some colours more than once
    q = gm.quantise(frame)
    assert q["ncolors"] == 256 and np.array_equal(q["palette"][q["indices"]], frame.reshape(-1, 3))
    assert len(set(q["labels"][cells].tolist())) == 256


def test_257_cells_and_a_box_that_cannot_be_split():
    rng = np.random.default_rng(4)
    cells = rng.permutation(32768)[:257]
    frame = frame_of_cells([(c >> 10, (c >> 5) & 31, c & 31) for c in cells])
    q = gm.quantise(frame)
    sizes = np.bincount(q["labels"][cells], minlength=256)
    assert q["ncolors"] == 256 and sorted(sizes.tolist()) == [1] * 255 + [2]
    # two cells, 1000 pixels of many colours in one of them: one split, and neither box can be split again
    crowd = np.stack([rng.integers(0, 8, 1000), rng.integers(0, 8, 1000), rng.integers(0, 8, 1000)], axis=1)
    frame = np.concatenate([crowd, [[255, 255, 255]]]).astype(np.uint8).reshape(1, -1, 3)
    q = gm.quantise(frame)
    assert q["ncolors"] == 2 and [b["ncells"] for b in q["boxes"]] == [1, 1] and [b["pop"] for b in q["boxes"]] == [1000, 1]
    assert all(gm.box_key(b["pop"], b["lo"], b["hi"], b["ncells"], i) == 0 for i, b in enumerate(q["boxes"]))
    assert q["palette"][1].tolist() == [255, 255, 255] and q["palette"][0].tolist() == [int((2 * crowd[:, k].sum() + 1000) // 2000) for k in range(3)]


def test_ties_on_every_choice():
    """One pixel in each corner cell of the cube: equal keys (the lowest box number is split), equal sides (R before G before B), and a
    cut that falls exactly on the median (2 x 4 >= 8: the lower side ends there).  The labels are worked out by hand."""
    corners = [(r, g, b) for r in (0, 31) for g in (0, 31) for b in (0, 31)]
    q = gm.quantise(frame_of_cells(corners))
    want = {(0, 0, 0): 0, (0, 0, 31): 4, (0, 31, 0): 2, (0, 31, 31): 6, (31, 0, 0): 1, (31, 0, 31): 5, (31, 31, 0): 3, (31, 31, 31): 7}
    assert q["ncolors"] == 8
    assert {c: int(q["labels"][c[0] << 10 | c[1] << 5 | c[2]]) for c in corners} == want
    # a tie between palette entries: a pixel half way between two goes to the lower index
    pal = np.zeros((256, 3), np.uint8)
    pal[0], pal[1], pal[2] = (10, 10, 10), (20, 10, 10), (10, 20, 10)
    assert gm.index_map(np.array([[[15, 10, 10], [15, 15, 10], [10, 15, 10], [21, 10, 10]]], np.uint8), pal, 3).tolist() == [0, 0, 0, 1]
    # the mean rounds halves up
    q = gm.quantise(np.array([[[0, 1, 2], [1, 2, 2]]], np.uint8))
    assert q["palette"][0].tolist() == [1, 2, 2]


# ---- quality and size
@pytest.fixture(scope="module")
def measured():
    out = {}
    for W, H in ((250, 136), (512, 512)):
        for kind in ("smooth", "noisy", "noise"):
            frame = pm.content(kind, W, H, seed=4)
            out[W, H, kind] = (frame, gm.quantise(frame))
    return out


def test_quality_against_pillows_median_cut(measured):
    for key, (frame, q) in measured.items():
        ours = ((q["palette"][q["indices"]].astype(np.float64) - frame.reshape(-1, 3)) ** 2).mean()
        ref = Image.fromarray(frame).quantize(256, Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE).convert("RGB")
        theirs = ((np.asarray(ref).astype(np.float64) - frame) ** 2).mean()
        print(f"{key}: model MSE {ours:.3f}  Pillow MEDIANCUT {theirs:.3f}  ratio {ours / theirs:.4f}  bound {QUALITY_BOUND[key]}")
        assert ours / theirs <= QUALITY_BOUND[key], key


def test_size_against_pillows_gif_save(measured):
    from vface_amd import hip
    for key, (frame, q) in measured.items():
        W, H, _ = key
        im = Image.fromarray(q["indices"].reshape(H, W), "P")
        im.putpalette(q["palette"].tobytes())
        buf = io.BytesIO()
        im.save(buf, "GIF")
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")), q["palette"][q["indices"]].reshape(H, W, 3))
        theirs = len(image_data_of(buf.getvalue()))
        ours = len(gm.image_data(q["indices"], hip.GIF_SEG_PIXELS))
        print(f"{key}: model {ours} bytes at seg_pixels {hip.GIF_SEG_PIXELS}  Pillow {theirs}  ratio {ours / theirs:.4f}  bound {SIZE_BOUND[key]}")
        assert ours / theirs <= SIZE_BOUND[key], key


# ---- seeded defects
def violations(frames, seg, defect):
    """What is wrong with the model's answer for ``frames`` [F, H, W, 3], each statement checked without the model's own code: the
    cells, the boxes, the means, the nearest entries, the file through Pillow and the stream through the model's decoder."""
    F, H, W, _ = frames.shape
    bad = []
    try:
        data, qs = gm.gif_file(frames, seg, defect)
    except Exception as e:                                                  # e.g. a mean over no pixel
        return [f"model: {type(e).__name__}"]
    for f, (frame, q) in enumerate(zip(frames, qs)):
        px = frame.reshape(-1, 3).astype(np.int64)
        cell = px[:, 0] // 8 * 1024 + px[:, 1] // 8 * 32 + px[:, 2] // 8
        if not np.array_equal(q["counts"], np.bincount(cell, minlength=32768)):
            bad.append("counts")
            continue
        used = np.flatnonzero(q["counts"])
        lab = q["labels"][cell]
        n = np.bincount(lab, minlength=256)
        if q["ncolors"] != min(256, len(used)) or (n[:q["ncolors"]] == 0).any() or n[q["ncolors"]:].any():
            bad.append("boxes")
            continue
        for i in range(q["ncolors"]):
            mean = np.floor(px[lab == i].mean(axis=0) + 0.5).astype(np.int64)      # halves up; exact: sums below 2^53
            if q["palette"][i].tolist() != mean.tolist():
                bad.append("palette")
                break
        if q["palette"][q["ncolors"]:].any():
            bad.append("padding")
        d = ((px[:, None, :] - q["palette"][None, :q["ncolors"]].astype(np.int64)) ** 2).sum(axis=2)
        lowest = np.array([np.flatnonzero(row == row.min())[0] for row in d])
        if not np.array_equal(q["indices"], lowest):
            bad.append("indices")
    try:
        im = Image.open(io.BytesIO(data))
        if getattr(im, "n_frames", 1) != F:
            bad.append("n_frames")
        for f, q in enumerate(qs):
            im.seek(f)
            if not np.array_equal(np.asarray(im.convert("RGB")), q["palette"][q["indices"]].reshape(H, W, 3)):
                bad.append("pixels")
    except Exception as e:                                                  # Pillow's OSError / SyntaxError / EOFError
        bad.append(f"pillow: {type(e).__name__}")
    return bad


def stream_violations(idx, seg, defect):
    """The LZW half alone on an index stream: the model's decoder, Pillow, and the promise of a forced Clear."""
    bad = []
    d = gm.lzw(idx, seg, defect)
    image = gm.sub_blocks(d["data"], defect)
    try:
        got, used = gm.decode_image_data(image, len(idx))
        if not np.array_equal(got, idx) or used != len(image):
            bad.append("decoder")
    except Exception as e:
        bad.append(f"decoder: {type(e).__name__}")
    try:
        if not np.array_equal(pillow_indices(grey_file(idx, image)), idx):
            bad.append("pillow")
    except Exception as e:
        bad.append(f"pillow: {type(e).__name__}")
    if len(idx) >= 12000 and seg > len(idx) and sum(s["forced"] for s in d["segments"]) < 1:
        bad.append("no forced Clear in 12 000 noise indices")
    return bad


@pytest.mark.parametrize("defect", gm.DEFECTS)
def test_seeded_defects_are_seen(defect):
    """Each one-line mistake of the model shows on inputs built for it; the same inputs without the defect are clean."""
    rng = np.random.default_rng(17)
    frames = [(np.stack([pm.content("noisy", 40, 24, seed=2), pm.patterns(1, 40, 24)["blocks"][0], pm.patterns(1, 40, 24)["noise"][0]]), 64),
              (np.array([[[[0, 1, 2], [1, 2, 2], [200, 9, 9], [0, 0, 0]]]], np.uint8), 4096),                # a mean of .5; two cells
              (np.array([[[[10, 10, 10], [20, 10, 10], [15, 10, 10]] * 2]], np.uint8)[:, :, :5], 4096),      # a pixel between two entries
              (frame_of_cells([(0, 0, 0), (9, 0, 0)], [1, 5])[None], 4096)]                                    # the median in the LAST coordinate
    streams = [(cases.lzw_cases()[name][0][0], cases.lzw_cases()[name][1]) for name in
               ("noise_fills_table", "next_512", "next_512_last", "next_1024", "next_4095", "bytes_510", "three_frames")]
    streams.append((rng.integers(0, 256, 700, dtype=np.uint8), 200))
    clean = [violations(f, seg, None) for f, seg in frames] + [stream_violations(s, seg, None) for s, seg in streams]
    assert not any(clean), clean
    found = [violations(f, seg, defect) for f, seg in frames] + [stream_violations(s, seg, defect) for s, seg in streams]
    assert any(found), defect


# ---- the host program under sanitizers
def host_compiler():
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    return cxx


def probe_records():
    """[("H", cells, counts) | ("S", indices, last)]: every histogram and stream of the tests above, and 20 000 seeded ones."""
    rng = np.random.default_rng(41)
    out = []
    for W, H in ((250, 136), (21, 5)):
        for frame in test_frames(3, W, H, seed=W + 2 * H):
            c = gm.histogram(frame)
            out.append(("H", np.flatnonzero(c), c[np.flatnonzero(c)]))
    corners = [r << 10 | g << 5 | b for r in (0, 31) for g in (0, 31) for b in (0, 31)]
    out += [("H", np.array(corners), np.ones(8, np.int64)), ("H", np.array([77]), np.array([1 << 24])),
            ("H", np.array([0, 32767]), np.array([1 << 23, 1 << 23])), ("H", rng.permutation(32768)[:257], np.ones(257, np.int64)),
            ("H", np.arange(32768), np.full(32768, 512, np.int64)), ("H", np.arange(32768), rng.integers(0, 1024, 32768))]
    for name, (frames, seg) in cases.lzw_cases().items():
        for idx in frames:
            for at in range(0, len(idx), seg):
                if at == 0 or seg > 1:
                    out.append(("S", idx[at:at + seg], at + seg >= len(idx)))
    for i in range(20000):
        if i % 2:
            k = int(rng.integers(1, 24))
            if i % 6 == 1:                              # neighbours in a small cube: long runs of ties
                base = rng.integers(0, 28, 3)
                cells = np.unique(((base[0] + rng.integers(0, 4, k)) << 10) | ((base[1] + rng.integers(0, 4, k)) << 5) | (base[2] + rng.integers(0, 4, k)))
            else:
                cells = rng.permutation(32768)[:k]
            counts = rng.integers(1, 4, len(cells)) if i % 4 == 1 else rng.integers(1, 1 << int(rng.integers(1, 20)), len(cells))
            out.append(("H", cells, counts))
        else:
            n = int(rng.integers(1, 160))
            out.append(("S", rng.integers(0, (2, 4, 256)[i % 3], n).astype(np.uint8), bool(i % 4)))
    return out


def test_cut_and_encoder_under_sanitizers(tmp_path):
    """csrc/gif_palette.hpp and csrc/gif_lzw.hpp as a host program with -fsanitize=address,undefined: labels, ncolors, codes and bit
    counts equal the model's; the program checks its own invariants (tests/gif_probe.cpp)."""
    exe = str(tmp_path / "gif_probe")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "gif_probe.cpp"), "-o", exe], check=True)
    records = probe_records()
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for r in records:
            if r[0] == "H":
                pairs = np.stack([np.asarray(r[1], np.uint32), np.asarray(r[2], np.uint32)], axis=1)
                f.write(b"H" + struct.pack("<i", len(pairs)) + np.ascontiguousarray(pairs).tobytes())
            else:
                f.write(b"S" + struct.pack("<ii", len(r[1]), int(r[2])) + np.ascontiguousarray(r[1], np.uint8).tobytes())
    done = subprocess.run([exe, path], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    lines = done.stdout.splitlines()
    assert lines[-1] == f"records {len(records)}" and len(lines) == len(records) + 1
    filled = full = 0
    for r, line in zip(records, lines):
        if r[0] == "H":
            counts = np.zeros(32768, np.int64)
            counts[np.asarray(r[1])] = r[2]
            labels, ncolors, _ = gm.boxes(counts)
            assert line == f"boxes {ncolors} " + " ".join(str(int(labels[c])) for c in r[1]), (r[1][:8], line[:80])
            full += ncolors == 256
        else:
            s = gm.lzw_segment(r[1], r[2])
            assert line == f"codes {s['bits']} " + " ".join(str(c) for c, _ in s["codes"]), (len(r[1]), line[:80])
            filled += s["forced"] > 0
    assert filled >= 2 and full >= 4, (filled, full)


# ---- the host half, the flags, the binding
def test_writer_refusals_and_header_bytes(tmp_path):
    import torch
    from vface_amd import hip
    from vface_amd.scripts import gif
    for W, H in ((0, 5), (5, 0), (65536, 1), (1, 65536)):
        with pytest.raises(ValueError, match="1..65535"):
            gif.GIFWriter(str(tmp_path / "no.gif"), W, H)
    with pytest.raises(ValueError, match="2\\^24"):
        gif.GIFWriter(str(tmp_path / "no.gif"), 4097, 4096)
    with pytest.raises(ValueError, match="seg_pixels"):
        gif.GIFWriter(str(tmp_path / "no.gif"), 8, 8, seg_pixels=65536)
    with pytest.raises(ValueError, match="seg_pixels"):
        gif.GIFWriter(str(tmp_path / "no.gif"), 8, 8, seg_pixels=0)
    w = gif.GIFWriter(str(tmp_path / "empty.gif"), 21, 5)
    assert w.seg_pixels == hip.GIF_SEG_PIXELS
    frame = test_frames(1, 21, 5, seed=1)
    with pytest.raises(hip.VFaceHipError, match="GPU"):
        w.write(torch.from_numpy(frame))
    with pytest.raises(hip.VFaceHipError, match="GPU"):
        w.write("frames")
    w.close()
    w.close()
    with pytest.raises(ValueError, match="closed"):
        w.write(torch.from_numpy(frame))
    assert (tmp_path / "empty.gif").read_bytes() == gm.header(21, 5) + b"\x3B" == gif.gif_header(21, 5) + gif.TRAILER
    assert gif.frame_header(21, 5) == gm.frame_header(21, 5) and gif.DELAY_CS == gm.DELAY_CS == 10

    class Stub(gif.GIFWriter):              # the device's half replaced by the model's: what write() and close() add around it
        def encode(self, frames_u8):
            qs = [gm.quantise(f) for f in frames_u8.numpy()]
            return [q["palette"].tobytes() for q in qs], [gm.image_data(q["indices"], self.seg_pixels) for q in qs]

    with Stub(str(tmp_path / "one.gif"), 21, 5, seg_pixels=64) as s:
        assert s.write(torch.from_numpy(frame)) == 1 and s.frames == 1
    data = (tmp_path / "one.gif").read_bytes()
    assert data == gm.gif_file(frame, 64)[0]
    im = Image.open(io.BytesIO(data))
    assert im.size == (21, 5) and getattr(im, "n_frames", 1) == 1 and im.info["duration"] == 100 and im.info["loop"] == 0


def test_flags():
    from vface_amd.scripts import VFace_inference_batch as cli
    opt = cli.build_parser().parse_args([])
    assert opt.gif_out is None and opt.gif_seg_pixels is None
    cli.check_gif_out_options(opt)
    opt = cli.build_parser().parse_args(["--gif_out", "a.gif", "--gif_seg_pixels", "2048"])
    assert (opt.gif_out, opt.gif_seg_pixels) == ("a.gif", 2048)
    opt.synthetic = False
    cli.check_gif_out_options(opt)
    with pytest.raises(SystemExit, match="needs --gif_out"):
        cli.check_gif_out_options(cli.build_parser().parse_args(["--gif_seg_pixels", "2048"]))
    for n in ("0", "65536"):
        with pytest.raises(SystemExit, match="1..65535"):
            cli.check_gif_out_options(cli.build_parser().parse_args(["--gif_out", "a.gif", "--gif_seg_pixels", n]))
    with pytest.raises(SystemExit, match="--synthetic writes no clip"):
        cli.check_options(cli.normalise_options(cli.build_parser().parse_args(["--synthetic", "--gif_out", "a.gif"])))


def test_binding():
    import torch
    from vface_amd import hip
    lib = hip.load()
    for name in ("vface_gif_histogram", "vface_gif_boxes", "vface_gif_palette", "vface_gif_map", "vface_gif_lzw", "vface_gif_lzw_bound",
                 "vface_gif_lzw_workspace_bytes"):
        assert hasattr(lib, name)
    for npix, seg in ((1, 1), (1, 4096), (300, 1), (300, 7), (34000, 4096), (4096, 4096), (12000, 12001), (1920 * 1080, 4096), (1 << 24, 65535),
                      (3839, 3839), (3840, 3840), (7678, 7678)):
        assert hip.gif_lzw_bound(npix, seg) == gm.lzw_bound(npix, seg), (npix, seg)
    for npix, seg in ((0, 1), (1, 0), (1, 65536), ((1 << 24) + 1, 4096)):
        assert lib.vface_gif_lzw_bound(npix, seg) == 0 and lib.vface_gif_lzw_workspace_bytes(npix, 1, seg) == 0
        with pytest.raises(hip.VFaceHipError):
            hip.gif_lzw_bound(npix, seg)
    assert lib.vface_gif_lzw_workspace_bytes(300, 0, 7) == 0 and lib.vface_gif_lzw_workspace_bytes(300, 2, 7) > 2 * 300 * 2
    # the worst case of every segment length fits the bound: noise, whose every code is one index long at first
    for seg in (1, 2, 300, 4000, 12001):
        idx = np.random.default_rng(seg).integers(0, 256, 12000, dtype=np.uint8)
        assert len(gm.image_data(idx, seg)) <= gm.lzw_bound(12000, seg)
    frames = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    for call in (lambda: hip.gif_histogram(frames), lambda: hip.gif_boxes(torch.zeros((1, 32768), dtype=torch.int32)),
                 lambda: hip.gif_palette(frames, None), lambda: hip.gif_map(frames, None, None),
                 lambda: hip.gif_lzw(torch.zeros((1, 16), dtype=torch.uint8))):
        with pytest.raises(hip.VFaceHipError, match="GPU"):
            call()
