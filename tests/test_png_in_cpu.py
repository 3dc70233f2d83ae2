"""The PNG decoder without a GPU: the format of tests/png_inflate_model.py held to zlib and Pillow, the constructed streams of
tests/png_in_cases.py, one stream per status, 20 000 seeded mutations, csrc/png_inflate.hpp's serial routine as a host program under
sanitizers against the model, seeded defects of the model that must be seen, the host half of vface_amd/scripts/png_in.py (the
chunk parser and its refusals, the folder reader, ``ClipInputs.from_png_folder``), the flag and the binding."""
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import png_in_cases as cases
import png_inflate_model as im
import png_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vface_amd", "csrc")
SIZES = ((1, 1), (2, 1), (1, 2), (3, 5), (21, 5), (85, 2), (86, 2), (250, 136))      # (W, H): those of the PNG-out tests
EXPECT = 784                                                                             # a 16 x 16 RGB file's filtered bytes
MUTATIONS = 20000


def host_compiler():
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    return cxx


def raw_inflate(body):
    d = zlib.decompressobj(-15)
    out = d.decompress(bytes(body))
    assert d.eof
    return out, len(body) - len(d.unused_data)


# ---- the model against zlib
@pytest.mark.parametrize("name", sorted(cases.zlib_streams()))
def test_model_inflates_what_zlib_wrote(name):
    body, data = cases.zlib_streams()[name]
    if name == "level0_stored_past_65535":
        assert len(data) > 65535 and body[0] & 6 == 0
    assert im.inflate(body, len(data)) == (0, len(data), len(body), data)


def test_model_inflates_the_encoders_bodies():
    """The bodies tests/png_model.py writes (what --png_encoder gpu writes): stripes of dynamic blocks closed by empty stored blocks."""
    for name, frames in pm.patterns(1, 21, 5, seed=1).items():
        rows = pm.filter_rows(frames[0])
        for stripe_rows in (1, 2, 16):
            body = pm.deflate_rows(rows, stripe_rows)["body"]
            assert im.inflate(body, rows.size) == (0, rows.size, len(body), rows.tobytes()), (name, stripe_rows)


@pytest.mark.parametrize("name", sorted(cases.constructed()))
def test_constructed_streams(name):
    """Each corner of the format: zlib, which knows nothing of the model, and the model agree byte for byte."""
    body = cases.constructed()[name]
    want, used = raw_inflate(body)
    assert im.inflate(body, len(want)) == (0, len(want), used, want), name
    if name == "bytes_after_the_final_block":
        assert used == len(body) - 4
    if name == "distance_32768":
        assert len(want) > 32768 + 258


def test_every_status_has_its_stream():
    """One constructed stream per status 1..14 yields exactly that status, none goes unseen, and zlib refuses each of them."""
    streams = cases.status_streams(EXPECT)
    assert sorted(streams) == list(range(1, 15))
    for want, body in streams.items():
        status, produced, consumed, data = im.inflate(body, EXPECT)
        assert status == want, (want, status)
        assert produced == len(data) <= EXPECT and consumed <= len(body)
        assert not cases.zlib_accepts(body, EXPECT)[0], want
    for name, (want, body) in cases.more_status_streams(EXPECT).items():
        assert im.inflate(body, EXPECT)[0] == want, name
        assert not cases.zlib_accepts(body, EXPECT)[0], name


def test_mutations_are_accepted_exactly_where_zlib_accepts():
    """20 000 valid bodies with one bit flipped, byte changed, tail cut or byte inserted: status 0 exactly when zlib reaches the end
    of the stream with ``expect`` bytes, and then the same bytes."""
    accepted, seen = 0, set()
    for body, expect in cases.mutations(MUTATIONS, 7):
        ok, want = cases.zlib_accepts(body, expect)
        status, produced, consumed, data = im.inflate(body, expect)
        assert (status == 0) == ok, (status, ok, body.hex())
        if ok:
            assert data == want
            accepted += 1
        seen.add(status)
    assert 1000 < accepted < MUTATIONS - 1000 and seen == set(range(15)), (accepted, sorted(seen))


# ---- the serial routine of csrc/png_inflate.hpp under sanitizers
def probe_records():
    records = [(body, len(raw_inflate(body)[0])) for body in cases.constructed().values()]
    records += [(body, len(data)) for body, data in cases.zlib_streams().values()]
    records += [(body, EXPECT) for body in cases.status_streams(EXPECT).values()]
    records += [(body, EXPECT) for _, body in cases.more_status_streams(EXPECT).values()]
    records += [(body, 16) for body in cases.status_streams(16).values()]
    records += [(cases.constructed()["ring_wrap"], 33000), (cases.constructed()["distance_32768"], 32768 + 100)]       # too long, mid-match
    return records + cases.mutations(MUTATIONS, 7)


def test_inflate_routine_under_sanitizers(tmp_path):
    """csrc/png_inflate.hpp as a host program with -fsanitize=address,undefined, every stream and output in a heap block of exactly
    its size: valid, constructed, refused and mutated streams give the model's status, produced, consumed and bytes."""
    exe = str(tmp_path / "png_inflate_probe")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "png_inflate_probe.cpp"), "-o", exe], check=True)
    records = probe_records()
    src, dst = str(tmp_path / "streams.bin"), str(tmp_path / "results.bin")
    with open(src, "wb") as f:
        for body, expect in records:
            f.write(struct.pack("<ii", len(body), expect) + body)
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert done.stdout.splitlines()[-1] == f"records {len(records)}"
    got, at = open(dst, "rb").read(), 0
    for k, (body, expect) in enumerate(records):
        status, produced, consumed = struct.unpack_from("<iii", got, at)
        data = got[at + 12:at + 12 + produced]
        at += 12 + produced
        assert (status, produced, consumed, data) == im.inflate(body, expect), (k, status, produced, consumed, body[:64].hex())
    assert at == len(got)


# ---- the filters
def test_each_filter_type_and_the_paeth_ties():
    """Rows where a, b and c differ, one row per type behind a seeded first row, per bpp; and the three Paeth ties by hand."""
    rng = np.random.default_rng(3)
    for bpp in (1, 3, 4):
        W, H = 7, 6
        rows = rng.integers(0, 256, (H, 1 + bpp * W), dtype=np.uint8)
        rows[:, 0] = [4, 0, 1, 2, 3, 4]
        status, rgb = im.unfilter(rows, W, H, bpp)
        assert status == 0
        mode = {1: "L", 3: "RGB", 4: "RGBA"}[bpp]
        data = cases.png_bytes(W, H, {1: 0, 3: 2, 4: 6}[bpp], rows.tobytes())
        with Image.open(io.BytesIO(data)) as pic:
            assert pic.mode == mode
            assert np.array_equal(np.asarray(pic.convert("RGB")), rgb), bpp
    # Paeth by the specification's own words on every (a, b, c) of a small cube, the true ties among them: b/c -> b, a/c -> a
    assert spec_paeth(2, 8, 4) == 8 and spec_paeth(8, 2, 4) == 8 and spec_paeth(1, 3, 2) == 2
    for a in range(13):
        for b in range(13):
            for c in range(13):
                status, rgb = im.unfilter(paeth_rows(a, b, c), 2, 2, 1)
                assert status == 0 and rgb[1, 0, 0] == a and rgb[1, 1, 0] == spec_paeth(a, b, c), (a, b, c)


def spec_paeth(a, b, c):
    """PNG specification 9.4, word for word."""
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    if pb <= pc:
        return b
    return c


def paeth_rows(a, b, c):
    """Grey, 2 x 2: row 0 (None) is (c, b); row 1 (Paeth) decodes to (a, paeth(a, b, c)): its first byte has 0 to the left and up
    left, so its predictor is c, and its second byte is 0."""
    return np.array([[0, c, b], [4, (a - c) & 255, 0]], np.uint8)


def test_a_filter_byte_above_4_is_refused_by_row():
    rows = np.zeros((5, 1 + 3 * 4), np.uint8)
    for bad in (0, 2, 4):
        r = rows.copy()
        r[bad, 0] = 5
        r[4, 0] = 5 if bad == 4 else 0
        status, rgb = im.unfilter(r, 4, 5, 3)
        assert status == 1 + bad and not rgb.any()


# ---- files: the parser and the model against Pillow
def decode_with_model(data, path="<png>"):
    from vface_amd.scripts import png_in
    f = png_in.parse_png(data, path)
    expect = (1 + f.bpp * f.W) * f.H
    status, produced, consumed, rows = im.inflate(f.body, expect)
    assert status == 0 and zlib.adler32(rows) == png_in.file_adler(f, consumed)
    status, rgb = im.unfilter(np.frombuffer(rows, np.uint8), f.W, f.H, f.bpp)
    assert status == 0
    return f, rgb


def pillow_rgb(data):
    with Image.open(io.BytesIO(data)) as pic:
        return np.asarray(pic.convert("RGB"))


TRNS = {2: struct.pack(">HHH", 10, 20, 30), 0: struct.pack(">H", 77)}


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("mode", ["RGB", "RGBA", "L"])
def test_files_decode_as_pillow_decodes_them(W, H, mode):
    """Pillow-written files of each type and size; with tRNS / gAMA (ignored, as convert("RGB") ignores them) and with the IDAT
    bytes cut into 1-byte and empty chunks and into 8 KiB chunks (the same body after parsing, the same pixels from Pillow)."""
    from vface_amd.scripts import png_in
    rng = np.random.default_rng(W * 1000 + H)
    channels = {"RGB": 3, "RGBA": 4, "L": 1}[mode]
    for kind in ("noise", "smooth"):
        frame = pm.patterns(1, W, H, seed=W + H)[kind][0]
        if mode == "RGBA":
            frame = np.concatenate([frame, rng.integers(0, 256, (H, W, 1), dtype=np.uint8)], axis=2)
        elif mode == "L":
            frame = np.ascontiguousarray(frame[:, :, 0])
        plain = cases.pillow_png(frame)
        f, rgb = decode_with_model(plain)
        assert (f.W, f.H, f.bpp) == (W, H, channels)
        assert np.array_equal(rgb, pillow_rgb(plain)), (mode, kind)
        assert np.array_equal(rgb, frame[:, :, :3] if channels > 1 else np.repeat(frame[:, :, None], 3, axis=2))
        extra = [(b"gAMA", struct.pack(">I", 45455))]
        if mode != "RGBA":
            extra.append((b"tRNS", TRNS[2 if mode == "RGB" else 0]))
        for split, chunks in ((None, extra), (0, ()), (8192, ()), (1, extra)):
            if split in (0, 1) and W * H > 1000 and kind == "noise":
                continue                                    # (100 000 one-byte chunks say nothing that 1 000 do not)
            data = cases.resplit(plain, split, chunks)
            g = png_in.parse_png(data)
            assert g == f, (mode, kind, split)
            assert np.array_equal(pillow_rgb(data), rgb), (mode, kind, split)


def test_pillow_accepts_bytes_behind_the_final_block():
    """The decoder accepts bytes of the body behind the final block's end and reads the checksum where the block ended; Pillow
    (libpng) accepts such a file too, which this pins.  Junk BETWEEN the final block and the checksum both refuse."""
    from vface_amd.scripts import png_in
    frame = pm.patterns(1, 21, 5, seed=2)["noise"][0]
    rows = pm.filter_rows(frame).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(rows) + c.flush()
    adler = struct.pack(">I", zlib.adler32(rows))
    for junk in (b"\x00", b"\x00\xFF\x13", b"\x00\xFF\x13\x77\x01\x02\x03"):
        data = cases.png_bytes(21, 5, 2, b"", stream=b"\x78\x9c" + body + adler + junk)
        assert np.array_equal(pillow_rgb(data), frame)
        f, rgb = decode_with_model(data)
        assert f.body == (body + adler + junk)[:-4] and np.array_equal(rgb, frame)
    data = cases.png_bytes(21, 5, 2, b"", stream=b"\x78\x9c" + body + b"\x00\xFF\x13" + adler)
    with pytest.raises(OSError):
        pillow_rgb(data)
    f = png_in.parse_png(data)
    status, produced, consumed, got = im.inflate(f.body, len(rows))
    assert (status, got, consumed) == (0, rows, len(body)) and png_in.file_adler(f, consumed) != zlib.adler32(got)


def test_the_encoders_files_decode_to_the_frames():
    """Encoder -> decoder is the identity: what tests/png_model.py (--png_encoder gpu) writes, the parser and the model read."""
    for name, frames in pm.patterns(1, 86, 18, seed=5).items():
        _, rgb = decode_with_model(pm.encode(frames[0], 16))
        assert np.array_equal(rgb, frames[0]), name


def refusal(data):
    from vface_amd.scripts import png_in
    with pytest.raises(SystemExit) as e:
        png_in.parse_png(data, "clip/7.png")
    assert str(e.value).startswith("clip/7.png: ")
    return str(e.value)


def test_parser_refusals_by_name():
    rows = bytes(1 + 3 * 2) * 2
    good = cases.png_bytes(2, 2, 2, rows)
    z = zlib.compress(rows)
    assert "no PNG signature" in refusal(b"\xFF\xD8\xFF\xE0" + good[4:])
    assert "palette" in refusal(cases.png_bytes(2, 2, 3, bytes(3) * 2))
    assert "grey + alpha" in refusal(cases.png_bytes(2, 2, 4, bytes(5) * 2))
    assert "16-bit" in refusal(cases.png_bytes(2, 2, 2, bytes(13) * 2, depth=16))
    assert "sub-byte" in refusal(cases.png_bytes(2, 2, 0, bytes(2) * 2, depth=4))
    assert "Adam7" in refusal(cases.png_bytes(2, 2, 2, rows, interlace=1))
    bad = bytearray(good)
    bad[len(good) - 12 - 4 - 3] ^= 1                             # a byte of the IDAT payload
    assert "bad CRC" in refusal(bytes(bad))
    assert "no IHDR" in refusal(good[:8] + good[8 + 25:])
    assert "no IHDR" in refusal(good[:8])
    assert "no IDAT" in refusal(good[:8 + 25] + cases.chunk(b"IEND", b""))
    assert "no IEND" in refusal(good[:-12])
    assert "truncated" in refusal(good[:-5])
    parts = good[:8 + 25] + cases.chunk(b"IDAT", z[:5]) + cases.chunk(b"tEXt", b"k\0v") + cases.chunk(b"IDAT", z[5:]) + cases.chunk(b"IEND", b"")
    assert "IDAT after another chunk" in refusal(parts)
    assert "critical chunk" in refusal(good[:8 + 25] + cases.chunk(b"ABCD", b"") + good[8 + 25:])

    def with_stream(s):
        return cases.png_bytes(2, 2, 2, b"", stream=s)
    assert "compression method 7" in refusal(with_stream(b"\x77" + z[1:]))
    assert "window size code 8" in refusal(with_stream(b"\x88\x1c" + z[2:]))
    assert "FCHECK" in refusal(with_stream(z[:1] + bytes([z[1] ^ 1]) + z[2:]))
    fdict = 0x20
    fdict |= 31 - (0x78 * 256 + fdict) % 31
    assert "FDICT" in refusal(with_stream(bytes([0x78, fdict]) + z[2:]))
    assert "shorter than its header" in refusal(with_stream(b"\x78\x9c\x00\x00\x00"))
    assert "an image of 0 x 2" in refusal(cases.png_bytes(0, 2, 2, rows))
    assert "wider than 8192 pixels" in refusal(cases.png_bytes(8193, 1, 0, bytes(8194)))
    # ancillary chunks are skipped wherever they stand, also behind the IDATs
    from vface_amd.scripts import png_in
    late = good[:-12] + cases.chunk(b"tIME", bytes(7)) + good[-12:]
    assert png_in.parse_png(late) == png_in.parse_png(good)


# ---- seeded defects
def defect_seen(defect):
    """True where some case tells the model with the defect from the model without it."""
    for name, body in cases.constructed().items():
        want = raw_inflate(body)[0]
        if im.inflate(body, len(want), defect)[::3] != (0, want):
            return True
    for body in cases.status_streams(EXPECT).values():
        if im.inflate(body, EXPECT, defect) != im.inflate(body, EXPECT):
            return True
    rng = np.random.default_rng(9)
    for bpp in (1, 3, 4):
        rows = rng.integers(0, 256, (6, 1 + bpp * 7), dtype=np.uint8)
        rows[:, 0] = [2, 0, 1, 2, 3, 4]
        if not np.array_equal(im.unfilter(rows, 7, 6, bpp, defect)[1], im.unfilter(rows, 7, 6, bpp)[1]):
            return True
    rows = paeth_rows(2, 8, 4)                                      # pb == pc < pa: the tie goes to b
    if not np.array_equal(im.unfilter(rows, 2, 2, 1, defect)[1], im.unfilter(rows, 2, 2, 1)[1]):
        return True
    return False


@pytest.mark.parametrize("defect", im.DEFECTS)
def test_seeded_defects_are_seen(defect):
    """Each one-line mistake of the model shows on some constructed stream, status stream or filter row."""
    assert defect_seen(defect), defect
    assert not defect_seen(None)


# ---- the folder reader, the clip form, the flag, the binding
def hip_max_w():
    from vface_amd import hip
    return hip.PNG_UNFILTER_MAX_W


def write_folder(root, frames, names=None):
    root.mkdir(exist_ok=True)
    for i, frame in enumerate(frames):
        Image.fromarray(frame).save(root / (names[i] if names else f"{i}.png"))
    return root


def test_folder_reader_and_frames(tmp_path):
    from vface_amd.scripts import clip_io, png_in
    frames = pm.patterns(4, 21, 5, seed=8)["noise"]
    folder = write_folder(tmp_path / "clip", frames, ["3.png", "5.png", "10.png", "11.png"])
    paths = [p for _, p in clip_io.list_frames(str(folder))]
    reader = png_in.PNGFolderReader(paths)
    assert (reader.W, reader.H, len(reader), reader.stage) == (21, 5, 4, "png_in")
    # the size comes from the first 33 bytes alone: a first file that is damaged further on opens, and is refused when it is read
    cut = tmp_path / "cut"
    cut.mkdir()
    (cut / "0.png").write_bytes(open(paths[0], "rb").read()[:60])
    opened = png_in.PNGFolderReader([str(cut / "0.png")])
    assert (opened.W, opened.H) == (21, 5)
    with pytest.raises(SystemExit, match=r"0\.png: truncated"):
        opened.read([0])
    (cut / "1.png").write_bytes(b"\xFF\xD8\xFF\xE0" + bytes(40))
    with pytest.raises(SystemExit, match=r"1\.png: no PNG signature and IHDR"):
        png_in.PNGFolderReader([str(cut / "1.png")])
    assert hip_max_w() == png_in.MAX_W
    got = reader.read([2, 0])
    assert isinstance(got, png_in.PNGFrames) and len(got) == 2 and got.paths == [paths[2], paths[0]]
    for record, frame in zip(got.records, (frames[2], frames[0])):
        rows = zlib.decompress(b"\x78\x9c" + record.body + struct.pack(">I", record.adler))
        assert np.array_equal(im.unfilter(np.frombuffer(rows, np.uint8), 21, 5, 3)[1], frame)
    # the rows of a tensor, as ClipInputs.batch uses them
    twin = got.clone()
    twin[0] = got[1]
    assert twin[0] is got[1] and got[0] is not got[1] and len(twin) == 2
    p = got.packed()
    host = p["buffer"].numpy()
    assert p["files"] == 2 and p["streams_at"] % 16 == 0
    assert host[:16].view(np.int64).tolist() == [0, len(got[0].body)]
    assert host[p["lengths_at"]:p["lengths_at"] + 8].view(np.int32).tolist() == [len(got[0].body), len(got[1].body)]
    assert host[p["streams_at"]:p["streams_at"] + p["stream_bytes"]].tobytes() == got[0].body + got[1].body
    # another size is refused from its header with the folder form's message; a .jpg by name
    Image.fromarray(frames[0][:, :20]).save(folder / "12.png")
    paths = [p for _, p in clip_io.list_frames(str(folder))]
    with pytest.raises(SystemExit, match=r"--target_frames: .*12\.png is 20 x 5, the clip's first frames are 21 x 5: the frames of a clip must all be one size"):
        png_in.PNGFolderReader(paths).read([4])
    Image.fromarray(frames[0]).save(folder / "13.jpg")
    with pytest.raises(SystemExit, match=r"--png_decoder gpu: .*13\.jpg is not a PNG file"):
        png_in.PNGFolderReader([p for _, p in clip_io.list_frames(str(folder))])


def test_clip_inputs_keeps_the_folders_frame_ids(tmp_path):
    """``ClipInputs.from_png_folder``: the folder's own frame ids, ``PNGFrames`` batches, and the crop-frame fallback of a frame
    without landmarks (it takes the parsed file of the frame before it, across a batch boundary too)."""
    from test_clip_io_cpu import square, template_landmarks
    from vface_amd.scripts import clip_io, png_in
    frames = pm.patterns(4, 64, 48, seed=2)["blocks"]
    folder = write_folder(tmp_path / "clip", frames, ["3.png", "5.png", "10.png", "11.png"])
    Image.fromarray(frames[0]).save(tmp_path / "src.png")
    lm = np.stack([template_landmarks(square(32, 24, 10 + i, 0.0)) for i in range(4)])
    lm[1] = np.nan
    lm[2] = np.nan
    np.savez(tmp_path / "lm.npz", frames=lm, source=template_landmarks(square(30, 20, 9, 0.1)))
    args = (str(folder), str(tmp_path / "src.png"), str(tmp_path / "lm.npz"), 4, 512, 512)
    clip, plain = clip_io.ClipInputs.from_png_folder(*args), clip_io.ClipInputs(*args)
    assert clip.frame_ids == plain.frame_ids == [3, 5, 10, 11] and clip.paths == plain.paths and clip.size == (48, 64)
    for k in (0, 1):
        b, want = clip.batch(k, 2), plain.batch(k, 2)
        assert isinstance(b["frames"], png_in.PNGFrames) and b["frame_ids"] == want["frame_ids"]
        assert b["frames"].paths == [plain.paths[2 * k], plain.paths[2 * k + 1]]
        assert np.array_equal(b["quads"], want["quads"]) and np.array_equal(b["landmarks"], want["landmarks"])
    assert clip.batch(0, 2)["crop_frames"].paths == [plain.paths[0], plain.paths[0]]
    assert clip.batch(1, 2)["crop_frames"].paths == [plain.paths[0], plain.paths[3]]
    assert clip.batch(1, 2)["frames"].paths == [plain.paths[2], plain.paths[3]]


def test_flag_and_its_refusals():
    from vface_amd.scripts import VFace_inference_batch as cli
    parser = cli.build_parser()
    assert parser.parse_args([]).png_decoder == "pillow"
    assert parser.parse_args(["--png_decoder", "gpu"]).png_decoder == "gpu"
    with pytest.raises(SystemExit):
        parser.parse_args(["--png_decoder", "zlib"])
    clip = ["--src_image", "s.png", "--landmarks", "l.npz", "--synthetic_weights", "--png_decoder", "gpu"]
    opt = cli.normalise_options(parser.parse_args(clip + ["--target_video", "clip.y4m"]))
    opt.synthetic = False
    with pytest.raises(SystemExit, match="--png_decoder gpu.*--target_video"):
        cli.check_options(opt)
    opt = cli.normalise_options(parser.parse_args(["--png_decoder", "gpu"]))
    opt.synthetic = True
    with pytest.raises(SystemExit, match="--png_decoder gpu.*--synthetic"):
        cli.check_options(opt)
    opt = cli.normalise_options(parser.parse_args(clip + ["--target_frames", "clip/"]))
    opt.synthetic = False
    cli.check_options(opt)                                   # the folder form takes it
    opt = cli.normalise_options(parser.parse_args([]))
    opt.synthetic = True
    cli.check_options(opt)                                   # and the default is nobody's business


def test_binding_and_refusals_without_a_gpu():
    """The two entry points are bound; the wrappers refuse host tensors before any call (there is no CPU fallback)."""
    import torch
    from vface_amd import hip
    lib = hip.load()
    assert lib.vface_png_inflate and lib.vface_png_unfilter and lib.vface_abi_version() == 8
    with pytest.raises(hip.VFaceHipError):
        hip.png_inflate(torch.zeros(8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 8)
    with pytest.raises(hip.VFaceHipError):
        hip.png_unfilter(torch.zeros((1, 14), dtype=torch.uint8), 2, 2, 3, torch.zeros(1, dtype=torch.int32))
    from vface_amd.scripts import png_in
    with pytest.raises(hip.VFaceHipError):
        png_in.decode(png_in.PNGFrames(1, 1, []), "cuda")
    with pytest.raises(hip.VFaceHipError):
        png_in.decode(png_in.PNGFrames(2, 2, [png_in.parse_png(cases.png_bytes(2, 2, 2, bytes(14)))]), "cpu")
