"""vface_png_inflate and vface_png_unfilter (csrc/png_in.hip) against the model (tests/png_inflate_model.py) bit for bit, inside
sentinel buffers; the decoder of vface_amd/scripts/png_in.py against Pillow and against the encoder of scripts/png.py; and the
real-clip run with --png_decoder gpu against the default.

Refused and mutated streams go to the device only because csrc/png_inflate.hpp's routine is green on them under sanitizers
(tests/test_png_in_cpu.py::test_inflate_routine_under_sanitizers), and every row buffer here is a view in a poisoned allocation."""
import functools
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_in_cases as cases
import png_inflate_model as im
import png_model as pm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL8 = 0xA5
ERR_ARG, ERR_SHAPE = -1, -3                                     # VFACE_ERR_* of include/vface_hip.h
# (W, H): the eight of the PNG-out tests; 640 x 200: rows of 1921 bytes, the frame crosses the 32 KiB ring eleven times; H = 65: one
# row past a band of 64; 130 x 129: two bands and a row, wider than the 64 steps of the skew
SIZES = ((1, 1), (2, 1), (1, 2), (3, 5), (21, 5), (85, 2), (86, 2), (250, 136), (640, 200), (7, 65), (130, 129))
COLOUR = {1: 0, 3: 2, 4: 6}


def poisoned(n, dtype=torch.uint8, lead=37, tail=64):
    """A view of n elements inside an allocation filled with the sentinel -> (view, whole)."""
    fill = SENTINEL8 if dtype == torch.uint8 else -7
    whole = torch.full((lead + n + tail,), fill, dtype=dtype, device=DEV)
    return whole[lead:lead + n], whole


def frame_clean(whole, n, lead=37):
    host = whole.cpu().numpy()
    fill = SENTINEL8 if host.dtype == np.uint8 else -7
    return bool((host[:lead] == fill).all() and (host[lead + n:] == fill).all())


def device_inflate(bodies, expect, stride=None, stream_pad=0):
    """vface_png_inflate on ``bodies`` through the raw entry point, every buffer a view in a poisoned allocation -> dict.  ``rows``
    is prefilled with the sentinel, so bytes that were not written still hold it."""
    from vface_amd import hip
    F = len(bodies)
    stride = expect + 11 if stride is None else stride
    lengths = np.array([len(b) for b in bodies], np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.int64)]).astype(np.int64)
    total = max(int(lengths.sum()), 1) + stream_pad
    streams, streams_whole = poisoned(total)
    joined = np.frombuffer(b"".join(bodies), np.uint8)
    streams[:len(joined)] = torch.from_numpy(joined.copy()).to(DEV)
    rows, rows_whole = poisoned(F * stride)
    meta, meta_whole = poisoned(5 * F, torch.int32)
    d_off, d_len = torch.from_numpy(offsets).to(DEV), torch.from_numpy(lengths).to(DEV)
    lib = hip.load()
    rc = lib.vface_png_inflate(streams.data_ptr(), total, d_off.data_ptr(), d_len.data_ptr(), F, rows.data_ptr(), stride, expect,
                               meta.data_ptr(), meta[F:].data_ptr(), meta[2 * F:].data_ptr(), meta[3 * F:].data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    m = meta.cpu().numpy()
    return {"status": m[:F].tolist(), "produced": m[F:2 * F].tolist(), "consumed": m[2 * F:3 * F].tolist(),
            "adler": m[3 * F:].reshape(F, 2).tolist(), "rows": rows.view(F, stride).cpu().numpy(), "d_rows": rows.view(F, stride),
            "d_status": meta[:F], "stride": stride,
            "clean": frame_clean(streams_whole, total) and frame_clean(rows_whole, F * stride) and frame_clean(meta_whole, 5 * F)}


def assert_inflated(got, wants, what):
    """``wants``: per file the model's (status, produced, consumed, bytes).  The produced bytes equal the model's, every byte behind
    them still holds the sentinel, the Adler halves are those of the produced bytes, and nothing outside the views was touched."""
    for f, (status, produced, consumed, data) in enumerate(wants):
        assert (got["status"][f], got["produced"][f], got["consumed"][f]) == (status, produced, consumed), (what, f)
        row = got["rows"][f]
        assert row[:produced].tobytes() == data, (what, f)
        assert (row[produced:] == SENTINEL8).all(), (what, f, "bytes behind produced were written")
        assert tuple(got["adler"][f]) == im.adler_halves(data), (what, f)
    assert got["clean"], what


def device_unfilter(d_rows, stride, W, H, bpp, d_status):
    from vface_amd import hip
    F = d_rows.shape[0]
    rgb, rgb_whole = poisoned(F * H * W * 3)
    status, status_whole = poisoned(F, torch.int32)
    rc = hip.load().vface_png_unfilter(d_rows.data_ptr(), stride, W, H, bpp, F, d_status.data_ptr(), rgb.data_ptr(), status.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return (rgb.view(F, H, W, 3).cpu().numpy(), status.cpu().tolist(),
            frame_clean(rgb_whole, F * H * W * 3) and frame_clean(status_whole, F))


@functools.lru_cache(maxsize=None)
def written_files(W, H, bpp):
    """Three Pillow-written files of one size with streams of different lengths (noise, smooth, flat; a tiny size may give two alike) -> [(file, rows, rgb)], the
    references from zlib and Pillow, which the model equals (tests/test_png_in_cpu.py); on small sizes the model is asked as well."""
    from vface_amd.scripts import png_in
    rng = np.random.default_rng(W * 31 + H)
    out = []
    for kind in ("noise", "smooth", "flat"):
        frame = pm.patterns(1, W, H, seed=W + 3 * H)[kind][0]
        if bpp == 4:
            frame = np.concatenate([frame, rng.integers(0, 256, (H, W, 1), dtype=np.uint8)], axis=2)
        elif bpp == 1:
            frame = np.ascontiguousarray(frame[:, :, 1])
        data = cases.pillow_png(frame)
        f = png_in.parse_png(data)
        rows = zlib.decompress(b"\x78\x9c" + f.body + f.adler.to_bytes(4, "big"))
        with Image.open(io.BytesIO(data)) as pic:
            rgb = np.asarray(pic.convert("RGB")).copy()
        if W * H <= 3000:
            assert im.inflate(f.body, len(rows)) == (0, len(rows), len(f.body), rows)
            assert np.array_equal(im.unfilter(np.frombuffer(rows, np.uint8), W, H, bpp)[1], rgb)
        out.append((f, rows, rgb))
    return out


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("bpp", [3, 4, 1])
def test_both_entry_points_equal_the_model(W, H, bpp):
    """Three files of different stream lengths in one call: rows, byte counts and Adler halves from the inflate, pixels from the
    unfilter, nothing written outside either."""
    files = written_files(W, H, bpp)
    assert all(f.bpp == bpp for f, _, _ in files) and (W * H < 100 or len({len(f.body) for f, _, _ in files}) >= 2)
    expect = (1 + bpp * W) * H
    got = device_inflate([f.body for f, _, _ in files], expect)
    assert_inflated(got, [(0, expect, len(f.body), rows) for f, rows, _ in files], f"{W}x{H} bpp {bpp}")
    rgb, status, clean = device_unfilter(got["d_rows"], got["stride"], W, H, bpp, got["d_status"])
    assert status == [0, 0, 0] and clean
    for k, (_, _, want) in enumerate(files):
        bad = np.argwhere(rgb[k] != want)
        assert bad.size == 0, (f"{W}x{H} bpp {bpp} file {k}: {len(bad)} bytes differ, first at (row, x, channel) {tuple(bad[0])}: "
                               f"got {rgb[k][tuple(bad[0])]}, want {want[tuple(bad[0])]}")


@functools.lru_cache(maxsize=None)
def constructed_reference(name):
    body = cases.constructed()[name]
    expect = len(zlib.decompressobj(-15).decompress(body))
    return body, expect, im.inflate(body, expect)


@pytest.mark.parametrize("name", sorted(n for n in cases.constructed() if n != "only_end_of_block"))        # (that one makes 0 bytes)
def test_constructed_streams(name):
    body, expect, want = constructed_reference(name)
    assert want[0] == 0
    assert_inflated(device_inflate([body], expect), [want], name)


def test_a_token_that_would_pass_expect_is_not_written():
    """The ring-wrap and far-distance streams with ``expect`` inside one of their matches: status 13, and the row ends before it."""
    for name, expect in (("ring_wrap", 33000), ("distance_32768", 32768 + 100)):
        body = cases.constructed()[name]
        want = im.inflate(body, expect)
        assert want[0] == 13 and want[1] < expect
        assert_inflated(device_inflate([body], expect), [want], name)


@functools.lru_cache(maxsize=None)
def small_files():
    """512 bodies for 16 x 16 RGB files (784 filtered bytes): valid ones, one stream per status 1..14, further refused streams, and
    seeded mutations of the valid ones -> (bodies, the model's results, W, H)."""
    from vface_amd.scripts import png_in
    W = H = 16
    expect = (1 + 3 * W) * H
    valid = []
    for kind, frames in pm.patterns(4, W, H, seed=16).items():
        for k, frame in enumerate(frames):
            valid.append(png_in.parse_png(cases.pillow_png(frame) if k % 2 else pm.encode(frame, 4 + k)).body)
    refused = list(cases.status_streams(expect).values()) + [b for _, b in cases.more_status_streams(expect).values()]
    rng = np.random.default_rng(33)
    bodies = valid + refused
    while len(bodies) < 512:
        b = bytearray(valid[len(bodies) % len(valid)])
        kind, at = len(bodies) % 4, int(rng.integers(0, len(b)))
        if kind == 0:
            b[at] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            b[at] = int(rng.integers(0, 256))
        elif kind == 2:
            del b[at:]
        else:
            b.insert(at, int(rng.integers(0, 256)))
        bodies.append(bytes(b))
    return bodies, [im.inflate(b, expect) for b in bodies], W, H


def test_512_files_in_one_call_every_status_among_them():
    """Each file has the model's status, produced and consumed, its row holds the model's bytes and nothing behind them; the
    unfilter skips and clears every file the inflate flagged and decodes the others."""
    bodies, wants, W, H = small_files()
    assert len(bodies) == 512 and {w[0] for w in wants} >= set(range(15))
    expect = (1 + 3 * W) * H
    got = device_inflate(bodies, expect)
    assert_inflated(got, wants, "512 files")
    rgb, status, clean = device_unfilter(got["d_rows"], got["stride"], W, H, 3, got["d_status"])
    assert clean
    decoded = 0
    for f, (st, _, _, data) in enumerate(wants):
        if st != 0:
            assert status[f] == 0 and not rgb[f].any(), f                  # not read, cleared
            continue
        want_status, want = im.unfilter(np.frombuffer(data, np.uint8), W, H, 3)
        assert status[f] == want_status and np.array_equal(rgb[f], want), f
        decoded += 1
    assert decoded >= 20


def test_more_files_than_the_grid_holds_and_ranges_outside_the_buffer():
    """1030 files of 5 x 1 (past PNG_INFLATE_GRID_CAP workgroups), and offsets / lengths that do not lie inside the stream buffer:
    status 1, nothing read or written for them."""
    from vface_amd import hip
    assert 1030 > hip.PNG_INFLATE_GRID_CAP
    expect = 16
    pool = list(cases.status_streams(expect).values()) + [cases.fixed_block(cases.BitWriter(), cases.run_tokens(16, 2)).bytes(),
                                                          cases.stored_block(cases.BitWriter(), bytes(range(1, 17))).bytes()]
    bodies = [pool[i % len(pool)] for i in range(1030)]
    wants = [im.inflate(b, expect) for b in pool]
    got = device_inflate(bodies, expect)
    assert_inflated(got, [wants[i % len(pool)] for i in range(1030)], "1030 files")
    rgb, status, clean = device_unfilter(got["d_rows"], got["stride"], 5, 1, 3, got["d_status"])
    assert clean
    for i in range(1030):
        st, _, _, data = wants[i % len(pool)]
        want_status, want = im.unfilter(np.frombuffer(data, np.uint8), 5, 1, 3) if st == 0 else (0, np.zeros((1, 5, 3), np.uint8))
        assert status[i] == want_status and np.array_equal(rgb[i], want), i
    # ranges outside the buffer
    lib, s = hip.load(), torch.cuda.current_stream().cuda_stream
    good = pool[-1]
    streams = torch.from_numpy(np.frombuffer(good, np.uint8).copy()).to(DEV)
    n = len(good)
    offsets = torch.tensor([0, 1, n, -1, 0, 1 << 40], dtype=torch.int64, device=DEV)
    lengths = torch.tensor([n, n, 1, 4, -1, 2], dtype=torch.int32, device=DEV)
    rows, rows_whole = poisoned(6 * 16)
    meta = torch.full((5 * 6,), -7, dtype=torch.int32, device=DEV)
    assert lib.vface_png_inflate(streams.data_ptr(), n, offsets.data_ptr(), lengths.data_ptr(), 6, rows.data_ptr(), 16, 16, meta.data_ptr(),
                                 meta[6:].data_ptr(), meta[12:].data_ptr(), meta[18:].data_ptr(), s) == 0
    torch.cuda.synchronize()
    m = meta.cpu().tolist()
    assert m[:6] == [0, 1, 1, 1, 1, 1] and m[6:12] == [16, 0, 0, 0, 0, 0] and m[12:18] == [n, 0, 0, 0, 0, 0]
    host = rows.cpu().numpy()
    assert host[:16].tolist() == list(range(1, 17)) and (host[16:] == SENTINEL8).all() and frame_clean(rows_whole, 96)


def test_a_filter_byte_of_5_is_refused_by_row():
    """In row 0, in the last row and in the first row of the second band; the file beside them decodes."""
    W, H, bpp = 5, 130, 3
    rng = np.random.default_rng(4)
    rows = rng.integers(0, 256, (4, H, 1 + bpp * W), dtype=np.uint8)
    rows[:, :, 0] = rng.integers(0, 5, (4, H))
    rows[1, 0, 0] = 5
    rows[2, H - 1, 0] = 5
    rows[3, 64, 0] = 5
    rows[3, 100, 0] = 200
    d_rows = torch.from_numpy(rows.reshape(4, -1)).to(DEV)
    rgb, status, clean = device_unfilter(d_rows, d_rows.shape[1], W, H, bpp, torch.zeros(4, dtype=torch.int32, device=DEV))
    assert status == [0, 1, H, 65] and clean
    assert np.array_equal(rgb[0], im.unfilter(rows[0], W, H, bpp)[1]) and not rgb[1:].any()


def test_refusals_by_code():
    from vface_amd import hip
    lib, s = hip.load(), torch.cuda.current_stream().cuda_stream
    t = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = t.data_ptr()
    ok = (p, 64, p, p, 1, p, 100, 100, p, p, p, p, s)                # (refused before any launch: the pointers are never followed)
    for at in (0, 2, 3, 5, 8, 9, 10, 11):
        assert lib.vface_png_inflate(*(0 if i == at else v for i, v in enumerate(ok))) == ERR_ARG, at
    assert lib.vface_png_inflate(p, 64, p, p, 0, p, 100, 100, p, p, p, p, s) == ERR_ARG
    assert lib.vface_png_inflate(p, 0, p, p, 1, p, 100, 100, p, p, p, p, s) == ERR_ARG
    assert lib.vface_png_inflate(p, 64, p, p, 1, p, 100, 0, p, p, p, p, s) == ERR_ARG
    assert lib.vface_png_inflate(p, 1 << 31, p, p, 1, p, 100, 100, p, p, p, p, s) == ERR_SHAPE
    assert lib.vface_png_inflate(p, 64, p, p, 1, p, 1 << 31, 1 << 31, p, p, p, p, s) == ERR_SHAPE
    assert lib.vface_png_inflate(p, 64, p, p, 1, p, 99, 100, p, p, p, p, s) == ERR_SHAPE
    ok = (p, 14, 2, 2, 3, 1, p, p, p, s)
    for at in (0, 6, 7, 8):
        assert lib.vface_png_unfilter(*(0 if i == at else v for i, v in enumerate(ok))) == ERR_ARG, at
    for at in (2, 3, 5):
        assert lib.vface_png_unfilter(*(0 if i == at else v for i, v in enumerate(ok))) == ERR_ARG, at
    for bpp in (0, 2, 5):
        assert lib.vface_png_unfilter(p, 100, 2, 2, bpp, 1, p, p, p, s) == ERR_SHAPE
    assert lib.vface_png_unfilter(p, 13, 2, 2, 3, 1, p, p, p, s) == ERR_SHAPE                          # file_stride below (1 + 3 W) H
    assert lib.vface_png_unfilter(p, 1 << 40, 1 << 20, 1 << 10, 3, 1, p, p, p, s) == ERR_SHAPE        # (1 + 3 W) H >= 2^31
    assert lib.vface_png_unfilter(p, 1 << 20, hip.PNG_UNFILTER_MAX_W + 1, 1, 3, 1, p, p, p, s) == ERR_SHAPE
    # the wrappers
    u8 = torch.zeros((1, 14), dtype=torch.uint8, device=DEV)
    i32 = torch.zeros(1, dtype=torch.int32, device=DEV)
    i64 = torch.zeros(1, dtype=torch.int64, device=DEV)
    for bad in ((u8[0].cpu(), i64, i32, 14), (u8[0], i32, i32, 14), (u8[0], i64, i32, 0), (u8[0], i64, i32.repeat(2), 14)):
        with pytest.raises(hip.VFaceHipError):
            hip.png_inflate(*bad)
    for bad in ((u8, 2, 2, 2, i32), (u8, 3, 2, 3, i32), (u8.cpu(), 2, 2, 3, i32), (u8, 2, 2, 3, i64)):
        with pytest.raises(hip.VFaceHipError):
            hip.png_unfilter(*bad)


# ---- the decoder of scripts/png_in.py
@pytest.mark.parametrize("W,H,stripe_rows", [(250, 136, None), (21, 5, 2)])
def test_encoder_then_decoder_is_the_identity(W, H, stripe_rows):
    """``png.PNGEncoder``'s own files, parsed and decoded on the device, are the frames that went in."""
    from vface_amd.scripts import png, png_in
    rgb = np.concatenate([pm.patterns(1, W, H, seed=9)[k] for k in ("smooth", "noise", "blocks")])
    frames = torch.from_numpy(rgb).to(DEV)
    enc = png.PNGEncoder(W, H) if stripe_rows is None else png.PNGEncoder(W, H, stripe_rows=stripe_rows)
    files = enc.encode(frames)
    back = png_in.decode(png_in.PNGFrames(W, H, [png_in.parse_png(d, f"<{k}>") for k, d in enumerate(files)]), DEV)
    assert back.dtype == torch.uint8 and back.is_cuda and torch.equal(back, frames)


def test_decode_mixes_types_and_names_what_does_not_decode():
    from vface_amd import hip
    from vface_amd.scripts import png_in
    W, H = 21, 5
    files = [written_files(W, H, bpp)[k] for bpp, k in ((3, 0), (1, 1), (4, 0), (3, 1))]
    got = png_in.decode(png_in.PNGFrames(W, H, [f for f, _, _ in files]), DEV).cpu().numpy()
    for k, (_, _, want) in enumerate(files):
        assert np.array_equal(got[k], want), k
    good = files[0][0]
    with pytest.raises(SystemExit, match=r"clip/9\.png: does not decode: .*\(status \d+"):
        png_in.decode(png_in.PNGFrames(W, H, [good, good._replace(path="clip/9.png", body=good.body[:-3])]), DEV)
    with pytest.raises(SystemExit, match=r"clip/9\.png: does not decode: the Adler-32"):
        png_in.decode(png_in.PNGFrames(W, H, [good._replace(path="clip/9.png", adler=good.adler ^ 1)]), DEV)
    rows = bytearray(files[0][1])
    rows[3 * (1 + 3 * W)] = 7
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    bad = good._replace(path="clip/9.png", body=c.compress(bytes(rows)) + c.flush(), adler=zlib.adler32(bytes(rows)))
    with pytest.raises(SystemExit, match=r"clip/9\.png: does not decode: row 3 has a filter type above 4"):
        png_in.decode(png_in.PNGFrames(W, H, [good, bad]), DEV)
    with pytest.raises(hip.VFaceHipError):
        png_in.decode(png_in.PNGFrames(W, H, [good, written_files(3, 5, 3)[0][0]]), DEV)


def test_a_1080p_noisy_frame_against_pillow(tmp_path):
    from vface_amd.scripts import clip_io, png_in
    frame = pm.content("noisy", 1920, 1080, seed=1)
    path = tmp_path / "0.png"
    Image.fromarray(frame).save(path)
    reader = png_in.PNGFolderReader([str(path)])
    got = reader.to_rgb(reader.read([0]), DEV)
    assert tuple(got.shape) == (1, 1080, 1920, 3) and torch.equal(got[0].cpu(), clip_io.load_image(str(path)))
    assert np.array_equal(got[0].cpu().numpy(), frame)


# ---- end to end
@pytest.fixture(scope="module")
def clip_runs(tmp_path_factory):
    """The small seeded clip of tests/test_png_gpu.py's run test (4 frames of 320 x 240, 2 per batch), its folder holding RGB and RGBA
    files under indices of the folder's own (2, 5, 8, ..); read by Pillow and by the device."""
    import yaml
    from test_clip_io_cpu import square, template_landmarks
    from test_clip_run_gpu import FH, FW, N, small_cfg
    from vface_amd.scripts import VFace_inference_batch as cli
    root = tmp_path_factory.mktemp("png_in")
    rng = np.random.default_rng(11)
    (root / "frames").mkdir()
    ids = [2 + 3 * i for i in range(N)]
    for i, frame in zip(ids, rng.integers(0, 256, (N, FH, FW, 3), dtype=np.uint8)):
        if i % 2:
            frame = np.concatenate([frame, rng.integers(0, 256, (FH, FW, 1), dtype=np.uint8)], axis=2)        # RGBA: alpha is dropped
        Image.fromarray(frame).save(root / "frames" / f"{i}.png")
    Image.fromarray(rng.integers(0, 256, (180, 200, 3), dtype=np.uint8)).save(root / "src.png")
    quads = np.stack([square(160 + 4 * i, 120 - 3 * i, 60 + 2 * i, 0.06 * i) for i in range(N)])
    np.savez(root / "lm.npz", frames=np.stack([template_landmarks(q) for q in quads]), source=template_landmarks(square(100, 90, 50, -0.1)),
             crops=rng.integers(100, 412, (N, 68, 2)).astype(np.float64), source_crop=rng.integers(100, 412, (68, 2)).astype(np.float64))
    (root / "small.yaml").write_text(yaml.safe_dump({"model": {"params": {"unet_config": {"params": small_cfg()}}}}))

    def run(tag, extra):
        args = ["--target_frames", str(root / "frames"), "--src_image", str(root / "src.png"), "--landmarks", str(root / "lm.npz"),
                "--synthetic_weights", "--config", str(root / "small.yaml"), "--H", "512", "--W", "512", "--max_steps", "1",
                "--ddim_steps", "50", "--n_frames", str(N), "--n_samples", "2", "--skip_save", "--Base_dir", str(root / tag), *extra]
        opt = cli.build_parser().parse_args(args)
        opt.return_samples = True
        torch.manual_seed(opt.seed)
        return cli.run_clip(opt)["batches"]

    return {"ids": ids, "gpu": run("g", ["--png_decoder", "gpu"]), "pillow": run("p", [])}


def test_clip_run_pastes_the_same_frames_either_way(clip_runs):
    ours = torch.cat([x["pasted_frames"] for x in clip_runs["gpu"]])
    theirs = torch.cat([x["pasted_frames"] for x in clip_runs["pillow"]])
    assert torch.equal(ours, theirs)
    assert [i for x in clip_runs["gpu"] for i in x["frame_ids"]] == clip_runs["ids"] == [i for x in clip_runs["pillow"] for i in x["frame_ids"]]


def test_png_in_is_timed_for_the_gpu_decoder_only(clip_runs):
    for x, y in zip(clip_runs["gpu"], clip_runs["pillow"]):
        assert x["stage_seconds"]["png_in"] > 0 and "png_in" not in y["stage_seconds"]
        assert set(x["stage_seconds"]) - set(y["stage_seconds"]) == {"png_in"} and set(x) == set(y)
