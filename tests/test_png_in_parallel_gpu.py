"""vface_png_inflate_parallel (csrc/png_in_par.hip) against the model (tests/png_inflate_par_model.py) and against vface_png_inflate
on the same inputs, bit for bit -- rows, status, produced, consumed, adler and info -- inside sentinel buffers; ``png_in.decode`` with
``inflate="parallel"`` against the serial path and Pillow; and the real-clip run with --png_in_inflate parallel against the default.

Refused and mutated streams go to the device only because csrc/png_inflate_par.hpp's routine is green on them under sanitizers
(tests/test_png_in_parallel_cpu.py::test_parallel_routine_under_sanitizers), and every buffer here is a view in a poisoned allocation."""
import functools
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_in_cases as cases
import png_inflate_par_cases as pc
import png_inflate_par_model as pmod
import png_model as pm
from test_png_in_gpu import DEV, SENTINEL8, device_inflate, frame_clean, poisoned, small_files

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_ALIGN, ERR_SHAPE = -1, -2, -3                      # VFACE_ERR_* of include/vface_hip.h
COLOUR = {1: 0, 3: 2, 4: 6}


def device_parallel(bodies, expect, chunk_bytes, stride=None, offsets=None, lengths=None):
    """vface_png_inflate_parallel through the raw entry point, every buffer -- the workspace of exactly the stated bytes too -- a view
    in a poisoned allocation -> dict.  ``rows`` is prefilled with the sentinel, so bytes that were not written still hold it."""
    from vface_amd import hip
    F = len(bodies)
    stride = expect + 11 if stride is None else stride
    if lengths is None:
        lengths = np.array([len(b) for b in bodies], np.int32)
        offsets = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.int64)]).astype(np.int64)
    joined = np.frombuffer(b"".join(bodies), np.uint8)
    total = max(len(joined), 1)
    streams, streams_whole = poisoned(total)
    streams[:len(joined)] = torch.from_numpy(joined.copy()).to(DEV)
    rows, rows_whole = poisoned(F * stride)
    meta, meta_whole = poisoned(5 * F, torch.int32)
    info, info_whole = poisoned(4 * F, torch.int32)
    lib = hip.load()
    need = lib.vface_png_inflate_parallel_workspace_bytes(F, total, expect, chunk_bytes)
    assert need > 0 and need % 16 == 0
    ws, ws_whole = poisoned(need, lead=48, tail=64)
    assert ws.data_ptr() % 16 == 0
    d_off, d_len = torch.from_numpy(np.asarray(offsets, np.int64)).to(DEV), torch.from_numpy(np.asarray(lengths, np.int32)).to(DEV)
    rc = lib.vface_png_inflate_parallel(streams.data_ptr(), total, d_off.data_ptr(), d_len.data_ptr(), F, rows.data_ptr(), stride, expect,
                                        meta.data_ptr(), meta[F:].data_ptr(), meta[2 * F:].data_ptr(), meta[3 * F:].data_ptr(), chunk_bytes,
                                        ws.data_ptr(), need, info.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    m = meta.cpu().numpy()
    clean = (frame_clean(streams_whole, total) and frame_clean(rows_whole, F * stride) and frame_clean(meta_whole, 5 * F)
             and frame_clean(info_whole, 4 * F) and frame_clean(ws_whole, need, lead=48))
    return {"status": m[:F].tolist(), "produced": m[F:2 * F].tolist(), "consumed": m[2 * F:3 * F].tolist(),
            "adler": m[3 * F:].reshape(F, 2).tolist(), "rows": rows.view(F, stride).cpu().numpy(), "info": info.view(F, 4).cpu().tolist(),
            "clean": clean}


@functools.lru_cache(maxsize=None)
def model(body, expect, chunk_bytes):
    return pmod.inflate_parallel(body, expect, chunk_bytes)


def assert_equals_model(got, bodies, expect, chunk_bytes, what, serial=None):
    """Per file: the model's status, produced, consumed, bytes, Adler halves and info; every byte behind ``produced`` still holds the
    sentinel; nothing outside the views was touched; and, where given, vface_png_inflate's own results on the same inputs."""
    for f, body in enumerate(bodies):
        want = model(body, expect, chunk_bytes)
        assert (got["status"][f], got["produced"][f], got["consumed"][f]) == (want.status, want.produced, want.consumed), (what, f, got["info"][f])
        row = got["rows"][f]
        assert row[:want.produced].tobytes() == want.data, (what, f)
        assert (row[want.produced:] == SENTINEL8).all(), (what, f, "bytes behind produced were written")
        assert tuple(got["adler"][f]) == want.adler, (what, f)
        assert tuple(got["info"][f]) == want.info, (what, f, got["info"][f], want.info)
        if serial is not None:
            assert (serial["status"][f], serial["produced"][f], serial["consumed"][f], serial["adler"][f]) == \
                   (got["status"][f], got["produced"][f], got["consumed"][f], got["adler"][f]), (what, f)
            assert np.array_equal(serial["rows"][f], row), (what, f)
    assert got["clean"], what


def inputs():
    """name -> (body, expect): families A and B and every constructed corner."""
    out = {"family_a": (pc.family_a()[0], len(pc.family_a()[1])), "family_b": (pc.family_b()[0], len(pc.family_b()[1]))}
    out.update({name: (case.body, case.expect) for name, case in pc.corners().items()})
    return out


@pytest.mark.parametrize("chunk_bytes", pc.CHUNKS)
def test_entry_point_equals_the_model_and_the_serial_entry_point(chunk_bytes):
    for name, (body, expect) in inputs().items():
        got = device_parallel([body], expect, chunk_bytes)
        assert_equals_model(got, [body], expect, chunk_bytes, (name, chunk_bytes), serial=device_inflate([body], expect))
        if name in pc.corners():
            assert got["info"][0][1] == pc.corners()[name].reason[chunk_bytes], name
    if chunk_bytes == 256:                              # the parallel path is taken, not only equalled
        for name, segments in (("family_a", 41), ("family_b", 82)):
            body, expect = inputs()[name]
            assert device_parallel([body], expect, 256)["info"][0] == [segments, 0, segments - 1, 0]


def test_files_of_different_kinds_in_one_call():
    """A file of 41 segments, the same file cut short (it falls back: a segment reports status 1), a file whose range lies outside
    the stream buffer, and a single-segment file of stored blocks, in one call."""
    body, data = pc.family_a()
    stored = cases.raw_deflate(data, 0)
    bodies = [body, body[:-700], b"", stored]
    lengths = np.array([len(body), len(body) - 700, 40, len(stored)], np.int32)
    total = len(body) + len(body) - 700 + len(stored)
    offsets = np.array([0, len(body), total - 20, 2 * len(body) - 700], np.int64)
    got = device_parallel(bodies, len(data), 256, offsets=offsets, lengths=lengths)
    assert got["info"] == [[41, 0, 40, 0], [0, 2, model(bodies[1], len(data), 256).info[2], 0], [0, 5, 0, 0], [1, 0, 0, 0]]
    assert got["status"] == [0, 1, 1, 0] and got["produced"][2] == 0 and got["consumed"][2] == 0
    assert (got["rows"][2] == SENTINEL8).all()
    keep = [0, 1, 3]
    part = {k: [v[i] for i in keep] if k != "clean" else v for k, v in got.items()}
    assert_equals_model(part, [bodies[i] for i in keep], len(data), 256, "mixed")


def test_512_files_in_one_call_every_status_among_them():
    bodies, wants, W, H = small_files()
    expect = (1 + 3 * W) * H
    assert len(bodies) == 512 and {w[0] for w in wants} >= set(range(15))
    got = device_parallel(bodies, expect, 64)
    assert_equals_model(got, bodies, expect, 64, "512 files")
    assert [(got["status"][f], got["produced"][f], got["consumed"][f]) for f in range(512)] == [w[:3] for w in wants]


def test_more_segments_than_the_decode_grid_and_more_files_than_the_resolve_grid():
    from vface_amd import hip
    body, data = pc.family_b()
    one = model(body, len(data), 64)
    copies = hip.PNG_INFLATE_PAR_DECODE_GRID_CAP // one.info[0] + 2
    assert one.info[1] == 0 and copies * one.info[0] > hip.PNG_INFLATE_PAR_DECODE_GRID_CAP and copies <= 40
    got = device_parallel([body] * copies, len(data), 64)
    assert_equals_model(got, [body] * copies, len(data), 64, "many segments")
    case = pc.corners()["final_block_ends_inside_a_byte"]
    files = hip.PNG_INFLATE_PAR_RESOLVE_GRID_CAP + 44
    got = device_parallel([case.body] * files, case.expect, 64)
    assert_equals_model(got, [case.body] * files, case.expect, 64, "many files")
    assert got["info"] == [[2, 0, 1, 0]] * files


def test_the_same_call_twice_into_the_same_workspace():
    """``hip.png_inflate_parallel`` keeps one workspace: B, then A (which leaves other tables and elements in it), then B again."""
    from vface_amd import hip

    def run(body, expect):
        streams = torch.from_numpy(np.frombuffer(body, np.uint8).copy()).to(DEV)
        rows, meta, info = hip.png_inflate_parallel(streams, torch.zeros(1, dtype=torch.int64, device=DEV),
                                                    torch.tensor([len(body)], dtype=torch.int32, device=DEV), expect, chunk_bytes=256)
        return rows.cpu().numpy().tobytes(), meta.cpu().tolist(), info.cpu().tolist()
    (a, da), (b, db) = pc.family_a(), pc.family_b()
    first = run(b, len(db))
    assert run(a, len(da))[0] == da
    assert run(b, len(db)) == first and first[0] == db and first[2] == [[82, 0, 81, 0]]
    assert len(hip._png_par_ws) == 1


def test_refusals_by_code():
    from vface_amd import hip
    lib, s = hip.load(), torch.cuda.current_stream().cuda_stream
    need = lib.vface_png_inflate_parallel_workspace_bytes(1, 64, 100, 64)
    t = torch.zeros(need + 4096, dtype=torch.uint8, device=DEV)
    p = t.data_ptr()
    assert p % 16 == 0
    ok = (p, 64, p, p, 1, p, 100, 100, p, p, p, p, 64, p, need, p, s)        # (refused before any launch: the pointers are never followed)
    call = lib.vface_png_inflate_parallel
    for at in (0, 2, 3, 5, 8, 9, 10, 11, 13):
        assert call(*(0 if i == at else v for i, v in enumerate(ok))) == ERR_ARG, at
    for at, bad in ((4, 0), (1, 0), (7, 0)):
        assert call(*(bad if i == at else v for i, v in enumerate(ok))) == ERR_ARG, at
    for at, bad in ((1, 1 << 31), (6, 99), (12, 60), (12, 66), (12, (1 << 20) + 4), (14, need - 1)):
        assert call(*(bad if i == at else v for i, v in enumerate(ok))) == ERR_SHAPE, (at, bad)
    assert call(*((p + 8) if i == 13 else v for i, v in enumerate(ok))) == ERR_ALIGN
    u8 = torch.zeros(14, dtype=torch.uint8, device=DEV)
    i32, i64 = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    for bad in ((u8.cpu(), i64, i32, 14), (u8, i32, i32, 14), (u8, i64, i32, 0), (u8, i64, i32.repeat(2), 14)):
        with pytest.raises(hip.VFaceHipError):
            hip.png_inflate_parallel(*bad)
    with pytest.raises(hip.VFaceHipError):
        hip.png_inflate_parallel(u8, i64, i32, 14, info=torch.zeros((1, 3), dtype=torch.int32, device=DEV))


# ---- the decoder of scripts/png_in.py
def family_rows(W, H, bpp, repeats):
    """Filtered rows of the families' kind: a random walk, every row's filter byte 0 .. 4; with ``repeats`` the second half of the
    rows repeats the first (family B's long references)."""
    n = 1 + bpp * W
    rows = np.frombuffer(pc.walk(n * H, W + H + bpp), np.uint8).reshape(H, n).copy()
    if repeats:
        rows[H // 2:H // 2 + H // 3] = rows[:H // 3]
    rows[:, 0] = np.arange(H) % 5
    return rows


@pytest.mark.parametrize("W,H", [(96, 64), (250, 136)])
@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_decode_parallel_equals_serial_and_pillow(W, H, bpp):
    from vface_amd.scripts import png_in
    records = []
    for repeats in (False, True):
        rows = family_rows(W, H, bpp, repeats).tobytes()
        stream = b"\x78\x01" + pc.deflate_small_blocks(rows) + zlib.adler32(rows).to_bytes(4, "big")
        records.append(png_in.parse_png(cases.png_bytes(W, H, COLOUR[bpp], b"", stream=stream), f"<{repeats}>"))
    frames = png_in.PNGFrames(W, H, records)
    par = png_in.decode(frames, DEV, inflate="parallel", chunk_bytes=256)
    info = png_in.last_info[0].cpu().tolist()
    ser = png_in.decode(frames, DEV, inflate="serial")
    assert png_in.last_info is None and torch.equal(par, ser)
    for k, r in enumerate(records):
        want = model(r.body, (1 + bpp * W) * H, 256)
        assert tuple(info[k]) == want.info and info[k][1] == 0 and info[k][0] >= (8 if W * H * bpp > 20000 else 2), (k, info[k])
        with Image.open(io.BytesIO(cases.png_bytes(W, H, COLOUR[bpp], b"", stream=b"\x78\x01" + r.body + r.adler.to_bytes(4, "big")))) as pic:
            assert np.array_equal(np.asarray(pic.convert("RGB")), par[k].cpu().numpy()), k


@pytest.mark.parametrize("W,H,stripe_rows", [(250, 136, None), (86, 40, 4), (21, 5, 2)])
def test_encoder_then_parallel_decoder_is_the_identity(W, H, stripe_rows):
    """``png.PNGEncoder``'s own files (a block per stripe) decode to the frames that went in, on as many segments as the model finds."""
    from vface_amd.scripts import png, png_in
    rgb = np.concatenate([pm.patterns(1, W, H, seed=9)[k] for k in ("smooth", "noise", "blocks")])
    frames = torch.from_numpy(rgb).to(DEV)
    enc = png.PNGEncoder(W, H) if stripe_rows is None else png.PNGEncoder(W, H, stripe_rows=stripe_rows)
    records = [png_in.parse_png(d, f"<{k}>") for k, d in enumerate(enc.encode(frames))]
    back = png_in.decode(png_in.PNGFrames(W, H, records), DEV, inflate="parallel", chunk_bytes=64)
    assert torch.equal(back, frames)
    info = png_in.last_info[0].cpu().tolist()
    wants = [model(r.body, (1 + 3 * W) * H, 64).info for r in records]
    assert [tuple(i) for i in info] == wants
    assert W * H < 1000 or any(w[0] >= 2 for w in wants)


def test_a_640x360_noisy_pillow_file_takes_the_parallel_path():
    from vface_amd import hip
    from vface_amd.scripts import png_in
    frame = pm.content("noisy", 640, 360, seed=1)
    data = cases.pillow_png(frame)
    record = png_in.parse_png(data)
    got = png_in.decode(png_in.PNGFrames(640, 360, [record]), DEV, inflate="parallel")
    with Image.open(io.BytesIO(data)) as pic:
        assert np.array_equal(np.asarray(pic.convert("RGB")), got[0].cpu().numpy())
    segments, reason, candidates, _ = png_in.last_info[0].cpu().tolist()[0]
    assert reason == 0 and segments == candidates + 1 and segments >= len(record.body) // (2 * hip.PNG_INFLATE_CHUNK_BYTES) >= 5, (segments, len(record.body))
    auto = png_in.decode(png_in.PNGFrames(640, 360, [record]), DEV, inflate="auto")
    assert torch.equal(auto, got) and (png_in.last_info is not None) == (len(record.body) > png_in.PARALLEL_MIN_BODY_BYTES)


# ---- end to end
@pytest.fixture(scope="module")
def clip_runs(tmp_path_factory):
    """The small seeded clip of tests/test_png_in_gpu.py (4 frames of 320 x 240, 2 per batch, RGB and RGBA files), read by Pillow and
    by the device with the parallel inflate."""
    import yaml
    from test_clip_io_cpu import square, template_landmarks
    from test_clip_run_gpu import FH, FW, N, small_cfg
    from vface_amd.scripts import VFace_inference_batch as cli
    root = tmp_path_factory.mktemp("png_in_par")
    rng = np.random.default_rng(11)
    (root / "frames").mkdir()
    ids = [2 + 3 * i for i in range(N)]
    for i, frame in zip(ids, rng.integers(0, 256, (N, FH, FW, 3), dtype=np.uint8)):
        if i % 2:
            frame = np.concatenate([frame, rng.integers(0, 256, (FH, FW, 1), dtype=np.uint8)], axis=2)
        Image.fromarray(frame).save(root / "frames" / f"{i}.png")
    Image.fromarray(rng.integers(0, 256, (180, 200, 3), dtype=np.uint8)).save(root / "src.png")
    quads = np.stack([square(160 + 4 * i, 120 - 3 * i, 60 + 2 * i, 0.06 * i) for i in range(N)])
    np.savez(root / "lm.npz", frames=np.stack([template_landmarks(q) for q in quads]), source=template_landmarks(square(100, 90, 50, -0.1)),
             crops=rng.integers(100, 412, (N, 68, 2)).astype(np.float64), source_crop=rng.integers(100, 412, (68, 2)).astype(np.float64))
    (root / "small.yaml").write_text(yaml.safe_dump({"model": {"params": {"unet_config": {"params": small_cfg()}}}}))

    def args(tag, extra):
        return ["--target_frames", str(root / "frames"), "--src_image", str(root / "src.png"), "--landmarks", str(root / "lm.npz"),
                "--synthetic_weights", "--config", str(root / "small.yaml"), "--H", "512", "--W", "512", "--max_steps", "1",
                "--ddim_steps", "50", "--n_frames", str(N), "--n_samples", "2", "--skip_save", "--Base_dir", str(root / tag), *extra]

    def run(tag, extra):
        opt = cli.build_parser().parse_args(args(tag, extra))
        opt.return_samples = True
        torch.manual_seed(opt.seed)
        return cli.run_clip(opt)["batches"]

    from vface_amd.scripts import png_in
    png_in.last_info = None
    parallel = run("g", ["--png_decoder", "gpu", "--png_in_inflate", "parallel"])
    info = [row for t in png_in.last_info for row in t.cpu().tolist()]
    return {"parallel": parallel, "info": info, "pillow": run("p", []), "refused": args("r", ["--png_in_inflate", "parallel"])}


def test_clip_run_pastes_the_same_frames_with_the_parallel_inflate(clip_runs):
    ours = torch.cat([x["pasted_frames"] for x in clip_runs["parallel"]])
    theirs = torch.cat([x["pasted_frames"] for x in clip_runs["pillow"]])
    assert torch.equal(ours, theirs)
    # (uniform noise: zlib stores it, and a file of stored blocks is one segment; what counts here is that the parallel entry point ran)
    assert clip_runs["info"] and all(row[1] == 0 and row[0] >= 1 for row in clip_runs["info"]), clip_runs["info"]


def test_the_flag_without_the_gpu_decoder_is_refused(clip_runs):
    from vface_amd.scripts import VFace_inference_batch as cli
    opt = cli.build_parser().parse_args(clip_runs["refused"])
    with pytest.raises(SystemExit, match="--png_in_inflate parallel.*--png_decoder gpu"):
        cli.run_clip(opt)
