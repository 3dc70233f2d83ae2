"""vface_png_filter and vface_png_deflate (csrc/png.hip) against the model (tests/png_model.py), bit for bit and byte for byte; the
encoder of vface_amd/scripts/png.py; and the real-clip run with --png_encoder gpu against the default."""
import io
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as cases
import png_model as pm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL8 = 0xA5
ERR_ARG, ERR_ALIGN, ERR_SHAPE = -1, -2, -3          # VFACE_ERR_* of include/vface_hip.h
SIZES = ((1, 1), (2, 1), (1, 2), (3, 5), (21, 5), (85, 2), (86, 2), (250, 136))      # (W, H); row_bytes 64, 256 and 259 among them


def filtered_in_sentinel(rgb):
    """The kernel's rows for ``rgb`` inside a uint8 buffer of SENTINEL8 -> (rows [F, H, 1 + 3 W], True where the rest is untouched)."""
    from vface_amd import hip
    F, H, W, _ = rgb.shape
    n, lead = F * H * (1 + 3 * W), 37
    buf = torch.full((lead + n + 64,), SENTINEL8, dtype=torch.uint8, device=DEV)
    view = buf[lead:lead + n].view(F, H, 1 + 3 * W)
    out = hip.png_filter(torch.from_numpy(rgb).to(DEV), out=view)
    assert out.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    return view.cpu().numpy(), bool((whole[:lead] == SENTINEL8).all() and (whole[lead + n:] == SENTINEL8).all())


def assert_rows(got, rgb, what):
    want = np.stack([pm.filter_rows(f) for f in rgb])
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} of {want.size} bytes differ, first at (frame, row, byte) {tuple(bad[0])}: "
                           f"got {got[tuple(bad[0])]}, model {want[tuple(bad[0])]}")


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("F", [1, 3])
def test_filter_equals_the_model(W, H, F):
    for name, rgb in pm.patterns(F, W, H, seed=3 * W + H).items():
        got, clean = filtered_in_sentinel(rgb)
        assert_rows(got, rgb, f"{name} {W}x{H} F={F}")
        assert clean, f"{name}: bytes outside the rows were written"


def test_filter_chooses_every_type():
    frame = pm.content("noisy", 96, 64, seed=2)
    rng = np.random.default_rng(1)
    extra = np.stack([np.zeros((96, 3), np.uint8), (np.arange(288).reshape(96, 3) * 5 % 256).astype(np.uint8),
                      rng.integers(0, 256, (96, 3), dtype=np.uint8)])
    rgb = np.concatenate([extra, extra[2:], frame])[None]
    assert set(pm.filter_rows(rgb[0])[:, 0].tolist()) >= {0, 1, 2, 4}
    got, clean = filtered_in_sentinel(rgb)
    assert_rows(got, rgb, "types")
    assert clean


def test_filter_past_the_grid_cap():
    """More rows than PNG_FILTER_GRID_CAP workgroups x 4 rows, no multiple of 4; two frames, so a frame's first row falls mid-grid."""
    from vface_amd import hip
    H = hip.PNG_FILTER_GRID_CAP * hip.PNG_FILTER_ROWS_PER_GROUP // 2 + 27
    assert 2 * H > hip.PNG_FILTER_GRID_CAP * hip.PNG_FILTER_ROWS_PER_GROUP and (2 * H) % 4
    rgb = np.random.default_rng(5).integers(0, 256, (2, H, 2, 3), dtype=np.uint8)
    got, clean = filtered_in_sentinel(rgb)
    assert_rows(got, rgb, "past the cap")
    assert clean


def device_deflate(rows, stripe_rows, out_bytes=None):
    """vface_png_deflate on ``rows`` [F, H, rb] with an output buffer of exactly ``out_bytes`` (default: the bodies' total) and a
    workspace of exactly the queried size, both with sentinel bytes behind -> dict."""
    from vface_amd import hip
    F, H, rb = rows.shape
    S = (H + stripe_rows - 1) // stripe_rows
    lib = hip.load()
    need = int(lib.vface_png_deflate_workspace_bytes(rb, H, F, stripe_rows))
    assert need > 0
    ws = torch.full((need + 256,), SENTINEL8, dtype=torch.uint8, device=DEV)
    cap = F * hip.png_deflate_bound(rb, H, stripe_rows)
    out = torch.full((cap + 64,), SENTINEL8, dtype=torch.uint8, device=DEV)
    lengths = torch.full((F + 4,), -7, dtype=torch.int32, device=DEV)
    offsets = torch.full((F + 4,), -7, dtype=torch.int64, device=DEV)
    adler = torch.full((F * S * 2 + 4,), -7, dtype=torch.int32, device=DEV)
    drows = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
    n = cap if out_bytes is None else out_bytes
    rc = lib.vface_png_deflate(drows.data_ptr(), rb, H, F, stripe_rows, out.data_ptr(), n, offsets.data_ptr(), lengths.data_ptr(),
                               adler.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return {"out": out.cpu().numpy(), "lengths": lengths.cpu().numpy(), "offsets": offsets.cpu().numpy(), "adler": adler.cpu().numpy(),
            "ws_clean": bool((ws[need:].cpu().numpy() == SENTINEL8).all()), "cap": cap, "n": n, "rows": drows}


@pytest.mark.parametrize("name", sorted(cases.deflate_cases()))
def test_deflate_equals_the_model(name):
    """Bodies byte for byte, lengths, offsets and Adler halves equal the model's; nothing behind the bodies, behind the buffer or
    behind the workspace is touched; zlib, which knows nothing of the model, inflates the device's stream to the input."""
    from vface_amd import hip
    rows, stripe_rows = cases.deflate_cases()[name]
    F = rows.shape[0]
    want = cases.model(name)
    bodies = [d["body"] for d in want]
    total = sum(len(b) for b in bodies)
    got = device_deflate(rows, stripe_rows)
    assert got["lengths"][:F].tolist() == [len(b) for b in bodies] and (got["lengths"][F:] == -7).all(), name
    assert got["offsets"][:F].tolist() == np.concatenate([[0], np.cumsum([len(b) for b in bodies])[:-1]]).tolist() and (got["offsets"][F:] == -7).all()
    assert got["out"][:total].tobytes() == b"".join(bodies), name
    assert (got["out"][total:] == SENTINEL8).all() and got["ws_clean"], name
    halves = [v for d in want for pair in d["adler"] for v in pair]
    assert got["adler"][:len(halves)].tolist() == halves and (got["adler"][len(halves):] == -7).all(), name
    at = 0
    for f in range(F):
        value = zlib.adler32(rows[f].tobytes())
        body = got["out"][at:at + len(bodies[f])].tobytes()
        assert zlib.decompress(b"\x78\x01" + body + struct.pack(">I", value)) == rows[f].tobytes(), (name, f)
        at += len(bodies[f])
    # the wrapper: its own workspace and worst-case buffer, same bytes
    out, meta, offsets = hip.png_deflate(got["rows"], stripe_rows)
    meta = meta.cpu().tolist()
    assert meta[:F] == [len(b) for b in bodies] and meta[F:] == halves and out[:total].cpu().numpy().tobytes() == b"".join(bodies)
    assert out.numel() == got["cap"] >= total and offsets.cpu().tolist() == got["offsets"][:F].tolist()


def test_deflate_reaches_the_bound_on_noise():
    rows, sr = cases.deflate_cases()["noise"]
    got = device_deflate(rows, sr)
    assert got["lengths"][0] == got["cap"] == 80000 + 2 * 5 + 2


def test_deflate_drops_what_a_short_buffer_cannot_hold():
    """out_bytes smaller than the bodies: the lengths are still the true ones and nothing behind out_bytes is written."""
    rows, sr = cases.deflate_cases()["three_frames"]
    want = b"".join(d["body"] for d in cases.model("three_frames"))
    short = len(want) - 101
    got = device_deflate(rows, sr, out_bytes=short)
    assert int(got["lengths"][:3].sum()) == len(want)
    assert got["out"][:short].tobytes() == want[:short] and (got["out"][short:] == SENTINEL8).all() and got["ws_clean"]


def test_refusals():
    from vface_amd import hip
    ok = torch.from_numpy(pm.patterns(2, 33, 18)["noise"]).to(DEV)
    for bad in (ok.cpu(), ok.float(), ok[..., :2], ok.permute(0, 2, 1, 3)):
        with pytest.raises(hip.VFaceHipError):
            hip.png_filter(bad)
    rows = hip.png_filter(ok)
    for bad in (rows.cpu(), rows.to(torch.int16), rows[0], rows[:, :, ::2]):
        with pytest.raises(hip.VFaceHipError):
            hip.png_deflate(bad)
    with pytest.raises(hip.VFaceHipError):
        hip.png_deflate(rows, 0)
    lib, s = hip.load(), torch.cuda.current_stream().cuda_stream
    p = rows.data_ptr()
    # refused before any launch: a workspace off 16 bytes (VFACE_ERR_ALIGN), row_bytes * H = 2^31 and a workspace too small (VFACE_ERR_SHAPE)
    assert lib.vface_png_deflate(p, 100, 18, 2, 16, p, 10, p, p, p, p + 1, 1 << 30, s) == ERR_ALIGN
    assert lib.vface_png_deflate(p, 1 << 20, 1 << 11, 1, 16, p, 10, p, p, p, p, 1 << 30, s) == ERR_SHAPE
    assert lib.vface_png_deflate(p, 100, 18, 2, 16, p, 10, p, p, p, p, 16, s) == ERR_SHAPE
    assert lib.vface_png_filter(0, 33, 18, 2, p, s) == ERR_ARG


@pytest.mark.parametrize("W,H,stripe_rows", [(250, 136, None), (21, 5, 2), (86, 2, 1)])
def test_encoder_writes_the_models_files(W, H, stripe_rows):
    from vface_amd import hip
    from vface_amd.scripts import png
    rgb = np.concatenate([pm.patterns(1, W, H, seed=9)[k] for k in ("smooth", "noise", "blocks")])
    enc = png.PNGEncoder(W, H) if stripe_rows is None else png.PNGEncoder(W, H, stripe_rows=stripe_rows)
    files = enc.encode(torch.from_numpy(rgb).to(DEV))
    assert len(files) == 3
    for f, data in enumerate(files):
        assert data == pm.encode(rgb[f], enc.stripe_rows), f
        im = Image.open(io.BytesIO(data))
        assert im.mode == "RGB" and im.size == (W, H) and np.array_equal(np.asarray(im), rgb[f])
    assert enc.encode(torch.from_numpy(rgb[:1]).to(DEV)) == files[:1]              # another batch size through the same encoder
    with pytest.raises(hip.VFaceHipError):
        enc.encode(torch.from_numpy(rgb).to(DEV)[:, :, :-1])
    with pytest.raises(hip.VFaceHipError):
        enc.encode(torch.from_numpy(rgb))


@pytest.mark.parametrize("encoder", ["gpu", "pillow"])
def test_both_sinks_write_through_the_flag(tmp_path, encoder):
    """Stand-in batches (pasted, ids, timer) through the seeded and the clip sink: the model's files under the usual names and a
    ``png_out`` stage with ``--png_encoder gpu``; Pillow's files and no such stage without it."""
    import types
    from vface_amd import hip
    from vface_amd.scripts import VFace_inference_batch as cli
    from vface_amd.scripts.outputs import ClipOutputs, SeededOutputs
    from vface_amd.scripts.pipeline import StageTimer
    W, H = 48, 32
    rgb = pm.patterns(3, W, H, seed=3)["blocks"]
    flag = ["--png_encoder", "gpu"] if encoder == "gpu" else []
    for sink_type, names in ((ClipOutputs, [f"results/{i}.png" for i in (4, 5, 6)]), (SeededOutputs, [f"pasted_b7_f{f}.png" for f in range(3)])):
        base = tmp_path / sink_type.__name__
        opt = cli.normalise_options(cli.build_parser().parse_args(["--Base_dir", str(base), *flag]))
        sink = sink_type(opt)
        b = types.SimpleNamespace(pasted=torch.from_numpy(rgb).to(DEV), frame_ids=[4, 5, 6], id=7, samples=torch.zeros(1, device=DEV),
                                  pixels=None, timer=StageTimer())
        sink.write(b)
        sink.close()
        assert ("png_out" in b.timer.seconds) == (encoder == "gpu")
        for f, name in enumerate(names):
            data = (base / name).read_bytes()
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), rgb[f]), name
            if encoder == "gpu":
                assert data == pm.encode(rgb[f], hip.PNG_STRIPE_ROWS), name
            else:
                buf = io.BytesIO()
                Image.fromarray(rgb[f]).save(buf, "PNG")
                assert data == buf.getvalue(), name


# ---- end to end
@pytest.fixture(scope="module")
def clip_runs(tmp_path_factory):
    """The small seeded clip of tests/test_demux_run_gpu.py's kind (4 frames of 320 x 240, 2 per batch), saved both ways."""
    import yaml
    from test_clip_io_cpu import square, template_landmarks
    from test_clip_run_gpu import FH, FW, N, small_cfg
    from vface_amd.scripts import VFace_inference_batch as cli
    root = tmp_path_factory.mktemp("png_out")
    rng = np.random.default_rng(11)
    (root / "frames").mkdir()
    for i, frame in enumerate(rng.integers(0, 256, (N, FH, FW, 3), dtype=np.uint8)):
        Image.fromarray(frame).save(root / "frames" / f"{i}.png")
    Image.fromarray(rng.integers(0, 256, (180, 200, 3), dtype=np.uint8)).save(root / "src.png")
    quads = np.stack([square(160 + 4 * i, 120 - 3 * i, 60 + 2 * i, 0.06 * i) for i in range(N)])
    np.savez(root / "lm.npz", frames=np.stack([template_landmarks(q) for q in quads]), source=template_landmarks(square(100, 90, 50, -0.1)),
             crops=rng.integers(100, 412, (N, 68, 2)).astype(np.float64), source_crop=rng.integers(100, 412, (68, 2)).astype(np.float64))
    (root / "small.yaml").write_text(yaml.safe_dump({"model": {"params": {"unet_config": {"params": small_cfg()}}}}))

    def run(tag, extra):
        args = ["--target_frames", str(root / "frames"), "--src_image", str(root / "src.png"), "--landmarks", str(root / "lm.npz"),
                "--synthetic_weights", "--config", str(root / "small.yaml"), "--H", "512", "--W", "512", "--max_steps", "1",
                "--ddim_steps", "50", "--n_frames", str(N), "--n_samples", "2", "--Base_dir", str(root / tag), *extra]
        opt = cli.build_parser().parse_args(args)
        opt.return_samples = True
        torch.manual_seed(opt.seed)
        return cli.run_clip(opt)["batches"]

    return {"root": root, "n": N, "gpu": run("g", ["--png_encoder", "gpu"]), "pillow": run("p", [])}


def test_clip_run_writes_the_same_pixels_either_way(clip_runs):
    from vface_amd import hip
    root = clip_runs["root"]
    pasted = torch.cat([x["pasted_frames"] for x in clip_runs["gpu"]]).cpu().numpy()
    assert torch.equal(torch.cat([x["pasted_frames"] for x in clip_runs["pillow"]]).cpu(), torch.from_numpy(pasted))
    for i in range(clip_runs["n"]):
        ours, theirs = (np.asarray(Image.open(root / tag / "results" / f"{i}.png")) for tag in ("g", "p"))
        assert np.array_equal(ours, theirs) and np.array_equal(ours, pasted[i]), i
        data = (root / "g" / "results" / f"{i}.png").read_bytes()
        assert data == pm.encode(pasted[i], hip.PNG_STRIPE_ROWS), i


def test_png_out_is_timed_for_the_gpu_encoder_only(clip_runs):
    for x, y in zip(clip_runs["gpu"], clip_runs["pillow"]):
        assert x["stage_seconds"]["png_out"] > 0 and "png_out" not in y["stage_seconds"]
        assert set(x["stage_seconds"]) - set(y["stage_seconds"]) == {"png_out"} and set(x) == set(y)
