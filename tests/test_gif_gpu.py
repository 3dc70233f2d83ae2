"""vface_gif_histogram, _boxes, _palette, _map and _lzw (csrc/gif.hip) against the model (tests/gif_model.py), bit for bit and each on
the MODEL's input to its stage; the writer of vface_amd/scripts/gif.py; and the real-clip run with --gif_out against the default."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import gif_cases as cases
import gif_model as gm
import png_model as pm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL8 = 0xA5
ERR_ARG, ERR_ALIGN, ERR_SHAPE = -1, -2, -3          # VFACE_ERR_* of include/vface_hip.h
SIZES = ((1, 1), (2, 1), (1, 2), (3, 5), (21, 5), (85, 2), (250, 136))      # (W, H)
PATTERNS = ("noise", "smooth", "flat", "extremes", "blocks")


@functools.lru_cache(maxsize=None)
def reference(W, H):
    """pattern -> (frames uint8 [3, H, W, 3], [gm.quantise of each]); F = 1 takes the first frame.  Computed once, never changed."""
    p = pm.patterns(3, W, H, seed=3 * W + H)
    return {k: (p[k], [gm.quantise(f) for f in p[k]]) for k in PATTERNS}


@functools.lru_cache(maxsize=None)
def model_image(W, H, name, f, seg):
    return gm.image_data(reference(W, H)[name][1][f]["indices"], seg)


class Guarded:
    """A device tensor of ``shape`` inside a byte buffer of SENTINEL8, 64 bytes in front and 64 behind; ``fill``: its own bytes."""

    def __init__(self, shape, dtype, fill=SENTINEL8, lead=64):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((lead + n + 64,), SENTINEL8, dtype=torch.uint8, device=DEV)
        self.view = self.buf[lead:lead + n].view(dtype).view(*shape)
        self.lead, self.n = lead, n
        if fill != SENTINEL8:
            self.buf[lead:lead + n] = fill

    def clean(self):
        whole = self.buf.cpu().numpy()
        return bool((whole[:self.lead] == SENTINEL8).all() and (whole[self.lead + self.n:] == SENTINEL8).all())

    def numpy(self):
        return self.view.cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stack(qs, key, dtype):
    return np.stack([np.asarray(q[key]) for q in qs]).astype(dtype)


def first_difference(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, model {want[tuple(bad[0])]}"


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("F", [1, 3])
def test_histogram_equals_the_model(W, H, F):
    from vface_amd import hip
    for name, (frames, qs) in reference(W, H).items():
        out = Guarded((F, hip.GIF_CELLS), torch.int32)
        assert hip.gif_histogram(dev(frames[:F]), out=out.view).data_ptr() == out.view.data_ptr()
        torch.cuda.synchronize()
        first_difference(out.numpy().astype(np.int64), stack(qs[:F], "counts", np.int64), f"counts {name} {W}x{H} F={F}")
        assert out.clean(), name


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("F", [1, 3])
def test_boxes_equal_the_model(W, H, F):
    from vface_amd import hip
    for name, (frames, qs) in reference(W, H).items():
        labels, ncolors = Guarded((F, hip.GIF_CELLS), torch.uint8), Guarded((F,), torch.int32)
        hip.gif_boxes(dev(stack(qs[:F], "counts", np.int32)), labels=labels.view, ncolors=ncolors.view)
        torch.cuda.synchronize()
        assert ncolors.numpy().tolist() == [q["ncolors"] for q in qs[:F]], name
        first_difference(labels.numpy(), stack(qs[:F], "labels", np.uint8), f"labels {name} {W}x{H} F={F}")
        assert labels.clean() and ncolors.clean(), name


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("F", [1, 3])
def test_palette_equals_the_model(W, H, F):
    from vface_amd import hip
    for name, (frames, qs) in reference(W, H).items():
        out = Guarded((F, 256, 3), torch.uint8)
        hip.gif_palette(dev(frames[:F]), dev(stack(qs[:F], "labels", np.uint8)), out=out.view)
        torch.cuda.synchronize()
        first_difference(out.numpy(), stack(qs[:F], "palette", np.uint8), f"palette {name} {W}x{H} F={F}")
        assert out.clean(), name


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("F", [1, 3])
def test_map_equals_the_model(W, H, F):
    from vface_amd import hip
    for name, (frames, qs) in reference(W, H).items():
        out = Guarded((F, W * H), torch.uint8, lead=37)
        hip.gif_map(dev(frames[:F]), dev(stack(qs[:F], "palette", np.uint8)), dev(np.array([q["ncolors"] for q in qs[:F]], np.int32)), out=out.view)
        torch.cuda.synchronize()
        first_difference(out.numpy(), stack(qs[:F], "indices", np.uint8), f"indices {name} {W}x{H} F={F}")
        assert out.clean(), name


def test_map_sends_ties_to_the_lowest_index_and_ignores_entries_past_ncolors():
    from vface_amd import hip
    pal = np.zeros((1, 256, 3), np.uint8)
    pal[0, 0], pal[0, 1], pal[0, 2], pal[0, 3] = (10, 10, 10), (20, 10, 10), (10, 20, 10), (15, 10, 10)
    frame = np.array([[[[15, 10, 10], [15, 15, 10], [10, 15, 10], [21, 10, 10], [0, 0, 0]]]], np.uint8)
    got = hip.gif_map(dev(frame), dev(pal), dev(np.array([3], np.int32))).cpu().numpy()[0]
    assert got.tolist() == gm.index_map(frame[0], pal[0], 3).tolist() == [0, 0, 0, 1, 0]


def test_reads_stop_at_the_frames_end():
    """66 049 pixels: one share of 65 536 and one of 513 for the histogram, four of 16 384 and one of 513 for the palette.  Bytes of 255
    follow the frames in the same allocation: a read past the end would count a white pixel."""
    from vface_amd import hip
    W = H = 257
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 200, (2, H, W, 3), dtype=np.uint8)
    assert (W * H) % hip.GIF_HIST_SHARE and (W * H) % hip.GIF_PALETTE_SHARE
    n = frames.size
    buf = torch.full((n + 4096,), 255, dtype=torch.uint8, device=DEV)
    buf[:n] = dev(frames).view(-1)
    view = buf[:n].view(2, H, W, 3)
    counts = hip.gif_histogram(view).cpu().numpy().astype(np.int64)
    want = np.stack([gm.histogram(f) for f in frames])
    first_difference(counts, want, "counts")
    assert counts[:, 32767].sum() == 0
    labels = [gm.boxes(c)[:2] for c in want]
    pal = hip.gif_palette(view, dev(np.stack([l for l, _ in labels]))).cpu().numpy()
    first_difference(pal, np.stack([gm.palette(f, l, nc) for f, (l, nc) in zip(frames, labels)]), "palette")


def test_more_frames_than_each_grid_holds():
    """1 x 1 frames, one more than the largest grid cap of the four quantiser stages: every stage's grid loops.  A frame of one pixel
    has one count, one box, its own colour and index 0 -- checked against the model on the first three."""
    from vface_amd import hip
    caps = (hip.GIF_HIST_GRID_CAP, hip.GIF_BOXES_GRID_CAP, hip.GIF_PALETTE_GRID_CAP, hip.GIF_MAP_GRID_CAP)
    F = max(caps) + 1
    frames = np.random.default_rng(2).integers(0, 256, (F, 1, 1, 3), dtype=np.uint8)
    d = dev(frames)
    counts = hip.gif_histogram(d)
    labels, ncolors = hip.gif_boxes(counts)
    pal = hip.gif_palette(d, labels)
    idx = hip.gif_map(d, pal, ncolors)
    px = frames.reshape(F, 3).astype(np.int64)
    cell = dev((px[:, 0] >> 3) << 10 | (px[:, 1] >> 3) << 5 | (px[:, 2] >> 3))
    assert bool((counts.sum(dim=1) == 1).all()) and bool((counts.gather(1, cell[:, None]) == 1).all())      # [F, 32768]: compared where it is
    assert not bool(labels.any()) and bool((ncolors == 1).all()) and not bool(idx.any())
    pal = pal.cpu().numpy()
    assert np.array_equal(pal[:, 0], px.astype(np.uint8)) and not pal[:, 1:].any()
    for f in range(3):
        q = gm.quantise(frames[f])
        assert q["counts"][int(cell[f])] == 1 and q["ncolors"] == 1 and np.array_equal(q["palette"], pal[f]) and not q["indices"].any()


# ---- LZW
def device_lzw(indices, seg, out_bytes=None, ws=None):
    """vface_gif_lzw on ``indices`` [F, npix] with an output buffer of exactly ``out_bytes`` (default: the bound) and a workspace of
    exactly the queried size, both with sentinel bytes around -> dict."""
    from vface_amd import hip
    F, npix = indices.shape
    lib = hip.load()
    need = int(lib.vface_gif_lzw_workspace_bytes(npix, F, seg))
    assert need > 0
    ws = Guarded((need,), torch.uint8) if ws is None else ws
    cap = F * hip.gif_lzw_bound(npix, seg)
    out = Guarded((cap,), torch.uint8, lead=37)
    offsets = Guarded((F + 1,), torch.int64)
    d = dev(indices)
    n = cap if out_bytes is None else out_bytes
    rc = lib.vface_gif_lzw(d.data_ptr(), npix, F, seg, out.view.data_ptr(), n, offsets.view.data_ptr(), ws.view.data_ptr(), need,
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return {"out": out.numpy(), "offsets": offsets.numpy().tolist(), "clean": out.clean() and offsets.clean() and ws.clean(), "cap": cap,
            "ws": ws, "indices": d}


def assert_lzw(got, images, what, written=None):
    """``images``: the model's image data per frame; ``written``: how many bytes the buffer could take (default all)."""
    want = b"".join(images)
    ends = np.cumsum([0] + [len(i) for i in images]).tolist()
    assert got["offsets"] == ends, (what, got["offsets"][:4], ends[:4])
    n = len(want) if written is None else written
    assert got["out"][:n].tobytes() == want[:n], what
    assert (got["out"][n:] == SENTINEL8).all() and got["clean"], f"{what}: bytes outside the image data were written"


@pytest.mark.parametrize("name", sorted(cases.lzw_cases()))
def test_lzw_equals_the_model_on_constructed_streams(name):
    from vface_amd import hip
    indices, seg = cases.lzw_cases()[name]
    images = [m["image"] for m in cases.model(name)]
    got = device_lzw(indices, seg)
    assert_lzw(got, images, name)
    for f, idx in enumerate(indices):                   # a decoder that knows nothing of the model reads the device's bytes
        data = got["out"][got["offsets"][f]:got["offsets"][f + 1]].tobytes()
        pal = np.repeat(np.arange(256, dtype=np.uint8), 3).tobytes()
        im = Image.open(io.BytesIO(gm.header(len(idx), 1) + gm.frame_header(len(idx), 1) + pal + data + b"\x3B"))
        assert np.array_equal(np.asarray(im.convert("RGB"))[0, :, 0], idx), (name, f)
    out, offsets = hip.gif_lzw(got["indices"], seg)     # the wrapper: its own workspace and worst-case buffer, same bytes
    assert offsets.cpu().tolist() == got["offsets"] and out.numel() == got["cap"]
    assert out[:got["offsets"][-1]].cpu().numpy().tobytes() == b"".join(images)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("F", [1, 3])
def test_lzw_equals_the_model_on_the_patterns(W, H, F):
    segs = (64, 4096, W * H + 1) + ((1,) if W * H <= 200 else ())
    for name, (frames, qs) in reference(W, H).items():
        indices = stack(qs[:F], "indices", np.uint8)
        for seg in segs:
            assert_lzw(device_lzw(indices, seg), [model_image(W, H, name, f, seg) for f in range(F)], f"{name} {W}x{H} F={F} seg {seg}")


def test_lzw_short_buffer_keeps_the_offsets_and_writes_nothing_behind_it():
    indices, seg = cases.lzw_cases()["three_frames"]
    images = [m["image"] for m in cases.model("three_frames")]
    short = sum(map(len, images)) - 101
    assert short > len(images[0]) + len(images[1])      # the cut falls inside the last frame
    assert_lzw(device_lzw(indices, seg, out_bytes=short), images, "short buffer", written=short)


def test_lzw_twice_into_one_workspace():
    """The second call finds the first call's codes, counts and bits in the workspace: a longer stream first, then a shorter one."""
    big, seg = cases.lzw_cases()["noise_three_tables_in_segments"]
    first = device_lzw(big, seg)
    assert_lzw(first, [m["image"] for m in cases.model("noise_three_tables_in_segments")], "first")
    small = np.zeros_like(big)
    again = device_lzw(small, seg, ws=first["ws"])
    assert_lzw(again, [gm.image_data(i, seg) for i in small], "second")
    assert_lzw(device_lzw(big, seg, ws=first["ws"]), [m["image"] for m in cases.model("noise_three_tables_in_segments")], "third")


def test_lzw_past_its_grid_caps():
    """More (frame, segment) pairs than GIF_LZW_GRID_CAP workgroups, and more codes and bytes than the packing grids hold threads:
    16 frames of 250 x 136 in segments of 7, and one frame in segments of 1."""
    from vface_amd import hip
    frames, qs = reference(250, 136)["smooth"]
    one = qs[0]["indices"]
    assert len(one) > hip.GIF_LZW_GRID_CAP
    assert_lzw(device_lzw(one[None], 1), [gm.image_data(one, 1)], "segments of 1")
    indices = np.stack([np.roll(qs[f % 3]["indices"], 17 * f) for f in range(16)])
    nseg = (indices.shape[1] + 6) // 7
    assert 16 * nseg * 8 > hip.GIF_LZW_FLAT_GRID_CAP * 256 and 16 * nseg > hip.GIF_LZW_GRID_CAP
    assert_lzw(device_lzw(indices, 7), [gm.image_data(i, 7) for i in indices], "16 frames, segments of 7")


def test_refusals():
    from vface_amd import hip
    ok = dev(pm.patterns(2, 33, 18)["noise"])
    for fn in (hip.gif_histogram, lambda t: hip.gif_palette(t, None), lambda t: hip.gif_map(t, None, None)):
        for bad in (ok.cpu(), ok.float(), ok[..., :2], ok.permute(0, 2, 1, 3)):
            with pytest.raises(hip.VFaceHipError):
                fn(bad)
    counts = hip.gif_histogram(ok)
    for bad in (counts.cpu(), counts.to(torch.int64), counts[0], counts[:, :100]):
        with pytest.raises(hip.VFaceHipError):
            hip.gif_boxes(bad)
    labels, ncolors = hip.gif_boxes(counts)
    with pytest.raises(hip.VFaceHipError):
        hip.gif_palette(ok, labels[:1])
    pal = hip.gif_palette(ok, labels)
    with pytest.raises(hip.VFaceHipError):
        hip.gif_map(ok, pal, ncolors.to(torch.int64))
    idx = hip.gif_map(ok, pal, ncolors)
    for bad in (idx.cpu(), idx.to(torch.int16), idx[0], idx[:, ::2]):
        with pytest.raises(hip.VFaceHipError):
            hip.gif_lzw(bad)
    for seg in (0, 65536):
        with pytest.raises(hip.VFaceHipError):
            hip.gif_lzw(idx, seg)
    lib, s = hip.load(), torch.cuda.current_stream().cuda_stream
    p = idx.data_ptr()
    # refused before any launch: W * H above 2^24 and a side above 65535, a workspace off 16 bytes, one too small, seg_pixels above 65535
    assert lib.vface_gif_histogram(p, 4097, 4096, 1, p, s) == ERR_SHAPE and lib.vface_gif_map(p, 65536, 1, 1, p, p, p, s) == ERR_SHAPE
    assert lib.vface_gif_palette(p, 4097, 4096, 1, p, p, p, s) == ERR_SHAPE and lib.vface_gif_palette(p, 4, 4, 1, p, p, p + 1, s) == ERR_ALIGN
    assert lib.vface_gif_lzw(p, 594, 2, 64, p, 10, p, p + 1, 1 << 30, s) == ERR_ALIGN
    assert lib.vface_gif_lzw(p, 594, 2, 64, p, 10, p, p, 16, s) == ERR_SHAPE
    assert lib.vface_gif_lzw(p, 594, 2, 65536, p, 10, p, p, 1 << 30, s) == ERR_SHAPE
    assert lib.vface_gif_lzw(p, (1 << 24) + 1, 1, 64, p, 10, p, p, 1 << 40, s) == ERR_SHAPE
    assert lib.vface_gif_lzw(0, 594, 2, 64, p, 10, p, p, 1 << 30, s) == ERR_ARG


# ---- the file
@pytest.mark.parametrize("W,H,seg", [(250, 136, None), (21, 5, 2), (85, 2, 171)])
def test_writer_writes_the_models_file(tmp_path, W, H, seg):
    from vface_amd import hip
    from vface_amd.scripts import gif
    frames, qs = reference(W, H)["blocks"]
    more, more_qs = reference(W, H)["smooth"]
    path = str(tmp_path / "a.gif")
    with (gif.GIFWriter(path, W, H) if seg is None else gif.GIFWriter(path, W, H, seg_pixels=seg)) as w:
        assert w.write(dev(frames)) == 3 and w.write(dev(more[:1])) == 1 and w.frames == 4        # two batches of different sizes
        with pytest.raises(hip.VFaceHipError):
            w.write(dev(frames)[:, :, :-1])
        with pytest.raises(hip.VFaceHipError):
            w.write(torch.from_numpy(frames))
        used = w.seg_pixels
    assert used == (hip.GIF_SEG_PIXELS if seg is None else seg)
    data = open(path, "rb").read()
    every = np.concatenate([frames, more[:1]])
    assert data == gm.gif_file(every, used, qs=qs + more_qs[:1])[0]
    im = Image.open(io.BytesIO(data))
    assert im.size == (W, H) and im.n_frames == 4 and im.info["loop"] == 0
    for f, q in enumerate(qs + more_qs[:1]):
        im.seek(f)
        assert im.info["duration"] == 100 and np.array_equal(np.asarray(im.convert("RGB")), q["palette"][q["indices"]].reshape(H, W, 3)), f


def test_clip_sink_writes_the_gif_even_with_skip_save(tmp_path):
    """Stand-in batches through the clip sink: --gif_out alone, with --skip_save, and beside the PNGs; the stage is timed."""
    import types
    from vface_amd import hip
    from vface_amd.scripts import VFace_inference_batch as cli
    from vface_amd.scripts.outputs import ClipOutputs
    from vface_amd.scripts.pipeline import StageTimer
    W, H = 48, 32
    rgb = pm.patterns(5, W, H, seed=3)["blocks"]
    for tag, flags in (("skip", ["--skip_save"]), ("save", ["--gif_seg_pixels", "100"])):
        base = tmp_path / tag
        opt = cli.normalise_options(cli.build_parser().parse_args(["--Base_dir", str(base), "--gif_out", str(tmp_path / f"{tag}.gif"), *flags]))
        sink = ClipOutputs(opt)
        timers = []
        for ids in ([0, 1, 2], [3, 4]):                  # a shorter last batch, as --whole_clip hands it over
            b = types.SimpleNamespace(pasted=dev(rgb[ids]), frame_ids=ids, id=0, samples=torch.zeros(1, device=DEV), pixels=None, timer=StageTimer())
            sink.write(b)
            timers.append(b.timer.seconds)
        sink.close()
        assert all(t["gif_out"] > 0 for t in timers)
        assert (base / "results").exists() == (tag == "save")
        seg = hip.GIF_SEG_PIXELS if tag == "skip" else 100
        assert (tmp_path / f"{tag}.gif").read_bytes() == gm.gif_file(rgb, seg)[0]


# ---- end to end
@pytest.fixture(scope="module")
def clip_runs(tmp_path_factory):
    """The small seeded clip of tests/test_png_gpu.py's kind (4 frames of 320 x 240, 2 per batch), with and without --gif_out."""
    import yaml
    from test_clip_io_cpu import square, template_landmarks
    from test_clip_run_gpu import FH, FW, N, small_cfg
    from vface_amd.scripts import VFace_inference_batch as cli
    root = tmp_path_factory.mktemp("gif_out")
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

    return {"root": root, "n": N, "gif": run("g", ["--gif_out", str(root / "clip.gif")]), "plain": run("p", [])}


def test_clip_run_writes_the_default_pngs_and_the_models_gif(clip_runs):
    from vface_amd import hip
    root = clip_runs["root"]
    pasted = torch.cat([x["pasted_frames"] for x in clip_runs["gif"]]).cpu().numpy()
    assert torch.equal(torch.cat([x["pasted_frames"] for x in clip_runs["plain"]]).cpu(), torch.from_numpy(pasted))
    for i in range(clip_runs["n"]):
        assert (root / "g" / "results" / f"{i}.png").read_bytes() == (root / "p" / "results" / f"{i}.png").read_bytes(), i
    data = (root / "clip.gif").read_bytes()
    want, qs = gm.gif_file(pasted, hip.GIF_SEG_PIXELS)
    assert data == want
    im = Image.open(io.BytesIO(data))
    assert im.n_frames == clip_runs["n"] and im.size == (pasted.shape[2], pasted.shape[1])
    for f, q in enumerate(qs):
        im.seek(f)
        assert np.array_equal(np.asarray(im.convert("RGB")), q["palette"][q["indices"]].reshape(pasted.shape[1:]))
    assert not (root / "p" / "clip.gif").exists()


def test_gif_out_is_timed_in_that_run_only(clip_runs):
    for x, y in zip(clip_runs["gif"], clip_runs["plain"]):
        assert x["stage_seconds"]["gif_out"] > 0 and "gif_out" not in y["stage_seconds"]
        assert set(x["stage_seconds"]) - set(y["stage_seconds"]) == {"gif_out"} and set(x) == set(y)
