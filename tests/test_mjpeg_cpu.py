"""The Motion-JPEG path without a GPU: the integer model (tests/jpeg_model.py) against the fp64 definition, against Pillow's decoder
and against Pillow's own encoder; its tables against Pillow's and against the kernel source; ten seeded defects each seen; the
reciprocal multiply and the value ranges the kernel relies on; the AVI round trip, the writer's and the command line's refusals."""
import io
import os
import re
import struct

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_model as jm
from conftest import ROOT
from vface_amd import hip
from vface_amd.scripts import VFace_inference_batch as cli
from vface_amd.scripts import mjpeg

QUALITIES = (50, 90, 100)
BIG = ((130, 50), (250, 136))          # the sizes of the comparison with Pillow's encoder (smaller frames make the ratio a coin toss)
MSE_BOUND = 1.02


def restarts(W, H):
    return (1, 3, jm.mcu_grid(W, H)[1])


def decode(frame: bytes):
    im = Image.open(io.BytesIO(frame))
    im.load()
    return im


def mse_against(rgb, frame: bytes):
    return float(((np.asarray(decode(frame).convert("RGB")).astype(np.float64) - rgb) ** 2).mean())


def pillow_frame(rgb, quality: int) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


# ---- the bound of the model against the definition, derived from the tables
def definition_bound():
    """eps [6, 64] (row-major): how far c / 2^15 of the model can lie from the fp64 DCT x of the fp64 Y'CbCr.
    - colour: the integer Y differs from the fp64 one by its rounding (1/2) and the rounding residues of its three coefficients
      times 255; a chroma sample by 1/2 (the clamp of 256 to 255 stays inside it: the fp64 value ends at 255.5) and the residues
      times the block sum 1020, over 2^18.  A pixel error e moves coefficient (v, u) by at most e * sum|a_v cos| * sum|a_u cos|.
    - rows: t differs from 4 T (T the exact 8-point transform of the integer pixels) by the shift's rounding (1/2) and the residues
      of the cosine row times 128, over 2^11.
    - columns: c differs from 2^15 x by the row error through sum|C[v]| and the residues of the cosine row times max|4 T|."""
    kr, kb = 0.299, 0.114
    res = lambda table, exact, scale: float(np.abs(table - np.asarray(exact) * scale).sum())
    e_y = 0.5 + res(jm.LUMA, [kr, 1 - kr - kb, kb], 65536.0) * 255 / 65536.0
    cb = np.array([-kr, -(1 - kr - kb), 1 - kb]) / (2 * (1 - kb))
    cr = np.array([1 - kr, -(1 - kr - kb), -kb]) / (2 * (1 - kr))
    e_c = 0.5 + max(res(jm.CB, cb, 65536.0), res(jm.CR, cr, 65536.0)) * 1020 / 2.0 ** 18
    l1 = np.abs(jm.C_EXACT).sum(axis=1)                                        # sum_n |a_k cos|, per frequency
    resid = np.abs(jm.C - 8192.0 * jm.C_EXACT).sum(axis=1)                     # rounding residues of a cosine row
    row_err = 0.5 + resid * 128 / 2048.0                                       # |t - 4 T|, per u
    t_peak = 4.0 * l1 * 128                                                    # |4 T|, per u
    c_err = np.abs(jm.C).sum(axis=1)[:, None] * row_err[None, :] + resid[:, None] * t_peak[None, :]       # [v][u], scale 2^15
    dct = (c_err / 32768.0).reshape(64)
    spread = (l1[:, None] * l1[None, :]).reshape(64)
    return np.stack([dct + spread * e_y] * 4 + [dct + spread * e_c] * 2)


def bound_violations(rgb, quality, defect=None) -> int:
    qy, qc = jm.quant_tables(quality)
    q = jm.coefficients(rgb, qy, qc, defect).astype(np.float64)
    inv = np.argsort(jm.ZIGZAG)
    q = q[..., inv]                                                            # back to row-major
    Q = np.stack([qy] * 4 + [qc] * 2).astype(np.float64)
    x = jm.fp64_coefficients(rgb)
    return int((np.abs(q - x / Q) > 0.5 + definition_bound() / Q + 1e-9).sum())


def test_bound_is_small():
    """The derived bound is a few levels at Q = 1 (the pixel rounding through the 8 x 8 sum dominates), not a loose one."""
    eps = definition_bound()
    assert 4.0 < eps.max() < 5.0 and eps.min() > 2.0, (eps.min(), eps.max())


@pytest.mark.parametrize("W,H", jm.SIZES)
def test_model_against_the_definition(W, H):
    for name, rgb in jm.patterns(2, W, H).items():
        for quality in QUALITIES:
            assert bound_violations(rgb, quality) == 0, (name, quality)


@pytest.mark.parametrize("W,H", jm.SIZES)
def test_pillow_decodes_every_model_frame(W, H):
    for name, rgb in jm.patterns(1, W, H).items():
        for quality in QUALITIES:
            qy, qc = jm.quant_tables(quality)
            coef = jm.coefficients(rgb, qy, qc)
            for restart in restarts(W, H):
                frame = jm.jpeg_frame(W, H, qy, qc, restart, jm.scan_bytes(coef[0], restart))
                assert decode(frame).size == (W, H), (name, quality, restart)


def mse_ratio(rgb, quality, restart, defect=None):
    frame = jm.encode_frames(rgb[None], quality, restart, defect)[0]
    return mse_against(rgb, frame) / mse_against(rgb, pillow_frame(rgb, quality))


@pytest.mark.parametrize("W,H", BIG)
def test_error_against_the_source_is_pillows(W, H):
    """Pillow's own encoder at the same quality and subsampling on the same image, both decoded by Pillow: the model's mean
    squared error is at most 1.02 x Pillow's.  Measured: 0.9951 .. 1.0014 over these 18 cases."""
    pats = jm.patterns(1, W, H)
    for name in ("smooth", "noise", "edges"):
        for quality in QUALITIES:
            r = mse_ratio(pats[name][0], quality, jm.mcu_grid(W, H)[1])
            print(f"{W}x{H} {name} q{quality}: {r:.4f}")
            assert r <= MSE_BOUND, (name, quality, r)


def segments(data: bytes):
    """(marker, payload) of every segment of a JPEG up to and including SOS."""
    pos = 2
    while True:
        marker, size = data[pos + 1], struct.unpack_from(">H", data, pos + 2)[0]
        yield marker, data[pos + 4:pos + 2 + size]
        if marker == 0xDA:
            return
        pos += 2 + size


def dqt_tables(data: bytes):
    """{table id: its 64 bytes as stored}; a DQT segment may hold one table or several."""
    out = {}
    for marker, payload in segments(data):
        if marker == 0xDB:
            for i in range(0, len(payload), 65):
                out[payload[i]] = payload[i + 1:i + 65]
    return out


def to_row_major(table):
    """Pillow's ``quantization`` has been zigzag in some versions and row-major in others: whichever of the two orders makes the
    table the scaled Annex-K one decides."""
    table = np.asarray(list(table), np.int64)
    return table, table[np.argsort(jm.ZIGZAG)]


@pytest.mark.parametrize("quality", [1, 10, 25, 49, 50, 75, 90, 95, 100])
def test_tables_are_pillows(quality):
    im = decode(pillow_frame(jm.patterns(1, 16, 16)["noise"][0], quality))
    ours, theirs = jm.quant_tables(quality), im.quantization
    for i in (0, 1):
        assert any(np.array_equal(ours[i], t) for t in to_row_major(theirs[i])), (quality, i)
        assert tuple(int(v) for v in ours[i]) == mjpeg.quant_tables(quality)[i]
    # and the tables in our DQT segments are, byte for byte, the tables in Pillow's
    pil = pillow_frame(jm.patterns(1, 16, 16)["noise"][0], quality)
    assert dqt_tables(jm.jpeg_frame(16, 16, *ours, 1, b"")) == dqt_tables(pil) and len(dqt_tables(pil)) == 2


def test_huffman_tables_are_pillows_and_the_kernels():
    """Pillow writes the typical tables of Annex K when it does not optimise: our four DHT segments equal its bytes; the arrays in
    csrc/mjpeg.hip, the DCT table and the zigzag there equal the model's."""
    pil = pillow_frame(jm.patterns(1, 16, 16)["noise"][0], 75)
    ours = mjpeg.jpeg_frame(16, 16, mjpeg.quant_tables(75), 1, b"")
    for cls_id, (bits, vals) in ((0x00, jm.DC_LUMA), (0x10, jm.AC_LUMA), (0x01, jm.DC_CHROMA), (0x11, jm.AC_CHROMA)):
        body = bytes([cls_id]) + bytes(bits) + bytes(vals)
        assert body in pil and body in ours, hex(cls_id)
    src = open(os.path.join(ROOT, "vface_amd", "csrc", "mjpeg.hip")).read()

    def ints(name):
        body = re.search(name + r"(?:\[\d+\])+ = \{(.*?)\};", src, flags=re.S).group(1)
        return [int(v, 0) for v in re.findall(r"-?(?:0x[0-9A-Fa-f]+|\d+)", body)]
    assert ints("kDct") == jm.C.reshape(-1).tolist() and ints("kZigzag") == jm.ZIGZAG.tolist()
    assert ints("kDcBits") == jm.DC_LUMA[0] + jm.DC_CHROMA[0] and ints("kAcBits") == jm.AC_LUMA[0] + jm.AC_CHROMA[0]
    assert ints("kAcVals") == jm.AC_LUMA[1] + jm.AC_CHROMA[1]
    assert jm.ZIGZAG.tolist() == list(mjpeg.ZIGZAG)
    assert int(re.search(r"kRecipShift = (\d+)", src).group(1)) == jm.RECIP_SHIFT


def defect_is_seen(defect) -> bool:
    """By one of the checks above: the bound against the definition, Pillow's decoder (raises, or another size), the error
    against Pillow's encoder."""
    for W, H in BIG:
        pats = jm.patterns(1, W, H)
        for name in ("smooth", "noise", "edges"):
            for quality in QUALITIES:
                if bound_violations(pats[name], quality, defect):
                    return True
                try:
                    frame = jm.encode_frames(pats[name], quality, 3, defect)[0]
                    if decode(frame).size != (W, H) or mse_ratio(pats[name][0], quality, 3, defect) > MSE_BOUND:
                        return True
                except Exception:
                    return True
    return False


@pytest.mark.parametrize("defect", jm.DEFECTS)
def test_seeded_defect_is_seen(defect):
    assert defect_is_seen(defect), defect


def test_value_ranges_and_the_reciprocal_multiply():
    """Every sum inside int32, |DC| <= 1024, |AC| <= 1023 (asserted in the model); and for every divisor d = Q << 15 a quality of
    1..100 produces -- in fact every Q in 1..255 -- and every dividend the transform can reach, the kernel's multiply by
    ceil(2^20 / Q) and shift equals the division, inside 32 bits."""
    r = jm.value_ranges()
    used = sorted({int(v) for quality in range(1, 101) for t in jm.quant_tables(quality) for v in t})
    assert used[0] == 1 and used[-1] == 255
    n = np.arange(r["n_peak"] + 1, dtype=np.int64)
    for Q in range(1, 256):
        m = int(jm.reciprocal(Q))
        assert int(n[-1]) * m < 2 ** 32
        assert np.array_equal((n * m) >> jm.RECIP_SHIFT, n // Q), Q
    # the form with d itself, as the issue states it, is the same number
    c = np.random.default_rng(0).integers(-r["c_peak"], r["c_peak"] + 1, 100000)
    for Q in (1, 2, 3, 17, 99, 255):
        d = Q << 15
        assert np.array_equal(np.sign(c) * ((np.abs(c) + (d >> 1)) // d), jm.quantise(c, np.int64(Q)))


def model_clip(F=3, W=48, H=32, quality=90):
    rgb = jm.patterns(F, W, H)["smooth"]
    return rgb, jm.encode_frames(rgb, quality, jm.mcu_grid(W, H)[1])


def test_avi_round_trip(tmp_path):
    """The model's file through the walker (sizes add up, even padding, index -> 00dc chunks, counts); the frames come back and
    decode; the writer, fed the same frames chunk by chunk, writes the same file byte for byte."""
    W, H = 48, 32
    rgb, frames = model_clip()
    data = jm.avi_file(frames, W, H)
    got = jm.walk_riff(data)
    assert got["frames"] == frames and got["avih"][4] == 3 and got["avih"][0] == 100000 and got["avih"][8:10] == (W, H)
    assert got["strh"]["type"] == b"vids" and got["strh"]["handler"] == b"MJPG" and (got["strh"]["scale"], got["strh"]["rate"]) == (1, 10)
    assert got["strf"]["compression"] == b"MJPG" and (got["strf"]["W"], got["strf"]["H"], got["strf"]["size"]) == (W, H, 40)
    assert got["avih"][7] == got["strh"]["buffer"] == max(len(f) for f in frames)
    for f in got["frames"]:
        assert decode(f).size == (W, H)
    # chunks of odd and of even size: the odd one is padded (the walker asserts the pad byte and that the sizes add up)
    mixed = jm.avi_file([b"abc", b"abcd", b"a"], W, H)
    assert jm.walk_riff(mixed)["frames"] == [b"abc", b"abcd", b"a"] and len(mixed) % 2 == 0
    path = str(tmp_path / "w.avi")
    w = mjpeg.MJPEGWriter(path, W, H)
    for f in frames:
        w._append(f)
    assert w.frames == 3
    w.close()
    w.close()
    assert open(path, "rb").read() == data
    empty = str(tmp_path / "e.avi")
    mjpeg.MJPEGWriter(empty, W, H).close()
    assert open(empty, "rb").read() == jm.avi_file([], W, H) and jm.walk_riff(open(empty, "rb").read())["frames"] == []


def test_frame_assembly_equals_the_models():
    for W, H, quality, restart in ((1, 1, 50, 1), (250, 136, 90, 16), (65535, 3, 100, 65535)):
        scan = bytes(range(7))
        assert mjpeg.jpeg_frame(W, H, mjpeg.quant_tables(quality), restart, scan) == jm.jpeg_frame(W, H, *jm.quant_tables(quality), restart, scan)
    for bad in ((0, 1, 1), (65536, 1, 1), (1, 1, 0), (1, 1, 65536)):
        with pytest.raises(ValueError):
            mjpeg.jpeg_header(bad[0], bad[1], mjpeg.quant_tables(90), bad[2])
    for quality in (0, 101):
        with pytest.raises(ValueError):
            mjpeg.quant_tables(quality)


def test_writer_refuses_what_it_cannot_write(tmp_path):
    path = str(tmp_path / "r.avi")
    assert mjpeg.MJPEGWriter.__init__.__defaults__ == (10, 90)
    for bad in (dict(quality=0), dict(quality=101), dict(fps=0)):
        with pytest.raises(ValueError):
            mjpeg.MJPEGWriter(path, 4, 2, **bad)
    with mjpeg.MJPEGWriter(path, 4, 2) as w:
        with pytest.raises(hip.VFaceHipError, match="device tensors"):
            w.write(torch.zeros(1, 2, 4, 3, dtype=torch.uint8))
        with pytest.raises(hip.VFaceHipError):
            w.write(np.zeros((1, 2, 4, 3), np.uint8))
        # 4 GiB: refused BEFORE the frame that would break the file; what was written stays a valid file
        frame = jm.encode_frames(np.zeros((1, 2, 4, 3), np.uint8), 90, 1)[0]
        w._append(frame)
        w._f.flush()
        before, pos = os.path.getsize(path), w._pos
        # the finished file would be: the chunks so far, this chunk, the index of two entries; one byte past what the size field holds
        chunk_and_index = 8 + len(frame) + (len(frame) & 1) + 8 + 32
        w._pos = mjpeg.RIFF_LIMIT + 8 - chunk_and_index + 1
        with pytest.raises(ValueError, match="past 4 GiB"):
            w._append(frame)
        w._f.flush()
        assert w.frames == 1 and os.path.getsize(path) == before
        w._pos = pos
    assert len(jm.walk_riff(open(path, "rb").read())["frames"]) == 1
    with pytest.raises(ValueError, match="closed"):
        w.write(torch.zeros(1, 2, 4, 3, dtype=torch.uint8))


def test_wrappers_refuse_host_tensors():
    q = torch.ones(64, dtype=torch.uint8)
    with pytest.raises(hip.VFaceHipError):
        hip.jpeg_coefficients(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), q, q)
    with pytest.raises(hip.VFaceHipError):
        hip.jpeg_entropy(torch.zeros(1, 1, 1, 6, 64, dtype=torch.int16), 1)
    assert hip.jpeg_mcu_grid(250, 136) == jm.mcu_grid(250, 136) == (9, 16)
    lib = hip.load()
    assert lib.vface_jpeg_entropy_workspace_bytes(0, 1, 1) == 0
    need = lib.vface_jpeg_entropy_workspace_bytes(144, 3, 16)
    assert need >= 3 * 9 * 16 * 6 * hip.JPEG_BLOCK_BYTES_BOUND and hip.jpeg_scan_bytes_bound(144, 16) == 9 * 16 * 6 * 416 + 16


CLIP = ("--target_frames", "d", "--src_image", "s.png", "--landmarks", "l.npz", "--synthetic_weights")


def test_command_line_flags_and_refusals():
    p = cli.build_parser()
    none = p.parse_args([])
    assert (none.video_codec, none.video_quality) == (None, None)
    opt = p.parse_args(["--video_out", "o.avi", "--video_codec", "mjpeg", "--video_quality", "75"])
    assert (opt.video_out, opt.video_codec, opt.video_quality) == ("o.avi", "mjpeg", 75)
    with pytest.raises(SystemExit):
        p.parse_args(["--video_codec", "h264"])
    for args, message in ((("--video_codec", "mjpeg"), "--video_codec says how --video_out is written: it needs --video_out FILE"),
                          (("--video_codec", "y4m"), "--video_codec says how --video_out is written"),
                          (("--video_out", "o.y4m", "--video_quality", "80"), "--video_quality is the quantiser of the JPEG encoder: it needs --video_codec mjpeg"),
                          (("--video_out", "o.y4m", "--video_codec", "y4m", "--video_quality", "80"), "it needs --video_codec mjpeg"),
                          (("--video_out", "o.avi", "--video_codec", "mjpeg", "--video_quality", "0"), "1..100; got 0"),
                          (("--video_out", "o.avi", "--video_codec", "mjpeg", "--video_quality", "101"), "1..100; got 101")):
        for base in (CLIP, ("--synthetic",)):
            with pytest.raises(SystemExit) as e:
                cli.check_options(cli.normalise_options(p.parse_args(list(base + args))))
            assert message in str(e.value), (args, str(e.value))
    for args in (("--video_out", "o.y4m"), ("--video_out", "o.y4m", "--video_codec", "y4m"), ("--video_out", "o.avi", "--video_codec", "mjpeg"),
                 ("--video_out", "o.avi", "--video_codec", "mjpeg", "--video_quality", "1")):
        cli.check_options(cli.normalise_options(p.parse_args(list(CLIP + args))))
    # the sink picks the writer from the normalised options: None -> y4m, quality None -> 90
    from vface_amd.scripts.outputs import ClipOutputs
    for args, want in (((), ("y4m", None)), (("--video_codec", "mjpeg"), ("mjpeg", None)), (("--video_codec", "mjpeg", "--video_quality", "55"), ("mjpeg", 55))):
        opt = cli.normalise_options(p.parse_args(["--video_out", "o", "--skip_save", "--Base_dir", "."] + list(args)))
        sink = ClipOutputs(opt)
        assert (sink.codec, sink.quality) == want
    assert mjpeg.DEFAULT_QUALITY == 90
