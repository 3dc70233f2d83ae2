"""The Motion-JPEG way in without a GPU: the decoder model (tests/jpeg_decode_model.py) against the encoder model, against Pillow
(libjpeg-turbo) and against its fp64 definition; its seeded defects; the header parser and the AVI reader of
vface_amd/scripts/mjpeg_in.py; the interval decoder of csrc/jpeg_interval.hpp as a host program under sanitizers."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import demux_model as dm
import jpeg_decode_model as jdm
import jpeg_model as jm
import mjpeg_in_cases as cases
from conftest import ROOT
from vface_amd.scripts import demux, mjpeg, mjpeg_in

CSRC = os.path.join(ROOT, "vface_amd", "csrc")
EPS = jdm.definition_bound()
# model pixel against the ROUNDED fp64 value: both are integers, the model lies within 0.5 + EPS of the value before rounding
MODEL_LEVELS = int(np.floor(0.5 + EPS + 0.5))
# worst |model RGB - Pillow RGB| measured over every frame of cases.pillow_frames() is 3 levels (mean squared difference at most
# 0.41 on a frame of more than one pixel; 1.33 on the 1 x 1 frame, whose three values differ by 2, 0, 0): libjpeg's colour tables
# round the Cb and Cr products separately and its upsampling rounds on its own, demux_model rounds once.  The bound is that + 1.
RGB_MEASURED, RGB_BOUND = 3, 4
# Pillow's own distance from the rounded fp64 value may not exceed one level on any test input.  Its chroma planes are seen only
# behind libjpeg's h2v2 "fancy" upsampling, so both sides of the chroma comparison go through ``jdm.libjpeg_upsample``: the (3, 1)/4
# weights with libjpeg's own rounding.  Its weights are non-negative, sum to 16 and end in one floor, so samples that differ by at
# most k levels give upsampled values that differ by at most k: the allowances of the samples carry over unchanged.
PILLOW_LEVELS = 1


# ---- round trip with the encoder's model
def test_round_trip_with_the_encoder_model():
    """jpeg_model.coefficients -> scan_bytes -> decode_scan gives the coefficients back bit for bit: every SIZES entry at restart 1,
    one MCU row and more than the frame, and every constructed entropy case."""
    streams = cases.round_trip_streams()
    assert len(streams) >= 3 * len(cases.SIZES) + len(cases.entropy_cases())
    for name, coef, restart, scan in streams:
        got, status = jdm.decode_scan(scan, coef.shape[0], restart, cases.ANNEX_K)
        assert status == jdm.OK, (name, jdm.STATUS[status])
        assert got.dtype == np.int16 and np.array_equal(got, coef), name
    wraps = [s for s in streams if s[0].startswith("rst_wraps")][0]
    assert len(jdm.split_intervals(wraps[3], wraps[1].shape[0], wraps[2])[0]) == 10


# ---- against Pillow
def pillow_planes(jpeg):
    im = Image.open(io.BytesIO(jpeg))
    im.draft("YCbCr", im.size)
    im.load()
    assert im.mode == "YCbCr"
    return np.asarray(im).astype(np.int64)


def compare_with_pillow(name, W, H, jpeg, coef, quant, defect=None):
    """One frame: the model's planes against Pillow's Y'CbCr decode, then the RGB.  -> (worst RGB difference, its mean square)."""
    rows = jdm.planes(coef[None], quant[None], W, H, defect)
    y, cb, cr = jdm.assemble(jdm.inverse_dct(jdm.dequantise(coef[None], quant[None], defect), defect), W, H)
    ref = np.clip(np.rint(jdm.fp64_pixels(coef[None], quant[None])), 0, 255).astype(np.int64)     # the rounded fp64 value, per sample
    ry, rcb, rcr = jdm.assemble(ref, W, H)
    pil = pillow_planes(jpeg)
    up = jdm.libjpeg_upsample
    for plane, (mine, want, theirs) in {"Y": (y[0], ry[0], pil[..., 0]), "Cb": (up(cb, W, H)[0], up(rcb, W, H)[0], pil[..., 1]),
                                        "Cr": (up(cr, W, H)[0], up(rcr, W, H)[0], pil[..., 2])}.items():
        pillow_own = np.abs(theirs - want).max()
        if defect is None:
            # a condition on the INPUTS: libjpeg's own inverse DCT stays within a level of the rounded definition
            assert pillow_own <= PILLOW_LEVELS, (name, plane, pillow_own)
        assert np.abs(mine - theirs).max() <= MODEL_LEVELS + pillow_own, (name, plane, np.abs(mine - theirs).max(), pillow_own)
    rgb = dm.i420_to_rgb(rows, W, H, "bt601", True, "centre")[0].astype(np.int64)
    want = np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB")).astype(np.int64)
    diff = np.abs(rgb - want)
    assert diff.max() <= RGB_BOUND, (name, diff.max())
    return int(diff.max()), float((diff ** 2).mean())


def test_model_against_pillow():
    decoded = cases.decoded_pillow_frames()
    assert len(decoded) == len(cases.VARIANTS) * len(cases.PILLOW_SIZES)
    worst, worst_mse = 0, 0.0
    for name, W, H, jpeg in cases.pillow_frames():
        coef, status, quant, w, h = decoded[name]
        assert status == jdm.OK and (w, h) == (W, H), (name, status)
        peak, mse = compare_with_pillow(name, W, H, jpeg, coef, quant)
        worst, worst_mse = max(worst, peak), max(worst_mse, mse)
    print(f"worst RGB difference {worst} levels, worst mean squared difference {worst_mse:.3f}")
    assert worst == RGB_MEASURED, worst         # the constant above cites what is measured here


def test_the_pillow_frames_are_what_they_promise():
    frames = {name: jpeg for name, W, H, jpeg in cases.pillow_frames()}
    marks = lambda j, m: [s for s in cases.segments(j) if s[0] == m]
    assert not marks(frames["no_dht_250x136_smooth"], 0xC4) and len(marks(frames["q90_250x136_smooth"], 0xC4)) >= 1
    j = frames["merged_tables_130x50_smooth"]
    assert len(marks(j, 0xDB)) == 1 and len(marks(j, 0xC4)) == 1
    assert len(mjpeg_in.parse_jpeg(j).quant) == 2 and mjpeg_in.parse_jpeg(j).huffman[(1, 1)] != tuple(map(tuple, jm.AC_CHROMA))
    assert marks(frames["com_app1_9x17_smooth"], 0xFE) and marks(frames["com_app1_9x17_smooth"], 0xE1)
    assert mjpeg_in.parse_jpeg(frames["restart_blocks_250x136_smooth"]).restart == 3
    assert mjpeg_in.parse_jpeg(frames["restart_rows_250x136_edges"]).restart == 16
    assert mjpeg_in.parse_jpeg(frames["q90_9x17_edges"]).restart == 0
    own = mjpeg_in.parse_jpeg(frames["qtables_130x50_edges"]).quant
    assert own[0].tolist() != jm.quant_tables(75)[0].tolist() and sorted(own) == [0, 1]
    assert mjpeg_in.parse_jpeg(frames["optimize_250x136_noise"]).huffman[(1, 0)] != (tuple(jm.AC_LUMA[0]), tuple(jm.AC_LUMA[1]))


# ---- the model against its definition
@pytest.mark.parametrize("quality", [30, 90, 100])
def test_model_against_the_fp64_definition(quality):
    """On random coefficients an encoder can produce the model stays within 0.5 + eps of the fp64 definition; eps is derived from
    the table's residues (``definition_bound``), not fitted."""
    assert 0.0 < EPS < 0.2
    coef, quant = jdm.legal_coefficients(np.random.default_rng(quality), quality, 6 * 400)
    exact = jdm.fp64_pixels(coef, quant)
    gap = np.abs(jdm.model_pixels_unrounded(coef, quant) - exact).max()
    print(f"quality {quality}: before the last rounding {gap:.4f} of {EPS:.4f}")
    assert gap <= EPS
    got = jdm.inverse_dct(jdm.dequantise(coef, quant))
    assert np.abs(got - np.clip(exact, 0, 255)).max() <= 0.5 + EPS
    assert np.abs(jdm.dequantise(coef, quant)).max() <= jdm.value_ranges()["legal_d"]


def test_every_sum_fits_int32_for_every_coefficient():
    r = jdm.value_ranges()
    assert max(r["product_peak"], r["pass1_peak"], r["pass2_peak"]) < 2 ** 31
    # the corners of the box, through the model: the extremes are reached inside what value_ranges allows
    quant = np.full((1, 3, 64), 255, np.uint8)
    for sign in (np.ones(64), -np.ones(64), np.sign(jdm.C[:, 0][:, None] * jdm.C[:, 0][None, :]).reshape(64)[np.argsort(jm.ZIGZAG)]):
        coef = (sign * 32767).astype(np.int16).reshape(1, 1, 1, 64).repeat(6, axis=2)
        d = jdm.dequantise(coef, quant)
        assert d.min() >= jdm.D_MIN and d.max() <= jdm.D_MAX
        s1 = np.einsum("vm,...vu->...mu", jdm.C, d)
        assert np.abs(s1).max() + (1 << 10) <= r["pass1_peak"]
        t = np.clip((s1 + (1 << 10)) >> 11, jdm.T_MIN, jdm.T_MAX)
        assert np.abs(np.einsum("un,...mu->...mn", jdm.C, t)).max() + (1 << 18) <= r["pass2_peak"]
        assert set(np.unique(jdm.inverse_dct(d))) <= set(range(256))


def test_kernel_constants_equal_the_model():
    src = open(os.path.join(CSRC, "mjpeg_in.hip")).read()
    body = src[src.index("constexpr int kIdct[8][8]"):]
    body = body[body.index("=") + 1:body.index(";")]
    table = np.array([int(v) for v in body.replace("{", " ").replace("}", " ").replace(",", " ").split()]).reshape(8, 8)
    assert np.array_equal(table, jdm.C)
    for text in (f"kDequantMax = {jdm.D_MAX};", f"kPass1Shift = {jdm.PASS1_SHIFT}, kPass1Max = {jdm.T_MAX};", f"kPass2Shift = {jdm.PASS2_SHIFT};"):
        assert text in src, text
    header = open(os.path.join(CSRC, "jpeg_interval.hpp")).read()
    for code, name in enumerate(("OK", "MARKER_COUNT", "MARKER_ORDER", "SHORT", "BAD_CODE", "DC_CATEGORY", "AC_SIZE", "RUN", "RANGE")):
        assert f"VF_JPEG_{name} = {code}," in header and jdm.STATUS[code] == name.lower()
    from vface_amd import hip
    assert sorted(hip.JPEG_STATUS) == list(range(9)) and hip.JPEG_TABLE_BYTES == mjpeg_in.TABLE_BYTES == 2304


# ---- seeded defects
def test_every_seeded_defect_is_seen():
    """Each defect of the model fails at least one of the assertions above: the round trip, or the comparison with Pillow."""
    streams = [s for s in cases.round_trip_streams() if s[0].split("_")[0] in ("250x136", "dc", "zero", "ff", "rst", "every")]
    frames = [f for f in cases.pillow_frames() if f[0] in ("q90_250x136_smooth", "restart_rows_130x50_smooth", "q30_130x50_edges")]
    assert len(frames) == 3 and len(streams) >= 8
    for defect in jdm.DEFECTS:
        seen = False
        for name, coef, restart, scan in streams:
            got, status = jdm.decode_scan(scan, coef.shape[0], restart, cases.ANNEX_K, defect)
            if status or not np.array_equal(got, coef):
                seen = True
                break
        for name, W, H, jpeg in () if seen else frames:
            coef, status, quant, _, _ = cases.decoded_pillow_frames()[name]
            try:
                compare_with_pillow(name, W, H, jpeg, coef, quant, defect)
            except AssertionError:
                seen = True
                break
        assert seen, f"defect {defect!r} passes every assertion"
    assert len(jdm.DEFECTS) >= 12


# ---- the parser
def base_frame(W=32, H=16, restart=2):
    coef = jm.coefficients(jm.patterns(1, W, H, seed=2)["smooth"], *jm.quant_tables(80))
    return jm.jpeg_frame(W, H, *jm.quant_tables(80), restart, jm.scan_bytes(coef[0], restart))


def replace_segment(jpeg, marker, new, which=0):
    segs = [s for s in cases.segments(jpeg) if s[0] == marker]
    _, lo, hi = segs[which]
    return jpeg[:lo] + new + jpeg[hi:]


def seg(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def test_parser_reads_what_it_promises():
    jpeg = base_frame()
    f = mjpeg_in.parse_jpeg(jpeg, "a.avi", 0)
    assert (f.W, f.H, f.restart) == (32, 16, 2) and [c[3:] for c in f.components] == [(0, 0, 0), (1, 1, 1), (1, 1, 1)]
    assert f.quant[0].tolist() == jm.quant_tables(80)[0].tolist() and f.quant[1].tolist() == jm.quant_tables(80)[1].tolist()
    assert jpeg[f.scan[0]:f.scan[1]] + b"\xFF\xD9" == jpeg[f.scan[0]:] and jpeg[f.scan[0] - 14:f.scan[0] - 12] == b"\xFF\xDA"
    assert f.huffman[(0, 0)] == (tuple(jm.DC_LUMA[0]), tuple(jm.DC_LUMA[1])) and f.huffman[(1, 1)] == (tuple(jm.AC_CHROMA[0]), tuple(jm.AC_CHROMA[1]))
    # without EOI the scan runs to the end of the chunk; DRI 0 = none; no DHT = Annex K; any legal order of the segments
    assert mjpeg_in.parse_jpeg(jpeg[:-2]).scan == (f.scan[0], len(jpeg) - 2)
    assert mjpeg_in.parse_jpeg(replace_segment(jpeg, 0xDD, seg(0xDD, b"\0\0"))).restart == 0
    assert mjpeg_in.parse_jpeg(cases.without(jpeg, 0xDD)).restart == 0
    assert mjpeg_in.parse_jpeg(cases.without(jpeg, 0xC4)).huffman == f.huffman
    segs = cases.segments(jpeg)
    shuffled = jpeg[:2] + b"".join(jpeg[lo:hi] for _, lo, hi in reversed(segs[:-1])) + jpeg[segs[-1][1]:]
    g = mjpeg_in.parse_jpeg(shuffled)
    assert (g.W, g.H, g.restart, g.huffman) == (32, 16, 2, f.huffman) and shuffled[g.scan[0]:g.scan[1]] == jpeg[f.scan[0]:f.scan[1]]
    assert mjpeg_in.parse_jpeg(cases.with_extra_segments(cases.merged(cases.merged(jpeg, 0xDB), 0xC4))).huffman == f.huffman
    # SOF1 with 8-bit samples and 8-bit tables is the same stream
    assert mjpeg_in.parse_jpeg(jpeg.replace(b"\xFF\xC0\x00\x11", b"\xFF\xC1\x00\x11")).W == 32
    # a table block the decoder reads: maxcode / valoff of T.81 F.2.2.3
    block = mjpeg_in.huffman_block(f)
    assert block.dtype == np.uint8 and block.shape == (mjpeg_in.TABLE_BYTES,)
    words = block[:128].view(np.int32)
    assert words[:4].tolist() == [-1, 0, 6, 14] and words[16:20].tolist() == [0, 0, -1, -8] and block[128:140].tolist() == list(range(12))


def test_parser_refuses_by_name():
    jpeg = base_frame()
    sof = [s for s in cases.segments(jpeg) if s[0] == 0xC0][0]
    sof_body = jpeg[sof[1] + 4:sof[2]]
    sos = [s for s in cases.segments(jpeg) if s[0] == 0xDA][0]

    def with_sof(body, marker=0xC0):
        return jpeg[:sof[1]] + seg(marker, body) + jpeg[sof[2]:]

    def sampling(*hv):
        comps = b"".join(bytes([i + 1, h << 4 | v, min(i, 1)]) for i, (h, v) in enumerate(hv))
        return with_sof(sof_body[:5] + bytes([len(hv)]) + comps)
    refusals = {
        "progressive (SOF2)": with_sof(sof_body, 0xC2),
        "lossless (SOF3)": with_sof(sof_body, 0xC3),
        "arithmetic coding (SOF9)": with_sof(sof_body, 0xC9),
        "arithmetic coding (a DAC segment)": jpeg[:sof[1]] + seg(0xCC, b"\0\0") + jpeg[sof[1]:],
        "sample precision 12": with_sof(bytes([12]) + sof_body[1:]),
        "quantisation table 1 has 16-bit entries": replace_segment(jpeg, 0xDB, seg(0xDB, bytes([0x11]) + bytes(128)), 1),
        "4:2:2: only 4:2:0": sampling((2, 1), (1, 1), (1, 1)),
        "4:4:4: only 4:2:0": sampling((1, 1), (1, 1), (1, 1)),
        "greyscale: only 4:2:0": sampling((1, 1)),
        "sampling 4x1 1x1 1x1: only 4:2:0": sampling((4, 1), (1, 1), (1, 1)),
        "a scan of 1 component(s)": jpeg[:sos[1]] + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + jpeg[sos[2]:],
        "a scan with Ss = 1, Se = 63": jpeg[:sos[1]] + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 1, 63, 0])) + jpeg[sos[2]:],
        "Ah/Al = 0x01": jpeg[:sos[1]] + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 1])) + jpeg[sos[2]:],
        "more than one scan": jpeg[:-2] + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])) + b"\x00\xFF\xD9",
        "a DNL segment": jpeg[:-2] + seg(0xDC, b"\0\x10") + b"\xFF\xD9",
        "the frame height is left to a DNL segment": with_sof(sof_body[:1] + b"\0\0" + sof_body[3:]),
        "an AVI1 segment with polarity 1": jpeg[:2] + seg(0xE0, b"AVI1\x01" + bytes(9)) + jpeg[2:],
        "names Huffman table (class 1, id 2)": jpeg[:sos[1]] + seg(0xDA, bytes([3, 1, 0x02, 2, 0x11, 3, 0x11, 0, 63, 0])) + jpeg[sos[2]:],
        "names quantisation table 1": cases.without(jpeg, 0xDB)[:2] + seg(0xDB, bytes([0]) + bytes([9] * 64)) + cases.without(jpeg, 0xDB)[2:],
        "no JPEG start-of-image marker": b"RIFF" + jpeg,
        "truncated frame": jpeg[:sof[1] + 7],
        "is no prefix code": replace_segment(jpeg, 0xC4, seg(0xC4, bytes([0x00, 3] + [0] * 15 + [0, 1, 2]))),
    }
    for words, data in refusals.items():
        with pytest.raises(SystemExit) as e:
            mjpeg_in.parse_jpeg(data, "clip.avi", 7)
        message = str(e.value)
        assert message.startswith("clip.avi: frame 7: ") and words in message, (words, message)
        if "4:2:0" in words or "progressive" in words:
            assert mjpeg_in.FFMPEG_LINE in message
    assert mjpeg_in.FFMPEG_LINE == "ffmpeg -i in -c:v mjpeg -pix_fmt yuvj420p clip.avi"
    # AVI1 with polarity 0 is a whole frame
    assert mjpeg_in.parse_jpeg(jpeg[:2] + seg(0xE0, b"AVI1\x00" + bytes(9)) + jpeg[2:]).W == 32
    # the tables are imported from the writer, not copied
    assert mjpeg_in.ZIGZAG is mjpeg.ZIGZAG and mjpeg_in.DHT is mjpeg.DHT


# ---- the reader
def clip_frames(n=3, W=32, H=16):
    rgb = jm.patterns(n, W, H, seed=4)["smooth"]
    return jm.encode_frames(rgb, 90, 2), W, H


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def rebuild(frames, W, H, movi_chunks, with_index=True, handler=b"MJPG", compression=b"MJPG"):
    """An AVI like jpeg_model.avi_file's with the 'movi' list made of ``movi_chunks`` [(fourcc, payload)]."""
    data = jm.avi_file(frames, W, H)
    movi_at = data.index(b"movi") - 8
    head = data[:movi_at].replace(b"vidsMJPG", b"vids" + handler).replace(b"\x18\x00MJPG", b"\x18\x00" + compression)
    movi, idx = bytearray(b"movi"), bytearray()
    for fourcc, payload in movi_chunks:
        idx += fourcc + struct.pack("<III", 0x10, len(movi), len(payload))
        movi += jm._chunk(fourcc, payload)
    body = head[8:] + jm._chunk(b"LIST", bytes(movi)) + (jm._chunk(b"idx1", bytes(idx)) if with_index else b"")
    return b"RIFF" + struct.pack("<I", len(body)) + body


def scans_of(read):
    return [r.scan for r in read.records]


def test_reader_walks_the_files(tmp_path):
    frames, W, H = clip_frames()
    want = [f[mjpeg_in.parse_jpeg(f).scan[0]:-2] for f in frames]
    with mjpeg_in.MJPEGReader(write(tmp_path / "a.avi", jm.avi_file(frames, W, H, fps=25))) as r:
        assert (r.W, r.H, len(r), r.fps, r.path, r.fixed_matrix) == (W, H, 3, (25, 1), str(tmp_path / "a.avi"), "bt601")
        got = r.read([2, 0, 1, 0])
        assert scans_of(got) == [want[2], want[0], want[1], want[0]] and got.indices == [2, 0, 1, 0] and len(got) == 4
        p = got.packed()
        assert p["lengths"].tolist() == [len(want[i]) for i in (2, 0, 1, 0)] and p["offsets"].tolist() == np.cumsum([0] + [len(want[i]) for i in (2, 0, 1)]).tolist()
        assert p["scans"].numpy().tobytes()[:sum(p["lengths"].tolist())] == want[2] + want[0] + want[1] + want[0]
        assert p["restart"].tolist() == [2] * 4 and tuple(p["quant"].shape) == (4, 3, 64) and tuple(p["tables"].shape) == (4, 2304)
        assert p["quant"][0, 0].tolist() == jm.quant_tables(90)[0].tolist() and p["quant"][0, 2].tolist() == jm.quant_tables(90)[1].tolist()
        # what ClipInputs.batch does with the rows of a read
        other = got.clone()
        other[1] = r.read([2])[0]
        assert scans_of(other)[1] == want[2] and scans_of(got)[1] == want[0]
        with pytest.raises(IndexError):
            r.read([3])
    with pytest.raises(ValueError):
        r.read([0])
    chunks = [(b"00dc", f) for f in frames]
    # no index: the 'movi' list is walked; audio chunks and 'rec ' framing are skipped; an index that names the audio too
    for name, data in (("noidx", rebuild(frames, W, H, chunks, with_index=False)),
                       ("audio", rebuild(frames, W, H, [chunks[0], (b"01wb", b"\1\2\3"), chunks[1], (b"01wb", b"\4\5"), chunks[2]])),
                       ("audio_noidx", rebuild(frames, W, H, [chunks[0], (b"01wb", b"\1\2\3"), chunks[1], chunks[2]], with_index=False)),
                       ("db", rebuild(frames, W, H, [(b"00db", f) for f in frames])),
                       ("case", rebuild(frames, W, H, chunks, handler=b"mjpg", compression=b"\0\0\0\0"))):
        with mjpeg_in.MJPEGReader(write(tmp_path / f"{name}.avi", data)) as r:
            assert len(r) == 3 and scans_of(r.read([0, 1, 2])) == want, name
    rec = jm.avi_file(frames, W, H)
    movi_at = rec.index(b"movi")
    inner = rec[movi_at + 4:rec.index(b"idx1")]
    grouped = rec[:movi_at - 4] + struct.pack("<I", len(inner) + 16) + b"movi" + b"LIST" + struct.pack("<I", len(inner) + 4) + b"rec " + inner
    grouped = b"RIFF" + struct.pack("<I", len(grouped) - 8) + grouped[8:]
    with mjpeg_in.MJPEGReader(write(tmp_path / "rec.avi", grouped)) as r:
        assert scans_of(r.read([0, 1, 2])) == want
    # a zero-length chunk repeats the frame before it
    with mjpeg_in.MJPEGReader(write(tmp_path / "repeat.avi", rebuild(frames, W, H, [chunks[0], (b"00dc", b""), chunks[1]]))) as r:
        assert len(r) == 3 and scans_of(r.read([0, 1, 2])) == [want[0], want[0], want[1]]
    with mjpeg_in.MJPEGReader(write(tmp_path / "repeat_noidx.avi", rebuild(frames, W, H, [chunks[0], (b"00dc", b""), chunks[1]], with_index=False))) as r:
        assert scans_of(r.read([1, 2])) == [want[0], want[1]]
    with pytest.raises(SystemExit, match="frame 0 is an empty chunk"):
        mjpeg_in.MJPEGReader(write(tmp_path / "empty0.avi", rebuild(frames, W, H, [(b"00dc", b""), chunks[0]])))
    # per-frame tables and restart intervals are the frame's own
    pil = [cases.pillow_jpeg(jm.patterns(1, W, H, seed=i)["noise"][0], quality=q, optimize=o, restart_marker_blocks=b)
           for i, (q, o, b) in enumerate(((50, True, 0), (90, False, 1), (70, True, 2)))]
    with mjpeg_in.MJPEGReader(write(tmp_path / "mixed.avi", jm.avi_file(pil, W, H))) as r:
        p = r.read([0, 1, 2]).packed()
        assert p["restart"].tolist() == [0, 1, 2] and len({bytes(t.numpy()) for t in p["tables"]}) == 3 and len({bytes(t.numpy()) for t in p["quant"]}) == 3


def avi_with_odml_index(frames, W, H):
    """``jm.avi_file``'s file the way ffmpeg lays it out: an ``indx`` super-index (no entries in use) in the stream's ``strl``, a
    ``LIST odml`` with ``dmlh`` and a JUNK chunk in ``hdrl``, an ``ix00`` standard index at the end of ``movi`` -- and the ``idx1``."""
    n, biggest = len(frames), max(len(f) for f in frames)
    avih = struct.pack("<14I", 100000, biggest * 10, 0, 0x10, n, 0, 1, biggest, W, H, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIiI4H", 0, 0, 0, 0, 1, 10, 0, n, biggest, -1, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    indx = struct.pack("<HBBI4s3I", 4, 0, 0, 0, b"00dc", 0, 0, 0) + bytes(16 * 4)
    strl = jm._chunk(b"LIST", b"strl" + jm._chunk(b"strh", strh) + jm._chunk(b"strf", strf) + jm._chunk(b"indx", indx))
    odml = jm._chunk(b"LIST", b"odml" + jm._chunk(b"dmlh", struct.pack("<I", n) + bytes(244)))
    hdrl = jm._chunk(b"LIST", b"hdrl" + jm._chunk(b"avih", avih) + strl + odml) + jm._chunk(b"JUNK", bytes(11))
    movi, idx, ix = bytearray(b"movi"), bytearray(), bytearray()
    for f in frames:
        idx += b"00dc" + struct.pack("<III", 0x10, len(movi), len(f))
        ix += struct.pack("<II", len(movi) + 8, len(f))
        movi += jm._chunk(b"00dc", f)
    movi += jm._chunk(b"ix00", struct.pack("<HBBI4sQI", 2, 0, 1, n, b"00dc", 0, 0) + bytes(ix))
    body = b"AVI " + hdrl + jm._chunk(b"LIST", bytes(movi)) + jm._chunk(b"idx1", bytes(idx))
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_reader_reads_a_one_riff_file_that_carries_opendml_indexes(tmp_path):
    """``indx`` / ``ix00`` / ``LIST odml`` in a file that ends in its first RIFF are index data: the frames are read, from ``idx1`` and
    from a walk of ``movi`` alike (``ix00`` is no frame).  The same file continued in ``AVIX`` is refused."""
    frames, W, H = clip_frames()
    want = [f[mjpeg_in.parse_jpeg(f).scan[0]:-2] for f in frames]
    data = avi_with_odml_index(frames, W, H)
    assert all(tag in data for tag in (b"indx", b"ix00", b"odml", b"dmlh", b"JUNK", b"idx1"))
    with mjpeg_in.MJPEGReader(write(tmp_path / "odml1.avi", data)) as r:
        assert (r.W, r.H, len(r), r.fps) == (W, H, 3, (10, 1)) and scans_of(r.read([0, 1, 2])) == want
    cut = data[:data.index(b"idx1")]
    with mjpeg_in.MJPEGReader(write(tmp_path / "odml1_noidx.avi", b"RIFF" + struct.pack("<I", len(cut) - 8) + cut[8:])) as r:
        assert len(r) == 3 and scans_of(r.read([0, 1, 2])) == want
    with pytest.raises(SystemExit, match="'AVIX' chunks \\(OpenDML"):
        mjpeg_in.MJPEGReader(write(tmp_path / "odml2.avi", data + b"RIFF" + struct.pack("<I", 4) + b"AVIX"))


def test_reader_refuses_by_name(tmp_path):
    frames, W, H = clip_frames()
    good = jm.avi_file(frames, W, H)
    chunks = [(b"00dc", f) for f in frames]
    with pytest.raises(SystemExit, match="'AVIX' chunks \\(OpenDML"):
        mjpeg_in.MJPEGReader(write(tmp_path / "odml.avi", good + b"RIFF" + struct.pack("<I", 4) + b"AVIX"))
    with pytest.raises(SystemExit, match="truncated"):
        mjpeg_in.MJPEGReader(write(tmp_path / "cut.avi", good[:len(good) // 2]))
    short = rebuild(frames, W, H, chunks, with_index=False)
    cut = short[:-40]
    cut = b"RIFF" + struct.pack("<I", len(cut) - 8) + cut[8:]
    with pytest.raises(SystemExit, match="truncated"):
        mjpeg_in.MJPEGReader(write(tmp_path / "cut2.avi", cut))
    with pytest.raises(SystemExit, match="not MJPG"):
        mjpeg_in.MJPEGReader(write(tmp_path / "h264.avi", rebuild(frames, W, H, chunks, handler=b"H264", compression=b"H264")))
    with pytest.raises(SystemExit, match="does not start with 'RIFF....AVI '.*ffmpeg -i in -c:v mjpeg"):
        mjpeg_in.MJPEGReader(write(tmp_path / "wave.avi", b"RIFF" + struct.pack("<I", 4) + b"WAVE"))
    with pytest.raises(SystemExit, match="no 'avih'"):
        mjpeg_in.MJPEGReader(write(tmp_path / "noavih.avi", good.replace(b"avih", b"JUNK")))
    with pytest.raises(SystemExit, match="no such file"):
        mjpeg_in.MJPEGReader(str(tmp_path / "nowhere.avi"))
    other = jm.encode_frames(jm.patterns(1, 48, 16, seed=4)["smooth"], 90, 2)
    with mjpeg_in.MJPEGReader(write(tmp_path / "sizes.avi", jm.avi_file(frames[:2] + other, W, H))) as r:
        assert len(r.read([0, 1])) == 2
        with pytest.raises(SystemExit, match="frame 2 is 48 x 16, frame 0 is 32 x 16"):
            r.read([2])
    grey = io.BytesIO()
    Image.fromarray(np.zeros((H, W), np.uint8)).save(grey, "JPEG")
    with mjpeg_in.MJPEGReader(write(tmp_path / "grey.avi", jm.avi_file(frames[:1] + [grey.getvalue()], W, H))) as r:
        with pytest.raises(SystemExit, match="frame 1: greyscale"):
            r.read([1])


def test_dispatch_is_by_content(tmp_path):
    frames, W, H = clip_frames()
    y4m = b"YUV4MPEG2 W4 H2 F25:1 Ip C420jpeg\n" + b"FRAME\n" + bytes(12)
    r = mjpeg_in.open_video(write(tmp_path / "really_y4m.avi", y4m))
    assert isinstance(r, demux.Y4MReader) and r.fixed_matrix is None and (r.W, r.H, len(r)) == (4, 2, 1)
    r.close()
    r = mjpeg_in.open_video(write(tmp_path / "really_avi.y4m", jm.avi_file(frames, W, H)))
    assert isinstance(r, mjpeg_in.MJPEGReader) and len(r) == 3
    r.close()
    with pytest.raises(SystemExit, match="does not start with 'YUV4MPEG2'"):
        mjpeg_in.open_video(write(tmp_path / "clip.mp4", b"\0\0\0\x18ftypmp42" + bytes(64)))
    with pytest.raises(SystemExit, match="no such file"):
        mjpeg_in.open_video(str(tmp_path / "nowhere.avi"))


def test_clip_inputs_over_the_reader(tmp_path):
    """ClipInputs.from_video over an MJPEGReader: the batches carry the reader's records, and a frame without landmarks takes the
    record of the frame before it, across a batch boundary too (``_read_again``)."""
    from test_clip_io_cpu import landmark_file
    from vface_amd.scripts import clip_io
    frames, W, H = clip_frames(4, 320, 240)
    lpath = str(tmp_path / "lm.npz")
    landmark_file(lpath)                                    # 4 frames, frame 2 without landmarks
    Image.fromarray(jm.patterns(1, 90, 100, seed=1)["smooth"][0]).save(tmp_path / "src.png")
    reader = mjpeg_in.MJPEGReader(write(tmp_path / "clip.avi", jm.avi_file(frames, W, H)))
    clip = clip_io.ClipInputs.from_video(reader, str(tmp_path / "src.png"), lpath, 4, 512, 512)
    b0, b1 = clip.batch(0, 2), clip.batch(1, 2)
    assert b0["crop_frames"] is b0["frames"] and b0["frames"].indices == [0, 1]
    assert b1["frames"].indices == [2, 3] and b1["crop_frames"].indices == [1, 3] and b1["crop_frames"] is not b1["frames"]
    reader.close()


# ---- the interval decoder under sanitizers
def interval_records():
    """[(scan, begin, end, table block, blocks, status, expected coefficients)] of every interval of the round-trip list, of the
    Pillow frames with tables of their own, and of the corruption cases."""
    def block(huffman):
        return np.concatenate([mjpeg_in.huffman_table(*t) for t in huffman[0]] + [mjpeg_in.huffman_table(*t) for t in huffman[1]])
    out = []

    def add(scan, mcus, restart, huffman):
        ranges, status = jdm.split_intervals(scan, mcus, restart)
        if status:
            return
        books = ([jdm.code_book(t) for t in huffman[0]], [jdm.code_book(t) for t in huffman[1]])
        step = mcus if restart <= 0 or restart >= mcus else restart
        for i, (begin, end) in enumerate(ranges):
            blocks = 6 * (min(i * step + step, mcus) - i * step)
            coef, code = jdm.decode_interval(scan, begin, end, books, blocks)
            out.append((scan, begin, end, block(huffman), blocks, code, coef))
    for name, coef, restart, scan in cases.round_trip_streams():
        add(scan, coef.shape[0], restart, cases.ANNEX_K)
    for name, W, H, jpeg in cases.pillow_frames():
        if name.split("_")[0] in ("optimize", "merged", "restart") and (W, H) != (250, 136) or name == "optimize_250x136_noise":
            frame = mjpeg_in.parse_jpeg(jpeg)
            add(jpeg[frame.scan[0]:frame.scan[1]], mjpeg_in.mcu_count(W, H), frame.restart, jdm.frame_tables(frame)[0])
    for name, (scan, mcus, restart, want) in cases.corruption_cases().items():
        add(scan, mcus, restart, cases.ANNEX_K)
    scan, huffman = cases.category12_tables()
    add(scan, 1, 0, huffman)
    return out


def test_interval_decoder_under_sanitizers(tmp_path):
    """csrc/jpeg_interval.hpp -- the function the kernel runs per lane -- as a host program with -fsanitize=address,undefined: the
    model's coefficients on the valid streams, the model's status on the corrupt ones, and 20 000 seeded mutations without a report.
    Every buffer is a heap allocation of exactly the promised size."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_interval_probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "jpeg_interval_probe.cpp"), "-o", exe], check=True)
    records = interval_records()
    statuses = {code for *_, code, _ in records}
    assert {jdm.OK, jdm.SHORT, jdm.BAD_CODE, jdm.RUN, jdm.DC_CATEGORY} <= statuses, statuses
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for scan, begin, end, block, blocks, code, coef in records:
            f.write(struct.pack("<I", len(scan)) + scan + struct.pack("<II", begin, end) + block.tobytes() + struct.pack("<II", blocks, code))
            f.write(np.ascontiguousarray(coef, np.int16).tobytes())
    done = subprocess.run([exe, path, "20000", "7"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    lines = done.stdout.splitlines()
    assert lines[0] == f"cases {len(records)} mutations 20000", lines[0]
    histogram = {int(l.split()[1][:-1]): int(l.split()[2]) for l in lines[1:]}
    assert sum(histogram.values()) == 20000 and histogram[jdm.OK] > 0 and histogram[jdm.SHORT] > 0 and histogram[jdm.BAD_CODE] > 0


def test_bindings_refuse_without_a_gpu():
    from vface_amd import hip
    scans = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(hip.VFaceHipError):
        hip.jpeg_scan_index(scans, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 1, 1)
    with pytest.raises(hip.VFaceHipError):
        hip.jpeg_planes(torch.zeros(1, 1, 6, 64, dtype=torch.int16), torch.ones(1, 3, 64, dtype=torch.uint8), 16, 16)
    with pytest.raises(hip.VFaceHipError):
        mjpeg_in.decode(mjpeg_in.MJPEGFrames("x.avi", 16, 16, []), "cuda")
    lib = hip.load()
    for name in ("vface_jpeg_scan_index", "vface_jpeg_decode_entropy", "vface_jpeg_planes"):
        assert name in hip.SIGNATURES and hasattr(lib, name)
    assert hip.jpeg_interval_count(144, 16) == 9 and hip.jpeg_interval_count(144, 0) == 1 and hip.jpeg_interval_count(5, 9) == 1
