"""The parallel inflate without a GPU: the protocol of tests/png_inflate_par_model.py held to the serial model on every stream of
tests/png_in_cases.py and 20 000 mutations at three chunk sizes, the conditions that show the parallel path is really taken, the
constructed corners of tests/png_inflate_par_cases.py, seeded defects of the model that must be seen, csrc/png_inflate_par.hpp's
host routine as a stand-alone program under sanitizers against the model, and the binding, the flag and ``inflate_path``."""
import os
import struct
import subprocess
import zlib

import pytest

import png_in_cases as cases
import png_inflate_model as im
import png_inflate_par_cases as pc
import png_inflate_par_model as pm
from test_png_in_cpu import CSRC, MUTATIONS, ROOT, host_compiler, probe_records

CHUNKS = pc.CHUNKS


def equals_serial(body, expect, chunk_bytes, defect=None):
    r = pm.inflate_parallel(body, expect, chunk_bytes, defect)
    status, produced, consumed, data = im.inflate(body, expect)
    return (r.status, r.produced, r.consumed, r.data) == (status, produced, consumed, data) and r.adler == im.adler_halves(data) and r


# ---- the model against the serial model
@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_model_equals_the_serial_model_on_every_stream(chunk_bytes):
    """zlib's streams, the constructed corners of the format, one stream per status and the further ways to them."""
    records = probe_records()[:-MUTATIONS]
    assert len(records) > 60
    taken = 0
    for body, expect in records:
        if expect == 0:
            continue                                    # (``only_end_of_block``: a file always expects a byte)
        r = equals_serial(body, expect, chunk_bytes)
        assert r, (chunk_bytes, expect, body[:32].hex())
        taken += r.info[0] > 1
    assert taken >= (1 if chunk_bytes < 4096 else 0)    # (some of them do run on more than one segment)


def test_model_equals_the_serial_model_on_mutations():
    """20 000 bodies with one bit flipped, byte changed, tail cut or byte inserted, at the three chunk sizes: status, produced,
    consumed, bytes and checksum are the serial model's, whether the file is accepted or falls back."""
    reasons = set()
    for body, expect in cases.mutations(MUTATIONS, 7):
        for chunk_bytes in CHUNKS:
            r = equals_serial(body, expect, chunk_bytes)
            assert r, (chunk_bytes, body.hex())
            reasons.add(r.info[1])
    assert {0, 2, 3} <= reasons, reasons


def test_quick_test_is_necessary_and_finds_no_false_candidate():
    """Every position that passes is among those the cheap test lets through, checked by brute force on a small stream; family A
    has no block start that is not a real one among its 84 k positions."""
    body = pc.corners()["candidate_on_first_and_last_bit"].body
    quick = set(pm.quick(body).tolist())
    real = [p for p in range(8 * len(body)) if pm.passes(body, p)]
    assert real == [0, 2048, 6143] and set(real) <= quick
    body, data = pc.family_a()
    starts, at, real = pm.block_starts(body), 0, []
    while True:                                     # the blocks' own starts, from the serial walk
        real.append(at)
        seg = pm.decode_segment(body, at, at + 1)
        assert seg.status == 0
        if seg.final:
            break
        at = seg.end
    bit = lambda p: body[p >> 3] >> (p & 7) & 1
    assert len(real) == 59 and list(starts) == [p for p in real if (bit(p + 1), bit(p + 2)) == (0, 1)] and len(starts) >= 58


# ---- the parallel path is taken
@pytest.mark.parametrize("family", ["a", "b"])
def test_families_take_the_parallel_path(family):
    body, data = pc.family_a() if family == "a" else pc.family_b()
    assert zlib.decompressobj(-15).decompress(body) == data
    r = pm.inflate_parallel(body, len(data), 256)
    assert (r.status, r.data, r.consumed) == (0, data, len(body)) and r.adler == im.adler_halves(data)
    assert r.info[1] == 0 and r.info[0] >= 8 and r.info[0] == r.info[2] + 1
    assert r.info[0] == (41 if family == "a" else 82)
    if family == "b":
        assert r.far >= 50 and r.hops >= 2          # references in front of their own segment; one through two earlier segments
    for chunk_bytes in (64, 4096):
        r = pm.inflate_parallel(body, len(data), chunk_bytes)
        assert r.info[1] == 0 and r.info[0] >= 3 and r.data == data


# ---- the protocol's corners
@pytest.mark.parametrize("name", sorted(pc.corners()))
def test_corners(name):
    case = pc.corners()[name]
    serial = im.inflate(case.body, case.expect)
    assert serial[0] == case.status
    for chunk_bytes in CHUNKS:
        r = pm.inflate_parallel(case.body, case.expect, chunk_bytes)
        assert (r.status, r.produced, r.consumed, r.data) == serial, chunk_bytes
        assert r.info[1] == case.reason[chunk_bytes], (chunk_bytes, r.info)
        assert (r.info[0] > 0) == (r.info[1] == 0) and r.info[2] == len(r.candidates) and r.info[3] == 0
        if chunk_bytes in case.candidates:
            assert r.candidates == case.candidates[chunk_bytes], chunk_bytes
    at64 = pm.inflate_parallel(case.body, case.expect, 64)
    if name == "block_longer_than_three_chunks":
        assert at64.info[0] == 2 and len(case.body) > 20 * 64
    if name == "shorter_than_one_chunk":
        assert len(case.body) < 64
    if name == "bytes_behind_the_final_block":
        assert at64.consumed == len(case.body) - 100
    if name == "distance_32768_from_a_segments_ends":
        seg = pm.decode_segment(case.body, at64.candidates[0], None)
        assert seg.elements[0] == pm.MARK and seg.elements[257] == pm.MARK | 257 and seg.far == 32768 and seg.far_matches == 2
    if name == "overlapping_match_across_markers":
        seg = pm.decode_segment(case.body, 2048, None)
        assert seg.elements[:50] == [pm.MARK | (32761 + i % 7) for i in range(50)]
    if name == "stored_fixed_and_dynamic_in_one_segment":
        assert at64.info[0] == 2 and at64.far == 1
    if name.startswith("planted"):
        assert at64.info == (0, 1, 2, 0)


# ---- seeded defects
def defect_seen(defect):
    """True where some case tells the model with the defect from the model without it."""
    for body, data in (pc.family_a(), pc.family_b()):
        r = pm.inflate_parallel(body, len(data), 256, defect)
        if r.info[1] != 0 or r.info[0] < 8 or r.data != data or r.adler != im.adler_halves(data):
            return True
    for name, case in pc.corners().items():
        for chunk_bytes in CHUNKS:
            r = pm.inflate_parallel(case.body, case.expect, chunk_bytes, defect)
            if (r.status, r.produced, r.consumed, r.data) != im.inflate(case.body, case.expect) or r.info[1] != case.reason[chunk_bytes]:
                return True
            if chunk_bytes in case.candidates and r.candidates != case.candidates[chunk_bytes]:
                return True
    # a segment that ends three bits behind the next one's start, in the same byte: the chain is checked on bits
    segs = [pm.Segment(0, 0, 803, False, [0] * 10, 0, 0), pm.Segment(800, 0, 1600, True, [0] * 6, 0, 0)]
    if pm.validate(segs, 16, defect) != 1:
        return True
    return False


@pytest.mark.parametrize("defect", pm.DEFECTS)
def test_seeded_defects_are_seen(defect):
    assert defect_seen(defect), defect
    assert not defect_seen(None)


# ---- the host routine of csrc/png_inflate_par.hpp under sanitizers
def par_records():
    records = [(body, expect) for body, expect in probe_records() if expect > 0]
    records += [(case.body, case.expect) for case in pc.corners().values()]
    records += [(body, len(data)) for body, data in (pc.family_a(), pc.family_b())]
    return [(body, expect, chunk_bytes) for body, expect in records for chunk_bytes in CHUNKS]


def test_parallel_routine_under_sanitizers(tmp_path):
    """csrc/png_inflate_par.hpp's vf_inf_stream_parallel as a stand-alone program with -fsanitize=address,undefined, every stream,
    plane, segment table and output in a heap block of exactly its size: status, produced, consumed, bytes, checksum, candidate list
    and reason are the model's on every stream above and the 20 000 mutations, at the three chunk sizes."""
    exe = str(tmp_path / "png_inflate_par_probe")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "png_inflate_par_probe.cpp"), "-o", exe], check=True)
    records = par_records()
    src, dst = str(tmp_path / "streams.bin"), str(tmp_path / "results.bin")
    with open(src, "wb") as f:
        for body, expect, chunk_bytes in records:
            f.write(struct.pack("<iii", len(body), expect, chunk_bytes) + body)
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert done.stdout.splitlines()[-1] == f"records {len(records)}"
    got, at = open(dst, "rb").read(), 0
    for k, (body, expect, chunk_bytes) in enumerate(records):
        head = struct.unpack_from("<10i", got, at)
        at += 40
        candidates = struct.unpack_from(f"<{head[9]}q", got, at)
        at += 8 * head[9]
        data = got[at:at + head[1]]
        at += head[1]
        want = pm.inflate_parallel(body, expect, chunk_bytes)
        assert (head[0], head[1], head[2], data) == (want.status, want.produced, want.consumed, want.data), (k, chunk_bytes, head)
        assert (head[3], head[4]) == want.adler and head[5:9] == want.info and candidates == want.candidates, (k, chunk_bytes, head)
    assert at == len(got)


# ---- the binding, the flag, the rule
def test_binding_and_refusals_without_a_gpu():
    import torch
    from vface_amd import hip
    from vface_amd.scripts import png_in
    lib = hip.load()
    assert lib.vface_png_inflate_parallel and lib.vface_png_inflate_parallel_workspace_bytes
    ws = hip.png_inflate_parallel_workspace_bytes
    assert ws(1, 1000, 500, 256) % 16 == 0 and ws(1, 1000, 500, 256) >= 2 * 500
    assert ws(2, 1000, 500, 256) > ws(1, 1000, 500, 256) and ws(1, 1000, 500, 64) > ws(1, 1000, 500, 256)
    for bad in ((0, 1000, 500, 256), (1, 0, 500, 256), (1, 1000, 0, 256), (1, 1000, 500, 60), (1, 1000, 500, 66), (1, 1000, 500, (1 << 20) + 4),
                (1, 1 << 31, 500, 256), (1, 1000, 1 << 31, 256)):
        assert lib.vface_png_inflate_parallel_workspace_bytes(*bad) == 0, bad
    host = (torch.zeros(8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(hip.VFaceHipError):
        hip.png_inflate_parallel(*host, 8)
    with pytest.raises(hip.VFaceHipError, match="chunk_bytes"):
        hip.png_inflate_parallel(*host, 8, chunk_bytes=102)
    frames = png_in.PNGFrames(2, 2, [png_in.parse_png(cases.png_bytes(2, 2, 2, bytes(14)))])
    with pytest.raises(hip.VFaceHipError):
        png_in.decode(frames, "cpu", inflate="parallel")
    with pytest.raises(hip.VFaceHipError, match="inflate"):
        png_in.decode(frames, "cuda", inflate="speculative")


def test_flag_and_its_refusals():
    from vface_amd.scripts import VFace_inference_batch as cli
    parser = cli.build_parser()
    assert parser.parse_args([]).png_in_inflate == "serial"
    for mode in ("auto", "serial", "parallel"):
        assert parser.parse_args(["--png_in_inflate", mode]).png_in_inflate == mode
    with pytest.raises(SystemExit):
        parser.parse_args(["--png_in_inflate", "speculative"])
    clip = ["--src_image", "s.png", "--landmarks", "l.npz", "--synthetic_weights", "--target_frames", "clip/"]
    for mode in ("auto", "parallel"):
        opt = cli.normalise_options(parser.parse_args(clip + ["--png_in_inflate", mode]))
        opt.synthetic = False
        with pytest.raises(SystemExit, match="--png_in_inflate.*--png_decoder gpu"):
            cli.check_options(opt)
        opt = cli.normalise_options(parser.parse_args(clip + ["--png_in_inflate", mode, "--png_decoder", "gpu"]))
        opt.synthetic = False
        cli.check_options(opt)
    opt = cli.normalise_options(parser.parse_args(clip))
    opt.synthetic = False
    cli.check_options(opt)                                   # the default is nobody's business


def test_inflate_path_rule():
    from vface_amd.scripts import png_in
    t = png_in.PARALLEL_MIN_BODY_BYTES
    assert t >= 2 * png_in.PARALLEL_CHUNK_BYTES
    for files in (1, 6, 32):
        assert png_in.inflate_path("serial", 100 * t * files, files) == "serial"
        assert png_in.inflate_path("parallel", 10, files) == "parallel"
        assert png_in.inflate_path("auto", t * files, files) == "serial"             # the mean body must EXCEED the threshold
        assert png_in.inflate_path("auto", (t + 1) * files, files) == "parallel"
    with pytest.raises(ValueError):
        png_in.inflate_path("speculative", 1, 1)
