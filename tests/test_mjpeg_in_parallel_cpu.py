"""The parallel entropy decoder of the Motion-JPEG way in, without a GPU: the per-subsequence routine of csrc/jpeg_subseq.hpp as a
host program under sanitizers (tests/jpeg_subseq_probe.cpp runs the kernel's algorithm with the lanes of a chunk as a loop) against
the serial routine and the integer model; the streams built to put a subsequence boundary where it hurts; the choice between the two
decoders, the command-line flag and the binding."""
import ctypes as C
import functools
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import jpeg_decode_model as jdm
import jpeg_model as jm
import mjpeg_in_cases as cases
from conftest import ROOT
from test_mjpeg_in_cpu import interval_records
from vface_amd.scripts import VFace_inference_batch as cli
from vface_amd.scripts import mjpeg_in

CSRC = os.path.join(ROOT, "vface_amd", "csrc")
SUBSEQ_BYTES = (4, 8, 32, 128)
LANES = (4, 64)                 # lanes per chunk: 4 makes chunk carries occur on small pictures
MUTATIONS = 20000               # in all, spread over the SUBSEQ_BYTES x LANES runs


def table_block(huffman):
    return np.concatenate([mjpeg_in.huffman_table(*t) for t in huffman[0]] + [mjpeg_in.huffman_table(*t) for t in huffman[1]])


def one_interval(scan, mcus, huffman):
    """The record of a scan without restart markers, expected status and coefficients by the model."""
    books = ([jdm.code_book(t) for t in huffman[0]], [jdm.code_book(t) for t in huffman[1]])
    coef, code = jdm.decode_interval(scan, 0, len(scan), books, 6 * mcus)
    return (scan, 0, len(scan), table_block(huffman), 6 * mcus, code, coef)


def pillow_scan(jpeg, W, H):
    frame = mjpeg_in.parse_jpeg(jpeg)
    return jpeg[frame.scan[0]:frame.scan[1]], mjpeg_in.mcu_count(W, H), frame.restart, jdm.frame_tables(frame)[0]


# ---- streams built around a boundary
def constructed_streams():
    """name -> (bit pieces [(what, bits)], mcus): Annex-K streams whose 4-byte subsequence boundary (bit 32 of the unstuffed bits;
    the pieces in front of it hold no FF byte unless the case is about one) falls where the name says."""
    code = cases._code
    dc0, eob = code(jm.DC_LUMA, 0), code(jm.AC_LUMA, 0x00)
    one = ("ac 0/1", code(jm.AC_LUMA, 0x01) + "0")                      # 3 bits: the value -1
    big = [("code 0/A", code(jm.AC_LUMA, 0x0A)), ("extra 0/A", "1000000001")]   # 16 + 10 bits: the value 513
    empty_y, empty_c = [("dc", dc0), ("eob", eob)], [("dc", code(jm.DC_CHROMA, 0)), ("eob", code(jm.AC_CHROMA, 0x00))]
    rest = empty_y * 3 + empty_c * 2 + (empty_y * 4 + empty_c * 2) * 2  # the other five blocks of MCU 0, then two empty MCUs
    out = {
        "boundary_in_code": ([("dc", dc0)] + [one] * 8 + big + [("eob", eob)] + rest, 3),
        "boundary_in_extra_bits": ([("dc", dc0)] + [one] * 4 + big + [("eob", eob)] + rest, 3),
        "boundary_between_ff_and_00": ([("dc", dc0)] + [one] * 7 + big + [("eob", eob)] + rest, 3),
        "boundary_at_block_end": ([("dc", code(jm.DC_LUMA, 1) + "1")] + [one] * 8 + [("eob", eob)] + rest, 3),
    }
    # a block far longer than a subsequence: AC size 10 in every position of every block of one MCU
    long_blocks = []
    for comp in (0, 0, 0, 0, 1, 1):
        dc, ac = (jm.DC_LUMA, jm.AC_LUMA) if comp == 0 else (jm.DC_CHROMA, jm.AC_CHROMA)
        long_blocks += [("dc", code(dc, 0))] + [("code 0/A", code(ac, 0x0A)), ("extra 0/A", "0110100101")] * 63
    out["size_10_throughout"] = (long_blocks, 1)
    # 29 empty MCUs = 174 blocks in 116 bytes: one 128-byte subsequence begins more than 170 blocks
    out["empty_blocks"] = ((empty_y * 4 + empty_c * 2) * 29, 29)
    return out


def piece_at(pieces, bit):
    at = 0
    for what, bits in pieces:
        if at <= bit < at + len(bits):
            return what, bit - at
        at += len(bits)
    return None, 0


def test_constructed_streams_put_the_boundary_where_they_say():
    built = constructed_streams()
    where = {name: piece_at(built[name][0], 32) for name in built}
    assert where["boundary_in_code"] == ("code 0/A", 6) and where["boundary_in_extra_bits"] == ("extra 0/A", 2)
    assert where["boundary_at_block_end"] == ("dc", 0) and piece_at(built["boundary_at_block_end"][0], 31) == ("eob", 3)
    for name in ("boundary_in_code", "boundary_in_extra_bits", "boundary_at_block_end"):
        assert b"\xFF" not in cases._bits("".join(b for _, b in built[name][0]))[:8], name
    scan = cases._bits("".join(b for _, b in built["boundary_between_ff_and_00"][0]))
    assert scan[3:5] == b"\xFF\x00" and b"\xFF" not in scan[:3]          # raw byte 4, where subsequence 1 begins, is the stuffed 00
    pieces = built["size_10_throughout"][0]
    assert len(pieces) == 6 * (1 + 2 * 63) and sum(len(b) for _, b in pieces) > 6 * 8 * 190
    scan = cases._bits("".join(b for _, b in built["empty_blocks"][0]))
    assert len(scan) <= 128 and built["empty_blocks"][1] * 6 >= 170 and b"\xFF" not in scan


# ---- the records the probe reads
@functools.lru_cache(maxsize=None)
def records():
    """[(name, record)]: every interval of test_mjpeg_in_cpu.interval_records() (the round-trip streams, the Pillow frames with
    tables of their own, the corruption cases, the category-12 tables), every Pillow frame without restart markers as one
    interval, the constructed streams, a flat picture and the smooth 512 x 384 one."""
    out = [(f"interval_{i}", r) for i, r in enumerate(interval_records())]
    decoded = cases.decoded_pillow_frames()
    for name, W, H, jpeg in cases.pillow_frames():
        scan, mcus, restart, huffman = pillow_scan(jpeg, W, H)
        if restart == 0:
            coef, status = decoded[name][0], decoded[name][1]
            out.append((name, (scan, 0, len(scan), table_block(huffman), 6 * mcus, status, coef)))
    for name, (pieces, mcus) in constructed_streams().items():
        record = one_interval(cases._bits("".join(b for _, b in pieces)), mcus, cases.ANNEX_K)
        assert record[5] == jdm.OK, name
        out.append((name, record))
    flat = cases.pillow_jpeg(np.full((136, 250, 3), FLAT_GREY, np.uint8), quality=90, optimize=True)
    scan, mcus, restart, huffman = pillow_scan(flat, 250, 136)
    assert restart == 0
    out.append(("flat_250x136", one_interval(scan, mcus, huffman)))
    smooth = cases.pillow_jpeg(jm.patterns(1, 512, 384, seed=33)["smooth"][0], quality=90)
    scan, mcus, restart, huffman = pillow_scan(smooth, 512, 384)
    assert restart == 0
    out.append(("smooth_q90_512x384", one_interval(scan, mcus, huffman)))
    return out


def host_compiler():
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    return cxx


def write_records(path, recs):
    with open(path, "wb") as f:
        for scan, begin, end, block, blocks, code, coef in recs:
            f.write(struct.pack("<I", len(scan)) + scan + struct.pack("<II", begin, end) + block.tobytes() + struct.pack("<II", blocks, code))
            f.write(np.ascontiguousarray(coef, np.int16).tobytes())


def parse_counts(stdout):
    """probe output -> {record index: (subsequences, chunks, rounds)}, {status: mutations}"""
    counts, histogram = {}, {}
    for line in stdout.splitlines():
        w = line.split()
        if w[0] == "record":
            counts[int(w[1])] = (int(w[3]), int(w[5]), int(w[7]))
        elif w[0] == "status":
            histogram[int(w[1][:-1])] = int(w[2])
    return counts, histogram


@pytest.fixture(scope="module")
def probe_runs(tmp_path_factory):
    """The probe under sanitizers, run once per (subseq_bytes, lanes) on every record: {(S, L): (counts, histogram)}."""
    tmp = tmp_path_factory.mktemp("subseq")
    exe = str(tmp / "jpeg_subseq_probe")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "jpeg_subseq_probe.cpp"), "-o", exe], check=True)
    recs = [r for _, r in records()]
    path = str(tmp / "cases.bin")
    write_records(path, recs)
    runs, per_run = {}, MUTATIONS // (len(SUBSEQ_BYTES) * len(LANES))
    for S in SUBSEQ_BYTES:
        for L in LANES:
            done = subprocess.run([exe, path, str(per_run), str(7 + S + L), str(S), str(L)], capture_output=True, text=True)
            assert done.returncode == 0, (S, L, done.stdout[-2000:] + done.stderr[-4000:])
            assert done.stdout.splitlines()[0] == f"cases {len(recs)} mutations {per_run}"
            runs[(S, L)] = parse_counts(done.stdout)
    return runs


def test_subsequence_decoder_under_sanitizers(probe_runs):
    """Coefficients and status equal vf_jpeg_decode_interval's and the model's on every record (the probe compares and exits 1
    otherwise), at every subsequence size and with chunk carries; 20 000 seeded mutations in all give the serial routine's result
    and no sanitizer report."""
    names = [n for n, _ in records()]
    statuses = {r[5] for _, r in records()}
    assert {jdm.OK, jdm.SHORT, jdm.BAD_CODE, jdm.RUN, jdm.DC_CATEGORY} <= statuses, statuses
    assert sum(n.split("_")[0] in ("q30", "q90", "q100", "optimize", "qtables", "no", "merged", "com") for n in names) == 8 * len(cases.PILLOW_SIZES)
    total = {}
    for (S, L), (counts, histogram) in probe_runs.items():
        assert sorted(counts) == list(range(len(names)))
        for i, (scan, begin, end, *_) in enumerate(r for _, r in records()):
            nsub = (end - begin) // S + 1
            assert counts[i][0] == nsub and counts[i][1] == -(-nsub // L) and 0 <= counts[i][2] <= nsub - counts[i][1], (names[i], S, L, counts[i])
        for code, n in histogram.items():
            total[code] = total.get(code, 0) + n
    assert sum(total.values()) == MUTATIONS and total[jdm.OK] > 0 and total[jdm.SHORT] > 0 and total[jdm.BAD_CODE] > 0
    # chunk carries did occur on small pictures
    assert max(c[1] for c in probe_runs[(4, 4)][0].values()) > 100 and max(c[1] for c in probe_runs[(128, 64)][0].values()) >= 2


FLAT_GREY = 140


def test_a_flat_picture_never_synchronises(probe_runs):
    """Every block of a flat picture is "DC 0, EOB"; where the luma and the chroma tables give those two symbols the same codes, a
    guess that is off by some slots runs parallel to the truth for ever, and the rounds advance one lane each: subsequences - 1
    per chunk, exactly.  The picture is in that regime by conditions on the INPUT, asserted here.  Pillow's ``optimize`` gives
    every table of this picture a 1-bit code "0" for DC 0 and for EOB, so every block but the first is the two bits "00", on
    either table and from either of the states k = 0 and k = 1: two lanes at the same bit in different (slot, k) consume the same
    bits and keep their distance.  An MCU is 12 bits and the first block's DC difference adds an odd number of bits, so every
    subsequence boundary -- a multiple of 32 bits -- falls behind a DC code, in state k = 1, which no guess (slot 0, k 0) is.  The
    scan's length is no multiple of 4, so the last subsequence does not begin at the end of the data, where the truth is (0, 0)."""
    i = [n for n, _ in records()].index("flat_250x136")
    scan, _, _, block, blocks, status, coef = records()[i][1]
    coef = coef.reshape(-1, 6, 64)
    assert not coef[:, :, 1:].any() and not np.diff(coef[:, :4, 0].reshape(-1)).any() and not coef[:, 4:, 0].any() and coef[0, 0, 0] != 0
    flat = cases.pillow_jpeg(np.full((136, 250, 3), FLAT_GREY, np.uint8), quality=90, optimize=True)
    dc, ac = pillow_scan(flat, 250, 136)[3]
    for comp in range(3):
        assert jm.huffman_codes(dc[comp])[0] == (0, 1) and jm.huffman_codes(ac[comp])[0x00] == (0, 1), comp
    category = abs(int(coef[0, 0, 0])).bit_length()
    surplus = jm.huffman_codes(dc[0])[category][1] - 1 + category
    assert surplus % 2 == 1 and b"\xFF" not in scan and len(scan) % 4 != 0 and len(scan) == -(-(12 * blocks // 6 + surplus) // 8), surplus
    for (S, L), (counts, _) in probe_runs.items():
        nsub, chunks, rounds = counts[i]
        print(f"flat 250x136, {S} bytes, {L} lanes: {nsub} subsequences, {chunks} chunks, {rounds} rounds")
        assert rounds == nsub - chunks, (S, L, counts[i])


def test_an_ordinary_picture_synchronises_early(probe_runs):
    """The smooth quality-90 512 x 384 picture at 128 bytes and the kernel's 64 lanes per chunk: rounds under a tenth of its
    subsequences (a throw-away model measured a mean synchronisation distance of 1.38 subsequences, 99th percentile 4).  A chunk
    whose guesses are not all right needs a round, so with 4 lanes per chunk a quarter of the subsequence count is the floor: that
    run is printed, and bounded by the worst case only."""
    i = [n for n, _ in records()].index("smooth_q90_512x384")
    for L in LANES:
        nsub, chunks, rounds = probe_runs[(128, L)][0][i]
        print(f"smooth q90 512x384, 128 bytes, {L} lanes: {nsub} subsequences, {chunks} chunks, {rounds} rounds")
    nsub, chunks, rounds = probe_runs[(128, 64)][0][i]
    assert nsub > 200 and rounds < nsub / 10, (nsub, rounds)


# ---- the choice, the flag, the binding
def frames_of(scans_and_restarts, W=64, H=48):
    recs = [mjpeg_in.FrameRecord(i, bytes(n), r, np.ones((3, 64), np.uint8), np.zeros(mjpeg_in.TABLE_BYTES, np.uint8))
            for i, (n, r) in enumerate(scans_and_restarts)]
    return mjpeg_in.MJPEGFrames("x.avi", W, H, recs), mjpeg_in.mcu_count(W, H)


def test_entropy_path_follows_the_interval_length(monkeypatch):
    frames, mcus = frames_of([(3000, 0), (3000, 0)])
    assert mcus == 12
    rows, mcus = frames_of([(3000, 4), (2000, 4)])
    mixed, _ = frames_of([(3000, 4), (3000, 0)])
    blocks, _ = frames_of([(3000, 1)])
    # as shipped: a frame without restart markers takes the parallel decoder (3000 bytes in one interval), short intervals do not
    assert mjpeg_in.entropy_path(frames, mcus) == "parallel" and mjpeg_in.entropy_path(mixed, mcus) == "parallel"
    assert mjpeg_in.entropy_path(rows, mcus) == "serial" and mjpeg_in.entropy_path(blocks, mcus) == "serial"
    one_mcu, one = frames_of([(40, 0)], 16, 16)
    assert one == 1 and mjpeg_in.entropy_path(one_mcu, one) == "serial"
    # the rule: the largest len(scan) / interval count of the call against the constant
    monkeypatch.setattr(mjpeg_in, "PARALLEL_MIN_INTERVAL_BYTES", 1000)
    assert mjpeg_in.entropy_path(frames, mcus) == "parallel" and mjpeg_in.entropy_path(rows, mcus) == "parallel"     # 3000 / 3
    assert mjpeg_in.entropy_path(blocks, mcus) == "serial"                                                          # 3000 / 12
    monkeypatch.setattr(mjpeg_in, "PARALLEL_MIN_INTERVAL_BYTES", 1001)
    assert mjpeg_in.entropy_path(rows, mcus) == "serial" and mjpeg_in.entropy_path(mixed, mcus) == "parallel"
    assert isinstance(mjpeg_in.PARALLEL_MIN_INTERVAL_BYTES, int) and mjpeg_in.SUBSEQ_BYTES % 4 == 0 and 4 <= mjpeg_in.SUBSEQ_BYTES <= 1024


BASE = ["--src_image", "s.png", "--landmarks", "l.npz", "--synthetic_weights"]


def test_the_flag_parses_and_is_refused_where_it_says_nothing(tmp_path):
    p = cli.build_parser()
    assert p.parse_args([]).video_in_entropy is None
    for value in ("auto", "serial", "parallel"):
        opt = p.parse_args(["--target_video", "c.avi", "--video_in_entropy", value] + BASE)
        assert opt.video_in_entropy == value
        cli.check_options(cli.normalise_options(opt))
    with pytest.raises(SystemExit):
        p.parse_args(["--video_in_entropy", "wavefront"])
    for more in (["--target_frames", "d"] + BASE, ["--synthetic"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["--video_in_entropy", "parallel"] + more)
        assert str(e.value) == "--video_in_entropy says how --target_video is decoded: it needs --target_video FILE.avi"
    # a YUV4MPEG2 file has no entropy coding: refused once the file's first bytes have said what it is
    y4m = tmp_path / "clip.y4m"
    y4m.write_bytes(b"YUV4MPEG2 W4 H2 F25:1 Ip C420jpeg\n" + b"FRAME\n" + bytes(12))
    avi = tmp_path / "clip.avi"
    avi.write_bytes(jm.avi_file(jm.encode_frames(jm.patterns(1, 32, 16, seed=4)["smooth"], 90, 2), 32, 16))
    for path, flag, words in ((y4m, "--video_in_entropy", "--video_in_entropy chooses the Huffman decoder of Motion-JPEG; .*clip.y4m is YUV4MPEG2"),
                              (avi, "--video_in_matrix", "--video_in_matrix names the matrix of a file that cannot tag it; .*clip.avi is Motion-JPEG")):
        opt = cli.normalise_options(p.parse_args(["--target_video", str(path), flag, "serial" if "entropy" in flag else "bt601"] + BASE))
        video = mjpeg_in.open_video(str(path))
        with pytest.raises(SystemExit, match=words):
            cli.check_video_in_reader(opt, video)
        video.close()
    for path, flag, value in ((avi, "--video_in_entropy", "parallel"), (y4m, "--video_in_matrix", "bt601")):
        video = mjpeg_in.open_video(str(path))
        cli.check_video_in_reader(cli.normalise_options(p.parse_args(["--target_video", str(path), flag, value] + BASE)), video)
        video.close()
    # the provider hands the choice to the AVI reader alone, "auto" without the flag
    from vface_amd.scripts import inputs
    src = open(inputs.__file__).read()
    assert 'getattr(opt, "video_in_entropy", None) or "auto"' in src and "entropy=self.entropy" in src


def test_binding_refuses_without_a_gpu():
    from vface_amd import hip
    scans = torch.zeros(16, dtype=torch.uint8)
    args = (scans, torch.zeros(1, 1, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
            torch.zeros(1, hip.JPEG_TABLE_BYTES, dtype=torch.uint8), 1)
    with pytest.raises(hip.VFaceHipError):
        hip.jpeg_decode_entropy_parallel(*args)
    with pytest.raises(hip.VFaceHipError, match="subseq_bytes must be a multiple of 4 in 4..1024"):
        hip.jpeg_decode_entropy_parallel(*args, subseq_bytes=6)
    with pytest.raises(hip.VFaceHipError, match="jpeg_decode_entropy_parallel: ranges must be int32"):
        hip.jpeg_decode_entropy_parallel(scans, torch.zeros(2, dtype=torch.int32), *args[2:])
    with pytest.raises(hip.VFaceHipError, match="entropy is auto, serial or parallel"):
        mjpeg_in.decode(mjpeg_in.MJPEGFrames("x.avi", 16, 16, []), "cuda", entropy="wavefront")
    with pytest.raises(hip.VFaceHipError):
        mjpeg_in.decode(frames_of([(40, 0)], 16, 16)[0], "cpu", entropy="parallel")
    lib = hip.load()
    for name in ("vface_jpeg_decode_entropy_parallel", "vface_jpeg_decode_entropy_parallel_workspace_bytes"):
        assert name in hip.SIGNATURES and hasattr(lib, name)
    assert lib.vface_jpeg_decode_entropy_parallel_workspace_bytes(5) >= 20
    # the lanes rule of csrc/jpeg_subseq.hpp, mirrored for the tests that compare `rounds`
    assert hip.jpeg_parallel_lanes(64 * 128 * 3, 3, 1, 128) == 256 and hip.jpeg_parallel_lanes(64 * 128 * 3 - 1, 3, 1, 128) == 64
    assert hip.jpeg_parallel_lanes(10 ** 6, 2, 68, 128) == 64 and hip.jpeg_parallel_lanes(40, 1, 1, 4) == 64
    header = open(os.path.join(CSRC, "jpeg_subseq.hpp")).read()
    assert "kVfJpegLanesShort = 64, kVfJpegLanesLong = 256;" in header and "kVfJpegSubseqMin = 4, kVfJpegSubseqMax = 1024;" in header
    assert "scan_bytes / intervals / subseq_bytes >= kVfJpegLanesShort ? kVfJpegLanesLong : kVfJpegLanesShort" in header
    assert "#include <hip" not in header and "hip_runtime" not in header


def test_new_entry_points_match_the_header_argument_for_argument():
    from vface_amd import hip
    text = open(os.path.join(ROOT, "include", "vface_hip.h")).read()
    kind = {C.c_void_p: "p", C.c_int64: "l", C.c_int: "i", C.c_size_t: "z"}
    for name, res in (("vface_jpeg_decode_entropy_parallel", "int"), ("vface_jpeg_decode_entropy_parallel_workspace_bytes", "size_t")):
        m = re.search(r"\b" + res + " " + name + r"\(([^;]*)\);", text)
        assert m, name
        want = ""
        for arg in (a.strip() for a in m.group(1).replace("\n", " ").split(",")):
            want += "p" if "*" in arg else "l" if arg.startswith("int64_t") else "z" if arg.startswith("size_t") else "i"
        assert "".join(kind[a] for a in hip.SIGNATURES[name][1]) == want, name
        assert hip.SIGNATURES[name][0] is (C.c_int if res == "int" else C.c_size_t)
    serial = re.search(r"\bint vface_jpeg_decode_entropy\(([^;]*)\);", text).group(1)
    parallel = re.search(r"\bint vface_jpeg_decode_entropy_parallel\(([^;]*)\);", text).group(1)
    norm = lambda s: [a.strip() for a in s.replace("\n", " ").split(",")]
    assert norm(parallel)[:11] == norm(serial)[:11] and norm(parallel)[-1] == norm(serial)[-1] == "void* stream"
