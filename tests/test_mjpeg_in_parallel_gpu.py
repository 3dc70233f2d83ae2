"""vface_jpeg_decode_entropy_parallel (csrc/mjpeg_in.hip, csrc/jpeg_subseq.hpp) against the decoder model
(tests/jpeg_decode_model.py) AND against vface_jpeg_decode_entropy in the same call sequence, bit for bit: coefficients, statuses,
and the round counter against the host program that runs the same routine (tests/jpeg_subseq_probe.cpp).

Every stream here, the corrupt ones included, and 20 000 mutations besides, has passed that host program under sanitizers first
(tests/test_mjpeg_in_parallel_cpu.py): nothing here is meant to provoke anything."""
import os
import subprocess

import numpy as np
import pytest
import torch

import jpeg_decode_model as jdm
import jpeg_model as jm
import mjpeg_in_cases as cases
from conftest import ROOT
from test_mjpeg_in_gpu import SENTINEL8, SENTINEL16, SENTINEL32, annex_k_block, model_rgb, stream_frames, table_block
from test_mjpeg_in_parallel_cpu import CSRC, constructed_streams, host_compiler, parse_counts, write_records

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PARALLEL_GRID_CAP = 4096        # kParallelGridCap of csrc/mjpeg_in.hip: workgroups of one (frame, interval) before the grid loops
ERR_ARG, ERR_ALIGN, ERR_SHAPE = -1, -2, -3


def run_both(frames, mcus, subseq_bytes, gap=5, lead=3):
    """``frames``: [(scan bytes, restart, table block)] of ``mcus`` MCUs each, through vface_jpeg_scan_index and then BOTH entropy
    decoders at the C ABI, every buffer inside sentinels: the coefficients of each a strided view at element ``lead`` of an int16
    sentinel buffer, frames ``mcus * 384 + gap`` apart; the workspace and the rounds with int32 sentinels behind them.
    -> dict(serial=(coef, status), parallel=(coef, status), rounds [F, most], clean, lanes, ranges, nbytes)."""
    from vface_amd import hip
    lib = hip.load()
    F = len(frames)
    lengths = [len(f[0]) for f in frames]
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    total = int(sum(lengths))
    most = max(jdm.interval_count(mcus, f[1]) for f in frames)
    scans = torch.full((64 + total + 64,), SENTINEL8, dtype=torch.uint8)
    scans[64:64 + total] = torch.from_numpy(np.frombuffer(b"".join(f[0] for f in frames) + b"\0", np.uint8)[:total].copy())
    before = scans.clone()
    scans = scans.to(DEV)
    ranges = torch.full((F * most * 2 + 8,), SENTINEL32, dtype=torch.int32, device=DEV)
    index_status = torch.full((F + 4,), SENTINEL32, dtype=torch.int32, device=DEV)
    d_off, d_len = torch.from_numpy(offsets).to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV)
    d_restart = torch.tensor([f[1] for f in frames], dtype=torch.int32, device=DEV)
    tables = torch.from_numpy(np.stack([f[2] for f in frames])).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    scan_ptr, nbytes = scans.data_ptr() + 64, max(total, 1)
    assert lib.vface_jpeg_scan_index(scan_ptr, nbytes, d_off.data_ptr(), d_len.data_ptr(), d_restart.data_ptr(), mcus, F, most,
                                     ranges.data_ptr(), index_status.data_ptr(), stream) == 0
    n, stride = mcus * 384, mcus * 384 + gap
    ws_bytes = int(lib.vface_jpeg_decode_entropy_parallel_workspace_bytes(F))
    assert ws_bytes % 4 == 0 and ws_bytes >= 4 * F
    ws = torch.full((ws_bytes // 4 + 4,), SENTINEL32, dtype=torch.int32, device=DEV)
    rounds = torch.full((F * most + 4,), SENTINEL32, dtype=torch.int32, device=DEV)
    out, clean = {}, True
    for which in ("serial", "parallel"):
        buf = torch.full((lead + F * stride + 64,), SENTINEL16, dtype=torch.int16, device=DEV)
        status = index_status.clone()
        if which == "serial":
            rc = lib.vface_jpeg_decode_entropy(scan_ptr, nbytes, ranges.data_ptr(), d_restart.data_ptr(), tables.data_ptr(), mcus, F, most,
                                               buf.data_ptr() + 2 * lead, stride, status.data_ptr(), stream)
        else:
            rc = lib.vface_jpeg_decode_entropy_parallel(scan_ptr, nbytes, ranges.data_ptr(), d_restart.data_ptr(), tables.data_ptr(), mcus, F,
                                                        most, buf.data_ptr() + 2 * lead, stride, status.data_ptr(), subseq_bytes,
                                                        ws.data_ptr(), ws_bytes, rounds.data_ptr(), stream)
        assert rc == 0, (which, rc)
        torch.cuda.synchronize()
        whole, st = buf.cpu().numpy(), status.cpu().numpy()
        outside = np.ones(whole.shape, bool)
        for f in range(F):
            outside[lead + f * stride:lead + f * stride + n] = False
        clean = clean and bool((whole[outside] == SENTINEL16).all()) and bool((st[F:] == SENTINEL32).all())
        out[which] = (np.stack([whole[lead + f * stride:lead + f * stride + n] for f in range(F)]).reshape(F, mcus, 6, 64), st[:F].copy())
    clean = clean and bool((ws[ws_bytes // 4:] == SENTINEL32).all()) and bool((rounds[F * most:] == SENTINEL32).all())
    clean = clean and bool((ranges[F * most * 2:] == SENTINEL32).all()) and torch.equal(scans.cpu(), before)
    out.update(clean=clean, rounds=rounds[:F * most].cpu().numpy().reshape(F, most), ranges=ranges[:F * most * 2].cpu().numpy().reshape(F, most, 2),
               lanes=hip.jpeg_parallel_lanes(nbytes, F, most, subseq_bytes), nbytes=nbytes)
    return out


def assert_same(got, want, what):
    """Both decoders against the model's (coefficients [F, mcus, 6, 64], statuses) and against each other."""
    for which in ("serial", "parallel"):
        coef, status = got[which]
        assert status.tolist() == list(want[1]), (what, which, status.tolist())
        bad = np.argwhere(coef != want[0])
        assert bad.size == 0, f"{what}, {which}: {len(bad)} coefficients differ from the model, first at (frame, mcu, block, k) {tuple(bad[0])}"
    assert np.array_equal(got["parallel"][0], got["serial"][0]) and np.array_equal(got["parallel"][1], got["serial"][1]), what
    assert got["clean"], f"{what}: something outside the buffers was written"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/jpeg_subseq_probe.cpp built without sanitizers -> rounds(frames, mcus, got, subseq_bytes): the host's round counts of
    every interval of a call, [F, most], at the lanes per chunk the entry point picked."""
    tmp = tmp_path_factory.mktemp("subseq_gpu")
    exe = str(tmp / "jpeg_subseq_probe")
    subprocess.run([host_compiler(), "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "jpeg_subseq_probe.cpp"), "-o", exe], check=True)

    def rounds(frames, mcus, got, subseq_bytes):
        recs, where, at = [], [], 0
        for f, (scan, restart, block) in enumerate(frames):
            count = jdm.interval_count(mcus, restart)
            step = mcus if restart <= 0 or restart >= mcus else restart
            for i in range(count):
                begin, end = (int(v) - at for v in got["ranges"][f, i])
                blocks = 6 * (min(i * step + step, mcus) - i * step)
                coef = got["serial"][0][f].reshape(-1, 64)[6 * i * step:6 * i * step + blocks]
                recs.append((scan, begin, end, block, blocks, 0, coef))
                where.append((f, i))
            at += len(scan)
        path = str(tmp / "cases.bin")
        write_records(path, recs)
        done = subprocess.run([exe, path, "0", "1", str(subseq_bytes), str(got["lanes"])], capture_output=True, text=True)
        assert done.returncode == 0, done.stdout[-1000:] + done.stderr[-2000:]
        counts, _ = parse_counts(done.stdout)
        out = np.zeros_like(got["rounds"])
        for k, (f, i) in enumerate(where):
            out[f, i] = counts[k][2]
        return out
    return rounds


# ---- against the model, the serial entry point and the host's round counts
@pytest.mark.parametrize("subseq_bytes", [4, 32, 128, 256])
def test_round_trip_streams_with_and_without_restart_markers(subseq_bytes, probe):
    """250 x 136 = 144 MCUs at restart 1, one MCU row and none, one call each and the three in one call; the noise picture at quality
    100 without markers, which at 4 bytes spans tens of chunks of 256 lanes."""
    by_restart = {f[1]: f for f in stream_frames("250x136_")}
    assert sorted(by_restart) == [1, 16, 147]
    coefs = {name.split("_r")[1]: coef for name, coef, restart, scan in cases.round_trip_streams() if name.startswith("250x136_")}
    for pick in ([1], [16], [147], [147, 1, 16]):
        frames = [by_restart[r] for r in pick]
        got = run_both(frames, 144, subseq_bytes, gap=3 + pick[0] % 5, lead=len(pick))
        assert_same(got, (np.stack([coefs[str(r)] for r in pick]), [0] * len(pick)), f"restart {pick}, {subseq_bytes} bytes")
        assert np.array_equal(got["rounds"], probe(frames, 144, got, subseq_bytes)), (pick, got["lanes"])
    noise = jm.coefficients(jm.patterns(1, 250, 136, seed=21)["noise"], *jm.quant_tables(100))[0].reshape(-1, 6, 64)
    frames = [(jm.scan_bytes(noise, 144), 0, annex_k_block())]
    got = run_both(frames, 144, subseq_bytes)
    assert_same(got, (noise[None], [0]), f"noise at quality 100, {subseq_bytes} bytes")
    want = probe(frames, 144, got, subseq_bytes)
    print(f"noise q100 250x136, {subseq_bytes} bytes, {got['lanes']} lanes: {len(frames[0][0]) // subseq_bytes + 1} subsequences, {int(want[0, 0])} rounds")
    assert np.array_equal(got["rounds"], want)
    if subseq_bytes == 4:
        assert got["lanes"] == 256 and len(frames[0][0]) // 4 + 1 >= 20 * 256


def test_pillow_frames_without_restart_markers(probe):
    """Frames libjpeg-turbo wrote as ONE interval: every variant without restart markers at every size -- optimised tables, own
    quantisation tables, no DHT, merged segments among them -- with the tables of the frame's own headers."""
    from vface_amd.scripts import mjpeg_in
    decoded = cases.decoded_pillow_frames()
    seen = set()
    for i, (name, W, H, jpeg) in enumerate(cases.pillow_frames()):
        frame = mjpeg_in.parse_jpeg(jpeg)
        if frame.restart:
            continue
        seen.add(name.split("_")[0])
        coef, status, _, _, _ = decoded[name]
        frames = [(jpeg[frame.scan[0]:frame.scan[1]], 0, mjpeg_in.huffman_block(frame))]
        for subseq_bytes in (4, 32, 128):
            got = run_both(frames, coef.shape[0], subseq_bytes, lead=i % 2)
            assert_same(got, (coef[None], [status]), f"{name}, {subseq_bytes} bytes")
            if (W, H) == (250, 136):
                assert np.array_equal(got["rounds"], probe(frames, coef.shape[0], got, subseq_bytes)), name
    assert {"optimize", "qtables", "no", "merged", "q100"} <= seen


def test_three_frames_with_three_table_sets_in_one_call(probe):
    from vface_amd.scripts import mjpeg_in
    by_name = {name: jpeg for name, W, H, jpeg in cases.pillow_frames()}
    names = ["optimize_130x50_edges", "merged_tables_130x50_smooth", "restart_rows_130x50_smooth"]
    parsed = [mjpeg_in.parse_jpeg(by_name[n]) for n in names]
    frames = [(by_name[n][p.scan[0]:p.scan[1]], p.restart, mjpeg_in.huffman_block(p)) for n, p in zip(names, parsed)]
    assert len({f[2].tobytes() for f in frames}) == 3 and [f[1] for f in frames] == [0, 0, 9] and len({len(f[0]) for f in frames}) == 3
    for subseq_bytes in (8, 128):
        got = run_both(frames, 36, subseq_bytes)
        assert_same(got, (np.stack([cases.decoded_pillow_frames()[n][0] for n in names]), [0, 0, 0]), names)
        assert np.array_equal(got["rounds"], probe(frames, 36, got, subseq_bytes)) and not got["rounds"][:2, 1:].any()


def test_constructed_boundaries(probe):
    """The streams of tests/test_mjpeg_in_parallel_cpu.py whose 4-byte boundary falls inside a code, inside extra bits, between FF
    and its 00 and at a block's end; blocks far longer than a subsequence; 174 empty blocks in one subsequence."""
    books = ([jdm.code_book(t) for t in cases.ANNEX_K[0]], [jdm.code_book(t) for t in cases.ANNEX_K[1]])
    for name, (pieces, mcus) in constructed_streams().items():
        scan = cases._bits("".join(b for _, b in pieces))
        coef, code = jdm.decode_interval(scan, 0, len(scan), books, 6 * mcus)
        frames = [(scan, 0, annex_k_block())]
        for subseq_bytes in (4, 128):
            got = run_both(frames, mcus, subseq_bytes)
            assert_same(got, (coef.reshape(1, mcus, 6, 64), [code]), name)
            assert code == 0 and np.array_equal(got["rounds"], probe(frames, mcus, got, subseq_bytes)), name


def test_more_one_mcu_frames_than_the_grid_cap():
    """More (frame, interval) items than workgroups, so the first workgroups stage a second frame's tables: one-MCU frames of six
    kinds, two table sets in turn; every frame against the model and the serial entry point."""
    coef = cases.entropy_cases()["partial_last_interval"][0][0]
    kinds = [(jm.scan_bytes(coef[i:i + 1], 1), 0, annex_k_block()) for i in range(4)]
    other = ([jm.DC_CHROMA, jm.DC_LUMA, jm.DC_LUMA], [jm.AC_CHROMA, jm.AC_LUMA, jm.AC_LUMA])
    kinds += [(scan, 0, table_block(other)) for scan, _, _ in kinds[:2]]
    want = [jdm.decode_scan(scan, 1, 0, cases.ANNEX_K if k < 4 else other) for k, (scan, _, _) in enumerate(kinds)]
    assert not any(status for _, status in want[:4]) and len({w[0].tobytes() for w in want}) >= 4
    pick = [(i * 5) % len(kinds) for i in range(PARALLEL_GRID_CAP + 37)]
    got = run_both([kinds[k] for k in pick], 1, 8, gap=1, lead=1)
    assert_same(got, (np.stack([want[k][0] for k in pick]), [want[k][1] for k in pick]), "past the grid cap")


def test_entropy_coder_then_parallel_decoder_is_the_identity():
    """hip.jpeg_entropy -> hip.jpeg_scan_index -> hip.jpeg_decode_entropy_parallel gives back random coefficients an encoder can
    produce (``jdm.legal_coefficients`` at qualities 30, 90 and 100), three frames of 144 MCUs, at restart intervals of a row, of 1
    and of the frame; through the wrappers, whose workspace is cached."""
    from vface_amd import hip
    rng = np.random.default_rng(14)
    host = np.concatenate([jdm.legal_coefficients(rng, quality, 6 * 144)[0] for quality in (30, 90, 100)])
    coef = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
    tables = torch.from_numpy(annex_k_block()).to(DEV).repeat(3, 1)
    for restart, subseq_bytes in ((16, 128), (1, 4), (144, 32), (144, 1024)):
        scans, lengths = hip.jpeg_entropy(coef, restart)
        offsets = torch.cumsum(lengths.to(torch.int64), 0) - lengths
        used = scans[:int(lengths.sum())]
        r = torch.full((3,), restart, dtype=torch.int32, device=DEV)
        ranges, status = hip.jpeg_scan_index(used, offsets, lengths, r, 144, hip.jpeg_interval_count(144, restart))
        back, status, rounds = hip.jpeg_decode_entropy_parallel(used, ranges, status, r, tables, 144, subseq_bytes, return_rounds=True)
        assert status.cpu().tolist() == [0, 0, 0] and tuple(back.shape) == (3, 144, 6, 64) and tuple(rounds.shape) == (3, ranges.shape[1])
        assert torch.equal(back, coef), (restart, subseq_bytes)
        again, _ = hip.jpeg_decode_entropy_parallel(used, ranges, status, r, tables, 144, subseq_bytes)
        assert torch.equal(again, coef)


CORRUPT = sorted(cases.corruption_cases()) + ["category_12"]


@pytest.mark.parametrize("name", CORRUPT)
def test_bad_bytes_give_the_serial_result_inside_the_buffers(name):
    """One corrupt frame between two good ones: the model's status and the model's coefficients (what the serial routine decoded
    before the fault, zeros behind it) from both entry points; the frames round it decode exactly; every sentinel is intact.
    (Each case has passed the host program under sanitizers, tests/test_mjpeg_in_parallel_cpu.py.)"""
    if name == "category_12":
        scan, huffman = cases.category12_tables()
        mcus, restart, want, block = 1, 0, jdm.DC_CATEGORY, table_block(huffman)
    else:
        (scan, mcus, restart, want), huffman, block = cases.corruption_cases()[name], cases.ANNEX_K, annex_k_block()
    good_coef = jm.coefficients(jm.patterns(2, 48 if mcus == 6 else 16, 32 if mcus == 6 else 16, seed=6)["noise"], *jm.quant_tables(90)).reshape(2, mcus, 6, 64)
    goods = [(jm.scan_bytes(good_coef[0], 2), 2, annex_k_block()), (jm.scan_bytes(good_coef[1], mcus), 0, annex_k_block())]
    frames = [goods[0], (scan, restart, block), goods[1]]
    model, status = jdm.decode_scan(scan, mcus, restart, huffman)
    assert status == want
    for subseq_bytes in (4, 128):
        got = run_both(frames, mcus, subseq_bytes)
        assert_same(got, (np.stack([good_coef[0], model, good_coef[1]]), [0, want, 0]), name)
        if want in (jdm.MARKER_COUNT, jdm.MARKER_ORDER):
            assert not got["rounds"][1].any()


def test_arguments_are_refused_by_code():
    from vface_amd import hip
    lib = hip.load()
    scans = torch.zeros(64, dtype=torch.uint8, device=DEV)
    r = torch.zeros(2, dtype=torch.int32, device=DEV)
    ranges = torch.zeros(2, 1, 2, dtype=torch.int32, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    tables = torch.from_numpy(annex_k_block()).to(DEV).repeat(2, 1)
    out = torch.zeros(2, 6, 6, 64, dtype=torch.int16, device=DEV)
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    rounds = torch.zeros(2, dtype=torch.int32, device=DEV)

    def call(scans_p=scans.data_ptr(), nbytes=64, tables_p=tables.data_ptr(), mcus=6, frames=2, most=1, stride=6 * 384, subseq=128,
             ws_p=ws.data_ptr(), ws_n=64, rounds_p=rounds.data_ptr()):
        return lib.vface_jpeg_decode_entropy_parallel(scans_p, nbytes, ranges.data_ptr(), r.data_ptr(), tables_p, mcus, frames, most,
                                                      out.data_ptr(), stride, status.data_ptr(), subseq, ws_p, ws_n, rounds_p, None)
    assert lib.vface_jpeg_decode_entropy_parallel_workspace_bytes(2) == 8 and lib.vface_jpeg_decode_entropy_parallel_workspace_bytes(0) == 0
    assert call() == 0 and call(rounds_p=None) == 0
    for bad in (dict(scans_p=None), dict(ws_p=None), dict(tables_p=None), dict(mcus=0), dict(frames=0), dict(most=0), dict(nbytes=0)):
        assert call(**bad) == ERR_ARG, bad
    for bad in (dict(subseq=0), dict(subseq=2), dict(subseq=6), dict(subseq=1028), dict(subseq=-4), dict(ws_n=7), dict(stride=6 * 384 - 1),
                dict(most=7), dict(nbytes=2 ** 31)):
        assert call(**bad) == ERR_SHAPE, bad
    for bad in (dict(tables_p=tables.data_ptr() + 2), dict(ws_p=ws.data_ptr() + 2)):
        assert call(**bad) == ERR_ALIGN, bad
    assert call(subseq=4) == 0 and call(subseq=1024) == 0
    torch.cuda.synchronize()
    for args in ((scans, ranges[:1], status, r, tables, 6), (scans, ranges, status[:1], r, tables, 6), (scans, ranges, status, r, tables[:, :100], 6),
                 (scans, ranges, status, r, tables.cpu(), 6), (scans, ranges.to(torch.int64), status, r, tables, 6)):
        with pytest.raises(hip.VFaceHipError, match="jpeg_decode_entropy_parallel: "):
            hip.jpeg_decode_entropy_parallel(*args)
    for subseq in (0, 6, 2048):
        with pytest.raises(hip.VFaceHipError, match="subseq_bytes must be a multiple of 4"):
            hip.jpeg_decode_entropy_parallel(scans, ranges, status, r, tables, 6, subseq)
    with pytest.raises(hip.VFaceHipError):
        hip.jpeg_decode_entropy_parallel(scans, ranges, status, r, tables, 6, out=torch.zeros(2, 6, 6, 64, dtype=torch.int32, device=DEV))


# ---- mjpeg_in.decode end to end
def test_decode_takes_the_parallel_path_for_files_without_restart_markers(tmp_path, monkeypatch):
    """An AVI of frames Pillow wrote without restart markers (what ffmpeg's encoder writes): ``entropy="parallel"`` equals
    ``entropy="serial"`` and the model's RGB, bit for bit; ``auto`` takes the parallel decoder for that file and the serial one for
    a file of this build's ``MJPEGWriter`` (one restart interval per MCU row)."""
    from vface_amd import hip
    from vface_amd.scripts import mjpeg, mjpeg_in
    W, H = 250, 136
    how = (dict(quality=90), dict(quality=60, optimize=True), dict(quality=100))
    jpegs = [cases.pillow_jpeg(jm.patterns(1, W, H, seed=50 + i)[p][0], **h) for i, (p, h) in enumerate(zip(("smooth", "edges", "noise"), how))]
    path = str(tmp_path / "pillow.avi")
    with open(path, "wb") as f:
        f.write(jm.avi_file(jpegs, W, H))
    calls = []
    serial, parallel = hip.jpeg_decode_entropy, hip.jpeg_decode_entropy_parallel
    monkeypatch.setattr(hip, "jpeg_decode_entropy", lambda *a, **k: calls.append("serial") or serial(*a, **k))
    monkeypatch.setattr(hip, "jpeg_decode_entropy_parallel", lambda *a, **k: calls.append("parallel") or parallel(*a, **k))
    want = model_rgb(jpegs)
    with mjpeg_in.MJPEGReader(path) as r:
        read = r.read([2, 0, 1, 0])
        assert mjpeg_in.entropy_path(read, mjpeg_in.mcu_count(W, H)) == "parallel"
        results = {e: mjpeg_in.decode(read, DEV, entropy=e) for e in ("serial", "parallel", "auto")}
        assert calls == ["serial", "parallel", "parallel"]
        for e, (rgb, status) in results.items():
            assert status == [0, 0, 0, 0] and np.array_equal(rgb.cpu().numpy(), want[[2, 0, 1, 0]]), e
        assert torch.equal(r.to_rgb(read, DEV, None, "sited", entropy="parallel"), results["serial"][0])
        assert torch.equal(r.to_rgb(read, DEV), results["serial"][0]) and calls[-2:] == ["parallel", "parallel"]
    own = str(tmp_path / "own.avi")
    with mjpeg.MJPEGWriter(own, W, H, quality=90) as w:
        w.write(torch.from_numpy(jm.patterns(2, W, H, seed=9)["smooth"]).to(DEV))
    del calls[:]
    with mjpeg_in.MJPEGReader(own) as r:
        read = r.read([0, 1])
        assert mjpeg_in.entropy_path(read, mjpeg_in.mcu_count(W, H)) == "serial"
        auto, status = mjpeg_in.decode(read, DEV)
        forced, status2 = mjpeg_in.decode(read, DEV, entropy="parallel")
        assert calls == ["serial", "parallel"] and status == status2 == [0, 0] and torch.equal(auto, forced)
    # a frame whose scan is cut: the serial routine's status from either decoder
    with open(path, "wb") as f:
        f.write(jm.avi_file([jpegs[0], jpegs[1][:len(jpegs[1]) // 2]], W, H))
    with mjpeg_in.MJPEGReader(path) as r:
        a, sa = mjpeg_in.decode(r.read([0, 1]), DEV, entropy="serial")
        b, sb = mjpeg_in.decode(r.read([0, 1]), DEV, entropy="parallel")
        assert sa == sb == [0, jdm.SHORT] and torch.equal(a, b)
