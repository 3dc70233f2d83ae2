"""vface_jpeg_scan_index, vface_jpeg_decode_entropy and vface_jpeg_planes (csrc/mjpeg_in.hip) against the decoder model
(tests/jpeg_decode_model.py), bit for bit; ``mjpeg_in.decode`` end to end on files Pillow and ``MJPEGWriter`` wrote.

The corruption cases show that bad bytes are refused without anything outside the buffers being touched.  Every one of them,
and 20 000 mutations besides, has passed the interval decoder's host program under sanitizers first
(tests/test_mjpeg_in_cpu.py::test_interval_decoder_under_sanitizers): nothing here is meant to provoke anything."""
import numpy as np
import pytest
import torch

import demux_model as dm
import jpeg_decode_model as jdm
import jpeg_model as jm
import mjpeg_in_cases as cases
from test_mjpeg_gpu import SIZES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL16, SENTINEL8, SENTINEL32 = 0x5A5A, 0xA5, -7
SCAN_GRID_CAP = 1024        # kScanGridCap of csrc/mjpeg_in.hip: workgroups of one frame before the grid loops
DECODE_GRID_CAP = 4096      # kDecodeGridCap: workgroups of one wave (64 intervals of one frame) before the grid loops
PLANES_GRID_CAP, MCU_PER_GROUP = 2048, 4


def table_block(huffman):
    from vface_amd.scripts import mjpeg_in
    return np.concatenate([mjpeg_in.huffman_table(*t) for t in huffman[0]] + [mjpeg_in.huffman_table(*t) for t in huffman[1]])


ANNEX_K_BLOCK = None


def annex_k_block():
    global ANNEX_K_BLOCK
    if ANNEX_K_BLOCK is None:
        ANNEX_K_BLOCK = table_block(cases.ANNEX_K)
    return ANNEX_K_BLOCK


def run_decoder(frames, mcus, gap=5, lead=3, decode=True):
    """``frames``: [(scan bytes, restart, table block)] of ``mcus`` MCUs each, through the two entry points at the C ABI with every
    buffer inside sentinels: the scans between 64 sentinel bytes, the ranges and statuses inside int32 sentinels, the coefficients
    a strided view at element ``lead`` of an int16 sentinel buffer, frames ``mcus * 384 + gap`` apart.
    -> dict(ranges [F, most, 2] relative to the scans' start, index_status, status, coef, clean)."""
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
    ranges = torch.full((8 + F * most * 2 + 8,), SENTINEL32, dtype=torch.int32, device=DEV)
    status = torch.full((4 + F + 4,), SENTINEL32, dtype=torch.int32, device=DEV)
    d_off, d_len = torch.from_numpy(offsets).to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV)
    d_restart = torch.tensor([f[1] for f in frames], dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    scan_ptr, nbytes = scans.data_ptr() + 64, max(total, 1)
    rc = lib.vface_jpeg_scan_index(scan_ptr, nbytes, d_off.data_ptr(), d_len.data_ptr(), d_restart.data_ptr(), mcus, F, most,
                                   ranges.data_ptr() + 32, status.data_ptr() + 16, stream)
    assert rc == 0
    torch.cuda.synchronize()
    out = {"index_status": status[4:4 + F].cpu().numpy().copy(), "ranges": ranges[8:8 + F * most * 2].cpu().numpy().reshape(F, most, 2).copy()}
    n, stride = mcus * 384, mcus * 384 + gap
    buf = torch.full((lead + F * stride + 64,), SENTINEL16, dtype=torch.int16, device=DEV)
    if decode:
        tables = torch.from_numpy(np.stack([f[2] for f in frames])).to(DEV)
        rc = lib.vface_jpeg_decode_entropy(scan_ptr, nbytes, ranges.data_ptr() + 32, d_restart.data_ptr(), tables.data_ptr(), mcus, F, most,
                                           buf.data_ptr() + 2 * lead, stride, status.data_ptr() + 16, stream)
        assert rc == 0
        torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    outside = np.ones(whole.shape, bool)
    for f in range(F):
        outside[lead + f * stride:lead + f * stride + n] = False
    st, rg = status.cpu().numpy(), ranges.cpu().numpy()
    out["clean"] = (bool((whole[outside] == SENTINEL16).all()) and bool((st[:4] == SENTINEL32).all() and (st[4 + F:] == SENTINEL32).all())
                    and bool((rg[:8] == SENTINEL32).all() and (rg[8 + F * most * 2:] == SENTINEL32).all()) and torch.equal(scans.cpu(), before))
    out["status"] = st[4:4 + F].copy()
    out["coef"] = np.stack([whole[lead + f * stride:lead + f * stride + n] for f in range(F)]).reshape(F, mcus, 6, 64)
    return out


def model_ranges(frames, mcus):
    """What vface_jpeg_scan_index must write: (ranges [F, most, 2] relative to the start of the scans, status [F])."""
    most = max(jdm.interval_count(mcus, f[1]) for f in frames)
    ranges, status, at = np.zeros((len(frames), most, 2), np.int32), np.zeros(len(frames), np.int32), 0
    for i, (scan, restart, _) in enumerate(frames):
        got, status[i] = jdm.split_intervals(scan, mcus, restart)
        for j, (lo, hi) in enumerate(got):
            ranges[i, j] = (at + lo, at + hi)
        at += len(scan)
    return ranges, status


def stream_frames(prefix):
    return [(scan, restart, annex_k_block()) for name, coef, restart, scan in cases.round_trip_streams() if name.startswith(prefix)]


# ---- vface_jpeg_scan_index
@pytest.mark.parametrize("F", [1, 3])
def test_scan_index_equals_the_model(F):
    """250 x 136 = 144 MCUs with restart 1 (143 markers: the RST numbers wrap 17 times), one MCU row, and none; three frames of
    three lengths in one flat buffer, the longest several rounds of the workgroup's 2048 bytes."""
    frames = stream_frames("250x136_")
    assert [f[1] for f in frames] == [1, 16, 147] and len({len(f[0]) for f in frames}) == 3 and max(len(f[0]) for f in frames) > 3 * 2048
    for pick in ([[0], [1], [2]] if F == 1 else [[0, 1, 2], [2, 0, 1]]):
        chosen = [frames[i] for i in pick]
        got = run_decoder(chosen, 144, decode=False)
        want, status = model_ranges(chosen, 144)
        assert got["clean"] and np.array_equal(got["index_status"], status) and not status.any()
        assert np.array_equal(got["ranges"], want), pick
    assert len(jdm.split_intervals(frames[0][0], 144, 1)[0]) == 144


def test_scan_index_past_the_grid_cap():
    """More frames than workgroups, so the first workgroups take a second frame; frames of 2 MCUs at restart 1 and of one interval."""
    coef = cases.entropy_cases()["partial_last_interval"][0][0]
    kinds = [(jm.scan_bytes(coef[i:i + 2], r or 2), r, annex_k_block()) for i in range(3) for r in (1, 0)]
    frames = [kinds[(i * 5) % len(kinds)] for i in range(SCAN_GRID_CAP + 37)]
    got = run_decoder(frames, 2, gap=0, lead=0)
    want, status = model_ranges(frames, 2)
    assert got["clean"] and np.array_equal(got["ranges"], want) and not got["status"].any() and not status.any()
    for i in (0, 1, SCAN_GRID_CAP - 1, SCAN_GRID_CAP, len(frames) - 1):
        assert np.array_equal(got["coef"][i], jdm.decode_scan(frames[i][0], 2, frames[i][1], cases.ANNEX_K)[0]), i


def test_scan_index_refuses_wrong_markers():
    """A wrong marker count and a wrong marker order each give their status, a row of zeros and cleared coefficients; the frames
    round them decode; nothing else is written."""
    good = stream_frames("250x136_r16")[0]
    scan = good[0]
    assert all(scan.count(bytes([0xFF, 0xD0 + m])) == 1 for m in range(8))
    fewer = scan.replace(b"\xFF\xD5", b"\x12\x34")
    more = scan[:100] + b"\xFF\xD1" + scan[100:]
    swapped = scan.replace(b"\xFF\xD3", b"\xFF\xD4")
    frames = [good, (fewer, 16, good[2]), good, (more, 16, good[2]), (swapped, 16, good[2]), good]
    got = run_decoder(frames, 144)
    want, status = model_ranges(frames, 144)
    assert status.tolist() == [0, jdm.MARKER_COUNT, 0, jdm.MARKER_COUNT, jdm.MARKER_ORDER, 0]
    assert got["clean"] and np.array_equal(got["index_status"], status) and np.array_equal(got["status"], status)
    assert np.array_equal(got["ranges"], want) and not got["ranges"][[1, 3, 4]].any()
    exact = jdm.decode_scan(scan, 144, 16, cases.ANNEX_K)[0]
    for i, s in enumerate(status):
        assert np.array_equal(got["coef"][i], exact if s == 0 else np.zeros_like(exact)), i


# ---- vface_jpeg_decode_entropy
def test_decode_entropy_equals_the_model_on_the_round_trip_list():
    """Every stream of the encoder model: the coefficients it was made from, bit for bit, in a strided view inside sentinels."""
    for i, (name, coef, restart, scan) in enumerate(cases.round_trip_streams()):
        got = run_decoder([(scan, restart, annex_k_block())], coef.shape[0], gap=(0 if i == 0 else 3 + 8 * (i % 5)), lead=i % 4)
        assert got["status"].tolist() == [0] and got["clean"], name
        bad = np.argwhere(got["coef"][0] != coef)
        assert bad.size == 0, f"{name}: {len(bad)} coefficients differ, first at (mcu, block, k) {tuple(bad[0])}"


def test_decode_entropy_past_the_grid_cap():
    """More (frame, chunk) items than workgroups, so the first workgroups stage a second frame's tables and decode it: frames of 2
    MCUs at restart 1 and of one interval, two table sets in turn; every frame against the model."""
    coef = cases.entropy_cases()["partial_last_interval"][0][0]
    kinds = [(jm.scan_bytes(coef[i:i + 2], r or 2), r, annex_k_block()) for i in range(3) for r in (1, 0)]
    # the same bytes read with the luma and chroma tables exchanged: another frame as far as the decoder can tell (it ends in a status)
    other = ([jm.DC_CHROMA, jm.DC_LUMA, jm.DC_LUMA], [jm.AC_CHROMA, jm.AC_LUMA, jm.AC_LUMA])
    swapped = table_block(other)
    kinds += [(scan, r, swapped) for scan, r, _ in kinds[:2]]
    want = [jdm.decode_scan(scan, 2, r, cases.ANNEX_K if block is annex_k_block() else other) for scan, r, block in kinds]
    assert not any(status for _, status in want[:6]) and len({w[0].tobytes() for w in want}) >= 4
    pick = [(i * 5) % len(kinds) for i in range(DECODE_GRID_CAP + 37)]
    got = run_decoder([kinds[k] for k in pick], 2, gap=1, lead=1)
    assert got["clean"]
    for i, k in enumerate(pick):
        assert got["status"][i] == want[k][1] and np.array_equal(got["coef"][i], want[k][0]), (i, k)


def test_decode_entropy_equals_the_model_on_the_pillow_list():
    """Frames libjpeg-turbo wrote: optimised tables, restart intervals in blocks and rows, own quantisation tables, no DHT, merged
    segments.  The tables come from the frame's headers (``mjpeg_in.parse_jpeg`` / ``huffman_block``)."""
    from vface_amd.scripts import mjpeg_in
    decoded = cases.decoded_pillow_frames()
    for i, (name, W, H, jpeg) in enumerate(cases.pillow_frames()):
        frame = mjpeg_in.parse_jpeg(jpeg)
        coef, status, _, _, _ = decoded[name]
        got = run_decoder([(jpeg[frame.scan[0]:frame.scan[1]], frame.restart, mjpeg_in.huffman_block(frame))], coef.shape[0], lead=i % 2)
        assert got["status"].tolist() == [0] == [status] and got["clean"], name
        assert np.array_equal(got["coef"][0], coef), name


def test_three_frames_with_three_table_sets_in_one_call():
    from vface_amd.scripts import mjpeg_in
    by_name = {name: jpeg for name, W, H, jpeg in cases.pillow_frames()}
    names = ["optimize_130x50_edges", "merged_tables_130x50_smooth", "restart_rows_130x50_smooth"]
    parsed = [mjpeg_in.parse_jpeg(by_name[n]) for n in names]
    frames = [(by_name[n][p.scan[0]:p.scan[1]], p.restart, mjpeg_in.huffman_block(p)) for n, p in zip(names, parsed)]
    assert len({f[2].tobytes() for f in frames}) == 3 and [f[1] for f in frames] == [0, 0, 9]
    got = run_decoder(frames, 36)
    assert got["clean"] and not got["status"].any()
    for i, n in enumerate(names):
        assert np.array_equal(got["coef"][i], cases.decoded_pillow_frames()[n][0]), n


def test_entropy_coder_then_decoder_is_the_identity():
    """hip.jpeg_entropy -> hip.jpeg_scan_index -> hip.jpeg_decode_entropy gives back random coefficients an encoder can produce
    (``jdm.legal_coefficients``: the quantised DCT of random, saturated and flat blocks at qualities 30, 90 and 100), three frames of
    the 144 MCUs of 250 x 136, at restart intervals of a row, of 1 and of the frame; through the wrappers."""
    from vface_amd import hip
    rng = np.random.default_rng(14)
    host = np.concatenate([jdm.legal_coefficients(rng, quality, 6 * 144)[0] for quality in (30, 90, 100)])
    assert host.shape == (3, 144, 6, 64) and np.abs(host[..., 0]).max() <= 1024 and np.abs(host[..., 1:]).max() <= 1023 and host.any(axis=(1, 2, 3)).all()
    coef = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
    for restart in (16, 1, 144):
        scans, lengths = hip.jpeg_entropy(coef, restart)
        offsets = torch.cumsum(lengths.to(torch.int64), 0) - lengths
        used = scans[:int(lengths.sum())]
        r = torch.full((3,), restart, dtype=torch.int32, device=DEV)
        ranges, status = hip.jpeg_scan_index(used, offsets, lengths, r, 144, hip.jpeg_interval_count(144, restart))
        tables = torch.from_numpy(annex_k_block()).to(DEV).repeat(3, 1)
        back, status = hip.jpeg_decode_entropy(used, ranges, status, r, tables, 144)
        assert status.cpu().tolist() == [0, 0, 0] and tuple(back.shape) == (3, 144, 6, 64)
        assert torch.equal(back, coef), restart


CORRUPT = sorted(cases.corruption_cases()) + ["category_12"]


@pytest.mark.parametrize("name", CORRUPT)
def test_bad_bytes_are_refused_inside_the_buffers(name):
    """One corrupt frame between two good ones: the model's status and the model's coefficients (what was decoded before the fault,
    zeros behind it); the frames round it decode exactly; the sentinels round the coefficients, the statuses, the ranges and the
    scans are intact.  (Each case has passed the host program under sanitizers, tests/test_mjpeg_in_cpu.py.)"""
    if name == "category_12":
        scan, huffman = cases.category12_tables()
        mcus, restart, want, block = 1, 0, jdm.DC_CATEGORY, table_block(huffman)
    else:
        (scan, mcus, restart, want), huffman, block = cases.corruption_cases()[name], cases.ANNEX_K, annex_k_block()
    good_coef = jm.coefficients(jm.patterns(2, 48 if mcus == 6 else 16, 32 if mcus == 6 else 16, seed=6)["noise"], *jm.quant_tables(90)).reshape(2, mcus, 6, 64)
    goods = [(jm.scan_bytes(good_coef[0], 2), 2, annex_k_block()), (jm.scan_bytes(good_coef[1], mcus), 0, annex_k_block())]
    frames = [goods[0], (scan, restart, block), goods[1]]
    got = run_decoder(frames, mcus)
    model, status = jdm.decode_scan(scan, mcus, restart, huffman)
    assert status == want and got["status"].tolist() == [0, want, 0], (got["status"], jdm.STATUS[want])
    assert got["clean"]
    assert np.array_equal(got["coef"][1], model) and np.array_equal(got["coef"][0], good_coef[0]) and np.array_equal(got["coef"][2], good_coef[1])


# ---- vface_jpeg_planes
def planes_in_sentinel(coef, quant, W, H, gap, lead):
    from vface_amd import hip
    F, nb = coef.shape[0], W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)
    stride = nb + gap
    buf = torch.full((lead + F * stride + 64,), SENTINEL8, dtype=torch.uint8, device=DEV)
    view = buf.as_strided((F, nb + min(gap, 2)), (stride, 1), lead)
    out = hip.jpeg_planes(torch.from_numpy(np.ascontiguousarray(coef)).to(DEV), torch.from_numpy(np.ascontiguousarray(quant)).to(DEV), W, H, out=view)
    assert out.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    outside = np.ones(whole.shape, bool)
    for f in range(F):
        outside[lead + f * stride:lead + f * stride + nb] = False
    return view[:, :nb].cpu().numpy(), bool((whole[outside] == SENTINEL8).all())


def assert_planes(got, coef, quant, W, H, what):
    want = jdm.planes(coef, quant, W, H)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} bytes differ, first at (frame, byte) {tuple(bad[0])}: got {got[tuple(bad[0])]}, model {want[tuple(bad[0])]}"


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("F", [1, 3])
def test_planes_equal_the_model(W, H, F):
    """Every size (below one block, one MCU, sides that are no multiple of 8 or 16, odd sides, more than one workgroup), 1 and 3
    frames with a quantisation table set per frame, rows with a gap between them at an odd byte inside sentinels."""
    qualities = (30, 90, 100)
    for i, name in enumerate(("smooth", "noise", "edges")):
        rgb = jm.patterns(F, W, H, seed=12)[name]
        tabs = [jm.quant_tables(qualities[(i + f) % 3]) for f in range(F)]
        coef = np.stack([jm.coefficients(rgb[f:f + 1], *tabs[f])[0] for f in range(F)]).reshape(F, -1, 6, 64)
        quant = np.stack([np.stack([t[0], t[1], t[1]]) for t in tabs]).astype(np.uint8)
        got, clean = planes_in_sentinel(coef, quant, W, H, gap=0 if i == 0 else 5 + 2 * i, lead=i)
        assert_planes(got, coef, quant, W, H, f"{name} {W}x{H} F={F}")
        assert clean, f"{name}: bytes outside the frames were written"


def test_planes_clamp_what_no_encoder_writes():
    """+-32767 everywhere and random int16 coefficients with Q = 255, 1 and per-component tables: the clamps of the model."""
    rng = np.random.default_rng(3)
    W, H = 48, 32
    coefs = np.stack([np.full((6, 6, 64), 32767, np.int16), np.full((6, 6, 64), -32768, np.int16),
                      rng.choice(np.array([-32768, 32767], np.int16), (6, 6, 64)), rng.integers(-32768, 32768, (6, 6, 64)).astype(np.int16),
                      rng.integers(-2100, 2100, (6, 6, 64)).astype(np.int16)])
    for quant in (np.full((5, 3, 64), 255, np.uint8), np.ones((5, 3, 64), np.uint8), rng.integers(1, 256, (5, 3, 64)).astype(np.uint8)):
        got, clean = planes_in_sentinel(coefs, quant, W, H, gap=7, lead=1)
        assert_planes(got, coefs, quant, W, H, "extremes")
        assert clean


def test_planes_past_the_grid_cap():
    W = H = 1450
    mr, mc = jm.mcu_grid(W, H)
    assert mr * mc > PLANES_GRID_CAP * MCU_PER_GROUP and (mr * mc) % MCU_PER_GROUP
    rng = np.random.default_rng(9)
    coef = (rng.integers(-30, 31, (1, mr * mc, 6, 64)) * (rng.random((1, mr * mc, 6, 64)) < 0.2)).astype(np.int16)
    coef[..., 0] = rng.integers(-60, 61, (1, mr * mc, 6))
    quant = np.stack([np.stack([t for t in (*jm.quant_tables(85), jm.quant_tables(85)[1])])]).astype(np.uint8)
    got, clean = planes_in_sentinel(coef, quant, W, H, gap=0, lead=0)
    assert_planes(got, coef, quant, W, H, "past the cap")
    assert clean


def test_wrappers_refuse_what_they_cannot_run():
    from vface_amd import hip
    ok = torch.zeros(2, 6, 6, 64, dtype=torch.int16, device=DEV)
    q = torch.ones(2, 3, 64, dtype=torch.uint8, device=DEV)
    assert tuple(hip.jpeg_planes(ok, q, 48, 32).shape) == (2, 48 * 32 + 2 * 24 * 16)
    for bad, bq, W, H in ((ok.cpu(), q, 48, 32), (ok.to(torch.int32), q, 48, 32), (ok, q[:1], 48, 32), (ok, q.cpu(), 48, 32), (ok, q, 64, 32),
                          (ok[..., :63], q, 48, 32), (ok, q.to(torch.int16), 48, 32)):
        with pytest.raises(hip.VFaceHipError):
            hip.jpeg_planes(bad, bq, W, H)
    with pytest.raises(hip.VFaceHipError):
        hip.jpeg_planes(ok, q, 48, 32, out=torch.zeros(2, 100, dtype=torch.uint8, device=DEV))
    scans = torch.zeros(64, dtype=torch.uint8, device=DEV)
    off, ln, r = torch.zeros(2, dtype=torch.int64, device=DEV), torch.full((2,), 32, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    ranges, status = hip.jpeg_scan_index(scans, off, ln, r, 6, 1)
    tables = torch.from_numpy(annex_k_block()).to(DEV).repeat(2, 1)
    for args in ((scans.cpu(), off, ln, r, 6, 1), (scans, off.to(torch.int32), ln, r, 6, 1), (scans, off, ln[:1], r, 6, 1), (scans, off, ln, r, 6, 7),
                 (scans, off, ln, r, 0, 1), (scans[:0], off, ln, r, 6, 1)):
        with pytest.raises(hip.VFaceHipError):
            hip.jpeg_scan_index(*args)
    for args in ((scans, ranges[:1], status, r, tables, 6), (scans, ranges, status[:1], r, tables, 6), (scans, ranges, status, r, tables[:, :100], 6),
                 (scans, ranges, status, r, tables.cpu(), 6), (scans, ranges.to(torch.int64), status, r, tables, 6)):
        with pytest.raises(hip.VFaceHipError):
            hip.jpeg_decode_entropy(*args)
    with pytest.raises(hip.VFaceHipError):
        hip.jpeg_decode_entropy(scans, ranges, status, r, tables, 6, out=torch.zeros(2, 6, 6, 64, dtype=torch.int32, device=DEV))
    lib = hip.load()
    assert lib.vface_jpeg_planes(ok.data_ptr(), 6 * 384 - 1, q.data_ptr(), 48, 32, 2, scans.data_ptr(), 4096, None) == -3
    assert lib.vface_jpeg_scan_index(scans.data_ptr(), 64, off.data_ptr(), ln.data_ptr(), r.data_ptr(), 6, 2, 7, ranges.data_ptr(), status.data_ptr(), None) == -3


# ---- mjpeg_in.decode end to end
def model_rgb(jpegs, chroma="centre"):
    out = []
    for jpeg in jpegs:
        coef, status, quant, W, H = jdm.decode_frame(jpeg)
        assert status == 0
        out.append(dm.i420_to_rgb(jdm.planes(coef[None], quant[None], W, H), W, H, "bt601", True, chroma)[0])
    return np.stack(out)


def test_decode_a_file_pillow_wrote(tmp_path):
    """Three 130 x 50 frames Pillow encoded, each with tables and a restart interval of its own, in an AVI: the model's RGB, bit for
    bit, in the order asked for, with both chroma modes; a frame whose scan is cut is named by ``to_rgb``."""
    from vface_amd import hip
    from vface_amd.scripts import mjpeg_in
    W, H = 130, 50
    how = (dict(quality=90, restart_marker_rows=1), dict(quality=60, optimize=True), dict(quality=100, restart_marker_blocks=2))
    jpegs = [cases.pillow_jpeg(jm.patterns(1, W, H, seed=40 + i)[p][0], **h) for i, (p, h) in enumerate(zip(("smooth", "edges", "noise"), how))]
    path = str(tmp_path / "pillow.avi")
    with open(path, "wb") as f:
        f.write(jm.avi_file(jpegs, W, H))
    with mjpeg_in.MJPEGReader(path) as r:
        read = r.read([2, 0, 1, 0])
        rgb, status = mjpeg_in.decode(read, DEV)
        assert status == [0, 0, 0, 0] and rgb.dtype == torch.uint8 and tuple(rgb.shape) == (4, H, W, 3)
        want = model_rgb(jpegs)
        assert np.array_equal(rgb.cpu().numpy(), want[[2, 0, 1, 0]])
        assert torch.equal(r.to_rgb(read, DEV, None, "sited"), rgb)
        assert np.array_equal(r.to_rgb(read, DEV, None, "nearest").cpu().numpy(), model_rgb(jpegs, "nearest")[[2, 0, 1, 0]])
        for bad in (read.packed(), None, mjpeg_in.MJPEGFrames(path, W, H, [])):
            with pytest.raises(hip.VFaceHipError):
                mjpeg_in.decode(bad, DEV)
        with pytest.raises(hip.VFaceHipError):
            mjpeg_in.decode(read, "cpu")
        with pytest.raises(hip.VFaceHipError):
            mjpeg_in.decode(read, DEV, chroma="left")
    cut = jpegs[1][:len(jpegs[1]) // 2]
    with open(path, "wb") as f:
        f.write(jm.avi_file([jpegs[0], jpegs[0], cut], W, H))
    with mjpeg_in.MJPEGReader(path) as r:
        rgb, status = mjpeg_in.decode(r.read([0, 2]), DEV)
        assert status == [0, jdm.SHORT] and np.array_equal(rgb[0].cpu().numpy(), want[0])
        with pytest.raises(SystemExit, match="pillow.avi: frame 2 does not decode: the bytes of a restart interval ran out"):
            r.to_rgb(r.read([1, 2]), DEV)


def test_writer_then_reader_on_the_device(tmp_path):
    """MJPEGWriter from device frames, MJPEGReader and ``decode`` back: the RGB the decoder model makes of the file's own frames
    (no encoder model in between), and within the 4 levels of tests/test_mjpeg_in_cpu.py RGB_BOUND of Pillow's decode of them."""
    import io
    from PIL import Image
    from vface_amd.scripts import mjpeg, mjpeg_in
    W, H = 250, 136
    rgb = jm.patterns(3, W, H, seed=9)["smooth"]
    path = str(tmp_path / "own.avi")
    with mjpeg.MJPEGWriter(path, W, H, quality=95) as w:
        w.write(torch.from_numpy(rgb).to(DEV))
    with mjpeg_in.MJPEGReader(path) as r:
        assert (r.W, r.H, len(r)) == (W, H, 3)
        back, status = mjpeg_in.decode(r.read([0, 1, 2]), DEV)
    assert status == [0, 0, 0]
    frames = jm.walk_riff(open(path, "rb").read())["frames"]
    assert np.array_equal(back.cpu().numpy(), model_rgb(frames))
    pillow = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in frames]).astype(int)
    assert np.abs(back.cpu().numpy().astype(int) - pillow).max() <= 4
