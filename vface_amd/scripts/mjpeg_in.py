"""The compressed way in for a target clip: Motion-JPEG in an AVI, the file ``scripts/mjpeg.py`` writes and the one ffmpeg
(``-c:v mjpeg``), capture cards and cameras produce.  The counterpart of ``scripts/demux.py``.

The reference hands the target video to ``cv2.VideoCapture`` (``REFace/scripts/VFace_inference_batch.py:240-285``).  H.264 stays
outside; baseline JPEG is built: the host walks the RIFF structure and parses each frame's HEADERS (``parse_jpeg``), the
entropy-coded scans cross to the device as they lie in the file -- about a tenth of the I420 bytes at quality 90 -- and
``decode`` runs ``hip.jpeg_scan_index`` (restart markers), ``hip.jpeg_decode_entropy`` (Huffman decoding, one lane per restart
interval), ``hip.jpeg_planes`` (dequantisation, inverse DCT) of csrc/mjpeg_in.hip and the existing ``hip.yuv420_to_rgb`` (JFIF:
full-range BT.601, centre-sited chroma) there.

- **8-bit baseline, 4:2:0, one scan of three components.**  Progressive, arithmetic-coded, 12-bit, 4:2:2 / 4:4:4 / grey frames,
  interlaced field pairs and DNL are refused by name; the conversion line is ``FFMPEG_LINE``.
- Tables and the restart interval may differ from frame to frame (ffmpeg writes Huffman tables per frame); a frame without DHT
  takes the typical tables of T.81 Annex K, as AVI MJPG frames commonly do.  Size and sampling are those of frame 0.
- **One RIFF only**: a file continued in ``AVIX`` chunks (OpenDML) is refused; ``indx`` / ``ix##`` chunks of a file that ends in its
  first RIFF are index data and are skipped.  Audio chunks are skipped.  Raw ``.mjpeg`` streams, QuickTime and MP4 are not read.
- A file without restart markers (ffmpeg's, Pillow's, most cameras') is ONE interval per frame: ``hip.jpeg_decode_entropy`` gives it
  one lane, ``hip.jpeg_decode_entropy_parallel`` cuts it into subsequences and decodes them on many lanes (csrc/jpeg_subseq.hpp).
  ``entropy_path`` chooses between the two; the coefficients are the same bit for bit.
"""
from __future__ import annotations

import os
import struct
from typing import Dict, List, NamedTuple, Tuple

import numpy as np
import torch

from .mjpeg import DHT, ZIGZAG

FFMPEG_LINE = "ffmpeg -i in -c:v mjpeg -pix_fmt yuvj420p clip.avi"
RIFF_MAGIC, AVI_MAGIC = b"RIFF", b"AVI "
TABLE_BYTES = 6 * 384           # hip.JPEG_TABLE_BYTES: DC tables of Y, Cb, Cr, then the AC tables (csrc/jpeg_interval.hpp)
_UNZIGZAG = np.array(ZIGZAG, np.int64)
_SOF_NAMES = {0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
              0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)",
              0xCA: "arithmetic coding, progressive (SOF10)", 0xCB: "arithmetic coding, lossless (SOF11)",
              0xCD: "arithmetic coding, differential (SOF13)", 0xCE: "arithmetic coding, differential progressive (SOF14)",
              0xCF: "arithmetic coding, differential lossless (SOF15)"}


class JpegFrame(NamedTuple):
    W: int
    H: int
    quant: Dict[int, np.ndarray]            # table id -> uint8 [64], row-major
    components: Tuple[tuple, ...]           # per component in scan order: (id, h, v, quantisation table, DC table, AC table)
    huffman: Dict[tuple, tuple]             # (class, id) -> (BITS, HUFFVAL)
    restart: int                            # MCUs per restart interval; 0 = none
    scan: Tuple[int, int]                   # [lo, hi) of the entropy-coded segment in the frame's bytes


def mcu_count(W: int, H: int) -> int:
    return ((int(W) + 15) // 16) * ((int(H) + 15) // 16)


def _refuse(path, k, what):
    raise SystemExit(f"{path}: frame {k}: {what}")


def parse_jpeg(data: bytes, path: str = "<jpeg>", k: int = 0) -> JpegFrame:
    """The headers of one frame: every segment up to SOS, then the extent of the scan.  Segments in any legal order, several
    tables per DQT / DHT, APPn and COM skipped, ``DRI 0`` = no restart interval, no DHT = the Annex-K tables.  What is not read
    raises ``SystemExit`` naming ``path``, frame ``k`` and what was found."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xFF\xD8":
        _refuse(path, k, f"no JPEG start-of-image marker (the chunk starts with {data[:4]!r})")
    quant, huffman = {}, {(cls_id >> 4, cls_id & 15): (tuple(bits), tuple(vals)) for cls_id, bits, vals in DHT}
    sof, restart, pos = None, 0, 2
    while True:
        if pos + 4 > n:
            _refuse(path, k, "the headers end before a start-of-scan marker (truncated frame)")
        if data[pos] != 0xFF:
            _refuse(path, k, f"byte {pos}: {data[pos]:#04x} where a marker should stand")
        marker = data[pos + 1]
        if marker == 0xFF:                          # fill byte
            pos += 1
            continue
        size = struct.unpack_from(">H", data, pos + 2)[0]
        body, end = pos + 4, pos + 2 + size
        if size < 2 or end > n:
            _refuse(path, k, f"segment {marker:#04x} at byte {pos} runs past the frame (truncated frame)")
        seg = data[body:end]
        if marker in (0xC0, 0xC1):
            if sof is not None:
                _refuse(path, k, "a second frame header (SOF)")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                _refuse(path, k, "a frame header (SOF) of the wrong length")
            if seg[0] != 8:
                _refuse(path, k, f"sample precision {seg[0]}: only 8-bit JPEG is read")
            H, W = struct.unpack_from(">HH", seg, 1)
            if H == 0:
                _refuse(path, k, "the frame height is left to a DNL segment: not read")
            if W == 0:
                _refuse(path, k, "a frame width of 0")
            sof = (W, H, tuple((seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])))
        elif marker in _SOF_NAMES:
            _refuse(path, k, f"{_SOF_NAMES[marker]} JPEG: only baseline Huffman-coded JPEG is read; convert with `{FFMPEG_LINE}`")
        elif marker == 0xCC:
            _refuse(path, k, f"arithmetic coding (a DAC segment): only Huffman-coded JPEG is read; convert with `{FFMPEG_LINE}`")
        elif marker == 0xDC:
            _refuse(path, k, "a DNL segment (the number of lines defined after the scan): not read")
        elif marker == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                if pq != 0:
                    _refuse(path, k, f"quantisation table {tq} has 16-bit entries: only 8-bit baseline tables are read")
                if tq > 3 or at + 65 > len(seg):
                    _refuse(path, k, f"a DQT segment that does not hold whole tables (id {tq})")
                table = np.zeros(64, np.uint8)
                table[_UNZIGZAG] = np.frombuffer(seg, np.uint8, 64, at + 1)
                if not table.all():
                    _refuse(path, k, f"quantisation table {tq} holds a 0")
                quant[tq] = table
                at += 65
        elif marker == 0xC4:
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    _refuse(path, k, "a DHT segment that does not hold whole tables")
                tc, th = seg[at] >> 4, seg[at] & 15
                bits = tuple(seg[at + 1:at + 17])
                count = sum(bits)
                if tc > 1 or th > 3 or count > 256 or at + 17 + count > len(seg):
                    _refuse(path, k, f"a DHT segment that does not hold whole tables (class {tc}, id {th}, {count} symbols)")
                code = 0
                for length, nb in enumerate(bits, 1):
                    code = (code + nb) << 1
                    if code > (2 << length):
                        _refuse(path, k, f"Huffman table (class {tc}, id {th}) is no prefix code: too many codes of {length} bits")
                huffman[(tc, th)] = (bits, tuple(seg[at + 17:at + 17 + count]))
                at += 17 + count
        elif marker == 0xDD:
            if len(seg) != 2:
                _refuse(path, k, "a DRI segment of the wrong length")
            restart = struct.unpack(">H", seg)[0]
        elif marker == 0xE0 and seg[:4] == b"AVI1" and len(seg) > 4 and seg[4] != 0:
            _refuse(path, k, f"an AVI1 segment with polarity {seg[4]}: one field of an interlaced pair; deinterlace first "
                             f"(`{FFMPEG_LINE} -vf yadif`)")
        elif marker == 0xDA:
            break
        elif 0xE0 <= marker <= 0xEF or marker == 0xFE:
            pass                                    # APPn, COM
        elif marker in (0xD8, 0xD9, 0x01) or 0xD0 <= marker <= 0xD7:
            _refuse(path, k, f"marker {marker:#04x} at byte {pos}, before the scan")
        pos = end
    if sof is None:
        _refuse(path, k, "a scan before any frame header (SOF)")
    W, H, comps = sof
    sampling = tuple((h, v) for _, h, v, _ in comps)
    if sampling != ((2, 2), (1, 1), (1, 1)):
        names = {((1, 1),): "greyscale", ((1, 1),) * 3: "4:4:4", ((2, 1), (1, 1), (1, 1)): "4:2:2", ((1, 2), (1, 1), (1, 1)): "4:4:0"}
        shown = names.get(sampling, "sampling " + " ".join(f"{h}x{v}" for h, v in sampling))
        _refuse(path, k, f"{shown}: only 4:2:0 (Y 2x2, Cb 1x1, Cr 1x1) is read; convert with `{FFMPEG_LINE}`")
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        _refuse(path, k, "a scan header (SOS) of the wrong length")
    if seg[0] != 3 or tuple(seg[1 + 2 * i] for i in range(3)) != tuple(c[0] for c in comps):
        _refuse(path, k, f"a scan of {seg[0]} component(s): only one interleaved scan of all three components is read")
    ss, se, ahal = seg[7], seg[8], seg[9]
    if (ss, se, ahal) != (0, 63, 0):
        _refuse(path, k, f"a scan with Ss = {ss}, Se = {se}, Ah/Al = {ahal:#04x}: only the sequential scan 0..63 is read")
    components = []
    for i, (cid, h, v, tq) in enumerate(comps):
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if tq not in quant:
            _refuse(path, k, f"component {cid} names quantisation table {tq}, which the frame does not define")
        for cls, th in ((0, td), (1, ta)):
            if (cls, th) not in huffman:
                _refuse(path, k, f"component {cid} names Huffman table (class {cls}, id {th}), which the frame does not define")
        components.append((cid, h, v, tq, td, ta))
    lo = end
    # inside a scan FF is followed by 00 or RSTm (or FF: fill); the first other marker ends it
    arr = np.frombuffer(data, np.uint8)
    ff = lo + np.flatnonzero(arr[lo:n - 1] == 0xFF)
    nxt = arr[ff + 1]
    ends = ff[(nxt != 0) & ((nxt & 0xF8) != 0xD0) & (nxt != 0xFF)]
    hi = n
    if ends.size:
        hi, marker = int(ends[0]), int(arr[ends[0] + 1])
        if marker == 0xDC:
            _refuse(path, k, "a DNL segment (the number of lines defined after the scan): not read")
        if marker != 0xD9:
            _refuse(path, k, f"marker {marker:#04x} after the scan: more than one scan is not read "
                             f"(progressive or non-interleaved JPEG); convert with `{FFMPEG_LINE}`")
    return JpegFrame(W, H, quant, tuple(components), huffman, restart, (lo, hi))


def huffman_table(bits, vals) -> np.ndarray:
    """(BITS, HUFFVAL) -> the 384 bytes ``VfJpegHuff`` of csrc/jpeg_interval.hpp: int32 maxcode[16] (-1 = no code of that length),
    int32 valoff[16] (index of the length's first symbol minus its first code), uint8 vals[256].  T.81 F.2.2.3."""
    out = np.zeros(96, np.int32)
    code = first = 0
    for length in range(16):
        nb = int(bits[length])
        out[length] = code + nb - 1 if nb else -1
        out[16 + length] = first - code
        first += nb
        code = (code + nb) << 1
    v = np.zeros(256, np.uint8)
    v[:len(vals)] = np.asarray(vals, np.uint8)[:256]
    return np.concatenate([out[:32].view(np.uint8), v])


def huffman_block(frame: JpegFrame) -> np.ndarray:
    """A frame's tables BY COMPONENT, uint8 [TABLE_BYTES]: the DC tables of Y, Cb, Cr, then their AC tables."""
    dc = [huffman_table(*frame.huffman[(0, c[4])]) for c in frame.components]
    ac = [huffman_table(*frame.huffman[(1, c[5])]) for c in frame.components]
    return np.concatenate(dc + ac)


def quant_block(frame: JpegFrame) -> np.ndarray:
    """A frame's quantisation tables by component, uint8 [3, 64], row-major."""
    return np.stack([frame.quant[c[3]] for c in frame.components])


class FrameRecord(NamedTuple):
    """What the device needs of one frame."""
    index: int
    scan: bytes
    restart: int
    quant: np.ndarray           # uint8 [3, 64]
    tables: np.ndarray          # uint8 [TABLE_BYTES]


class MJPEGFrames:
    """What ``MJPEGReader.read`` returns: one ``FrameRecord`` per frame asked for, in that order.  It behaves like the rows of a
    tensor where ``clip_io.ClipInputs.batch`` needs it to (``len``, ``frames[i]``, ``frames[row] = other[i]``, ``clone()``) and
    ``packed()`` lays the records out for the device: one flat buffer of the scans, per-frame offsets, lengths, restart intervals,
    quantisation tables and Huffman tables."""

    def __init__(self, path: str, W: int, H: int, records: List[FrameRecord]):
        self.path, self.W, self.H, self.records = path, W, H, list(records)

    def __len__(self):
        return len(self.records)

    def __getitem__(self, i):
        return self.records[i]

    def __setitem__(self, i, record: FrameRecord):
        self.records[i] = record

    def clone(self):
        return MJPEGFrames(self.path, self.W, self.H, self.records)

    @property
    def indices(self):
        return [r.index for r in self.records]

    def packed(self) -> dict:
        lengths = np.array([len(r.scan) for r in self.records], np.int32)
        offsets = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.int64)]).astype(np.int64)
        scans = np.frombuffer(b"".join(r.scan for r in self.records) + b"\0\0\0\0", np.uint8).copy()   # (never empty)
        return {"scans": torch.from_numpy(scans), "offsets": torch.from_numpy(offsets), "lengths": torch.from_numpy(lengths),
                "restart": torch.tensor([r.restart for r in self.records], dtype=torch.int32),
                "quant": torch.from_numpy(np.stack([r.quant for r in self.records])),
                "tables": torch.from_numpy(np.stack([r.tables for r in self.records]))}


# ``entropy="auto"`` takes the parallel decoder once the longest restart interval of a call averages this many scan bytes: just under
# the shortest intervals tools/bench_mjpeg_in.py measured (the writer's 512 x 512 frames, one interval per MCU row, 1789 bytes on
# average), where the parallel form already wins by 1.46x; it wins by more on every longer one.  Shorter intervals were
# not measured and stay serial.
PARALLEL_MIN_INTERVAL_BYTES = 1750
SUBSEQ_BYTES = 256              # the parallel decoder's subsequence size: beats the serial form on every case of the sweep (so does 512)


def entropy_path(frames: "MJPEGFrames", mcus: int) -> str:
    """``"serial"`` | ``"parallel"`` for one ``decode`` call, from the host's records alone: parallel when the largest
    ``len(scan) / interval count`` of the call reaches ``PARALLEL_MIN_INTERVAL_BYTES`` -- every file without restart markers but
    the smallest, and files with restart markers whose intervals are long."""
    from ..hip import jpeg_interval_count
    longest = max(len(r.scan) / jpeg_interval_count(mcus, r.restart) for r in frames.records)
    return "parallel" if longest >= PARALLEL_MIN_INTERVAL_BYTES else "serial"


def decode(frames: MJPEGFrames, device, chroma: str = "centre", entropy: str = "auto"):
    """``MJPEGReader.read``'s result -> ``(rgb, status)``: device uint8 [F, H, W, 3] and the per-frame status as a host list
    (0 = decoded; ``hip.JPEG_STATUS`` names the others -- such a frame's pixels are those of the coefficients that were decoded
    before the fault, zeros behind them).  ``chroma``: centre (JFIF's siting; the (3, 1)/4 weights are libjpeg's "fancy"
    upsampling) | nearest.  ``entropy``: serial (one lane per restart interval) | parallel (many lanes inside an interval) | auto
    (``entropy_path``); the result does not depend on it.  A handful of launches and one copy of the statuses; there is no host
    decoder."""
    from .. import hip
    if entropy not in ("auto", "serial", "parallel"):
        raise hip.VFaceHipError(f"mjpeg_in.decode: entropy is auto, serial or parallel; got {entropy!r}")
    if not isinstance(frames, MJPEGFrames) or len(frames) == 0:
        raise hip.VFaceHipError("mjpeg_in.decode: frames must be what MJPEGReader.read returned, at least one frame")
    device = torch.device(device)
    if device.type != "cuda":
        raise hip.VFaceHipError("mjpeg_in.decode: the decoder runs on the GPU (no CPU fallback)")
    if chroma not in ("centre", "nearest"):
        raise hip.VFaceHipError(f"mjpeg_in.decode: chroma is centre or nearest; got {chroma!r}")
    p = {name: t.to(device) for name, t in frames.packed().items()}
    mcus = mcu_count(frames.W, frames.H)
    most = max(hip.jpeg_interval_count(mcus, r.restart) for r in frames.records)
    ranges, status = hip.jpeg_scan_index(p["scans"], p["offsets"], p["lengths"], p["restart"], mcus, most)
    if (entropy_path(frames, mcus) if entropy == "auto" else entropy) == "parallel":
        coef, status = hip.jpeg_decode_entropy_parallel(p["scans"], ranges, status, p["restart"], p["tables"], mcus, SUBSEQ_BYTES)
    else:
        coef, status = hip.jpeg_decode_entropy(p["scans"], ranges, status, p["restart"], p["tables"], mcus)
    rows = hip.jpeg_planes(coef, p["quant"], frames.W, frames.H)
    rgb = hip.yuv420_to_rgb(rows, frames.W, frames.H, matrix="bt601", full_range=True, chroma=chroma)
    return rgb, status.cpu().tolist()


class MJPEGReader:
    """``MJPEGReader(path)``: ``.W``, ``.H``, ``.fps`` (rate, scale), ``len()`` = the frame count, ``read(indices)`` = an
    ``MJPEGFrames`` in the order asked for.  The RIFF structure is walked on open by ``seek`` (the frames themselves are only read
    by ``read``): ``avih`` must be there and the first video stream's handler or ``biCompression`` must say MJPG; the frames come
    from ``idx1`` where it is present and points at them, from a walk of ``movi`` otherwise.  A video chunk of zero length repeats
    the frame before it."""
    fixed_matrix = "bt601"          # JFIF fixes full-range BT.601: --video_in_matrix has nothing to say

    def __init__(self, path: str):
        self.path = path
        if not os.path.isfile(path):
            raise SystemExit(f"{path}: no such file (an AVI is read by seek; a pipe cannot be)")
        self._f = open(path, "rb")
        try:
            self._index()
        except BaseException:
            self.close()
            raise

    # ---- RIFF
    def _at(self, pos, n):
        self._f.seek(pos)
        return self._f.read(n)

    def _index(self):
        path = self.path
        size = os.fstat(self._f.fileno()).st_size
        head = self._at(0, 12)
        if len(head) < 12 or head[:4] != RIFF_MAGIC or head[8:12] != AVI_MAGIC:
            raise SystemExit(f"{path}: does not start with 'RIFF....AVI ': this is not an AVI file; make one with `{FFMPEG_LINE}`")
        riff_end = 8 + struct.unpack_from("<I", head, 4)[0]
        if riff_end > size:
            raise SystemExit(f"{path}: truncated: the RIFF header promises {riff_end} bytes, the file has {size}")
        self._avih = self._video = self._movi = None
        self._streams, idx1 = [], None
        pos = 12
        while pos + 8 <= riff_end:
            fourcc, n = struct.unpack("<4sI", self._at(pos, 8))
            body = pos + 8
            if body + n > riff_end:
                raise SystemExit(f"{path}: truncated: chunk {fourcc!r} at byte {pos} promises {n} bytes, {riff_end - body} are left")
            if fourcc == b"LIST":
                kind = self._at(body, 4)
                if kind == b"hdrl":
                    self._header_list(self._at(body + 4, n - 4))
                elif kind == b"movi":
                    self._movi = (body, body + n)           # from the 'movi' fourcc: idx1 offsets count from it
            elif fourcc == b"idx1":
                idx1 = self._at(body, n)
            pos = body + n + (n & 1)
        if riff_end + 12 <= size and self._at(riff_end, 4) == RIFF_MAGIC and self._at(riff_end + 8, 4) == b"AVIX":
            raise SystemExit(f"{path}: the file goes on in 'AVIX' chunks (OpenDML, AVI 2.0): only one RIFF is read; "
                             f"rewrite it under 1 GiB per file, or as `{FFMPEG_LINE}`")
        if self._avih is None:
            raise SystemExit(f"{path}: no 'avih' header: not a complete AVI file")
        if self._video is None:
            raise SystemExit(f"{path}: no video stream")
        number, handler, compression, self.fps = self._video
        if b"MJPG" not in (handler.upper(), compression.upper()):
            raise SystemExit(f"{path}: the video stream is {handler!r} / {compression!r}, not MJPG: only Motion-JPEG is decoded; "
                             f"convert with `{FFMPEG_LINE}`")
        if self._movi is None:
            raise SystemExit(f"{path}: no 'movi' list: the file holds no frames")
        tags = (b"%02ddc" % number, b"%02ddb" % number)
        self._chunks = self._from_idx1(idx1, tags) if idx1 else None
        if self._chunks is None:
            self._chunks = self._walk_movi(tags)
        # a zero-length chunk repeats the frame before it
        self._frames: List[Tuple[int, int]] = []
        for k, (at, n) in enumerate(self._chunks):
            if n == 0:
                if k == 0:
                    raise SystemExit(f"{path}: frame 0 is an empty chunk: there is no frame before it to repeat")
                self._frames.append(self._frames[-1])
            else:
                self._frames.append((at, n))
        self.W = self.H = None
        if self._frames:
            first = self._parse(0)
            self.W, self.H = first.W, first.H

    def _header_list(self, data: bytes):
        """The chunks of ``hdrl``: ``avih``, and of every ``strl`` its ``strh`` and ``strf``; the first video stream is kept."""
        def walk(lo, hi, stream):
            pos = lo
            while pos + 8 <= hi:
                fourcc, n = struct.unpack_from("<4sI", data, pos)
                body = pos + 8
                if body + n > hi:
                    raise SystemExit(f"{self.path}: truncated: header chunk {fourcc!r} runs past its list")
                if fourcc == b"LIST":
                    if data[body:body + 4] == b"strl":
                        s = {}
                        walk(body + 4, body + n, s)
                        self._streams.append(s)
                elif fourcc == b"avih":
                    self._avih = data[body:body + n]
                elif fourcc in (b"strh", b"strf") and stream is not None:
                    stream[fourcc] = data[body:body + n]
                pos = body + n + (n & 1)
        walk(0, len(data), None)
        for number, s in enumerate(self._streams):
            strh, strf = s.get(b"strh", b""), s.get(b"strf", b"")
            if len(strh) >= 32 and strh[:4] == b"vids" and self._video is None:
                scale, rate = struct.unpack_from("<II", strh, 20)
                self._video = (number, strh[4:8], strf[16:20] if len(strf) >= 20 else b"", (rate, scale))

    def _from_idx1(self, idx1: bytes, tags):
        """(position of the chunk's data, size) per video frame from the index, or None where the index does not point at the
        chunks it names (offsets count from the 'movi' fourcc, or in some writers from the start of the file)."""
        entries = [struct.unpack_from("<4sIII", idx1, 16 * i) for i in range(len(idx1) // 16)]
        video = [(off, n) for fourcc, _, off, n in entries if fourcc in tags]
        if not video:
            return None
        lo, hi = self._movi
        for base in (lo, 0):
            at = base + video[0][0]
            if lo <= at and at + 8 <= hi and self._at(at, 4) in tags:
                out = []
                for k, (off, n) in enumerate(video):
                    if base + off + 8 + n > hi:
                        raise SystemExit(f"{self.path}: frame {k} is truncated: the index places {n} bytes at {base + off}, "
                                         f"the 'movi' list ends at {hi}")
                    out.append((base + off + 8, n))
                return out
        return None

    def _walk_movi(self, tags):
        out, (lo, hi) = [], self._movi
        pos = lo + 4
        while pos + 8 <= hi:
            fourcc, n = struct.unpack("<4sI", self._at(pos, 8))
            if fourcc == b"LIST":                   # 'rec ' groups: only their framing is skipped
                pos += 12
                continue
            if pos + 8 + n > hi:
                raise SystemExit(f"{self.path}: frame {len(out)} is truncated: chunk {fourcc!r} at byte {pos} promises {n} bytes, "
                                 f"{hi - pos - 8} are left")
            if fourcc in tags:
                out.append((pos + 8, n))
            pos += 8 + n + (n & 1)
        return out

    # ---- frames
    def __len__(self):
        return len(self._frames)

    def frame_bytes(self, k) -> bytes:
        """The complete JPEG of frame ``k`` as it lies in the file: every frame is a ``.jpg`` of its own."""
        at, n = self._frames[k]
        data = self._at(at, n)
        if len(data) != n:
            raise SystemExit(f"{self.path}: frame {k} is truncated (the file changed while it was read)")
        return data

    def _parse(self, k):
        return parse_jpeg(self.frame_bytes(k), self.path, k)

    def read(self, indices) -> MJPEGFrames:
        if self._f is None:
            raise ValueError(f"{self.path} is closed")
        records = []
        for i in (int(i) for i in indices):
            if not 0 <= i < len(self._frames):
                raise IndexError(f"{self.path}: frame {i} of {len(self._frames)}")
            data = self.frame_bytes(i)
            frame = parse_jpeg(data, self.path, i)
            if (frame.W, frame.H) != (self.W, self.H):
                raise SystemExit(f"{self.path}: frame {i} is {frame.W} x {frame.H}, frame 0 is {self.W} x {self.H}: the frames of a clip "
                                 f"must all be one size")
            records.append(FrameRecord(i, data[frame.scan[0]:frame.scan[1]], frame.restart, quant_block(frame), huffman_block(frame)))
        return MJPEGFrames(self.path, self.W, self.H, records)

    def to_rgb(self, frames: MJPEGFrames, device, matrix=None, chroma_upsample: str = "sited", entropy: str = "auto") -> torch.Tensor:
        """The common surface of the readers (``demux.Y4MReader.to_rgb``): what ``read`` returned -> device uint8 [F, H, W, 3].
        ``entropy``: ``decode``'s.  A frame that does not decode ends the run."""
        from .. import hip
        rgb, status = decode(frames, device, "nearest" if chroma_upsample == "nearest" else "centre", entropy)
        for record, code in zip(frames.records, status):
            if code:
                raise SystemExit(f"{self.path}: frame {record.index} does not decode: {hip.JPEG_STATUS.get(code, code)} (status {code})")
        return rgb

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def open_video(path: str):
    """The reader of ``--target_video``, chosen by the file's first 12 bytes, not by its name: ``YUV4MPEG2`` = ``demux.Y4MReader``,
    ``RIFF....AVI `` = ``MJPEGReader``; anything else gets the Y4M reader's refusal."""
    from .demux import Y4MReader
    head = b""
    if os.path.isfile(path):
        with open(path, "rb") as f:
            head = f.read(12)
    if head[:4] == RIFF_MAGIC and head[8:12] == AVI_MAGIC:
        return MJPEGReader(path)
    return Y4MReader(path)
