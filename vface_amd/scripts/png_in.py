"""The way in from a folder of PNG frames, decoded on the GPU: the counterpart of ``scripts/png.py``.

The reference writes the target clip as ``{index}.png`` (``REFace/scripts/VFace_inference_batch.py:285``) and reads the folder back
frame by frame with Pillow on one host core.  With ``--png_decoder gpu`` the host only walks each file's chunks (``parse_png``:
signature, CRC of every chunk, IHDR, the IDAT payloads joined, the zlib header), the deflate bodies cross to the device as they lie
in the files -- less than half of the RGB bytes even for a noisy frame -- and ``decode`` runs ``hip.png_inflate`` (RFC 1951, one
wave per file) and ``hip.png_unfilter`` (the five filter types, a skewed wavefront over the rows) of csrc/png_in.hip there.  The
host receives per file a status, two byte counts and the two halves of Adler-32, folds the checksum (``png.adler32_combine``) and
compares it with the file's.  There is no host inflate on this path.

- **8-bit, not interlaced**, colour type 2 (RGB), 6 (RGBA: alpha is dropped, as ``Image.convert("RGB")`` drops it) or 0 (grey:
  replicated).  ``tRNS``, ``gAMA`` and every other ancillary chunk are skipped, as ``convert("RGB")`` ignores them for these
  types.  Palette, grey + alpha, 16-bit and sub-byte depths and Adam7 are refused by name, as is a ``.jpg`` in the folder.
- Bytes of the zlib stream behind the final block's end and its Adler-32 are accepted, as libpng and Pillow accept them: the
  checksum is read where the decoder says the final block ended (``file_adler``).
- A file that does not decode ends the run with its name, the status by name and, for a filter byte above 4, the row.
- ``--png_in_inflate parallel`` (``decode(inflate="parallel")``) inflates one file on many waves, block by block
  (``hip.png_inflate_parallel``, csrc/png_in_par.hip): the same bytes, statuses and messages; ``auto`` picks by ``inflate_path``.
- The source image stays Pillow's: one image per clip.

The format is stated in ``tests/png_inflate_model.py``; it decodes what ``--png_encoder gpu`` wrote.
"""
from __future__ import annotations

import struct
import zlib
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from .png import SIGNATURE, adler32_combine

BPP = {2: 3, 6: 4, 0: 1}            # colour type -> bytes per pixel at 8 bits
MAX_W = 8192                        # hip.PNG_UNFILTER_MAX_W: the widest frame ``hip.png_unfilter`` takes
_COLOUR_NAMES = {3: "palette", 4: "grey + alpha"}
# hip.png_inflate's status (csrc/png_inflate.hpp: VfInfStatus)
INFLATE_STATUS = {1: "the deflate stream ends early", 2: "block type 3", 3: "stored block: LEN != ~NLEN",
                  4: "more than 286 literal/length or 30 distance codes", 5: "the code-length code is over-subscribed or incomplete",
                  6: "a code-length repeat with nothing to repeat, or past the last length", 7: "no end-of-block code",
                  8: "the literal/length code set is over-subscribed or incomplete", 9: "the distance code set is over-subscribed or incomplete",
                  10: "invalid literal/length code", 11: "invalid distance code", 12: "a distance reaches in front of the image's first byte",
                  13: "the stream holds more bytes than the image", 14: "the stream holds fewer bytes than the image"}


class PNGFile(NamedTuple):
    """What the device needs of one file."""
    path: str
    W: int
    H: int
    bpp: int
    body: bytes             # the deflate body: the zlib stream without its 2-byte header and its last 4 bytes
    adler: int              # those 4 bytes: the file's Adler-32 of the filtered rows (``file_adler``)


def _refuse(path, what):
    raise SystemExit(f"{path}: {what}")


def parse_png(data: bytes, path: str = "<png>") -> PNGFile:
    """One file's chunks: the signature, then every chunk up to IEND with its CRC checked; IHDR first, the IDAT payloads joined in
    order (any split: 1-byte and empty chunks too), every other chunk skipped.  What is not read raises ``SystemExit`` naming
    ``path`` and what was found."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        _refuse(path, f"no PNG signature (the file starts with {data[:8]!r})")
    pos, n = 8, len(data)
    head, idat, seen_idat, closed, ended = None, [], False, False, False
    while pos < n:
        if pos + 12 > n:
            _refuse(path, f"truncated: {n - pos} byte(s) at {pos} where a chunk should stand")
        size, kind = struct.unpack_from(">I4s", data, pos)
        if pos + 12 + size > n:
            _refuse(path, f"truncated: chunk {kind!r} at byte {pos} promises {size} bytes, {n - pos - 12} are left")
        payload = data[pos + 8:pos + 8 + size]
        if struct.unpack_from(">I", data, pos + 8 + size)[0] != zlib.crc32(payload, zlib.crc32(kind)):
            _refuse(path, f"chunk {kind!r} at byte {pos}: bad CRC")
        pos += 12 + size
        if head is None:
            if kind != b"IHDR":
                _refuse(path, f"no IHDR: the first chunk is {kind!r}")
            if size != 13:
                _refuse(path, f"an IHDR of {size} bytes")
            head = struct.unpack(">IIBBBBB", payload)
            continue
        if kind == b"IHDR":
            _refuse(path, "a second IHDR")
        if kind == b"IDAT":
            if closed:
                _refuse(path, "an IDAT after another chunk intervened: the IDAT chunks of a PNG are consecutive")
            seen_idat = True
            idat.append(payload)
        elif kind == b"IEND":
            ended = True
            break
        else:
            closed = seen_idat
            if not (kind[0] & 0x20):
                _refuse(path, f"critical chunk {kind!r} is not read")
    if head is None:
        _refuse(path, "no IHDR: the file holds no chunk")
    if not ended:
        _refuse(path, "no IEND: the file ends inside its chunks (truncated)")
    if not seen_idat:
        _refuse(path, "no IDAT: the file holds no image data")
    W, H, depth, colour, compression, filtering, interlace = head
    if W == 0 or H == 0:
        _refuse(path, f"an image of {W} x {H}")
    if colour in _COLOUR_NAMES:
        _refuse(path, f"{_COLOUR_NAMES[colour]} PNG (colour type {colour}): only RGB, RGBA and grey are decoded on the GPU; "
                      "convert the frames, or leave --png_decoder at pillow")
    if colour not in BPP:
        _refuse(path, f"colour type {colour}")
    if depth != 8:
        _refuse(path, f"bit depth {depth}: only 8-bit PNG is decoded on the GPU ({'16-bit' if depth == 16 else 'sub-byte'} samples); "
                      "convert the frames, or leave --png_decoder at pillow")
    if compression != 0 or filtering != 0:
        _refuse(path, f"compression method {compression}, filter method {filtering}: PNG defines only 0 and 0")
    if interlace != 0:
        _refuse(path, f"interlaced PNG (Adam7, interlace method {interlace}): not decoded on the GPU; convert the frames, or leave "
                      "--png_decoder at pillow")
    bpp = BPP[colour]
    if W > MAX_W:
        _refuse(path, f"{W} x {H}: frames wider than {MAX_W} pixels are not decoded on the GPU (the unfilter keeps one row of the image "
                      "in LDS); leave --png_decoder at pillow")
    if (1 + bpp * W) * H >= 1 << 31:
        _refuse(path, f"{W} x {H}: an image's filtered rows stay below 2^31 bytes")
    stream = b"".join(idat)
    if len(stream) < 2 + 4:
        _refuse(path, f"a zlib stream of {len(stream)} byte(s): shorter than its header and checksum")
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8:
        _refuse(path, f"zlib compression method {cmf & 15}: only deflate (8) is defined")
    if cmf >> 4 > 7:
        _refuse(path, f"zlib window size code {cmf >> 4}: above 7 (32 KiB)")
    if (cmf * 256 + flg) % 31:
        _refuse(path, "zlib header check (FCHECK) fails")
    if flg & 0x20:
        _refuse(path, "the zlib stream asks for a preset dictionary (FDICT): PNG has none")
    return PNGFile(path, W, H, bpp, stream[2:-4], struct.unpack(">I", stream[-4:])[0])


def file_adler(record: PNGFile, consumed: int):
    """The Adler-32 the FILE states for its rows, once the decoder has said where the final block ended: the four bytes behind
    ``body[:consumed]``.  They are ``record.adler`` where the stream ends with its checksum; a stream with bytes behind the
    checksum (libpng and Pillow accept them) carries it further in front.  None where fewer than four bytes follow."""
    if consumed == len(record.body):
        return record.adler
    tail = record.body[consumed:consumed + 4] + struct.pack(">I", record.adler)
    return struct.unpack(">I", tail[:4])[0] if consumed <= len(record.body) else None


class PNGFrames:
    """What ``PNGFolderReader.read`` returns: one ``PNGFile`` per frame asked for, in that order.  It behaves like the rows of a
    tensor where ``clip_io.ClipInputs.batch`` needs it to (``len``, ``frames[i]``, ``frames[row] = other[i]``, ``clone()``), and
    ``packed()`` lays the bodies out for the device."""

    def __init__(self, W: int, H: int, records: List[PNGFile]):
        self.W, self.H, self.records = W, H, list(records)

    def __len__(self):
        return len(self.records)

    def __getitem__(self, i):
        return self.records[i]

    def __setitem__(self, i, record: PNGFile):
        self.records[i] = record

    def clone(self):
        return PNGFrames(self.W, self.H, self.records)

    @property
    def paths(self):
        return [r.path for r in self.records]

    def packed(self, staging: Optional[torch.Tensor] = None) -> dict:
        """One pinned uint8 buffer for ONE upload -- offsets (int64 per file), lengths (int32 per file), then the bodies back to
        back -- and where its three parts lie: ``{"buffer", "files", "offsets_at", "lengths_at", "streams_at", "stream_bytes"}``.
        ``staging``: a pinned uint8 buffer to lay them out in if it is large enough (``decode`` keeps one between batches);
        ``buffer`` is then its front."""
        F = len(self.records)
        lengths = np.array([len(r.body) for r in self.records], np.int32)
        offsets = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.int64)]).astype(np.int64)
        streams_at = (12 * F + 15) & ~15
        stream_bytes = max(int(lengths.sum()), 1)       # (never empty)
        if staging is not None and staging.numel() >= streams_at + stream_bytes:
            buf = staging[:streams_at + stream_bytes]
        else:
            buf = torch.empty(streams_at + stream_bytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        host = buf.numpy()
        host[:8 * F] = offsets.view(np.uint8)
        host[8 * F:12 * F] = lengths.view(np.uint8)
        host[streams_at:] = 0
        host[streams_at:streams_at + int(lengths.sum())] = np.frombuffer(b"".join(r.body for r in self.records), np.uint8)
        return {"buffer": buf, "files": F, "offsets_at": 0, "lengths_at": 8 * F, "streams_at": streams_at, "stream_bytes": stream_bytes}


_staging = {}                       # decode's pinned upload buffer
INFLATE_MODES = ("auto", "serial", "parallel")
PARALLEL_CHUNK_BYTES = 16384        # hip.PNG_INFLATE_CHUNK_BYTES: about one of zlib's level-6 blocks of a noisy frame
# ``auto`` takes the parallel inflate where the mean deflate body of a batch exceeds this many bytes.  Source: tools/bench_png_in.py,
# profiles/r13_a_png_inflate_parallel_stages.jsonl ("Frames in, PNG: one stream on many waves"): Pillow's smooth 512 x 512
# file (0.12 MB, 3 segments) is where the two paths are level (51.5 against 57.9 ms), every Huffman-coded case above it gains 4.9x or
# more.  Body size cannot see stored-block files, where the serial inflate is a copy and wins.  The default of --png_in_inflate stays
# ``serial`` until the ``png_in`` stage has been timed in a production-size run.
PARALLEL_MIN_BODY_BYTES = 8 * PARALLEL_CHUNK_BYTES
last_info = None                    # the parallel inflate's info rows of the last ``decode`` (one int32 [F, 4] tensor per bpp group), or None


def inflate_path(mode: str, body_bytes: int, files: int) -> str:
    """Which inflate a batch of ``files`` deflate bodies of ``body_bytes`` bytes in all takes: ``mode`` itself, or for ``auto``
    ``"parallel"`` where the mean body exceeds ``PARALLEL_MIN_BODY_BYTES`` and ``"serial"`` otherwise."""
    if mode not in INFLATE_MODES:
        raise ValueError(f"inflate must be one of {INFLATE_MODES}; got {mode!r}")
    if mode != "auto":
        return mode
    return "parallel" if body_bytes > PARALLEL_MIN_BODY_BYTES * max(int(files), 1) else "serial"


def decode(frames: PNGFrames, device, inflate: str = "serial", chunk_bytes: Optional[int] = None) -> torch.Tensor:
    """``PNGFolderReader.read``'s result -> device uint8 [F, H, W, 3].  Per group of files with one bpp (a folder usually is one
    group): one upload of the packed bodies from pinned memory, one ``hip.png_inflate``, one ``hip.png_unfilter`` and one small copy
    back of status, produced, consumed, the Adler halves and the unfilter status.  A file that does not decode -- a non-zero
    status, an Adler-32 other than the file's, a filter byte above 4 -- raises ``SystemExit`` with its path.
    ``inflate``: ``"serial"`` (one wave per file), ``"parallel"`` (``hip.png_inflate_parallel``: many waves per file, chunks of
    ``chunk_bytes``, by default ``PARALLEL_CHUNK_BYTES``; the same bytes, statuses and messages) or ``"auto"`` (``inflate_path``)."""
    from .. import hip
    global last_info
    if inflate not in INFLATE_MODES:
        raise hip.VFaceHipError(f"png_in.decode: inflate must be one of {INFLATE_MODES}; got {inflate!r}")
    if not isinstance(frames, PNGFrames) or len(frames) == 0:
        raise hip.VFaceHipError("png_in.decode: frames must be what PNGFolderReader.read returned, at least one frame")
    device = torch.device(device)
    if device.type != "cuda":
        raise hip.VFaceHipError("png_in.decode: the decoder runs on the GPU (no CPU fallback)")
    W, H = frames.W, frames.H
    for r in frames.records:
        if (r.W, r.H) != (W, H):
            raise hip.VFaceHipError(f"png_in.decode: {r.path} is {r.W} x {r.H}, the batch is {W} x {H}")
    groups = {}
    for row, r in enumerate(frames.records):
        groups.setdefault(r.bpp, []).append(row)
    rgb, last_info = None, None
    for bpp, rows_of in groups.items():
        part = PNGFrames(W, H, [frames.records[i] for i in rows_of])
        p = part.packed(_staging.get("buffer"))
        if p["buffer"].numel() > _staging.get("bytes", 0):                      # pinned once, kept between batches, grown when needed
            _staging["buffer"], _staging["bytes"] = p["buffer"], p["buffer"].numel()
        F = p["files"]
        dev = p["buffer"].to(device, non_blocking=True)                         # the one upload (its bytes have crossed by the copy back)
        offsets = dev[:8 * F].view(torch.int64)
        lengths = dev[p["lengths_at"]:p["lengths_at"] + 4 * F].view(torch.int32)
        streams = dev[p["streams_at"]:]
        expect = (1 + bpp * W) * H
        meta = torch.empty((6, F), dtype=torch.int32, device=device)
        if inflate_path(inflate, sum(len(r.body) for r in part.records), F) == "parallel":
            rows, _, info = hip.png_inflate_parallel(streams, offsets, lengths, expect, chunk_bytes or PARALLEL_CHUNK_BYTES, meta=meta[:5])
            last_info = (last_info or []) + [info]
        else:
            rows, _ = hip.png_inflate(streams, offsets, lengths, expect, meta=meta[:5])
        out, _ = hip.png_unfilter(rows, W, H, bpp, meta[0], status=meta[5])
        status, produced, consumed, halves_a, halves_b, bad_row = meta.cpu().tolist()       # the one copy back
        halves = halves_a + halves_b                                            # [F][2], flat
        for f, r in enumerate(part.records):
            if status[f]:
                _refuse(r.path, f"does not decode: {INFLATE_STATUS.get(status[f], status[f])} (status {status[f]}, after {consumed[f]} of "
                                f"{len(r.body)} bytes of the deflate stream and {produced[f]} of {expect} bytes of the image)")
            adler = adler32_combine([(halves[2 * f], halves[2 * f + 1], produced[f])])
            stated = file_adler(r, consumed[f])
            if adler != stated:
                _refuse(r.path, f"does not decode: the Adler-32 of the decoded bytes is {adler:#010x}, the file says {stated:#010x}")
            if bad_row[f]:
                _refuse(r.path, f"does not decode: row {bad_row[f] - 1} has a filter type above 4")
        if len(groups) == 1:
            return out
        if rgb is None:
            rgb = torch.empty((len(frames), H, W, 3), dtype=torch.uint8, device=device)
        rgb[torch.tensor(rows_of, device=device)] = out
    return rgb


class PNGFolderReader:
    """A folder's ``{index}.png`` files behind what ``clip_io.ClipInputs`` asks of a reader: ``.W``, ``.H`` (the first file's IHDR: 33 bytes are read for it),
    ``len()``, ``read(indices) -> PNGFrames`` (indices into ``paths``) and ``to_rgb``.  ``read`` parses the files it is asked for;
    a frame of another size than the first is refused from its header."""
    stage = "png_in"                # the stage ``inputs.ClipRunInputs`` times this reader's work as: ``read`` and ``to_rgb``
    inflate = "serial"              # --png_in_inflate: which inflate ``to_rgb`` asks ``decode`` for

    def __init__(self, paths: List[str], path: str = "--target_frames"):
        self.path, self.paths = path, list(paths)
        if not self.paths:
            raise SystemExit(f"{path}: no frame files")
        for p in self.paths:
            if not p.lower().endswith(".png"):
                raise SystemExit(f"--png_decoder gpu: {p} is not a PNG file: JPEG frames in the folder are read by Pillow only; "
                                 "convert them, or leave --png_decoder at pillow")
        self.W, self.H = self._size(0)

    def _size(self, i):
        """(W, H) from the file's first 33 bytes -- the signature and the IHDR chunk -- alone; ``read`` checks the file."""
        with open(self.paths[i], "rb") as f:
            head = f.read(33)
        if len(head) < 33 or head[:8] != SIGNATURE or head[12:16] != b"IHDR":
            _refuse(self.paths[i], f"no PNG signature and IHDR (the file starts with {head[:16]!r})")
        return struct.unpack_from(">II", head, 16)

    def _parse(self, i) -> PNGFile:
        with open(self.paths[i], "rb") as f:
            return parse_png(f.read(), self.paths[i])

    def __len__(self):
        return len(self.paths)

    def read(self, indices) -> PNGFrames:
        records = []
        for i in (int(i) for i in indices):
            r = self._parse(i)
            if (r.W, r.H) != (self.W, self.H):
                raise SystemExit(f"--target_frames: {r.path} is {r.W} x {r.H}, the clip's first frames are {self.W} x {self.H}: the "
                                 f"frames of a clip must all be one size")
            records.append(r)
        return PNGFrames(self.W, self.H, records)

    def to_rgb(self, frames: PNGFrames, device) -> torch.Tensor:
        return decode(frames, device, inflate=self.inflate)

    def close(self):
        pass
