"""The dataset's PNG files decoded on the device: what `np.array(Image.open(path))` returns in LoadMultiImages and LoadSeg
(open_loop_training/code/datasets/pipelines/loading.py:40-49, :127-131), from the file bytes.  The host walks the chunks
(`parse_png`) and packs the zlib streams; inflate and unfilter run on the device (csrc/png.hip, tt_png_decode_u8 in
include/thinktwice_hip.h).  What stays in the loader is reading the files.

    decoder = png.PngDecoder()
    raw, depth_png, seg_png = decoder.decode_sample_batch(rgb_files, depth_files, seg_files)   # [B][T][N], [B][N], [B][N] of bytes
    depth, seg = labels.RawLabelDecoder(cfg.seg_label_idxs)(raw, depth_png, seg_png)

Specified for the files PIL writes (`Image.fromarray(a).save(path)`): 8-bit, non-interlaced, colour type 0 or 2.  Anything
else is a ValueError on the host.

Checksums.  By default none is checked.  `PngDecoder(verify=("adler32",))` verifies every zlib stream's Adler-32 on the device
against the scanlines the inflate wrote: that is the check `np.array(Image.open(path))` makes ("broken data stream"), so it
is the setting for parity with the reference loader.  `verify=("adler32", "crc32")`, or `verify=True`, also verifies every
IDAT chunk's CRC-32 on the device (tt_png_decode_u8_verified; the few dozen bytes of the other chunks are checked on the
host), which PIL does not.  A file that fails is an image status like any other decode error (TT_PNGV_BAD_ADLER32,
TT_PNGV_BAD_CRC32) and leaves its destination untouched.  `verify_crc=True` is the older all-host CRC check (zlib.crc32 over
every chunk: host time over the whole batch's file bytes).  `device_adler32` and `device_crc32` are the checksum kernels on
their own (tt_checksum_ranges_u8): zlib.adler32 / zlib.crc32 of byte ranges of a device tensor.

Segmented files.  A zlib stream has no restart points, so a PIL-written file is one wave's work.  `segment_png` (once per
dataset, on the host; `python -m thinktwice_amd.png_segment SRC DST` for a tree) writes a file's stream again with a full
flush after every R rows -- still one valid zlib stream in a valid PNG, the pixels and filter bytes untouched -- and records
the cut points in a private ancillary chunk, `ttSG`, before the first IDAT (big-endian: version u8 = 1, rows_per_segment u32,
num_segments u32 = ceil(H / R), then num_segments + 1 offsets u32 into the concatenated IDAT payload, offsets[0] = 2).  Segment
i, bytes [offsets[i], offsets[i + 1]), is whole non-final deflate blocks, the last one the empty stored block 00 00 FF FF, and
inflates alone to rows [i * R, min((i + 1) * R, H)); after the last segment come one empty final block and the Adler-32.
`read_segments` returns a file's index, checked against the file.  `PngDecoder(segments="auto")`, the default, decodes such a
file with one wave per segment (tt_png_decode_u8_segmented, csrc/png_segments.hip) and every other file as before, mixed
freely in one call, with the same results, statuses and `verify=`; "ignore" takes every file the old way, "require" makes a
file without an index a ValueError.  `parse_png` ignores the chunk, as it does any ancillary chunk."""
import bisect
import collections
import ctypes
import struct
import zlib

import numpy as np

from . import _lib
from .ops import check, lib, ptr

SIGNATURE = b"\x89PNG\r\n\x1a\n"
# idat_crcs: the CRC field of every IDAT chunk, one per piece of zlib_stream; only PngDecoder(verify="crc32") collects them
# segments: the file's SegmentIndex if it is to be decoded by segments, else None
PngInfo = collections.namedtuple("PngInfo", "width height channels zlib_stream idat_crcs segments", defaults=(None, None))
# The cut points of a segmented file (segment_png, read_segments): segment i is bytes [offsets[i], offsets[i + 1]) of the
# concatenated IDAT payload and inflates alone to rows [i * R, min((i + 1) * R, H)); offsets[-1] is where the tail starts.
SegmentIndex = collections.namedtuple("SegmentIndex", "rows_per_segment offsets")
SEGMENT_CHUNK = b"ttSG"                 # ancillary, private, unsafe to copy: an editor that rewrites IDAT drops it
SEGMENT_VERSION = 1
SEGMENT_MARKER = b"\x00\x00\xff\xff"   # the empty stored block a flush leaves: every segment ends in it
SEGMENT_MODES = ("auto", "ignore", "require")
PngImage = _lib.structs()["tt_png_image"]
PngChunk = _lib.structs()["tt_png_chunk"]
PngSegment = _lib.structs()["tt_png_segment"]
ChecksumRange = _lib.structs()["tt_checksum_range"]
STATUS_NAMES = {v: k for k, v in _lib.constants().items() if k.startswith("TT_PNG_") and not k.startswith("TT_PNG_MAX")}
STATUS_NAMES.update({_lib.TT_PNGV_BAD_ADLER32: "TT_PNGV_BAD_ADLER32", _lib.TT_PNGV_BAD_CRC32: "TT_PNGV_BAD_CRC32"})
VERIFY_FLAGS = {"adler32": _lib.TT_PNGV_ADLER32, "crc32": _lib.TT_PNGV_CRC32}


class PngDecodeError(_lib.TTError):
    """Some images of a call did not decode: `failed` is [(index, status name)], in call order."""

    def __init__(self, failed):
        self.failed = failed
        super().__init__("PNG decode failed for " + ", ".join(f"image {i}: {name}" for i, name in failed))


def parse_png(data, verify_crc=False):
    """file bytes -> PngInfo(width, height, channels, zlib_stream): the IDAT chunks' payload, concatenated.  Host only.
    ValueError, naming what was found, for anything but an 8-bit non-interlaced grey or RGB file with consecutive IDAT chunks
    and an IEND at its end.  verify_crc: check every chunk's CRC-32 (zlib.crc32); off by default, it is host time."""
    width, height, channels, parts = _walk(data, verify_crc)
    return PngInfo(width, height, channels, bytes(parts[0]) if len(parts) == 1 else b"".join(parts))


def _walk(data, verify_crc, idat_crcs=None, segs=None):
    """(width, height, channels, [the IDAT bodies as views of `data`]): nothing is copied.  idat_crcs: a list that receives
    the CRC field of every IDAT chunk, for the device to verify; every other chunk is then verified here (zlib.crc32).
    segs: a list that receives (body, "before" | "after" the IDAT run) of every `ttSG` chunk, for _index."""
    data = memoryview(data if isinstance(data, (bytes, bytearray, memoryview)) else bytes(data)).cast("B")
    if len(data) < 8 or bytes(data[:8]) != SIGNATURE:
        raise ValueError("not a PNG file: bad signature")
    pos, ihdr, idat, state = 8, None, [], "before"         # of the IDAT run: before, inside, after
    while True:
        if pos + 12 > len(data):
            raise ValueError(f"PNG: the file ends at byte {len(data)} inside a chunk header (no IEND)")
        n, kind = struct.unpack_from(">I4s", data, pos)
        if pos + 12 + n > len(data):
            raise ValueError(f"PNG: chunk {kind!r} at byte {pos} has length {n}, which runs past the file's {len(data)} bytes")
        body = data[pos + 8:pos + 8 + n]
        if verify_crc or (idat_crcs is not None and kind != b"IDAT"):
            want, = struct.unpack_from(">I", data, pos + 8 + n)
            if zlib.crc32(body, zlib.crc32(kind)) != want:
                raise ValueError(f"PNG: chunk {kind!r} at byte {pos} fails its CRC-32")
        pos += 12 + n
        if ihdr is None and kind != b"IHDR":
            raise ValueError(f"PNG: the first chunk is {kind!r}, not IHDR")
        if kind == b"IHDR":
            if ihdr is not None or n != 13:
                raise ValueError("PNG: a second or malformed IHDR")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            if state == "after":
                raise ValueError("PNG: IDAT chunks are not consecutive")
            state = "inside"
            idat.append(body)
            if idat_crcs is not None:
                idat_crcs.append(struct.unpack_from(">I", data, pos - 4)[0])
        elif kind == b"IEND":
            break
        else:
            if not kind[0] & 0x20:
                raise ValueError(f"PNG: critical chunk {kind!r} is not supported" + (" (a palette file)" if kind == b"PLTE" else ""))
            if state == "inside":
                state = "after"
            if kind == SEGMENT_CHUNK and segs is not None:
                segs.append((bytes(body), state))
    if pos != len(data):
        raise ValueError(f"PNG: {len(data) - pos} bytes after IEND")
    width, height, depth, colour, compression, filter_method, interlace = ihdr
    if depth != 8:
        raise ValueError(f"PNG: bit depth {depth}, only 8 is supported")
    if colour not in (0, 2):
        what = {3: "palette", 4: "grey + alpha", 6: "RGBA"}.get(colour, "unknown")
        raise ValueError(f"PNG: colour type {colour} ({what}), only 0 (grey) and 2 (RGB) are supported")
    if compression != 0 or filter_method != 0:
        raise ValueError(f"PNG: compression method {compression}, filter method {filter_method}: only 0 / 0 exist")
    if interlace != 0:
        raise ValueError(f"PNG: interlace method {interlace} (Adam7), only non-interlaced files are supported")
    if width < 1 or height < 1:
        raise ValueError(f"PNG: {width} x {height} pixels")
    if not idat:
        raise ValueError("PNG: no IDAT chunk")
    return width, height, 1 if colour == 0 else 3, idat


def _parts(info):
    """The pieces of an image's zlib stream: PngDecoder parses into views of the file bytes (a PngInfo whose zlib_stream is
    the tuple of IDAT bodies) and writes them straight into the staging buffer; a PngInfo from parse_png holds one piece."""
    z = info.zlib_stream
    return z if isinstance(z, tuple) else (z,)


def _up(n, a):
    return (n + a - 1) // a * a


# ------------------------------------------------------------------------------------------------------- segmented files
def _payload_bytes(parts, starts, a, b):
    """Bytes [a, b) of the concatenated IDAT payload, whose pieces `parts` begin at `starts`."""
    out, i = [], max(bisect.bisect_right(starts, a) - 1, 0)
    while a < b and i < len(parts):
        lo = a - starts[i]
        piece = parts[i][lo:lo + (b - a)]
        out.append(bytes(piece))
        a += len(piece)
        i += 1
    return b"".join(out)


def _index(height, parts, segs):
    """The SegmentIndex of a file from what _walk collected (`segs`: its ttSG chunks), or None if it has none.  ValueError,
    naming the property, for a chunk that does not describe the file's stream (read_segments lists them)."""
    if not segs:
        return None
    if len(segs) > 1:
        raise ValueError(f"PNG: {len(segs)} ttSG chunks, at most one")
    body, where = segs[0]
    if where != "before":
        raise ValueError("PNG: the ttSG chunk comes after the IDAT chunks, it must stand before the first")
    if len(body) < 9:
        raise ValueError(f"ttSG: a body of {len(body)} bytes is shorter than its fixed fields")
    version, rows, n = struct.unpack_from(">BII", body)
    if version != SEGMENT_VERSION:
        raise ValueError(f"ttSG: unknown version {version}, this reader knows {SEGMENT_VERSION}")
    if rows < 1:
        raise ValueError("ttSG: rows_per_segment is 0")
    if n != -(-height // rows):
        raise ValueError(f"ttSG: num_segments {n}, but {height} rows in segments of {rows} are {-(-height // rows)}")
    if len(body) != 9 + 4 * (n + 1):
        raise ValueError(f"ttSG: a body of {len(body)} bytes, {n} segments need {9 + 4 * (n + 1)}")
    offsets = struct.unpack_from(f">{n + 1}I", body, 9)
    starts, total = [], 0
    for part in parts:
        starts.append(total)
        total += len(part)
    if offsets[0] != 2:
        raise ValueError(f"ttSG: offsets[0] is {offsets[0]}, the first segment starts after the two zlib header bytes")
    for i in range(n):
        if offsets[i + 1] <= offsets[i]:
            raise ValueError(f"ttSG: offsets are not increasing at segment {i}: {offsets[i]}, {offsets[i + 1]}")
    if offsets[n] > total:
        raise ValueError(f"ttSG: offset {offsets[n]} is past the IDAT payload's {total} bytes")
    for i in range(n):
        if offsets[i + 1] - offsets[i] < 5:
            raise ValueError(f"ttSG: segment {i} has {offsets[i + 1] - offsets[i]} bytes, shorter than the 5 of an empty one")
        if _payload_bytes(parts, starts, offsets[i + 1] - 4, offsets[i + 1]) != SEGMENT_MARKER:
            raise ValueError(f"ttSG: segment {i} does not end in the empty stored block 00 00 FF FF at byte {offsets[i + 1]}")
    tail = _payload_bytes(parts, starts, offsets[n], min(total, offsets[n] + 10))
    if not ((len(tail) == 6 and tail[:2] == b"\x03\x00") or (len(tail) == 9 and tail[:5] == b"\x01" + SEGMENT_MARKER)):
        raise ValueError(f"ttSG: the tail at byte {offsets[n]} is not one empty final block and the four Adler-32 bytes")
    return SegmentIndex(rows, tuple(offsets))


def read_segments(data, verify_crc=False):
    """file bytes -> the file's SegmentIndex (its `ttSG` chunk, checked against the file), or None if it has no such chunk.
    ValueError, naming the property, for: an unknown version or R = 0; num_segments != ceil(H / R); a body of another length;
    offsets[0] != 2 or offsets that do not increase; a segment shorter than 5 bytes or one that does not end in 00 00 FF FF;
    a tail that is not an empty final block plus four bytes; an offset past the payload; a second ttSG, or one after IDAT.
    What is NOT checked is that every segment inflates to its rows: a stale index (the stream rewritten, the chunk kept)
    that passes these checks is an image status on the device, never a wrong image."""
    segs = []
    _, height, _, parts = _walk(data, verify_crc, None, segs)
    return _index(height, parts, segs)


def _chunks(data):
    """[(kind, body)] of a file _walk has accepted."""
    data, pos, out = memoryview(data).cast("B"), 8, []
    while pos < len(data):
        n, kind = struct.unpack_from(">I4s", data, pos)
        out.append((kind, bytes(data[pos + 8:pos + 8 + n])))
        pos += 12 + n
    return out


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(kind)))


def segment_png(data, rows_per_segment=16, level=6, idat_bytes=65536):
    """file bytes -> the bytes of the same image as a SEGMENTED file: its zlib stream written again with a full flush
    (Z_FULL_FLUSH) after every `rows_per_segment` rows, and a `ttSG` chunk before the first IDAT that records where every
    segment starts.  The filtered scanlines are kept byte for byte (nothing is filtered again), every other chunk stays where
    it was, an older ttSG is dropped; the result is a valid PNG file for any reader, some per cent larger.  Segmenting the
    result again with the same parameters returns it unchanged.  Host only, once per dataset: PngDecoder then gives every
    segment a wave of its own."""
    rows_per_segment, idat_bytes = int(rows_per_segment), int(idat_bytes)
    if rows_per_segment < 1 or idat_bytes < 1:
        raise ValueError(f"rows_per_segment {rows_per_segment} and idat_bytes {idat_bytes} must be at least 1")
    data = bytes(data)
    width, height, channels, parts = _walk(data, False)
    stride = 1 + width * channels
    lines = zlib.decompress(b"".join(parts))
    if len(lines) != height * stride:
        raise ValueError(f"PNG: the stream holds {len(lines)} scanline bytes, {height} x (1 + {width} x {channels}) are {height * stride}")
    co = zlib.compressobj(level, zlib.DEFLATED, 15)
    pieces, offsets, total = [], [], 0
    for row in range(0, height, rows_per_segment):
        piece = co.compress(lines[row * stride:(row + rows_per_segment) * stride]) + co.flush(zlib.Z_FULL_FLUSH)
        offsets.append(total + (2 if row == 0 else 0))
        pieces.append(piece)
        total += len(piece)
    offsets.append(total)
    pieces.append(co.flush(zlib.Z_FINISH))
    stream = b"".join(pieces)
    index = struct.pack(f">BII{len(offsets)}I", SEGMENT_VERSION, rows_per_segment, len(offsets) - 1, *offsets)
    out, written = [SIGNATURE], False
    for kind, body in _chunks(data):
        if kind == SEGMENT_CHUNK:
            continue
        if kind == b"IDAT":
            if not written:
                out.append(_chunk(SEGMENT_CHUNK, index))
                out.extend(_chunk(b"IDAT", stream[i:i + idat_bytes]) for i in range(0, len(stream), idat_bytes))
                written = True
            continue
        out.append(_chunk(kind, body))
    out = b"".join(out)
    if read_segments(out) != SegmentIndex(rows_per_segment, tuple(offsets)):        # (what the decoder will go by)
        raise AssertionError("segment_png: the index written does not read back")
    return out


def parse_files(files, segments="auto", verify_crc=False, idat_crcs=False):
    """[file bytes] -> [PngInfo] as PngDecoder packs them: the stream as views of the file's IDAT bodies, with idat_crcs the
    chunks' CRC fields, and the SegmentIndex under the `segments` mode of PngDecoder ("auto", "ignore", "require").  Host only."""
    if segments not in SEGMENT_MODES:
        raise ValueError(f"segments: {segments!r} not in {SEGMENT_MODES}")
    out = []
    for i, f in enumerate(files):
        crcs = [] if idat_crcs else None
        segs = None if segments == "ignore" else []
        width, height, channels, parts = _walk(f, verify_crc, crcs, segs)
        index = _index(height, parts, segs)
        if index is None and segments == "require":
            raise ValueError(f'file {i} has no segment index (ttSG chunk) and segments="require": write it with segment_png')
        out.append(PngInfo(width, height, channels, tuple(parts), None if crcs is None else tuple(crcs), index))
    return out


class PngDecoder:
    """Decodes batches of PNG files on `device`.  Holds and reuses the pinned staging buffer, the device copy of it, the
    workspace and the status array: they grow when a batch needs more and never shrink.  One call = one pinned host-to-device
    copy (the image table, the chunk table if CRC-32s are verified, the segment table if a file has an index, and every
    stream), two launches (five with `verify`, two more with segmented files), and -- with check=True -- one small copy of
    the statuses back.
    The streams are copied once on the host, from the file bytes into the staging buffer.  The buffers are reused from call
    to call without synchronising, so all calls of one decoder must be on ONE stream (the current stream at each call); use a
    decoder per stream otherwise."""

    def __init__(self, device="cuda", verify_crc=False, verify=(), segments="auto"):
        """verify: a subset of {"adler32", "crc32"} to verify on the device (True: both; see the module text); the default
        verifies nothing.  verify_crc=True is the all-host CRC-32 check and excludes "crc32".
        segments: "auto" decodes a file that carries a segment index (segment_png) with one wave per segment and every
        other file as before, mixed freely in one call; "ignore" decodes every file the old way; "require" makes a file
        without an index a ValueError.  An index that does not describe its file is a ValueError under "auto" and "require"."""
        import torch
        if segments not in SEGMENT_MODES:
            raise ValueError(f"segments: {segments!r} not in {SEGMENT_MODES}")
        self.segments = segments
        verify = ("adler32", "crc32") if verify is True else (() if verify in (False, None) else
                                                              ((verify,) if isinstance(verify, str) else tuple(verify)))
        unknown = [v for v in verify if v not in VERIFY_FLAGS]
        if unknown:
            raise ValueError(f"verify: {unknown} not in {sorted(VERIFY_FLAGS)}")
        if verify_crc and "crc32" in verify:
            raise ValueError('verify_crc=True checks every CRC-32 on the host, verify="crc32" on the device: choose one')
        self.verify = tuple(sorted(set(verify)))
        self.verify_flags = sum(VERIFY_FLAGS[v] for v in self.verify)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("PngDecoder needs a GPU device: there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.verify_crc = verify_crc
        self._stage = self._packed = self._work = self._status = self._copied = self._chunks = self._segs = None

    def _grow(self, name, n, **kw):
        import torch
        t = getattr(self, name)
        if t is None or t.numel() < n:
            t = torch.empty(_up(max(n, 1), 1 << 16), **kw)
            setattr(self, name, t)
        return t

    def _pack(self, infos, dst_offsets):
        """The call's one host buffer, in the pinned staging tensor: the image table, with verify="crc32" the chunk table
        (self._chunks: the table and its offset, else None), the segment table if an image has a SegmentIndex (self._segs,
        alike), then every stream at a 16-byte aligned offset -> (table, its bytes)."""
        import torch
        n = len(infos)
        if not 1 <= n <= _lib.TT_PNG_MAX_IMAGES:
            raise ValueError(f"{n} images in one call, 1..{_lib.TT_PNG_MAX_IMAGES}")
        table = (PngImage * n)()
        pos = _up(ctypes.sizeof(table), 256)
        self._chunks = None
        if self.verify_flags & VERIFY_FLAGS["crc32"]:
            if any(info.idat_crcs is None or len(info.idat_crcs) != len(_parts(info)) for info in infos):
                raise ValueError('verify="crc32" needs every IDAT chunk\'s CRC field: decode files, not bare streams')
            chunks = (PngChunk * sum(len(info.idat_crcs) for info in infos))()
            if len(chunks) > _lib.TT_PNG_MAX_CHUNKS:
                raise ValueError(f"{len(chunks)} IDAT chunks in one call, at most {_lib.TT_PNG_MAX_CHUNKS}")
            self._chunks = (chunks, pos)
            pos = _up(pos + ctypes.sizeof(chunks), 256)
        self._segs = None
        num_segs = sum(len(info.segments.offsets) - 1 for info in infos if info.segments is not None)
        if num_segs:
            if num_segs > _lib.TT_PNG_MAX_SEGMENTS:
                raise ValueError(f"{num_segs} segments in one call, at most {_lib.TT_PNG_MAX_SEGMENTS}")
            self._segs = ((PngSegment * num_segs)(), pos)
            pos = _up(pos + ctypes.sizeof(self._segs[0]), 256)
        for i, (info, dst) in enumerate(zip(infos, dst_offsets)):
            im = table[i]
            nbytes = sum(len(part) for part in _parts(info))
            im.stream_offset, im.stream_bytes, im.dst_offset = pos, nbytes, dst
            im.width, im.height, im.channels = info.width, info.height, info.channels
            pos = _up(pos + nbytes, 16)
        if self._chunks:
            j = 0
            for i, (im, info) in enumerate(zip(table, infos)):
                at = im.stream_offset
                for part, crc in zip(_parts(info), info.idat_crcs):
                    ch = self._chunks[0][j]
                    ch.offset, ch.bytes, ch.crc, ch.image = at, len(part), crc, i
                    at += len(part)
                    j += 1
        if self._segs:
            j = 0
            for i, (im, info) in enumerate(zip(table, infos)):
                if info.segments is None:
                    continue
                rows, offsets = info.segments
                for k in range(len(offsets) - 1):
                    sg = self._segs[0][j]
                    sg.offset, sg.bytes = im.stream_offset + offsets[k], offsets[k + 1] - offsets[k]
                    sg.image, sg.first_row, sg.rows = i, k * rows, min(rows, info.height - k * rows)
                    j += 1
        if self._copied is not None:
            self._copied.synchronize()                      # the previous call's copy has left the staging buffer
        host = self._grow("_stage", pos, dtype=torch.uint8, pin_memory=True).numpy()
        host[:ctypes.sizeof(table)] = np.frombuffer(table, dtype=np.uint8)
        for extra in (self._chunks, self._segs):
            if extra:
                host[extra[1]:extra[1] + ctypes.sizeof(extra[0])] = np.frombuffer(extra[0], dtype=np.uint8)
        for im, info in zip(table, infos):                   # the one copy of the streams on the host
            at = im.stream_offset
            for part in _parts(info):
                host[at:at + len(part)] = np.frombuffer(part, dtype=np.uint8)
                at += len(part)
        return table, pos

    def _run(self, infos, dst_offsets, out_base, out_bytes, check_status):
        """infos: [PngInfo]; image i goes to byte dst_offsets[i] of the uint8 device tensor out_base (out_bytes long)."""
        import torch
        n = len(infos)
        table, total = self._pack(infos, dst_offsets)
        stage = self._stage
        packed = self._grow("_packed", total, dtype=torch.uint8, device=self.device)
        if int(lib().tt_png_workspace_bytes(table, n)) <= 0:        # the sizes tt_png_decode_u8 refuses
            raise ValueError(f"an image is wider than {_lib.TT_PNG_MAX_WIDTH} pixels or has more than 2^31 - 1 scanline bytes")
        chunks, chunks_at = self._chunks or (None, 0)
        segs, segs_at = self._segs or (None, 0)
        if segs:
            need = int(lib().tt_png_segmented_workspace_bytes(table, n, chunks, len(chunks) if chunks else 0, self.verify_flags,
                                                              segs, len(segs)))
        else:
            need = int(lib().tt_png_verify_workspace_bytes(table, n, chunks, len(chunks) if chunks else 0, self.verify_flags))
        if need <= 0:
            raise _lib.TTError(("tt_png_segmented_workspace_bytes: " if segs else "tt_png_verify_workspace_bytes: ")
                               + lib().tt_last_error().decode())
        work = self._grow("_work", need, dtype=torch.uint8, device=self.device)
        status = self._grow("_status", 4 * n, dtype=torch.uint8, device=self.device)[:4 * n].view(torch.int32)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            packed[:total].copy_(stage[:total], non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record(stream)
            if segs:
                check(lib().tt_png_decode_u8_segmented(ptr(packed), total, table, ptr(packed), n, chunks,
                                                       ptr(packed) + chunks_at if chunks else None, len(chunks) if chunks else 0,
                                                       self.verify_flags, segs, ptr(packed) + segs_at, len(segs), ptr(work),
                                                       work.numel(), ptr(out_base), out_bytes, ptr(status), stream.cuda_stream),
                      "tt_png_decode_u8_segmented")
            elif self.verify_flags:
                check(lib().tt_png_decode_u8_verified(ptr(packed), total, table, ptr(packed), n, chunks,
                                                      ptr(packed) + chunks_at if chunks else None, len(chunks) if chunks else 0,
                                                      self.verify_flags, ptr(work), work.numel(), ptr(out_base), out_bytes,
                                                      ptr(status), stream.cuda_stream), "tt_png_decode_u8_verified")
            else:
                check(lib().tt_png_decode_u8(ptr(packed), total, table, ptr(packed), n, ptr(work), work.numel(), ptr(out_base),
                                             out_bytes, ptr(status), stream.cuda_stream), "tt_png_decode_u8")
        self.last_packed_bytes = total
        if not check_status:
            return status.clone()
        failed = [(i, STATUS_NAMES.get(s, str(s))) for i, s in enumerate(status.cpu().tolist()) if s != 0]
        if failed:
            raise PngDecodeError(failed)
        return None

    def _parse(self, files):
        return parse_files(files, self.segments, self.verify_crc, bool(self.verify_flags & VERIFY_FLAGS["crc32"]))

    def decode(self, files, out=None, check=True):
        """A list of file bytes of equal (H, W, C) -> uint8 [n, H, W, 3] on the device ([n, H, W] for grey files), freshly
        allocated or `out` (contiguous, that shape).  check=True reads the statuses back and raises PngDecodeError if any
        image failed; check=False stays asynchronous and returns (images, int32 status tensor [n])."""
        import torch
        infos = self._parse(files)
        if not infos:
            raise ValueError("no files")
        w, h, c = infos[0][:3]
        for i, info in enumerate(infos):
            if tuple(info[:3]) != (w, h, c):
                raise ValueError(f"file {i} is {info.height} x {info.width} x {info.channels}, file 0 is {h} x {w} x {c}")
        shape = (len(infos), h, w, 3) if c == 3 else (len(infos), h, w)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != self.device
              or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape} on {self.device}")
        status = self._run(infos, [i * h * w * c for i in range(len(infos))], out, out.numel(), check)
        return out if check else (out, status)

    def decode_sample_batch(self, rgb_files, depth_files, seg_files, check=True):
        """The nested lists [B][T][N] (camera frames), [B][N] (depth maps) and [B][N] (segmentation maps) of file bytes ->
        (raw uint8 [B, T, N, H, W, 3], depth_png uint8 [B, N, H, W, 3], seg_png uint8 [B, N, H, W]) from ONE tt_png_decode_u8
        call: what labels.RawLabelDecoder and preprocess.TrainImagePipeline take.  Camera order within N is the caller's."""
        import torch
        B = len(rgb_files)
        T = len(rgb_files[0]) if B else 0
        N = len(rgb_files[0][0]) if T else 0
        if not (B and T and N):
            raise ValueError("rgb_files must be a non-empty [B][T][N] nest of file bytes")
        if any(len(s) != T or any(len(t) != N for t in s) for s in rgb_files):
            raise ValueError(f"rgb_files is ragged: every sample needs {T} sweeps of {N} cameras")
        for what, nest in (("depth_files", depth_files), ("seg_files", seg_files)):
            if len(nest) != B or any(len(s) != N for s in nest):
                raise ValueError(f"{what} must be a [{B}][{N}] nest of file bytes")
        rgb = self._parse([f for s in rgb_files for t in s for f in t])
        dep = self._parse([f for s in depth_files for f in s])
        seg = self._parse([f for s in seg_files for f in s])
        w, h = rgb[0].width, rgb[0].height
        for what, infos, c in (("rgb", rgb, 3), ("depth", dep, 3), ("seg", seg, 1)):
            for i, info in enumerate(infos):
                if (info.width, info.height, info.channels) != (w, h, c):
                    raise ValueError(f"{what} file {i} is {info.height} x {info.width} x {info.channels}, expected {h} x {w} x {c}")
        n_raw, n_dep, n_seg = len(rgb) * h * w * 3, len(dep) * h * w * 3, len(seg) * h * w
        o_dep = _up(n_raw, 256)
        o_seg = o_dep + _up(n_dep, 256)
        buf = torch.empty(o_seg + n_seg, dtype=torch.uint8, device=self.device)        # the three tensors are views of it
        offsets = ([i * h * w * 3 for i in range(len(rgb))] + [o_dep + i * h * w * 3 for i in range(len(dep))]
                   + [o_seg + i * h * w for i in range(len(seg))])
        status = self._run(rgb + dep + seg, offsets, buf, buf.numel(), check)
        out = (buf[:n_raw].view(B, T, N, h, w, 3), buf[o_dep:o_dep + n_dep].view(B, N, h, w, 3),
               buf[o_seg:o_seg + n_seg].view(B, N, h, w))
        return out if check else out + (status,)


def _device_checksum(kind, data, ranges, start):
    import torch
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or not data.is_cuda or not data.is_contiguous() or data.dim() != 1:
        raise ValueError("data must be a contiguous one-dimensional uint8 device tensor")
    ranges = [(0, data.numel())] if ranges is None else [(int(o), int(n)) for o, n in ranges]
    n = len(ranges)
    if not 1 <= n <= _lib.TT_CHECKSUM_MAX_RANGES:
        raise ValueError(f"{n} ranges in one call, 1..{_lib.TT_CHECKSUM_MAX_RANGES}")
    table = (ChecksumRange * n)()
    for entry, (offset, nbytes) in zip(table, ranges):
        entry.offset, entry.bytes = offset, nbytes
    if start is not None:
        start = torch.as_tensor(np.asarray(start, dtype=np.uint32).reshape(n).view(np.int32)).to(data.device)
    need = int(lib().tt_checksum_workspace_bytes(table, n))
    if need <= 0:
        raise ValueError("a range has a negative length, or the ranges make more than 2^31 - 1 tiles")
    table_dev = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(data.device)
    work = torch.empty(need, dtype=torch.uint8, device=data.device)
    out = torch.empty(n, dtype=torch.int32, device=data.device)
    with torch.cuda.device(data.device):
        check(lib().tt_checksum_ranges_u8(ptr(data), data.numel(), table, ptr(table_dev), n, kind, ptr(start), ptr(out), ptr(work),
                                          need, torch.cuda.current_stream(data.device).cuda_stream), "tt_checksum_ranges_u8")
    return out.view(torch.uint32)


def device_adler32(data, ranges=None, start=None):
    """zlib.adler32(data[o:o + n], start) for every (o, n) of `ranges` (None: the whole tensor), on the device
    (tt_checksum_ranges_u8).  data: a contiguous 1-D uint8 device tensor; ranges may have any length, alignment and order;
    start: None (1) or one uint32 per range.  Returns a uint32 device tensor [len(ranges)]; asynchronous."""
    return _device_checksum(_lib.TT_CHECKSUM_ADLER32, data, ranges, start)


def device_crc32(data, ranges=None, start=None):
    """zlib.crc32(data[o:o + n], start) for every (o, n) of `ranges`: as device_adler32, start None meaning 0."""
    return _device_checksum(_lib.TT_CHECKSUM_CRC32, data, ranges, start)
