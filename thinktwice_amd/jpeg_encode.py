"""JPEG files written on the device, and a Motion JPEG writer that turns them into a video of a drive.

    enc = jpeg_encode.JpegEncoder()                       # quality=90, subsampling="420", restart_rows=1
    files = enc.encode([frame_u8, grey_u8])               # uint8 device tensors (H, W, 3), (H, W, 1) or (H, W) -> [bytes]

Every file is a complete baseline JPEG (JFIF) for any reader.  Colour conversion, chroma mean, DCT, quantisation, Huffman coding
with the standard tables and the file's layout run on the device (tt_jpeg_encode_u8 in include/thinktwice_hip.h;
csrc/jpeg_encode.hip, csrc/jpeg_core.h); the host copies the finished bytes.  The buffer handling is png_encode's
DeviceFileEncoder, shared with PngEncoder.  There is no decoder: the dataset is PNG.

    video = jpeg_encode.MjpegWriter("drive.avi", 1600, 900, fps=2.0)      # host only
    video.add(files[0]); ...; video.close()

`png_encode.FrameRecorder.submit(images, files, video)` routes names ending in .jpg / .jpeg and video frames here."""
import ctypes
import os
import struct

from . import _lib
from .ops import lib, ptr
from .png_encode import DeviceFileEncoder

EncImage = _lib.structs()["tt_jpeg_enc_image"]
SUBSAMPLING = {"444": _lib.TT_JPEG_444, "420": _lib.TT_JPEG_420}
HEADER_BYTES_GREY = 330                                    # everything before the scan; 613 with three components


class JpegEncoder(DeviceFileEncoder):
    """Encodes batches of uint8 device images to JPEG files on `device`: one call = one tt_jpeg_encode_u8 and one
    device-to-host copy; buffers, stream and pinned pool as DeviceFileEncoder states them.  quality 1..100 scales the Annex K
    quantisation tables as PIL does; subsampling "444" or "420" (grey images ignore it); a restart interval is `restart_rows`
    MCU rows (8 pixel rows, 16 at 4:2:0) and is coded by one workgroup."""

    Image, ENTRY, MIN_FILE = EncImage, "tt_jpeg_encode_u8", HEADER_BYTES_GREY + 2

    def __init__(self, device="cuda", quality=90, subsampling="420", restart_rows=1):
        if str(subsampling) not in SUBSAMPLING:
            raise ValueError(f"subsampling: {subsampling!r} not in {sorted(SUBSAMPLING)}")
        if not 1 <= int(quality) <= 100:
            raise ValueError(f"quality {quality} must be in 1..100")
        if int(restart_rows) < 1:
            raise ValueError(f"restart_rows {restart_rows} must be at least 1")
        self.quality, self.subsampling, self.restart_rows = int(quality), str(subsampling), int(restart_rows)
        super().__init__(device)

    def _describe(self, im):
        im.quality, im.subsampling, im.restart_rows = self.quality, SUBSAMPLING[self.subsampling], self.restart_rows

    def _refusal(self):
        return f"is larger than 65535, or {self.restart_rows} MCU rows per restart interval make a DRI value above 65535"

    def _bound(self, im):
        return lib().tt_jpeg_encode_bound(ctypes.byref(im), 1)

    def _workspace(self, table, n):
        return lib().tt_jpeg_encode_workspace_bytes(table, n)

    def _launch(self, pixels, pixel_bytes, table, table_dev, n, work, files, files_bytes, stream):
        return lib().tt_jpeg_encode_u8(ptr(pixels), pixel_bytes, table, ptr(table_dev), n, ptr(work), work.numel(), ptr(files),
                                       files_bytes, ptr(files), stream.cuda_stream)


def frame_size(jpeg):
    """(width, height) of a baseline JPEG file, from its SOF0 segment."""
    if jpeg[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file: no SOI")
    at = 2
    while at + 4 <= len(jpeg):
        if jpeg[at] != 0xFF:
            raise ValueError(f"not a JPEG file: no marker at byte {at}")
        marker, n = jpeg[at + 1], int.from_bytes(jpeg[at + 2:at + 4], "big")
        if marker == 0xC0:
            if at + 9 > len(jpeg):
                break
            return int.from_bytes(jpeg[at + 7:at + 9], "big"), int.from_bytes(jpeg[at + 5:at + 7], "big")
        if marker == 0xDA:
            break
        at += 2 + n
    raise ValueError("no SOF0 segment before the scan: not a baseline JPEG file")


class MjpegWriter:
    """A RIFF AVI file with one Motion JPEG video stream, written by the host.  `add(jpeg_bytes)` appends a frame (a complete
    baseline JPEG file whose SOF0 size is (width, height), anything else is refused), `close()` finishes the file.

    Layout: RIFF 'AVI ' { LIST 'hdrl' { 'avih', LIST 'strl' { 'strh' (vids / MJPG), 'strf' (BITMAPINFOHEADER, MJPG, 24 bits) } },
    LIST 'movi' { '00dc' chunks, padded to even length }, 'idx1' (every entry a key frame, offsets relative to the 'movi'
    fourcc) }.  The RIFF, movi and idx1 sizes, the frame counts and dwSuggestedBufferSize are patched in place at close() and
    after every `index_every` frames: then the index is written behind the last frame and the file flushed, and the next frame
    overwrites that index.  A writer that is abandoned right there leaves a file that ends in a valid index; one abandoned
    further on leaves frames beyond what the header counts until the next index.
    RIFF sizes are 32 bits and OpenDML is not written: before the file would pass `max_bytes` (1 GiB) it is closed and
    name_0001.avi, name_0002.avi, ... are begun.  `paths` lists the files written."""

    HEADER = 224                                            # bytes before the first chunk of 'movi'
    MOVI = 220                                              # of the 'movi' fourcc

    def __init__(self, path, width, height, fps, index_every=100, max_bytes=1 << 30):
        width, height, index_every, max_bytes = int(width), int(height), int(index_every), int(max_bytes)
        if not (1 <= width <= 65535 and 1 <= height <= 65535):
            raise ValueError(f"a frame of {width} x {height}: 1..65535")
        if not float(fps) > 0:
            raise ValueError(f"fps {fps} must be positive")
        if index_every < 1:
            raise ValueError(f"index_every {index_every} must be at least 1")
        if not self.HEADER + 24 <= max_bytes <= 0xFFFFFFF0:
            raise ValueError(f"max_bytes {max_bytes}: a RIFF size has 32 bits")
        self.path, self.width, self.height, self.fps = os.fspath(path), width, height, float(fps)
        self.index_every, self.max_bytes = index_every, max_bytes
        self.rate, self.scale = max(1, round(self.fps * 1000)), 1000
        self.frames = 0                                     # of all files
        self.paths = []
        self._file = None
        self._closed = False
        self._open()

    def _open(self):
        k = len(self.paths)
        stem, ext = os.path.splitext(self.path)
        path = self.path if k == 0 else f"{stem}_{k:04d}{ext}"
        self.paths.append(path)
        self._file = open(path, "wb")
        self._index = []                                    # (offset from the 'movi' fourcc, bytes) per frame of this file
        self._end = self.HEADER                             # where the next chunk goes
        self._largest = 0
        self._file.write(self._header())

    def _header(self):
        n, movi = len(self._index), self._end - self.MOVI
        total = self._end + 8 + 16 * n
        avih = struct.pack("<14I", round(1e6 * self.scale / self.rate), 0, 0, 0x10, n, 0, 1, self._largest, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._largest, 0xFFFFFFFF, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        out = (b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
               + b"LIST" + struct.pack("<I", movi) + b"movi")
        assert len(out) == self.HEADER
        return out

    def _write_index(self):
        """The index behind the last frame, the header's sizes and counts; the file position returns to the last frame's end."""
        f = self._file
        f.seek(self._end)
        f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
        f.write(b"".join(b"00dc" + struct.pack("<III", 0x10, at, size) for at, size in self._index))
        f.truncate()
        f.seek(0)
        f.write(self._header())
        f.flush()
        f.seek(self._end)

    def add(self, jpeg):
        if self._closed:
            raise RuntimeError("MjpegWriter.add after close()")
        jpeg = bytes(jpeg)
        size = frame_size(jpeg)
        if size != (self.width, self.height):
            raise ValueError(f"a frame of {size[0]} x {size[1]} in a video of {self.width} x {self.height}")
        padded = len(jpeg) + (len(jpeg) & 1)
        if self._index and self._end + 8 + padded + 8 + 16 * (len(self._index) + 1) > self.max_bytes:
            self._write_index()
            self._file.close()
            self._open()
        self._file.seek(self._end)
        self._file.write(b"00dc" + struct.pack("<I", len(jpeg)) + jpeg + b"\x00" * (padded - len(jpeg)))
        self._index.append((self._end - self.MOVI, len(jpeg)))
        self._end += 8 + padded
        self._largest = max(self._largest, padded)
        self.frames += 1
        if len(self._index) % self.index_every == 0:
            self._write_index()

    def close(self):
        if not self._closed:
            self._closed = True
            self._write_index()
            self._file.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
