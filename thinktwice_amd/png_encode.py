"""PNG files written on the device, and a recorder that keeps what a closed-loop agent saw.

    enc = png_encode.PngEncoder()                         # rows_per_segment=16, filter="adaptive"
    files = enc.encode([frame_u8, depth_u8, tags_u8])     # uint8 device tensors (H, W, 3), (H, W, 1) or (H, W) -> [bytes]

Every file is a complete 8-bit grey or RGB PNG for any reader, and born SEGMENTED: its zlib stream restarts after every
`rows_per_segment` rows and the `ttSG` chunk of png.py records where, so `png.PngDecoder(segments="auto")` gives every segment
a wave of its own without a pass of `png.segment_png`.  Filter pass, deflate, container and checksums run on the device
(tt_png_encode_u8 in include/thinktwice_hip.h; csrc/png_encode.hip, csrc/png_deflate.h); the host copies the finished bytes.

    rec = png_encode.FrameRecorder(root)                  # a writer thread; at most max_pending submissions in flight
    rec.submit({"rgb_front/0003.png": frame_u8}, {"meta/0003.json": b"{...}"})
    rec.close()

`AgentTick(..., recorder=rec)` records every `record_every`-th tick that way (agent_tick.py).  A name ending in .jpg / .jpeg and
the frames of `submit(..., video={"debug.avi": canvas_u8})` go to jpeg_encode.py's JpegEncoder and MjpegWriter; the buffer
handling of both encoders is DeviceFileEncoder below."""
import ctypes
import os
import queue
import threading

import numpy as np

from . import _lib
from .ops import check, lib, ptr
from .png_segment import DEFAULT_ROWS

EncImage = _lib.structs()["tt_png_enc_image"]
FILTERS = {"none": _lib.TT_PNGE_FILTER_NONE, "sub": _lib.TT_PNGE_FILTER_SUB, "up": _lib.TT_PNGE_FILTER_UP, "avg": _lib.TT_PNGE_FILTER_AVG,
           "paeth": _lib.TT_PNGE_FILTER_PAETH, "adaptive": _lib.TT_PNGE_FILTER_ADAPTIVE}


def _up(n, a):
    return (n + a - 1) // a * a


class PendingFiles:
    """The files of one `encode_async` on their way to the host: `ready()` never blocks, `result()` waits for the copy if it
    has to and returns the list of `bytes`.  `minimum`: the smallest file the format has (57 bytes for PNG), `entry` the name
    an impossible size is reported under."""

    def __init__(self, host, event, slots, keep, pool, minimum=57, entry="tt_png_encode_u8"):
        self._host, self._event, self._slots, self._keep, self._pool = host, event, slots, keep, pool
        self._minimum, self._entry = minimum, entry
        self._result = None

    def ready(self):
        return self._result is not None or self._event.query()

    def result(self):
        if self._result is None:
            self._event.synchronize()
            host = self._host.numpy()
            n = len(self._slots)
            sizes = host[:8 * n].view(np.int64)
            out = []
            for (offset, capacity), size in zip(self._slots, sizes.tolist()):
                if not self._minimum <= size <= capacity:
                    raise _lib.TTError(f"{self._entry} reported a file of {size} bytes in a slot of {capacity}")
                out.append(host[offset:offset + size].tobytes())
            self._result = out
            self._pool.append(self._host)                   # the pinned buffer goes back to its encoder
            self._host = self._keep = None
        return self._result


class DeviceFileEncoder:
    """What PngEncoder and jpeg_encode.JpegEncoder share: batches of uint8 device images -> files on `device`.  Holds and
    reuses the pixel staging tensor, the workspace and the slot buffer: they grow when a batch needs more and never shrink.
    One call = one entry call and one device-to-host copy (the file sizes and the slots, up to the end of the last slot: how
    much of a slot is used is known on the device only, and nothing here waits for it).  The buffers are reused without
    synchronising, so all calls of one encoder must be on ONE stream (the current stream at each call).  The pinned host
    buffers of finished calls are reused.  A format states its table entry (`_describe`), its three C entries (`_bound`,
    `_workspace`, `_launch`) and ENTRY / MIN_FILE."""

    Image = ENTRY = MIN_FILE = None

    def __init__(self, device="cuda"):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} needs a GPU device: there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._pixels = self._work = self._files = self._table = None
        self._pool = []                                      # pinned buffers whose PendingFiles has been read

    def _grow(self, name, n, **kw):
        import torch
        t = getattr(self, name)
        if t is None or t.numel() < n:
            t = torch.empty(_up(max(n, 1), 1 << 16), **kw)
            setattr(self, name, t)
        return t

    def _table_of(self, images):
        """-> (the image table, the tensors as contiguous [H, W, C] views, bytes of pixels, bytes of the slot buffer).  The slot
        buffer begins with the int64 file sizes; every slot is the format's bound of its image, rounded up to 16 bytes."""
        import torch
        n = len(images)
        if not 1 <= n <= _lib.TT_PNG_MAX_IMAGES:
            raise ValueError(f"{n} images in one call, 1..{_lib.TT_PNG_MAX_IMAGES}")
        table, views = (self.Image * n)(), []
        pixel_at, file_at = 0, _up(8 * n, 256)
        for i, (im, t) in enumerate(zip(table, images)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != self.device or t.dim() not in (2, 3)
                    or (t.dim() == 3 and t.shape[2] not in (1, 3)) or t.numel() == 0):
                raise ValueError(f"image {i}: a non-empty uint8 tensor (H, W, 3), (H, W, 1) or (H, W) on {self.device} is needed")
            views.append(t)
            im.height, im.width, im.channels = t.shape[0], t.shape[1], (t.shape[2] if t.dim() == 3 else 1)
            im.pixel_offset, im.file_offset = pixel_at, file_at
            self._describe(im)
            bound = int(self._bound(im))
            if bound <= 0:
                raise ValueError(f"image {i}: {im.height} x {im.width} x {im.channels} {self._refusal()}")
            im.file_capacity = _up(bound, 16)
            pixel_at = _up(pixel_at + t.numel(), 256)
            file_at += im.file_capacity
        return table, views, pixel_at, file_at

    def encode_async(self, images):
        """-> PendingFiles.  The device work and the copy to a pinned host buffer of this call are queued on the current
        stream; nothing waits."""
        import torch
        table, views, pixel_bytes, files_bytes = self._table_of(list(images))
        n = len(table)
        need = int(self._workspace(table, n))
        if need <= 0:
            raise _lib.TTError(f"{self.ENTRY}: the workspace size of the image table was refused")
        pixels = self._grow("_pixels", pixel_bytes, dtype=torch.uint8, device=self.device)
        work = self._grow("_work", need, dtype=torch.uint8, device=self.device)
        files = self._grow("_files", files_bytes, dtype=torch.uint8, device=self.device)
        raw = np.frombuffer(table, dtype=np.uint8)
        table_dev = self._grow("_table", len(raw), dtype=torch.uint8, device=self.device)
        host = None
        while self._pool and host is None:                   # (a buffer too small for this call is dropped: they only grow)
            t = self._pool.pop()
            host = t if t.numel() >= files_bytes else None
        if host is None:
            host = torch.empty(_up(files_bytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            table_dev[:len(raw)].copy_(torch.from_numpy(raw.copy()), non_blocking=False)
            for im, t in zip(table, views):
                pixels[im.pixel_offset:im.pixel_offset + t.numel()].view(t.shape).copy_(t)
            check(self._launch(pixels, pixel_bytes, table, table_dev, n, work, files, files_bytes, stream), self.ENTRY)
            host[:files_bytes].copy_(files[:files_bytes], non_blocking=True)
            event = torch.cuda.Event()
            event.record(stream)
        return PendingFiles(host, event, [(im.file_offset, im.file_capacity) for im in table], (table, views), self._pool,
                            self.MIN_FILE, self.ENTRY)

    def encode(self, images):
        """A list of uint8 device tensors, each (H, W, 3), (H, W, 1) or (H, W), of any mix of shapes -> a list of `bytes`, one
        file per image."""
        return self.encode_async(images).result()


class PngEncoder(DeviceFileEncoder):
    """Encodes batches of uint8 device images to PNG files on `device`: one call = one tt_png_encode_u8 and one device-to-host
    copy; buffers, stream and pinned pool as DeviceFileEncoder states them."""

    Image, ENTRY, MIN_FILE = EncImage, "tt_png_encode_u8", 57

    def __init__(self, device="cuda", rows_per_segment=DEFAULT_ROWS, filter="adaptive"):
        if filter not in FILTERS:
            raise ValueError(f"filter: {filter!r} not in {sorted(FILTERS)}")
        if int(rows_per_segment) < 1:
            raise ValueError(f"rows_per_segment {rows_per_segment} must be at least 1")
        self.rows_per_segment, self.filter = int(rows_per_segment), filter
        super().__init__(device)

    def _describe(self, im):
        im.rows_per_segment, im.filter = self.rows_per_segment, FILTERS[self.filter]

    def _refusal(self):
        return f"at {self.rows_per_segment} rows per segment makes a segment or a stream of more than 2^31 - 8 bytes"

    def _bound(self, im):
        return lib().tt_png_encode_bound(ctypes.byref(im), 1)

    def _workspace(self, table, n):
        return lib().tt_png_encode_workspace_bytes(table, n)

    def _launch(self, pixels, pixel_bytes, table, table_dev, n, work, files, files_bytes, stream):
        return lib().tt_png_encode_u8(ptr(pixels), pixel_bytes, table, ptr(table_dev), n, ptr(work), work.numel(), ptr(files),
                                      files_bytes, ptr(files), stream.cuda_stream)


def is_jpeg_name(rel):
    return os.fspath(rel).lower().endswith((".jpg", ".jpeg"))


class FrameRecorder:
    """Writes what `submit` is given under `root`, from a thread of its own.

    submit(images, files, video): `images` {relative path: uint8 device tensor} are encoded on the caller's stream -- a name
    that ends in .jpg / .jpeg (any case) by the recorder's JpegEncoder (jpeg_encode.py; `jpeg_encoder`, or a default one made
    at the first such name), every other name by its PngEncoder, each in ONE `encode_async`: a submission with PNG names only
    makes exactly one call, of the PNG encoder.  `files` {relative path: bytes} are written as they are.  `video` {relative
    .avi path: one uint8 (H, W, 3) device tensor} appends a frame to a Motion JPEG file: the frame is encoded in the same JPEG
    call as the submission's other JPEG images, and the writer thread appends it to that path's `jpeg_encode.MjpegWriter`,
    opened at the first frame with that frame's size and `video_fps`; the frames of a video stand in the order of `submit`.
    The writer thread waits for the encoders' copies, creates directories as needed, writes every ordinary file under a
    temporary name and renames it when it is complete.  With `max_pending` submissions outstanding, submit BLOCKS until one
    is written and counts that in `stalls`: a frame is never dropped.  An exception in the writer thread surfaces at the
    next submit or at close(); close() drains the queue first and finishes every video."""

    def __init__(self, root, encoder=None, max_pending=4, jpeg_encoder=None, video_fps=20.0):
        if int(max_pending) < 1:
            raise ValueError(f"max_pending {max_pending} must be at least 1")
        if not float(video_fps) > 0:
            raise ValueError(f"video_fps {video_fps} must be positive")
        self.root, self.encoder = os.fspath(root), encoder if encoder is not None else PngEncoder()
        self.jpeg_encoder, self.video_fps = jpeg_encoder, float(video_fps)
        self.stalls = self.submitted = self.written = 0
        self._videos = {}                                    # relative path -> MjpegWriter (the writer thread's)
        self._slots = threading.Semaphore(int(max_pending))
        self._queue = queue.Queue()
        self._error = None
        self._closed = False
        self._thread = threading.Thread(target=self._run, name="FrameRecorder", daemon=True)
        self._thread.start()

    def _path(self, rel):
        rel = os.path.normpath(rel)
        if os.path.isabs(rel) or rel.startswith(".."):
            raise ValueError(f"{rel!r} does not lie under the recorder's root")
        return os.path.join(self.root, rel)

    def _write(self, rel, data):
        path = self._path(rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, path)

    def _append(self, rel, data):
        writer = self._videos.get(rel)
        if writer is None:
            from . import jpeg_encode
            path = self._path(rel)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            width, height = jpeg_encode.frame_size(data)
            writer = self._videos[rel] = jpeg_encode.MjpegWriter(path, width, height, self.video_fps)
        writer.add(data)

    def _run(self):
        while True:
            job = self._queue.get()
            if job is None:
                return
            names, pending, files, jpeg_names, jpeg_pending, videos = job
            try:
                if self._error is None:                      # (after an error the queue is drained without writing)
                    for rel, data in zip(names, pending.result() if pending is not None else ()):
                        self._write(rel, data)
                    encoded = jpeg_pending.result() if jpeg_pending is not None else ()
                    for rel, data in zip(jpeg_names, encoded):
                        self._write(rel, data)
                    for rel, data in zip(videos, encoded[len(jpeg_names):]):
                        self._append(rel, data)
                    for rel, data in files.items():
                        self._write(rel, data)
                    self.written += 1
            except BaseException as e:
                self._error = e
            finally:
                self._slots.release()

    def _raise(self):
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    def submit(self, images, files=None, video=None):
        if self._closed:
            raise RuntimeError("FrameRecorder.submit after close()")
        self._raise()
        files, video = dict(files or {}), dict(video or {})
        for rel in list(images) + list(files) + list(video):
            self._path(rel)
        for rel in video:
            if not os.fspath(rel).lower().endswith(".avi"):
                raise ValueError(f"video {rel!r}: the recorder writes Motion JPEG in AVI files, name it .avi")
        png = {rel: t for rel, t in images.items() if not is_jpeg_name(rel)}
        jpeg = {rel: t for rel, t in images.items() if is_jpeg_name(rel)}
        if (jpeg or video) and self.jpeg_encoder is None:
            from . import jpeg_encode
            self.jpeg_encoder = jpeg_encode.JpegEncoder(device=getattr(self.encoder, "device", "cuda"))
        if not self._slots.acquire(blocking=False):
            self.stalls += 1
            self._slots.acquire()
        try:
            pending = self.encoder.encode_async(list(png.values())) if png else None
            jpeg_pending = self.jpeg_encoder.encode_async(list(jpeg.values()) + list(video.values())) if jpeg or video else None
        except BaseException:
            self._slots.release()
            raise
        self.submitted += 1
        self._queue.put((list(png), pending, files, list(jpeg), jpeg_pending, list(video)))

    def close(self):
        if not self._closed:
            self._closed = True
            self._queue.put(None)
            self._thread.join()
            for writer in self._videos.values():
                try:
                    writer.close()
                except BaseException as e:
                    self._error = self._error or e
        self._raise()
