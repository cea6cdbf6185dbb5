"""PNG files written on the device (thinktwice_amd.png_encode: PngEncoder; csrc/png_encode.hip: tt_png_encode_u8) against the
host build of the same source (tools/png_encode_host_check.cpp, built here WITHOUT sanitizers), file for file and byte for
byte, over every case of tests/png_encode_cases.py in ONE call with all shapes mixed; and read back by the package's own
decoder, one wave per segment.  What the bytes must be -- scanlines, filter choice, bounds, PIL -- is checked on the host
build's files in test_png_encode_host.py; equality carries it over to the device."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import png_encode_cases as E  # noqa: E402
from test_png_encode_host import run_checker  # noqa: E402
from thinktwice_amd import _lib, png, png_encode  # noqa: E402
from thinktwice_amd.ops import lib, ptr  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GAP = 100                                                    # guard bytes before, between and after the slots (a multiple of 4)


@functools.lru_cache(maxsize=None)
def _host_files():
    files, _, run = run_checker(sanitize=False)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return files


def _table(cases):
    """The image table of `cases`, the packed pixels, the size of the slot buffer: slots of exactly tt_png_encode_bound bytes
    rounded up to 4, GAP sentinel bytes around each."""
    table = (png_encode.EncImage * len(cases))()
    pixels, at = [], GAP
    for im, (name, img, rows, mode) in zip(table, cases):
        im.height, im.width, im.channels = img.shape
        im.rows_per_segment, im.filter = rows, E.MODES[mode]
        im.pixel_offset = sum(len(p) for p in pixels)
        pixels.append(img.tobytes())
        im.file_offset = at
        im.file_capacity = int(lib().tt_png_encode_bound(ctypes.byref(im), 1))
        assert im.file_capacity == E.stored_only_size(img, rows), name
        at += (im.file_capacity + 3) // 4 * 4 + GAP
    return table, b"".join(pixels), at


def _encode(table, pixels, files_bytes):
    """One tt_png_encode_u8 over a sentinel-filled slot buffer -> (the buffer, the file sizes), on the host."""
    n = len(table)
    dev = torch.device("cuda")
    px = torch.from_numpy(np.frombuffer(pixels, dtype=np.uint8).copy()).to(dev)
    table_dev = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(dev)
    need = int(lib().tt_png_encode_workspace_bytes(table, n))
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    files = torch.full((files_bytes,), SENTINEL, dtype=torch.uint8, device=dev)
    sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    rc = lib().tt_png_encode_u8(ptr(px), px.numel(), table, ptr(table_dev), n, ptr(work), need, ptr(files), files_bytes, ptr(sizes),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().tt_last_error().decode()
    torch.cuda.synchronize()
    return files.cpu().numpy(), sizes.cpu().tolist()


@functools.lru_cache(maxsize=None)
def _device_run():
    table, pixels, files_bytes = _table(E.cases())
    return (table, pixels, files_bytes) + _encode(table, pixels, files_bytes)


def test_device_bytes_equal_the_host_builds_file_for_file_and_nothing_else_is_written():
    table, _, _, buf, sizes = _device_run()
    covered = np.zeros(buf.shape, dtype=bool)
    for im, size, want, (name, *_rest) in zip(table, sizes, _host_files(), E.cases()):
        assert size == len(want), (name, size, len(want))
        got = buf[im.file_offset:im.file_offset + size].tobytes()
        assert got == want, f"{name}: first difference at byte {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)}"
        covered[im.file_offset:im.file_offset + size] = True
    assert bool((buf[~covered] == SENTINEL).all()), "a byte past a file's size or between the slots was written"


def test_two_calls_give_identical_bytes():
    table, pixels, files_bytes, buf, sizes = _device_run()
    again, sizes_again = _encode(table, pixels, files_bytes)
    assert sizes_again == sizes and np.array_equal(again, buf)


def test_the_package_decoder_reads_the_device_written_files_by_segments():
    table, _, _, buf, sizes = _device_run()
    narrow = [(im, size, case) for im, size, case in zip(table, sizes, E.cases()) if case[1].shape[1] <= _lib.TT_PNG_MAX_WIDTH]
    assert len(narrow) >= len(E.cases()) - 3                 # (two 40,000-pixel rows and the fibonacci row: wider than the unfilter takes)
    by_shape = {}
    for im, size, (name, img, rows, mode) in narrow:
        by_shape.setdefault(img.shape, []).append((buf[im.file_offset:im.file_offset + size].tobytes(), img))
    seg, whole = png.PngDecoder(segments="require", verify=True), png.PngDecoder(segments="ignore", verify=True)
    for (h, w, c), group in by_shape.items():
        files = [f for f, _ in group]
        want = torch.from_numpy(np.stack([img for _, img in group]))
        got, status = seg.decode(files, check=False)
        assert status.cpu().tolist() == [_lib.TT_PNG_OK] * len(files), (h, w, c)
        plain = whole.decode(files)
        got, plain = got.cpu().reshape(want.shape), plain.cpu().reshape(want.shape)
        assert torch.equal(got, want) and torch.equal(plain, want), (h, w, c)


def test_encoder_object_mixed_shapes_and_async_equal_encode():
    enc = png_encode.PngEncoder()
    picks = [c for c in E.cases() if c[2] == E.DEFAULT_ROWS and c[3] == "adaptive"]
    tensors = [torch.from_numpy(img.copy()).cuda() for _, img, _, _ in picks]
    tensors[0] = tensors[0][:, :, 0]                         # (H, W) for a grey image
    files = enc.encode(tensors)
    host = {name: f for (name, *_), f in zip(E.cases(), _host_files())}
    assert files == [host[name] for name, *_ in picks]
    pending = enc.encode_async(tensors)
    assert pending.result() == files and pending.ready()
    assert enc.encode(tensors[3:5]) == files[3:5]            # the buffers are reused
    with pytest.raises(ValueError):
        enc.encode([tensors[1].float()])
    with pytest.raises(ValueError):
        png_encode.PngEncoder(filter="best")


def _refused(mutate, match, **kw):
    cases = E.cases()[4:7]
    table, pixels, files_bytes = _table(cases)
    n = len(table)
    dev = torch.device("cuda")
    px = torch.from_numpy(np.frombuffer(pixels, dtype=np.uint8).copy()).to(dev)
    need = int(lib().tt_png_encode_workspace_bytes(table, n))
    table_dev = torch.zeros(ctypes.sizeof(table), dtype=torch.uint8, device=dev)
    work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    files = torch.full((files_bytes,), SENTINEL, dtype=torch.uint8, device=dev)
    sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    args = dict(pixels=ptr(px), pixel_bytes=px.numel(), table=table, table_dev=ptr(table_dev), n=n, work=ptr(work), work_bytes=need,
                files=ptr(files), files_bytes=files_bytes, sizes=ptr(sizes))
    mutate(table, args)
    rc = lib().tt_png_encode_u8(args["pixels"], args["pixel_bytes"], args["table"], args["table_dev"], args["n"], args["work"],
                                args["work_bytes"], args["files"], args["files_bytes"], args["sizes"],
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and match in lib().tt_last_error().decode(), (match, rc, lib().tt_last_error().decode())
    assert bool((files == SENTINEL).all()) and bool((sizes == -1).all()), f"{match}: something was launched"


def _set(field, value, image=1):
    def mutate(table, args):
        setattr(table[image], field, value)
    return mutate


def _arg(name, value):
    def mutate(table, args):
        args[name] = value(args[name]) if callable(value) else value
    return mutate


@pytest.mark.parametrize("mutate, match", [
    (_arg("pixels", None), "null pointer"), (_arg("table_dev", None), "null pointer"), (_arg("work", None), "null pointer"),
    (_arg("files", None), "null pointer"), (_arg("sizes", None), "null pointer"),
    (_arg("work", lambda p: p + 16), "misaligned"), (_arg("files", lambda p: p + 1), "misaligned"),
    (_arg("sizes", lambda p: p + 4), "misaligned"), (_arg("table_dev", lambda p: p + 4), "misaligned"),
    (_arg("n", 0), "images"),
    (_set("channels", 2), "channels"), (_set("channels", 4), "channels"), (_set("height", 0), "pixels"), (_set("width", 0), "pixels"),
    (_set("rows_per_segment", 0), "rows_per_segment"), (_set("filter", 6), "unknown filter mode"), (_set("filter", -1), "unknown filter mode"),
    (_set("file_offset", GAP + 2), "multiple of 4"), (_set("file_offset", GAP, image=2), "overlap"),
    (_set("file_capacity", 100), "tt_png_encode_bound"), (_arg("files_bytes", lambda b: b - 2 * GAP), "outside the"),
    (_arg("pixel_bytes", lambda b: b - 1), "outside the"), (_arg("work_bytes", lambda b: b - 1), "workspace"),
    (_set("width", 1 << 30), "2^31 - 8"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_every_refusal_comes_before_any_launch(mutate, match):
    _refused(mutate, match)
