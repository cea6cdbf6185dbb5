"""JPEG files written on the device (thinktwice_amd.jpeg_encode: JpegEncoder; csrc/jpeg_encode.hip: tt_jpeg_encode_u8) against
the numpy restatement tests/jpeg_ref.py and the host build of the same source (tools/jpeg_encode_host_check.cpp, built here
WITHOUT sanitizers), file for file and byte for byte, over every case of tests/jpeg_encode_cases.py in ONE call with all
shapes mixed.  What the bytes must be -- PIL, the tables, the bounds, fidelity and size -- is checked on the restatement and
on the host build's files in test_jpeg_ref.py and test_jpeg_encode_host.py; equality carries it over to the device."""
import ctypes
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import jpeg_encode_cases as E  # noqa: E402
import jpeg_ref  # noqa: E402
from test_jpeg_encode_host import run_checker  # noqa: E402
from thinktwice_amd import jpeg_encode  # noqa: E402
from thinktwice_amd.ops import lib, ptr  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GAP = 100                                                    # guard bytes before, between and after the slots (a multiple of 4)


@functools.lru_cache(maxsize=None)
def _full_frame():
    img = E.camera(900, 1600, 3, 11)
    img.setflags(write=False)
    return ("camera_900x1600x3_q90_420_r1", img, 90, "420", 1)


@functools.lru_cache(maxsize=None)
def _host_files():
    """The host build's files of every case, then of the full-size frame."""
    files, _, run = run_checker(sanitize=False, extra=(_full_frame(),))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return files


def _table(cases):
    """The image table of `cases`, the packed pixels, the size of the slot buffer: slots of exactly tt_jpeg_encode_bound bytes
    rounded up to 4, GAP sentinel bytes around each."""
    table = (jpeg_encode.EncImage * len(cases))()
    pixels, at = [], GAP
    for im, (name, img, quality, sub, rr) in zip(table, cases):
        im.height, im.width, im.channels = img.shape
        im.quality, im.subsampling, im.restart_rows = quality, E.SUBSAMPLING[sub], rr
        im.pixel_offset = sum(len(p) for p in pixels)
        pixels.append(img.tobytes())
        im.file_offset = at
        im.file_capacity = int(lib().tt_jpeg_encode_bound(ctypes.byref(im), 1))
        assert im.file_capacity > 0, name
        at += (im.file_capacity + 3) // 4 * 4 + GAP
    return table, b"".join(pixels), at


def _encode(table, pixels, files_bytes):
    """One tt_jpeg_encode_u8 over a sentinel-filled slot buffer -> (the buffer, the file sizes), on the host."""
    n = len(table)
    dev = torch.device("cuda")
    px = torch.from_numpy(np.frombuffer(pixels, dtype=np.uint8).copy()).to(dev)
    table_dev = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(dev)
    need = int(lib().tt_jpeg_encode_workspace_bytes(table, n))
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    files = torch.full((files_bytes,), SENTINEL, dtype=torch.uint8, device=dev)
    sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    rc = lib().tt_jpeg_encode_u8(ptr(px), px.numel(), table, ptr(table_dev), n, ptr(work), need, ptr(files), files_bytes, ptr(sizes),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().tt_last_error().decode()
    torch.cuda.synchronize()
    return files.cpu().numpy(), sizes.cpu().tolist()


@functools.lru_cache(maxsize=None)
def _device_run():
    table, pixels, files_bytes = _table(E.cases())
    return (table, pixels, files_bytes) + _encode(table, pixels, files_bytes)


@functools.lru_cache(maxsize=None)
def _reference_files():
    return [jpeg_ref.encode(img, quality, sub, rr) for _, img, quality, sub, rr in E.cases()]


def test_device_bytes_equal_the_restatement_and_the_host_build_and_nothing_else_is_written():
    table, _, _, buf, sizes = _device_run()
    covered = np.zeros(buf.shape, dtype=bool)
    for im, size, want, host, (name, *_rest) in zip(table, sizes, _reference_files(), _host_files(), E.cases()):
        assert host == want, name
        assert size == len(want), (name, size, len(want))
        got = buf[im.file_offset:im.file_offset + size].tobytes()
        assert got == want, f"{name}: first difference at byte {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)}"
        covered[im.file_offset:im.file_offset + size] = True
    assert bool((buf[~covered] == SENTINEL).all()), "a byte past a file's size or between the slots was written"


def test_two_calls_give_identical_bytes():
    table, pixels, files_bytes, buf, sizes = _device_run()
    again, sizes_again = _encode(table, pixels, files_bytes)
    assert sizes_again == sizes and np.array_equal(again, buf)


def test_batch_order_and_restart_rows_change_only_the_interval_structure():
    """The same images in two batch orders give the same files; at two restart_rows values only the interval structure may
    differ: the decoded coefficients are the same, the DRI value and the markers follow restart_rows."""
    picks = [c for c in E.cases() if c[0].startswith(("camera", "hud", "image_17x33", "rows"))]
    by_order = []
    for order in (picks, picks[::-1]):
        table, pixels, files_bytes = _table(order)
        buf, sizes = _encode(table, pixels, files_bytes)
        by_order.append({c[0]: buf[im.file_offset:im.file_offset + s].tobytes() for im, s, c in zip(table, sizes, order)})
    assert by_order[0] == by_order[1]
    other = [(name, img, quality, sub, 3 - rr if rr in (1, 2) else 1) for name, img, quality, sub, rr in picks]
    table, pixels, files_bytes = _table(other)
    buf, sizes = _encode(table, pixels, files_bytes)
    for im, s, (name, img, quality, sub, rr) in zip(table, sizes, other):
        f = buf[im.file_offset:im.file_offset + s].tobytes()
        a, b = jpeg_ref.decode_coefficients(f), jpeg_ref.decode_coefficients(by_order[0][name])
        assert all(np.array_equal(x, y) for x, y in zip(a.coefficients, b.coefficients)), name
        mcu = 16 if (img.shape[2] == 3 and sub == "420") else 8
        assert a.dri == rr * -(-img.shape[1] // mcu) and f == jpeg_ref.encode(img, quality, sub, rr), name


def test_encoder_object_mixed_shapes_async_and_other_work_on_the_stream():
    enc = jpeg_encode.JpegEncoder(quality=90, subsampling="420", restart_rows=1)
    picks = [(c, f) for c, f in zip(E.cases(), _reference_files()) if c[2:] == (90, "420", 1)]
    tensors = [torch.from_numpy(c[1].copy()).cuda() for c, _ in picks]
    tensors[0] = tensors[0][:, :, 0]                         # (H, W) for a grey image
    want = [f for _, f in picks]
    assert enc.encode(tensors) == want
    pending = enc.encode_async(tensors)
    x = torch.randn(256, 256, device="cuda")
    y = (x @ x).sum()                                        # other work behind the encoder on the same stream
    assert pending.result() == want and pending.ready() and bool(torch.isfinite(y))
    assert enc.encode(tensors[3:5]) == want[3:5]            # the buffers are reused
    with pytest.raises(ValueError):
        enc.encode([tensors[1].float()])
    for kw in (dict(subsampling="422"), dict(quality=0), dict(quality=101), dict(restart_rows=0)):
        with pytest.raises(ValueError):
            jpeg_encode.JpegEncoder(**kw)


def test_one_full_size_frame_opens_in_pil_and_equals_the_host_build():
    from PIL import Image
    name, img, quality, sub, rr = _full_frame()
    enc = jpeg_encode.JpegEncoder(quality=quality, subsampling=sub, restart_rows=rr)
    f = enc.encode([torch.from_numpy(img.copy()).cuda()])[0]
    assert f == _host_files()[-1], (len(f), len(_host_files()[-1]))
    im = Image.open(io.BytesIO(f))
    im.load()
    assert im.size == (1600, 900) and im.mode == "RGB"
    err = np.abs(np.asarray(im).astype(np.int32) - img.astype(np.int32))
    assert err.mean() < 4.0, err.mean()                      # (a picture of the source, not a measure: fidelity is guarded on the host)


def _refused(mutate, match):
    cases = E.cases()[6:9]
    table, pixels, files_bytes = _table(cases)
    n = len(table)
    dev = torch.device("cuda")
    px = torch.from_numpy(np.frombuffer(pixels, dtype=np.uint8).copy()).to(dev)
    need = int(lib().tt_jpeg_encode_workspace_bytes(table, n))
    table_dev = torch.zeros(ctypes.sizeof(table), dtype=torch.uint8, device=dev)
    work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    files = torch.full((files_bytes,), SENTINEL, dtype=torch.uint8, device=dev)
    sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    args = dict(pixels=ptr(px), pixel_bytes=px.numel(), table=table, table_dev=ptr(table_dev), n=n, work=ptr(work), work_bytes=need,
                files=ptr(files), files_bytes=files_bytes, sizes=ptr(sizes))
    mutate(table, args)
    rc = lib().tt_jpeg_encode_u8(args["pixels"], args["pixel_bytes"], args["table"], args["table_dev"], args["n"], args["work"],
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


REFUSALS = [
    (_arg("pixels", None), "null pointer"), (_arg("table", None), "null pointer"), (_arg("table_dev", None), "null pointer"),
    (_arg("work", None), "null pointer"), (_arg("files", None), "null pointer"), (_arg("sizes", None), "null pointer"),
    (_arg("work", lambda p: p + 16), "misaligned"), (_arg("files", lambda p: p + 1), "misaligned"),
    (_arg("sizes", lambda p: p + 4), "misaligned"), (_arg("table_dev", lambda p: p + 4), "misaligned"),
    (_arg("n", 0), "images"), (_arg("n", 1025), "images"),
    (_set("channels", 2), "channels"), (_set("channels", 4), "channels"), (_set("height", 0), "pixels"), (_set("width", 0), "pixels"),
    (_set("height", 65536), "pixels"), (_set("width", 65536), "pixels"),
    (_set("quality", 0), "quality"), (_set("quality", 101), "quality"),
    (_set("subsampling", 2), "unknown subsampling"), (_set("subsampling", -1), "unknown subsampling"),
    (_set("restart_rows", 0), "restart_rows"), (_set("restart_rows", 65536), "DRI value"),
    (_set("file_offset", GAP + 2), "multiple of 4"), (_set("file_offset", GAP, image=2), "overlap"),
    (_set("file_capacity", 100), "tt_jpeg_encode_bound"), (_arg("files_bytes", lambda b: b - 2 * GAP), "outside the"),
    (_arg("pixel_bytes", lambda b: b - 1), "outside the"), (_arg("work_bytes", lambda b: b - 1), "workspace"),
]


def test_every_refusal_comes_before_any_launch():
    for mutate, match in REFUSALS:
        _refused(mutate, match)
    im = jpeg_encode.EncImage(width=1600, height=900, channels=3, quality=90, subsampling=E.SUBSAMPLING["420"], restart_rows=1)
    assert lib().tt_jpeg_encode_bound(ctypes.byref(im), 1) == 613 + 432 * 57 * 100 * 6 + 2 * 57
    im.restart_rows = 656                                    # 656 * 100 MCUs
    assert lib().tt_jpeg_encode_bound(ctypes.byref(im), 1) == 0 and lib().tt_jpeg_encode_workspace_bytes(ctypes.byref(im), 1) == 0
