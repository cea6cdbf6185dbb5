"""jpeg_encode.MjpegWriter and the recorder's routing, on the CPU.  The RIFF reader below is written from the AVI
specification (RIFF chunks: fourcc, little-endian size, payload, a pad byte after an odd payload; LIST / RIFF chunks carry a
type fourcc and hold chunks) and does not import the writer: the chunk tree must close exactly at the file's end, the counts
of avih / strh must equal the frames added, and every idx1 entry must point at a 00dc chunk PIL decodes."""
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import jpeg_ref  # noqa: E402


def chunks(data, at, end):
    """-> [(fourcc, list type or None, payload offset, payload size)] of the chunks in data[at:end], which they fill exactly."""
    out = []
    while at < end:
        assert at + 8 <= end, f"a chunk header at {at} passes the end {end}"
        cc, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        assert at + 8 + size <= end, f"{cc} at {at}: {size} bytes pass the end {end}"
        if cc in (b"RIFF", b"LIST"):
            out.append((cc, data[at + 8:at + 12], at + 12, size - 4))
        else:
            out.append((cc, None, at + 8, size))
        at += 8 + size + (size & 1)
    assert at == end, f"the chunks end at {at}, the container at {end}"
    return out


def read_avi(data):
    """-> dict(avih, strh, strf: the unpacked headers; frames: [bytes] by idx1; movi_frames: number of 00dc chunks)."""
    (cc, kind, at, size), = chunks(data, 0, len(data))
    assert (cc, kind) == (b"RIFF", b"AVI ")
    top = chunks(data, at, at + size)
    assert [(c, k) for c, k, _, _ in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl = chunks(data, top[0][2], top[0][2] + top[0][3])
    assert [(c, k) for c, k, _, _ in hdrl] == [(b"avih", None), (b"LIST", b"strl")] and hdrl[0][3] == 56
    strl = chunks(data, hdrl[1][2], hdrl[1][2] + hdrl[1][3])
    assert [(c, k) for c, k, _, _ in strl] == [(b"strh", None), (b"strf", None)] and strl[0][3] == 56 and strl[1][3] == 40
    avih = struct.unpack_from("<14I", data, hdrl[0][2])
    strh = struct.unpack_from("<4s4sIHHIIIIIIII4H", data, strl[0][2])
    strf = struct.unpack_from("<IiiHH4sIiiII", data, strl[1][2])
    movi = chunks(data, top[1][2], top[1][2] + top[1][3])
    assert all(c == b"00dc" for c, _, _, _ in movi)
    movi_fourcc = top[1][2] - 4
    n = top[2][3] // 16
    assert top[2][3] == 16 * n
    frames = []
    for i in range(n):
        cc, flags, offset, size = struct.unpack_from("<4sIII", data, top[2][2] + 16 * i)
        assert cc == b"00dc" and flags & 0x10, i
        assert (b"00dc", None, movi_fourcc + offset + 8, size) == movi[i], (i, movi[i])
        frames.append(data[movi_fourcc + offset + 8:movi_fourcc + offset + 8 + size])
    return dict(avih=avih, strh=strh, strf=strf, frames=frames, movi_frames=len(movi))


def _frames(n, h=24, w=40, seed=0):
    rng = np.random.default_rng(seed)
    imgs = [np.clip(rng.integers(0, 40, (h, w, 3)) + 20 * i + np.arange(w)[None, :, None] * 3, 0, 255).astype(np.uint8) for i in range(n)]
    return imgs, [jpeg_ref.encode(img, 70 + (i % 5), "420", 1) for i, img in enumerate(imgs)]


def _check(path, want, w=40, h=24, fps=4.0):
    from PIL import Image
    avi = read_avi(open(path, "rb").read())
    n = len(want)
    assert avi["movi_frames"] == n and len(avi["frames"]) == n and avi["frames"] == want
    assert avi["avih"][4] == n and avi["strh"][9] == n                          # dwTotalFrames, dwLength
    assert avi["avih"][0] == round(1e6 / fps) and avi["strh"][7] / avi["strh"][6] == fps
    assert avi["avih"][3] & 0x10 and avi["avih"][6] == 1 and avi["avih"][8:10] == (w, h)
    assert avi["strh"][:2] == (b"vids", b"MJPG") and avi["strh"][-2:] == (w, h)
    assert avi["strf"][:6] == (40, w, h, 1, 24, b"MJPG")
    largest = max(len(f) + (len(f) & 1) for f in want)
    assert avi["avih"][7] == largest and avi["strh"][10] == largest              # dwSuggestedBufferSize
    for f in avi["frames"]:
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.size == (w, h)
    return avi


def test_the_file_is_a_closed_riff_tree_whose_index_finds_every_frame(tmp_path):
    from PIL import Image
    from thinktwice_amd.jpeg_encode import MjpegWriter, frame_size
    imgs, files = _frames(7)
    files[2] = jpeg_ref.encode(imgs[2], 71, "420", 1)
    assert any(len(f) & 1 for f in files) and any(not len(f) & 1 for f in files)      # odd and even payloads
    path = tmp_path / "drive.avi"
    with MjpegWriter(path, 40, 24, 4.0) as video:
        for f in files:
            video.add(f)
    assert video.frames == 7 and video.paths == [os.fspath(path)] and frame_size(files[0]) == (40, 24)
    avi = _check(path, files)
    for f, img in zip(avi["frames"], imgs):                                          # the frames that were added, in order
        err = np.abs(np.asarray(Image.open(io.BytesIO(f))).astype(np.int32) - img.astype(np.int32))
        assert err.mean() < 12, err.mean()
    # PIL's own files are frames too
    out = io.BytesIO()
    Image.fromarray(imgs[0]).save(out, "JPEG", quality=80)
    with MjpegWriter(tmp_path / "pil.avi", 40, 24, 4.0) as video:
        video.add(out.getvalue())
    _check(tmp_path / "pil.avi", [out.getvalue()])


def test_an_abandoned_writer_leaves_the_frames_of_the_last_periodic_index(tmp_path):
    from thinktwice_amd.jpeg_encode import MjpegWriter
    _, files = _frames(9, seed=1)
    path = tmp_path / "killed.avi"
    video = MjpegWriter(path, 40, 24, 4.0, index_every=4)
    for f in files[:4]:
        video.add(f)
    _check(path, files[:4])                                  # read while the writer is open and never closed: a valid file
    for f in files[4:8]:
        video.add(f)                                         # (frame 5 overwrote the first index)
    _check(path, files[:8])
    video.add(files[8])
    video.close()
    _check(path, files)
    with pytest.raises(RuntimeError):
        video.add(files[0])


def test_roll_over_before_the_size_limit_and_refusals(tmp_path):
    from thinktwice_amd.jpeg_encode import MjpegWriter
    _, files = _frames(6, seed=2)
    limit = 224 + 3 * (max(len(f) for f in files) + 9) + 8 + 16 * 3
    path = tmp_path / "long.avi"
    video = MjpegWriter(path, 40, 24, 4.0, max_bytes=limit)
    for f in files:
        video.add(f)
    video.close()
    assert video.paths == [os.fspath(path), os.fspath(tmp_path / "long_0001.avi")]      # the limit holds three frames and their index
    got = []
    for p in video.paths:
        assert os.path.getsize(p) <= limit
        got += _check(p, files[len(got):len(got) + read_avi(open(p, "rb").read())["movi_frames"]])["frames"]
    assert got == files
    # a frame of another size, and bytes that are no JPEG file
    _, other = _frames(1, h=16, w=40)
    video = MjpegWriter(tmp_path / "refuse.avi", 40, 24, 4.0)
    with pytest.raises(ValueError, match="40 x 16"):
        video.add(other[0])
    with pytest.raises(ValueError):
        video.add(b"\x89PNG\r\n\x1a\n" + bytes(40))
    video.add(files[0])
    video.close()
    _check(tmp_path / "refuse.avi", files[:1])
    for kw in (dict(width=0), dict(fps=0), dict(index_every=0), dict(max_bytes=1 << 33)):
        args = dict(path=tmp_path / "x.avi", width=40, height=24, fps=4.0)
        args.update(kw)
        with pytest.raises(ValueError):
            MjpegWriter(**args)


class _Pending:
    def __init__(self, files):
        self.files = files

    def result(self):
        return self.files


class _StubEncoder:
    """Records its calls; `files` maps an image (here: any object) to the bytes it "encodes" to."""

    def __init__(self, encode):
        self.calls, self._encode = [], encode

    def encode_async(self, images):
        self.calls.append(list(images))
        return _Pending([self._encode(im) for im in images])


def test_the_recorder_routes_by_extension_and_appends_video_frames_in_order(tmp_path):
    from thinktwice_amd import png_encode
    imgs, files = _frames(3, seed=3)
    png, jpg = _StubEncoder(lambda im: b"PNG" + bytes([im])), _StubEncoder(lambda im: files[im])
    rec = png_encode.FrameRecorder(tmp_path, encoder=png, jpeg_encoder=jpg, max_pending=2, video_fps=4.0)
    rec.submit({"rgb_front/0000.png": 0, "depth/0000.png": 1}, {"meta/0000.json": b"{}"})
    assert len(png.calls) == 1 and png.calls[0] == [0, 1] and jpg.calls == []        # PNG names only: one PNG call, no JPEG call
    rec.submit({"rgb_front/0001.JPG": 1, "tags/0001.png": 7, "rgb_left/0001.jpeg": 2}, video={"debug.avi": 0})
    assert png.calls[1:] == [[7]] and jpg.calls == [[1, 2, 0]]                       # one call each; the video frame rides with the JPEGs
    rec.submit({}, video={"debug.avi": 1, "sub/second.avi": 2})
    rec.submit({}, video={"debug.avi": 2})
    assert len(png.calls) == 2 and jpg.calls[1:] == [[1, 2], [2]]
    with pytest.raises(ValueError, match=".avi"):
        rec.submit({}, video={"debug.mp4": 0})
    with pytest.raises(ValueError):
        rec.submit({}, video={"../debug.avi": 0})
    rec.close()
    assert rec.submitted == 4 and rec.written == 4
    assert (tmp_path / "rgb_front/0000.png").read_bytes() == b"PNG\x00" and (tmp_path / "tags/0001.png").read_bytes() == b"PNG\x07"
    assert (tmp_path / "rgb_front/0001.JPG").read_bytes() == files[1] and (tmp_path / "rgb_left/0001.jpeg").read_bytes() == files[2]
    assert (tmp_path / "meta/0000.json").read_bytes() == b"{}"
    _check(tmp_path / "debug.avi", files)
    _check(tmp_path / "sub/second.avi", files[2:])
    assert not [p for p in tmp_path.rglob("*") if ".tmp" in p.name]
