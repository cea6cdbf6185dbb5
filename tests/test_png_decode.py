"""The dataset's PNG files decoded on the device (thinktwice_amd.png, csrc/png.hip: tt_png_decode_u8) against the arrays the
files were made from.  Everything is compared BIT FOR BIT: a PNG decode has one right answer.  Every stream comes from
tests/png_cases.py; the same cases run through the same inflate source on the CPU under sanitizers in test_png_host.py.

Shapes.  The unfilter runs 64 rows as one wavefront band, so 64 x 3, 65 x 3 and 130 x 9 have none, one and two hand-overs
between bands; 1 x 1, 1 x 7 and 5 x 1 have no left or no upper neighbour; every row byte count but one is no multiple of 4.
The inflate has no size thresholds but its 8 KiB flush, its 4 KiB input stage and the 32 KiB ring: the level-0 case
(67,950 bytes in two stored blocks) and the hand-assembled 32,768-distance streams cross all three."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import png_cases as P  # noqa: E402
from thinktwice_amd import _lib, calib, labels, png, synth  # noqa: E402
from thinktwice_amd.ops import lib, ptr  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f21_png_decode.npz")
SENTINEL = 0xA5
IDXS = [1, 4, 5, 6, 7, 8, 10, 12, 18]           # configs/thinktwice.py:108


@functools.lru_cache(maxsize=None)
def _decoder():
    return png.PngDecoder()


def _info(stream, h, w, c):
    return png.PngInfo(w, h, c, stream)


def _ragged(cases, gap=97, check=True, decoder=None):
    """cases [(stream, h, w, c)] -> (uint8 buffer as numpy, [offset], statuses or None): one call, every image in its own
    slot of one sentinel-filled buffer, `gap` sentinel bytes (no multiple of 16) before, between and after the slots."""
    offsets, pos = [], gap
    for _, h, w, c in cases:
        offsets.append(pos)
        pos += h * w * c + gap
    out = torch.full((pos,), SENTINEL, dtype=torch.uint8, device="cuda")
    status = (decoder or _decoder())._run([_info(*k) for k in cases], offsets, out, out.numel(), check)
    torch.cuda.synchronize()
    return out.cpu().numpy(), offsets, (None if status is None else status.cpu().numpy())


def _check_slots(buf, offsets, cases, want):
    """want[i]: the array of image i, None where its slot must still be sentinel; everything between the slots is sentinel."""
    covered = np.zeros(buf.shape, dtype=bool)
    for i, ((_, h, w, c), o) in enumerate(zip(cases, offsets)):
        n = h * w * c
        covered[o:o + n] = True
        if want[i] is None:
            assert bool((buf[o:o + n] == SENTINEL).all()), f"image {i}: a failed image's destination was written"
        else:
            assert np.array_equal(buf[o:o + n], np.asarray(want[i]).reshape(-1)), f"image {i} differs"
    assert bool((buf[~covered] == SENTINEL).all()), "bytes outside the destinations were written"


# ------------------------------------------------------------------------------------------------------------- good cases
def test_every_size_filter_compressor_and_hand_assembled_stream_in_one_ragged_call():
    good = P.good_cases()
    cases = [(s, h, w, c) for _, s, h, w, c, _ in good]
    buf, offsets, _ = _ragged(cases)
    _check_slots(buf, offsets, cases, [img for *_, img in good])


@pytest.mark.parametrize("h, w", P.SIZES)
@pytest.mark.parametrize("c", [1, 3])
def test_decode_returns_the_batch_of_one_size_with_every_filter(h, w, c):
    img = P.image(h, w, c)
    src = img if c == 3 else img[:, :, 0]
    files = [P.write_png(src, P.filter_types(f, h), idat_bytes=(100, 65536)[i % 2], ancillary=bool(i % 2))
             for i, f in enumerate(P.FILTERS)]
    out = _decoder().decode(files)
    assert out.dtype == torch.uint8 and tuple(out.shape) == ((len(files), h, w, 3) if c == 3 else (len(files), h, w))
    for i in range(len(files)):
        assert np.array_equal(out[i].cpu().numpy(), src), P.FILTERS[i]
    into = torch.zeros_like(out)
    assert _decoder().decode(files, out=into) is into and torch.equal(into, out)


def test_ragged_mix_in_strided_slots_leaves_the_bytes_around_them_and_beyond_the_workspace():
    big = P.image(300, 700, 3, seed=11)                                    # 630,300 scanline bytes
    noisy = np.random.default_rng(4).integers(0, 256, (400, 900, 3), dtype=np.uint8)       # incompressible: > 1 MB of stream
    flat = np.full((200, 500, 1), 9, dtype=np.uint8)                       # tens of bytes of stream
    items = [(big, "random", "level6"), (flat, "none", "level9"), (noisy, "paeth", "level1"), (P.image(5, 1, 1), "sub", "fixed"),
             (P.image(65, 3, 3), "average", "level6"), (noisy[:50, :60, :1].copy(), "up", "level0")]
    cases = [(P.COMPRESSORS[comp](P.filter_rows(a, P.filter_types(f, a.shape[0]))),) + a.shape for a, f, comp in items]
    sizes = sorted(len(k[0]) for k in cases)
    assert sizes[0] < 100 and sizes[-1] > 1 << 20
    dec = png.PngDecoder()
    table = (png.PngImage * len(cases))()
    for im, (_, h, w, c) in zip(table, cases):
        im.width, im.height, im.channels = w, h, c
    need = int(lib().tt_png_workspace_bytes(table, len(cases)))
    assert need == sum(-(-(h * (1 + w * c)) // 256) * 256 for _, h, w, c in cases)
    dec._work = torch.full((need + 65536,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf, offsets, _ = _ragged(cases, gap=1000 + 7, decoder=dec)
    _check_slots(buf, offsets, cases, [a for a, _, _ in items])
    assert bool((dec._work[need:] == SENTINEL).all()), "the workspace was written beyond tt_png_workspace_bytes"


def test_two_calls_give_identical_bytes():
    good = P.good_cases()[::5]
    cases = [(s, h, w, c) for _, s, h, w, c, _ in good]
    a, _, _ = _ragged(cases)
    b, _, _ = _ragged(cases)
    assert np.array_equal(a, b)


def test_golden_f21_files_decode_to_what_the_reference_loaded():
    g = np.load(GOLDEN)
    for kind in ("rgb", "depth", "seg"):
        out = _decoder().decode([g[f"{kind}_file"].tobytes()])[0].cpu().numpy()
        assert out.shape == g[f"{kind}_array"].shape and np.array_equal(out, g[f"{kind}_array"]), kind


# -------------------------------------------------------------------------------------------------------------- full size
@functools.lru_cache(maxsize=None)
def _full_size():
    """One 900 x 1600 sample with T = 2, N = 1: (arrays, files) of the two frames, the depth-coded image and the tag map.
    The depth is a smooth ramp in CARLA's 24-bit code; the filters cycle through all five types."""
    d, t, c = synth.raw_label_bytes(19, 1, 900, 1600)
    yy, xx = np.mgrid[0:900, 0:1600]
    code = ((yy * 11 + xx * 7) * 16777215 // (900 * 11 + 1600 * 7)).astype(np.uint32)
    depth = np.stack([code & 255, (code >> 8) & 255, code >> 16], axis=-1).astype(np.uint8)
    prev = synth.raw_camera_frames(3, T=1, N=1)[0, 0]
    arrays = {"prev": prev, "key": c[0], "depth": depth, "seg": t[0]}
    types = [y % 5 for y in range(900)]
    files = {k: P.write_png(a, types, compressor="level1") for k, a in arrays.items()}
    for a in arrays.values():
        a.setflags(write=False)
    return arrays, files


@pytest.mark.parametrize("kind", ["key", "depth", "seg"])
def test_one_full_size_image_of_each_kind(kind):
    arrays, files = _full_size()
    out = _decoder().decode([files[kind]])
    assert np.array_equal(out[0].cpu().numpy(), arrays[kind])


def test_one_sample_through_decoder_label_decoder_and_image_pipeline():
    from thinktwice_amd.preprocess import IdaSampler, TrainImagePipeline
    arrays, files = _full_size()
    raw, depth_png, seg_png = _decoder().decode_sample_batch([[[files["prev"]], [files["key"]]]], [[files["depth"]]], [[files["seg"]]])
    assert tuple(raw.shape) == (1, 2, 1, 900, 1600, 3) and tuple(depth_png.shape) == (1, 1, 900, 1600, 3)
    assert tuple(seg_png.shape) == (1, 1, 900, 1600) and raw.is_contiguous() and depth_png.is_contiguous() and seg_png.is_contiguous()
    want_raw = torch.from_numpy(np.stack([arrays["prev"], arrays["key"]])[None, :, None]).cuda()
    want_depth, want_seg = (torch.from_numpy(np.array(arrays[k])[None, None]).cuda() for k in ("depth", "seg"))
    assert torch.equal(raw, want_raw) and torch.equal(depth_png, want_depth) and torch.equal(seg_png, want_seg)
    conf = dict(calib.IDA_AUG_CONF, final_dim=(128, 256), resize_lim=(0.16, 0.18))
    dec, pipe, params = labels.RawLabelDecoder(IDXS), TrainImagePipeline(conf), IdaSampler(conf, seed=4).sample(1, 1)
    a = pipe(raw, *dec(raw, depth_png, seg_png), params=params)
    b = pipe(want_raw, *dec(want_raw, want_depth, want_seg), params=params)
    for k in ("img", "depth", "seg"):
        assert torch.equal(a[k], b[k]), k


# -------------------------------------------------------------------------------------------------------------- malformed
def test_malformed_streams_between_good_images_end_in_their_status_and_touch_nothing():
    """Error paths that must return codes.  Precondition, kept by the order of work and not by this test: the identical list,
    png_cases.malformed_cases(), passes the sanitized CPU run of the same inflate source (tests/test_png_host.py, in the CPU
    suite) before it is put on a device.  No sanitizer and no compiler runs from here."""
    mal = P.malformed_cases()
    good = [k for k in P.good_cases() if k[0] in ("37x53x3_random", "compressor_flushes", "hand_overlapping_matches", "65x3x1_paeth")]
    cases, want, expected = [], [], []
    for i, (name, stream, status) in enumerate(mal):
        cases.append((stream, P.MAL_H, P.MAL_W, P.MAL_C))
        want.append(None)
        expected.append(P.STATUS[status])
        _, s, h, w, c, img = good[i % len(good)]
        cases.append((s, h, w, c))
        want.append(img)
        expected.append(0)
    buf, offsets, status = _ragged(cases, check=False)
    names = [n for n, _, _ in mal]
    got = {names[i // 2]: int(status[i]) for i in range(0, len(cases), 2)}
    assert got == {n: P.STATUS[s] for n, _, s in mal}
    assert status.tolist() == expected
    _check_slots(buf, offsets, cases, want)
    with pytest.raises(png.PngDecodeError) as e:
        _ragged(cases, check=True)
    assert e.value.failed == [(i, png.STATUS_NAMES[s]) for i, s in enumerate(expected) if s]
    for i, s in enumerate(expected):
        if s:
            assert f"image {i}: {png.STATUS_NAMES[s]}" in str(e.value)


# ------------------------------------------------------------------------------------------------ the entry's refusals
def test_every_host_side_refusal_returns_an_error_and_launches_nothing():
    img = P.image(4, 5, 3)
    stream = P.COMPRESSORS["level6"](P.filter_rows(img, [0] * 4))
    packed_host = np.zeros(1024, dtype=np.uint8)
    packed_host[256:256 + len(stream)] = np.frombuffer(stream, dtype=np.uint8)

    def table(n=2, **kw):
        t = (png.PngImage * max(n, 1))()
        for i in range(max(n, 1)):
            t[i].stream_offset, t[i].stream_bytes, t[i].dst_offset = 256, len(stream), 64 * i
            t[i].width, t[i].height, t[i].channels = 5, 4, 3
        for k, v in kw.items():
            setattr(t[0], k, v)
        return t

    good = table()
    packed_host[:ctypes.sizeof(good)] = np.frombuffer(good, dtype=np.uint8)
    packed = torch.from_numpy(packed_host).cuda()
    work = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    base = dict(packed=ptr(packed), packed_bytes=1024, host=good, dev=ptr(packed), n=2, work=ptr(work), work_bytes=4096,
                out=ptr(out), out_bytes=4096, status=ptr(status))

    def call(**kw):
        a = dict(base, **kw)
        return lib().tt_png_decode_u8(a["packed"], a["packed_bytes"], a["host"], a["dev"], a["n"], a["work"], a["work_bytes"],
                                      a["out"], a["out_bytes"], a["status"], None)

    wide = _lib.TT_PNG_MAX_WIDTH + 1
    refusals = {
        "null packed": dict(packed=None), "null host table": dict(host=None), "null device table": dict(dev=None),
        "null workspace": dict(work=None), "null output": dict(out=None), "null status": dict(status=None),
        "no images": dict(n=0), "negative count": dict(n=-1), "too many images": dict(n=_lib.TT_PNG_MAX_IMAGES + 1),
        "two channels": dict(host=table(channels=2)), "four channels": dict(host=table(channels=4)),
        "zero width": dict(host=table(width=0)), "negative height": dict(host=table(height=-4)),
        "scanlines beyond int32": dict(host=table(width=8000, height=100000)),
        "row beyond the unfilter's limit": dict(host=table(width=wide)),
        "stream past the packed bytes": dict(host=table(stream_offset=1024 - len(stream) + 1)),
        "negative stream offset": dict(host=table(stream_offset=-1)),
        "stream of five bytes": dict(host=table(stream_bytes=5)),
        "destination past the output": dict(host=table(dst_offset=4096 - 59)),
        "negative destination": dict(host=table(dst_offset=-1)),
        "overlapping destinations": dict(host=table(dst_offset=64 + 59)),
        "workspace one byte short": dict(work_bytes=511),
        "misaligned workspace": dict(work=ptr(work) + 16), "misaligned packed buffer": dict(packed=ptr(packed) + 4),
    }
    for what, kw in refusals.items():
        assert call(**kw) < 0, what
        assert lib().tt_last_error().decode().startswith("tt_png_decode_u8"), what
    assert lib().tt_png_workspace_bytes(table(width=wide), 2) == 0 and lib().tt_png_workspace_bytes(good, 0) == 0
    assert lib().tt_png_workspace_bytes(good, 2) == 512
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((work == SENTINEL).all()) and bool((status == -7).all())
    assert call() == 0                                                  # the same arguments, unspoilt, decode
    torch.cuda.synchronize()
    assert status[:2].tolist() == [0, 0] and np.array_equal(out[64:124].cpu().numpy(), img.reshape(-1))
