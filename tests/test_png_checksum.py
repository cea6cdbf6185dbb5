"""The checksum kernels (thinktwice_amd.png.device_adler32 / device_crc32: tt_checksum_ranges_u8) and the verified PNG decode
(PngDecoder(verify=...): tt_png_decode_u8_verified) on the device.  The truth for every value is Python's zlib.adler32,
zlib.crc32 and zlib.decompress, and everything is compared BIT FOR BIT.  The cases are tests/png_checksum_cases.py's; the same
cases run through the same source on the CPU under sanitizers in test_png_checksum_host.py.

Shapes.  A tile is T = TT_CHECKSUM_TILE bytes and a lane's slice T / 256 = 256 bytes: the lengths surround 4 (the word loop),
16, 64, 256 (one slice), 4096, 5552 (zlib's NMAX) and T, 2T, 5T (one, three and six workgroups per range)."""
import ctypes
import functools
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import png_cases as P  # noqa: E402
import png_checksum_cases as K  # noqa: E402
from thinktwice_amd import _lib, png, synth  # noqa: E402
from thinktwice_amd.ops import lib, ptr  # noqa: E402

pytestmark = pytest.mark.gpu
T = K.T
SENTINEL = 0xA5
DEVICE = {K.ADLER32: png.device_adler32, K.CRC32: png.device_crc32}
KINDS = [pytest.param(K.ADLER32, id="adler32"), pytest.param(K.CRC32, id="crc32")]
OK, BAD_ADLER, BAD_CRC = 0, K.STATUS["TT_PNGV_BAD_ADLER32"], K.STATUS["TT_PNGV_BAD_CRC32"]


def _run(kind, data, ranges=None, start=None):
    """data: uint8 numpy array -> [uint32 as int] from the device."""
    out = DEVICE[kind](torch.from_numpy(np.array(data, dtype=np.uint8)).cuda(), ranges, start)      # (a copy: some cases are read-only)
    assert out.dtype == torch.uint32 and tuple(out.shape) == (1 if ranges is None else len(ranges),)
    return out.cpu().numpy().astype(np.int64).tolist()


# ------------------------------------------------------------------------------------------------------------ op level
def test_the_header_constants_are_the_case_generators():
    assert _lib.TT_CHECKSUM_TILE == T == 65536 and (_lib.TT_CHECKSUM_ADLER32, _lib.TT_CHECKSUM_CRC32) == (K.ADLER32, K.CRC32)
    assert (_lib.TT_PNGV_BAD_ADLER32, _lib.TT_PNGV_BAD_CRC32, _lib.TT_PNGV_ADLER32, _lib.TT_PNGV_CRC32) == (11, 12, 1, 2)
    assert png.STATUS_NAMES[11] == "TT_PNGV_BAD_ADLER32" and png.STATUS_NAMES[12] == "TT_PNGV_BAD_CRC32"


@pytest.mark.parametrize("kind", KINDS)
def test_every_length_equals_zlib(kind):
    total, ranges = K.packed_ranges(K.LENGTHS)
    data = K.random_bytes(total, 1)
    assert _run(kind, data, ranges) == K.expected(kind, data, ranges)
    for n in (0, 1, T + 1):                                            # ranges=None: the whole tensor
        if n:
            assert _run(kind, data[:n]) == K.expected(kind, data[:n], [(0, n)])


@pytest.mark.parametrize("kind", KINDS)
def test_every_alignment_equals_zlib_whatever_surrounds_the_range(kind):
    n = 4097
    ranges = [(64 * i + i, n) for i in range(16)]                      # start residues 0 .. 15 mod 16
    assert sorted(o % 16 for o, _ in ranges) == list(range(16))
    payload = K.random_bytes(n, 5)
    results = []
    for seed in (6, 7):
        data = K.random_bytes(64 * 16 + 16 + n + 33, seed)
        want = []
        for i, (o, _) in enumerate(ranges):                            # the ranges overlap: one call per range
            buf = data.copy()
            buf[o:o + n] = payload
            results.append(_run(kind, buf, [ranges[i]]))
            want.append(K.expected(kind, buf, [ranges[i]]))
            assert results[-1] == want[-1], (seed, i)
    assert results[:16] == results[16:]


def test_adler32_extremes():
    for name, a, start in K.adler_extremes():
        if len(a) == 0:
            continue                                                   # (an empty tensor has no device pointer: see below)
        assert _run(K.ADLER32, a, [(0, len(a))], [start]) == [zlib.adler32(a.tobytes(), start)], name
    starts = [(65520 << 16) | 65520, 65520, 65520 << 16]
    assert _run(K.ADLER32, np.zeros(4, np.uint8), [(2, 0)] * 3, starts) == starts          # empty ranges return their start


def test_crc32_start_values_constant_ranges_and_one_tile_plus_one_byte():
    rng = np.random.default_rng(12)
    total, ranges = K.packed_ranges([0, 1, 255, 257, 5553, T, T + 1, 2 * T + 3])
    data = K.random_bytes(total, 13)
    start = rng.integers(0, 1 << 32, len(ranges), dtype=np.uint64)
    assert _run(K.CRC32, data, ranges, start) == K.expected(K.CRC32, data, ranges, start)
    for fill in (0, 255):
        a = np.full(T + 1, fill, dtype=np.uint8)
        for r in ([(0, T + 1)], [(1, T)], [(0, 1), (0, 0), (3, 257)]):
            assert _run(K.CRC32, a, r) == K.expected(K.CRC32, a, r), (fill, r)


@pytest.mark.parametrize("kind", KINDS)
def test_two_hundred_shuffled_ranges_with_empty_adjacent_and_overlapping_ones(kind):
    total, ranges = K.many_ranges()
    assert len(ranges) > 200 and sum(n == 0 for _, n in ranges) > 10
    data = K.random_bytes(total, 3)
    assert _run(kind, data, ranges) == K.expected(kind, data, ranges)
    start = np.random.default_rng(4).integers(0, 1 << 32, len(ranges), dtype=np.uint64)
    assert _run(kind, data, ranges, start) == K.expected(kind, data, ranges, start)


def test_every_host_side_refusal_of_the_op_returns_an_error_and_launches_nothing():
    data = torch.from_numpy(K.random_bytes(1000, 2)).cuda()

    def table(n=2, **kw):
        t = (png.ChecksumRange * max(n, 1))()
        for i in range(max(n, 1)):
            t[i].offset, t[i].bytes = 10 * i, 300
        for k, v in kw.items():
            setattr(t[0], k, v)
        return t

    good = table()
    dev = torch.from_numpy(np.frombuffer(good, dtype=np.uint8).copy()).cuda()
    need = int(lib().tt_checksum_workspace_bytes(good, 2))
    assert need > 0
    work = torch.full((need + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    base = dict(data=ptr(data), data_bytes=1000, host=good, dev=ptr(dev), n=2, kind=K.CRC32, start=None, out=ptr(out), work=ptr(work),
                work_bytes=need)

    def call(**kw):
        a = dict(base, **kw)
        return lib().tt_checksum_ranges_u8(a["data"], a["data_bytes"], a["host"], a["dev"], a["n"], a["kind"], a["start"], a["out"],
                                           a["work"], a["work_bytes"], None)

    refusals = {
        "null data": dict(data=None), "null host table": dict(host=None), "null device table": dict(dev=None),
        "null output": dict(out=None), "null workspace": dict(work=None),
        "no ranges": dict(n=0), "negative count": dict(n=-1), "too many ranges": dict(n=_lib.TT_CHECKSUM_MAX_RANGES + 1),
        "negative bytes": dict(host=table(bytes=-1)), "negative offset": dict(host=table(offset=-1)),
        "range past the data": dict(host=table(offset=701)), "range past shorter data": dict(data_bytes=309),
        "unknown kind": dict(kind=2), "negative kind": dict(kind=-1),
        "workspace one byte short": dict(work_bytes=need - 1), "misaligned workspace": dict(work=ptr(work) + 16),
    }
    for what, kw in refusals.items():
        assert call(**kw) < 0, what
        assert lib().tt_last_error().decode().startswith("tt_checksum_ranges_u8"), what
    assert lib().tt_checksum_workspace_bytes(table(bytes=-1), 2) == 0 and lib().tt_checksum_workspace_bytes(good, 0) == 0
    torch.cuda.synchronize()
    assert bool((work == SENTINEL).all()) and bool((out == -7).all())
    assert call() == 0                                                  # the same arguments, unspoilt
    torch.cuda.synchronize()
    raw = data.cpu().numpy().tobytes()
    assert out.view(torch.uint32)[:2].cpu().numpy().tolist() == [zlib.crc32(raw[0:300]), zlib.crc32(raw[10:310])]
    assert bool((work[need:] == SENTINEL).all()), "the workspace was written beyond tt_checksum_workspace_bytes"


# -------------------------------------------------------------------------------------------------------- decode level
@functools.lru_cache(maxsize=None)
def _decoder(verify):
    return png.PngDecoder(verify=verify)


def _decode_slots(decoder, files, shapes, gap=97):
    """files of any sizes -> (buffer as numpy, [offset], statuses): one call, every image in its own slot of a sentinel-filled
    buffer, as test_png_decode._ragged does for bare streams."""
    infos = decoder._parse(files)
    offsets, pos = [], gap
    for h, w, c in shapes:
        offsets.append(pos)
        pos += h * w * c + gap
    out = torch.full((pos,), SENTINEL, dtype=torch.uint8, device="cuda")
    status = decoder._run(infos, offsets, out, out.numel(), False)
    torch.cuda.synchronize()
    return out.cpu().numpy(), offsets, status.cpu().numpy().tolist()


def _check_slots(buf, offsets, shapes, want):
    covered = np.zeros(buf.shape, dtype=bool)
    for i, ((h, w, c), o) in enumerate(zip(shapes, offsets)):
        n = h * w * c
        covered[o:o + n] = True
        if want[i] is None:
            assert bool((buf[o:o + n] == SENTINEL).all()), f"image {i}: a failed image's destination was written"
        else:
            assert np.array_equal(buf[o:o + n], np.asarray(want[i]).reshape(-1)), f"image {i} differs"
    assert bool((buf[~covered] == SENTINEL).all()), "bytes outside the destinations were written"


def test_every_good_file_whole_split_and_with_bytes_after_its_trailer_verifies():
    good = K.good_files()
    files, shapes, imgs = [d for _, d, _ in good], [img.shape for _, _, img in good], [img for _, _, img in good]
    assert any(len(bytes(p)) > T for f in files for p in png._walk(f, False)[3]), "one chunk must be longer than a tile"
    plain, offsets, status0 = _decode_slots(_decoder(()), files, shapes)
    for verify in (True, ("adler32",), ("crc32",)):
        buf, offsets, status = _decode_slots(_decoder(verify), files, shapes)
        assert status == [OK] * len(files) == status0, [good[i][0] for i, s in enumerate(status) if s]
        _check_slots(buf, offsets, shapes, imgs)
        assert np.array_equal(buf, plain)


def test_corrupted_files_between_good_neighbours_end_in_their_status_and_touch_nothing():
    bad, near = K.corrupted_files(), K.neighbours()
    files, shapes, want_both, want_adler, st_both, st_adler, st_plain, want_plain = [], [], [], [], [], [], [], []
    for i, (name, data, both, adler, img, stream) in enumerate(bad):
        files += [data, near[i % 2][0]]
        shapes += [K.CORRUPT_SIZE] * 2
        want_both += [img if both == "TT_PNG_OK" else None, near[i % 2][1]]
        want_adler += [img if adler == "TT_PNG_OK" else None, near[i % 2][1]]
        st_both += [K.STATUS[both], OK]
        st_adler += [K.STATUS[adler], OK]
    for verify, st, want in ((True, st_both, want_both), (("adler32",), st_adler, want_adler)):
        buf, offsets, status = _decode_slots(_decoder(verify), files, shapes)
        assert status == st, verify
        _check_slots(buf, offsets, shapes, want)
    # the gap being closed: zlib refuses stream (a), the unverified decode accepts it and returns other bytes than the image's
    name, data, _, _, _, stream = bad[0]
    with pytest.raises(zlib.error, match="incorrect data check"):
        zlib.decompress(stream)
    h, w, c = K.CORRUPT_SIZE
    buf, offsets, status = _decode_slots(_decoder(()), [data, near[0][0]], [K.CORRUPT_SIZE] * 2)
    assert status == [OK, OK]
    got = buf[offsets[0]:offsets[0] + h * w * c]
    assert not np.array_equal(got, P.image(h, w, c).reshape(-1)) and np.array_equal(buf[offsets[1]:offsets[1] + h * w * c], near[0][1].reshape(-1))
    # check=True names the two new statuses
    with pytest.raises(png.PngDecodeError) as e:
        _decoder(True).decode(files)
    assert e.value.failed == [(i, png.STATUS_NAMES[s]) for i, s in enumerate(st_both) if s]
    assert "TT_PNGV_BAD_ADLER32" in str(e.value) and "TT_PNGV_BAD_CRC32" in str(e.value)


def test_every_malformed_stream_keeps_its_status_under_verification():
    mal = P.malformed_cases()
    near = K.neighbours()[0]
    files, shapes, expected = [], [], []
    for name, stream, status in mal:
        files += [P.png_file(P.MAL_W, P.MAL_H, P.MAL_C, stream, idat_bytes=333), near[0]]
        shapes += [(P.MAL_H, P.MAL_W, P.MAL_C), K.CORRUPT_SIZE]
        expected += [P.STATUS[status], OK]
    _, _, plain = _decode_slots(_decoder(()), files, shapes)
    buf, offsets, status = _decode_slots(_decoder(True), files, shapes)
    assert plain == expected and status == expected
    _check_slots(buf, offsets, shapes, [None, near[1]] * len(mal))


def test_a_corrupted_crc_of_a_chunk_that_is_not_idat_is_a_host_error_before_any_launch():
    h, w, c = K.CORRUPT_SIZE
    stream = P.COMPRESSORS["level6"](P.filter_rows(P.image(h, w, c), [0] * h))
    for kind in (b"IHDR", b"tEXt", b"IEND"):
        data = K.chunked_file(w, h, c, stream, [10], bad_other=kind)
        with pytest.raises(ValueError, match="CRC-32"):
            _decoder(True).decode([data])
        with pytest.raises(ValueError, match="CRC-32"):
            _decoder(("crc32",)).decode([data])
        assert np.array_equal(_decoder(("adler32",)).decode([data])[0].cpu().numpy(), P.image(h, w, c))
    with pytest.raises(ValueError, match="choose one"):
        png.PngDecoder(verify_crc=True, verify=("crc32",))
    with pytest.raises(ValueError, match="verify"):
        png.PngDecoder(verify=("md5",))
    assert png.PngDecoder(verify_crc=True, verify=("adler32",)).verify == ("adler32",) and png.PngDecoder().verify == ()


def test_flags_0_through_the_verified_entry_equals_the_plain_entry_on_a_mixed_call_and_refusals():
    mal = P.malformed_cases()[::4]
    good = P.good_cases()[::9]
    cases = [(s, P.MAL_H, P.MAL_W, P.MAL_C) for _, s, _ in mal] + [(s, h, w, c) for _, s, h, w, c, _ in good]
    dec = png.PngDecoder()
    infos = [png.PngInfo(w, h, c, s) for s, h, w, c in cases]
    offsets, pos = [], 5
    for s, h, w, c in cases:
        offsets.append(pos)
        pos += h * w * c + 5
    table, total = dec._pack(infos, offsets)
    packed = dec._stage[:total].cuda()
    n = len(cases)
    need = int(lib().tt_png_workspace_bytes(table, n))
    assert int(lib().tt_png_verify_workspace_bytes(table, n, None, 0, 0)) == need
    results = []
    for verified in (False, True):
        work = torch.full((need,), SENTINEL, dtype=torch.uint8, device="cuda")
        out = torch.full((pos,), SENTINEL, dtype=torch.uint8, device="cuda")
        status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        if verified:
            rc = lib().tt_png_decode_u8_verified(ptr(packed), total, table, ptr(packed), n, None, None, 0, 0, ptr(work), need, ptr(out), pos,
                                                 ptr(status), None)
        else:
            rc = lib().tt_png_decode_u8(ptr(packed), total, table, ptr(packed), n, ptr(work), need, ptr(out), pos, ptr(status), None)
        assert rc == 0
        torch.cuda.synchronize()
        results.append((out.cpu().numpy(), status.cpu().numpy().tolist()))
    assert np.array_equal(results[0][0], results[1][0]) and results[0][1] == results[1][1]
    assert results[0][1] == [P.STATUS[s] for _, _, s in mal] + [0] * len(good)

    # the verified entry's own refusals, before any launch: one chunk per image is the good table
    def chunks(**kw):
        t = (png.PngChunk * n)()
        for i in range(n):
            t[i].offset, t[i].bytes, t[i].crc, t[i].image = table[i].stream_offset, table[i].stream_bytes, 0, i
        for k, v in kw.items():
            setattr(t[1], k, v)
        return t

    full = int(lib().tt_png_verify_workspace_bytes(table, n, chunks(), n, 3))
    assert full > need
    work = torch.full((full,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.full((pos,), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    base = dict(host=chunks(), dev=ptr(packed), nc=n, flags=3, work_bytes=full)

    def call(**kw):
        a = dict(base, **kw)
        return lib().tt_png_decode_u8_verified(ptr(packed), total, table, ptr(packed), n, a["host"], a["dev"], a["nc"], a["flags"], ptr(work),
                                               a["work_bytes"], ptr(out), pos, ptr(status), None)

    refusals = {
        "unknown flag bit": dict(flags=4), "negative flags": dict(flags=-1), "null host chunk table": dict(host=None),
        "null device chunk table": dict(dev=None), "no chunks": dict(nc=0), "too many chunks": dict(nc=_lib.TT_PNG_MAX_CHUNKS + 1),
        "image out of range": dict(host=chunks(image=n)), "negative image": dict(host=chunks(image=-1)),
        "chunks out of image order": dict(host=chunks(image=3)), "an image without chunks": dict(host=chunks(image=0)),
        "chunk before its stream": dict(host=chunks(offset=table[1].stream_offset - 1)),
        "chunk past its stream": dict(host=chunks(bytes=table[1].stream_bytes + 1)),
        "chunks end inside the stream": dict(host=chunks(bytes=table[1].stream_bytes - 1)), "negative chunk": dict(host=chunks(bytes=-1)),
        "chunk table ends early": dict(nc=n - 1), "workspace one byte short": dict(work_bytes=full - 1),
    }
    for what, kw in refusals.items():
        assert call(**kw) < 0, what
        assert lib().tt_last_error().decode().startswith("tt_png_decode_u8"), what
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((work == SENTINEL).all()) and bool((status == -7).all())


def test_two_verified_calls_on_one_decoder_reuse_the_buffers_and_stay_correct():
    dec = png.PngDecoder(verify=True)
    good = K.good_files()
    first = [g for g in good[:40]]
    second = [g for g in good[150:] + good[:3]]
    for batch in (first, second, first):
        buf, offsets, status = _decode_slots(dec, [d for _, d, _ in batch], [img.shape for _, _, img in batch])
        assert status == [OK] * len(batch)
        _check_slots(buf, offsets, [img.shape for _, _, img in batch], [img for _, _, img in batch])
    work = dec._work
    bad = K.corrupted_files()[0]
    _, _, status = _decode_slots(dec, [bad[1], first[0][1]], [K.CORRUPT_SIZE, first[0][2].shape])
    assert status == [BAD_ADLER, OK] and dec._work is work


def test_one_full_size_sample_through_decode_sample_batch_verified():
    """Four 900 x 1600 images side by side (B = 1, T = 2, N = 1), as test_png_decode.py: 66 Adler-32 tiles per camera frame."""
    d, t, c = synth.raw_label_bytes(19, 1, 900, 1600)
    yy, xx = np.mgrid[0:900, 0:1600]
    code = ((yy * 11 + xx * 7) * 16777215 // (900 * 11 + 1600 * 7)).astype(np.uint32)
    depth = np.stack([code & 255, (code >> 8) & 255, code >> 16], axis=-1).astype(np.uint8)
    prev = synth.raw_camera_frames(3, T=1, N=1)[0, 0]
    arrays = {"prev": prev, "key": c[0], "depth": depth, "seg": t[0]}
    types = [y % 5 for y in range(900)]
    files = {k: P.write_png(a, types, compressor="level1") for k, a in arrays.items()}
    raw, depth_png, seg_png = png.PngDecoder(verify=True).decode_sample_batch([[[files["prev"]], [files["key"]]]], [[files["depth"]]],
                                                                               [[files["seg"]]])
    assert np.array_equal(raw.cpu().numpy(), np.stack([arrays["prev"], arrays["key"]])[None, :, None])
    assert np.array_equal(depth_png.cpu().numpy(), depth[None, None]) and np.array_equal(seg_png.cpu().numpy(), t[0][None, None])
