"""Segmented PNG files decoded on the device, one wave per segment (thinktwice_amd.png: PngDecoder(segments=...);
csrc/png_segments.hip: tt_png_decode_u8_segmented) against the arrays the files were made from AND against the unsegmented
decode of the same files, bit for bit.  Every stream comes from tests/png_segment_cases.py; the same cases run through the
same inflate source on the CPU under sanitizers in test_png_segments_host.py, which is where the malformed ones go first.

Shapes (png_segment_cases.py).  Odd scanline strides (163, 5, 31, 7, 2101) put every segment boundary at another alignment
against the inflate's 16-byte stores: a store wider than what a segment owns at its two ends would show as a wrong byte in a
neighbouring segment's rows, or as a difference between two runs.  40 x 700 x 3 has segments longer than the 8 KiB flush, the
4 KiB input stage, one stored block and the 32 KiB ring.  The inflate has no other size thresholds."""
import ctypes
import functools
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import png_cases as P  # noqa: E402
import png_segment_cases as S  # noqa: E402
from thinktwice_amd import _lib, png  # noqa: E402
from thinktwice_amd.ops import lib, ptr  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@functools.lru_cache(maxsize=None)
def _decoder(segments="auto", verify=()):
    return png.PngDecoder(segments=segments, verify=verify)


def _ragged(infos, gap=97, check=True, decoder=None, order=None):
    """[PngInfo] -> (uint8 buffer as numpy, [offset], statuses or None): one call, every image in its own slot of one
    sentinel-filled buffer, `gap` sentinel bytes (no multiple of 16) before, between and after the slots; order: the slots'
    order in the buffer (a permutation), default the call's."""
    sizes = [i.height * i.width * i.channels for i in infos]
    offsets, pos = [0] * len(infos), gap
    for k in (order if order is not None else range(len(infos))):
        offsets[k] = pos
        pos += sizes[k] + gap
    out = torch.full((pos,), SENTINEL, dtype=torch.uint8, device="cuda")
    status = (decoder or _decoder())._run(infos, offsets, out, out.numel(), check)
    torch.cuda.synchronize()
    return out.cpu().numpy(), offsets, (None if status is None else status.cpu().numpy())


def _check_slots(buf, offsets, infos, want):
    """want[i]: the array of image i, None where its slot must still be sentinel; everything between the slots is sentinel."""
    covered = np.zeros(buf.shape, dtype=bool)
    for i, (info, o) in enumerate(zip(infos, offsets)):
        n = info.height * info.width * info.channels
        covered[o:o + n] = True
        if want[i] is None:
            assert bool((buf[o:o + n] == SENTINEL).all()), f"image {i}: a failed image's destination was written"
        else:
            assert np.array_equal(buf[o:o + n], np.asarray(want[i]).reshape(-1)), f"image {i} differs"
    assert bool((buf[~covered] == SENTINEL).all()), "bytes outside the destinations were written"


def _files(cases):
    return [data for _, data, *_ in cases]


# ------------------------------------------------------------------------------------------------------------ bit-equality
def test_every_shape_filter_rows_and_level_equals_the_source_and_the_unsegmented_decode_twice():
    good = S.good_cases()
    files = _files(good)
    assert any(S.uses_dynamic_blocks(f) for f in files) and any(n.endswith("level0") for n, *_ in good)
    infos = _decoder()._parse(files)
    assert all(i.segments is not None for i in infos)
    assert {i.segments.rows_per_segment for i in infos} >= {1, 2, 7, 64, 37, 65, 130}
    order = np.random.default_rng(5).permutation(len(infos)).tolist()
    buf, offsets, _ = _ragged(infos, order=order)
    _check_slots(buf, offsets, infos, [img for _, _, _, _, _, img, _ in good])
    again, _, _ = _ragged(infos, order=order)
    assert np.array_equal(buf, again), "two runs differ"
    plain = _decoder("ignore")._parse(files)
    assert all(i.segments is None for i in plain)
    whole, _, _ = _ragged(plain, order=order, decoder=_decoder("ignore"))
    assert np.array_equal(buf, whole), "the segmented and the unsegmented decode of the same files differ"


@functools.lru_cache(maxsize=None)
def _full_size():
    img = P.image(900, 1600, 3, seed=2)
    img.setflags(write=False)
    return img, png.segment_png(P.write_png(img, [y % 5 for y in range(900)], compressor="level1"), 16)


def test_one_full_size_frame_in_57_segments():
    img, data = _full_size()
    assert len(png.read_segments(data).offsets) - 1 == 57
    out = _decoder().decode([data])
    assert np.array_equal(out[0].cpu().numpy(), img)
    assert torch.equal(out, _decoder("ignore").decode([data]))
    assert torch.equal(out, _decoder("require", verify=True).decode([data]))


# ----------------------------------------------------------------------------------------------------------- mixed batches
def test_segmented_and_plain_files_mixed_in_decode_and_decode_sample_batch():
    h, w = 37, 54
    rng = np.random.default_rng(12)

    def make(c, seed, rows):
        img = P.image(h, w, c, seed=seed)
        src = img if c == 3 else img[:, :, 0]
        data = P.write_png(src, P.filter_types(P.FILTERS[seed % 6], h, seed), compressor=("level6", "level0", "level9")[seed % 3])
        return src, (png.segment_png(data, rows) if rows else data)

    B, T, N = 2, 2, 2
    rgb = [[[make(3, 10 * b + 3 * t + n, (0, 7, 1, 64)[(b + t + n) % 4]) for n in range(N)] for t in range(T)] for b in range(B)]
    dep = [[make(3, 50 + 2 * b + n, (16, 0)[(b + n) % 2]) for n in range(N)] for b in range(B)]
    seg = [[make(1, 70 + 2 * b + n, (0, 2)[(b + n) % 2]) for n in range(N)] for b in range(B)]
    files = lambda nest: [[[f for _, f in t] for t in s] if isinstance(s[0], list) else [f for _, f in s] for s in nest]  # noqa: E731
    arrays = lambda nest: np.array([[[a for a, _ in t] for t in s] if isinstance(s[0], list) else [a for a, _ in s] for s in nest])  # noqa: E731
    for dec in (_decoder(), _decoder(verify=True)):
        raw, depth_png, seg_png = dec.decode_sample_batch(files(rgb), files(dep), files(seg))
        assert np.array_equal(raw.cpu().numpy(), arrays(rgb)) and np.array_equal(depth_png.cpu().numpy(), arrays(dep))
        assert np.array_equal(seg_png.cpu().numpy(), arrays(seg))
    flat = [x for s in rgb for t in s for x in t] + [x for s in dep for x in s]
    out = _decoder().decode([f for _, f in flat])
    assert np.array_equal(out.cpu().numpy(), np.array([a for a, _ in flat]))
    grey = [x for s in seg for x in s]
    assert np.array_equal(_decoder().decode([f for _, f in grey]).cpu().numpy(), np.array([a for a, _ in grey]))
    # grey and RGB, segmented and plain, in one call, the destinations in shuffled order
    both = flat + grey
    infos = _decoder()._parse([f for _, f in both])
    assert {i.segments is None for i in infos} == {True, False} and {i.channels for i in infos} == {1, 3}
    order = rng.permutation(len(infos)).tolist()
    buf, offsets, _ = _ragged(infos, order=order)
    _check_slots(buf, offsets, infos, [a for a, _ in both])
    with pytest.raises(ValueError, match="no segment index"):
        _decoder("require").decode([f for _, f in flat])


# ------------------------------------------------------------------------------------------------------------ verification
def _edit_payload(data, fn, fix_crc=True):
    """The file with fn(bytearray payload) applied to its IDAT payload (in place), written as one IDAT chunk; fix_crc=False
    keeps the CRC field of the unedited payload."""
    chunks = png._chunks(data)
    payload = bytearray(b"".join(b for k, b in chunks if k == b"IDAT"))
    crc = struct.pack(">I", zlib.crc32(bytes(payload), zlib.crc32(b"IDAT")))
    fn(payload)
    out, done = [png.SIGNATURE], False
    for k, b in chunks:
        if k != b"IDAT":
            out.append(png._chunk(k, b))
        elif not done:
            done = True
            out.append(png._chunk(k, bytes(payload)) if fix_crc else struct.pack(">I", len(payload)) + k + bytes(payload) + crc)
    return b"".join(out)


def test_verify_passes_good_files_and_names_a_flipped_literal_and_a_flipped_crc_field():
    good = [k for k in S.good_cases() if k[0].startswith(("37x54x3_", "65x4x1_paeth", "40x700x3"))]
    files = _files(good)
    for verify in (("adler32",), True):
        dec = _decoder(verify=verify)
        buf, offsets, _ = _ragged(dec._parse(files), decoder=dec)
        _check_slots(buf, offsets, dec._parse(files), [k[5] for k in good])

    name, data, h, w, c, img, lines = next(k for k in S.good_cases() if k[0] == "37x54x3_paeth_R7_level0")
    index = png.read_segments(data)

    def flip_literal(payload):                           # a stored byte of the third segment: 00, LEN, NLEN, then the row bytes
        at = index.offsets[2] + 5 + 20
        assert payload[at] == lines[2 * 7 * (1 + w * c) + 20]
        payload[at] ^= 0x40

    def nothing(payload):
        pass

    literal = _edit_payload(data, flip_literal)
    assert png.read_segments(literal) == index
    with pytest.raises(zlib.error):
        zlib.decompress(png.parse_png(literal).zlib_stream)
    flipped = bytearray(_edit_payload(data, nothing))
    at = flipped.index(b"IDAT") - 4
    n, = struct.unpack_from(">I", flipped, at)
    flipped[at + 8 + n] ^= 1                             # the first byte of the IDAT chunk's CRC field
    crc = bytes(flipped)
    others = [k for k in S.good_cases() if k[0].startswith("130x10x3_random")]
    files = [others[0][1], literal, others[1][1], crc, others[2][1]]
    want = [others[0][5], None, others[1][5], None, others[2][5]]
    dec = _decoder(verify=True)
    infos = dec._parse(files)
    buf, offsets, status = _ragged(infos, decoder=dec, check=False)
    assert status.tolist() == [0, _lib.TT_PNGV_BAD_ADLER32, 0, _lib.TT_PNGV_BAD_CRC32, 0]
    _check_slots(buf, offsets, infos, want)
    dec = _decoder(verify=("adler32",))                  # the CRC field is then nobody's: that file decodes
    infos = dec._parse(files)
    buf, offsets, status = _ragged(infos, decoder=dec, check=False)
    assert status.tolist() == [0, _lib.TT_PNGV_BAD_ADLER32, 0, 0, 0]
    _check_slots(buf, offsets, infos, [others[0][5], None, others[1][5], img, others[2][5]])
    with pytest.raises(png.PngDecodeError, match="image 1: TT_PNGV_BAD_ADLER32"):
        dec.decode([data, literal])
    buf, offsets, status = _ragged(_decoder()._parse(files), check=False)          # unverified: the flipped byte is decoded
    assert status.tolist() == [0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------- malformed indices and segments
def test_malformed_indices_and_segments_between_good_images_end_in_a_status_and_touch_nothing():
    """Error paths that must return codes.  Precondition, kept by the order of work and not by this test: the identical list,
    png_segment_cases.malformed_cases(), passes the sanitized CPU run of the same inflate source
    (tests/test_png_segments_host.py, in the CPU suite) before it is put on a device.  No sanitizer and no compiler runs here."""
    mal = S.malformed_cases()
    names = ("37x54x3_random_R7_level6", "65x4x1_paeth_R1_level6", "130x10x3_average_R64_level0", "64x2x3_up_R2_level6")
    good = [k for k in S.good_cases() if k[0] in names]
    assert len(good) == len(names)
    good_infos = _decoder()._parse(_files(good))
    infos, want, expected = [], [], []
    for i, (name, payload, h, w, c, index, status) in enumerate(mal):
        infos.append(png.PngInfo(w, h, c, payload, None, index))
        want.append(None)
        expected.append(None if status is None else P.STATUS[status])
        infos.append(good_infos[i % len(good)])
        want.append(good[i % len(good)][5])
        expected.append(0)
    for verify in ((), ("adler32",)):
        buf, offsets, status = _ragged(infos, check=False, decoder=_decoder(verify=verify))
        got = {mal[i // 2][0]: int(status[i]) for i in range(0, len(infos), 2)}
        assert all(s != 0 for s in got.values()), {n: s for n, s in got.items() if s == 0}
        forced = {m[0]: P.STATUS[m[6]] for m in mal if m[6] is not None}
        assert {n: got[n] for n in forced} == forced
        assert [int(s) for s in status[1::2]] == [0] * len(mal)
        _check_slots(buf, offsets, infos, want)
    with pytest.raises(png.PngDecodeError) as e:
        _ragged(infos, check=True)
    assert [i for i, _ in e.value.failed] == list(range(0, len(infos), 2))
    assert e.value.failed[0] == (0, "TT_PNG_BAD_DISTANCE")


def test_the_lowest_numbered_failing_segment_gives_the_status():
    """Two broken segments in one image: segment 1 a stored length mismatch, segment 2 a final block; whichever wave ends
    first, the image's status is segment 1's."""
    h, w, c = 12, 9, 3
    lines = P.filter_rows(P.image(h, w, c, seed=21), P.filter_types("random", h, 21))
    payload, offsets = S._cut(lines, 1 + w * c, 4, h, level=0)
    bad = bytearray(payload)
    bad[offsets[1] + 1] ^= 0x10
    bad[offsets[2]] |= 1
    info = png.PngInfo(w, h, c, bytes(bad), None, png.SegmentIndex(4, offsets))
    for _ in range(3):
        buf, offsets_, status = _ragged([info], check=False)
        assert status.tolist() == [P.STATUS["TT_PNG_BAD_STORED_LEN"]]
        _check_slots(buf, offsets_, [info], [None])


def test_a_stale_index_in_a_file_is_a_status_not_a_wrong_image():
    name, payload, h, w, c, index, status = next(m for m in S.malformed_cases() if m[0] == "rows_5_cut_at_4")
    body = struct.pack(f">BII{len(index.offsets)}I", 1, index.rows_per_segment, len(index.offsets) - 1, *index.offsets)
    plain = P.png_file(w, h, c, payload)
    at = plain.index(b"IDAT") - 4
    data = plain[:at] + png._chunk(b"ttSG", body) + plain[at:]
    assert png.read_segments(data) == index                              # it passes every check the host can make
    with pytest.raises(png.PngDecodeError, match="image 0: TT_PNG_OUTPUT_SHORT"):
        _decoder().decode([data])
    img = _decoder("ignore").decode([data])[0].cpu().numpy()             # the stream itself is whole
    assert np.array_equal(img, P.image(h, w, c, seed=21))


# ------------------------------------------------------------------------------------------------ the entry's refusals
def test_every_refusal_of_the_segment_table_returns_an_error_and_launches_nothing():
    h, w, c = 12, 9, 3
    stride = 1 + w * c
    img = P.image(h, w, c, seed=21)
    lines = P.filter_rows(img, P.filter_types("none", h))
    payload, offsets = S._cut(lines, stride, 4, h)
    at = [256, 1024]                                                     # two images with the same stream
    packed_host = np.zeros(4096, dtype=np.uint8)
    for a in at:
        packed_host[a:a + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    images = (png.PngImage * 2)()
    for i, im in enumerate(images):
        im.stream_offset, im.stream_bytes, im.dst_offset, im.width, im.height, im.channels = at[i], len(payload), 512 * i, w, h, c

    def table(edit=None, n=6):
        t = (png.PngSegment * max(n, 1))()
        for j in range(min(n, 6)):
            i, k = divmod(j, 3)
            t[j].offset, t[j].bytes = at[i] + offsets[k], offsets[k + 1] - offsets[k]
            t[j].image, t[j].first_row, t[j].rows = i, 4 * k, 4
        if edit:
            edit(t)
        return t

    def set_(j, **kw):
        def edit(t):
            for k, v in kw.items():
                setattr(t[j], k, v)
        return edit

    def swap(a, b):
        def edit(t):
            x = bytes(t[a])
            ctypes.memmove(ctypes.byref(t[a]), ctypes.byref(t[b]), ctypes.sizeof(t[a]))
            ctypes.memmove(ctypes.byref(t[b]), x, len(x))
        return edit

    good = table()
    packed_host[:80] = np.frombuffer(images, dtype=np.uint8)
    packed_host[2048:2048 + ctypes.sizeof(good)] = np.frombuffer(good, dtype=np.uint8)
    packed = torch.from_numpy(packed_host).cuda()
    need = int(lib().tt_png_segmented_workspace_bytes(images, 2, None, 0, 0, good, 6))
    assert need == int(lib().tt_png_verify_workspace_bytes(images, 2, None, 0, 0)) + 256
    assert int(lib().tt_png_segmented_workspace_bytes(images, 2, None, 0, 1, good, 6)) == \
        int(lib().tt_png_verify_workspace_bytes(images, 2, None, 0, 1)) + 256
    assert int(lib().tt_png_segmented_workspace_bytes(images, 2, None, 0, 0, None, 0)) == need - 256
    work = torch.full((need + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    base = dict(host=good, dev=ptr(packed) + 2048, n=6, work_bytes=need)

    def call(**kw):
        a = dict(base, **kw)
        return lib().tt_png_decode_u8_segmented(ptr(packed), 4096, images, ptr(packed), 2, None, None, 0, 0, a["host"], a["dev"], a["n"],
                                                ptr(work), a["work_bytes"], ptr(out), 4096, ptr(status), None)

    last = offsets[3] - offsets[2]
    refusals = {
        "null host table": dict(host=None), "null device table": dict(dev=None), "misaligned device table": dict(dev=ptr(packed) + 2052),
        "negative count": dict(n=-1), "too many segments": dict(n=_lib.TT_PNG_MAX_SEGMENTS + 1),
        "image index out of range": dict(host=table(set_(5, image=2))), "negative image index": dict(host=table(set_(0, image=-1))),
        "images not in increasing order": dict(host=table(swap(2, 3))),
        "segments of an image not in row order": dict(host=table(swap(0, 1))),
        "first row not the next row": dict(host=table(set_(1, first_row=5))),
        "no rows": dict(host=table(set_(1, rows=0))), "rows overlap the next segment": dict(host=table(set_(1, rows=5))),
        "rows past the image": dict(host=table(set_(5, rows=5))),
        "rows short at the end of the table": dict(host=table(n=5), n=5), "rows short before the next image": dict(host=table(set_(2, rows=3))),
        "first segment not after the header": dict(host=table(set_(0, offset=at[0] + 1))),
        "a gap between segments": dict(host=table(set_(1, offset=at[0] + offsets[1] + 1))),
        "an empty segment": dict(host=table(set_(2, bytes=0))),
        "a segment into the tail": dict(host=table(set_(2, bytes=last + 1))),
        "a segment of another image's stream": dict(host=table(set_(3, offset=at[0] + 2))),
        "workspace one byte short": dict(work_bytes=need - 1),
    }
    for what, kw in refusals.items():
        assert call(**kw) < 0, what
        assert lib().tt_last_error().decode().startswith("tt_png_decode_u8"), what
        if "host" in kw and kw["host"] is not None:
            assert int(lib().tt_png_segmented_workspace_bytes(images, 2, None, 0, 0, kw["host"], kw.get("n", 6))) == 0, what
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((work == SENTINEL).all()) and bool((status == -7).all())
    assert call() == 0                                                   # the same arguments, unspoilt, decode
    torch.cuda.synchronize()
    assert status[:2].tolist() == [0, 0] and bool((work[need:] == SENTINEL).all())
    for i in range(2):
        assert np.array_equal(out[512 * i:512 * i + h * w * c].cpu().numpy(), img.reshape(-1))
    assert call(n=3, host=table(n=3)) == 0                               # image 1 has no entry: its whole stream, one wave
    torch.cuda.synchronize()
    assert status[:2].tolist() == [0, 0]
