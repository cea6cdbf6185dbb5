"""Every segmented stream the segment tests use (test_png_segments_cpu.py, test_png_segments_host.py with
tools/png_segment_host_check.cpp, test_png_segments.py): png.segment_png over the files of tests/png_cases.py, and the
malformed list -- indices that do not fit their stream and streams that are not what an index promises -- each with the
status it must end in, or None where the format does not force one code.  Standard library, numpy and thinktwice_amd.png's
host functions only.

Shapes.  A segment's rows start at first_row * (1 + W * C) of the image's scanlines; 163, 5, 31 and 7 are odd strides, so with
R = 1 every boundary of (37, 54, 3), (65, 4, 1), (130, 10, 3) and (64, 2, 3) is misaligned against the 16-byte stores of the
inflate, and so is every second one at any other R.  (1, 1) and (5, 1) are one segment of one row and five of a few bytes.
R = 64 and R = H are one segment for all but 65 and 130 rows; R = 7 leaves a short last segment."""
import functools
import struct
import zlib

import numpy as np

import png_cases as P
from thinktwice_amd import png

SHAPES = [(37, 54, 3), (65, 4, 1), (130, 10, 3), (64, 2, 3), (1, 1, 1), (1, 1, 3), (5, 1, 1), (5, 1, 3)]
ROWS = [1, 2, 7, 64, "H"]
LEVELS = {"level0": 0, "level6": 6}                      # stored blocks; Huffman blocks (dynamic for all but the smallest)
MARKER = b"\x00\x00\xff\xff"


def lines_of(img, types):
    a = img[:, :, None] if img.ndim == 2 else img
    return P.filter_rows(a, types)


def payload_of(data):
    return png.parse_png(data).zlib_stream


# ------------------------------------------------------------------------------------------------------------ good cases
@functools.lru_cache(maxsize=None)
def good_cases():
    """[(name, segmented file, h, w, c, uint8 [h, w, c], the filtered scanlines)]: every shape x filter x R x level."""
    out = []
    for h, w, c in SHAPES:
        img = P.image(h, w, c, seed=3)
        for f in P.FILTERS:
            types = P.filter_types(f, h, 3)
            plain = P.write_png(img if c == 3 else img[:, :, 0], types, idat_bytes=(100, 65536)[len(out) % 2], ancillary=bool(len(out) % 3))
            for r in ROWS:
                for level_name, level in LEVELS.items():
                    rows = h if r == "H" else r
                    out.append((f"{h}x{w}x{c}_{f}_R{r}_{level_name}", png.segment_png(plain, rows, level, idat_bytes=(77, 65536)[len(out) % 2]),
                                h, w, c, img, lines_of(img, types)))
    # segments longer than the inflate's 8 KiB flush and its 4 KiB input stage, at an odd stride (2101): 7 rows are 14,707
    # bytes and 33 rows 69,333 (more than one 65,535-byte stored block, more than the 32 KiB ring)
    h, w, c = 40, 700, 3
    img = P.image(h, w, c, seed=8)
    types = P.filter_types("random", h, 8)
    plain = P.write_png(img, types)
    for rows in (7, 33):
        for level_name, level in LEVELS.items():
            out.append((f"{h}x{w}x{c}_random_R{rows}_{level_name}", png.segment_png(plain, rows, level), h, w, c, img, lines_of(img, types)))
    for case in out:
        case[5].setflags(write=False)
    return out


def uses_dynamic_blocks(data):
    """Some segment of the file opens with a dynamic Huffman block (BTYPE 2)."""
    payload, index = payload_of(data), png.read_segments(data)
    return any((payload[o] >> 1) & 3 == 2 for o in index.offsets[:-1])


# ------------------------------------------------------------------------------------------------------ malformed cases
def _cut(lines, stride, rows, h, level=6, flush=zlib.Z_FULL_FLUSH):
    """The scanlines as one zlib stream with `flush` after every `rows` rows -> (payload, offsets)."""
    co = zlib.compressobj(level, zlib.DEFLATED, 15)
    pieces, offsets, total = [], [], 0
    for row in range(0, h, rows):
        piece = co.compress(lines[row * stride:(row + rows) * stride]) + co.flush(flush)
        offsets.append(total + (2 if row == 0 else 0))
        pieces.append(piece)
        total += len(piece)
    offsets.append(total)
    return b"".join(pieces) + co.flush(zlib.Z_FINISH), tuple(offsets)


def inflates_alone(payload, a, b, want):
    """zlib's own verdict on a segment: bytes [a, b) as a raw deflate stream give exactly `want`."""
    d = zlib.decompressobj(-15)
    try:
        return d.decompress(payload[a:b]) == want
    except zlib.error:
        return False


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """[(name, payload, h, w, c, png.SegmentIndex, status name or None)]: one image each.  None: not TT_PNG_OK, the code is
    not forced by the format."""
    out = []
    h, w, c = 24, 21, 3                                  # stride 64: repetitive rows put every match one row back
    stride = 1 + w * c
    row = bytes([0]) + bytes((7 * i) & 255 for i in range(w * c))
    lines = row * h
    payload, offsets = _cut(lines, stride, 4, h, flush=zlib.Z_SYNC_FLUSH)
    assert zlib.decompress(payload) == lines
    assert inflates_alone(payload, offsets[0], offsets[1], lines[:4 * stride])
    assert not any(inflates_alone(payload, offsets[i], offsets[i + 1], lines[:4 * stride]) for i in range(1, len(offsets) - 1)), \
        "after a sync flush the later segments must reach back before their start"
    out.append(("cut_at_sync_flush", payload, h, w, c, png.SegmentIndex(4, offsets), "TT_PNG_BAD_DISTANCE"))

    h, w, c = 12, 9, 3                                   # stride 28
    stride = 1 + w * c
    img = P.image(h, w, c, seed=21)
    lines = P.filter_rows(img, P.filter_types("random", h, 21))
    payload, offsets = _cut(lines, stride, 4, h)
    good = png.SegmentIndex(4, offsets)
    for i in range(3):
        assert inflates_alone(payload, offsets[i], offsets[i + 1], lines[4 * i * stride:4 * (i + 1) * stride])
    out.append(("offset_one_byte_late", payload, h, w, c, png.SegmentIndex(4, (offsets[0], offsets[1] + 1) + offsets[2:]), None))
    out.append(("offset_one_byte_early", payload, h, w, c, png.SegmentIndex(4, offsets[:2] + (offsets[2] - 1,) + offsets[3:]), None))
    out.append(("rows_5_cut_at_4", payload, h, w, c, png.SegmentIndex(5, offsets), "TT_PNG_OUTPUT_SHORT"))
    p5, o5 = _cut(lines, stride, 5, h)
    out.append(("rows_4_cut_at_5", p5, h, w, c, png.SegmentIndex(4, o5), "TT_PNG_OUTPUT_OVERRUN"))
    final = bytearray(payload)
    final[offsets[1]] |= 1                               # BFINAL of the second segment's first block
    out.append(("final_block_inside_a_segment", bytes(final), h, w, c, good, "TT_PNG_BAD_BLOCK_TYPE"))
    assert payload[offsets[2] - 4:offsets[2]] == MARKER
    short = payload[:offsets[2] - 4] + payload[offsets[2]:]
    out.append(("cut_before_its_marker", short, h, w, c, png.SegmentIndex(4, offsets[:2] + tuple(o - 4 for o in offsets[2:])),
                "TT_PNG_TRUNCATED"))
    stored, so = _cut(lines, stride, 4, h, level=0)
    bad = bytearray(stored)
    bad[so[1] + 1] ^= 0x10                               # LEN of the second segment's stored block, NLEN as it was
    out.append(("stored_len_in_a_segment", bytes(bad), h, w, c, png.SegmentIndex(4, so), "TT_PNG_BAD_STORED_LEN"))
    for name, stream, _ in P.malformed_cases():          # each as the single segment of an image, behind its own two header bytes
        tail = b"\x03\x00" + struct.pack(">I", 1)
        out.append((f"single_segment_{name}", stream + tail, P.MAL_H, P.MAL_W, P.MAL_C, png.SegmentIndex(P.MAL_H, (2, len(stream))), None))
    return out


def window_of(payload):
    return 1 << ((payload[0] >> 4) + 8) if (payload[0] >> 4) <= 7 else 32768


# ------------------------------------------------------------------------------------- the case file of the host checker
def write_case_file(path):
    """Every good and malformed case for tools/png_segment_host_check.cpp, little-endian: "TTPNGS01", int32 count; per case
    int32 name length, name, int32 h, w, c, expected status (-1: any but 0), window, number of segments, int64 payload
    length, payload, per segment int64 offset, bytes and int32 first row, rows, then int64 length and bytes of the expected
    scanlines (good cases only)."""
    cases = []
    for name, data, h, w, c, _, lines in good_cases():
        cases.append((name, payload_of(data), h, w, c, png.read_segments(data), 0, lines))
    for name, payload, h, w, c, index, status in malformed_cases():
        cases.append((name, payload, h, w, c, index, -1 if status is None else P.STATUS[status], b""))
    with open(path, "wb") as f:
        f.write(b"TTPNGS01" + struct.pack("<i", len(cases)))
        for name, payload, h, w, c, index, status, lines in cases:
            nm, (rows, offsets) = name.encode(), index
            n = len(offsets) - 1
            f.write(struct.pack("<i", len(nm)) + nm + struct.pack("<iiiiii", h, w, c, status, window_of(payload), n))
            f.write(struct.pack("<q", len(payload)) + payload)
            for k in range(n):
                f.write(struct.pack("<qqii", offsets[k], offsets[k + 1] - offsets[k], k * rows, min(rows, h - k * rows)))
            f.write(struct.pack("<q", len(lines)) + lines)
    return len(cases)
