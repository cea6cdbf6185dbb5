"""Every case of the checksum tests is made here (test_png_checksum.py on the device, test_png_checksum_host.py with
tools/png_checksum_host_check.cpp and test_png_checksum_cases.py on the CPU): byte ranges for the op (tt_checksum_ranges_u8),
and PNG files whose checksums are wrong while deflate's own rules and the output size still hold, for the verified decode
(tt_png_decode_u8_verified).  Seeded; standard library and numpy only; the streams and the writer are tests/png_cases.py's.
The truth for every value is zlib.adler32, zlib.crc32 and zlib.decompress."""
import functools
import os
import re
import struct
import zlib

import numpy as np

import png_cases as P

_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "thinktwice_hip.h")
T = int(re.search(r"#define\s+TT_CHECKSUM_TILE\s+(\d+)", open(_HEADER).read()).group(1))
ADLER32, CRC32 = 0, 1                       # enum tt_checksum_kind
STATUS = dict(P.STATUS, TT_PNGV_BAD_ADLER32=11, TT_PNGV_BAD_CRC32=12)
ZLIB = {ADLER32: zlib.adler32, CRC32: zlib.crc32}
# 5552 is zlib's NMAX; 255 .. 257 surround the 256-byte slice of one lane, 4095 .. 4097 sixteen of them
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 5551, 5552, 5553, T - 1, T, T + 1, 2 * T + 3,
           5 * T + 1]
FRAME_BYTES = 900 * (1 + 1600 * 3)          # 4,320,900: one camera frame's scanlines


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def expected(kind, data, ranges, start=None):
    """[zlib's value] for every (offset, bytes) of `ranges` over the uint8 array `data`."""
    raw = data.tobytes()
    return [ZLIB[kind](raw[o:o + n], (1 if kind == ADLER32 else 0) if start is None else int(start[i])) & 0xffffffff
            for i, (o, n) in enumerate(ranges)]


def packed_ranges(lengths, gap=3):
    """One range per length, laid out one after the other with `gap` bytes between them (so that the starts fall on every
    alignment) -> (total bytes, [(offset, bytes)])."""
    ranges, pos = [], 1
    for n in lengths:
        ranges.append((pos, n))
        pos += n + gap
    return pos, ranges


def many_ranges(count=200, seed=8):
    """(total bytes, [(offset, bytes)]): `count` ranges in shuffled order, zero-length ones among them, some adjacent (one
    begins where another ends), some overlapping, lengths up to a little more than a tile."""
    rng = np.random.default_rng(seed)
    ranges, pos = [], 0
    for i in range(count):
        n = int(rng.choice([0, 1, int(rng.integers(2, 300)), int(rng.integers(300, 9000)), T + int(rng.integers(-2, 3))],
                           p=[0.15, 0.1, 0.4, 0.3, 0.05]))
        n = {50: T + 2, 120: 2 * T + 1}.get(i, n)                       # two ranges of more than one tile, whatever was drawn
        ranges.append((pos, n))
        pos += n + (0 if i % 3 else int(rng.integers(0, 20)))          # two of three ranges are adjacent to their successor
    ranges += [(ranges[5][0] + 1, ranges[5][1] + ranges[6][1] // 2)]     # one that overlaps two others
    order = rng.permutation(len(ranges))
    return pos + 1, [ranges[i] for i in order]


@functools.lru_cache(maxsize=None)
def adler_extremes():
    """[(name, uint8 array, start value)]: one whole-buffer range each."""
    ff = lambda n: np.full(n, 255, dtype=np.uint8)
    out = [(f"ff_{n}", ff(n), 1) for n in (5552, 5553, T, 3 * T + 7)]
    out.append(("ff_full_frame", ff(FRAME_BYTES), 1))
    out += [(f"zero_{n}", np.zeros(n, dtype=np.uint8), 1) for n in (1, 257, T + 1)]
    wrap = np.concatenate([ff(256), np.array([240], dtype=np.uint8)])
    assert int(wrap.sum()) == 65520 and zlib.adler32(wrap.tobytes()) & 0xffff == 0
    out.append(("sum_65520_a_wraps_to_0", wrap, 1))
    for a, b in ((65520, 65520), (65520, 0), (0, 65520)):
        out.append((f"start_a{a}_b{b}", random_bytes(T + 77, a + b), (b << 16) | a))
        out.append((f"start_a{a}_b{b}_ff", ff(5553), (b << 16) | a))
        out.append((f"start_a{a}_b{b}_empty", ff(0), (b << 16) | a))
    for _, a, _ in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------ files
def chunked_file(w, h, c, stream, cuts, crc_flip=None, ancillary=False, bad_other=None):
    """The file around `stream` with its IDAT payload cut at the byte positions `cuts` (sorted, repeats make empty chunks).
    crc_flip: index of the IDAT chunk whose CRC field gets one bit flipped.  bad_other: b"IHDR", b"tEXt" or b"IEND", the
    non-IDAT chunk whose CRC field gets one bit flipped."""
    def chunk(kind, body, flip=False):
        crc = zlib.crc32(kind + body) ^ (0x00010000 if flip else 0)
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", crc)

    out = P.png_ref.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if c == 1 else 2, 0, 0, 0), bad_other == b"IHDR")
    if ancillary or bad_other == b"tEXt":
        out += chunk(b"tEXt", b"Comment\0made by tests/png_checksum_cases.py", bad_other == b"tEXt")
    edges = [0] + list(cuts) + [len(stream)]
    assert edges == sorted(edges)
    for i in range(len(edges) - 1):
        out += chunk(b"IDAT", stream[edges[i]:edges[i + 1]], crc_flip == i)
    return out + chunk(b"IEND", b"", bad_other == b"IEND")


def split_points(n, seed):
    """Cuts of an n-byte stream: an empty chunk, two 1-byte chunks, a cut inside the four trailer bytes; for a stream of more
    than T + 8 bytes the first chunk is longer than T."""
    rng = np.random.default_rng(seed)
    lo = T + 1 if n > T + 8 else 0
    a = int(rng.integers(lo, max(n - 4, lo + 1)))
    return sorted(min(x, n) for x in (a, a, a + 1, a + 2, n - 2))


@functools.lru_cache(maxsize=None)
def good_files():
    """[(name, file bytes, uint8 [h, w, c])]: every good stream of png_cases whole in one IDAT, then cut by split_points, and
    one stream with bytes after its trailer inside the last IDAT."""
    out = []
    for i, (name, stream, h, w, c, img) in enumerate(P.good_cases()):
        out.append((name + "/whole", chunked_file(w, h, c, stream, [], ancillary=i % 3 == 0), img))
        out.append((name + "/split", chunked_file(w, h, c, stream, split_points(len(stream), i)), img))
    name, stream, h, w, c, img = P.good_cases()[7]
    tail = stream + b"\xab\xcd\xef\x01\x02"
    assert zlib.decompressobj().decompress(tail) == zlib.decompress(stream)
    out.append((name + "/bytes_after_trailer", chunked_file(w, h, c, tail, [len(stream) - 1]), img))
    return out


CORRUPT_SIZE = (37, 53, 3)                  # of png_cases.SIZES


def _stored(seed=0):
    h, w, c = CORRUPT_SIZE
    img = P.image(h, w, c, seed=seed)
    raw = P.filter_rows(img, P.filter_types("random", h, seed))
    stream = P.COMPRESSORS["level0"](raw)
    assert len(raw) < 65535 and stream[2] == 1 and stream[7:7 + len(raw)] == raw          # one final stored block
    return img, raw, stream


@functools.lru_cache(maxsize=None)
def corrupted_files():
    """[(name, file bytes, status name with both checks on, status name with Adler-32 only, image or None, stream)]: the image
    is what a decode that ends in TT_PNG_OK must give."""
    h, w, c = CORRUPT_SIZE
    img, raw, stream = _stored()
    row = 1 + w * c
    k = 11 * row + 17                        # a literal that is no filter byte
    assert k % row != 0
    flipped = bytearray(stream)
    flipped[7 + k] ^= 0x10
    flipped = bytes(flipped)
    out = [("a_stored_literal_flipped_crc_repaired", chunked_file(w, h, c, flipped, []), "TT_PNGV_BAD_ADLER32", "TT_PNGV_BAD_ADLER32",
            None, flipped)]
    for i in range(4):
        s = bytearray(stream)
        s[len(s) - 4 + i] ^= 1 << (2 * i)
        out.append((f"b_trailer_byte_{i}_flipped_crc_repaired", chunked_file(w, h, c, bytes(s), [len(s) - 2] if i % 2 else []),
                    "TT_PNGV_BAD_ADLER32", "TT_PNGV_BAD_ADLER32", None, bytes(s)))
    good = P.COMPRESSORS["level6"](raw)
    cuts = [len(good) // 4, len(good) // 2, 3 * len(good) // 4]
    for which, idx in (("first", 0), ("middle", 2), ("last", 3)):
        out.append((f"c_crc_field_of_{which}_idat_flipped", chunked_file(w, h, c, good, cuts, crc_flip=idx), "TT_PNGV_BAD_CRC32",
                    "TT_PNG_OK", img, good))
    plain = P.png_file(w, h, c, flipped)
    broken = bytearray(chunked_file(w, h, c, stream, []))
    at = broken.index(b"IDAT") + 4 + 7 + k
    broken[at] ^= 0x10                       # the same literal, the chunk's CRC field left as it was
    assert bytes(broken) != plain and len(broken) == len(plain)
    out.append(("d_stored_literal_flipped_crc_not_repaired", bytes(broken), "TT_PNGV_BAD_CRC32", "TT_PNGV_BAD_ADLER32", None, flipped))
    return out


def neighbours():
    """Two good files of CORRUPT_SIZE to decode in the same call: [(file bytes, image)]."""
    h, w, c = CORRUPT_SIZE
    out = []
    for seed, comp in ((21, "level6"), (22, "fixed")):
        img = P.image(h, w, c, seed=seed)
        out.append((P.write_png(img, P.filter_types("random", h, seed), compressor=comp, idat_bytes=700), img))
    return out


# ------------------------------------------------------------------------------------- the case file of the host checker
def write_case_file(path):
    """Every case for tools/png_checksum_host_check.cpp, little-endian: "TTCKSC01", int32 count; per case int32 name length,
    name, int32 type.  Type 0, ranges: int32 kind, int64 buffer bytes, buffer, int32 ranges; per range int64 offset, int64
    bytes, uint32 start, uint32 expected.  Type 1, a file's stream: int32 h, w, c, expected status (both checks on), int64
    stream bytes, stream, int32 chunks; per chunk int64 bytes, uint32 CRC field.  Returns the count."""
    cases = []

    def ranges_case(name, kind, data, ranges, start=None):
        want = expected(kind, data, ranges, start)
        body = struct.pack("<iq", kind, len(data)) + data.tobytes() + struct.pack("<i", len(ranges))
        for i, (o, n) in enumerate(ranges):
            s = (1 if kind == ADLER32 else 0) if start is None else int(start[i])
            body += struct.pack("<qqII", o, n, s, want[i])
        cases.append((name, 0, body))

    total, ranges = packed_ranges(LENGTHS)
    data = random_bytes(total, 1)
    rng = np.random.default_rng(2)
    for kind, what in ((ADLER32, "adler32"), (CRC32, "crc32")):
        ranges_case(f"{what}_lengths", kind, data, ranges)
        ranges_case(f"{what}_lengths_random_start", kind, data, ranges, rng.integers(0, 1 << 32, len(ranges), dtype=np.uint64))
        total_m, many = many_ranges()
        ranges_case(f"{what}_many_ranges", kind, random_bytes(total_m, 3), many)
        for fill in (0, 255):
            ranges_case(f"{what}_all_{fill}", kind, np.full(T + 1, fill, dtype=np.uint8), [(0, T + 1), (0, 0), (1, T)])
    for name, a, start in adler_extremes():
        ranges_case("adler32_" + name, ADLER32, a, [(0, len(a))], [start])

    def stream_case(name, data, status):
        crcs = []
        from thinktwice_amd import png
        w, h, c, parts = png._walk(data, False, crcs)
        body = struct.pack("<iiii", h, w, c, STATUS[status])
        stream = b"".join(bytes(p) for p in parts)
        body += struct.pack("<q", len(stream)) + stream + struct.pack("<i", len(parts))
        for p, crc in zip(parts, crcs):
            body += struct.pack("<qI", len(p), crc)
        cases.append((name, 1, body))

    for name, data, _ in good_files():
        stream_case("good_" + name, data, "TT_PNG_OK")
    for name, data, both, _, _, _ in corrupted_files():
        stream_case("corrupt_" + name, data, both)
    h, w, c = P.MAL_H, P.MAL_W, P.MAL_C
    for name, stream, status in P.malformed_cases():
        stream_case("malformed_" + name, P.png_file(w, h, c, stream, idat_bytes=333), status)
    with open(path, "wb") as f:
        f.write(b"TTCKSC01" + struct.pack("<i", len(cases)))
        for name, kind, body in cases:
            nm = name.encode()
            f.write(struct.pack("<i", len(nm)) + nm + struct.pack("<i", kind) + body)
    return len(cases)
