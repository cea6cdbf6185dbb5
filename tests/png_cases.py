"""Every stream the PNG tests use is made here (test_png_ref.py, test_png_host.py with tools/png_host_check.cpp,
test_png_decode.py): a PNG writer with forced per-row filter types, a chosen compressor and IDAT chunk size; hand-assembled
fixed-Huffman blocks for what zlib never emits; and the malformed list, each with the status it must end in.  Standard
library and numpy only.

Hand-assembled streams hold only bytes 0..4, so that every byte is a valid filter type wherever the rows fall; their image is
whatever the restatement's unfilter makes of them (png_ref.unfilter), their truth is the scanline bytes the assembler tracked."""
import functools
import struct
import zlib

import numpy as np

import png_ref

# include/thinktwice_hip.h, enum tt_png_status (test_png_ref.py checks the two against each other)
STATUS = {"TT_PNG_OK": 0, "TT_PNG_TRUNCATED": 1, "TT_PNG_BAD_ZLIB_HEADER": 2, "TT_PNG_BAD_BLOCK_TYPE": 3,
          "TT_PNG_BAD_STORED_LEN": 4, "TT_PNG_BAD_CODE_LENGTHS": 5, "TT_PNG_BAD_SYMBOL": 6, "TT_PNG_BAD_DISTANCE": 7,
          "TT_PNG_OUTPUT_OVERRUN": 8, "TT_PNG_OUTPUT_SHORT": 9, "TT_PNG_BAD_FILTER": 10}

# 64 x 3, 65 x 3 and 130 x 9: none, one and two hand-overs between the 64-row bands of the unfilter's wavefront
SIZES = [(1, 1), (1, 7), (5, 1), (64, 3), (65, 3), (130, 9), (37, 53)]
FILTERS = ["none", "sub", "up", "average", "paeth", "random"]


# ------------------------------------------------------------------------------------------------------------- the writer
def image(h, w, c, seed=0):
    """uint8 [h, w, c]: a ramp, flat patches and some noise, so that a compressor finds literals, short and long matches."""
    rng = np.random.default_rng(1000003 * seed + 1009 * h + 17 * w + c)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(3 * yy + 5 * xx + 40 * k) & 255 for k in range(c)], axis=-1).astype(np.uint8)
    noise = rng.random((h, w)) < 0.3
    img[noise] = rng.integers(0, 256, (int(noise.sum()), c), dtype=np.uint8)
    if h > 4 and w > 4:
        img[h // 3:h // 3 + max(h // 4, 1), w // 4:w // 4 + max(w // 2, 1)] = 200
    return img


def filter_types(name, h, seed=0):
    if name == "random":
        return np.random.default_rng(77 + seed + h).integers(0, 5, h).tolist()
    return [FILTERS.index(name)] * h


def filter_rows(img, types):
    """uint8 [h, w, c] under one filter type per row -> the filtered scanlines, bytes."""
    h, w, c = img.shape
    x = img.astype(np.int64)
    out = np.zeros((h, 1 + w * c), dtype=np.uint8)
    for y in range(h):
        row = x[y]
        b = x[y - 1] if y else np.zeros((w, c), dtype=np.int64)
        a = np.concatenate([np.zeros((1, c), dtype=np.int64), row[:-1]])
        cc = np.concatenate([np.zeros((1, c), dtype=np.int64), b[:-1]])
        ft = types[y]
        pred = [0, a, b, (a + b) >> 1, png_ref.paeth(a, b, cc)][ft] if ft else 0
        out[y, 0] = ft
        out[y, 1:] = ((row - pred) & 255).reshape(-1)
    return out.tobytes()


def _deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return co.compress(raw) + co.flush()


def _with_flushes(raw):
    """A full flush and a sync flush in the middle: empty stored blocks, the reader realigned to a byte."""
    co = zlib.compressobj(6)
    a, b = len(raw) // 3, 2 * len(raw) // 3
    return (co.compress(raw[:a]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[a:b]) + co.flush(zlib.Z_SYNC_FLUSH)
            + co.compress(raw[b:]) + co.flush())


COMPRESSORS = {
    "level0": lambda r: _deflate(r, 0),
    "level1": lambda r: _deflate(r, 1),
    "level6": lambda r: _deflate(r, 6),
    "level9": lambda r: _deflate(r, 9),
    "fixed": lambda r: _deflate(r, 6, zlib.Z_FIXED),
    "rle": lambda r: _deflate(r, 6, zlib.Z_RLE),
    "huffman_only": lambda r: _deflate(r, 6, zlib.Z_HUFFMAN_ONLY),
    "wbits9": lambda r: _deflate(r, 6, wbits=9),
    "flushes": _with_flushes,
}


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png_file(w, h, c, stream, idat_bytes=65536, ancillary=False, depth=8, colour=None, interlace=0):
    """The file around a zlib stream: IHDR, an optional tEXt chunk, the stream cut into IDAT chunks of `idat_bytes`, IEND."""
    colour = (0 if c == 1 else 2) if colour is None else colour
    out = png_ref.SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))
    if ancillary:
        out += _chunk(b"tEXt", b"Comment\0made by tests/png_cases.py")
    for i in range(0, max(len(stream), 1), idat_bytes):
        out += _chunk(b"IDAT", stream[i:i + idat_bytes])
    return out + _chunk(b"IEND", b"")


def write_png(img, types=None, compressor="level6", idat_bytes=65536, ancillary=False):
    """uint8 [h, w] or [h, w, c] -> file bytes, under forced filter types (default: None on every row)."""
    a = img[:, :, None] if img.ndim == 2 else img
    h, w, c = a.shape
    return png_file(w, h, c, COMPRESSORS[compressor](filter_rows(a, types or [0] * h)), idat_bytes, ancillary)


# ----------------------------------------------------------------------------------------------------- the bit assembler
class Bits:
    """deflate's bit order: fields from the least significant bit of each byte, Huffman codes most significant bit first."""

    def __init__(self):
        self.out, self.acc, self.k = bytearray(), 0, 0

    @property
    def n(self):
        return 8 * len(self.out) + self.k

    def field(self, value, bits):
        self.acc |= value << self.k
        self.k += bits
        while self.k >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.k -= 8

    def code(self, value, bits):
        self.field(int(format(value, f"0{bits}b")[::-1], 2), bits)

    def copy(self):
        b = Bits()
        b.out, b.acc, b.k = bytearray(self.out), self.acc, self.k
        return b

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.k else b"")


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
          8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class FixedBlock:
    """One final fixed-Huffman block inside a zlib wrapper, assembled symbol by symbol; `raw` is what it inflates to."""

    def __init__(self, header=b"\x78\x9c"):
        self.header, self.bits, self.raw = header, Bits(), bytearray()
        self.bits.field(1, 1)
        self.bits.field(1, 2)

    def litlen(self, sym):
        if sym < 144:
            self.bits.code(0x30 + sym, 8)
        elif sym < 256:
            self.bits.code(0x190 + sym - 144, 9)
        elif sym < 280:
            self.bits.code(sym - 256, 7)
        else:
            self.bits.code(0xC0 + sym - 280, 8)

    def lit(self, data):
        for b in data:
            self.litlen(b)
        self.raw += bytes(data)

    def match(self, length, dist, length_sym=None, dist_sym=None):
        ls = max(i for i in range(29) if _LBASE[i] <= length) if length_sym is None else length_sym
        self.litlen(257 + ls)
        self.bits.field(length - _LBASE[ls], _LEXT[ls])
        ds = max(i for i in range(30) if _DBASE[i] <= dist) if dist_sym is None else dist_sym
        self.bits.code(ds, 5)
        self.after_dist_code = self.bits.n
        self.bits.field(dist - _DBASE[ds], _DEXT[ds])
        for i in range(length):
            self.raw.append(self.raw[len(self.raw) - dist] if dist <= len(self.raw) else 0)

    def stream(self, end=True):
        b = self.bits.copy()
        if end:
            b.code(0, 7)
        return self.header + b.bytes() + struct.pack(">I", zlib.adler32(bytes(self.raw)))


def _small(rng, n):
    return rng.integers(0, 5, n, dtype=np.uint8).tobytes()


def _shape_for(n, w=100):
    """(h, w, extra): a grey image of h rows of 1 + w bytes holds n bytes and `extra` more."""
    h = -(-n // (1 + w))
    return h, w, h * (1 + w) - n


def _finish(name, blk, rng, w=100):
    h, w, extra = _shape_for(len(blk.raw), w)
    blk.lit(_small(rng, extra))
    stream = blk.stream()
    assert zlib.decompress(stream) == bytes(blk.raw), name
    return name, stream, h, w, 1, bytes(blk.raw)


@functools.lru_cache(maxsize=None)
def hand_cases():
    """[(name, stream, h, w, c, scanline bytes)]: what zlib's deflate never writes."""
    rng = np.random.default_rng(321)
    out = []
    blk = FixedBlock()                                   # the farthest distance there is (deflate stops at 32,506)
    blk.lit(_small(rng, 32768))
    blk.match(258, 32768)
    blk.match(3, 32768)
    out.append(_finish("distance_32768", blk, rng))
    blk = FixedBlock()                                   # the overlap every parallel copy gets wrong first
    blk.lit(b"\x03")
    blk.match(258, 1)
    blk.lit(b"\x01\x02")
    blk.match(258, 2)
    blk.match(257, 3)
    blk.match(130, 64)
    blk.match(130, 65)
    blk.match(200, 63)
    out.append(_finish("overlapping_matches", blk, rng, w=52))
    blk = FixedBlock()                                   # first and last length of every length code
    blk.lit(_small(rng, 300))
    for ls in range(29):
        for length in {_LBASE[ls], min(_LBASE[ls] + (1 << _LEXT[ls]) - 1, 257 if ls == 27 else 258)}:
            blk.match(length, int(rng.integers(1, 300)), length_sym=ls)
            blk.lit(_small(rng, 2))
    out.append(_finish("every_length_code", blk, rng))
    blk = FixedBlock()                                   # first and last distance of every distance code
    blk.lit(_small(rng, 32768))
    for ds in range(30):
        for dist in (_DBASE[ds], _DBASE[ds] + (1 << _DEXT[ds]) - 1):
            blk.match(int(rng.integers(3, 12)), dist, dist_sym=ds)
            blk.lit(_small(rng, 1))
    out.append(_finish("every_distance_code", blk, rng))
    return out


# ----------------------------------------------------------------------------------------------------------- good cases
@functools.lru_cache(maxsize=None)
def good_cases():
    """[(name, stream, h, w, c, uint8 [h, w, c])]: every size x channels x filter at level 6, every compressor, every
    hand-assembled stream.  The arrays are read-only."""
    out = []
    for h, w in SIZES:
        for c in (1, 3):
            img = image(h, w, c)
            for f in FILTERS:
                out.append((f"{h}x{w}x{c}_{f}", COMPRESSORS["level6"](filter_rows(img, filter_types(f, h))), h, w, c, img))
    for name in COMPRESSORS:
        h, w, c = (150, 150, 3) if name == "level0" else (37, 53, 3)          # level 0: more than one 65,535-byte stored block
        img = image(h, w, c, seed=5)
        out.append((f"compressor_{name}", COMPRESSORS[name](filter_rows(img, filter_types("random", h, 5))), h, w, c, img))
    flat = np.full((40, 300, 1), 7, dtype=np.uint8)                           # a label map: length-258 matches at distance 1
    out.append(("flat_label_map", COMPRESSORS["level6"](filter_rows(flat, [0] * 40)), 40, 300, 1, flat))
    for name, stream, h, w, c, raw in hand_cases():
        out.append((f"hand_{name}", stream, h, w, c, png_ref.unfilter(raw, h, w, c)))
    for case in out:
        case[5].setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------ malformed cases
MAL_H, MAL_W, MAL_C = 24, 40, 3                          # the image every malformed stream claims to be


def _dynamic_header(code_lengths, symbols, tail_bits=64):
    """zlib header + a final dynamic block header: HLIT = HDIST = 0, the 19 code-length code lengths given by symbol, then
    `symbols` as (code, bits) pairs, then zero bits."""
    b = Bits()
    b.field(1, 1)
    b.field(2, 2)
    b.field(0, 5)
    b.field(0, 5)
    b.field(15, 4)
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        b.field(code_lengths.get(s, 0), 3)
    for code, bits in symbols:
        b.code(code, bits)
    b.field(0, tail_bits)
    return b"\x78\x9c" + b.bytes()


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """[(name, stream, status name)], every stream at least 6 bytes, for an image of MAL_H x MAL_W x MAL_C."""
    rng = np.random.default_rng(99)
    img = image(MAL_H, MAL_W, MAL_C, seed=9)
    raw = filter_rows(img, filter_types("random", MAL_H, 9))
    n = len(raw)
    good = COMPRESSORS["level9"](raw)
    out = []

    def no_output_yet(cut):                              # the cut falls inside the first block's header
        d = zlib.decompressobj()
        return d.decompress(good[:cut]) == b"" and not d.eof

    assert (good[2] >> 1) & 3 == 2 and no_output_yet(6) and no_output_yet(16), "the base stream must open with a dynamic block"
    out.append(("cut_in_block_header", good[:6], "TT_PNG_TRUNCATED"))
    out.append(("cut_in_code_length_run", good[:16], "TT_PNG_TRUNCATED"))
    out.append(("cut_in_symbols", good[:len(good) // 2], "TT_PNG_TRUNCATED"))
    out.append(("cut_in_adler32", good[:-2], "TT_PNG_TRUNCATED"))
    out.append(("cut_before_adler32", good[:-4], "TT_PNG_TRUNCATED"))
    blk = FixedBlock()
    blk.lit(_small(rng, 20))
    out.append(("cut_in_literal", blk.stream(end=False)[:2 + 9], "TT_PNG_TRUNCATED"))      # byte edges fall inside 8-bit codes
    blk = FixedBlock()
    blk.lit(_small(rng, 600))
    blk.match(240, 513 + 100)                            # 5 extra length bits, 8 extra distance bits
    cut = 2 + (blk.after_dist_code + 7) // 8
    assert blk.after_dist_code < 8 * (cut - 2) < blk.bits.n
    out.append(("cut_in_extra_bits", blk.stream(end=False)[:cut], "TT_PNG_TRUNCATED"))
    stored = COMPRESSORS["level0"](raw)
    out.append(("cut_in_stored_bytes", stored[:100], "TT_PNG_TRUNCATED"))

    def zlib_header(cmf, fdict=0):                       # with a valid FCHECK
        flg = fdict << 5
        return bytes([cmf, flg + (31 - ((cmf << 8) + flg) % 31) % 31])

    assert zlib_header(0x78) == b"\x78\x01"
    out.append(("zlib_method_7", zlib_header(0x77) + good[2:], "TT_PNG_BAD_ZLIB_HEADER"))
    out.append(("zlib_fcheck", b"\x78\x9d" + good[2:], "TT_PNG_BAD_ZLIB_HEADER"))
    out.append(("zlib_preset_dictionary", zlib_header(0x78, 1) + good[2:], "TT_PNG_BAD_ZLIB_HEADER"))
    out.append(("zlib_window_64k", zlib_header(0x88) + good[2:], "TT_PNG_BAD_ZLIB_HEADER"))
    out.append(("block_type_3", b"\x78\x9c\x07" + bytes(8), "TT_PNG_BAD_BLOCK_TYPE"))
    out.append(("stored_len_mismatch", b"\x78\x01\x01\x05\x00\x00\x00" + bytes(9), "TT_PNG_BAD_STORED_LEN"))
    out.append(("oversubscribed_code_length_code", _dynamic_header({s: 1 for s in range(19)}, []), "TT_PNG_BAD_CODE_LENGTHS"))
    # code-length code {1: '0', 18: '1'}: 257 literal/length codes of length 1 and one distance code
    out.append(("oversubscribed_literal_code", _dynamic_header({1: 1, 18: 1}, [(0, 1)] * 258), "TT_PNG_BAD_CODE_LENGTHS"))
    # code-length code {1: '0', 16: '1'}: the first symbol repeats a length that is not there
    out.append(("repeat_without_previous", _dynamic_header({1: 1, 16: 1}, [(1, 1)]), "TT_PNG_BAD_CODE_LENGTHS"))
    out.append(("incomplete_code_length_code", _dynamic_header({1: 1}, [(0, 1)] * 258), "TT_PNG_BAD_CODE_LENGTHS"))
    blk = FixedBlock()
    blk.lit(_small(rng, 3))
    blk.match(3, 4)
    out.append(("distance_before_start", blk.stream(), "TT_PNG_BAD_DISTANCE"))
    blk = FixedBlock(header=b"\x18\x19")                 # a 512-byte window
    blk.lit(_small(rng, 600))
    blk.match(3, 513)
    out.append(("distance_beyond_window", blk.stream(), "TT_PNG_BAD_DISTANCE"))
    for sym in (286, 287):
        blk = FixedBlock()
        blk.lit(_small(rng, 5))
        blk.litlen(sym)
        out.append((f"length_symbol_{sym}", blk.stream() + bytes(4), "TT_PNG_BAD_SYMBOL"))
    for sym in (30, 31):
        blk = FixedBlock()
        blk.lit(_small(rng, 5))
        blk.litlen(257)
        blk.bits.code(sym, 5)
        out.append((f"distance_symbol_{sym}", blk.stream() + bytes(4), "TT_PNG_BAD_SYMBOL"))
    out.append(("one_byte_long", COMPRESSORS["level6"](raw + b"\0"), "TT_PNG_OUTPUT_OVERRUN"))
    out.append(("one_byte_long_stored", COMPRESSORS["level0"](raw + b"\0"), "TT_PNG_OUTPUT_OVERRUN"))
    out.append(("one_byte_short", COMPRESSORS["level6"](raw[:-1]), "TT_PNG_OUTPUT_SHORT"))
    bad = bytearray(raw)
    bad[(MAL_H // 2) * (1 + MAL_W * MAL_C)] = 5
    out.append(("filter_type_5", COMPRESSORS["level6"](bytes(bad)), "TT_PNG_BAD_FILTER"))
    assert all(len(s) >= 6 for _, s, _ in out) and n == MAL_H * (1 + MAL_W * MAL_C)
    return out


# ------------------------------------------------------------------------------------- the case file of the host checker
def write_case_file(path):
    """Every good and malformed case for tools/png_host_check.cpp, little-endian: "TTPNGC01", int32 count; per case int32
    name length, name, int32 h, w, c, expected status, int64 stream length, stream, int64 pixel bytes, pixels (good only)."""
    cases = [(n, s, h, w, c, 0, img.tobytes()) for n, s, h, w, c, img in good_cases()]
    cases += [(n, s, MAL_H, MAL_W, MAL_C, STATUS[st], b"") for n, s, st in malformed_cases()]
    with open(path, "wb") as f:
        f.write(b"TTPNGC01" + struct.pack("<i", len(cases)))
        for name, stream, h, w, c, status, pixels in cases:
            nm = name.encode()
            f.write(struct.pack("<i", len(nm)) + nm + struct.pack("<iiii", h, w, c, status))
            f.write(struct.pack("<q", len(stream)) + stream + struct.pack("<q", len(pixels)) + pixels)
    return len(cases)
