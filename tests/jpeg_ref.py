"""A numpy restatement of the device's JPEG encoder, written from ITU-T T.81 and the arithmetic the header of
thinktwice_amd/csrc/jpeg_core.h states, not from its code: the DCT is a matrix product, the zig-zag order is generated, the
bits are strings.  Plus a minimal baseline parser and entropy decoder that reads any baseline file (its own tables, any
sampling factors), so that the restatement is held to PIL in tests/test_jpeg_ref.py and the device to the restatement.

    encode(img, quality, subsampling, restart_rows) -> bytes
    quantised_coefficients(img, quality, subsampling) -> [per component int16 (block rows, block columns, 64), zig-zag order]
    decode_coefficients(file) -> Decoded (the same arrays, the markers, the DRI value, the stuffed bytes, ...)"""
import collections

import numpy as np

# T.81 Annex K.1, K.2 (row-major)
BASE_QUANT = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32], dtype=np.int64)

# T.81 Annex K.3: (BITS, HUFFVAL) of the DC and AC tables, luminance then chrominance
_AC_LUM = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHR = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFF = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], bytes(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], bytes(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], _AC_LUM),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], _AC_CHR),
}                                                           # (class 0 DC / 1 AC, destination 0 / 1)


def zigzag_order():
    """The row-major index of every zig-zag position: anti-diagonals in turn, odd ones downwards."""
    order = sorted(((y + x, y if (y + x) % 2 else x, 8 * y + x) for y in range(8) for x in range(8)))
    return np.array([i for _, _, i in order])


ZIGZAG = zigzag_order()


def quant_tables(quality):
    """-> int64 [2, 64], row-major."""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((BASE_QUANT * s + 50) // 100, 1, 255)


def dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    t = 8192.0 * np.cos((2 * x + 1) * u * np.pi / 16)
    t[0] /= np.sqrt(2.0)
    return np.rint(t).astype(np.int64)


def canonical_codes(bits, vals):
    """-> {symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _geometry(img, subsampling):
    h, w = img.shape[:2]
    colour = img.ndim == 3 and img.shape[2] == 3
    s420 = colour and subsampling == "420"
    m = 16 if s420 else 8
    return h, w, colour, s420, m, -(-w // m), -(-h // m)


def component_planes(img, subsampling):
    """-> the component planes, int64, padded to whole MCUs by repeating the last column and row."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and subsampling in ("444", "420")
    h, w, colour, s420, m, mx, my = _geometry(img, subsampling)
    px = img.reshape(h, w, -1).astype(np.int64)
    px = np.pad(px, ((0, my * m - h), (0, mx * m - w), (0, 0)), mode="edge")
    if not colour:
        return [px[:, :, 0]]
    r, g, b = px[:, :, 0], px[:, :, 1], px[:, :, 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    if s420:
        cb, cr = [(c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2 for c in (cb, cr)]
    return [y, cb, cr]


def quantised_coefficients(img, quality, subsampling="420", restart_rows=1):
    """-> per component int16 (block rows, block columns, 64): the quantised coefficients in zig-zag order, over the picture
    padded to whole MCUs."""
    q = quant_tables(quality)
    t = dct_matrix()
    out = []
    for c, plane in enumerate(component_planes(img, subsampling)):
        by, bx = plane.shape[0] // 8, plane.shape[1] // 8
        s = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128             # [by, bx, y, x]
        p = np.einsum("ux,abyx->abyu", t, s)
        r = (p + 1024) >> 11
        f = np.einsum("vy,abyu->abvu", t, r).reshape(by, bx, 64)
        qt = q[1 if c else 0]
        v = (np.abs(f) + (qt << 16)) // (qt << 17)
        v[:, :, 1:] = np.minimum(v[:, :, 1:], 1023)
        out.append((np.sign(f) * v)[:, :, ZIGZAG].astype(np.int16))
    return out


def mcu_blocks(coefs, s420, mx, my):
    """The blocks in scan order: [my, mx, blocks per MCU, 64]."""
    if len(coefs) == 1:
        return coefs[0].reshape(my, mx, 1, 64)
    y, cb, cr = coefs
    if not s420:
        return np.stack([y, cb, cr], axis=2)
    y = y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
    return np.concatenate([y, cb[:, :, None], cr[:, :, None]], axis=2)


def _bits(code, length):
    return format(code, "0%db" % length)


def _value_bits(v):
    size = int(abs(v)).bit_length()
    return size, (_bits(v if v >= 0 else v + (1 << size) - 1, size) if size else "")


def entropy_code(blocks, tables, counts=None):
    """One restart interval: blocks [n, 64] with their component numbers `comps` folded in as (component, block) pairs ->
    the bit string.  counts: a Counter of what was coded."""
    dc, ac = tables
    pred = collections.defaultdict(int)
    out = []
    for comp, blk in blocks:
        t = 1 if comp else 0
        diff = int(blk[0]) - pred[comp]
        pred[comp] = int(blk[0])
        size, extra = _value_bits(diff)
        out.append(_bits(*dc[t][size]) + extra)
        if counts is not None:
            counts["dc%d" % size] += 1
        run = 0
        for v in blk[1:].tolist():
            if v == 0:
                run += 1
                continue
            while run >= 16:
                out.append(_bits(*ac[t][0xF0]))
                run -= 16
                if counts is not None:
                    counts["zrl"] += 1
            size, extra = _value_bits(v)
            out.append(_bits(*ac[t][(run << 4) | size]) + extra)
            if counts is not None:
                counts["ac%d" % size] += 1
            run = 0
        if run:
            out.append(_bits(*ac[t][0]))
            if counts is not None:
                counts["eob"] += 1
    return "".join(out)


def header_bytes(h, w, colour, s420, quality, dri):
    q = quant_tables(quality)
    nc = 3 if colour else 1

    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body

    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += seg(0xDB, b"".join(bytes([t]) + bytes(q[t][ZIGZAG].tolist()) for t in range(2 if colour else 1)))
    comps = b"".join(bytes([c + 1, 0x22 if (c == 0 and s420) else 0x11, 1 if c else 0]) for c in range(nc))
    out += seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc]) + comps)
    dht = b""
    for t in range(2 if colour else 1):
        for cls in (0, 1):
            bits, vals = HUFF[(cls, t)]
            dht += bytes([(cls << 4) | t]) + bytes(bits) + bytes(vals)
    out += seg(0xC4, dht)
    out += seg(0xDD, dri.to_bytes(2, "big"))
    out += seg(0xDA, bytes([nc]) + b"".join(bytes([c + 1, 0x11 if c else 0x00]) for c in range(nc)) + b"\x00\x3f\x00")
    return out


def encode(img, quality=90, subsampling="420", restart_rows=1, counts=None):
    """-> the file the device writes for these pixels and parameters.  counts: a Counter filled with what the entropy coder
    coded (dcN / acN per category, zrl, eob, stuffed, intervals)."""
    img = np.asarray(img)
    h, w, colour, s420, m, mx, my = _geometry(img, subsampling)
    assert 1 <= h <= 65535 and 1 <= w <= 65535 and restart_rows >= 1 and restart_rows * mx <= 65535
    blocks = mcu_blocks(quantised_coefficients(img, quality, subsampling), s420, mx, my)
    bpm = blocks.shape[2]
    comp_of = [0] if bpm == 1 else [0, 1, 2] if bpm == 3 else [0, 0, 0, 0, 1, 2]
    tables = ([canonical_codes(*HUFF[(0, t)]) for t in (0, 1)], [canonical_codes(*HUFF[(1, t)]) for t in (0, 1)])
    out = bytearray(header_bytes(h, w, colour, s420, quality, restart_rows * mx))
    n_int = -(-my // restart_rows)
    for k in range(n_int):
        rows = blocks[k * restart_rows:(k + 1) * restart_rows].reshape(-1, 64)
        bits = entropy_code([(comp_of[i % bpm], b) for i, b in enumerate(rows)], tables, counts)
        bits += "1" * (-len(bits) % 8)
        raw = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
        if counts is not None:
            counts["stuffed"] += raw.count(b"\xff")
            counts["intervals"] += 1
        out += raw.replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD9 if k == n_int - 1 else 0xD0 + (k & 7)])
    return bytes(out)


# ------------------------------------------------------------------------------------------------ the parser and decoder
Decoded = collections.namedtuple("Decoded", "height width components sampling qtables coefficients markers dri stuffed huffman")


class _BitReader:
    def __init__(self, data):
        self.bits = bin(int.from_bytes(b"\x01" + data, "big"))[3:]
        self.at = 0

    def take(self, n):
        v = self.bits[self.at:self.at + n]
        if len(v) < n:
            raise ValueError("the interval's bits ran out")
        self.at += n
        return int(v, 2) if n else 0

    def symbol(self, lookup):
        for length in range(1, 17):
            key = (length, self.bits[self.at:self.at + length])
            if key in lookup:
                self.at += length
                return lookup[key]
        raise ValueError("no Huffman code matches")


def _extend(v, size):
    return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1


def decode_coefficients(data):
    """A baseline (SOF0) file with one interleaved scan -> Decoded: the quantised coefficients per component, int16 (block
    rows, block columns, 64) in zig-zag order over whole MCUs; markers [(offset, marker byte)] of every marker in the file;
    dri (0 without DRI); stuffed: the FF 00 pairs of the scan; the Huffman tables as {(class, id): (bits, values)}."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    markers, at = [(0, 0xD8)], 2
    qtables, huffman, frame, dri, scan = {}, {}, None, 0, None
    while True:
        assert data[at] == 0xFF and data[at + 1] not in (0x00, 0xFF), f"no marker at {at}"
        m = data[at + 1]
        markers.append((at, m))
        n = int.from_bytes(data[at + 2:at + 4], "big")
        body = data[at + 4:at + 2 + n]
        if m == 0xDB:
            p = 0
            while p < len(body):
                assert body[p] >> 4 == 0, "16-bit quantisation table"
                qtables[body[p] & 15] = np.frombuffer(body[p + 1:p + 65], np.uint8).astype(np.int64)        # zig-zag order
                p += 65
        elif m == 0xC0:
            assert body[0] == 8
            h, w, nc = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            frame = (h, w, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nc)])
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise ValueError("not a baseline file")
        elif m == 0xC4:
            p = 0
            while p < len(body):
                bits = list(body[p + 1:p + 17])
                huffman[(body[p] >> 4, body[p] & 15)] = (bits, bytes(body[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        elif m == 0xDD:
            dri = int.from_bytes(body, "big")
        elif m == 0xDA:
            ns = body[0]
            scan = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
            assert body[1 + 2 * ns:] == b"\x00\x3f\x00", "not a sequential scan"
            at += 2 + n
            break
        at += 2 + n
    h, w, comps = frame
    assert [c[0] for c in comps] == [s[0] for s in scan], "the scan is not all components, interleaved"
    if len(comps) == 1:                                     # a scan of one component is not interleaved: its MCU is one block
        comps = [(comps[0][0], 1, 1, comps[0][3])]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    lookups = {k: {(length, format(code, "0%db" % length)): sym for sym, (code, length) in canonical_codes(*v).items()}
               for k, v in huffman.items()}
    # the scan: split at the markers, unstuff
    intervals, cur, stuffed = [], bytearray(), 0
    while True:
        nxt = data.index(b"\xff", at)
        cur += data[at:nxt]
        follow = data[nxt + 1]
        if follow == 0x00:
            cur.append(0xFF)
            stuffed += 1
            at = nxt + 2
        elif 0xD0 <= follow <= 0xD7:
            assert follow == 0xD0 + (len(intervals) & 7), f"RST{follow - 0xD0} after interval {len(intervals)}"
            markers.append((nxt, follow))
            intervals.append(bytes(cur))
            cur = bytearray()
            at = nxt + 2
        elif follow == 0xD9:
            markers.append((nxt, follow))
            intervals.append(bytes(cur))
            assert nxt + 2 == len(data), "bytes after EOI"
            break
        else:
            raise ValueError(f"marker {follow:#x} inside the scan")
    per = dri if dri else mx * my
    assert len(intervals) == -(-(mx * my) // per), (len(intervals), mx, my, per)
    coefs = [np.zeros((my * c[2], mx * c[1], 64), np.int16) for c in comps]
    for k, raw in enumerate(intervals):
        rd = _BitReader(raw)
        pred = [0] * len(comps)
        for m in range(k * per, min((k + 1) * per, mx * my)):
            for ci, (cid, ch, cv, _) in enumerate(comps):
                dc_l, ac_l = lookups[(0, scan[ci][1])], lookups[(1, scan[ci][2])]
                for j in range(cv):
                    for i in range(ch):
                        blk = coefs[ci][(m // mx) * cv + j, (m % mx) * ch + i]
                        size = rd.symbol(dc_l)
                        pred[ci] += _extend(rd.take(size), size)
                        blk[0] = pred[ci]
                        p = 1
                        while p < 64:
                            rs = rd.symbol(ac_l)
                            if rs == 0:
                                break
                            p += rs >> 4
                            if rs & 15:
                                assert p < 64, "a run past the block"
                                blk[p] = _extend(rd.take(rs & 15), rs & 15)
                            p += 1
        left = rd.bits[rd.at:]
        assert len(left) < 8 and set(left) <= {"1"}, f"interval {k}: {len(left)} bits left, not padding"
    return Decoded(h, w, len(comps), [(c[1], c[2]) for c in comps], [qtables[c[3]] for c in comps], coefs, markers, dri, stuffed, huffman)


def reconstruct_planes(dec):
    """Dequantise and invert the DCT in floating point -> per component float64 plane (whole MCUs), level shift undone."""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    t = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    t[0] /= np.sqrt(2.0)
    inv = np.empty(64, np.int64)
    inv[ZIGZAG] = np.arange(64)
    out = []
    for c, q in zip(dec.coefficients, dec.qtables):
        by, bx = c.shape[:2]
        f = (c.astype(np.float64) * q)[:, :, inv].reshape(by, bx, 8, 8)
        s = np.einsum("vy,abvu,ux->abyx", t, f, t)
        out.append(s.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8) + 128.0)
    return out
