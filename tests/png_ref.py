"""The restatement of the PNG decoder (thinktwice_amd/png.py, csrc/png.hip) for the family of files the dataset holds: 8-bit,
non-interlaced, colour type 0 or 2.  `parse` walks the chunks, zlib.decompress inflates, the unfilter is numpy (PNG
specification, section 9).  Standard library and numpy only."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def parse(data):
    """file bytes -> (width, height, channels, zlib stream)."""
    assert data[:8] == SIGNATURE
    pos, idat, ihdr, seen_end = 8, [], None, False
    while pos < len(data):
        assert not seen_end
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert len(body) == n and pos + 12 + n <= len(data)
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            seen_end = True
        pos += 12 + n
    assert seen_end and ihdr is not None
    w, h, depth, colour, comp, filt, lace = ihdr
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    return w, h, (1 if colour == 0 else 3), b"".join(idat)


def paeth(a, b, c):
    """Elementwise PaethPredictor on int arrays (or ints)."""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def unfilter(raw, h, w, c):
    """filtered scanlines, h * (1 + w * c) bytes -> uint8 [h, w, c]; ValueError for a wrong size or a filter type above 4."""
    if len(raw) != h * (1 + w * c):
        raise ValueError(f"{len(raw)} scanline bytes, {h} x (1 + {w} x {c}) expected")
    lines = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + w * c)
    if int(lines[:, 0].max()) > 4:
        raise ValueError(f"filter type {int(lines[:, 0].max())}")
    out = np.zeros((h, w, c), dtype=np.int64)
    up = np.zeros((w, c), dtype=np.int64)
    for y in range(h):
        ft, x = int(lines[y, 0]), lines[y, 1:].reshape(w, c).astype(np.int64)
        if ft == 0:
            row = x
        elif ft == 1:
            row = np.cumsum(x, axis=0) & 255
        elif ft == 2:
            row = (x + up) & 255
        else:
            row = np.zeros((w, c), dtype=np.int64)
            xs, ups = x.tolist(), up.tolist()
            for ch in range(c):
                a = cc = 0
                for i in range(w):
                    b = ups[i][ch]
                    if ft == 3:
                        v = (xs[i][ch] + ((a + b) >> 1)) & 255
                    else:
                        p = a + b - cc
                        pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                        v = (xs[i][ch] + (a if pa <= pb and pa <= pc else b if pb <= pc else cc)) & 255
                    row[i, ch] = v
                    a, cc = v, b
        out[y] = row
        up = row
    return out.astype(np.uint8)


def decode_stream(stream, h, w, c):
    """zlib stream -> uint8 [h, w, c] ([h, w] for grey); zlib.error or ValueError for a bad one."""
    img = unfilter(zlib.decompress(stream), h, w, c)
    return img[:, :, 0] if c == 1 else img


def decode(data):
    w, h, c, stream = parse(data)
    return decode_stream(stream, h, w, c)
