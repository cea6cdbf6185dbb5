"""Every image the encoder tests use (test_png_encode_host.py with tools/png_encode_host_check.cpp, test_png_encode.py on the
device): (name, uint8 [h, w, c], rows per segment, filter mode), the numpy restatement of the filter pass -- the adaptive
choice included -- and the case file the host checker reads.  Standard library and numpy only, plus tests/png_cases.py for
the five filters.

Shapes.  1 x 1 x 1, 1 x 1 x 3 and 3 x 5 x 1 are the minimal sizes; 17 x 33 x 3 is two segments, the second of one row;
16 x 700 x 3 exactly one; 40 x 700 x 3 at R = 7 and 33 the decoder suite's own pair (a short last segment; more than one
65,535-byte stored block); 16 x 1600 x 3 a 76.8 KB segment, longer than deflate's window and than one stored block;
4 x 40000 x 1 of four identical random rows under filter `none` has its only long match at distance 40,001, which no
deflate stream may use: an encoder that forgets the window limit writes a stream that does not inflate, here and nowhere else.

Contents.  constant and all-255 (runs: the run bound); the depth ramp and the tag map of the dataset's label files; uniform
noise (the stored fallback); `camera` (a smooth gradient plus small noise); two values in two long runs, a two-pixel image
and a two-valued row shorter than one 64-position step (a block whose matches all have ONE distance; a stored block; a
dynamic block without a match); `fibonacci`: a byte histogram of Fibonacci counts over FIB_SYMBOLS symbols in a shuffled
order under filter `none` (with the filter byte and the end-of-block symbol as the sequence's two ones).  The Huffman code of
that histogram is 18 levels deep; the host test reads the checker's limiter count for it and fails at 0."""
import functools
import struct

import numpy as np

import png_cases as P

MODES = {"none": 0, "sub": 1, "up": 2, "avg": 3, "paeth": 4, "adaptive": 5}
DEFAULT_ROWS = 16
FIB_SYMBOLS = 17
FIB_SEED = 5


def camera(h, w, c, seed=0):
    rng = np.random.default_rng(9000 + seed)
    yy = (np.arange(h, dtype=np.float32)[:, None, None] % 200) * 0.9
    xx = (np.arange(w, dtype=np.float32)[None, :, None] % 320) * 0.35
    noise = rng.integers(0, 12, (h, w, c)).astype(np.float32)
    return np.clip(noise + yy + xx + 20 * np.arange(c, dtype=np.float32), 0, 255).astype(np.uint8)


def noise(h, w, c, seed=0):
    return np.random.default_rng(100 + seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def depth_ramp(h, w, seed=0):
    """A smooth ramp in CARLA's 24-bit depth code (R lowest)."""
    yy, xx = np.mgrid[0:h, 0:w]
    a, b = 5 + seed % 7, 3 + seed % 5
    code = ((yy * a + xx * b) * 16777215 // (h * a + w * b)).astype(np.uint32)
    return np.stack([code & 255, (code >> 8) & 255, code >> 16], axis=-1).astype(np.uint8)


def tag_map(h, w, seed=0):
    """Semantic tags in 16 x 16 blocks, as synth.raw_label_bytes lays them out."""
    rng = np.random.default_rng(300 + seed)
    palette = np.array([0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 12, 22], dtype=np.uint8)
    blocks = palette[rng.integers(0, len(palette), (-(-h // 16), -(-w // 16)))]
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 16, axis=0), 16, axis=1)[:h, :w, None])


def fibonacci(symbols=FIB_SYMBOLS, seed=FIB_SEED):
    """1 x n x 1: `symbols` distinct non-zero byte values with the Fibonacci counts 2, 3, 5, 8, ..., in a shuffled order.  The
    two singletons that complete the sequence 1, 1, 2, 3, 5, ... are the stream's own: the row's filter byte 0 and the block's
    end-of-block symbol.  (With two more symbols of count 1 the optimal code is two interleaved chains of half the depth.)"""
    rng = np.random.default_rng(seed)
    counts = [2, 3]
    while len(counts) < symbols:
        counts.append(counts[-1] + counts[-2])
    values = (1 + rng.permutation(255)[:symbols]).astype(np.uint8)
    data = np.repeat(values, counts)
    return rng.permutation(data).reshape(1, -1, 1)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, img, rows=DEFAULT_ROWS, mode="adaptive"):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        img.setflags(write=False)
        out.append((f"{name}_{img.shape[0]}x{img.shape[1]}x{img.shape[2]}_R{rows}_{mode}", img, rows, mode))

    for h, w, c in ((1, 1, 1), (1, 1, 3), (3, 5, 1)):
        add("image", P.image(h, w, c, seed=2))
        add("constant", np.full((h, w, c), 77))
    for mode in MODES:
        add("image", P.image(17, 33, 3, seed=4), mode=mode)
    add("constant", np.full((16, 700, 3), 93))
    add("all255", np.full((16, 700, 3), 255))
    add("noise", noise(16, 700, 3, 1), mode="none")
    add("camera", camera(16, 700, 3, 1))
    for rows in (7, 33):
        add("camera", camera(40, 700, 3, 2), rows)
        add("image", P.image(40, 700, 3, seed=8), rows, "paeth")
        add("noise", noise(40, 700, 3, 2), rows)
    add("camera", camera(16, 1600, 3, 3))
    add("ramp", depth_ramp(16, 1600, 1))
    add("tags", tag_map(16, 1600, 1))
    add("noise", noise(16, 1600, 3, 3), mode="none")
    add("constant", np.full((16, 1600, 3), 200))
    add("all255", np.full((16, 1600, 3), 255))
    add("rows4same", np.repeat(noise(1, 40000, 1, 4), 4, axis=0), mode="none")
    add("tworuns", np.repeat(np.array([[31], [32]], dtype=np.uint8), 40000, axis=1)[:, :, None], mode="none")
    add("twopixels", np.array([[[7], [9]]], dtype=np.uint8), mode="none")
    add("nomatch", (np.arange(60) % 7 == 3).astype(np.uint8).reshape(1, 60, 1) * 9 + 5, mode="none")
    add("fibonacci", fibonacci(), mode="none")
    return out


def filtered_all(img):
    """uint8 [5, h, 1 + w * c]: the image's scanlines under each of the five filter types (every one from the RAW row above)."""
    h = img.shape[0]
    return np.stack([np.frombuffer(P.filter_rows(img, [t] * h), dtype=np.uint8).reshape(h, -1) for t in range(5)])


def filter_types(img, mode):
    """The type of every row under `mode`.  adaptive: per row and type the sum of |residual as int8|; the smallest sum wins,
    the lowest type number on a tie (np.argmin returns the first minimum)."""
    h = img.shape[0]
    if mode != "adaptive":
        return [MODES[mode]] * h
    res = filtered_all(img)[:, :, 1:].astype(np.int64)
    sums = np.where(res < 128, res, 256 - res).sum(axis=2)            # [5, h]
    return np.argmin(sums, axis=0).tolist()


def scanlines(img, mode):
    return P.filter_rows(img, filter_types(img, mode))


def segment_bytes(img, rows):
    """The filtered bytes of every segment."""
    h, w, c = img.shape
    rows = min(rows, h)
    return [min(rows, h - y) * (1 + w * c) for y in range(0, h, rows)]


def stored_only_size(img, rows):
    """The file with every segment as stored blocks: per segment n + 5 * ceil(n / 65535) + 5, the zlib header and tail, the
    container's fixed bytes (signature, IHDR, ttSG, the IDAT and IEND frames)."""
    n = segment_bytes(img, rows)
    return sum(k + 5 * -(-k // 65535) + 5 for k in n) + 2 + 6 + container_bytes(len(n))


def container_bytes(num_segments):
    return 8 + 25 + (12 + 9 + 4 * (num_segments + 1)) + 12 + 12


def write_case_file(path):
    """magic, count, then per case: name, (H, W, C, R, mode) int32, the pixels.  Returns the number of cases."""
    with open(path, "wb") as f:
        f.write(b"TTPNGE01" + struct.pack("<i", len(cases())))
        for name, img, rows, mode in cases():
            f.write(struct.pack("<i", len(name)) + name.encode())
            f.write(struct.pack("<5i", *img.shape, rows, MODES[mode]))
            f.write(img.tobytes())
    return len(cases())
