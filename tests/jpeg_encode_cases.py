"""Every image the JPEG encoder tests use (test_jpeg_ref.py, test_jpeg_encode_host.py with tools/jpeg_encode_host_check.cpp,
test_jpeg_encode.py on the device): (name, uint8 [h, w, c], quality, subsampling, restart_rows), and the case file the host
checker reads.  Standard library, numpy and tests/jpeg_ref.py only.  The smallest shapes at which each mechanism can go wrong;
`cases()` asserts, through jpeg_ref's counters, that each case built for a mechanism reaches it.

Shapes.  1 x 1, 7 x 9 and 17 x 33, grey / 4:4:4 / 4:2:0: partial MCUs in both directions, an odd chroma size.  16 x 513 at
4:4:4 and 16 x 1033 at 4:2:0 are 65 MCUs per row, one more than lanes (and 195 / 390 blocks: several entropy steps, the last
one partial).  80 x 16 grey at restart_rows 1 is ten intervals (RST7 is followed by RST0); 16 x 16 x 3 at 4:2:0 is one.
40 x 24 x 3 at 4:2:0 is three MCU rows, at restart_rows 1, 2 and 7 (larger than the image).

Contents.  Uniform noise at quality 100 (stuffed FF bytes); black and white 8 x 8 blocks in turn at quality 100 (DC difference
category 11); a 0 / 255 pixel checkerboard at quality 100 (an AC value of category 10); one far high-frequency basis function
at quality 10 (ZRL); a flat image (EOB only); quality 1, 50, 90 and 100 of one image; `camera` (a gradient plus small noise);
`hud` (flat areas with sharp one-pixel text edges, what the debug renderer draws).

The noise of the colour images is one value per pixel, added to all three channels, as a sensor's noise is mostly luminance.
Noise drawn per channel is chroma noise that 4:2:0 removes whatever the quality: on such images PIL's own file at quality
q - 5 measured a HIGHER PSNR than its file at q (28.60 against 28.25 dB on 7 x 9, 32.72 against 32.64 dB at quality 50), so
the fidelity condition of test_jpeg_encode_host.py, which presumes that PSNR falls with the quality, said nothing there.  That
test asserts the premise on PIL's files alone, case by case."""
import collections
import functools
import struct

import numpy as np

import jpeg_ref

SUBSAMPLING = {"444": 0, "420": 1}


def camera(h, w, c, seed=0):
    rng = np.random.default_rng(9100 + seed)
    yy = (np.arange(h, dtype=np.float32)[:, None, None] % 200) * 0.9
    xx = (np.arange(w, dtype=np.float32)[None, :, None] % 320) * 0.35
    noise = rng.integers(0, 12, (h, w, 1)).astype(np.float32)     # (of the luminance: see the module's text)
    tint = np.arange(c, dtype=np.float32)                             # a smooth chroma gradient: the channels' slopes differ
    return np.clip(noise + yy * (1 - 0.2 * tint) + xx * (1 + 0.3 * tint) + 20 * tint, 0, 255).astype(np.uint8)


def noise(h, w, c, seed=0):
    return np.random.default_rng(200 + seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def hud(h, w, seed=0):
    """A dark panel, two flat rectangles and rows of 5 x 7 glyph-like bit patterns in a light colour."""
    rng = np.random.default_rng(400 + seed)
    img = np.full((h, w, 3), (24, 24, 32), dtype=np.uint8)
    img[h // 8:h // 2, w // 10:w // 3] = (200, 40, 40)
    img[h // 3:h - 4, w // 2:w - 6] = (40, 90, 200)
    for y in range(3, h - 8, 10):
        for x in range(3, w - 6, 7):
            glyph = rng.integers(0, 2, (7, 5)).astype(bool)
            img[y:y + 7, x:x + 5][glyph] = (235, 235, 235)
    return img


def far_coefficient(zz=45, amplitude=120.0):
    """8 x 8 grey: the basis function of zig-zag position zz around mid grey."""
    n = int(jpeg_ref.ZIGZAG[zz])
    v, u = divmod(n, 8)
    y, x = np.arange(8)[:, None], np.arange(8)[None, :]
    b = np.cos((2 * y + 1) * v * np.pi / 16) * np.cos((2 * x + 1) * u * np.pi / 16)
    return np.clip(np.rint(128 + amplitude * b), 0, 255).astype(np.uint8)[:, :, None]


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, img, quality=90, sub="420", rr=1, expect=None):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.ndim == 2:
            img = img[:, :, None]
        img.setflags(write=False)
        full = f"{name}_{img.shape[0]}x{img.shape[1]}x{img.shape[2]}_q{quality}_{sub}_r{rr}"
        if expect is not None:
            counts = collections.Counter()
            jpeg_ref.encode(img, quality, sub, rr, counts)
            assert expect(counts), (full, dict(counts))
        out.append((full, img, quality, sub, rr))

    for h, w in ((1, 1), (7, 9), (17, 33)):
        add("image", camera(h, w, 1, 1) + noise(h, w, 1, 1) // 8)
        add("image", camera(h, w, 3, 2) + noise(h, w, 1, 2) // 8, sub="444")
        add("image", camera(h, w, 3, 3) + noise(h, w, 1, 3) // 8, sub="420")
    add("wide65", camera(16, 513, 3, 4), sub="444", expect=lambda c: c["intervals"] == 2)
    add("wide65", camera(16, 1033, 3, 5), sub="420", expect=lambda c: c["intervals"] == 1)
    add("rstwrap", camera(80, 16, 1, 6), expect=lambda c: c["intervals"] == 10)
    add("single", camera(16, 16, 3, 7), sub="420", expect=lambda c: c["intervals"] == 1)
    for rr, n in ((1, 3), (2, 2), (7, 1)):
        add("rows", camera(40, 24, 3, 8), rr=rr, expect=lambda c, n=n: c["intervals"] == n)
    add("noise", noise(32, 32, 3, 1), 100, "444", expect=lambda c: c["stuffed"] >= 1)
    blocks = np.kron((np.indices((2, 4)).sum(axis=0) % 2) * 255, np.ones((8, 8), dtype=np.int64))
    add("blocks", blocks, 100, expect=lambda c: c["dc11"] >= 1)
    add("checker", (np.indices((16, 16)).sum(axis=0) % 2) * 255, 100, expect=lambda c: c["ac10"] >= 1)
    add("far", far_coefficient(), 10, expect=lambda c: c["zrl"] >= 1)
    add("flat", np.full((24, 40, 3), 77), expect=lambda c: c["eob"] == 6 * 2 * 3 and not any(k.startswith("ac") for k in c))
    for q in (1, 50, 90, 100):
        add("quality", camera(24, 40, 3, 9) + noise(24, 40, 1, 9) // 16, q)
    add("camera", camera(64, 96, 3, 10), sub="420")
    add("camera", camera(64, 96, 3, 10), sub="444", rr=2)
    add("hud", hud(48, 80), sub="420")
    add("hud", hud(48, 80), sub="444")
    return out


def write_case_file(path, extra=()):
    """magic, count, then per case: name, (H, W, C, quality, subsampling, restart_rows) int32, the pixels.  `extra`: more
    cases of the same form, after cases().  Returns the number of cases."""
    every = list(cases()) + list(extra)
    with open(path, "wb") as f:
        f.write(b"TTJPGE01" + struct.pack("<i", len(every)))
        for name, img, quality, sub, rr in every:
            f.write(struct.pack("<i", len(name)) + name.encode())
            f.write(struct.pack("<6i", *img.shape, quality, SUBSAMPLING[sub], rr))
            f.write(img.tobytes())
    return len(every)
