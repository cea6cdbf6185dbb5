"""tests/jpeg_ref.py, the numpy restatement the device's JPEG encoder is held to, is itself held to an independent
implementation here: PIL (libjpeg) opens every file it writes, agrees on the quantisation and Huffman tables, and the
restatement's parser and entropy decoder read PIL's own baseline files to coefficients from which PIL's decoded pixels follow.
CPU only."""
import io
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import jpeg_encode_cases as E  # noqa: E402
import jpeg_ref  # noqa: E402

PIL_SUBSAMPLING = {"444": 0, "420": 2}


def pil_file(img, quality, sub, restart_rows=0):
    from PIL import Image
    out = io.BytesIO()
    arr = img[:, :, 0] if img.shape[2] == 1 else img
    kw = {"restart_marker_rows": restart_rows} if restart_rows else {}
    Image.fromarray(arr).save(out, "JPEG", quality=quality, subsampling=PIL_SUBSAMPLING[sub], optimize=False, **kw)
    return out.getvalue()


def test_zigzag_and_tables_are_the_standards():
    z = jpeg_ref.ZIGZAG
    assert sorted(z.tolist()) == list(range(64)) and z[:6].tolist() == [0, 1, 8, 16, 9, 2] and z[-3:].tolist() == [55, 62, 63]
    t = jpeg_ref.dct_matrix()
    assert sorted(set(np.abs(t).ravel().tolist())) == [1598, 3135, 4551, 5793, 6811, 7568, 8035]
    for (cls, _), (bits, vals) in jpeg_ref.HUFF.items():
        assert sum(bits) == len(vals) == len(set(vals)) == (162 if cls else 12)
        codes = jpeg_ref.canonical_codes(bits, vals)
        assert sum(2.0 ** -n for _, n in codes.values()) < 1.0                  # a prefix code that leaves the all-ones code free
    assert jpeg_ref.quant_tables(50)[0].tolist() == jpeg_ref.BASE_QUANT[0].tolist() and (jpeg_ref.quant_tables(100) == 1).all()


def test_pil_opens_every_file_and_agrees_on_size_mode_and_tables():
    from PIL import Image
    for name, img, quality, sub, rr in E.cases():
        f = jpeg_ref.encode(img, quality, sub, rr)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            im = Image.open(io.BytesIO(f))
            im.load()
        h, w, c = img.shape
        assert im.size == (w, h) and im.mode == ("L" if c == 1 else "RGB") and im.format == "JPEG", name
        own = Image.open(io.BytesIO(pil_file(img, quality, sub)))
        assert {k: list(v) for k, v in im.quantization.items()} == {k: list(v) for k, v in own.quantization.items()}, name
        assert im.info.get("jfif") == 257 and im.info.get("jfif_density") == (1, 1) and im.info.get("jfif_unit") == 0, name
        assert f[:2] == b"\xff\xd8" and f[-2:] == b"\xff\xd9", name


def test_the_decoder_reads_back_what_the_encoder_quantised():
    for name, img, quality, sub, rr in E.cases():
        f = jpeg_ref.encode(img, quality, sub, rr)
        dec = jpeg_ref.decode_coefficients(f)
        want = jpeg_ref.quantised_coefficients(img, quality, sub)
        assert (dec.height, dec.width, dec.components) == img.shape, name
        assert len(dec.coefficients) == len(want) and all(np.array_equal(a, b) for a, b in zip(dec.coefficients, want)), name
        h, w, c = img.shape
        m = 16 if (c == 3 and sub == "420") else 8
        mx, my = -(-w // m), -(-h // m)
        assert dec.dri == rr * mx, name
        order = [m for _, m in dec.markers]
        assert order[:7] == [0xD8, 0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA] and order[-1] == 0xD9, name
        n_int = -(-my // rr)
        assert order[7:-1] == [0xD0 + (k & 7) for k in range(n_int - 1)], name
        assert dec.stuffed == f[dec.markers[6][0]:].count(b"\xff\x00"), name


@pytest.mark.parametrize("restart_rows", [0, 1, 2])
def test_the_decoder_reads_pils_own_files_and_pils_pixels_follow_from_its_coefficients(restart_rows):
    """Not only self-consistent: PIL's baseline files (standard tables, optimize=False, with and without restart markers) are
    parsed and entropy-decoded; dequantised and inverse-transformed in floating point, the coefficients give PIL's decoded
    planes to within libjpeg's integer IDCT (1 level; the draft mode hands out YCbCr without the colour conversion)."""
    from PIL import Image
    seen = 0
    for name, img, quality, sub, _ in E.cases():
        h, w, c = img.shape
        if (c == 3 and sub == "420") or quality < 50:       # (fancy chroma upsampling; coarse tables: 1 level no longer holds)
            continue
        f = pil_file(img, quality, sub, restart_rows)
        dec = jpeg_ref.decode_coefficients(f)
        assert dec.huffman == {k: (v[0], v[1]) for k, v in jpeg_ref.HUFF.items() if k in dec.huffman}, name
        assert (dec.dri > 0) == (restart_rows > 0), name
        im = Image.open(io.BytesIO(f))
        if c == 3:
            im.draft("YCbCr", im.size)
            assert im.mode == "YCbCr", name
        got = np.asarray(im).reshape(h, w, c).astype(np.float64)
        planes = jpeg_ref.reconstruct_planes(dec)
        for k in range(c):
            want = np.clip(planes[k][:h, :w], 0, 255)
            assert np.abs(got[:, :, k] - want).max() <= 1.0 + 1e-6, (name, k, np.abs(got[:, :, k] - want).max())
        seen += 1
    assert seen >= 10
