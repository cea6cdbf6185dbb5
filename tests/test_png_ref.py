"""The PNG cases (tests/png_cases.py) against the restatement (tests/png_ref.py: chunk walking, zlib.decompress, a numpy
unfilter), PIL where it is installed, and the host parser thinktwice_amd.png.parse_png.  No device."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import png_cases as P  # noqa: E402
import png_ref as R  # noqa: E402
from thinktwice_amd import _lib, png  # noqa: E402


def _files():
    """[(name, file bytes, array)]: every good case as a file, IDAT chunk sizes and the ancillary chunk alternating."""
    out = []
    for i, (name, stream, h, w, c, img) in enumerate(P.good_cases()):
        out.append((name, P.png_file(w, h, c, stream, idat_bytes=(100, 65536)[i % 2], ancillary=i % 3 == 0), img))
    return out


def _squeeze(img):
    return img[:, :, 0] if img.shape[2] == 1 else img


def test_status_names_match_the_header():
    consts = _lib.constants()
    assert {k: consts[k] for k in P.STATUS} == P.STATUS
    assert {k for k in consts if k.startswith("TT_PNG_") and not k.startswith("TT_PNG_MAX")} == set(P.STATUS)


def test_every_good_case_decodes_under_the_restatement_to_its_array():
    for name, data, img in _files():
        assert np.array_equal(R.decode(data), _squeeze(img)), name


def test_hand_assembled_streams_inflate_to_the_bytes_the_assembler_tracked():
    for name, stream, h, w, c, raw in P.hand_cases():
        assert zlib.decompress(stream) == raw and len(raw) == h * (1 + w * c), name
    far = dict((n, s) for n, s, *_ in P.hand_cases())["distance_32768"]
    assert zlib.decompress(far[2:-4], -15) == zlib.decompress(far)


def test_every_case_decodes_under_pil_and_pil_files_under_the_restatement():
    Image = pytest.importorskip("PIL.Image")
    import io
    for name, data, img in _files():
        assert np.array_equal(np.array(Image.open(io.BytesIO(data))), _squeeze(img)), name
    for h, w, c in ((45, 80, 3), (45, 80, 1), (1, 1, 3), (130, 9, 1)):
        img = _squeeze(P.image(h, w, c, seed=3))
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        assert np.array_equal(R.decode(buf.getvalue()), img)
        info = png.parse_png(buf.getvalue(), verify_crc=True)
        assert (info.width, info.height, info.channels) == (w, h, c)


def test_every_malformed_stream_is_refused_by_the_restatement():
    for name, stream, status in P.malformed_cases():
        assert status in P.STATUS and status != "TT_PNG_OK"
        with pytest.raises((zlib.error, ValueError)):
            R.decode_stream(stream, P.MAL_H, P.MAL_W, P.MAL_C)


def test_parse_png_equals_the_restatements_parser():
    for name, data, img in _files():
        for crc in (False, True):
            info = png.parse_png(data, verify_crc=crc)
            assert (info.width, info.height, info.channels, bytes(info.zlib_stream)) == R.parse(data), name


def _one(**kw):
    img = P.image(4, 5, 3)
    return P.png_file(5, 4, 3, zlib.compress(P.filter_rows(img, [0] * 4)), **kw)


@pytest.mark.parametrize("what, data", [
    ("bit depth 16", _one(depth=16)),
    ("palette", _one(colour=3)),
    ("RGBA", _one(colour=6)),
    ("alpha", _one(colour=4)),
    ("interlace", _one(interlace=1)),
    ("after IEND", _one() + b"\0"),
    ("runs past", _one()[:60]),
    ("no IEND", _one()[:-12]),
    ("signature", b"\x89PNX" + _one()[4:]),
])
def test_parse_png_names_the_unsupported_property(what, data):
    with pytest.raises(ValueError, match=what):
        png.parse_png(data)


def test_parse_png_refuses_split_idat_runs_a_plte_chunk_and_a_bad_crc():
    good = _one(idat_bytes=20)
    first_idat = good.index(b"IDAT") - 4
    n, = struct.unpack_from(">I", good, first_idat)
    text = P._chunk(b"tEXt", b"k\0v")
    split = good[:first_idat + 12 + n] + text + good[first_idat + 12 + n:]
    with pytest.raises(ValueError, match="not consecutive"):
        png.parse_png(split)
    plte = good[:first_idat] + P._chunk(b"PLTE", bytes(3)) + good[first_idat:]
    with pytest.raises(ValueError, match="PLTE"):
        png.parse_png(plte)
    broken = bytearray(good)
    broken[first_idat + 9] ^= 1
    assert png.parse_png(bytes(broken)).width == 5                # not checked by default
    with pytest.raises(ValueError, match="CRC-32"):
        png.parse_png(bytes(broken), verify_crc=True)
