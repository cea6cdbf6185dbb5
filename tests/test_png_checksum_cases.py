"""The case generators of the checksum tests (tests/png_checksum_cases.py) against zlib and the host parser: a "corrupted" file
must really keep deflate's rules and the output size and fail only its checksum, a CRC-only case must have intact data, the
chunk CRCs the parser collects must be the chunks', and the tile table must cover every range exactly once.  No device."""
import ctypes
import io
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import png_cases as P  # noqa: E402
import png_checksum_cases as K  # noqa: E402
import png_ref as R  # noqa: E402
from thinktwice_amd import _lib, png  # noqa: E402


def _stream(data):
    crcs = []
    w, h, c, parts = png._walk(data, False, crcs)
    return w, h, c, [bytes(p) for p in parts], crcs


def _chunk_crcs_hold(data):
    """[bool per IDAT chunk]: zlib.crc32(b"IDAT" + body) is the chunk's CRC field."""
    _, _, _, parts, crcs = _stream(data)
    return [zlib.crc32(b"IDAT" + p) == crc for p, crc in zip(parts, crcs)]


def test_constants_and_status_names_match_the_header():
    c = _lib.constants()
    assert K.T == c["TT_CHECKSUM_TILE"] and (K.ADLER32, K.CRC32) == (c["TT_CHECKSUM_ADLER32"], c["TT_CHECKSUM_CRC32"])
    assert {k: c[k] for k in ("TT_PNGV_BAD_ADLER32", "TT_PNGV_BAD_CRC32")} == {k: v for k, v in K.STATUS.items() if k.startswith("TT_PNGV")}
    assert max(P.STATUS.values()) == 10 and sorted(png.STATUS_NAMES) == list(range(13))
    assert ctypes.sizeof(png.PngChunk) == 24 and ctypes.sizeof(png.ChecksumRange) == 16


def test_every_corrupted_case_inflates_to_the_right_size_and_fails_only_what_it_says():
    h, w, c = K.CORRUPT_SIZE
    for name, data, both, adler, img, stream in K.corrupted_files():
        ww, hh, cc, parts, crcs = _stream(data)
        assert (hh, ww, cc) == (h, w, c) and b"".join(parts) == stream, name
        d = zlib.decompressobj(-15)                                    # the deflate stream alone: its own rules and the size hold ...
        raw = d.decompress(stream[2:])
        assert d.eof and d.unused_data == stream[-4:] and len(raw) == h * (1 + w * c), name
        assert all(raw[y * (1 + w * c)] <= 4 for y in range(h)), name
        adler_ok = zlib.adler32(raw) == int.from_bytes(stream[-4:], "big")
        crc_ok = all(_chunk_crcs_hold(data))
        if both == "TT_PNGV_BAD_ADLER32":                              # ... and zlib.decompress refuses the stream
            assert crc_ok and not adler_ok and adler == both and img is None, name
            with pytest.raises(zlib.error, match="incorrect data check"):
                zlib.decompress(stream)
        elif name.startswith("c_"):                                    # CRC only: the data is intact
            assert not crc_ok and adler_ok and adler == "TT_PNG_OK" and sum(_chunk_crcs_hold(data)) == len(parts) - 1, name
            assert np.array_equal(R.unfilter(zlib.decompress(stream), h, w, c), img), name
        else:                                                          # (d): both wrong, the CRC-32 is reported
            assert name.startswith("d_") and not crc_ok and not adler_ok and (both, adler) == ("TT_PNGV_BAD_CRC32", "TT_PNGV_BAD_ADLER32")
    names = [n[0] for n, *_ in K.corrupted_files()]
    assert names == ["a"] + ["b"] * 4 + ["c"] * 3 + ["d"]
    # which chunk of (c) is broken: the first, a middle one, the last
    broken = [_chunk_crcs_hold(d).index(False) for n, d, *_ in K.corrupted_files() if n.startswith("c_")]
    assert broken == [0, 2, 3]


def test_good_files_are_good_and_their_splits_are_what_they_claim():
    seen = {"empty": 0, "one_byte": 0, "cut_in_trailer": 0, "longer_than_tile": 0, "after_trailer": 0}
    for name, data, img in K.good_files():
        w, h, c, parts, crcs = _stream(data)
        assert all(_chunk_crcs_hold(data)), name
        stream = b"".join(parts)
        d = zlib.decompressobj()
        raw = d.decompress(stream)
        assert d.eof and np.array_equal(R.unfilter(raw, h, w, c), img), name
        end = len(stream) - len(d.unused_data)                        # the trailer is stream[end - 4:end]
        assert zlib.adler32(raw) == int.from_bytes(stream[end - 4:end], "big"), name
        seen["after_trailer"] += len(d.unused_data) > 0
        seen["longer_than_tile"] += any(len(p) > K.T for p in parts)
        if name.endswith("/split"):
            seen["empty"] += any(len(p) == 0 for p in parts)
            seen["one_byte"] += sum(len(p) == 1 for p in parts) >= 2
            edges = np.cumsum([len(p) for p in parts])[:-1]
            seen["cut_in_trailer"] += any(end - 4 < e < end for e in edges)
    n = len(P.good_cases())
    assert seen["empty"] == n and seen["one_byte"] == n and seen["cut_in_trailer"] == n, seen
    assert seen["longer_than_tile"] >= 2 and seen["after_trailer"] == 1, seen


def test_walk_collects_every_idat_crc_and_checks_the_other_chunks_on_the_host():
    for name, data, img in K.good_files()[::7]:
        crcs = []
        w, h, c, parts = png._walk(data, False, crcs)
        assert crcs == [zlib.crc32(b"IDAT" + bytes(p)) for p in parts] and len(crcs) >= 1, name
        assert png._walk(data, False)[:3] == (w, h, c)
    h, w, c = K.CORRUPT_SIZE
    stream = P.COMPRESSORS["level6"](P.filter_rows(P.image(h, w, c), [0] * h))
    for kind in (b"IHDR", b"tEXt", b"IEND"):
        data = K.chunked_file(w, h, c, stream, [10], bad_other=kind)
        assert png._walk(data, False)[0] == w                          # not checked by default
        with pytest.raises(ValueError, match="CRC-32"):
            png._walk(data, False, [])
    flipped = K.chunked_file(w, h, c, stream, [10], crc_flip=1)         # an IDAT's field is the device's to check
    crcs = []
    png._walk(flipped, False, crcs)
    assert crcs[0] == zlib.crc32(b"IDAT" + stream[:10]) and crcs[1] == zlib.crc32(b"IDAT" + stream[10:]) ^ 0x00010000
    with pytest.raises(ValueError, match="CRC-32"):
        png._walk(flipped, True)


def test_op_cases_are_what_they_claim():
    total, ranges = K.many_ranges()
    assert len(ranges) > 200 and all(0 <= o and o + n <= total for o, n in ranges)
    starts = {o for o, _ in ranges}
    assert sum(n == 0 for _, n in ranges) > 10 and sum(n > 0 and o + n in starts for o, n in ranges) > 50      # adjacent ones
    assert [o for o, _ in ranges] != sorted(o for o, _ in ranges) and any(n > K.T for _, n in ranges)
    residues = {o % 16 for o, _ in K.packed_ranges(K.LENGTHS)[1]}          # the word loop sees every start alignment
    assert {r % 4 for r in residues} == {0, 1, 2, 3} and len(residues) >= 12
    names = {n for n, _, _ in K.adler_extremes()}
    assert {"ff_5552", "ff_5553", f"ff_{K.T}", f"ff_{3 * K.T + 7}", "ff_full_frame", "sum_65520_a_wraps_to_0"} <= names
    assert len(dict((n, a) for n, a, _ in K.adler_extremes())["ff_full_frame"]) == 4320900


def test_the_tile_table_covers_every_range_exactly_once(tmp_path):
    """The builder is C++ (csrc/png_checksum.h: plan_count, plan_write, range_tiles): tools/png_checksum_host_check.cpp checks,
    for every ranges case of the case file, that each range's tiles follow each other in order from first_tile[range], that
    each is at most T bytes and only a range's last one is shorter, that together they are exactly the range, that a
    zero-length range keeps its first_tile entry and owns no tile, and that 256 planners build the same table as one.  Here
    (without sanitizers, which test_png_checksum_host.py adds): every ranges case passes it, the 201-range one among them."""
    import host_tool
    cases = str(tmp_path / "cases.bin")
    K.write_case_file(cases)
    exe = host_tool.build("png_checksum_host_check", tmp_path, sanitize=False, extra_flags=("-O1",))    # (as before: the last -O wins)
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    assert run.returncode == 0 and ", 0 failed" in run.stdout.splitlines()[-1]
    ok = [l for l in run.stdout.splitlines() if l.startswith("ok  ") and " ranges, 0 wrong" in l]
    assert len(ok) >= 28 and any("many_ranges: 201 ranges" in l for l in ok)


def test_what_pil_does_with_a_bad_adler32_and_with_a_bad_idat_crc():
    """Information: PIL (12.2.0 where this was written) raises on case (a), as the reference loader therefore does, and accepts
    case (c): verifying the IDAT CRC-32 goes beyond the reference."""
    Image = pytest.importorskip("PIL.Image")
    files = {n[0]: (d, img) for n, d, _, _, img, _ in K.corrupted_files() if n[0] in "ac"}
    with pytest.raises(OSError, match="broken data stream"):
        np.array(Image.open(io.BytesIO(files["a"][0])))
    assert np.array_equal(np.array(Image.open(io.BytesIO(files["c"][0]))), files["c"][1])
