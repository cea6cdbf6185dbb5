"""The file convention of segmented PNG files on the host (thinktwice_amd/png.py: segment_png, read_segments, the `ttSG`
chunk, PngDecoder's `segments=` modes as parse_files applies them; thinktwice_amd/png_segment.py, the command-line tool).
No GPU: what the device makes of these files is test_png_segments.py, the same inflate source under sanitizers
test_png_segments_host.py."""
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import png_cases as P  # noqa: E402
import png_segment_cases as S  # noqa: E402
from thinktwice_amd import png, png_segment  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(h):
    return [1, 2, 7, 64, h, h + 5]


def _plain(h, w, c, f, i=0):
    img = P.image(h, w, c)
    src = img if c == 3 else img[:, :, 0]
    types = P.filter_types(f, h)
    return src, P.filter_rows(img, types), P.write_png(src, types, idat_bytes=(100, 65536)[i % 2], ancillary=True)


@pytest.mark.parametrize("h, w", P.SIZES)
@pytest.mark.parametrize("c", [1, 3])
def test_segmented_files_are_valid_hold_the_same_scanlines_and_every_segment_inflates_alone(h, w, c):
    stride = 1 + w * c
    for i, f in enumerate(P.FILTERS):
        src, lines, plain = _plain(h, w, c, f, i)
        for r in _rows(h):
            for level in (0, 6):
                out = png.segment_png(plain, r, level, idat_bytes=(64, 65536)[i % 2])
                info = png.parse_png(out, verify_crc=True)
                assert (info.height, info.width, info.channels) == (h, w, c)
                assert zlib.decompress(info.zlib_stream) == lines, (f, r, level)
                index = png.read_segments(out, verify_crc=True)
                n = -(-h // r)
                assert index.rows_per_segment == r and len(index.offsets) == n + 1 and index.offsets[0] == 2
                for k in range(n):
                    a, b = index.offsets[k], index.offsets[k + 1]
                    assert info.zlib_stream[b - 4:b] == b"\x00\x00\xff\xff"
                    d = zlib.decompressobj(-15)
                    assert d.decompress(info.zlib_stream[a:b]) == lines[k * r * stride:(k + 1) * r * stride], (f, r, level, k)
                    assert not d.eof and d.unused_data == b""
                tail = info.zlib_stream[index.offsets[n]:]
                assert tail[:-4] in (b"\x03\x00", b"\x01\x00\x00\xff\xff") and tail[-4:] == struct.pack(">I", zlib.adler32(lines))
                assert png.segment_png(out, r, level, idat_bytes=(64, 65536)[i % 2]) == out, "segmenting twice"
                kinds = [k for k, _ in png._chunks(out)]
                assert kinds.count(b"ttSG") == 1 and kinds.index(b"ttSG") == kinds.index(b"IDAT") - 1
                assert [kb for kb in png._chunks(out) if kb[0] not in (b"IDAT", b"ttSG")] == \
                    [kb for kb in png._chunks(plain) if kb[0] != b"IDAT"], "the other chunks, in place"


@pytest.mark.parametrize("h, w", P.SIZES)
def test_pil_opens_a_segmented_file_to_the_same_array(h, w):
    Image = pytest.importorskip("PIL.Image")
    for c in (1, 3):
        for f in P.FILTERS:
            src, _, plain = _plain(h, w, c, f)
            for r in _rows(h):
                got = np.array(Image.open(io.BytesIO(png.segment_png(plain, r))))
                assert got.shape == src.shape and np.array_equal(got, src), (c, f, r)


def test_resegmenting_with_other_parameters_replaces_the_index_and_keeps_the_pixels():
    src, lines, plain = _plain(37, 53, 3, "random")
    a = png.segment_png(plain, 7)
    b = png.segment_png(a, 16, level=9)
    assert png.read_segments(b).rows_per_segment == 16 and [k for k, _ in png._chunks(b)].count(b"ttSG") == 1
    assert zlib.decompress(png.parse_png(b).zlib_stream) == lines
    assert png.segment_png(b, 7) == a
    assert png.read_segments(plain) is None
    with pytest.raises(ValueError):
        png.segment_png(plain, 0)


# ---------------------------------------------------------------------------------------------------- read_segments' refusals
def _rebuild(data, edit):
    """The file with `edit(chunks)` applied to its [(kind, body)] list, CRCs made right again."""
    chunks = [list(kb) for kb in png._chunks(data)]
    chunks = edit(chunks) or chunks
    return png.SIGNATURE + b"".join(png._chunk(k, b) for k, b in chunks)


def _with_index(data, fn):
    """fn(version, rows, n, offsets list) -> the new tuple; the ttSG body is rewritten from it."""
    def edit(chunks):
        for kb in chunks:
            if kb[0] == b"ttSG":
                version, rows, n = struct.unpack_from(">BII", kb[1])
                version, rows, n, offsets = fn(version, rows, n, list(struct.unpack_from(f">{n + 1}I", kb[1], 9)))
                kb[1] = struct.pack(f">BII{len(offsets)}I", version, rows, n, *offsets)
    return _rebuild(data, edit)


def _with_payload(data, fn):
    def edit(chunks):
        payload = fn(bytearray(b"".join(b for k, b in chunks if k == b"IDAT")))
        first = [k for k, _ in chunks].index(b"IDAT")
        return [kb for kb in chunks[:first] if kb[0] != b"IDAT"] + [[b"IDAT", bytes(payload)]] + [kb for kb in chunks[first:] if kb[0] != b"IDAT"]
    return _rebuild(data, edit)


def _corrupted():
    """{refusal reason: (file, a word of the message)}: one hand-corrupted file per reason."""
    h, w, c = 37, 53, 3
    src, lines, plain = _plain(h, w, c, "paeth")
    good = png.segment_png(plain, 7)                                     # 6 segments
    index = png.read_segments(good)
    o = index.offsets

    def move_index_after_idat(chunks):
        sg = [kb for kb in chunks if kb[0] == b"ttSG"]
        rest = [kb for kb in chunks if kb[0] != b"ttSG"]
        return rest[:-1] + sg + rest[-1:]

    def second_index(chunks):
        i = [k for k, _ in chunks].index(b"ttSG")
        return chunks[:i] + [chunks[i], list(chunks[i])] + chunks[i + 1:]

    files = {
        "unknown version": (_with_index(good, lambda v, r, n, off: (2, r, n, off)), "version"),
        "R = 0": (_with_index(good, lambda v, r, n, off: (v, 0, n, off)), "rows_per_segment"),
        "n != ceil(H / R)": (_with_index(good, lambda v, r, n, off: (v, 8, n, off)), "num_segments"),
        "body length": (_with_index(good, lambda v, r, n, off: (v, r, n, off + [off[-1] + 1])), "body"),
        "offsets[0] != 2": (_with_index(good, lambda v, r, n, off: (v, r, n, [3] + off[1:])), "offsets[0]"),
        "offsets not increasing": (_with_index(good, lambda v, r, n, off: (v, r, n, off[:2] + [off[1]] + off[3:])), "increasing"),
        "segment shorter than 5 bytes": (_with_index(good, lambda v, r, n, off: (v, r, n, off[:2] + [off[1] + 4] + off[3:])), "shorter"),
        "segment without its marker": (_with_index(good, lambda v, r, n, off: (v, r, n, off[:2] + [off[2] - 1] + off[3:])), "00 00 FF FF"),
        "tail not an empty final block": (_with_payload(good, lambda p: p[:o[-1]] + b"\x02" + p[o[-1] + 1:]), "tail"),
        "tail too long": (_with_payload(good, lambda p: p + b"\0"), "tail"),
        "tail too short": (_with_payload(good, lambda p: p[:-1]), "tail"),
        "offset past the payload": (_with_index(good, lambda v, r, n, off: (v, r, n, off[:-1] + [len(png.parse_png(good).zlib_stream) + 1])),
                                    "past"),
        "second ttSG": (_rebuild(good, second_index), "at most one"),
        "ttSG after IDAT": (_rebuild(good, move_index_after_idat), "after the IDAT"),
        "short body": (_rebuild(good, lambda ch: [[k, b[:8]] if k == b"ttSG" else [k, b] for k, b in ch]), "fixed fields"),
    }
    return lines, good, files


def test_every_refusal_of_read_segments_is_a_value_error_and_parse_png_ignores_the_chunk():
    lines, good, files = _corrupted()
    assert png.parse_files([good], "require")[0].segments == png.read_segments(good)
    for reason, (data, word) in files.items():
        for mode in ("auto", "require"):
            with pytest.raises(ValueError) as e:
                png.parse_files([good, data], mode)
            assert word in str(e.value), (reason, str(e.value))
        with pytest.raises(ValueError):
            png.read_segments(data)
        assert png.parse_files([data], "ignore")[0].segments is None
        info = png.parse_png(data, verify_crc=True)                      # as any ancillary chunk: ignored
        if not reason.startswith("tail"):                                # (those three have another stream)
            assert zlib.decompress(info.zlib_stream) == lines, reason


def test_segments_modes_on_files_without_an_index():
    _, _, plain = _plain(5, 1, 1, "sub")
    assert png.parse_files([plain], "auto")[0].segments is None and png.parse_files([plain], "ignore")[0].segments is None
    with pytest.raises(ValueError, match="no segment index"):
        png.parse_files([png.segment_png(plain, 2), plain], "require")
    with pytest.raises(ValueError, match="segments"):
        png.parse_files([plain], "sometimes")


def test_the_malformed_list_fails_zlib_too_where_a_status_is_forced():
    """The cases the device tests expect a status for are wrong for zlib as well: their segments do not inflate alone to
    their rows."""
    for name, payload, h, w, c, (rows, offsets), status in S.malformed_cases():
        if status is None:
            continue
        stride = 1 + w * c
        lines = None
        try:
            lines = zlib.decompress(payload)
        except zlib.error:
            pass
        bad = [k for k in range(len(offsets) - 1)
               if lines is None or not S.inflates_alone(payload, offsets[k], offsets[k + 1], lines[k * rows * stride:(k + 1) * rows * stride])]
        assert bad, name


# --------------------------------------------------------------------------------------------------------------- the tool
def _tree(tmp_path):
    src = tmp_path / "src"
    (src / "a" / "b").mkdir(parents=True)
    files = {}
    for i, (rel, (h, w, c)) in enumerate({"rgb.png": (37, 53, 3), "a/seg.PNG": (65, 3, 1), "a/b/depth.png": (130, 9, 3)}.items()):
        arr, _, data = _plain(h, w, c, P.FILTERS[i])
        (src / rel).write_bytes(data)
        files[rel] = (arr, data)
    (src / "a" / "notes.txt").write_bytes(b"not a picture")
    (src / "a" / "b" / "palette.png").write_bytes(P.png_file(2, 2, 1, zlib.compress(bytes(6)), colour=3))
    return src, files


def test_cli_mirrors_a_tree_in_process(tmp_path, capsys):
    src, files = _tree(tmp_path)
    dst = tmp_path / "dst"
    assert png_segment.main([str(src), str(dst), "--rows", "7", "--workers", "1"]) == 0
    out = capsys.readouterr()
    assert "3 files segmented at 7 rows per segment" in out.out and "1 other files copied" in out.out and "1 PNG files left unchanged" in out.out
    assert "palette.png" in out.err
    for rel, (arr, data) in files.items():
        got = (dst / rel).read_bytes()
        assert got == png.segment_png(data, 7) and png.read_segments(got).rows_per_segment == 7
    assert (dst / "a" / "notes.txt").read_bytes() == b"not a picture"
    assert (dst / "a" / "b" / "palette.png").read_bytes() == (src / "a" / "b" / "palette.png").read_bytes()
    with pytest.raises(SystemExit):
        png_segment.main([str(src), str(src / "inside")])
    with pytest.raises(SystemExit):
        png_segment.main([str(src), str(dst), "--rows", "0"])
    assert png_segment.MAX_WORKERS == 16 and png_segment.DEFAULT_ROWS >= 1


def test_cli_as_a_module_with_a_pool_and_on_one_file(tmp_path):
    src, files = _tree(tmp_path)
    dst = tmp_path / "dst"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "thinktwice_amd.png_segment", str(src), str(dst), "--workers", "2", "--level", "1"],
                         capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-2000:]
    assert f"3 files segmented at {png_segment.DEFAULT_ROWS} rows per segment" in run.stdout
    for rel, (arr, data) in files.items():
        assert (dst / rel).read_bytes() == png.segment_png(data, png_segment.DEFAULT_ROWS, 1)
    one = tmp_path / "one.png"
    assert png_segment.main([str(src / "rgb.png"), str(one), "--rows", "64"]) == 0
    assert one.read_bytes() == png.segment_png(files["rgb.png"][1], 64)
