"""The rasteriser's per-pixel rules (thinktwice_amd/csrc/render_raster.h) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: the stand-alone tools/render_host_check.cpp, built here with -fsanitize=address,undefined and run as a
child process over the case file of tests/render_cases.py.  Its canvases and dropped-point counts must equal the numpy
restatement's (tests/render_ref.py) byte for byte, the lists the entry must refuse must be refused, and the run must be clean."""
import functools
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_tool  # noqa: E402
import render_cases as R  # noqa: E402
import render_ref  # noqa: E402


@functools.lru_cache(maxsize=None)
def _checked():
    """Builds the checker, runs it over every case -> ({name: (rc, dropped, canvas or None)}, the run)."""
    with tempfile.TemporaryDirectory() as tmp:
        cases, out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
        exe = host_tool.build("render_host_check", tmp, sanitize=True, extra_flags=("-ffp-contract=off",))
        R.write_case_file(cases)
        run = subprocess.run([exe, cases, out], capture_output=True, text=True)
        data = open(out, "rb").read() if os.path.exists(out) else b""
    got, at = {}, 0
    for c in R.cases("cpu"):
        if at + 12 > len(data):
            break
        rc, dropped = struct.unpack_from("<iq", data, at)
        at += 12
        canvas = None
        if rc == 0:
            n = c.dl.height * c.dl.width * 3
            canvas = np.frombuffer(data, np.uint8, n, at).reshape(c.dl.height, c.dl.width, 3)
            at += n
        got[c.name] = (rc, dropped, canvas)
    return got, run


def test_the_checker_runs_clean_under_the_sanitizers():
    got, run = _checked()
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.splitlines()[-1] == f"{len(R.cases('cpu'))} cases, 0 failed"
    assert len(got) == len(R.cases("cpu"))


@pytest.mark.parametrize("name", [c.name for c in R.cases("cpu") if not c.expect_error])
def test_canvas_and_dropped_points_equal_the_restatement(name):
    got, _ = _checked()
    case = next(c for c in R.cases("cpu") if c.name == name)
    want, dropped = render_ref.render(case.dl)
    rc, got_dropped, canvas = got[name]
    assert rc == 0
    print(f"{name}: {int((canvas != want).any(-1).sum())} pixels differ, dropped {got_dropped} / {dropped}")
    assert got_dropped == dropped
    assert np.array_equal(canvas, want)


def test_refused_lists_are_refused():
    got, _ = _checked()
    errors = [c.name for c in R.cases("cpu") if c.expect_error]
    assert len(errors) >= 12
    for name in errors:
        assert got[name][0] != 0, name


def test_reversed_segments_cover_the_same_pixels():
    got, _ = _checked()
    for hw in (0, 8, 23):
        a, b = got[f"segments_fwd_hw{hw}"][2], got[f"segments_rev_hw{hw}"][2]
        assert np.array_equal(a, b) and (hw == 0 or a.any())
