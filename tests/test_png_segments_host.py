"""The segment inflate (thinktwice_amd/csrc/png_inflate.h: inflate_segment, inflate_span) on the CPU under AddressSanitizer
and UndefinedBehaviorSanitizer: the stand-alone tools/png_segment_host_check.cpp, built here with
-fsanitize=address,undefined and run as a child process over the case file of tests/png_segment_cases.py.  This is where the
malformed indices and segments meet the code first: every segment's input and every image's scanlines are heap blocks of the
exact size, so an access outside them is a sanitizer report, and the checker itself fails a case in which a segment changed
a byte outside its own rows.  The device tests (test_png_segments.py) use the identical cases."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_tool  # noqa: E402
import png_segment_cases as S  # noqa: E402


def test_segment_inflate_under_sanitizers_over_every_case(tmp_path):
    exe, cases = host_tool.build("png_segment_host_check", tmp_path, sanitize=True), str(tmp_path / "cases.bin")
    count = S.write_case_file(cases)
    assert count == len(S.good_cases()) + len(S.malformed_cases())
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    lines = run.stdout.splitlines()
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert lines[-1] == f"{count} cases, 0 failed"
    assert sum(l.startswith("ok  ") for l in lines) == count
