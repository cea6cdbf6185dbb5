"""The inflate core (thinktwice_amd/csrc/png_inflate.h) on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: the
stand-alone tools/png_host_check.cpp, built here with -fsanitize=address,undefined and run as a child process over the case
file of tests/png_cases.py.  This is where the malformed streams meet the code first: every buffer of the checker is a heap
block of the exact size, so an access outside the stream, the scanlines or the image is a sanitizer report, and any report
fails the run.  The device test of the malformed list (test_png_decode.py) uses the identical cases."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_tool  # noqa: E402
import png_cases as P  # noqa: E402


def test_inflate_core_under_sanitizers_over_every_case(tmp_path):
    exe, cases = host_tool.build("png_host_check", tmp_path, sanitize=True), str(tmp_path / "cases.bin")
    count = P.write_case_file(cases)
    assert count == len(P.good_cases()) + len(P.malformed_cases())
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    lines = run.stdout.splitlines()
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert lines[-1] == f"{count} cases, 0 failed"
    assert sum(l.startswith("ok  ") for l in lines) == count
