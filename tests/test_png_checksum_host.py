"""The checksum source (thinktwice_amd/csrc/png_checksum.h) and the inflate's trailer hand-out (png_inflate.h) on the CPU under
AddressSanitizer and UndefinedBehaviorSanitizer: the stand-alone tools/png_checksum_host_check.cpp, built here with
-fsanitize=address,undefined and run as a child process over the case file of tests/png_checksum_cases.py -- the op-level
lengths, extremes and many-range tables, and every good, corrupted and malformed stream of the device test
(test_png_checksum.py).  The checker runs the tile table builder, every lane's slice, the workgroup's combine and the fold, lane
by lane; every range, stream and chunk body is a heap block of its exact size, so a read past a range's end is a sanitizer
report, and any report fails the run."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_tool  # noqa: E402
import png_checksum_cases as K  # noqa: E402


def test_checksum_source_under_sanitizers_over_every_case(tmp_path):
    exe, cases = host_tool.build("png_checksum_host_check", tmp_path, sanitize=True), str(tmp_path / "cases.bin")
    count = K.write_case_file(cases)
    assert count > 250
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    lines = run.stdout.splitlines()
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert lines[-1] == f"{count} cases, 0 failed"
    assert sum(l.startswith("ok  ") for l in lines) == count
