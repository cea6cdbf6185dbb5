"""CPU, build container only: golden F22 is exactly what the reference's own CarlaDataset, DistributedGroupSampler and
DistributedSampler produce.  tests/golden/gen_f22_dataset.py --check re-runs them (the reference's modules under the stand-ins
of ref_stubs.py and the few the script sets) in a subprocess -- the stand-in modules must not leak into this pytest process --
and compares every array with the committed file bit for bit."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import ref_stubs  # noqa: E402


@pytest.mark.skipif(not ref_stubs.reference_available(), reason="needs the reference checkout (build container only)")
def test_committed_golden_f22_is_what_the_reference_produces():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_f22_dataset.py"), "--check"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "bit-identical (149 arrays)" in r.stdout
