"""CPU, build container only: golden F21's arrays are exactly what the reference's own loaders return for its files.
tests/golden/gen_f21_png_decode.py --check writes the committed file bytes into a temporary dataset tree and runs
LoadMultiImages.load_img and LoadSeg.load_img over them (the reference's loading.py under the stand-ins of ref_stubs.py, PIL the
real one) in a subprocess -- the stand-in modules must not leak into this pytest process -- and compares bit for bit."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import ref_stubs  # noqa: E402


def _has_pil():
    try:
        import PIL.Image  # noqa: F401
        return True
    except ImportError:
        return False


@pytest.mark.skipif(not (ref_stubs.reference_available() and _has_pil()),
                    reason="needs the reference checkout and PIL (build container only)")
def test_committed_golden_f21_is_what_the_reference_loads():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_f21_png_decode.py"), "--check"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "bit-identical (3 files)" in r.stdout


def test_golden_f21_holds_what_it_is_for():
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "f21_png_decode.npz"))
    used = set()
    for kind, shape in (("rgb", (45, 80, 3)), ("depth", (45, 80, 3)), ("seg", (45, 80))):
        assert g[f"{kind}_array"].shape == shape and g[f"{kind}_array"].dtype == np.uint8
        assert g[f"{kind}_file"].tobytes()[:8] == b"\x89PNG\r\n\x1a\n"
        used |= set(g[f"{kind}_filters"].tolist())
    assert used >= {0, 1, 2, 4}
