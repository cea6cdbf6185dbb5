"""The JPEG encoder core (thinktwice_amd/csrc/jpeg_core.h) on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: the
stand-alone tools/jpeg_encode_host_check.cpp, built here with -fsanitize=address,undefined and run as a child process over
the case file of tests/jpeg_encode_cases.py.  The tool encodes every case with the host build of the device's source (one
thread playing the 64 lanes) and writes the files out; this module holds them byte for byte to tests/jpeg_ref.py, checks the
size bounds, and guards fidelity and size against PIL (libjpeg) at the same quality, subsampling and standard tables.

Fidelity.  PSNR of PIL's decode of our file against the source, beside PIL's own file.  The hard condition: ours at quality q
is no worse than PIL's at q - 5 (q <= 5: q - 1, at least 1).  The regression guard: PIL's PSNR minus ours at the same q,
measured on these host-built bytes (which are the device's) and asserted at the measured gap + 0.1 dB (PSNR_GAP_DB, also in
profiles/jpeg_encode.txt).  Size: our bytes over PIL's with optimize=False and restart_marker_rows equal to ours, asserted at
the measured ratio + 5 % (SIZE_RATIO): a guard against regression, not a target."""
import functools
import io
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_tool  # noqa: E402
import jpeg_encode_cases as E  # noqa: E402
import jpeg_ref  # noqa: E402

HEADER = {1: 330, 3: 613}
GUARDED = ("camera_64x96x3_q90_420_r1", "camera_64x96x3_q90_444_r2", "hud_48x80x3_q90_420_r1", "hud_48x80x3_q90_444_r1",
           "quality_24x40x3_q1_420_r1", "quality_24x40x3_q50_420_r1", "quality_24x40x3_q90_420_r1", "quality_24x40x3_q100_420_r1",
           "noise_32x32x3_q100_444_r1", "image_17x33x1_q90_420_r1")
# measured (PIL's PSNR - ours in dB, our bytes / PIL's bytes) per guarded case
PSNR_GAP_DB = {"camera_64x96x3_q90_420_r1": -0.014, "camera_64x96x3_q90_444_r2": 0.001, "hud_48x80x3_q90_420_r1": -0.017,
               "hud_48x80x3_q90_444_r1": -0.029, "quality_24x40x3_q1_420_r1": 0.000, "quality_24x40x3_q50_420_r1": -0.017,
               "quality_24x40x3_q90_420_r1": 0.062, "quality_24x40x3_q100_420_r1": 0.225, "noise_32x32x3_q100_444_r1": 0.005,
               "image_17x33x1_q90_420_r1": -0.001}
SIZE_RATIO = {"camera_64x96x3_q90_420_r1": 0.9799, "camera_64x96x3_q90_444_r2": 0.9839, "hud_48x80x3_q90_420_r1": 0.9940,
              "hud_48x80x3_q90_444_r1": 0.9948, "quality_24x40x3_q1_420_r1": 0.9758, "quality_24x40x3_q50_420_r1": 1.0099,
              "quality_24x40x3_q90_420_r1": 1.0591, "quality_24x40x3_q100_420_r1": 1.0451, "noise_32x32x3_q100_444_r1": 0.9953,
              "image_17x33x1_q90_420_r1": 0.9917}


def run_checker(sanitize, extra=()):
    """Builds the checker, runs it over every case (and `extra`) -> ([file bytes], {name: (bytes, intervals, bound, header)},
    the run)."""
    with tempfile.TemporaryDirectory() as tmp:
        cases, out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out")
        os.mkdir(out)
        exe = host_tool.build("jpeg_encode_host_check", tmp, sanitize)
        count = E.write_case_file(cases, extra)
        run = subprocess.run([exe, cases, out], capture_output=True, text=True)
        files = [open(os.path.join(out, f"{i}.jpg"), "rb").read() for i in range(count)] if run.returncode == 0 else []
    stats = {}
    for line in run.stdout.splitlines():
        m = re.fullmatch(r"ok   (\S+): bytes (\d+) intervals (\d+) bound (\d+) header (\d+)", line)
        if m:
            stats[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    return files, stats, run


@functools.lru_cache(maxsize=None)
def _checked():
    return run_checker(sanitize=True)


def test_encoder_core_under_sanitizers_stays_inside_every_buffer():
    files, stats, run = _checked()
    count = len(E.cases())
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.splitlines()[-1] == f"{count} cases, 0 failed"            # (the tool's guard bytes are part of its verdict)
    assert len(stats) == count and len(files) == count
    for (name, img, *_), f in zip(E.cases(), files):
        size, _, bound, header = stats[name]
        assert size == len(f) and header == HEADER[img.shape[2]] and header + 2 <= len(f) <= bound, (name, stats[name])


def test_every_file_is_byte_equal_to_the_numpy_restatement():
    files, _, _ = _checked()
    for (name, img, quality, sub, rr), f in zip(E.cases(), files):
        want = jpeg_ref.encode(img, quality, sub, rr)
        assert f == want, f"{name}: {len(f)} bytes, the restatement {len(want)}; first difference at " \
                          f"{next((i for i, (a, b) in enumerate(zip(f, want)) if a != b), min(len(f), len(want)))}"


def test_the_bound_counts_the_format():
    """header + 432 bytes a block (64 coefficients of at most 16 + 11 bits, every byte stuffed) + a marker per interval."""
    _, stats, _ = _checked()
    for name, img, quality, sub, rr in E.cases():
        h, w, c = img.shape
        m = 16 if (c == 3 and sub == "420") else 8
        mx, my = -(-w // m), -(-h // m)
        blocks = mx * my * (1 if c == 1 else 6 if m == 16 else 3)
        n_int = -(-my // rr)
        assert stats[name][1:] == (n_int, HEADER[c] + 432 * blocks + 2 * n_int, HEADER[c]), (name, stats[name])


def test_the_cases_as_one_table_walk_the_shared_slot_arithmetic():
    """The tool's batch pass (csrc/file_slots.h under the sanitizers): all cases in one workspace and one file buffer, every file
    equal to the case's own.  A unit is a group of 64 blocks, a part a restart interval."""
    _, _, run = _checked()
    m = re.fullmatch(r"batch: (\d+) images, (\d+) units, (\d+) parts, (\d+) workspace bytes: ok", run.stdout.splitlines()[-2])
    assert m, run.stdout.splitlines()[-2:]
    units = parts = 0
    for name, img, quality, sub, rr in E.cases():
        h, w, c = img.shape
        mcu = 16 if (c == 3 and sub == "420") else 8
        mx, my = -(-w // mcu), -(-h // mcu)
        units += -(-(mx * my * (1 if c == 1 else 6 if mcu == 16 else 3)) // 64)
        parts += -(-my // rr)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (len(E.cases()), units, parts)


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def _pil(img, quality, sub, rr=0):
    from PIL import Image
    out = io.BytesIO()
    kw = {"restart_marker_rows": rr} if rr else {}
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img).save(out, "JPEG", quality=quality, subsampling={"444": 0, "420": 2}[sub],
                                                                      optimize=False, **kw)
    return out.getvalue()


def _decoded(f, shape):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(f))).reshape(shape)


def measurements():
    """{name: (our PSNR, PIL's at the same quality, PIL's at the hard condition's quality, our bytes, PIL's bytes)}"""
    files, _, _ = _checked()
    out = {}
    for (name, img, quality, sub, rr), f in zip(E.cases(), files):
        lower = max(1, quality - 1) if quality <= 5 else quality - 5
        same = _pil(img, quality, sub)
        out[name] = (_psnr(_decoded(f, img.shape), img), _psnr(_decoded(same, img.shape), img),
                     _psnr(_decoded(_pil(img, lower, sub), img.shape), img), len(f), len(_pil(img, quality, sub, rr)))
    return out


def test_fidelity_is_no_worse_than_pil_five_quality_steps_down_and_the_gap_at_the_same_quality_is_guarded():
    got = measurements()
    for name, (ours, same, lower, _, _) in got.items():
        print(f"{name}: PSNR {ours:.3f} dB, PIL {same:.3f} dB at the same quality, {lower:.3f} dB at the lower one")
        assert same >= lower, (name, same, lower)           # the premise, on PIL's files alone: its PSNR falls with the quality
        assert ours >= lower, (name, ours, lower)
    assert set(PSNR_GAP_DB) == set(GUARDED)
    for name, gap in PSNR_GAP_DB.items():
        ours, same, _, _, _ = got[name]
        assert same - ours <= gap + 0.1, (name, same - ours, gap)


def test_file_size_regression_guard_against_pil():
    got = measurements()
    assert set(SIZE_RATIO) == set(GUARDED)
    for name, ratio in SIZE_RATIO.items():
        _, _, _, ours, pil = got[name]
        print(f"{name}: {ours} bytes, {ours / pil:.4f} of PIL's {pil}")
        assert ours / pil <= ratio * 1.05, (name, ours / pil, ratio)
