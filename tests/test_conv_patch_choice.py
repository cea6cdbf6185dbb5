"""tt_conv2d_plan (host only, no device) answers for the pair-format 3 x 3 layers that stage their input as halo patches
(csrc/conv_x3_patch.hip; csrc/conv_choose.cpp choose_x3_patch): the family from kPatchMinRows output rows on, the per-tap tiles below it
and on every edge of the kernel's contract."""
import importlib.util
import json
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_spec = importlib.util.spec_from_file_location("conv_choice_sweep", os.path.join(ROOT, "tools", "conv_choice_sweep.py"))
sweep = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sweep)

PATCH64 = "conv_x3_run3_kernel<64, patch> pre-split A"
PATCH32 = "conv_x3_run3_kernel<32, patch> pre-split A"
TILE64 = "conv_igemm_glds_kernel<float, 64, 8, 1, 128, 2, false, true> pre-split A"
TILE32 = "conv_igemm_glds_kernel<float, 32, 8, 1, 128, 2, false, true> pre-split A"
MIN_ROWS = int(re.search(r"constexpr int kPatchMinRows = (\d+);",
                         open(os.path.join(ROOT, "thinktwice_amd", "csrc", "conv_choose.h")).read()).group(1))


def _plan(N, H, W, cin, cout, k=3, over=None, **kw):
    """Label (or "ERROR: text") of the pair-format bf16x3 layer; `over`: descriptor fields set after ops.conv2d's."""
    from thinktwice_amd import _lib
    L = _lib.lib()
    row, _ = sweep.describe(sweep.D("patch", N, H, W, cin, cout, k=k, x3=True, in_pair=True, **kw), L)
    row.update(over or {})
    return sweep.plan_label(L, sweep.dict_to_desc(row))


def test_the_threshold_is_above_the_recorded_table():
    assert MIN_ROWS > 8192 and MIN_ROWS % 128 == 0


def test_the_labels_start_with_a_prefix_the_bench_counts_three_mfmas_for():
    from thinktwice_amd import bench_forward
    for label in (PATCH64, PATCH32):
        assert bench_forward.mfma_per_product(label, "bf16x3") == 3 and bench_forward.mfma_per_product(label, "bf16x3h") == 3


def test_both_sides_of_the_row_threshold():
    h = MIN_ROWS // 128
    for cout, new, old in ((64, PATCH64, TILE64), (12, PATCH32, TILE32), (8, PATCH32, TILE32), (32, PATCH32, TILE32)):
        assert _plan(1, h, 128, 64, cout) == new, cout
        assert _plan(1, h - 1, 128, 64, cout) == old, cout
        assert _plan(1, h, 127, 64, cout) == old, cout              # one row short
    assert _plan(1, h, 128, 32, 32, out_pair=True) == PATCH32
    assert _plan(1, h, 128, 96, 64, out_pair=True) == PATCH64
    assert _plan(1, h, 128, 128, 64) == TILE64                       # 64-wide from K = 1152 on: the per-tap tile
    assert _plan(1, h, 128, 128, 32) == PATCH32
    assert _plan(2, h // 2, 128, 64, 64) == PATCH64                  # rows count over the batch


def test_the_model_layers():
    # the fused seg head and ResNet layer1's conv2 at B = 8 (64 images) and B = 1 (8 images)
    for N in (64, 8):
        assert _plan(N, 224, 448, 64, 12) == PATCH32
        assert _plan(N, 112, 224, 64, 64, out_pair=True) == PATCH64


def test_each_contract_edge_keeps_a_pre_split_tile():
    h = 4 * MIN_ROWS // 128                                           # enough rows for the strided layer too
    assert _plan(1, h, 128, 64, 64) == PATCH64
    assert _plan(1, h, 128, 64, 64, stride=2) == TILE64
    assert _plan(1, h, 128, 64, 64, pad=2, over=dict(dil=2)) == TILE64
    assert _plan(1, h, 128, 64, 64, k=1) == TILE64
    assert _plan(1, h, 128, 64, 128) == "conv_igemm_glds_kernel<float, 128, 8, 1, 128, 2, false, true> pre-split A"
    assert _plan(1, h, 128, 64, 64, res=1) == TILE64
    assert _plan(1, h, 128, 64, 64, k=(3, 1), pad=0) == TILE64
    # a window inside a wider buffer is inside the contract on the 16-channel groups, the existing error off them
    assert _plan(1, h, 128, 64, 64, cs=128, in_coff=32) == PATCH64
    assert _plan(1, h, 128, 64, 64, cs=96, in_coff=8) == \
        f"ERROR: tt_conv2d_fwd: pair-format layer outside the LDS-DMA bf16x3 kernel's contract (M={h * 128} Cin=64 Cout=64)"


def test_the_recorded_pair_rows_keep_their_labels():
    from thinktwice_amd import _lib
    L = _lib.lib()
    rows = {r["name"]: r for r in json.load(open(os.path.join(ROOT, "tests", "conv_choice_cases.json")))["cases"]}
    for name, label in (("pair M=2048", TILE64), ("pair Cout=8", TILE32), ("pair Cout=32", TILE32), ("pair 64-wide", TILE64)):
        assert rows[name]["label"] == label
        assert sweep.plan_label(L, sweep.dict_to_desc(rows[name]["desc"])) == label, name
