"""Where the chooser (csrc/conv_choose.cpp) hands a sparse 3x3x3 layer to the weight-resident kernel of csrc/sp_conv_l2.hip: from
kSpL2MinRows allocated rows on, for bf16x3 layers with 16 / 32 input and 16 / 32 / 64 output channels -- and nowhere else.  Host only,
through tt_conv2d_plan with the case builder of tools/conv_choice_sweep.py."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_spec = importlib.util.spec_from_file_location("conv_choice_sweep", os.path.join(ROOT, "tools", "conv_choice_sweep.py"))
sweep = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sweep)
S = sweep.S

MIN_ROWS = int(re.search(r"kSpL2MinRows\s*=\s*(\d+)", open(os.path.join(ROOT, "thinktwice_amd", "csrc", "conv_choose.h")).read()).group(1))
GLDS = "conv_igemm_glds_kernel<{}, {}, {}, {}, 128, 2, true, {}>"


def _plan(case):
    from thinktwice_amd import _lib
    L = _lib.lib()
    return sweep.plan_label(L, sweep.dict_to_desc(sweep.describe(case, L)[0]))


def _old_label(Cin, Cout, stride):
    """What these layers ran on before: the run-staged kernel for stride-1 32 -> 32 / 64, else the gathered LDS-DMA tile"""
    if Cin == 32 and stride == 1 and Cout in (32, 64):
        return f"sp_conv_runs_kernel<{Cout // 32}, 8, 1>"
    bn = 32 if Cout <= 32 else 64
    return GLDS.format("float", bn, 8, 1, "true")


def test_the_threshold_is_within_the_bounds_the_levels_need():
    """at most 65,536: the batch-1 allocation of the 16-channel level must take the new kernel"""
    assert 2048 < MIN_ROWS <= 65536


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cout", [16, 32, 64])
@pytest.mark.parametrize("Cin", [16, 32])
def test_both_sides_of_the_row_threshold(Cin, Cout, stride):
    assert _plan(S("at", MIN_ROWS, Cin, Cout, stride=stride, x3=True)) == f"sp_conv_runs_l2_kernel<{Cin}>"
    assert _plan(S("far above", 1 << 22, Cin, Cout, stride=stride, x3=True)) == f"sp_conv_runs_l2_kernel<{Cin}>"
    assert _plan(S("below", MIN_ROWS - 1, Cin, Cout, stride=stride, x3=True)) == _old_label(Cin, Cout, stride)


@pytest.mark.parametrize("M", [MIN_ROWS, 1 << 20])
def test_the_other_layers_keep_their_kernels_at_any_row_count(M):
    assert _plan(S("64", M, 64, 64, x3=True)) == "sp_conv_runs_kernel<2, 8, 1>"
    assert _plan(S("128", M, 128, 128, x3=True)) == "sp_conv_runs_kernel<2, 4, 2>"
    assert _plan(S("32 -> 128", M, 32, 128, x3=True)) == "sp_conv_runs_kernel<2, 4, 2>"
    assert _plan(S("32 -> 48", M, 32, 48, x3=True)) == GLDS.format("float", 64, 8, 1, "true")
    assert _plan(S("Cin 8", M, 8, 16)).startswith("conv_igemm_kernel<float")        # the input conv (K = 216: no pair-format weights)
    # a tile plan (row_perm), exact f32, 16-bit storage: never the bf16x3 weight-resident kernel
    assert _plan(S("plan", M, 32, 32, x3=True, plan=True)) == GLDS.format("float", 32, 8, 1, "true")
    assert _plan(S("f32", M, 32, 32)).startswith("conv_igemm_kernel<float")
    assert _plan(S("f32 16", M, 16, 16)).startswith("conv_igemm_kernel<float")
    assert _plan(S("bf16", M, 32, 32, dt="bf16")) == GLDS.format("16-bit", 32, 8, 1, "false")
    assert _plan(S("f16", M, 16, 64, dt="f16")) == GLDS.format("16-bit", 64, 8, 1, "false")
