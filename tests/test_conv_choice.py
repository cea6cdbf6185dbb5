"""Which kernel a convolution runs on is decided in one host function (csrc/conv_choose.cpp) that tt_conv2d_plan answers from
without a device.  tests/conv_choice_cases.json holds what the dispatch chose -- on an MI355X, through ops.conv2d / ops.gather_conv
(tools/conv_choice_sweep.py --launch) -- at the commit before the chooser existed, over a case list that reaches every launch site
and both sides of every threshold; the chooser must reproduce it, and the label expectations the GPU tests of tests/test_conv.py
hold, row for row.  Its last rows were never launched: they are that commit's tt_conv2d_splitk_slices (host only) on layers beyond
the bounds at which ops.conv2d asks, with the workspace the answer sizes attached."""
import ctypes
import json
import os

import pytest
import torch

from thinktwice_amd import ops
from tools import conv_choice_sweep as sweep

ROWS = json.load(open(os.path.join(os.path.dirname(__file__), "conv_choice_cases.json")))["cases"]

X3_SPLITK = "conv_igemm_glds_kernel<float, 64, 8, 1, 128, 2, false, true> split-K"


def _lib():
    from thinktwice_amd import _lib
    return _lib.lib()


def _plan(case):
    """Label (or "ERROR: text") tt_conv2d_plan gives the descriptor ops.conv2d / ops.gather_conv build for a sweep-style case."""
    return ops.plan_label(sweep.dict_to_desc(sweep.describe(case, _lib())[0]))


def test_the_recorded_choices_are_reproduced():
    L = _lib()
    assert len(ROWS) > 100
    bad = []
    for r in ROWS:
        got = ops.plan_label(sweep.dict_to_desc(r["desc"]))
        if "label" not in r:      # a query-only row: with the slices it asked for the layer splits K, with none it does not
            if got.startswith("ERROR") or ("split-K" in got) != (r["query"] > 0):
                bad.append((r["name"], got, r["query"]))
        elif got != r["label"]:
            bad.append((r["name"], got, r["label"]))
        if "query" in r:        # what the caller asked before it attached the workspace
            asked = {k: v for k, v in r["desc"].items() if k not in ("splitk_ws", "splitk_slices")}
            n = int(L.tt_conv2d_splitk_slices(ctypes.byref(sweep.dict_to_desc(asked))))
            if n != r["query"]:
                bad.append((r["name"], n, r["query"]))
    assert not bad, bad
    # the far bounds of the bf16x3 split-K tile, on both sides: counts of the commit before the chooser
    asked = {r["name"]: (r["query"], ops.plan_label(sweep.dict_to_desc(r["desc"]))) for r in ROWS if "label" not in r}
    for name, n in (("query x3 M=8192", 2), ("query x3 K=1024", 4), ("query x3 255 tiles", 2), ("query x3 32 taps", 4)):
        assert asked[name] == (n, X3_SPLITK), (name, asked[name])
    for name in ("query x3 M=8193", "query x3 K=992", "query x3 256 tiles", "query x3 33 taps", "query x3 pixel shuffle"):
        assert asked[name][0] != asked[name.replace("8193", "8192").replace("992", "1024").replace("256", "255").replace("33", "32")
                                       .replace("pixel shuffle", "K=1024")][0] and asked[name][1] != X3_SPLITK, (name, asked[name])


def test_the_case_list_of_the_sweep_is_the_recorded_one():
    """The committed table was recorded from tools/conv_choice_sweep.py's list: same names, same descriptors."""
    L = _lib()
    cases = sweep.CASES + sweep.QUERIES
    assert [c["name"] for c in cases] == [r["name"] for r in ROWS]
    for c, r in zip(cases, ROWS):
        assert {k: v for k, v in sweep.describe(c, L)[0].items() if v} == r["desc"], c["name"]


def test_the_label_tables_of_the_gpu_tests_hold():
    """PIPE_CASES, SPLITK_X3_CASES, PAIR_CASES, the run-staged sparse cases and the per-device launch-state labels of
    tests/test_conv.py, imported (not copied) and replayed through tt_conv2d_plan."""
    import test_conv as T
    from thinktwice_amd import weights  # noqa: F401  (test_conv's helpers import it lazily)
    D, S = sweep.D, sweep.S
    for i, (N, H, W, Cin, Cout, k, stride, _act, _bn, res, window, kern) in enumerate(T.PIPE_CASES):
        win = dict(cs=Cin + 64, in_coff=32) if window else {}
        assert _plan(D(f"pipe {i}", N, H, W, Cin, Cout, k=k, stride=stride, x3=True, res=res, **win)).replace(" + tail", "") == kern, i
    for i, (N, H, W, Cin, Cout, k, _act, _bn, res, window) in enumerate(T.SPLITK_X3_CASES):
        win = dict(cs=Cin + 64, in_coff=32) if window else {}
        assert _plan(D(f"splitk {i}", N, H, W, Cin, Cout, k=k, x3=True, res=res, **win)) == X3_SPLITK, i
        exact = _plan(D(f"splitk exact {i}", N, H, W, Cin, Cout, k=k, res=res, **win))
        assert "split-K" in exact and "conv_igemm_kernel" in exact, (i, exact)
    for i, (N, H, W, Cin, Cout, k, stride, _act) in enumerate(T.PAIR_CASES):
        assert "pre-split A" in _plan(D(f"pair {i}", N, H, W, Cin, Cout, k=k, stride=stride, x3=True, in_pair=True)), i
    sparse = next(m for m in T.test_run_staged_sparse_conv_on_cell_ordered_rulebooks.pytestmark if m.name == "parametrize").args[1]
    for Cin, Cout, stride, occ, dims in sparse:
        g = torch.Generator().manual_seed(Cin + Cout + stride)
        live = T._grid_rulebook(*dims, occ, stride, g)[0].shape[0]
        if live >= 2048:          # (the gather_conv of that test passes no stride: the run kernel's own default)
            assert _plan(S("runs", live + 300, Cin, Cout, x3=True)).startswith("sp_conv_runs_kernel"), (Cin, Cout, stride)
    # test_launch_state_is_per_device: its tensors, in its order
    g = torch.Generator().manual_seed(23)
    for shape in ((1, 129, 256, 128), (1, 129, 256, 128), (256, 1, 1, 128), (256, 3, 3, 128)):
        T._mk(shape, g)
    rows = T._grid_rulebook(2, 10, 60, 60, 0.10, 1, g)[0].shape[0]
    got = [_plan(D("1x1", 1, 129, 256, 128, 256, x3=True)), _plan(D("3x3", 1, 129, 256, 128, 256, k=3, x3=True)),
           _plan(D("h2", 1, 129, 256, 128, 256, k=3, dt="f16", h2=True)), _plan(S("sparse", rows, 32, 32, x3=True))]
    assert got == T.LAUNCH_STATE_LABELS, got


def test_pair_ok_over_the_grid():
    """ops.pair_ok from plain numbers: more than 4096 rows (up to there the non-pair consumer would be the exact-f32 small kernel, so
    the caller is stricter than the library, which takes pair format from 2048 rows) and a layer the library takes.  Wherever it says
    yes, the library plans the pair-format layer the sweep tool describes; the answers themselves are stated here."""
    yes = 0
    for rows in (2048, 4096, 4097, 65536):
        for cin in (16, 32, 48, 64, 96):
            for cout in (4, 8, 12, 32, 48, 64, 96, 256):
                for k in (1, 3):
                    ok = ops.pair_ok(rows, cin, cout, k * k)
                    assert ok == (rows > 4096 and cin % 32 == 0 and k * k * cin >= 64 and cout not in (4, 48)), (rows, cin, cout, k)
                    if ok:
                        yes += 1
                        label = _plan(sweep.D("pair", 1, 1, rows, cin, cout, k=k, pad=k // 2, x3=True, in_pair=True))
                        assert "pre-split A" in label, (rows, cin, cout, k, label)
    assert yes == 2 * 5 * 6         # rows 4097 / 65536 x (cin 32 / 64 / 96 with k = 3, cin 64 / 96 with k = 1) x cout 8 / 12 / 32 / 64 / 96 / 256


def test_the_refusals_keep_their_texts():
    assert _plan(sweep.D("h2", 1, 1, 300, 32, 64, dt="f16", h2=True)) == \
        "ERROR: tt_conv2d_fwd: weight_h2 layer outside the h2 kernel's contract (Cin=32 KH*KW=1)"
    assert _plan(sweep.D("pair", 1, 64, 128, 64, 48, k=3, x3=True, in_pair=True)) == \
        "ERROR: tt_conv2d_fwd: pair-format layer outside the LDS-DMA bf16x3 kernel's contract (M=8192 Cin=64 Cout=48)"
    L = _lib()
    d = sweep.dict_to_desc(sweep.describe(sweep.D("x", 1, 1, 300, 64, 64), L)[0])
    assert L.tt_conv2d_plan(ctypes.byref(d), None, 0) != 0 and b"tt_conv2d_plan" in L.tt_last_error()
    d.in_ = None
    buf = ctypes.create_string_buffer(96)
    assert L.tt_conv2d_plan(ctypes.byref(d), buf, 96) != 0 and L.tt_last_error() == b"tt_conv2d_fwd: null pointer"


def _family(label):
    return label.split("<")[0] + (" split-K" if "split-K" in label else "")


@pytest.mark.gpu
def test_a_launch_runs_the_kernel_the_plan_names():
    """One real launch per kernel family -- the smallest recorded case of each -- reports the label tt_conv2d_plan gives its
    descriptor."""
    by_name = {c["name"]: c for c in sweep.CASES}
    pick = {}
    for r in ROWS:
        if "label" not in r or r["label"].startswith("ERROR"):
            continue
        d = r["desc"]
        work = d["N"] * d["OH"] * d["OW"] * d["Cout"] * d["KH"] * d["KW"] * d["Cin"]
        fam = _family(r["label"])
        if fam not in pick or work < pick[fam][0]:
            pick[fam] = (work, r["name"])
    assert len(pick) >= 10, sorted(pick)
    for rec in sweep.run_launch([by_name[name] for _, name in sorted(pick.values())]):
        assert rec["label"] == ops.plan_label(sweep.dict_to_desc(rec["desc"])), rec["name"]
