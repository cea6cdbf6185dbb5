"""Which kernel a weight gradient runs on is decided in one host file (csrc/wgrad_choose.cpp) that tt_conv2d_wgrad_plan and
tt_gather_conv_wgrad_plan answer from without a device.  tests/wgrad_choice_cases.json holds what the launchers chose -- kernel name
with template arguments, grid and LDS bytes, read from one rocprofv3 kernel trace on an MI355X (tools/wgrad_choice_sweep.py --launch,
then --trace) -- at the commit before the chooser existed, over a case list that reaches every kernel family and both sides of every
condition; the chooser must reproduce it row for row."""
import ctypes
import importlib.util
import json
import os

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_spec = importlib.util.spec_from_file_location("wgrad_choice_sweep", os.path.join(ROOT, "tools", "wgrad_choice_sweep.py"))
sweep = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sweep)
ROWS = json.load(open(os.path.join(ROOT, "tests", "wgrad_choice_cases.json")))["cases"]


def _lib():
    from thinktwice_amd import _lib
    return _lib.lib()


def test_the_recorded_choices_are_reproduced():
    L = _lib()
    assert len(ROWS) == len(sweep.runs()) > 120
    bad = []
    for (c, mode), r in zip(sweep.runs(), ROWS):
        assert (c["name"], mode) == (r["name"], r["mode"])
        for x3 in ((mode == "x3",) if c["kind"] == "dense" else (False, True)):     # the gathered layer: one answer under both
            rc, label = sweep.plan_call(L, c, x3)
            got = sweep.parse_label(label) if rc == 0 else L.tt_last_error()
            if rc != 0 or (got["kernel"], got["grid"], got["lds"]) != (r["kernel"], r["grid"], r["lds"]):
                bad.append((r, got))
            # the launch's dynamic LDS is not in a kernel trace: it must be what the named instantiation stages
            elif got["dynamic_lds"] != sweep.stage_bytes(got["kernel"]):
                bad.append((r, got))
    assert not bad, bad


def test_every_kernel_family_and_tile_is_in_the_record():
    kernels = {r["kernel"] for r in ROWS}
    for fam in ("conv_wgrad_kernel", "conv_wgrad_wide_kernel<", "conv_wgrad_lds_kernel<", "gather_wgrad_kernel", "gather_wgrad_wide_kernel<"):
        assert any(k.startswith(fam) for k in kernels), fam
    assert {k for k in kernels if k.startswith("conv_wgrad_lds_kernel")} == \
        {"conv_wgrad_lds_kernel<%d, %d>" % (i, j) for i in (1, 2, 4) for j in (1, 2, 4)}
    assert {k for k in kernels if k.startswith("conv_wgrad_wide_kernel")} == \
        {"conv_wgrad_wide_kernel<%d, %d>" % (i, j) for i in (1, 2, 4) for j in (1, 2, 4) if (i, j) != (2, 2)}


def test_the_case_list_holds_the_cases_of_the_gpu_tests():
    import inspect

    import test_conv_bwd as T
    dense = {(c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["stride"], c["pad"], c["dil"]) for c in sweep.CASES if c["kind"] == "dense"}
    assert set(T.CASES) <= dense and list(T.CASES) == sweep.BWD_CASES
    pairs = next(m for m in T.test_gather_conv_wgrad_matches_dense_sum.pytestmark if m.name == "parametrize").args[1]
    assert list(pairs) == sweep.GATHER_PAIRS
    assert "1500, 1237, 27" in inspect.getsource(T.test_gather_conv_wgrad_matches_dense_sum)       # M, live, taps of the sweep's G rows


def test_the_workspace_queries_are_the_plans_slices():
    """Each workspace query is slices x Cout x taps x cin_pad x 4 of the plan it sizes: the f32 plan for a dense layer (the query
    knows neither x3 nor OW; the LDS-staged kernel's splits are clamped to it), the one plan of a gathered layer."""
    L = _lib()
    for c in sweep.CASES:
        rc, label = sweep.plan_call(L, c, False)
        assert rc == 0, (c["name"], L.tt_last_error())
        p = sweep.parse_label(label)
        taps = c["k"] ** 2 if c["kind"] == "dense" else c["taps"]
        assert sweep.workspace_bytes(L, c) == p["slices"] * c["Cout"] * taps * ((c["Cin"] + 3) // 4 * 4) * 4, c["name"]
        if c["kind"] == "dense":        # under x3 never more slices than that workspace holds
            rc, label = sweep.plan_call(L, c, True)
            assert rc == 0 and sweep.parse_label(label)["slices"] <= p["slices"], c["name"]


def test_the_regrouped_geometry_is_spelled():
    L = _lib()
    by_name = {c["name"]: c for c in sweep.CASES}
    geo = {n: sweep.parse_label(sweep.plan_call(L, by_name[n], True)[1])["geometry"] for n in ("bwd 21", "bwd 22", "bwd 23", "bwd 19")}
    assert geo == {"bwd 21": "N=1 OH=1 OW=160 H=1 W=160",       # 20 rows of 8 pixels: no divisor from 16 on but 20 itself
                   "bwd 22": None,                              # 7 rows of 9 pixels: 15 rows would be needed
                   "bwd 23": "N=1 OH=4 OW=128 H=4 W=128",       # 32 rows of 16 pixels: 8 rows each
                   "bwd 19": "N=1 OH=30 OW=128 H=30 W=128"}     # the linear layer over 3840 rows
    assert sweep.parse_label(sweep.plan_call(L, by_name["bwd 21"], False)[1])["geometry"] is None      # exact f32: never regrouped


def test_the_plan_refuses_what_the_launch_refuses():
    L = _lib()
    c = sweep.CASES[0]
    assert sweep.plan_call(L, c, True, misalign=4)[1].startswith("conv_wgrad_kernel ")     # misaligned x: routed, not refused
    assert sweep.plan_call(L, c, True)[1].startswith("conv_wgrad_lds_kernel<1, 1> ")
    buf = ctypes.create_string_buffer(192)

    def dense(x, ws_bytes, label, label_bytes):       # bwd 0 under x3
        return L.tt_conv2d_wgrad_plan(x, 2, 20, 24, 64, 64, 0, 0x2000, 20, 24, 64, 64, 0, 3, 3, 1, 1, 1, 64, 0, 0x3000, 0x4000, ws_bytes,
                                      1, label, label_bytes)
    assert dense(0x1000, 1 << 30, buf, 192) == 0
    assert dense(0x1000, 1 << 30, None, 0) != 0 and b"tt_conv2d_wgrad_plan" in L.tt_last_error()
    assert dense(0x1000, 16, buf, 192) != 0 and L.tt_last_error() == b"tt_conv2d_wgrad: workspace too small"
    assert dense(None, 1 << 30, buf, 192) != 0 and L.tt_last_error() == b"tt_conv2d_wgrad: bad argument"

    def gathered(ws_bytes):
        return L.tt_gather_conv_wgrad_plan(0x1000, 64, 64, 0x2000, 0x3000, 1500, 27, 0x4000, 64, 64, 64, 0, 0x5000, 0x6000, ws_bytes, 0,
                                           buf, 192)
    assert gathered(1 << 30) == 0 and buf.value.startswith(b"gather_wgrad_kernel grid 27 x ")
    assert gathered(16) != 0 and L.tt_last_error() == b"tt_gather_conv_wgrad: workspace too small"
