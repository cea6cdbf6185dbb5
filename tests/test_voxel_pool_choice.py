"""Which kernels a voxel pool / a fused lift-splat runs on is decided in one host file (csrc/voxel_pool_choose.cpp) that
tt_voxel_pool_fwd_plan and tt_lift_splat_fwd_plan answer from without a device.  tests/voxel_pool_choice_cases.json holds what the
launchers chose -- every dispatched kernel's name with template arguments, grid, workgroup size and LDS bytes, read from rocprofv3
kernel traces on an MI355X (tools/voxel_pool_choice_sweep.py --launch with the counting sort on and off, then --table) -- and what the
size queries answered at the commit before the chooser existed, over a case list that reaches every arm and both sides of every
condition; the chooser must reproduce it row for row.  TT_VP_SORT is read once per process, so each setting is replayed by a
child process of its own."""
import ctypes
import functools
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "voxel_pool_choice_sweep.py")
_spec = importlib.util.spec_from_file_location("voxel_pool_choice_sweep", TOOL)
sweep = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sweep)
ROWS = json.load(open(os.path.join(ROOT, "tests", "voxel_pool_choice_cases.json")))["cases"]


def _lib():
    from thinktwice_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def _tool(mode, sort):
    r = subprocess.run([sys.executable, TOOL, mode, "--sort", str(sort)], check=True, capture_output=True, text=True, cwd=ROOT)
    return {c["name"]: c for c in json.loads(r.stdout)["cases"]}


@pytest.mark.parametrize("sort", [1, 0])
def test_the_recorded_choices_and_sizes_are_reproduced(sort):
    rows = [r for r in ROWS if r["sort"] == sort]
    cases = sweep.runs(sort)
    assert [c["name"] for c in cases] == [r["name"] for r in rows] and len(rows) > (100 if sort else 40)
    plan, sizes = _tool("--plan", sort), _tool("--bytes", sort)
    bad = []
    for c, r in zip(cases, rows):
        if "bytes" in r and sizes[c["name"]]["bytes"] != r["bytes"]:
            bad.append((r, sizes[c["name"]]))
        if c["kind"] not in ("pool", "lift"):
            continue
        got = plan[c["name"]]
        if "rc" in r:
            if (got.get("rc"), got.get("error")) != (r["rc"], r["error"]):
                bad.append((r, got))
        elif got.get("launches") != r["launches"]:
            bad.append((r, got))
        # a launch's dynamic LDS is not in a kernel trace: it must be what the kernel's layout takes for the case
        elif got["dynamic_lds"] != [sweep.dynamic_lds(c, k[0]) for k in r["launches"]]:
            bad.append((r, got))
    assert not bad, bad


def test_every_arm_and_instantiation_is_in_the_record():
    seen = {tuple(k[0] for k in r["launches"]) for r in ROWS if "launches" in r}
    count = ("vp_cs_count_kernel", "vp_cs_scan_kernel", "vp_cs_scatter_kernel")
    want = {(), ("voxel_pool_scalar_kernel",), *[("voxel_pool_rows_kernel<%d>" % nv,) for nv in (1, 2, 3, 4)],
            ("voxel_pool_p1_kernel<1, 16, true>", "voxel_pool_p2_kernel"), ("voxel_pool_p1_kernel<4, 4, true>", "voxel_pool_p2_kernel"),
            count + ("vp_planned_segments_kernel<1, 32, true>", "vp_planned_cells_kernel<1>"),
            count + ("vp_planned_segments_kernel<4, 4, true>", "vp_planned_cells_kernel<4>"),
            ("vp_planned_segments_kernel<1, 32, true>", "vp_planned_cells_kernel<1>"),
            ("vp_planned_segments_kernel<4, 4, true>", "vp_planned_cells_kernel<4>")}
    for t in ("float", "unsigned short", "tt::f16_t"):
        want |= {("lift_splat_kernel<%s>" % t,), ("lift_splat_strip_kernel<%s>" % t,), ("lift_splat_strip_kernel<%s>" % t, "lift_splat_cells_kernel")}
    # the per-pixel kernel is only reached by shapes outside the strip kernel's limits: recorded for f32
    want -= {("lift_splat_kernel<unsigned short>",), ("lift_splat_kernel<tt::f16_t>",)}
    assert seen == want, seen ^ want


def test_the_static_plan_runs_the_streaming_kernels_of_the_counting_sort():
    """tt_voxel_pool_fwd_planned has no plan entry: its two launches come from the function that also ends a counting-sort call
    (vp_planned_launches).  Recorded rows: one group of B x cells keys, floor(total / 64) + keys + 1 segments, 4 per workgroup."""
    by_c = {}
    for r in ROWS:
        if r["name"].startswith("C=") and r["name"].endswith("32768 points") and r["sort"] and len(r["launches"]) == 5:
            by_c[r["launches"][3][0]] = [k[0] for k in r["launches"][3:]]
    n = 0
    for c in sweep.CASES:
        if c["kind"] == "planned":
            r = next(r for r in ROWS if r["name"] == c["name"])
            keys, total = c["B"] * 441, c["B"] * c["Np"]
            seg, cel = r["launches"]
            assert (seg[1], seg[2], cel[1], cel[2]) == ((total // 64 + keys + 1 + 3) // 4, 256, keys, 256), r
            assert seg[0] == "vp_planned_segments_kernel<%s, true>" % ("1, 32" if c["C"] <= 256 else "4, 4"), r
            if seg[0] in by_c:
                assert [seg[0], cel[0]] == by_c[seg[0]]
            assert r["bytes"]["planned_workspace"] == (total // 64 + keys + 1) * c["C"] * 4
            n += 1
    assert n >= 9 and len(by_c) == 2


def test_the_case_list_holds_the_cases_of_the_gpu_tests():
    import test_voxel_pool as T

    def params(f):
        return list(next(m for m in f.pytestmark if m.name == "parametrize").args[1])
    assert params(T.test_b1_symbol_tt_voxel_pool_fwd_directly) == sweep.TEST_DIRECT
    assert params(T.test_hip_voxel_pool_matches_oracle_random) == sweep.TEST_RANDOM
    assert params(T.test_planned_voxel_pool_matches_oracle_random) == sweep.TEST_PLANNED
    assert [p[:4] for p in params(T.test_counting_sort_path_matches_oracle_and_the_static_plan)] == sweep.TEST_SORT
    names = {c["name"] for c in sweep.CASES}
    for t in sweep.TEST_DIRECT:
        assert "direct %d %d %d" % t in names
    for t in sweep.TEST_RANDOM:
        assert "random %d %d %d" % t in names
    for t in sweep.TEST_PLANNED:
        assert "planned %d %d %d" % t in names
    for t in sweep.TEST_SORT:
        assert "sort %d %d %d" % t[:3] in names and "sort %d %d %d small ws" % t[:3] in names
    # the two lift-splat tests: their shapes, with and without the workspace
    lift = {(c["B"], c["ncam"], c["D"], c["fH"], c["fW"], c["C"], tuple(c["grid"]), c["ws"]) for c in sweep.CASES if c["kind"] == "lift"}
    for ws in (True, False):
        assert (2, 4, 80, 7, 9, 64, (21, 21, 1), ws) in lift and (2, 4, 80, 16, 24, 80, (32, 32, 1), ws) in lift


def test_the_workspace_query_is_the_largest_arm():
    """tt_voxel_pool_workspace_bytes is the most any arm takes: with the counting sort off the two-phase arm's own size (restated in
    the sweep tool), which is what the full workspace then selects; with it on the bytes of the arm selected -- the label's `ws` --
    unless the two-phase arm, though not selected, would take more (70,001 points of 256 channels)."""
    for sort in (1, 0):
        plan, sizes = _tool("--plan", sort), _tool("--bytes", sort)
        for c in sweep.runs(sort):
            if c["kind"] == "pool" and c["ws"] == "full" and c["mis"] is None and c["ws_entry"]:
                ws, query = plan[c["name"]]["ws"], sizes[c["name"]]["bytes"]["workspace"]
                if sort:
                    assert query == ws or (ws and query == sweep.two_phase_bytes(c) > ws), c["name"]
                else:
                    assert query == ws and ws in (0, sweep.two_phase_bytes(c)), c["name"]


def test_the_plan_refuses_what_the_launch_refuses():
    L = _lib()
    buf = ctypes.create_string_buffer(512)
    A = 0x100000

    def pool(B, Np, C, geom=A, grid=(21, 21, 1), ws=None, nb=0, ws_entry=1, label=buf, label_bytes=512):
        return L.tt_voxel_pool_fwd_plan(B, Np, C, grid[0], grid[1], grid[2], geom, 2 * A, 3 * A, 4 * A, ws, nb, ws_entry, label, label_bytes)
    assert pool(2, 1000, 4) == 0 and buf.value == b"voxel_pool_rows_kernel<1> grid 1 block 256 lds 0 ws 0"
    assert pool(0, 1000, 4) == 0 and buf.value == b"ws 0"
    assert pool(2, 1000, 4, label=None, label_bytes=0) != 0 and b"tt_voxel_pool_fwd_plan" in L.tt_last_error()
    assert pool(-1, 1000, 4) != 0 and L.tt_last_error() == b"tt_voxel_pool_fwd: bad sizes B=-1 Np=1000 C=4"
    assert pool(2, 1000, 0) != 0 and L.tt_last_error() == b"tt_voxel_pool_fwd: bad sizes B=2 Np=1000 C=0"
    assert pool(2, 1000, 4, grid=(21, 21, 0)) != 0 and L.tt_last_error() == b"tt_voxel_pool_fwd: bad voxel grid"
    assert pool(2, 1000, 4, geom=None) != 0 and L.tt_last_error() == b"tt_voxel_pool_fwd: null pointer"
    assert pool(0, 1000, 4, geom=None) == 0                      # no points: returns before it looks at the pointers
    assert pool(1, 8192, 4, geom=None, ws=5 * A, nb=1 << 30) != 0 and L.tt_last_error() == b"tt_voxel_pool_fwd_ws: null pointer"

    def lift(D=8, C=4, dtype=0, cstride=4, ws=None, nb=0, depth=A):
        return L.tt_lift_splat_fwd_plan(1, 1, D, 4, 4, C, 21, 21, 1, depth, 2 * A, dtype, 3 * A, 4 * A, cstride, 0, 0, ws, nb, buf, 512)
    assert lift() == 0 and buf.value.startswith(b"lift_splat_strip_kernel<float> grid 2 block 256 lds ") and buf.value.endswith(b" ws 0")
    assert lift(depth=None) != 0 and L.tt_last_error() == b"tt_lift_splat_fwd: null pointer"
    assert lift(C=6) != 0 and L.tt_last_error() == b"tt_lift_splat_fwd: C=6 unsupported"
    assert lift(dtype=7) != 0 and L.tt_last_error() == b"tt_lift_splat_fwd: bad dtype 7"
    need = int(L.tt_lift_splat_workspace_bytes(1, 1, 8, 4, 4, 4, 21, 21))
    assert lift(ws=5 * A, nb=need) == 0 and buf.value.endswith(b" + lift_splat_cells_kernel grid 111 block 256 lds 0 ws %d" % need)
    assert lift(ws=5 * A, nb=need - 1) != 0 and L.tt_last_error() == b"tt_lift_splat_fwd_ws: workspace %d B < %d B" % (need - 1, need)
