"""Which form a decoder row chain runs in is decided in one host file (csrc/chain_choose.cpp) that tt_mlp_chain_plan answers from
without a device.  tests/chain_choice_cases.json holds what ops.mlp_chain chose at the commit before the chooser existed -- which
launch entry it called with which n_groups / n_split / workspace bytes, or its TTError (tools/chain_choice_sweep.py --table: the
launch entries replaced by recorders, the capacity patched) -- over the decoder's own stage lists at row counts, hints and
capacities that reach both sides of every condition; the chooser must reproduce it row for row.  TT_CHAIN_WIDE is read once per
process, so each setting is replayed by a child process of its own."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "chain_choice_sweep.py")
_spec = importlib.util.spec_from_file_location("chain_choice_sweep", TOOL)
sweep = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sweep)
ROWS = json.load(open(os.path.join(ROOT, "tests", "chain_choice_cases.json")))["cases"]
BY_NAME = {r["name"]: r for r in ROWS}


def _lib():
    from thinktwice_amd import _lib
    return _lib.lib()


def _stages(dims, srcs):
    from thinktwice_amd import ops
    arr = (ops._ChainStage * (len(dims) - 1))()
    for i in range(len(dims) - 1):
        arr[i].w = 0x1000
        arr[i].K, arr[i].Kp, arr[i].N, arr[i].in_sel = dims[i], (dims[i] + 15) // 16 * 16, dims[i + 1], srcs[i]
    return arr


def _plan(R, arr, n_split=1, groups=0, force=0, cap=128, x_stride=None):
    """(rc, tt_chain_choice, error text)"""
    from thinktwice_amd import ops
    L, c = _lib(), ops._ChainChoice()
    rc = L.tt_mlp_chain_plan(R, arr[0].Kp if x_stride is None else x_stride, len(arr), arr, n_split, groups, force, cap, ctypes.byref(c))
    return rc, c, L.tt_last_error().decode()


@pytest.mark.parametrize("env", [1, 0])
def test_the_recorded_choices_are_reproduced(env):
    cases = sweep.runs(env)
    rows = ROWS[:len(sweep.runs(1))] if env else ROWS[len(sweep.runs(1)):]
    assert [c["name"] for c in cases] == [r["name"] for r in rows] and len(rows) > (700 if env else 100)
    r = subprocess.run([sys.executable, TOOL, "--plan", "--env", str(env)], check=True, capture_output=True, text=True, cwd=ROOT)
    got = json.loads(r.stdout)["cases"]
    bad = [(a, b) for a, b in zip(rows, got) if a != b]
    assert len(got) == len(rows) and not bad, bad[:5]


def test_every_arm_is_in_the_record():
    """rows, rows split, wide with 1 / 2 / 4 row blocks per workgroup, wide refused, wide -> rows on a small device, the switch;
    and the grid of every wide row: 1, 2 or 4 row blocks per workgroup."""
    seen = set()
    for c in sweep.cases():
        r = BY_NAME[c["name"]]
        blocks = (c["R"] + 31) // 32
        if "error" in r:
            assert c["wide"] is True and "co-resident" in r["error"]
            seen.add("wide refused")
        elif r["entry"] == "tt_mlp_chain":
            assert r["n_split"] == c["n_split"]
            seen.add("rows split" if r["n_split"] > 1 else "rows")
            if c["wide"] is None and blocks <= 16:
                assert c["env"] == 0 or c["cap"] < 128
                seen.add("switched off" if c["env"] == 0 else "wide -> rows on a small device")
        else:
            rb = 1 if blocks <= 1 else 2 if blocks == 2 else 4
            seen.add("wide, %d row blocks per workgroup" % rb)
            if r["n_groups"] != (c["groups"] or 16):
                seen.add("wide, groups clamped")
            rc, ch, _ = _plan(c["R"], sweep.stage_array(c["list"]), c["n_split"], c["groups"] or 0, 2, c["cap"], sweep.x_cols(c["list"]))
            assert rc == 0 and ch.wide == 1 and ch.row_groups == (blocks + rb - 1) // rb and ch.row_groups * ch.n_groups <= min(128, c["cap"])
            assert ch.dynamic_lds == 0 and ch.workspace_bytes == r["ws"]
    assert seen == {"rows", "rows split", "wide, 1 row blocks per workgroup", "wide, 2 row blocks per workgroup",
                    "wide, 4 row blocks per workgroup", "wide, groups clamped", "wide refused", "wide -> rows on a small device",
                    "switched off"}, seen


def test_dynamic_lds_and_the_lds_refusal():
    # ffn 256 -> 1024 -> 256: one kept buffer of 32 rows x (1024 x 4 + 16) B
    rc, c, _ = _plan(70, _stages([256, 1024, 256], [-1, 0]), force=1)
    assert rc == 0 and (c.wide, c.row_groups, c.n_split, c.dynamic_lds, c.workspace_bytes) == (0, 3, 1, 32 * (1024 * 4 + 16), 0)
    # nothing kept: the launch's minimum
    rc, c, _ = _plan(1, _stages([256, 256], [-1]), force=1)
    assert rc == 0 and c.dynamic_lds == 16
    # look query chain: the 512-wide buffer at the start of the window, the 256-wide one (its input in the lower half) at the end
    rc, c, _ = _plan(3840, sweep.stage_array("look"), x_stride=1552)
    assert rc == 0 and (c.wide, c.row_groups, c.dynamic_lds) == (0, 120, 160 * 1024)
    # the three-stage chain of test_wide_hidden_chain_and_lds_budget: 131,584 B + a kept 33,280 B do not fit; the wide form keeps
    # them in the workspace (3 row blocks -> one workgroup of 4: 128 rows x (1024 + 256) columns)
    three = _stages([256, 1024, 256, 8], [-1, 0, 1])
    rc, c, err = _plan(70, three, force=1)
    assert rc == -1 and err == "tt_mlp_chain: intermediates of stage 1 do not fit in 160 KiB of LDS"
    rc, c, _ = _plan(70, three, force=2)
    assert rc == 0 and (c.wide, c.row_groups, c.n_groups, c.workspace_bytes) == (1, 1, 16, 128 * (1024 + 256) * 4)
    assert c.workspace_bytes == _lib().tt_mlp_chain_wide_workspace_bytes(70, 3, three)


def test_the_plan_refuses_what_the_launch_refuses():
    merge = _stages([1024, 512, 512, 256], [-1, 0, 1])
    assert _plan(4, merge)[0] == 0
    assert _plan(4, merge, n_split=4, force=1)[::2] == (-1, "tt_mlp_chain: n_split > 1 needs a single stage")
    assert _plan(4, merge, n_split=4)[0] == 0                                  # the wide form has no n_split
    assert _plan(0, merge)[::2] == (-1, "tt_mlp_chain_wide: bad arguments")
    assert _plan(4096, merge, x_stride=1020)[::2] == (-1, "tt_mlp_chain: stage 0: x rows (stride 1020) must cover the padded K = 1024 "
                                                      "(finite padding)")
    assert _plan(4, merge, x_stride=1026)[::2] == (-1, "tt_mlp_chain_wide: x must be 16 B aligned rows")
    for force, who in ((1, "tt_mlp_chain"), (2, "tt_mlp_chain_wide")):
        assert _plan(8, _stages([32, 64, 16], [-1, 0]), force=force)[0] == 0
        bad = _stages([32, 64, 16], [-1, 0])
        bad[1].K = bad[1].Kp = 48
        assert _plan(8, bad, force=force)[::2] == (-1, who + ": stage 1: K=48 but stage 0 has N=64")
        bad = _stages([32, 64, 16], [-1, 1])
        assert _plan(8, bad, force=force)[::2] == (-1, who + ": stage 1 reads stage 1")
        bad = _stages([32, 64, 16], [-1, 0])
        bad[0].w = 0x1004
        assert _plan(8, bad, force=force)[::2] == (-1, who + ": stage 0 weights unaligned")
    # the launch entry's own column groups: exact, refused beyond 64 and beyond the device
    assert _plan(480, merge, groups=32, force=3)[1].n_groups == 32 and _plan(480, merge, groups=36, force=2)[1].n_groups == 32
    rc, _, err = _plan(480, merge, groups=65, force=3)
    assert rc == -1 and "co-resident" in err
    rc, _, err = _plan(480, merge, groups=36, force=3)
    assert rc == -1 and err == ("tt_mlp_chain_wide: 4 row groups x 36 column groups: at most 128 workgroups per launch can be guaranteed "
                                "co-resident on this device")
    assert _plan(480, merge, groups=36, force=3, cap=144)[0] == 0
    L = _lib()
    assert L.tt_mlp_chain_plan(4, 1024, 3, merge, 1, 0, 0, 128, None) == -1 and L.tt_last_error() == b"tt_mlp_chain_plan: bad arguments"
    assert _plan(4, merge, force=4)[0] == -1 and _plan(4, merge, cap=-1)[0] == -1 and _plan(4, merge, force=1, cap=-1)[0] == 0


def test_the_form_depends_on_the_rows_alone():
    """ops.chain_is_wide asks about a one-stage chain; every recorded row of the same rows, capacity and switch has that form."""
    one = _stages([16, 1], [-1])
    for c in sweep.runs(1):
        if c["wide"] is None:
            rc, ch, _ = _plan(c["R"], one, cap=c["cap"])
            assert rc == 0 and ch.wide == (BY_NAME[c["name"]]["entry"] == "tt_mlp_chain_wide"), c["name"]
