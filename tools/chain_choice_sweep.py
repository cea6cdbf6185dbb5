"""Which form a decoder row chain runs in (tt_mlp_chain / tt_mlp_chain_wide), with which grid and workspace, over a fixed list of
calls: the decoder's own stage lists at row counts and hints that reach both sides of every condition of csrc/chain_choose.cpp.

  --record  (no GPU) every case through ops.mlp_chain itself, with the two launch entries on the ctypes handle replaced by recorders
            that do not call through, ops.chain_wide_max_workgroups patched to the case's capacity and tensors that are only
            addresses: which entry was called with which n_groups / n_split / workspace bytes, or the TTError.  Uses nothing but
            what the package has had all along, so it runs on any commit.
  --plan    (no GPU) the same rows from tt_mlp_chain_plan.
  --table   (no GPU) --record of both settings of TT_CHAIN_WIDE (read once per process: the other one is a child process).
            tests/chain_choice_cases.json is --table at the commit before the chooser existed; tests/test_chain_choice.py replays
            it through --plan.
  --cases   (no GPU) the list as input lines of tools/chain_choose_check.cpp, the chooser alone under a host sanitizer.
  --launch  (GPU) every case of the real capacity once through ops.mlp_chain, random weights; records the sha256 of every stage
            output (equal hashes = equal bits).  Under `rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python
            tools/chain_choice_sweep.py --launch` the trace holds the chains' kernels in the order of the list.
  --trace DIR   (no GPU) the chain kernels of such a trace in dispatch order: name, grid in workgroups (x, y), LDS bytes.

Every mode prints one JSON document (--out FILE writes it): {"cases": [...]}.  --env 0 runs a mode with TT_CHAIN_WIDE=0.
"""
import argparse
import csv
import ctypes
import glob
import hashlib
import json
import os
import re
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

REAL_CAP = 128          # tt_mlp_chain_wide_max_workgroups() as read on an MI355X: 1 resident workgroup x 256 CUs / 2 launches
NONE, RELU, GELU = 0, 1, 3


def S(K, N, src, act=NONE, out=False, res=False, side=0):
    return dict(K=K, N=N, src=src, act=act, out=out, res=res, side=side)


_MERGE = [S(1024, 512, -1, RELU), S(512, 512, 0, RELU, out=True), S(512, 256, 1, RELU, side=2), S(256, 64, None, RELU), S(64, 2, None, res=True, out=True),
          S(512, 256, 1, RELU, side=4), S(256, 64, None, RELU), S(64, 4, None, res=True, out=True)]


def _order(idx, srcs):
    return [dict(_MERGE[i], src=s) for i, s in zip(idx, srcs)]


# the decoder's chains (decoder_fused.py), by their dimensions: name -> (stages, n_split, groups as the call site gives them)
LISTS = {
    "look": ([S(1544, 512, -1, GELU), S(512, 256, 0, GELU), S(256, 512, 1, out=True), S(256, 256, 1, out=True)], 1, None),
    "ffn": ([S(256, 1024, -1, GELU), S(1024, 256, 0, res=True, out=True)], 1, None),
    "output_proj": ([S(1024, 512, -1, GELU), S(512, 256, 0, out=True)], 1, None),
    "merge, wide order": (_order((0, 1, 2, 5, 3, 6, 4, 7), (-1, 0, 1, 1, 2, 3, 4, 5)), 1, None),
    "merge, row order": (_order((0, 1, 2, 3, 4, 5, 6, 7), (-1, 0, 1, 2, 3, 1, 5, 6)), 1, None),
    "bev broadcast": ([S(2048, 1152, -1, out=True)], 5, 36),
    "flat": ([S(2304, 512, -1, RELU), S(512, 256, 0, res=True, out=True)], 1, None),
    "flat, split head": ([S(2304, 512, -1, RELU, out=True)], 4, None),
    "flat, split tail": ([S(512, 256, -1, res=True, out=True)], 1, None),
    "coarse ctrl": ([S(384, 512, -1, RELU), S(512, 512, 0, RELU), S(512, 256, 1, RELU, out=True), S(256, 256, 2, RELU), S(256, 256, 3, RELU),
                     S(256, 1, 4, out=True), S(256, 512, 2, RELU), S(512, 512, 6, RELU), S(512, 512, 7, RELU), S(512, 8, 8, out=True),
                     S(512, 512, 7, RELU), S(512, 8, 10, out=True)], 1, None),
}
ROWS = [1, 32, 33, 64, 65, 480, 512, 513, 544, 3840]
GROUPS = [None, 1, 3, 16, 36, 64]
CAPS = [REAL_CAP, 256, 8, 3, 1]       # 256: beyond the room the choice gives a launch anyway
SINGLE = ("bev broadcast", "flat, split head", "flat, split tail")       # n_split > 1 needs a single stage


def cases():
    out, seen = [], set()

    def add(lst, R, groups="own", n_split="own", wide=None, cap=REAL_CAP, env=1):
        groups = LISTS[lst][2] if groups == "own" else groups
        n_split = LISTS[lst][1] if n_split == "own" else n_split
        name = "%s R=%d groups=%s n_split=%d wide=%s cap=%d env=%d" % (lst, R, groups, n_split, wide, cap, env)
        if name not in seen:
            seen.add(name)
            out.append(dict(name=name, list=lst, R=R, groups=groups, n_split=n_split, wide=wide, cap=cap, env=env))
    for env in (1, 0):                                      # every chain at every row count as its call site asks for it
        for lst in LISTS:
            for R in ROWS:
                add(lst, R, env=env)
    for lst in ("look", "merge, wide order", "bev broadcast"):       # the hints
        for R in (1, 33, 65, 480, 513):
            for g in GROUPS:
                for w in (None, False, True):
                    add(lst, R, groups=g, wide=w)
    for lst in SINGLE:
        for R in (1, 513, 3840):
            for ns in (1, 4, 5):
                for w in (None, False, True):
                    add(lst, R, n_split=ns, wide=w)
    for cap in CAPS[1:]:                                    # smaller devices: the clamp, the fallback and the refusal
        for lst in ("look", "merge, wide order"):
            for R in (1, 33, 65, 480, 512, 513):
                for g in (None, 16, 64):
                    for w in (None, True):
                        add(lst, R, groups=g, wide=w, cap=cap)
    for R in (1, 513):                                      # the switch does not reach a forced form
        for w in (False, True):
            add("look", R, wide=w, env=0)
    return out


def runs(env):
    return [c for c in cases() if c["env"] == env]


def wiring(lst):
    """The stages of a list with every src resolved (None: the stage before)."""
    return [dict(s, src=i - 1 if s["src"] is None else s["src"]) for i, s in enumerate(LISTS[lst][0])]


def _error(e):
    return dict(error=re.sub(r"^\w+ failed \(rc=-?\d+\): ", "", str(e)))


# ---------------------------------------------------------------------------------------------------------------- --record
class _Addr:
    """A device tensor as far as ops.mlp_chain looks at one, without a device."""
    is_cuda = True

    def __init__(self, rows, cols, addr):
        import torch
        self.shape, self.dtype, self.device, self._addr = (rows, cols), torch.float32, torch.device("cuda", 0), addr

    def dim(self):
        return 2

    def stride(self, i):
        return (self.shape[1], 1)[i]

    def numel(self):
        return self.shape[0] * self.shape[1]

    def data_ptr(self):
        return self._addr


class _Lin:
    def __init__(self, s):
        self.K, self.N, self.act, self.side_k = s["K"], s["N"], s["act"], s["side"]
        self.Kp = (self.K + 15) // 16 * 16
        self.w, self.bias, self.side_w = _Addr(self.N, self.Kp, 0x100000), None, _Addr(self.N, 8, 0x200000)


def stage_dicts(lst, R, lin, tensor):
    """The stage dicts ops.mlp_chain takes: lin(s) a ChainLinear, tensor(rows, cols) an f32 tensor, of either kind."""
    st = []
    for s in wiring(lst):
        d = {"lin": lin(s), "src": s["src"]}
        if s["out"]:
            d["out"] = (tensor(R, s["N"]), 0)
        if s["res"]:
            d["res"] = (tensor(R, s["N"]), 0)
        if s["side"]:
            d["side"] = tensor(R, s["side"])
        st.append(d)
    return st


def x_cols(lst):
    return max((s["K"] + 15) // 16 * 16 for s in wiring(lst) if s["src"] < 0)


def run_record(env):
    from thinktwice_amd import _lib, ops
    L, calls = _lib.lib(), []
    L.tt_mlp_chain = lambda x, R, xs, n, arr, n_split, st: calls.append(dict(entry="tt_mlp_chain", n_split=n_split)) or 0
    L.tt_mlp_chain_wide = lambda x, R, xs, n, arr, g, ws, nb, st: calls.append(dict(entry="tt_mlp_chain_wide", n_groups=g, ws=nb)) or 0
    ops._st = lambda t: None
    ops._workspace = lambda nbytes, device: _Addr(int(nbytes), 1, 0x7000000)
    out = []
    for c in runs(env):
        ops.chain_wide_max_workgroups = lambda device, cap=c["cap"]: cap
        del calls[:]
        try:
            ops.mlp_chain(_Addr(c["R"], x_cols(c["list"]), 0x3000000), stage_dicts(c["list"], c["R"], _Lin, lambda r, n: _Addr(r, n, 0x4000000)),
                          n_split=c["n_split"], groups=c["groups"], wide=c["wide"])
            assert len(calls) == 1
            out.append(dict(name=c["name"], **calls[0]))
        except _lib.TTError as e:
            out.append(dict(name=c["name"], **_error(e)))
    return out


# ---------------------------------------------------------------------------------------------------------------- --plan
def stage_array(lst):
    from thinktwice_amd import ops
    st = wiring(lst)
    arr = (ops._ChainStage * len(st))()
    for d, s in zip(arr, st):
        d.w, d.K, d.Kp, d.N, d.act, d.in_sel = 0x100000, s["K"], (s["K"] + 15) // 16 * 16, s["N"], s["act"], s["src"]
        if s["side"]:
            d.side, d.side_w, d.side_stride, d.side_k = 0x4000000, 0x200000, s["side"], s["side"]
    return arr


def plan_call(L, c, force=None):
    """(rc, tt_chain_choice) of tt_mlp_chain_plan for a case, with the hints translated as ops.mlp_chain does."""
    from thinktwice_amd import ops
    arr, ch = stage_array(c["list"]), ops._ChainChoice()
    force = (0 if c["wide"] is None else 2 if c["wide"] else 1) if force is None else force
    rc = L.tt_mlp_chain_plan(c["R"], x_cols(c["list"]), len(arr), arr, c["n_split"], 0 if c["groups"] is None else max(1, c["groups"]), force,
                             c["cap"], ctypes.byref(ch))
    return rc, ch


def run_plan(env):
    from thinktwice_amd import _lib
    L, out = _lib.lib(), []
    for c in runs(env):
        rc, ch = plan_call(L, c)
        if rc:
            out.append(dict(name=c["name"], error=L.tt_last_error().decode()))
        elif ch.wide:
            out.append(dict(name=c["name"], entry="tt_mlp_chain_wide", n_groups=ch.n_groups, ws=ch.workspace_bytes))
        else:
            out.append(dict(name=c["name"], entry="tt_mlp_chain", n_split=ch.n_split))
    return out


def run_cases():
    """Lines for tools/chain_choose_check.cpp: R x_stride n_split groups force max_workgroups nstages, then K Kp N in_sel side_k per
    stage; every case with its own force and as the launch entry would take it (force 3)."""
    lines = []
    for c in cases():
        st = wiring(c["list"])
        tail = " ".join("%d %d %d %d %d" % (s["K"], (s["K"] + 15) // 16 * 16, s["N"], s["src"], s["side"]) for s in st)
        for force in ((0 if c["wide"] is None else 2 if c["wide"] else 1), 3):
            lines.append("%d %d %d %d %d %d %d %s" % (c["R"], x_cols(c["list"]), c["n_split"], c["groups"] or 0, force, c["cap"], len(st), tail))
    return lines


# ---------------------------------------------------------------------------------------------------------------- --launch
def run_launch(env):
    import torch
    from thinktwice_amd import ops
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=g, device="cuda")
    lins = {}

    def lin(lst):
        if lst not in lins:
            lins[lst] = [ops.ChainLinear(rnd(s["N"], s["K"] + s["side"]) * s["K"] ** -0.5, rnd(s["N"]) * 0.1, act=s["act"], side_k=s["side"])
                         for s in wiring(lst)]
        it = iter(lins[lst])
        return lambda s: next(it)
    out = []
    for i, c in enumerate(runs(env)):
        if c["cap"] != REAL_CAP:
            continue
        g.manual_seed(1000 + i)
        x = rnd(c["R"], x_cols(c["list"]))
        st = stage_dicts(c["list"], c["R"], lin(c["list"]), rnd)
        outs = [d["out"][0] for d in st if "out" in d]
        for t in outs:
            t.fill_(float("nan"))
        try:
            ops.mlp_chain(x, st, n_split=c["n_split"], groups=c["groups"], wide=c["wide"])
            torch.cuda.synchronize()
            out.append(dict(name=c["name"], sha=[hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in outs]))
        except ops.TTError as e:
            out.append(dict(name=c["name"], **_error(e)))
    assert ops.chain_faults() == 0
    return out


def run_trace(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = []
    for r in csv.DictReader(open(f)):
        m = re.search(r"\bmlp_chain(?:_wide)?_kernel\b", r["Kernel_Name"])
        if m:
            wx, wy = int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"])
            rows.append((int(r["Start_Timestamp"]), dict(kernel=m.group(0), grid=[int(r["Grid_Size_X"]) // wx, int(r["Grid_Size_Y"]) // wy],
                                                         lds=int(r.get("LDS_Block_Size", r.get("Group_Segment_Size", 0))))))
    rows.sort(key=lambda r: r[0])
    return [r for _, r in rows]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    for m in ("--record", "--plan", "--table", "--cases", "--launch"):
        g.add_argument(m, action="store_true")
    g.add_argument("--trace", metavar="DIR")
    ap.add_argument("--env", type=int, choices=(0, 1), default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    os.environ["TT_CHAIN_WIDE"] = "1" if a.table else str(a.env)
    if a.cases:
        print("\n".join(run_cases()))
        return
    if a.table:
        import subprocess
        off = subprocess.run([sys.executable, __file__, "--record", "--env", "0"], check=True, capture_output=True, text=True).stdout
        rows = run_record(1) + json.loads(off)["cases"]
    else:
        rows = run_record(a.env) if a.record else run_plan(a.env) if a.plan else run_launch(a.env) if a.launch else run_trace(a.trace)
    text = "{\"cases\": [\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in rows) + "\n]}\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)
    print(f"{len(rows)} rows", file=sys.stderr)


if __name__ == "__main__":
    main()
