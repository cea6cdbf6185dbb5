"""Which kernels a voxel pool / a fused lift-splat runs on, over a fixed list of calls that reaches every arm of tt_voxel_pool_fwd /
_fwd_ws / _fwd_planned and tt_lift_splat_fwd / _fwd_ws and both sides of every condition in csrc/voxel_pool_choose.cpp.

  --launch  (GPU) every launchable case once, through the C entries themselves; records the sha256 of every output (out, pos_memo,
            and for the extra rows grad_in / geom).  Uses nothing but entries the library has had all along, so it runs on any commit.
            Under `rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python tools/voxel_pool_choice_sweep.py --launch` the
            trace holds the case's pool / lift-splat kernels in the order of the list.
  --trace DIR   (no GPU) joins such a trace to the list: per case every dispatched kernel's name with its template arguments, grid
            in workgroups, workgroup size and LDS bytes as rocprofv3 saw them (its LDS_Block_Size: the kernel's STATIC LDS -- a
            launch's dynamic LDS is not in the trace).
  --bytes   (no GPU) what the five size queries answer per case.
  --plan    (no GPU) the same rows from tt_voxel_pool_fwd_plan / tt_lift_splat_fwd_plan.
  --cases   (no GPU) the list as input lines of tools/voxel_pool_choose_check.cpp, the chooser alone under a host sanitizer.
  --table DIR_SORT_ON DIR_SORT_OFF   (no GPU) the committed table: --trace of both processes, --bytes, and the derived rows.

TT_VP_SORT is read once per process: `--sort 0` runs the cases that have a workspace with the counting sort turned off (a second
process, a second trace).  Every mode prints one JSON document (--out FILE writes it): {"cases": [{"name", "sort", ...}]}.
tests/voxel_pool_choice_cases.json is --table at the commit before the chooser existed (the rows that cannot be launched are
"derived": their answer read off that commit's code); tests/test_voxel_pool_choice.py replays it through the plan entries.
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

# static LDS per kernel as a trace reports it: the compiler's "LDS Size" of the instantiation (32784, 128, 3072, 12288, 16) in the
# 512-byte granules of the allocation; the others have none
STATIC_LDS = {"voxel_pool_p1_kernel<1, 16, true>": 33280, "voxel_pool_p1_kernel<4, 4, true>": 33280, "vp_cs_scan_kernel": 512,
              "vp_planned_cells_kernel<1>": 3072, "vp_planned_cells_kernel<4>": 12288, "lift_splat_strip_kernel<float>": 512,
              "lift_splat_strip_kernel<unsigned short>": 512, "lift_splat_strip_kernel<tt::f16_t>": 512}
DTYPES = {"f32": 0, "bf16": 1, "f16": 2}       # TT_F32 / TT_BF16 / TT_F16


def P(name, B=2, Np=1000, C=4, grid=(21, 21, 1), ws="full", mis=None, ws_entry=1, **kw):
    """A pool call.  ws: "full" (tt_voxel_pool_workspace_bytes), "sort" / "two_phase" (exactly that arm's bytes), "sort-1" /
    "two_phase-1", "small" (1024 bytes), None (null), or a byte count.  mis: "feats" / "out" / "ws": that pointer + 4 bytes."""
    return dict(kind="pool", name=name, B=B, Np=Np, C=C, grid=list(grid), ws=ws if ws_entry else None, mis=mis, ws_entry=ws_entry, **kw)


def L(name, B=1, ncam=1, D=8, fH=4, fW=4, C=4, grid=(21, 21, 1), dt="f32", ws=True, cstride=None, **kw):
    """A lift-splat call (ws: with the workspace of tt_lift_splat_workspace_bytes, or null)."""
    return dict(kind="lift", name=name, B=B, ncam=ncam, D=D, fH=fH, fW=fW, C=C, grid=list(grid), dt=dt, ws=ws,
                cstride=cstride or C, **kw)


# the parametrisations of the GPU tests in tests/test_voxel_pool.py (tests/test_voxel_pool_choice.py checks that none is missing)
TEST_DIRECT = [(1, 1, 4), (2, 63, 256), (3, 1000, 256), (2, 777, 7), (1, 300, 1024), (2, 20000, 256)]
TEST_RANDOM = [(1, 1, 4), (2, 63, 256), (2, 64, 256), (3, 1000, 256), (1, 4097, 512), (2, 777, 7), (1, 300, 1024), (2, 128, 36),
               (2, 20000, 256), (1, 9000, 64), (3, 8193, 1024)]
TEST_PLANNED = [(1, 1, 4), (2, 63, 256), (3, 1000, 256), (1, 4097, 512), (2, 20000, 256), (1, 9000, 64), (3, 8193, 1024)]
TEST_SORT = [(2, 20000, 256, (21, 21, 1)), (1, 70001, 256, (21, 21, 1)), (3, 16385, 64, (21, 21, 1)), (2, 40000, 512, (32, 32, 1)),
             (4, 9000, 128, (21, 21, 2)), (8, 8192, 256, (21, 21, 1))]

CASES = (
    [P("direct %d %d %d" % t, *t, ws_entry=0) for t in TEST_DIRECT] + [P("random %d %d %d" % t, *t) for t in TEST_RANDOM] +
    [dict(kind="planned", name="planned %d %d %d" % t, B=t[0], Np=t[1], C=t[2], grid=[21, 21, 1]) for t in TEST_PLANNED] +
    [P("sort %d %d %d" % t[:3], *t) for t in TEST_SORT] + [P("sort %d %d %d small ws" % t[:3], *t, ws="small") for t in TEST_SORT] + [
        # ---- channels: NV = 1 .. 4 of the rows kernel (no workspace) and the C % 4 / C <= 1024 edges
        *[P("C=%d" % C, C=C, ws=None) for C in (4, 7, 256, 260, 512, 516, 768, 772, 1024, 1028)],
        # ---- the same edges where a workspace arm would otherwise take the call
        *[P("C=%d, 32768 points" % C, B=2, Np=16384, C=C) for C in (7, 256, 260, 1024, 1028)],
        # ---- total points: 4 * kChunk (two-phase) and 4 * kCsChunk (counting sort)
        P("total 8191", B=1, Np=8191), P("total 8192", B=1, Np=8192), P("total 32767", B=1, Np=32767), P("total 32768", B=1, Np=32768),
        # ---- cells: kCsMaxCells (32 x 32 against 25 x 41), kMaxCells (32 x 64 against 2049 x 1)
        P("cells 1024", B=1, Np=32768, grid=(32, 32, 1)), P("cells 1025", B=1, Np=32768, grid=(25, 41, 1)),
        P("cells 2048", B=1, Np=32768, grid=(32, 64, 1)), P("cells 2049", B=1, Np=32768, grid=(2049, 1, 1)),
        # ---- points per sample: 64 / 65 chunks of kCsChunk
        P("Np 524288", B=1, Np=524288), P("Np 524289", B=1, Np=524289),
        # ---- workspace bytes and pointers
        P("ws = sort bytes", B=2, Np=16384, ws="sort"), P("ws = sort bytes - 1", B=2, Np=16384, ws="sort-1"),
        P("ws = two-phase bytes", B=2, Np=16384, ws="two_phase"), P("ws = two-phase bytes - 1", B=2, Np=16384, ws="two_phase-1"),
        P("ws null", B=2, Np=16384, ws=None),
        P("feats + 4 B", B=2, Np=16384, mis="feats"), P("out + 4 B", B=2, Np=16384, mis="out"), P("ws + 4 B", B=2, Np=16384, mis="ws"),
        P("ws + 4 B, two-phase sizes", B=1, Np=8192, mis="ws"), P("feats + 4 B, no ws", B=1, Np=1000, ws=None, mis="feats"),
        P("ws_entry = 0", B=2, Np=16384, ws_entry=0),
        # ---- nothing to launch
        P("B = 0", B=0, Np=1000), P("Np = 0", B=2, Np=0),
        # ---- the rows kernel's grid: one block, and the clamp at 4096 blocks (16 per CU)
        P("total 64", B=1, Np=64, ws=None), P("4095 blocks", B=1, Np=8386560, ws=None), P("4096 blocks", B=1, Np=8386561, ws=None),
        # ---- point indices past an int: never the counting sort.  Too large to launch: read off the code.
        P("total 2^31 - 524288", B=4095, Np=524288, ws=1 << 50, plan_only=True), P("total 2^31", B=4096, Np=524288, ws=1 << 50, plan_only=True),
        # ---- the planned streaming kernels: <1, 32, true> + cells<1> against <4, 4, true> + cells<4>
        dict(kind="planned", name="planned C=256", B=2, Np=1000, C=256, grid=[21, 21, 1]),
        dict(kind="planned", name="planned C=260", B=2, Np=1000, C=260, grid=[21, 21, 1]),
        # ---- not dispatched anywhere, in the list for their bits: the backward (both kernels) and the frustum index
        dict(kind="bwd", name="bwd C=4", B=2, Np=1000, C=4, grid=[21, 21, 1]), dict(kind="bwd", name="bwd C=7", B=2, Np=1000, C=7, grid=[21, 21, 1]),
        dict(kind="frustum", name="frustum index", B=2, ncam=2, D=8, fH=4, fW=5),
        # ---- lift-splat, with and without the workspace: strip height, depth bins, cells, odd width, storage type, kStageC
        *[L("lift %s%s" % (n, "" if ws else ", no ws"), ws=ws, **kw) for n, kw in [
            ("fH=32", dict(fH=32)), ("fH=33", dict(fH=33)), ("D=128", dict(D=128)), ("cells 2048", dict(grid=(32, 64, 1))),
            ("cells 2049", dict(grid=(2049, 1, 1))), ("fW=5", dict(fW=5)), ("f32", {}), ("bf16", dict(dt="bf16")), ("f16", dict(dt="f16")),
            ("C=128", dict(C=128)), ("C=132", dict(C=132)), ("2 x 3 cams", dict(B=2, ncam=3)),
            ("test shape, random cells", dict(B=2, ncam=4, D=80, fH=7, fW=9, C=64, geom="random")),
            ("test shape 32 x 32", dict(B=2, ncam=4, D=80, fH=16, fW=24, C=80, grid=(32, 32, 1))),
        ] for ws in (True, False)],
        L("lift D=129", D=129, plan_only=True), L("lift D=129, no ws", D=129, ws=False, plan_only=True),
        L("lift out_cstride=6", cstride=6, plan_only=True), L("lift out_cstride=6, no ws", cstride=6, ws=False),
    ])


def runs(sort):
    """The cases of one process: all of them with the counting sort on, those a workspace arm could take with it off."""
    return [c for c in CASES if sort or (c["kind"] == "pool" and c["ws_entry"] and c["ws"] is not None)]


def two_phase_bytes(c):
    cps = (c["Np"] + 2047) // 2048
    return cps * c["B"] * 64 * c["C"] * 4 + c["B"] * c["grid"][0] * c["grid"][1] * cps * 4 + 256


def ws_request(Lib, c):
    """Bytes of the workspace a pool case passes.  "sort" is the query's answer with the counting sort on, "two_phase" that arm's
    own size (the query's answer with it off)."""
    ws = c["ws"]
    if ws is None or isinstance(ws, int):
        return ws
    if ws == "small":
        return 1024
    full = int(Lib.tt_voxel_pool_workspace_bytes(c["B"], c["Np"], c["C"], c["grid"][0], c["grid"][1]))
    base = two_phase_bytes(c) if ws.startswith("two_phase") else full
    return base - 1 if ws.endswith("-1") else base


# ---------------------------------------------------------------------------------------------------------------- --launch
def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _geom(torch, B, Np, grid, g):
    X, Y, Z = grid
    return torch.stack([torch.randint(-2, X + 2, (B, Np), generator=g, device="cuda"), torch.randint(-2, Y + 2, (B, Np), generator=g, device="cuda"),
                        torch.randint(-1, Z + 1, (B, Np), generator=g, device="cuda")], -1).to(torch.int32).contiguous()


def _ray_geom(torch, c):
    """Ray-like geometry, as a frustum gives it: azimuth from (camera, column), range from the depth bin, so that a strip of two
    columns falls into fewer than kMaxSlots cells and the workspace form adds nothing with atomics (random cells overflow the
    slots, and the overflow is added in whatever order the atomics land).  The last image row looks over the grid's edge."""
    import math
    B, n, D, fH, fW, (X, Y, Z) = c["B"], c["ncam"], c["D"], c["fH"], c["fW"], c["grid"]
    ar = lambda k, shape: torch.arange(k, device="cuda").view(shape).float()
    b, cam, d, h, w = ar(B, (B, 1, 1, 1, 1)), ar(n, (1, n, 1, 1, 1)), ar(D, (1, 1, D, 1, 1)), ar(fH, (1, 1, 1, fH, 1)), ar(fW, (1, 1, 1, 1, fW))
    az = cam * (math.pi / 2) + (w / fW - 0.5) * 1.4 + 0.05 * b
    rng = 0.5 + d * 0.25
    full = (B, n, D, fH, fW)
    gx = torch.floor(X / 2 + rng * torch.cos(az)).expand(full)
    gy = torch.floor(Y / 2 + rng * torch.sin(az)).expand(full)
    gz = torch.where(h.expand(full) == fH - 1, float(Z), 0.0)
    return torch.stack([gx, gy, gz], -1).reshape(B, n * D * fH * fW, 3).to(torch.int32).contiguous()


def _buf(torch, n, dtype, mis, fill=None, g=None):
    """n elements of a 4-byte dtype, 16-byte aligned or (mis) 4 bytes past that."""
    raw = torch.empty(n + 4, dtype=dtype, device="cuda")
    v = raw[1:n + 1] if mis else raw[:n]
    if fill is None:
        v.copy_(torch.randn(n, generator=g, device="cuda"))
    else:
        v.fill_(fill)
    assert v.data_ptr() % 16 == (4 if mis else 0)
    return raw, v


def run_launch(sort):
    import torch
    from thinktwice_amd import _lib, ops
    from thinktwice_amd.voxel_pooling import VoxelPoolPlan
    Lib, ci, cll = _lib.lib(), ctypes.c_int, ctypes.c_longlong
    out_rows = []
    for i, c in enumerate(runs(sort)):
        if c.get("plan_only"):
            continue
        g = torch.Generator(device="cuda").manual_seed(1000 + i)
        rec = {}
        st = _lib.cur_stream(torch.device("cuda", 0))
        if c["kind"] in ("pool", "planned", "bwd"):
            B, Np, C, (X, Y, Z) = c["B"], c["Np"], c["C"], c["grid"]
            geom = _geom(torch, B, Np, c["grid"], g)
        if c["kind"] == "pool":
            mis = c["mis"]
            _, feats = _buf(torch, B * Np * C, torch.float32, mis == "feats", g=g)
            _, out = _buf(torch, B * Y * X * C, torch.float32, mis == "out", fill=0.0)
            pm = torch.full((B, Np, 3), -1, dtype=torch.int32, device="cuda")
            nb = ws_request(Lib, c)
            ws = None if nb is None else torch.empty(nb // 4 + 8, dtype=torch.int32, device="cuda")
            wp = None if ws is None else ctypes.c_void_p(ws.data_ptr() + (4 if mis == "ws" else 0))
            if c["ws_entry"]:
                rc = Lib.tt_voxel_pool_fwd_ws(ci(B), ci(Np), ci(C), ci(X), ci(Y), ci(Z), _lib.ptr(geom), ctypes.c_void_p(feats.data_ptr()),
                                              ctypes.c_void_p(out.data_ptr()), _lib.ptr(pm), wp, cll(nb or 0), st)
            else:
                rc = Lib.tt_voxel_pool_fwd(ci(B), ci(Np), ci(C), ci(X), ci(Y), ci(Z), _lib.ptr(geom), ctypes.c_void_p(feats.data_ptr()),
                                           ctypes.c_void_p(out.data_ptr()), _lib.ptr(pm), st)
            _lib.check(rc, c["name"])
            rec = dict(out=_sha(out), pos_memo=_sha(pm))
        elif c["kind"] == "planned":
            feats = torch.randn(B, Np, C, generator=g, device="cuda")
            rec = dict(out=_sha(VoxelPoolPlan(geom, c["grid"])(feats)))
        elif c["kind"] == "bwd":
            gz, gy, gx = geom[..., 2], geom[..., 1], geom[..., 0]
            inr = (gx >= 0) & (gx < X) & (gy >= 0) & (gy < Y) & (gz >= 0) & (gz < Z)
            b = torch.arange(B, device="cuda", dtype=torch.int32).view(B, 1).expand(B, Np)
            pm = torch.where(inr.unsqueeze(-1), torch.stack([b, gy, gx], -1), torch.full_like(geom, -1)).contiguous()
            go = torch.randn(B, Y, X, C, generator=g, device="cuda")
            gi = torch.empty(B, Np, C, device="cuda")
            _lib.check(Lib.tt_voxel_pool_bwd(ci(B), ci(Np), ci(C), ci(X), ci(Y), _lib.ptr(pm), _lib.ptr(go), _lib.ptr(gi), st), c["name"])
            rec = dict(grad_in=_sha(gi))
        elif c["kind"] == "frustum":
            fr = torch.randn(c["D"], c["fH"], c["fW"], 4, generator=g, device="cuda")
            mats = torch.randn(c["B"] * c["ncam"], 2, 4, 4, generator=g, device="cuda")
            geom, gf = ops.frustum_voxel_index(fr, mats, [-10.0, -10.0, -1.0], [1.0, 1.0, 2.0], c["B"], c["ncam"], want_f32=True)
            rec = dict(geom=_sha(geom), geom_f32=_sha(gf))
        else:
            B, n, D, fH, fW, C, (X, Y, Z) = c["B"], c["ncam"], c["D"], c["fH"], c["fW"], c["C"], c["grid"]
            tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[c["dt"]]
            depth = (torch.randn(B * n, fH, fW, D, generator=g, device="cuda") * 2).to(tdt)
            ctx = torch.randn(B * n, fH, fW, C, generator=g, device="cuda").to(tdt)
            geom = _geom(torch, B, n * D * fH * fW, c["grid"], g) if c.get("geom") == "random" else _ray_geom(torch, c)
            out = torch.zeros(B, Y, X, c["cstride"], device="cuda")
            nb = int(Lib.tt_lift_splat_workspace_bytes(ci(B), ci(n), ci(D), ci(fH), ci(fW), ci(C), ci(X), ci(Y))) if c["ws"] else 0
            ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda") if c["ws"] else None
            _lib.check(Lib.tt_lift_splat_fwd_ws(ci(B), ci(n), ci(D), ci(fH), ci(fW), ci(C), ci(X), ci(Y), ci(Z), _lib.ptr(depth), _lib.ptr(ctx),
                                                ci(DTYPES[c["dt"]]), _lib.ptr(geom), _lib.ptr(out), ci(c["cstride"]), ci(0), ci(0), _lib.ptr(ws),
                                                cll(nb), st), c["name"])
            rec = dict(out=_sha(out))
        torch.cuda.synchronize()
        out_rows.append(dict(name=c["name"], sort=sort, sha=rec))
    return out_rows


# ---------------------------------------------------------------------------------------------------------------- --trace
KERNEL = re.compile(r"\b((?:voxel_pool_(?:rows|scalar|p1|p2)|vp_cs_(?:count|scan|scatter)|vp_planned_(?:segments|cells)|"
                    r"lift_splat(?:_strip|_cells)?)_kernel(?:<[^>]*>)?)")
FOLLOWERS = ("voxel_pool_p2_kernel", "vp_cs_scan_kernel", "vp_cs_scatter_kernel", "vp_planned_cells_kernel", "lift_splat_cells_kernel")


def launches_nothing(c):
    return c["kind"] in ("bwd", "frustum") or (c["kind"] == "pool" and c["B"] * c["Np"] == 0)


def run_trace(d, sort):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = []
    for r in csv.DictReader(open(f)):
        m = KERNEL.search(r["Kernel_Name"])
        if m:
            lds = r.get("LDS_Block_Size", r.get("Group_Segment_Size"))
            rows.append((int(r["Start_Timestamp"]), [m.group(1), int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_X"]),
                                                     int(lds)]))
    rows.sort(key=lambda r: r[0])
    # a call's kernels: a leader (rows, scalar, p1, count, strip, pixel, or the segments kernel of a static plan) and its followers
    groups = []
    for _, k in rows:
        name = k[0].split("<")[0]
        after_scatter = name == "vp_planned_segments_kernel" and groups and groups[-1][-1][0] == "vp_cs_scatter_kernel"
        if name in FOLLOWERS or after_scatter:
            groups[-1].append(k)
        else:
            groups.append([k])
    out, i = [], 0
    for c in runs(sort):
        if c.get("plan_only"):
            continue
        mine = []
        if not launches_nothing(c):
            mine = groups[i]
            i += 1
        out.append(dict(name=c["name"], sort=sort, launches=mine))
    assert i == len(groups), (i, len(groups))
    return out


# ---------------------------------------------------------------------------------------------------------------- --bytes
def run_bytes(sort):
    from thinktwice_amd import _lib
    Lib = _lib.lib()
    out = []
    for c in runs(sort):
        if c["kind"] in ("pool", "planned"):
            B, Np, C, X, Y = c["B"], c["Np"], c["C"], c["grid"][0], c["grid"][1]
            b = dict(workspace=int(Lib.tt_voxel_pool_workspace_bytes(B, Np, C, X, Y)), plan=int(Lib.tt_voxel_pool_plan_bytes(B, Np, X, Y)),
                     plan_workspace=int(Lib.tt_voxel_pool_plan_workspace_bytes(B, Np)),
                     planned_workspace=int(Lib.tt_voxel_pool_planned_workspace_bytes(B, Np, C, X, Y)))
        elif c["kind"] == "lift":
            b = dict(lift_splat_workspace=int(Lib.tt_lift_splat_workspace_bytes(c["B"], c["ncam"], c["D"], c["fH"], c["fW"], c["C"], c["grid"][0],
                                                                               c["grid"][1])))
        else:
            continue
        out.append(dict(name=c["name"], sort=sort, bytes=b))
    return out


# ---------------------------------------------------------------------------------------------------------------- --plan
def plan_call(Lib, c):
    """(rc, label) of the plan entry for a pool / lift case; pointers are dummy 256-byte aligned addresses (+ 4 where the case says)."""
    buf = ctypes.create_string_buffer(512)
    A = 0x100000
    X, Y, Z = c["grid"]
    if c["kind"] == "pool":
        nb = ws_request(Lib, c)
        m = lambda k: 4 if c["mis"] == k else 0
        rc = Lib.tt_voxel_pool_fwd_plan(c["B"], c["Np"], c["C"], X, Y, Z, A, 2 * A + m("feats"), 3 * A + m("out"), 4 * A,
                                        None if nb is None else 5 * A + m("ws"), nb or 0, c["ws_entry"], buf, len(buf))
    else:
        nb = int(Lib.tt_lift_splat_workspace_bytes(c["B"], c["ncam"], c["D"], c["fH"], c["fW"], c["C"], c["grid"][0], c["grid"][1])) if c["ws"] else 0
        rc = Lib.tt_lift_splat_fwd_plan(c["B"], c["ncam"], c["D"], c["fH"], c["fW"], c["C"], X, Y, Z, A, 2 * A, DTYPES[c["dt"]], 3 * A, 4 * A,
                                        c["cstride"], 0, 0, 5 * A if c["ws"] else None, nb, buf, len(buf))
    return rc, buf.value.decode()


def parse_label(label):
    """([[kernel, grid, block, static LDS]], [dynamic LDS], ws bytes) of a plan label."""
    head, _, ws = label.rpartition("ws ")
    launches, dyn = [], []
    for part in [p for p in head.strip().split(" + ") if p]:
        m = re.match(r"^(.*) grid (\d+) block (\d+) lds (\d+)$", part)
        assert m, label
        launches.append([m.group(1), int(m.group(2)), int(m.group(3)), STATIC_LDS.get(m.group(1), 0)])
        dyn.append(int(m.group(4)))
    return launches, dyn, int(ws)


def dynamic_lds(c, kernel):
    """Dynamic LDS a launch needs, restated: vp_cs_count_kernel 16 waves x cells rounded up to 64 x (u16 count + u64 lane mask);
    lift_splat_strip_kernel lift_splat_strip_lds(D, C, cells) of csrc/voxel_pool_choose.h."""
    cells = c["grid"][0] * c["grid"][1]
    if kernel == "vp_cs_count_kernel":
        return 16 * ((cells + 63) // 64 * 64) * 10
    if kernel.startswith("lift_splat_strip_kernel"):
        D, C = c["D"], c["C"]
        pd = (D + 3) // 4 * 4
        if pd & 4 == 0:
            pd += 4
        a = 64 * pd * 4 + 64 * D * 2
        b = 68 * 64 * 4 + (cells + 64 + 3) // 4 * 4 * 4 + max(a, 64 * min(C, 128) * 4)
        return (b + 15) // 16 * 16
    return 0


def run_plan(sort):
    from thinktwice_amd import _lib
    Lib = _lib.lib()
    out = []
    for c in runs(sort):
        if c["kind"] not in ("pool", "lift"):
            continue
        rc, label = plan_call(Lib, c)
        if rc:
            out.append(dict(name=c["name"], sort=sort, rc=rc, error=Lib.tt_last_error().decode()))
        else:
            launches, dyn, ws = parse_label(label)
            out.append(dict(name=c["name"], sort=sort, launches=launches, dynamic_lds=dyn, ws=ws))
    return out


def run_cases():
    """The list as lines for tools/voxel_pool_choose_check.cpp (the stand-alone chooser program of the sanitizer build): every pool
    call with and without the LDS opt-in granted, every lift-splat call."""
    from thinktwice_amd import _lib
    Lib, A, lines = _lib.lib(), 0x100000, []
    for c in CASES:
        if c["kind"] == "pool":
            nb = ws_request(Lib, c)
            m = lambda k: 4 if c["mis"] == k else 0
            for granted in (1, 0):
                lines.append("pool %d %d %d %d %d %d %d %d %d %d %d" % (c["B"], c["Np"], c["C"], c["grid"][0], c["grid"][1], 2 * A + m("feats"),
                                                                       3 * A + m("out"), 0 if nb is None else 5 * A + m("ws"), nb or 0, c["ws_entry"], granted))
        elif c["kind"] == "lift":
            lines.append("lift %d %d %d %d %d %d %d %d %d %s" % (c["B"], c["ncam"], c["D"], c["fH"], c["fW"], c["C"], c["grid"][0], c["grid"][1],
                                                                 c["ws"], {"f32": "float", "bf16": "unsigned short", "f16": "tt::f16_t"}[c["dt"]]))
    return lines


# ---------------------------------------------------------------------------------------------------------------- --table
# The rows that cannot be launched, read off the code of tt_voxel_pool_fwd_ws / tt_lift_splat_fwd_ws at the commit before the
# chooser: 4095 samples of 524,288 points are 64 chunks each and 2^31 - 524,288 points (the counting sort, or with it off the
# two-phase kernels: 256 chunks of 2048 per sample); 4096 such samples are 2^31 points, past an int: two-phase.  Segment
# capacity per sample 524288 / 64 + 441 + 1 = 8634.  The lift-splat refusals are its TT_REQUIREs, in their order.
DERIVED = {
    ("total 2^31 - 524288", 1): dict(launches=[["vp_cs_count_kernel", 64 * 4095, 1024, 0], ["vp_cs_scan_kernel", 4095, 1024, 512],
                                               ["vp_cs_scatter_kernel", 4095 * 524288 // 256, 256, 0],
                                               ["vp_planned_segments_kernel<1, 32, true>", (8634 * 4095 + 3) // 4, 256, 0],
                                               ["vp_planned_cells_kernel<1>", 441 * 4095, 256, 3072]]),
    ("total 2^31 - 524288", 0): dict(launches=[["voxel_pool_p1_kernel<1, 16, true>", 256 * 4095, 512, 33280],
                                               ["voxel_pool_p2_kernel", 441 * 4095, 64, 0]]),
    ("total 2^31", 1): dict(launches=[["voxel_pool_p1_kernel<1, 16, true>", 256 * 4096, 512, 33280], ["voxel_pool_p2_kernel", 441 * 4096, 64, 0]]),
    ("lift D=129", 1): dict(rc=-1, error="tt_lift_splat_fwd: D=129 unsupported (1..128)"),
    ("lift D=129, no ws", 1): dict(rc=-1, error="tt_lift_splat_fwd: D=129 unsupported (1..128)"),
    ("lift out_cstride=6", 1): dict(rc=-1, error="tt_lift_splat_fwd: workspace form needs 16 B aligned rows"),
}
DERIVED[("total 2^31", 0)] = DERIVED[("total 2^31", 1)]


def run_table(dirs, sizes_sort_off):
    """The committed table: per process (counting sort on, off) the trace rows, the size queries and the derived rows."""
    rows = []
    for sort, d in ((1, dirs[0]), (0, dirs[1])):
        trace = {r["name"]: r for r in run_trace(d, sort)}
        sizes = {r["name"]: r for r in (run_bytes(1) if sort else sizes_sort_off)}
        for c in runs(sort):
            r = dict(name=c["name"], sort=sort)
            if c.get("plan_only"):
                r.update(DERIVED[(c["name"], sort)], derived=True)
            else:
                r["launches"] = trace[c["name"]]["launches"]
            if c["name"] in sizes:
                r["bytes"] = sizes[c["name"]]["bytes"]
            rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--launch", action="store_true")
    g.add_argument("--trace", metavar="DIR")
    g.add_argument("--bytes", action="store_true")
    g.add_argument("--plan", action="store_true")
    g.add_argument("--cases", action="store_true")
    g.add_argument("--table", nargs=2, metavar=("DIR_SORT_ON", "DIR_SORT_OFF"))
    ap.add_argument("--sort", type=int, choices=(0, 1), default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    os.environ["TT_VP_SORT"] = "1" if a.table else str(a.sort)
    if a.cases:
        print("\n".join(run_cases()))
        return
    if a.table:       # the size queries with the sort off come from a process of their own (the flag is read once)
        import subprocess
        off = subprocess.run([sys.executable, __file__, "--bytes", "--sort", "0"], check=True, capture_output=True, text=True).stdout
        cases = run_table(a.table, json.loads(off)["cases"])
    else:
        cases = run_launch(a.sort) if a.launch else run_trace(a.trace, a.sort) if a.trace else run_bytes(a.sort) if a.bytes else run_plan(a.sort)
    text = "{\"cases\": [\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]}\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)
    print(f"{len(cases)} rows", file=sys.stderr)


if __name__ == "__main__":
    main()
