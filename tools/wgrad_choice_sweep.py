"""Which kernel a weight gradient runs on, over a fixed list of layers that reaches every kernel family of tt_conv2d_wgrad /
tt_conv2d_wgrad_x3 / tt_gather_conv_wgrad and both sides of every condition in csrc/wgrad_choose.cpp.

  --launch  (GPU) real buffers through ops.conv2d_wgrad (once fresh, once with accumulate=True onto a seeded dw) and
            ops.gather_conv_wgrad (ragged live count); records the sha256 of every result.  Uses nothing but those two calls, so it
            runs on any commit.  Under `rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python tools/wgrad_choice_sweep.py
            --launch` the trace holds one weight-gradient kernel per call, in the order of the list.
  --trace DIR   (no GPU) joins such a trace to the list: per case and mode the kernel's name with its template arguments, grid x / y
            in workgroups and LDS bytes as rocprofv3 saw them (its LDS_Block_Size: the kernel's STATIC LDS -- a launch's dynamic
            LDS is not in the trace).
  --plan    (no GPU) the same rows from tt_conv2d_wgrad_plan / tt_gather_conv_wgrad_plan (`lds`: the static LDS of the kernel named),
            plus the label's dynamic LDS, slices and geometry.

Every mode prints one JSON document (--out FILE writes it): {"cases": [{"name", "mode", ...}]}.  tests/wgrad_choice_cases.json is the
--trace output of the commit before the chooser existed; tests/test_wgrad_choice.py replays it through the plan entries.
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

# static LDS of the two 64 x 64 workgroup-tile kernels (the three waves' tiles of the in-workgroup sum); the others have none
STATIC_LDS = {"conv_wgrad_kernel": 3 * 64 * 64 * 4, "gather_wgrad_kernel": 3 * 64 * 64 * 4}


def D(name, N, H, W, Cin, Cout, k=1, stride=1, pad=0, dil=1, x_coff=0, cs=None):
    """A dense layer: ops.conv2d_wgrad's arguments.  cs: channels of the x buffer (> Cin: a channel window at x_coff)."""
    return dict(kind="dense", name=name, N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, dil=dil, x_coff=x_coff,
                cs=cs or (Cin + 3) // 4 * 4)


def G(name, M, live, Cin, Cout):
    """A gathered layer: 27 taps over M allocated rows of which `live` are in use (ops.gather_conv_wgrad)."""
    return dict(kind="gather", name=name, M=M, live=live, Cin=Cin, Cout=Cout, taps=27)


# tests/test_conv_bwd.py::CASES, in its order (tests/test_wgrad_choice.py checks that none is missing)
BWD_CASES = [
    (2, 20, 24, 64, 64, 3, 1, 1, 1), (3, 17, 23, 32, 96, 3, 1, 1, 1), (2, 28, 28, 128, 64, 1, 1, 0, 1), (2, 30, 32, 64, 128, 3, 2, 1, 1),
    (2, 30, 32, 64, 128, 1, 2, 0, 1), (2, 24, 24, 64, 64, 3, 1, 6, 6), (4, 40, 48, 3, 64, 7, 2, 3, 1), (1, 21, 21, 256, 256, 3, 1, 1, 1),
    (8, 64, 96, 64, 64, 3, 1, 1, 1), (2, 16, 21, 160, 200, 3, 1, 1, 1), (2, 14, 14, 512, 96, 1, 1, 0, 1), (3, 18, 16, 48, 320, 3, 2, 1, 1),
    (2, 24, 31, 32, 12, 3, 1, 1, 1), (2, 12, 16, 24, 256, 1, 1, 0, 1), (2, 12, 16, 200, 20, 3, 1, 1, 1), (2, 30, 40, 128, 512, 3, 2, 1, 1),
    (2, 20, 70, 384, 128, 1, 1, 0, 1), (2, 24, 24, 256, 128, 3, 1, 6, 6), (3, 9, 33, 256, 512, 3, 1, 1, 1),
    (3840, 1, 1, 1544, 512, 1, 1, 0, 1), (40, 8, 8, 128, 128, 3, 1, 1, 1),
    (1, 20, 8, 64, 64, 1, 1, 0, 1), (1, 7, 9, 64, 64, 1, 1, 0, 1), (2, 16, 16, 64, 64, 1, 1, 0, 1),
]
GATHER_PAIRS = [(16, 16), (32, 64), (64, 64), (128, 128), (48, 160), (130, 24)]      # tests/test_conv_bwd.py, the gathered test

CASES = [D("bwd %d" % i, N, H, W, Cin, Cout, k, s, p, d) for i, (N, H, W, Cin, Cout, k, s, p, d) in enumerate(BWD_CASES)] + [
    # ---- the LDS-staged kernel's ">= 64 channels on both sides", and the f32 tile rule's 32 / 33 and 127 / 128
    D("Cout=63", 2, 20, 24, 64, 63, 3, pad=1), D("Cout=60", 2, 20, 24, 64, 60, 3, pad=1),
    D("Cin=63", 2, 20, 24, 63, 64, 3, pad=1), D("Cin=60", 2, 20, 24, 60, 64, 3, pad=1),
    D("Cout=127", 2, 20, 24, 64, 127, 3, pad=1), D("Cout=124", 2, 20, 24, 64, 124, 3, pad=1), D("Cout=128", 2, 20, 24, 64, 128, 3, pad=1),
    D("Cin=127", 2, 20, 24, 127, 64, 3, pad=1), D("Cin=124", 2, 20, 24, 124, 64, 3, pad=1), D("Cin=128", 2, 20, 24, 128, 64, 3, pad=1),
    D("Cout=255", 2, 20, 24, 64, 255, 3, pad=1), D("Cout=252", 2, 20, 24, 64, 252, 3, pad=1), D("Cout=256", 2, 20, 24, 64, 256, 3, pad=1),
    D("Cin=255", 2, 20, 24, 255, 64, 3, pad=1), D("Cin=252", 2, 20, 24, 252, 64, 3, pad=1), D("Cin=256", 2, 20, 24, 256, 64, 3, pad=1),
    D("Cout=32", 2, 20, 24, 64, 32, 3, pad=1), D("Cout=33", 2, 20, 24, 64, 33, 3, pad=1),
    D("Cin=32", 2, 20, 24, 32, 64, 3, pad=1), D("Cin=33", 2, 20, 24, 33, 64, 3, pad=1),
    # ---- rows of at least 16 pixels; 16-byte aligned channel windows
    D("OW=15", 2, 20, 15, 64, 64, 3, pad=1), D("OW=16", 2, 20, 16, 64, 64, 3, pad=1),
    D("x_coff=2", 2, 20, 24, 64, 64, 3, pad=1, x_coff=2, cs=72), D("x_coff=4", 2, 20, 24, 64, 64, 3, pad=1, x_coff=4, cs=72),
    D("x_cstride=70", 2, 20, 24, 64, 64, 3, pad=1, cs=70),
    # ---- 1 x 1 regrouping (exact, late and no divisor are "bwd 21-23"): too few rows to regroup on both sides of 16 pixels, rows that
    # are long enough already, all rows merged into one pseudo-row, a stride that forbids it
    D("1x1 OW=16, 3 rows: not regrouped", 1, 3, 16, 64, 64), D("1x1 OW=15, 3 rows: not regrouped", 1, 3, 15, 64, 64),
    D("1x1 OW=128: not regrouped", 1, 6, 128, 64, 64), D("1x1 OW=127, 7 rows: one pseudo-row", 1, 7, 127, 64, 64),
    D("1x1 4 rows: one pseudo-row", 1, 4, 32, 64, 64), D("1x1 stride 2: not regrouped", 2, 16, 16, 64, 64, 1, stride=2),
    # ---- the split: rows / 4 below the wanted count, fewer than four rows, the most splits a layer can get (one tile: 1024)
    D("rows/4 = 2", 1, 8, 40, 64, 64, 3, pad=1), D("3 rows", 1, 3, 40, 64, 64, 3, pad=1), D("1024 splits", 8, 640, 8, 4, 12),
] + [G("gather %d->%d" % p, 1500, 1237, *p) for p in GATHER_PAIRS] + [
    # ---- gathered: fewer than 64 rows, both sides of the second split's 65th row, a 33-channel side, many rows over one tile per tap
    G("gather M=40", 40, 33, 64, 64), G("gather M=64", 64, 60, 32, 32), G("gather M=65", 65, 65, 32, 32),
    G("gather Cin=33", 1500, 1237, 33, 128), G("gather Cin=4", 70000, 65000, 4, 12),
]

MODES = ("f32", "x3")


def runs():
    """(case, mode) in launch order: every dense case under both arithmetics, every gathered case once (it has one entry)."""
    return [(c, m) for c in CASES for m in (MODES if c["kind"] == "dense" else MODES[:1])]


def out_hw(c):
    k, s, p, d = c["k"], c["stride"], c["pad"], c["dil"]
    return (c["H"] + 2 * p - d * (k - 1) - 1) // s + 1, (c["W"] + 2 * p - d * (k - 1) - 1) // s + 1


# ---------------------------------------------------------------------------------------------------------------- --launch
def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run_launch():
    import torch
    from thinktwice_amd import ops
    out = []
    for i, (c, mode) in enumerate(runs()):
        g = torch.Generator().manual_seed(1000 + i)
        if c["kind"] == "dense":
            OH, OW = out_hw(c)
            x = torch.randn(c["N"], c["H"], c["W"], c["cs"], generator=g).cuda()
            dy = torch.randn(c["N"], OH, OW, c["Cout"], generator=g).cuda()
            cp = (c["Cin"] + 3) // 4 * 4
            seed = torch.randn(c["Cout"], c["k"], c["k"], cp, generator=g).cuda()
            args = (x, dy, c["k"], c["k"], c["stride"], c["pad"], c["dil"])
            kw = dict(cin=c["Cin"], in_coff=c["x_coff"], cin_pad=cp, x3=mode == "x3")
            dw = ops.conv2d_wgrad(*args, **kw)
            acc = ops.conv2d_wgrad(*args, out=seed, accumulate=True, **kw)
            rec = dict(sha=_sha(dw), sha_accumulate=_sha(acc))
        else:
            R_in = max(c["M"] // 2, 8)
            x = torch.randn(R_in, c["Cin"], generator=g)
            dy = torch.randn(c["M"], c["Cout"], generator=g)
            nbr = torch.randint(0, R_in, (c["M"], c["taps"]), generator=g, dtype=torch.int32)
            nbr[torch.rand(c["M"], c["taps"], generator=g) < 0.6] = -1
            nbr[:, 5] = -1
            m_dev = torch.tensor([c["live"]], dtype=torch.int32, device="cuda")
            dw = ops.gather_conv_wgrad(x.cuda(), nbr.cuda(), m_dev, dy.cuda(), c["taps"], cin_pad=(c["Cin"] + 3) // 4 * 4)
            rec = dict(sha=_sha(dw))
        out.append(dict(name=c["name"], mode=mode, **rec))
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------- --trace
KERNEL = re.compile(r"\b((?:conv|gather)_wgrad(?:_wide|_lds)?_kernel(?:<[^>]*>)?)")


def run_trace(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = []
    for r in csv.DictReader(open(f)):
        m = KERNEL.search(r["Kernel_Name"])
        if m:
            lds = r.get("LDS_Block_Size", r.get("Group_Segment_Size"))
            rows.append((int(r["Start_Timestamp"]), m.group(1), int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]),
                         int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"]), int(lds)))
    rows.sort()
    out, i = [], 0
    for c, mode in runs():
        n = 2 if c["kind"] == "dense" else 1
        mine = rows[i:i + n]
        i += n
        assert len(mine) == n and all(r[1:] == mine[0][1:] for r in mine), (c["name"], mode, mine)
        out.append(dict(name=c["name"], mode=mode, kernel=mine[0][1], grid=[mine[0][2], mine[0][3]], lds=mine[0][4]))
    assert i == len(rows), (i, len(rows))
    return out


# ---------------------------------------------------------------------------------------------------------------- --plan
LABEL = re.compile(r"^(\S+(?:<[^>]*>)?) grid (\d+) x (\d+) lds (\d+) reduce (\d+)(?: as (.*))?$")


def plan_call(L, c, x3, misalign=0):
    """(rc, label) of the plan entry for a case; pointers are dummy 64-byte aligned addresses (+ misalign on x)."""
    buf = ctypes.create_string_buffer(192)
    P = 0x100000
    if c["kind"] == "dense":
        OH, OW = out_hw(c)
        cp = (c["Cin"] + 3) // 4 * 4
        rc = L.tt_conv2d_wgrad_plan(P + misalign, c["N"], c["H"], c["W"], c["Cin"], c["cs"], c["x_coff"], 2 * P, OH, OW, c["Cout"], c["Cout"],
                                    0, c["k"], c["k"], c["stride"], c["pad"], c["dil"], cp, 0, 3 * P, 4 * P, workspace_bytes(L, c),
                                    int(x3), buf, len(buf))
    else:
        cp = (c["Cin"] + 3) // 4 * 4
        rc = L.tt_gather_conv_wgrad_plan(P, c["Cin"], c["Cin"], 2 * P, 3 * P, c["M"], c["taps"], 4 * P, c["Cout"], c["Cout"], cp, 0, 5 * P,
                                         6 * P, workspace_bytes(L, c), int(x3), buf, len(buf))
    return rc, buf.value.decode()


def workspace_bytes(L, c):
    cp = (c["Cin"] + 3) // 4 * 4
    if c["kind"] == "dense":
        return int(L.tt_conv2d_wgrad_workspace_bytes(c["N"], out_hw(c)[0], c["Cout"], c["Cin"], cp, c["k"], c["k"]))
    return int(L.tt_gather_conv_wgrad_workspace_bytes(c["M"], c["Cout"], c["Cin"], cp, c["taps"]))


def parse_label(label):
    m = LABEL.match(label)
    assert m, label
    kernel = m.group(1)
    return dict(kernel=kernel, grid=[int(m.group(2)), int(m.group(3))], lds=STATIC_LDS.get(kernel, 0), dynamic_lds=int(m.group(4)),
                slices=int(m.group(5)), geometry=m.group(6))


def stage_bytes(kernel):
    """Dynamic LDS a kernel instantiation needs: the LDS-staged kernel's two stages of 32 pixels x (64 bi + 64 bj) f32 channels."""
    m = re.match(r"conv_wgrad_lds_kernel<(\d), (\d)>", kernel)
    return 2 * 32 * 64 * (int(m.group(1)) + int(m.group(2))) * 4 if m else 0


def run_plan():
    from thinktwice_amd import _lib
    L = _lib.lib()
    out = []
    for c, mode in runs():
        rc, label = plan_call(L, c, mode == "x3")
        assert rc == 0, (c["name"], L.tt_last_error())
        out.append(dict(name=c["name"], mode=mode, **parse_label(label)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--launch", action="store_true")
    g.add_argument("--trace", metavar="DIR")
    g.add_argument("--plan", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    cases = run_launch() if a.launch else run_trace(a.trace) if a.trace else run_plan()
    text = "{\"cases\": [\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]}\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)
    print(f"{len(cases)} rows, {len({c['kernel'] for c in cases if 'kernel' in c})} distinct kernels", file=sys.stderr)


if __name__ == "__main__":
    main()
