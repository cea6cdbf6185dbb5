"""Numbers behind profiles/train_lidar_union.txt (one MI355X): the multi-sweep clouds of a training batch, B = 8 samples of
T = 2 sweeps of 65,536 points, built three ways on the same inputs on the same box:

  * the one launch of tt_lidar_union_sweeps (sweeps.SweepUnion's kernel; also the whole SweepUnion call);
  * the same result composed from torch's own device operators: per sample a matmul, the cats of union2one
    (carla_dataset.py:314-328), and a zero-padded stack;
  * the numpy restatement on the host (tests/sweep_union_ref.py).

    python -m thinktwice_amd.bench_sweeps [--batch 8] [--points 65536] [--rounds 30] [--out profiles/train_lidar_union.txt]

Device events around windows of back-to-back calls (a call is a few microseconds: one call per window would time the launch),
after 3 warm-up rounds, the variants alternating in one process, the kernel variant twice (A/A).  The kernel is timed on one
buffer set -- 38 MB, which stays in the 256 MB Infinity Cache from call to call -- and rotating over sets that together exceed
it.  Nothing here is measured on the host except the restatement."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

from . import build, ops, sweeps
from .ops import lib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _windows(fns, inner, rounds):
    """{name: [microseconds per call]}: `rounds` windows of inner[name] back-to-back calls each, the variants alternating."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner[k]):
                fn()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / inner[k])
    return us


def main(B, n, rounds, emit):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sweep_union_ref as R
    T, Np = 2, 2 * n
    rng = np.random.default_rng(20)
    host = [[R.random_cloud(rng, n) for _ in range(T)] for _ in range(B)]
    can_bus = np.stack([R.random_can_bus(rng, T) for _ in range(B)])
    mats = np.stack([sweeps.curr2key_matrices(c) for c in can_bus])
    dev = [[torch.from_numpy(s).cuda() for s in per] for per in host]
    mats_dev = torch.from_numpy(mats).cuda()
    union = sweeps.SweepUnion()

    # the entry alone: one input buffer, the table built once
    sets = max(2, -(-300_000_000 // (B * T * n * 16 + B * Np * 20)))
    pts = [torch.from_numpy(np.concatenate([s for per in host for s in per])).cuda() for _ in range(sets)]
    outs = [torch.empty(B, 1, Np, 5, dtype=torch.float32, device="cuda") for _ in range(sets)]
    table = (sweeps.UnionSweep * (B * T))()
    for i in range(B * T):
        table[i].first_row, table[i].count = i * n, n
        table[i].m[:] = mats[i // T, i % T].ravel().tolist()
    stream, L = ops.cur_stream(pts[0].device), lib()
    turn = [0]

    def kernel(rotate):
        i = turn[0] = (turn[0] + 1) % sets if rotate else 0
        rc = L.tt_lidar_union_sweeps(pts[i].data_ptr(), B * T * n, table, B, T, Np, outs[i].data_ptr(), stream)
        assert rc == 0, L.tt_last_error().decode()

    def composed():
        clouds = []
        for b in range(B):
            key, old = dev[b][1], dev[b][0]
            k5 = torch.cat([key, torch.zeros(len(key), 1, device="cuda")], dim=1)
            o5 = torch.cat([(mats_dev[b, 0] @ old.T).T, torch.full((len(old), 1), -1.0, device="cuda")], dim=1)
            clouds.append(torch.cat([k5, o5]))
        out = torch.zeros(B, 1, Np, 5, device="cuda")
        for b, c in enumerate(clouds):
            out[b, 0, :len(c)] = c
        return out

    fns = {"kernel": lambda: kernel(False), "kernel again": lambda: kernel(False), "kernel, rotating": lambda: kernel(True),
           "SweepUnion, device sweeps": lambda: union(dev, curr2key=mats), "SweepUnion, host sweeps": lambda: union(host, curr2key=mats),
           "torch composition": composed}
    inner = {"kernel": 200, "kernel again": 200, "kernel, rotating": 200, "SweepUnion, device sweeps": 20, "SweepUnion, host sweeps": 4,
             "torch composition": 20}
    us = _windows(fns, inner, rounds)
    med = {k: statistics.median(v) for k, v in us.items()}
    moved = B * T * n * 16 + B * Np * 20
    emit(f"B = {B}, T = {T}, {n} points per sweep, Np = {Np}: {B * Np} output rows; device events around windows of back-to-back "
         f"calls, {rounds} rounds after 3 warm-up rounds, the variants alternating in one process")
    what = {"kernel": f"tt_lidar_union_sweeps, one launch, one buffer set ({inner['kernel']} calls per window)",
            "kernel again": "the same again (A/A)",
            "kernel, rotating": f"the same, rotating over {sets} buffer sets ({sets * moved / 1e6:.0f} MB in all)",
            "SweepUnion, device sweeps": "SweepUnion(...) on 16 device tensors (one device concatenation + table + launch)",
            "SweepUnion, host sweeps": "SweepUnion(...) on 16 numpy arrays (pinned staging copy + upload + launch)",
            "torch composition": "torch: per-sample matmul, cat, zero-padded stack"}
    for k in fns:
        emit(f"  {what[k]:90s} median {med[k]:9.2f} us (min {min(us[k]):.2f}, max {max(us[k]):.2f})")
    emit(f"  A/A spread: {med['kernel again'] - med['kernel']:+.2f} us")
    emit(f"  bytes moved by the kernel: {B * T * n * 16} read (16 per point) + {B * Np * 20} written (20 per row) = {moved} "
         f"({moved / 1e6:.1f} MB)")
    emit(f"  achieved: {moved / med['kernel'] / 1e3:.0f} GB/s on one buffer set (resident in the Infinity Cache between calls: not an "
         f"HBM rate), {moved / med['kernel, rotating'] / 1e3:.0f} GB/s rotating")
    emit(f"  torch composition / one launch: {med['torch composition'] / med['kernel']:.1f} x (against the whole SweepUnion call on "
         f"device sweeps: {med['torch composition'] / med['SweepUnion, device sweeps']:.1f} x)")
    emit(f"  host-to-device bytes per batch: 5 floats per point from the loader {B * Np * 20} -> 4 floats per point "
         f"{B * T * n * 16}: {B * Np * 20 - B * T * n * 16} bytes ({(B * Np * 20 - B * T * n * 16) / 1e6:.1f} MB) fewer")

    t0 = time.perf_counter()
    want = R.collate([R.union_points(per, m) for per, m in zip(host, mats)], Np)
    t1 = time.perf_counter()
    kernel(False)
    torch.cuda.synchronize()
    got = outs[0].cpu().numpy()[:, 0]
    bound = R.collate([R.points_bound(per, m) for per, m in zip(host, mats)], Np).astype(np.float64)
    ratio, exact = R.worst_ratio(got, want, bound)
    comp = composed().cpu().numpy()[:, 0]
    ratio_c, exact_c = R.worst_ratio(comp, want, bound)
    emit(f"  tests/sweep_union_ref.py on the same batch on this box, one process, host clock, one pass: {(t1 - t0) * 1e3:.0f} ms "
         f"({(t1 - t0) * 1e6 / med['kernel']:.0f} x the launch)")
    emit(f"  device against the restatement: worst |error| / bound {ratio:.3f}, rows that must be bit-equal "
         f"{'are' if exact else 'ARE NOT'}; torch composition against it: {ratio_c:.3f}, {'are' if exact_c else 'ARE NOT'}")
    return med


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured on the host")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"build {build.source_fingerprint()} device {torch.cuda.get_device_name(0)}")
    main(a.batch, a.points, a.rounds, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
