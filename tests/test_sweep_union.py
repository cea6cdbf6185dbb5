"""The multi-sweep clouds of a training batch on the device (thinktwice_amd.sweeps.SweepUnion, csrc/lidar_union.hip:
tt_lidar_union_sweeps) against the numpy restatement of union2one (tests/sweep_union_ref.py), which golden F20 pins to the
reference's own function (tests/test_sweep_union_ref.py).

Lattice cases (dyadic coordinates under dyadic matrices: every product and sum exact in f32) are equal to the restatement in
EVERY bit.  Random cases are held to the bound between two f32 evaluations of a 4-term dot product, 2 gamma_4 sum |m_k p_k| per
element from the inputs (sweep_union_ref.points_bound); where that bound is zero -- the key sweep's rows, the time column, the
padding rows -- they too are compared as uint32.

The shapes are the smallest at which the kernel can go wrong.  A workgroup owns 1024 output rows in four rounds of 256, a wave
64 of them, so the per-sample counts put empty segments, a one-row segment and segment and sample boundaries in the middle of a
wave ([0, 5] | [257, 63] | [64, 1]), at a wave's edge (64), across three sweeps ([3, 0, 130]) and across workgroups
([700, 500] | [1, 1100]: 2400 rows, three workgroups); Np is the largest total and a larger, odd one.  The raw-ABI runner lays
the segments out of order with NaN rows between and around them, and hands over an output that sits between sentinel guard
rows and is prefilled with NaN: a read outside a segment, a row left unwritten or a write outside `out` all show."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sweep_union_ref as R  # noqa: E402
from thinktwice_amd import ops, sweeps as S  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD_ROWS = 8
SENTINEL = -12345.0
CASES = {                                                    # name: (counts[b][t], the two Np)
    "wave_edges": ([[0, 5], [257, 63], [64, 1]], (320, 333)),
    "three_sweeps": ([[3, 0, 130]], (133, 200)),
    "three_workgroups": ([[700, 500], [1, 1100]], (1200, 1201)),
}
CASE_IDS = [(name, which) for name in CASES for which in (0, 1)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _expected(sweeps, mats, Np):
    return R.collate([R.union_points(per, m) for per, m in zip(sweeps, mats)], Np)


def _table(first, counts, mats):
    n = len(first)
    table = (S.UnionSweep * n)()
    for i in range(n):
        table[i].first_row, table[i].count = int(first[i]), int(counts[i])
        table[i].m[:] = np.asarray(mats[i], np.float32).ravel().tolist()
    return table


def _scattered(sweeps, seed):
    """One (rows, 4) buffer holding every sweep's rows as a segment, the segments in a shuffled order with 1..3 NaN rows before,
    between and after them; first_row per (b, t) in table order."""
    rng = np.random.default_rng(seed)
    flat = [s for per in sweeps for s in per]
    first, chunks, row = [0] * len(flat), [], 0
    for i in rng.permutation(len(flat)):
        gap = int(rng.integers(1, 4))
        chunks.append(np.full((gap, 4), np.nan, np.float32))
        first[i], row = row + gap, row + gap + len(flat[i])
        chunks.append(flat[i])
    chunks.append(np.full((2, 4), np.nan, np.float32))
    return np.concatenate(chunks), first


def _guarded(rows):
    """(whole, out): `out` = `rows` x 5 floats of NaN inside a buffer with GUARD_ROWS sentinel rows on either side."""
    whole = torch.full(((rows + 2 * GUARD_ROWS) * 5,), SENTINEL, dtype=torch.float32, device="cuda")
    out = whole[GUARD_ROWS * 5:(GUARD_ROWS + rows) * 5]
    out.fill_(float("nan"))
    return whole, out


def _guards_intact(whole):
    w = whole.cpu().numpy()
    return bool((w[:GUARD_ROWS * 5] == SENTINEL).all() and (w[-GUARD_ROWS * 5:] == SENTINEL).all())


def _run_raw(sweeps, mats, Np, seed=0):
    """The entry through ctypes on the scattered layout -> ([B, Np, 5] numpy, whether the guard rows survived)."""
    B, T = len(sweeps), len(sweeps[0])
    buf, first = _scattered(sweeps, seed)
    pts = torch.from_numpy(buf).cuda()
    whole, out = _guarded(B * Np)
    table = _table(first, [len(s) for per in sweeps for s in per], mats.reshape(B * T, 4, 4))
    rc = ops.lib().tt_lidar_union_sweeps(pts.data_ptr(), len(buf), table, B, T, Np, out.data_ptr(), ops.cur_stream(out.device))
    assert rc == 0, ops.lib().tt_last_error().decode()
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(B, Np, 5), _guards_intact(whole)


def _case(name, which, lattice):
    counts, nps = CASES[name]
    sweeps, mats = R.make_case(sum(map(ord, name)), counts, lattice)
    return sweeps, mats, nps[which]


def _check_fixed_rows(got, sweeps, Np):
    """What no matrix can change, as uint32: the key sweep's rows with time +0.0, every time column, every padding row."""
    T = len(sweeps[0])
    for b, per in enumerate(sweeps):
        n_key, total = len(per[-1]), sum(len(s) for s in per)
        assert np.array_equal(_bits(got[b, :n_key, :4]), _bits(per[-1]))
        times = np.concatenate([np.full(len(per[t]), t - (T - 1), np.float32) for t in range(T - 1, -1, -1)])
        assert np.array_equal(_bits(got[b, :total, 4]), _bits(times))
        assert not _bits(got[b, total:]).any()                       # five +0.0: not NaN (written), not -0.0


# ------------------------------------------------------------------------------------------------------------- raw entry
@pytest.mark.parametrize("name,which", CASE_IDS)
def test_lattice_cases_equal_the_restatement_in_every_bit(name, which):
    sweeps, mats, Np = _case(name, which, lattice=True)
    got, guards = _run_raw(sweeps, mats, Np)
    assert guards
    assert np.array_equal(_bits(got), _bits(_expected(sweeps, mats, Np)))
    _check_fixed_rows(got, sweeps, Np)


@pytest.mark.parametrize("name,which", CASE_IDS)
def test_random_cases_are_within_the_dot_product_bound(name, which):
    sweeps, mats, Np = _case(name, which, lattice=False)
    got, guards = _run_raw(sweeps, mats, Np, seed=1)
    assert guards and not np.isnan(got).any()
    _check_fixed_rows(got, sweeps, Np)
    want = _expected(sweeps, mats, Np)
    bound = R.collate([R.points_bound(per, m) for per, m in zip(sweeps, mats)], Np).astype(np.float64)
    ratio, exact = R.worst_ratio(got, want, bound)
    print(f"{name} Np {Np}: device against the restatement, worst |error| / bound = {ratio:.3f}")
    assert exact and ratio <= 1.0
    assert np.array_equal(_bits(got)[bound == 0], _bits(want)[bound == 0])


def test_the_documented_arithmetic_is_what_runs():
    """One rounded product, then three fused multiply-adds in column order (thinktwice_hip.h), restated in exact rational
    arithmetic with one rounding to f32 per step."""
    from fractions import Fraction

    def f32(x):                                                 # a Fraction -> the nearest f32, ties to even
        if x == 0:
            return np.float32(0)
        e = -149                                                # the ulp is 2^e: 2^23 <= |x| / 2^e < 2^24, or subnormal
        while abs(x) >= Fraction(2) ** (e + 24):
            e += 1
        q = x / Fraction(2) ** e
        n = q.numerator // q.denominator                        # floor
        rest = q - n
        n += 1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1) else 0
        return np.float32(float(n) * 2.0 ** e)

    sweeps, mats, Np = _case("wave_edges", 0, lattice=False)
    got, _ = _run_raw(sweeps, mats, Np)
    p, m = sweeps[1][0][:16], mats[1, 0]                        # sample 1: its older sweep follows the 63 key rows
    moved = got[1, len(sweeps[1][1]):len(sweeps[1][1]) + 16, :4]
    for r in range(16):
        for j in range(4):
            acc = f32(Fraction(float(m[j, 0])) * Fraction(float(p[r, 0])))
            for k in (1, 2, 3):
                acc = f32(Fraction(float(m[j, k])) * Fraction(float(p[r, k])) + Fraction(float(acc)))
            assert _bits(moved[r, j]) == _bits(acc), (r, j)


def test_two_calls_are_bit_identical():
    sweeps, mats, Np = _case("three_workgroups", 1, lattice=False)
    a, _ = _run_raw(sweeps, mats, Np, seed=2)
    b, _ = _run_raw(sweeps, mats, Np, seed=2)
    c, _ = _run_raw(sweeps, mats, Np, seed=3)                   # another layout of the same segments
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))


def test_every_rejected_argument_returns_its_error_and_writes_nothing():
    sweeps, mats, _ = _case("three_sweeps", 0, lattice=True)
    counts = [len(s) for s in sweeps[0]]                        # [3, 0, 130]
    buf, first = _scattered(sweeps, 0)
    pts = torch.from_numpy(buf).cuda()
    whole, out = _guarded(200)
    before = whole.cpu().numpy().view(np.uint32).copy()
    L, stream = ops.lib(), ops.cur_stream(out.device)
    m3 = mats.reshape(3, 4, 4)
    good = dict(points=pts.data_ptr(), num_rows=len(buf), table=_table(first, counts, m3), B=1, T=3, Np=133, out=out.data_ptr())

    def rc(**kw):
        a = dict(good, **kw)
        return L.tt_lidar_union_sweeps(a["points"], a["num_rows"], a["table"], a["B"], a["T"], a["Np"], a["out"], stream)

    big = (S.UnionSweep * 34)()                                 # B * T = 34 empty sweeps
    bad = {
        "null points with rows to read": rc(points=None),
        "null out": rc(out=None),
        "null table": rc(table=None),
        "points not 16-byte aligned": rc(points=pts.data_ptr() + 4),
        "negative first_row": rc(table=_table([first[0], -1, first[2]], counts, m3)),
        "negative count": rc(table=_table(first, [3, -1, 130], m3)),
        "segment past the buffer": rc(num_rows=first[2] + 129),
        "T < 2": rc(T=1),
        "B < 1": rc(B=0),
        "B * T over the table": rc(table=big, B=17, T=2),
        "counts over Np": rc(Np=132),
        "B * Np over the grid": rc(table=_table([0] * 4, [0] * 4, np.zeros((4, 4, 4))), B=2, T=2, Np=2 ** 30),
    }
    torch.cuda.synchronize()
    assert {k: v for k, v in bad.items() if v != -1} == {}
    assert b"tt_lidar_union_sweeps" in L.tt_last_error()
    assert np.array_equal(whole.cpu().numpy().view(np.uint32), before)
    assert rc() == 0 and rc(points=None, table=_table([0] * 3, [0] * 3, m3), Np=0) == 0     # the good call; an all-empty one
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()[:133 * 5]), _bits(_expected(sweeps, mats, 133)).ravel())


# ------------------------------------------------------------------------------------------------------------ SweepUnion
@pytest.mark.parametrize("name,which", [("wave_edges", 1), ("three_sweeps", 0)])
def test_sweep_union_from_host_device_and_mixed_sweeps(name, which):
    sweeps, mats, Np = _case(name, which, lattice=True)
    want = _expected(sweeps, mats, Np)
    on_dev = [[torch.from_numpy(s).cuda() for s in per] for per in sweeps]
    mixed = [[(torch.from_numpy(s).cuda() if (b + t) % 2 else s) for t, s in enumerate(per)] for b, per in enumerate(sweeps)]
    union = S.SweepUnion(pad_to=Np)
    for form in (sweeps, on_dev, mixed, [[torch.from_numpy(s) for s in per] for per in sweeps]):
        out = union(form, curr2key=mats)
        assert out["points"].shape == (len(sweeps), 1, Np, 5) and out["points"].is_cuda and out["points"].is_contiguous()
        assert np.array_equal(_bits(out["points"].cpu().numpy()[:, 0]), _bits(want))
        assert out["points_size"] == [[len(s) for s in per] for per in sweeps]
    most = max(sum(len(s) for s in per) for per in sweeps)
    out = S.SweepUnion()(sweeps, curr2key=mats)                 # pad_to = None: the batch's largest total
    assert out["points"].shape == (len(sweeps), 1, most, 5)
    assert np.array_equal(_bits(out["points"].cpu().numpy()[:, 0]), _bits(want[:, :most]))


def test_sweep_union_from_can_bus():
    counts = CASES["wave_edges"][0]
    rng = np.random.default_rng(11)
    sweeps = [[R.random_cloud(rng, n) for n in per] for per in counts]
    can_bus = np.stack([R.random_can_bus(rng, 2) for _ in counts])
    out = S.SweepUnion()(sweeps, can_bus)
    mats = out["curr2key"].numpy()
    assert mats.shape == (3, 2, 4, 4) and mats.dtype == np.float32
    assert np.array_equal(_bits(mats), _bits(np.stack([S.curr2key_matrices(c) for c in can_bus])))
    got = out["points"].cpu().numpy()[:, 0]
    _check_fixed_rows(got, sweeps, 320)
    bound = R.collate([R.points_bound(per, m) for per, m in zip(sweeps, mats)], 320).astype(np.float64)
    ratio, exact = R.worst_ratio(got, _expected(sweeps, mats, 320), bound)
    assert exact and ratio <= 1.0


def test_voxelize_gives_the_same_voxels_from_the_device_union_as_from_the_restated_cloud():
    from thinktwice_amd import config
    from thinktwice_amd.lidarnet import LidarNet
    sweeps, mats, Np = _case("three_workgroups", 1, lattice=True)
    sweeps = [[s * np.float32([0.25, 0.25, 0.25, 1.0]) for s in per] for per in sweeps]      # still dyadic; more points in range
    le = dict(config.model_config()["lidar_encoder"])
    le.pop("type")
    net = LidarNet(**le)
    dev = S.SweepUnion(pad_to=Np)(sweeps, curr2key=mats)["points"][:, 0]
    ref = torch.from_numpy(_expected(sweeps, mats, Np)).cuda()
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(ref.cpu().numpy()))
    (fa, ca, na, _), (fb, cb, nb, _) = net.voxelize(dev), net.voxelize(ref)
    n = int(na.item())
    assert n == int(nb.item()) and n > 100
    assert torch.equal(ca[:n], cb[:n]) and np.array_equal(_bits(fa[:n].cpu().numpy()), _bits(fb[:n].cpu().numpy()))


def test_fill_sweeps_feeds_the_camera_meta_assembly():
    from thinktwice_amd import calib, camera, synth
    counts = CASES["wave_edges"][0]
    rng = np.random.default_rng(12)
    sweeps = [[R.random_cloud(rng, n) for n in per] for per in counts]
    can_bus = np.stack([R.random_can_bus(rng, 2) for _ in counts])
    data = synth.make_batch(3, num_points=8, with_img=False)
    ida_before = [[m["ida_mats"].clone() for m in per] for per in data["img_metas"]]
    out = S.SweepUnion()(sweeps, can_bus)
    l2c = np.stack([calib.camera_tables()[1]] * 2)
    metas = [S.sweep_metas(cb, l2c, ps) for cb, ps in zip(can_bus, out["points_size"])]
    assert S.fill_sweeps(data, out, metas) is data and data["points"] is out["points"]
    stacked = camera.stack_img_metas(data["img_metas"])
    for b in range(3):
        for t in range(2):
            meta = data["img_metas"][b][t]
            assert torch.equal(meta["ida_mats"], ida_before[b][t]) and meta["prev_bev"] == (t > 0)
            assert meta["points_size"] == counts[b] and torch.equal(meta["curr2key"], out["curr2key"][b, t])
            assert torch.equal(stacked["sensor2ego_mats"][b, t], meta["currlidar2keycam"].transpose(1, 2))
    assert camera.geometry_matrices(stacked, 0).shape == (12, 2, 4, 4)
    with pytest.raises(ValueError):
        S.fill_sweeps(data, out, metas[:2])
