"""CPU: the numpy restatement of union2one (tests/sweep_union_ref.py) and the host functions of thinktwice_amd/sweeps.py against
golden F20, which is the reference's own union2one on four tiny queues (tests/golden/README_f20.md).

Bit for bit, as uint32 / uint64: the key sweep's rows, the time column, prev_bev, the rewritten can_bus, points_size, every
matrix entry that involves no sum (the rotation block, the zeros and ones, the key frame's identity and its lidar2cam).

Within a bound that follows from the arithmetic, computed per element from the inputs: the two translation entries of curr2key,
currlidar2keycam and the moved coordinates.  Any f32 evaluation of an n-term dot product -- any order, fused multiply-add or
not -- differs from the exact value by at most gamma_n * sum |a_k b_k|, gamma_n = n u / (1 - n u), u = 2^-24; two evaluations
therefore by at most twice that (sweep_union_ref.matmul_bound; n = the number of non-zero terms: 2 for a translation entry of
R @ T in the closed form sweeps.curr2key_matrix uses, up to 4 for a point component or an entry of lidar2cam @ curr2key).
Where one side's operand is itself only known within such a bound (currlidar2keycam from OUR curr2key against the reference's
from ITS curr2key), the operand's bound is carried through: |L| @ dM, times 1 + 2 gamma_4 for its own rounding.

Every comparison prints its largest error / bound ratio (pytest -s); the figures are recorded in profiles/train_lidar_union.txt."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sweep_union_ref as R  # noqa: E402
from thinktwice_amd import sweeps as S  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f20_sweep_union.npz")
NUM_QUEUES = 4


@functools.lru_cache(maxsize=None)
def _golden():
    """[(dict of one queue's arrays, its clouds split per frame)], lidar2cam: loaded once, read-only."""
    z = np.load(GOLDEN)
    queues = []
    for q in range(NUM_QUEUES):
        g = {k[len(f"q{q}_"):]: z[k] for k in z.files if k.startswith(f"q{q}_")}
        for a in g.values():
            a.setflags(write=False)
        clouds = np.split(g["clouds_in"], np.cumsum(g["sizes"])[:-1])
        queues.append((g, clouds))
    l2c = z["lidar2cam"]
    l2c.setflags(write=False)
    return queues, l2c


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _curr2key_bound(can_bus_in):
    """[T, 4, 4]: matmul_bound(R, T) of every older frame -- non-zero only at the two translation entries ... and at the entries
    that are a single product by 1 (n = 1), which are exact all the same and are compared bit for bit besides."""
    T = len(can_bus_in)
    return np.stack([R.matmul_bound(*R.rotation_translation(can_bus_in[-1], can_bus_in[t])) for t in range(T - 1)]
                    + [np.zeros((4, 4))])


def _check_curr2key(got, g, who):
    bound = _curr2key_bound(g["can_bus_in"])
    ratio, exact = R.worst_ratio(got, g["curr2key"], bound)
    print(f"{who}: curr2key, worst |error| / bound = {ratio:.3f}")
    assert exact and ratio <= 1.0
    no_sum = np.ones((4, 4), bool)
    no_sum[:2, 3] = False
    assert np.array_equal(_bits(np.asarray(got)[:, no_sum]), _bits(g["curr2key"][:, no_sum]))
    assert np.array_equal(_bits(np.asarray(got)[-1]), _bits(np.eye(4, dtype=np.float32)))
    return bound


def _check_currlidar2keycam(got, own_curr2key, c2k_bound, g, l2c, who):
    T = len(g["sizes"])
    worst = 0.0
    for t in range(T - 1):
        L = l2c.astype(np.float64)
        bound = R.matmul_bound(l2c, g["curr2key"][t]) + np.abs(L) @ c2k_bound[t] * (1 + 2 * R.gamma(4))
        ratio, exact = R.worst_ratio(got[t], g["currlidar2keycam"][t], bound)
        assert exact and ratio <= 1.0, (t, ratio)
        worst = max(worst, ratio)
    print(f"{who}: currlidar2keycam, worst |error| / bound = {worst:.3f}")
    assert np.array_equal(_bits(got[-1]), _bits(g["currlidar2keycam"][-1]))          # the key frame's: its lidar2cam
    assert np.array_equal(_bits(got[-1]), _bits(l2c))


# -------------------------------------------------------------------------------------------------- the golden itself
def test_golden_f20_holds_the_cases_it_is_for():
    queues, l2c = _golden()
    assert sorted(len(g["sizes"]) for g, _ in queues) == [2, 2, 3, 3]
    assert {0, 1, 5, 67} == {int(n) for g, _ in queues for n in g["sizes"]}
    assert any(g["sizes"][-1] == 0 for g, _ in queues) and l2c.shape == (4, 4, 4)
    inten = np.concatenate([g["clouds_in"][:, 3] for g, _ in queues])
    assert ((inten != 0) & (inten != 1)).all() and inten.max() > 2
    diffs = np.concatenate([g["can_bus_in"][-1, -2] - g["can_bus_in"][:-1, -2] for g, _ in queues])
    assert (diffs > np.pi).any() and (diffs < -np.pi).any() and (np.abs(diffs) < np.pi).any()
    for g, _ in queues:                      # the intensity-as-w quirk: the translation of a moved point is scaled by it
        assert g["points"].shape == (1, int(g["sizes"].sum()), 5) and g["points"].dtype == np.float32


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("q", range(NUM_QUEUES))
def test_restated_cloud_against_the_reference(q):
    g, clouds = _golden()[0][q]
    got = R.union_points(clouds, g["curr2key"])                  # under the reference's own matrices
    want = g["points"][0]
    assert got.shape == want.shape and got.dtype == np.float32
    n_key = int(g["sizes"][-1])
    assert np.array_equal(_bits(got[:n_key]), _bits(want[:n_key]))                       # copied rows, time 0 included
    assert np.array_equal(_bits(got[:n_key, :4]), _bits(clouds[-1]))
    assert np.array_equal(_bits(got[:, 4]), _bits(want[:, 4]))                           # the time column
    T = len(clouds)
    times = np.concatenate([np.full(len(clouds[t]), t - (T - 1), np.float32) for t in range(T - 1, -1, -1)])
    assert np.array_equal(_bits(got[:, 4]), _bits(times))
    ratio, exact = R.worst_ratio(got, want, R.points_bound(clouds, g["curr2key"]))
    print(f"queue {q}: restated moved coordinates, worst |error| / bound = {ratio:.3f}")
    assert exact and ratio <= 1.0


def test_the_intensity_stands_in_for_w():
    """A moved point is M[:, :3] . xyz + intensity * M[:, 3], and its new 'intensity' is row 3 of M applied likewise."""
    g, clouds = _golden()[0][0]
    M, p = g["curr2key"][0].astype(np.float64), clouds[0].astype(np.float64)
    moved = g["points"][0][len(clouds[1]):, :4].astype(np.float64)
    assert np.allclose(moved, p[:, :3] @ M[:, :3].T + p[:, 3:4] * M[:, 3], rtol=0, atol=1e-4)
    assert not np.allclose(moved[:, :3], (p[:, :3] @ M[:3, :3].T + M[:3, 3]), rtol=0, atol=1e-2)    # NOT the homogeneous form


@pytest.mark.parametrize("q", range(NUM_QUEUES))
def test_restated_metas_against_the_reference(q):
    (g, clouds), l2c = _golden()[0][q], _golden()[1]
    T = len(clouds)
    metas = R.sweep_metas(g["can_bus_in"], [l2c] * T, g["sizes"].tolist())
    assert np.array_equal(_bits(np.stack([m["can_bus"] for m in metas])), _bits(g["can_bus"]))
    assert [m["prev_bev"] for m in metas] == g["prev_bev"].tolist() == [False] + [True] * (T - 1)
    assert all(m["points_size"] == g["sizes"].tolist() for m in metas)
    c2k = np.stack([m["curr2key"] for m in metas])
    bound = _check_curr2key(c2k, g, f"queue {q} restated")
    _check_currlidar2keycam([m["currlidar2keycam"] for m in metas], c2k, bound, g, l2c, f"queue {q} restated")


def test_lattice_cases_are_exact_in_any_order():
    """The lattice generators' promise: every product and partial sum is exact in f32, so the float64-accumulated restatement,
    an f32 sum in column order and one in reverse order agree in every bit."""
    sweeps, mats = R.make_case(3, [[40, 90]], lattice=True)
    p, m = sweeps[0][0], mats[0, 0]
    want = R.union_points(sweeps[0], mats[0])[len(sweeps[0][1]):, :4]
    fwd = ((m[:, 0] * p[:, 0:1] + m[:, 1] * p[:, 1:2]) + m[:, 2] * p[:, 2:3]) + m[:, 3] * p[:, 3:4]
    rev = ((m[:, 3] * p[:, 3:4] + m[:, 2] * p[:, 2:3]) + m[:, 1] * p[:, 1:2]) + m[:, 0] * p[:, 0:1]
    assert fwd.dtype == np.float32 and np.array_equal(_bits(fwd), _bits(want)) and np.array_equal(_bits(rev), _bits(want))
    assert np.isnan(mats[:, -1]).all() and (m[3] != [0, 0, 0, 1]).any()


# ------------------------------------------------------------------------------------------- thinktwice_amd/sweeps.py
def test_ego_shift_is_the_restatement():
    rng = np.random.default_rng(1)
    for dx, dy, yaw in rng.uniform(-200, 200, (50, 3)).tolist() + [[0.0, 0.0, 10.0], [0.0, -1.0, 180.0]]:
        assert S.ego_shift(dx, dy, yaw) == R.ego_shift(dx, dy, yaw)


@pytest.mark.parametrize("q", range(NUM_QUEUES))
def test_sweep_metas_against_the_reference(q):
    (g, clouds), l2c = _golden()[0][q], _golden()[1]
    T = len(clouds)
    metas = S.sweep_metas(g["can_bus_in"], np.stack([l2c] * T), g["sizes"].tolist())
    assert len(metas) == T
    assert np.array_equal(_bits(np.stack([m["can_bus"] for m in metas])), _bits(g["can_bus"]))
    assert all(m["can_bus"].dtype == np.float64 for m in metas)
    assert [m["prev_bev"] for m in metas] == g["prev_bev"].tolist()
    assert all(m["points_size"] == g["sizes"].tolist() for m in metas)
    c2k = np.stack([m["curr2key"].numpy() for m in metas])
    assert c2k.dtype == np.float32
    bound = _check_curr2key(c2k, g, f"queue {q} sweeps.py")
    l2k = [m["currlidar2keycam"].numpy() for m in metas]
    assert all(a.dtype == np.float32 and a.shape == (4, 4, 4) for a in l2k)
    _check_currlidar2keycam(l2k, c2k, bound, g, l2c, f"queue {q} sweeps.py")
    assert np.array_equal(_bits(S.curr2key_matrices(g["can_bus_in"])), _bits(c2k))
    assert np.array_equal(g["can_bus_in"], np.load(GOLDEN)[f"q{q}_can_bus_in"])          # the inputs were not written to


def test_curr2key_matrix_closed_form():
    """The form the docstring states: two rounded products and one rounded add per translation entry, nothing fused."""
    rng = np.random.default_rng(2)
    for _ in range(20):
        cb = R.random_can_bus(rng, 2)
        rot, tr = R.rotation_translation(cb[1], cb[0])
        m = S.curr2key_matrix(cb[1], cb[0])
        c, s, tx, ty = rot[0, 0], rot[0, 1], tr[0, 3], tr[1, 3]
        assert m.dtype == np.float32
        assert m[0, 3] == np.float32(np.float32(c * tx) + np.float32(s * ty))
        assert m[1, 3] == np.float32(np.float32(-s * tx) + np.float32(c * ty))
        want = rot.copy()
        want[:2, 3] = m[:2, 3]
        assert np.array_equal(_bits(m), _bits(want + np.float32(0)))


def test_sweep_union_refuses_what_the_reference_does_not_build():
    cloud = np.zeros((3, 4), np.float32)
    cb = np.zeros((1, 2, 18))
    with pytest.raises(ValueError, match="carla_dataset.py:327-328"):
        S.SweepUnion()([[cloud]], cb[:, :1])
    with pytest.raises(ValueError, match="pad_to"):
        S.SweepUnion(pad_to=5)([[cloud, cloud]], cb)
    with pytest.raises(ValueError, match="at most"):
        S.SweepUnion()([[cloud, cloud]] * 17, np.zeros((17, 2, 18)))
    with pytest.raises(ValueError, match="same number of sweeps"):
        S.SweepUnion()([[cloud, cloud], [cloud]], cb)
    with pytest.raises(ValueError, match="float32"):
        S.SweepUnion()([[cloud.astype(np.float64), cloud]], cb)
    with pytest.raises(ValueError):
        S.SweepUnion(pad_to=-1)
