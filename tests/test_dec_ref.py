"""The references and limits of tests/dec_ref.py, checked on the CPU: the float64 restatements against the oracle the goldens
were checked against, the operand split, the window every GPU case's limit must lie in (so that test_dec_ops.py is neither
vacuous nor unreachable), and two subtly wrong emulations that the limits catch -- and the old 1e-3 tolerance would not, had the
fault been ten times smaller."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dec_ref as D  # noqa: E402
from dec_ref import A64, BEV_Q, GRU_P, X3, rel_err  # noqa: E402


def _sd64(sd):
    return {k: v.double() for k, v in sd.items()}


# ----------------------------------------------------------------------------- the restatements are the oracle's functions
def test_gru_restatement_is_the_oracle():
    from oracle import model_ref as M
    c = D.gru_case("B2")
    sd = _sd64(c["sd"])
    with torch.no_grad():
        want = M.spatial_gru(sd, GRU_P, c["inp6"].double()[..., None, None].expand(-1, 4, 6, 21, 21), c["state"].double())
    for t in range(4):
        assert rel_err(c["ref"][t], want[:, t]) < 1e-12


def test_grid2feat_restatement_is_the_oracle():
    from oracle import model_ref as M
    c = D.flat_case("maps4")
    with torch.no_grad():
        flat, mids = M.flatten_tail(_sd64(c["sd"]), c["maps"].double())
    for got, want in zip(c["ref"], mids + [flat]):
        assert rel_err(got, want) < 1e-12


def test_bev_update_restatement_is_the_oracle():
    from oracle import model_ref as M
    c = D.bev_case("B1")
    sd, q = _sd64(c["sd"]), BEV_Q
    bev, hb = c["bev"].double(), c["hb"].double()
    with torch.no_grad():
        x = torch.cat([bev, hb[..., None, None].expand(-1, 2048, 21, 21)], 1)
        want = M.conv(sd, q + ".BEV_feat_update_module.2", F.relu(M.conv(sd, q + ".BEV_feat_update_module.0", x, 1, 1)), 1, 1) + bev
        g_want = torch.einsum("nckl,bc->bkln", sd[q + ".BEV_feat_update_module.0.weight"][:, 32:], hb).reshape(-1, 1152)
    assert rel_err(c["ref"][0], g_want) < 1e-12
    assert rel_err(c["ref"][1], want) < 1e-12


def test_chain_restatement_is_torch_linear():
    c = D.chain_case("res-side2-R45")
    st = c["stages"][0]
    x = torch.cat([st["side"][:, :2], c["x"][:, :64]], 1).double()
    want = F.relu(F.linear(x, st["w"].double(), st["bias"].double()) + st["res"][:, 8:48].double())
    assert rel_err(c["ref"][0], want) < 1e-12


def test_border_classes_and_tap_table():
    cls, v = D.border_classes(), D.valid_taps()
    assert cls[0, 0] == 0 and cls[0, 20] == 2 and cls[20, 0] == 6 and cls[20, 20] == 8 and cls[7, 9] == 4 and cls[0, 5] == 1
    n = v.sum(0)
    assert bool((n[cls == 4] == 9).all()) and all(bool((n[cls == k] == 4).all()) for k in (0, 2, 6, 8))
    assert all(bool((n[cls == k] == 6).all()) for k in (1, 3, 5, 7))
    assert int(D.valid_taps(True).sum()) == int(v.sum()) + 1


# ----------------------------------------------------------------------------- the split
def test_split_carries_sixteen_bits():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-20, 20, (1 << 16,), generator=g).float())
    hi, lo = D.split(x)
    assert bool(((hi + lo - x).abs() <= 2.0 ** -16 * x.abs()).all())
    assert bool((hi.bfloat16().float() == hi).all()) and bool((lo.bfloat16().float() == lo).all())
    exact = x.bfloat16().float()
    assert bool((D.split(exact)[1] == 0).all())
    assert bool((D.pair_round(exact) == exact).all())


# ----------------------------------------------------------------------------- every GPU case's limit lies in the window
def _window(c, what):
    for i, lim in enumerate(c["limit"]):
        f32 = rel_err(c["f32"][i], c["ref"][i])
        assert lim < 1e-4, (what, i, lim)
        assert lim > f32, (what, i, lim, f32)
        assert all(bool(torch.isfinite(t[i]).all()) for t in (c["ref"], c["emu"], c["f32"])), (what, i)


@pytest.mark.parametrize("name", D.GRU_CASES)
def test_gru_limits_are_neither_vacuous_nor_unreachable(name):
    c = D.gru_case(name)
    _window(c, name)
    assert c["limit"][3] <= 4.0 * c["limit"][0], c["limit"]           # the recurrence does not amplify
    print(name, ["%.2e" % v for v in c["limit"]])


@pytest.mark.parametrize("name", D.FLAT_CASES)
def test_flatten_limits_are_neither_vacuous_nor_unreachable(name):
    _window(D.flat_case(name), name)
    print(name, ["%.2e" % v for v in D.flat_case(name)["limit"]])


@pytest.mark.parametrize("name", D.BEV_CASES)
def test_bev_limits_are_neither_vacuous_nor_unreachable(name):
    _window(D.bev_case(name), name)
    print(name, ["%.2e" % v for v in D.bev_case(name)["limit"]])


@pytest.mark.parametrize("name", D.CHAIN_CASES)
def test_chain_limits_are_neither_vacuous_nor_unreachable(name):
    _window(D.chain_case(name), name)


def test_saturated_case_saturates():
    """The +-100 channels are exactly 0 / 1 in f32 and the +-12 ones within 1e-5 of it: the case reaches the tails it is for."""
    c = D.gru_case("saturated")
    b = c["sd"][f"{GRU_P}.conv_update.2.bias"]
    assert float(torch.sigmoid(b[16:18] - 5).min()) == 1.0 and float(torch.sigmoid(b[18:20] + 5).max()) == 0.0
    assert float(b[0:8].min()) > 11.8 and float(b[8:16].max()) < -11.8


# ----------------------------------------------------------------------------- a subtly wrong kernel would be caught
def _over(fn, c, idx, kernel):
    """The worst error of the wrong emulation fn(A) over tensor idx's limit: `check` must refuse it."""
    with torch.no_grad():
        bad = fn(c)
    err = rel_err(bad[idx], c["ref"][idx])
    with pytest.raises(AssertionError, match="over its limit"):
        D.check_rule(kernel + " (wrong on purpose)", "cpu", bad[idx], c["ref"][idx], c["limit"][idx], c["scale"][idx])
    D.G._WORST.pop(kernel + " (wrong on purpose)", None)
    assert err > c["limit"][idx]
    return err


def _gru(A):
    return lambda c: D.spatial_gru(A, c["sd"], GRU_P, c["inp6"], c["state"])


def _flat(A):
    def run(c):
        flat, mids = D.grid2feat(A, c["sd"], c["maps"])
        return mids + [flat]
    return run


def _bev(A):
    return lambda c: [D.bev_g(A, c["sd"], BEV_Q, c["hb"]), D.bev_update(A, c["sd"], BEV_Q, c["bev"], c["hb"])]


def test_a_dropped_cross_term_is_over_every_limit_and_near_the_old_tolerance():
    """lo * hi dropped: over the limit of every output -- but only 2 - 4 x the 1e-3 that tests/test_decoder_fused.py allows, so a
    fault a tenth of that size (a lo half wrong on a tenth of the K steps) passes there and is still over the limits here."""
    A = X3(drop_lo_hi=True)
    for fn, c, idxs, kernel in ((_gru(A), D.gru_case("B2"), range(4), "dec_gru"), (_flat(A), D.flat_case("maps4"), range(4), "dec_flatten"),
                                (_bev(A), D.bev_case("B1"), (0, 1), "dec_bev_update")):
        for i in idxs:
            err = _over(fn, c, i, kernel)
            print(kernel, i, "dropped lo*hi: %.2e, limit %.2e" % (err, c["limit"][i]))
            assert err < 1e-2, (kernel, i, err)                   # nothing like a wide margin over 1e-3 ...
            assert c["limit"][i] < err / 10 < 1e-3, (kernel, i, err, c["limit"][i])     # ... and a tenth of it: old passes, new fails


def test_a_ninth_tap_in_one_corner_class_is_over_the_limit():
    """The constant-input term of border class 0 summing the tap outside the map as well (the GRU's six input channels; the BEV
    update's broadcast channels; grid2feat has no such term)."""
    A = X3(ninth_tap=True)
    for i in range(4):
        _over(_gru(A), D.gru_case("B2"), i, "dec_gru")
    _over(_bev(A), D.bev_case("B1"), 1, "dec_bev_update")
    with torch.no_grad():                                         # the term is not in G, and not in grid2feat
        assert torch.equal(_bev(A)(D.bev_case("B1"))[0], D.bev_case("B1")["emu"][0])
