"""The float64 references and input generators of tests/look_ref.py, held to oracle/model_ref.py on the CPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import look_ref as K  # noqa: E402
from glue_ref import vjp  # noqa: E402

TIGHT = 1e-12


def close(a, b, tol=TIGHT):
    scale = max(float(b.abs().max()), 1.0)
    assert a.shape == b.shape and float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


def oracle_msda(c):
    """oracle.model_ref.msda_core on the kernel layout: value (BC,S,256), offsets (R,512), logits (R,256), ref (R,2)."""
    from oracle import model_ref as M
    hw = c["level_hw"]
    BC = c["value"].shape[0]
    norm = torch.tensor([[w, h] for h, w in hw], dtype=torch.float64)

    def f(value, offsets, logits):
        off = offsets.reshape(BC, K.Q, 8, 4, 8, 2)
        loc = c["ref"].double().reshape(BC, K.Q, 1, 1, 1, 2) + off / norm.view(1, 1, 1, 4, 1, 2)
        aw = logits.reshape(BC, K.Q, 8, 32).softmax(-1).reshape(BC, K.Q, 8, 4, 8)
        return M.msda_core(value.reshape(BC, -1, 8, 32), hw, loc, aw).reshape(BC * K.Q, 256)
    return f


@pytest.mark.parametrize("name", ["random", "lattice"])
def test_msda_ref_and_its_three_gradients_match_the_oracle_core(name):
    """On the lattice case the samples at exactly integral coordinates pin the one-sided (right-hand) offset derivative to
    F.grid_sample's."""
    c = K.msda_case(name, 1)
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(K.CAMS * K.Q, 256, generator=g)
    xs = [c["value"], c["offsets"], c["logits"]]

    def mine(value, offsets, logits):
        return K.msda_ref(value, offsets, logits, c["ref"].double(), c["level_hw"])
    orc = oracle_msda(c)
    with torch.no_grad():
        close(mine(*[x.double() for x in xs]), orc(*[x.double() for x in xs]))
    for a, b in zip(vjp(mine, xs, dy), vjp(orc, xs, dy)):
        close(a, b)
    if name == "lattice":                      # the one-sided derivative is exercised: integral coordinates with a non-zero gradient
        x, _ = K.msda_pixels(c["offsets"].double(), c["ref"].double(), c["level_hw"])
        d = vjp(mine, xs, dy)[1].reshape(-1, 8, 4, 8, 2)[..., 0]
        assert int(((x == x.round()) & (d != 0)).sum()) > 100


def test_msda_ref_reads_its_channel_window():
    c = K.random_case(1)
    wide = torch.full((K.CAMS, c["value"].shape[1], 320), float("nan"), dtype=torch.float64)
    wide[..., 32:288] = c["value"].double()
    a = K.msda_ref(wide, c["offsets"].double(), c["logits"].double(), c["ref"].double(), c["level_hw"], coff=32)
    assert torch.equal(a, K.msda_forward_refs("random", 1)[0])


def test_msda_proj_ref_is_msda_ref_on_the_projected_value():
    g = torch.Generator().manual_seed(4)
    c = K.random_case(1)
    maps = [torch.randn(K.CAMS, h, w, 256, generator=g, dtype=torch.float64) for h, w in c["level_hw"]]
    W = torch.randn(256, 256, generator=g, dtype=torch.float64) / 16
    bias, vshift = torch.randn(256, generator=g, dtype=torch.float64), torch.randn(4, 4, 256, generator=g, dtype=torch.float64)
    value = torch.empty(K.CAMS, c["value"].shape[1], 256, dtype=torch.float64)
    start = 0
    for lv, m in enumerate(maps):                                   # position by position, camera by camera
        for bc in range(K.CAMS):
            value[bc, start:start + m.shape[1] * m.shape[2]] = torch.nn.functional.linear(m[bc].reshape(-1, 256), W, bias) + vshift[lv, bc % 4]
        start += m.shape[1] * m.shape[2]
    args = [c["offsets"].double(), c["logits"].double(), c["ref"].double()]
    close(K.msda_proj_ref(maps, *args, W, bias, vshift), K.msda_ref(value, *args, c["level_hw"]))


def _oracle_pack(wp, l2i, ida, hw):
    from oracle import model_ref as M
    ref, mask = M.project_queries(K.look_points(wp), l2i.double(), ida.double(), hw)
    order = torch.argsort((~mask).to(torch.int8), dim=-1, stable=True)
    count = mask.sum(-1)
    slot_ok = torch.arange(120).view(1, 1, 120) < count.unsqueeze(-1)
    rpack = torch.gather(ref, 2, order.unsqueeze(-1).expand(-1, -1, -1, 2)) * slot_ok.unsqueeze(-1)
    qos = torch.where(slot_ok, order, torch.full_like(order, -1))
    return rpack, qos, count, int(count.max()), ref, mask


PROJ_CASES = [("dyadic", 0)] + [("random", s) for s in K.PROJ_SEEDS] + [("degenerate", 0)]


def projection_case(kind, seed, B):
    if kind == "dyadic":
        return K.dyadic_projection_case(B)
    wp, l2i, ida, hw = K.random_projection_case(B, seed)
    return (wp, torch.zeros_like(l2i), ida, hw) if kind == "degenerate" else (wp, l2i, ida, hw)


@pytest.mark.parametrize("kind,seed", PROJ_CASES, ids=[f"{k}{s}" for k, s in PROJ_CASES])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_project_pack_ref_matches_the_oracle_projection_and_packing(kind, seed, B):
    wp, l2i, ida, hw = projection_case(kind, seed, B)
    packed, qos, count, max_len, bound = K.project_pack_ref(wp, l2i, ida, hw)
    o_packed, o_qos, o_count, o_max, _, _ = _oracle_pack(wp, l2i, ida, hw)
    close(packed, o_packed)
    assert torch.equal(qos.long(), o_qos) and torch.equal(count.long(), o_count) and max_len == o_max
    assert bool((packed[qos < 0] == 0).all()) and bool((bound >= 0).all())
    if kind == "degenerate":
        assert max_len == 0 and int(count.abs().sum()) == 0


@pytest.mark.parametrize("B", [1, 2, 3])
def test_random_projection_cases_have_no_ambiguous_point(B):
    for seed in K.PROJ_SEEDS:
        wp, l2i, ida, hw = K.random_projection_case(B, seed)
        assert int(K.ambiguous_points(wp, l2i, ida, hw).sum()) == 0, seed
        _, _, count, max_len, _ = K.project_pack_ref(wp, l2i, ida, hw)
        assert 0 < max_len < 120 and int((count > 0).sum()) >= 2           # something is packed, something is padded


@pytest.mark.parametrize("B", [1, 3])
def test_dyadic_projection_case_holds_what_it_promises(B):
    wp, l2i, ida, hw = K.dyadic_projection_case(B)
    rx, ry, iz, _, _, _ = K.project_ref(wp, l2i, ida, hw)
    _, qos, count, _, _ = K.project_pack_ref(wp, l2i, ida, hw)
    for b in range(B):
        assert count[b].tolist()[:2] == [120, 0]
        assert bool((iz[b, 1] == K.EPS32).all())                                  # excluded by the strict comparison alone
        first = int(((qos[b, 2] >= 0) & (qos[b, 2] < 64)).sum())
        assert 0 < first < int(count[b, 2]) < 120                                 # sparse, on both sides of the ballot boundary
        assert bool((iz[b, 2] < 0).any()) and bool((iz[b, 2] == 0).any())          # behind the camera, and on its plane
        front = iz[b, 3] > K.EPS32
        for v in (rx[b, 3], ry[b, 3]):
            assert bool(((v == 0) & front).any()) and bool(((v == 1) & front).any())
    # exact in f32: the f32 evaluation of the same expression gives the same packed values
    p32 = K.project_pack_ref(wp, l2i, ida, hw)[0].float().double()
    assert torch.equal(p32, K.project_pack_ref(wp, l2i, ida, hw)[0])


@pytest.mark.parametrize("raw_ctrl", [False, True])
def test_gather_query_ref_matches_the_oracle_query_rows(raw_ctrl):
    """Against the query / grid_sample / gather lines of oracle.model_ref.look_module, with the oracle's own packing order."""
    import torch.nn.functional as F
    B = 2
    g = torch.Generator().manual_seed(11)
    wp, l2i, ida, hw = K.random_projection_case(B, 0)
    _, _, t, maps = K.gather_inputs(B, g)
    o_packed, o_qos, count, _, ref_full, mask = _oracle_pack(wp, l2i, ida, hw)
    ctrl_sp = F.softplus(t["ctrl"]) if raw_ctrl else t["ctrl"]
    p3 = K.look_points(wp)
    ctrl_q = torch.cat([ctrl_sp.unsqueeze(2).expand(B, 4, 15, 4).reshape(B, 60, 4), torch.zeros(B, 60, 4, dtype=torch.float64)], 1)
    emb = torch.cat([t["temporal"].unsqueeze(1).expand(4, 15, 128).reshape(60, 128),
                     t["static"].unsqueeze(1).expand(4, 15, 128).reshape(60, 128)], 0).unsqueeze(0).expand(B, 120, 128)
    query = torch.cat([ctrl_q, p3, emb, t["meas"].unsqueeze(1).expand(B, 120, 128), t["flat"].unsqueeze(1).expand(B, 120, 256)], -1)
    grid = ref_full.reshape(B * 4, 120, 1, 2) * 2 - 1.0
    samp = [F.grid_sample(m.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros", align_corners=False)[..., 0] for m in maps]
    samp = torch.stack(samp, -1).permute(0, 2, 1, 3).reshape(B, 4, 120, 1024)
    order = torch.argsort((~mask).to(torch.int8), dim=-1, stable=True)
    slot_ok = torch.arange(120).view(1, 1, 120) < count.unsqueeze(-1)
    qfull = torch.cat([query.unsqueeze(1).expand(B, 4, 120, 519), samp], -1)
    want = torch.gather(qfull, 2, order.unsqueeze(-1).expand(B, 4, 120, 1543)) * slot_ok.unsqueeze(-1)
    got = K.gather_query_ref(o_qos.to(torch.int32), o_packed, wp.double(), t["ctrl"], t["temporal"], t["static"], t["meas"], t["flat"],
                             maps, raw_ctrl=raw_ctrl)
    close(got, want.reshape(-1, 1543))
    assert int(count.sum()) > 100


def test_gather_query_ref_on_the_hand_made_slots_matches_grid_sample():
    import torch.nn.functional as F
    B = 1
    g = torch.Generator().manual_seed(12)
    qos, ref, t, maps = K.gather_inputs(B, g)
    got = K.gather_query_ref(qos, ref.double(), t["wp"], t["ctrl"], t["temporal"], t["static"], t["meas"], t["flat"], maps)
    grid = ref.double().reshape(4, 120, 1, 2) * 2 - 1
    samp = torch.stack([F.grid_sample(m.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros", align_corners=False)[..., 0]
                        for m in maps], -1).permute(0, 2, 1, 3).reshape(480, 1024)
    live = (qos.reshape(-1) >= 0)
    close(got[:, 519:], samp * live.unsqueeze(1))
    assert bool((got[~live] == 0).all()) and int((~live).sum()) > 80


@pytest.mark.parametrize("B", [1, 2, 3])
def test_sca_reduce_ref_is_the_three_reference_lines(B):
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B * 4 * 120, 256, generator=g, dtype=torch.float64)
    for max_len in (0, B - 1, B, B + 1, 64, 119, 120, 500):
        ml = min(max_len, 120)
        att = x.reshape(B, 4, 120, 256)[:, :, :ml].clone()
        att[:, :, :B] = 0
        att = att / max(B, 1.0)
        close(K.sca_reduce_ref(x, max_len, B), att.sum(-2).reshape(B, 1024))


def test_merge_in_ref_is_layer_norm_of_the_concatenation():
    g = torch.Generator().manual_seed(2)
    B = 3
    fflat, look, temporal, meas = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((B * 4, 256), (B, 256), (4, 128), (B, 128)))
    cat = K.merge_in_cat(fflat, look, temporal, meas)
    for b in range(B):
        for t in range(4):
            assert torch.equal(cat[b * 4 + t], torch.cat([fflat[b * 4 + t], look[b], torch.zeros(256, dtype=torch.float64), temporal[t], meas[b]]))


# ----------------------------------------------------------------------------- the generators' conditions
@pytest.mark.parametrize("B", [1, 2, 3])
def test_random_case_conditions(B):
    c = K.random_case(B)
    x, y = K.msda_pixels(c["offsets"].double(), c["ref"].double(), c["level_hw"])
    assert int(K.integer_band(x).sum()) == 0 and int(K.integer_band(y).sum()) == 0
    n_in = n_all = 0
    for lv, (H, W) in enumerate(c["level_hw"]):
        _, _, valid = K.bilinear_corners(x[:, :, lv], y[:, :, lv], H, W)
        n_in += int(valid.sum())
        n_all += valid.numel()
    assert 0.2 <= n_in / n_all <= 0.8, n_in / n_all
    lg = c["logits"].reshape(-1, 8, 32)
    assert float(lg.abs().max()) > 25 and bool((lg[:, 3] == lg[:, 3, :1]).all())
    assert bool(((lg[:, 5].max(-1).values - lg[:, 5].median(-1).values) > 15).all())


@pytest.mark.parametrize("B", [1, 2, 3])
def test_lattice_case_conditions(B):
    c = K.lattice_case(B)
    x, y = K.msda_pixels(c["offsets"].double(), c["ref"].double(), c["level_hw"])
    x32, y32 = K.msda_pixels(c["offsets"], c["ref"], c["level_hw"])
    assert torch.equal(x32.double(), x) and torch.equal(y32.double(), y)           # exact in f32
    assert torch.equal(c["ref"] * 64, (c["ref"] * 64).round()) and torch.equal(c["offsets"] * 8, (c["offsets"] * 8).round())
    for lv, (H, W) in enumerate(c["level_hw"]):
        for t in K.lattice_targets(W):
            assert int((x[:, :, lv] == t).sum()) > 0, (lv, "x", t)
        for t in K.lattice_targets(H):
            assert int((y[:, :, lv] == t).sum()) > 0, (lv, "y", t)
        if W > 2:                                                                  # an interior exact integer
            assert int(((x[:, :, lv] == W // 2) & (y[:, :, lv] > 0) & (y[:, :, lv] < H - 1)).sum()) > 0
