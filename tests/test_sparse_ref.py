"""The references of tests/sparse_ref.py against torch itself, on the CPU: the generalised rulebook builder against F.conv3d on the
scattered grid (and against tests/test_conv.py::_grid_rulebook where the two overlap), the symmetry and uniqueness conditions on
every rulebook the GPU tests use, the dense layout against spconv's dense().view(), and the two float64 losses against
oracle/train_ref.py.  No test here needs a device; the last one asks the library's host-only chooser."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sparse_ref as S  # noqa: E402
from glue_ref import vjp  # noqa: E402
from test_conv import _grid_rulebook  # noqa: E402


@pytest.mark.parametrize("stride,geom", [(1, "subm"), (2, "s2")])
def test_rulebook_reproduces_grid_rulebook_where_they_overlap(stride, geom):
    dims, occ = (2, 7, 12, 13), 0.3
    want, rows_in = _grid_rulebook(*dims, occ, stride, torch.Generator().manual_seed(5))
    nbr, coords, rows = S.rulebook(S.occupancy(*dims, occ, torch.Generator().manual_seed(5)), **S.GEOM[geom])
    assert rows == rows_in and torch.equal(nbr, want) and coords.shape == (nbr.shape[0], 4)


@pytest.mark.parametrize("geom", list(S.GEOM))
def test_rulebook_gather_matmul_is_conv3d_on_the_scattered_grid(geom):
    """Scatter to a dense grid, F.conv3d in float64: equal to gather-and-matmul on every live output cell, and (strided layers) zero on
    every other cell.  Rows are in (b, z, y, x) cell order."""
    G = S.GEOM[geom]
    g = torch.Generator().manual_seed(len(geom))
    vol = S.occupancy(2, 5, 7, 8, 0.08, g)
    nbr, coords, rows_in = S.rulebook(vol, **G)
    taps = G["kernel"][0] * G["kernel"][1] * G["kernel"][2]
    assert nbr.shape[1] == taps and rows_in == int(vol.sum())
    feats = torch.randn(rows_in, 3, generator=g, dtype=torch.float64)
    w = torch.randn(4, 1, taps, 3, generator=g, dtype=torch.float64)
    dense = S.dense_conv3d(feats, vol, w, G["kernel"], G["stride"], G["pad"])
    assert tuple(dense.shape[2:]) == S.out_dims((5, 7, 8), G["kernel"], G["stride"], G["pad"], G["subm"])
    c = coords.long()
    got = S.gather_matmul(feats, nbr, w)
    assert float((dense[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] - got).abs().max()) < 1e-12
    key = ((c[:, 0] * dense.shape[2] + c[:, 1]) * dense.shape[3] + c[:, 2]) * dense.shape[4] + c[:, 3]
    assert bool((key[1:] > key[:-1]).all())                    # cell order, no cell twice
    if G["subm"]:
        assert torch.equal(c, vol.nonzero())
    else:
        live = torch.zeros(dense.shape[0], *dense.shape[2:], dtype=torch.bool)
        live[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = True
        assert int((~live).sum()) > 0 and float(dense.permute(0, 2, 3, 4, 1)[~live].abs().max()) == 0.0
        assert bool((nbr >= 0).any(1).all())                   # every output row has an input


@pytest.mark.parametrize("name", S.all_rulebook_names())
def test_symmetry_and_uniqueness_hold_on_every_rulebook_the_gpu_tests_use(name):
    """Conditions, not measurements: the submanifold input gradient reuses the layer's rulebook with flipped taps, the strided one
    stores one output row per (input row, tap)."""
    rb = S.case_rulebook(name)
    nbr, rows_in = rb["nbr"], rb["rows_in"]
    taps = nbr.shape[1]
    if rb["geom"]["subm"]:
        S.assert_subm_symmetry(nbr)
        assert torch.equal(nbr[:, taps // 2].long(), torch.arange(rows_in))      # the centre tap is the row itself
    S.assert_inverse_unique(nbr, rows_in)
    inv = S.inverse_rulebook(nbr, nbr.shape[0], rows_in + 3)
    m, t = (nbr >= 0).nonzero(as_tuple=True)
    assert torch.equal(inv[nbr[m, t].long(), t].long(), m) and int((inv >= 0).sum()) == m.numel()
    assert bool((inv[rows_in:] == -1).all())
    if rb["geom"]["subm"]:      # the flipped rulebook IS the transposed one
        assert torch.equal(inv[:rows_in], nbr.flip(1))


def test_the_conditions_notice_a_broken_rulebook():
    nbr = S.case_rulebook("subm 32->32 small")["nbr"]
    with pytest.raises(AssertionError):
        S.assert_subm_symmetry(nbr.roll(1, 1))
    dup = S.case_rulebook("3 taps")["nbr"].clone()
    m, t = (dup >= 0).nonzero(as_tuple=True)
    dup[(m[0] + 1) % dup.shape[0], t[0]] = dup[m[0], t[0]]
    with pytest.raises(AssertionError):
        S.assert_inverse_unique(dup, S.case_rulebook("3 taps")["rows_in"])
    # live count: rows beyond it are not transposed, and a count above M clamps
    nbr = S.case_rulebook("3 taps")["nbr"]
    assert int((S.inverse_rulebook(nbr, 0, 10) >= 0).sum()) == 0
    assert torch.equal(S.inverse_rulebook(nbr, nbr.shape[0] + 7, 400), S.inverse_rulebook(nbr, nbr.shape[0], 400))
    assert int((S.inverse_rulebook(nbr, 1, 400) >= 0).sum()) == int((nbr[0] >= 0).sum())


def test_dense_layout_is_spconv_dense_view_and_the_pair_is_adjoint():
    B, D, H, W, C, live = 2, 2, 5, 7, 3, 23
    g = torch.Generator().manual_seed(0)
    cells = torch.randperm(B * D * H * W, generator=g)[:live + 4]
    coords = torch.stack([cells // (D * H * W), cells // (H * W) % D, cells // W % H, cells % W], 1).to(torch.int32)
    x = torch.randn(live + 4, C, generator=g, dtype=torch.float64)
    vol = torch.zeros(B, C, D, H, W, dtype=torch.float64)               # SparseConvTensor.dense(): (B, C, D, H, W)
    for r in range(live):
        b, z, y, xx = coords[r].tolist()
        vol[b, :, z, y, xx] = x[r]
    want = vol.view(B, C * D, H, W).permute(0, 2, 3, 1)                  # .view(N, C * D, H, W), channel-last
    assert torch.equal(S.sp_to_dense(x, coords, live, (D, H, W), B), want)
    gd = torch.randn(B, H, W, C * D, generator=g, dtype=torch.float64)
    back = vjp(lambda t: S.sp_to_dense(t, coords, live, (D, H, W), B), [x], gd)[0]
    assert torch.equal(back[:live], S.sp_from_dense(gd, coords, live, (D, H, W))) and float(back[live:].abs().max()) == 0.0
    xi = torch.randint(-8, 9, (live, C), generator=g).double()
    gi = torch.randint(-8, 9, (B, H, W, C * D), generator=g).double()
    assert float((S.sp_to_dense(xi, coords, live, (D, H, W), B) * gi).sum()) == float((xi * S.sp_from_dense(gi, coords, live, (D, H, W))).sum())


def test_float64_losses_match_the_oracle():
    """Same inputs through oracle/train_ref.py (float32) and the float64 restatements: value and autograd gradient within 2e-6 of
    the value / of max|gradient| (the float32 oracle's own rounding)."""
    from oracle import train_ref as T
    g = torch.Generator().manual_seed(1)
    B, N, H, W, C = 1, 2, 16, 24, 12
    logits = torch.randn(B * N, H // 2, W // 2, C, generator=g) * 2
    labels = torch.randint(0, C, (B, N, H, W), generator=g).float()
    labels[torch.rand(B, N, H, W, generator=g) < 0.1] = 255.0
    a = logits.clone().requires_grad_(True)
    la = T.seg_loss(a.permute(0, 3, 1, 2), labels, 2)
    la.backward()
    b = logits.double().requires_grad_(True)
    lb, u, cnt = S.seg_focal(b, labels, 2)
    lb.backward()
    assert abs(float(la.detach()) - float(lb.detach())) < 2e-6 * abs(float(lb.detach())) and cnt == int((labels[..., ::2, ::2] != 255).sum())
    assert float((a.grad.double() - b.grad).abs().max()) < 2e-6 * float(b.grad.abs().max())
    assert float(b.grad[labels.view(B * N, H, W)[:, ::2, ::2] == 255].abs().max()) == 0.0

    d_bound, f = [1.0, 41.0, 0.5], 4
    D = 80
    gt = torch.rand(B, N, H, W, generator=g) * 45.0
    gt[torch.rand(B, N, H, W, generator=g) < 0.9] = 0.0
    gt[0, 0, :8, :8] = 0.0
    gt[0, 0, 0, 0], gt[0, 0, 0, 4], gt[0, 0, 4, 0], gt[0, 1, 0, 0], gt[0, 1, 0, 5] = 0.5, 1.0, 40.5, 41.0, -3.0
    dl = torch.randn(B * N, H // f, W // f, D, generator=g)
    a = dl.clone().requires_grad_(True)
    la = T.depth_loss(a.permute(0, 3, 1, 2), gt, d_bound, f)
    la.backward()
    b = dl.double().requires_grad_(True)
    lb, div, bins = S.depth_bce(b, gt, d_bound, f)
    lb.backward()
    assert abs(float(la.detach()) - float(lb.detach())) < 2e-6 * abs(float(lb.detach())) and div == int((bins >= 1).sum()) > 3
    assert float((a.grad.double() - b.grad).abs().max()) < 2e-6 * float(b.grad.abs().max())
    assert bins[0, 0, 1].item() == 1 and bins[0, 1, 0].item() == 80          # 1.0 -> bin 0, 40.5 -> bin 79 (stored + 1)
    # a map without foreground: divisor 1, zero loss, zero gradient
    z = dl.double().requires_grad_(True)
    lz, div, _ = S.depth_bce(z, torch.zeros(B, N, H, W), d_bound, f)
    lz.backward()
    assert div == 1 and float(lz.detach()) == 0.0 and float(z.grad.abs().max()) == 0.0
    assert float(T.depth_loss(dl.permute(0, 3, 1, 2), torch.zeros(B, N, H, W), d_bound, f)) == 0.0


def test_the_kernel_table_is_what_the_chooser_plans():
    """tests/test_sparse_bwd.py::KERNELS against tt_conv2d_plan on the descriptor ops.gather_conv_dgrad builds (host only, as
    tests/test_conv_choice.py::_plan does); every sparse kernel family the backward runs on appears in it."""
    import test_sparse_bwd as B
    from thinktwice_amd import ops
    B.test_the_kernel_table_covers_every_family()
    got = {name: (ops.plan_label(B.dgrad_desc(name, False)), ops.plan_label(B.dgrad_desc(name, True))) for name in S.DGRAD_CASES}
    assert got == B.KERNELS, got
    z = S.dgrad_sizes("subm 32->32 small")
    assert z["in_alloc"] < 2048 <= S.dgrad_sizes("subm 32->32")["live_in"]
    assert S.dgrad_sizes("subm 16->16")["in_alloc"] == S.min_l2_rows() + 37
