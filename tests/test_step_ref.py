"""The references of tests/step_ref.py against torch's float64 operators, on the CPU: what the GPU parity tests of BatchNorm,
dropout and the optimizer (test_bn_ops.py, test_dropout_ops.py, test_optim_ops.py) are held to is itself held to torch here."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_ref as S  # noqa: E402
from glue_ref import vjp  # noqa: E402

TOL = 1e-10          # float64 references of the same formula in another operation order


def close(got, want, what, tol=TOL):
    """|got - want| <= tol * max|want| per column (the columns of a case differ by up to 1e18 in magnitude)."""
    got, want = got.double().reshape(-1, got.shape[-1]), want.double().reshape(-1, want.shape[-1])
    scale = want.abs().amax(0, keepdim=True).clamp_min(1e-300)
    err = float(((got - want).abs() / scale).max()) if got.numel() else 0.0
    assert err <= tol, f"{what}: {err:.3e}"


@pytest.mark.parametrize("c", S.BN_CASES, ids=[c.id for c in S.BN_CASES])
def test_batchnorm_references_equal_torch_float64(c):
    d = S.bn_case_data(c)
    z = d["z"].double()
    C = c.C
    f = S.bn_forward_ref(z, d["gamma"], d["beta"], c.eps, c.momentum, d["rm"], d["rv"], c.groups, c.live, d["res"], c.act)
    rows = S.bn_row_groups(c.M, c.groups, c.live)
    good = torch.ones(C, dtype=torch.bool)
    if c.data == "bad":
        good[2] = good[5] = False
        # the guard of bn_finalize_kernel, which torch does not have: the two channels keep their running statistics
        assert torch.equal(f["running_mean"][~good], d["rm"].double()[~good])
        assert torch.equal(f["running_var"][~good], d["rv"].double()[~good])
    eps, mom = S.f32r(c.eps), S.f32r(c.momentum)
    ga = None if d["gamma"] is None else d["gamma"].double()
    be = None if d["beta"] is None else d["beta"].double()
    rm = None if d["rm"] is None else d["rm"].double().clone()
    rv = None if d["rv"] is None else d["rv"].double().clone()

    if any(b - a == 1 for a, b in rows):             # torch refuses one row: mean = z, var = 0, xhat = 0 by hand
        assert c.groups == 1 and rows[0] == (0, 1)
        assert torch.equal(f["mean"][0], z[0]) and float(f["var"].abs().max()) == 0.0
        want = f["shift"] + sum(r.double()[0] for r in d["res"])
        close(f["out"][:1], (torch.relu(want) if c.act else want).view(1, C), "out, one row")
        assert torch.equal(f["running_var"], (1.0 - mom) * rv + mom * 0.0)          # the biased value: 0
        b = S.bn_backward_ref(d["dy"], f["out"], z, f, c.act)
        assert float(b["dz"][:1].abs().max()) == 0.0
        return
    if all(b == a for a, b in rows):                 # no live row: nothing changes
        assert torch.equal(f["running_mean"], rm) and torch.equal(f["running_var"], rv)
        assert bool(torch.isfinite(f["scale"]).all()) and float(f["mean"].abs().max()) == 0.0
        return

    def fwd(zz, gamma, beta, *res, rmb=None, rvb=None):
        outs = []
        for a, b in rows:
            v = F.batch_norm(zz[a:b], rmb, rvb, gamma, beta, True, mom, eps)
            for r in res:
                v = v + r[a:b]
            outs.append(torch.relu(v) if c.act else v)
        return torch.cat(outs)

    want = fwd(z, ga, be, *[r.double() for r in d["res"]], rmb=rm, rvb=rv)
    n_live = rows[-1][1]
    close(f["out"][:n_live][:, good], want[:, good], "out")
    assert bool(torch.isnan(f["out"][n_live:]).all())
    for i, (a, b) in enumerate(rows):
        close(f["mean"][i:i + 1, good], z[a:b].mean(0, keepdim=True)[:, good], "mean")
        close(f["var"][i:i + 1, good], z[a:b].var(0, unbiased=False, keepdim=True)[:, good], "var")
    if rm is not None:
        close(f["running_mean"][good].view(1, -1), rm[good].view(1, -1), "running_mean")
        close(f["running_var"][good].view(1, -1), rv[good].view(1, -1), "running_var")

    # backward: torch autograd through the same float64 graph
    dy = d["dy"].double()[:n_live]
    leaves = [z[:n_live], ga if ga is not None else torch.ones(C, dtype=torch.float64),
              be if be is not None else torch.zeros(C, dtype=torch.float64)] + [r.double()[:n_live] for r in d["res"]]
    grads = vjp(lambda *t: fwd(*t), leaves, dy)
    b = S.bn_backward_ref(d["dy"], f["out"], z, f, c.act)
    close(b["dz"][:n_live][:, good], grads[0][:, good], "dz")
    close(b["sgx"].sum(0, keepdim=True)[:, good], grads[1].view(1, C)[:, good], "dgamma")
    close(b["sg"].sum(0, keepdim=True)[:, good], grads[2].view(1, C)[:, good], "dbeta")
    for gr in grads[3:]:
        close(b["dres"][:n_live][:, good], gr[:, good], "dres")
    assert torch.equal(b["g"][n_live:], d["dy"].double()[n_live:])

    # the bound helpers: finite, positive, of the output's shape
    fb = S.bn_forward_bounds(z, f, d["res"])
    bb = S.bn_backward_bounds(z, f, fb, b)
    for name, t, shape in (("mean", fb["mean"], (c.groups, C)), ("invstd", fb["invstd"], (c.groups, C)),
                           ("scale", fb["scale"], (c.groups, C)), ("out", fb["out"][:n_live], (n_live, C)),
                           ("dz", bb["dz"][:n_live], (n_live, C)), ("sg", bb["sg"], (c.groups, C)), ("sgx", bb["sgx"], (c.groups, C))):
        assert tuple(t.shape) == shape, name
        assert bool((torch.isfinite(t[..., good]) & (t[..., good] > 0)).all()), name
    if rm is not None:
        for name in ("running_mean", "running_var"):
            assert fb[name].shape == (C,) and bool((torch.isfinite(fb[name][good]) & (fb[name][good] > 0)).all()), name


def test_constant_column_has_zero_variance_and_returns_beta():
    c = next(c for c in S.BN_CASES if c.id == "constant-column")
    d = S.bn_case_data(c)
    f = S.bn_forward_ref(d["z"], d["gamma"], d["beta"], c.eps, c.momentum, d["rm"], d["rv"])
    assert float(f["var"][0, 0]) == 0.0 and float(f["invstd"][0, 0]) == 1.0 / np.sqrt(S.f32r(c.eps))
    assert torch.equal(f["out"][:, 0], d["beta"].double()[0].expand(c.M))


def test_conditioned_column_one_pass_variance_is_inside_its_bound():
    """The kernel's one-pass E[z^2] - mean^2 in f64, restated: its distance from the two-pass value against the bound's term."""
    c = next(c for c in S.BN_CASES if c.id == "cond-mean100-dev0.01")
    z = S.bn_case_data(c)["z"].double()[:, 0]
    n = z.numel()
    one = float((z * z).sum() / n - (z.sum() / n) ** 2)
    two = float(((z - z.mean()) ** 2).mean())
    rel = abs(one - two) / two
    print(f"one-pass variance off the two-pass value by {rel:.3e} relative")
    assert abs(one - two) <= (3 * n + 6) * S.U64 * float((z * z).mean())


@pytest.mark.parametrize("start", [0, 9, 100000])
def test_adamw_ref_equals_torch_adamw_in_float64(start):
    gen = torch.Generator().manual_seed(5 + start)
    n = 1000
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([par], **hp)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    if start:                                        # moments of an optimizer that has run `start` steps
        m, v = torch.randn(n, generator=gen, dtype=torch.float64) * 0.1, torch.rand(n, generator=gen, dtype=torch.float64) * 0.01
        par.grad = torch.zeros_like(par)
        opt.step()
        st = opt.state[par]
        st["exp_avg"].copy_(m), st["exp_avg_sq"].copy_(v)
        st["step"].fill_(float(start)) if torch.is_tensor(st["step"]) else st.__setitem__("step", start)
        par.data.copy_(p0)
    for k in range(3):
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        par.grad = g.clone()
        opt.step()
        p, m, v = S.adamw_ref(p, g, m, v, start + k + 1, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], round_hyper=False)
        st = opt.state[par]
        for got, want, what in ((p, par.detach(), "p"), (m, st["exp_avg"], "m"), (v, st["exp_avg_sq"], "v")):
            rel = float((got - want).abs().max() / want.abs().max())
            assert rel <= 1e-12, (what, k, rel)
    bp, bm, bv = S.adamw_bounds(p, g, m, v, start + 4, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], 0.25)
    for t in (bp, bm, bv):
        assert t.shape == (n,) and bool((torch.isfinite(t) & (t > 0)).all())


def test_grad_norm_reference_and_bound():
    g = torch.randn(1000, generator=torch.Generator().manual_seed(2))
    assert abs(S.grad_norm_ref(g) - float(torch.linalg.vector_norm(g.double()))) <= 1e-12 * S.grad_norm_ref(g)
    b = S.grad_norm_bound(g)
    assert np.isfinite(b) and 0 < b < 1e-4
    assert S.clip_factor_ref(np.float32(50.0), 100.0) == np.float32(1.0)
    assert S.clip_factor_ref(np.float32(200.0), 100.0) == np.float32(100.0) / (np.float32(200.0) + np.float32(1e-6))


N_DROP = 2 ** 20 + 300


@pytest.mark.parametrize("seed", S.DROPOUT_SEEDS, ids=[hex(s) for s in S.DROPOUT_SEEDS])
def test_dropout_keep_rule_keeps_its_share(seed):
    for p in S.DROPOUT_PS:
        keep = S.dropout_keep_ref(seed, N_DROP, p)
        assert keep.dtype == np.uint8 and keep.shape == (N_DROP,)
        share = float(keep.mean())
        sigma = np.sqrt(p * (1 - p) / N_DROP)
        print(f"seed {seed:#x} p {p}: kept {share:.6f}, {abs(share - (1 - p)) / sigma if sigma else 0.0:.2f} sigma off")
        assert abs(share - (1 - p)) <= 5 * sigma
        if p == 0:
            assert bool(keep.all())


def test_dropout_keep_rule_seeds_are_independent():
    p = 0.5
    masks = [S.dropout_keep_ref(s, N_DROP, p) for s in S.DROPOUT_SEEDS]
    sigma = np.sqrt(0.25 / N_DROP)
    for i in range(len(masks)):
        for j in range(i + 1, len(masks)):
            agree = float((masks[i] == masks[j]).mean())
            assert abs(agree - 0.5) <= 5 * sigma, (i, j, agree)


def test_dropout_inverse_keep_probability_is_f32():
    assert S.dropout_inv_keep(0.0) == np.float32(1.0) and S.dropout_inv_keep(0.5) == np.float32(2.0)
    assert S.dropout_inv_keep(0.9).dtype == np.float32


def test_dropout_edge_seeds_draw_exactly_p():
    """dropout_seed_drawing: the chosen element draws exactly (float) p -- kept, by >= --, and is dropped one ulp above."""
    for p, u24 in S.DROPOUT_EDGES:
        assert np.float32(u24) * np.float32(2.0 ** -24) == np.float32(p)
        for index in (0, 5, 254):
            seed = S.dropout_seed_drawing(u24, index)
            assert S.dropout_keep_ref(seed, 255, p)[index] == 1
            above = float(np.nextafter(np.float32(p), np.float32(1)))
            assert S.dropout_keep_ref(seed, 255, above)[index] == 0
            if p > 0:
                assert S.dropout_keep_ref(seed, 255, float(np.nextafter(np.float32(p), np.float32(0))))[index] == 1


def test_bn_sum_depth_counts_the_launch_geometry():
    # 131329 rows, C = 3, scalar: 512 workgroups of 257 rows, TY = 85 row lanes: 4 + 85 + 64 + 10
    assert S.bn_launch_blocks(131072 + 257) == 512 and S.bn_sum_depth(131072 + 257, 3) == 4 + 85 + 64 + 10
    # the 16-byte kernel at C = 4: one channel lane, 256 row lanes
    assert S.bn_sum_depth(131072 + 257, 4, vec=True) == 2 + 256 + 64 + 10
    assert S.bn_launch_blocks(6145) == 25 and S.bn_launch_blocks(3 * 6145, 3) == 25 and S.bn_launch_blocks(70) == 1
    # never more than the rows there are: a device row count of 37 in 5000 allocated rows, one row, none
    assert S.bn_sum_depth(5000, 6, live=37) == 37 and S.bn_sum_depth(1, 4, vec=True) == 1 and S.bn_sum_depth(5000, 6, live=0) == 1
