"""CPU checks of tests/glue_ref.py: the float64 restatements against the formulations the suite already trusts, the
summation bound on a hand-computed example, and the tie / nearest rules of this torch that the GPU tests rely on."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import glue_ref as G  # noqa: E402


def test_lift_splat_restatement_matches_voxel_pool_of_the_materialised_volume():
    """The formulation of test_voxel_pool.py (softmax (x) context -> c_ref.voxel_pool_fwd), here on f32-valued inputs."""
    from oracle import c_ref
    B, N, D, H, W, C = 2, 2, 9, 3, 4, 8
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(B * N, H, W, D, generator=g) * 2
    ctx = torch.randn(B * N, H, W, C, generator=g)
    Np = N * D * H * W
    geom = torch.stack([torch.randint(-2, 9, (B, Np), generator=g), torch.randint(-2, 7, (B, Np), generator=g),
                        torch.randint(-1, 2, (B, Np), generator=g)], -1).to(torch.int32)
    got = G.lift_splat_ref(logits.double(), ctx.double(), geom, (7, 5, 1), B, N)
    vol = logits.permute(0, 3, 1, 2).softmax(1).unsqueeze(1) * ctx.permute(0, 3, 1, 2).unsqueeze(2)      # [BN,C,D,H,W]
    vol = vol.reshape(B, N, C, D, H, W).permute(0, 1, 3, 4, 5, 2).contiguous()
    ref, _ = c_ref.voxel_pool_fwd(geom.numpy(), vol.reshape(B, -1, C).numpy(), (7, 5, 1))
    assert got.shape == (B, 5, 7, C)
    assert float(np.abs(got.numpy() - ref).max()) < 2e-6 * float(np.abs(ref).max())     # f32 softmax / product / output of the oracle
    kept = ((geom >= 0) & (geom < torch.tensor([7, 5, 1]))).all(-1)
    assert 0 < int(kept.sum()) < kept.numel()                                           # both kept and dropped points


def test_sum_bound_on_a_hand_computed_example():
    # 3 addends 1, 2^-24, 2^-24 summed left to right in f32 lose both small terms: error 2^-23 <= (3 + 0) * 2^-24 * (1 + 2^-23)
    assert G.sum_bound(10.0, 6, 2) == 8 * 2.0 ** -24 * 10.0
    v = torch.tensor([1.0, 2.0 ** -24, 2.0 ** -24])
    s = torch.tensor(0.0)
    for t in v:
        s = s + t
    err = abs(float(s.double() - v.double().sum()))
    assert err == 2.0 ** -23 and err <= G.sum_bound(float(v.double().abs().sum()), 3, 0)
    b = G.sum_bound(torch.tensor([1.0, 2.0], dtype=torch.float64), 4, 1)
    assert torch.equal(b, torch.tensor([5 * 2.0 ** -24, 10 * 2.0 ** -24], dtype=torch.float64))


def test_f32_limit_never_falls_below_eight_roundings():
    r = torch.tensor([1.0, -2.0], dtype=torch.float64)
    assert G.f32_limit(r.float(), r) == 8 * G.U32
    assert G.f32_limit((r * (1 + 1e-5)).float(), r) > 3.9e-5


def test_float64_max_pool_backward_routes_to_the_first_maximum():
    g = torch.Generator().manual_seed(0)
    vals = torch.tensor([0.0, 0.0, 0.0, 1.0, 2.0], dtype=torch.float64)
    for shape in [(1, 5, 6, 2), (2, 7, 4, 1), (1, 1, 1, 1), (1, 2, 3, 2)]:
        x = vals[torch.randint(0, 5, shape, generator=g)]
        if shape[1] > 2:
            x[0, :2, :2] = float("-inf")                                   # a window of -inf only: still its first element
        N, H, W, C = shape
        dy = torch.randint(-3, 4, (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), generator=g).double()
        xt = x.clone().requires_grad_(True)
        F.max_pool2d(xt.permute(0, 3, 1, 2), 3, 2, 1).backward(dy.permute(0, 3, 1, 2))
        assert torch.equal(xt.grad, G.maxpool3x3s2_bwd_first_max(x, dy))


def test_amax_backward_splits_evenly_among_ties():
    x = torch.tensor([[0.0, 0.0, 0.0, 0.0], [1.0, 3.0, 3.0, 2.0], [5.0, 1.0, 2.0, 3.0]], dtype=torch.float64, requires_grad=True)
    x.amax(1).backward(torch.tensor([4.0, 6.0, 7.0], dtype=torch.float64))
    assert torch.equal(x.grad, torch.tensor([[1.0, 1, 1, 1], [0, 3, 3, 0], [7, 0, 0, 0]], dtype=torch.float64))


def test_integer_nearest_rule_is_torchs_nearest():
    for H in range(1, 40):
        for h in range(1, H + 1):
            src = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1)
            want = F.interpolate(src, size=(H, 1), mode="nearest").view(H).long()
            assert torch.equal(G.nearest_index(H, h), want), (H, h)
    src = torch.randn(2, 2, 3, 4, dtype=torch.float64)
    want = F.interpolate(src.permute(0, 3, 1, 2), size=(5, 7), mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(G.nearest_up(src, 5, 7), want)


def test_deformable_column_restatement_matches_the_oracle():
    from oracle import model_ref
    g = torch.Generator().manual_seed(1)
    for N, H, W, C, cs in [(1, 2, 2, 4, 18), (2, 5, 7, 8, 27)]:
        x = torch.randn(N, H, W, C, generator=g)
        off = torch.randn(N, H, W, cs, generator=g) * 3
        off[0, 0, 0, 0], off[0, 0, 0, 16] = -0.5 + 1.0, 0.5 - 1.0 + (H - 1)       # tap 0: py = -0.5; tap 8: py = H - 0.5
        got = G.deform_cols(x, off)
        ref = model_ref.deform_im2col(x.double().permute(0, 3, 1, 2), off[..., :18].double().permute(0, 3, 1, 2))   # (B,C,9,H,W)
        ref = ref.permute(0, 3, 4, 2, 1).reshape(N * H * W, 9, C)
        assert float((got - ref).abs().max()) < 1e-12 * float(ref.abs().max())
        s = G.deform_sample(x, off)
        assert float(s["py"][0, 0, 0, 0]) == -0.5 and float(s["py"][0, 0, 0, 8]) == H - 0.5
    z = torch.zeros(1, 3, 4, 18)
    x = torch.randn(1, 3, 4, 4, generator=g)
    assert torch.equal(G.deform_cols(x, z), G.im2col3x3_zero_pad(x.double()))


def test_softplus_derivative_from_the_saved_output_needs_expm1():
    """What tt_ew_bwd's softplus branches compute from the saved f32 output o = softplus(pre): sigmoid(pre) = 1 - exp(-o).
    In f32 the literal form cancels for negative pre-activations (the defect of the parent commit); -expm1f(-o) does not."""
    pre = torch.tensor([-30.0, -20.0, -17.0, -15.0, -10.0, -5.0, 0.0, 5.0, 19.9, 20.1, 25.0])
    o = F.softplus(pre)
    want = -torch.expm1(-o.double())
    old = (1.0 - torch.exp(-o)).double()
    new = (-torch.expm1(-o)).double()
    rel_old = ((old - want).abs() / want).tolist()
    assert rel_old[0] == 1.0 and rel_old[1] == 1.0 and rel_old[2] > 0.2 and rel_old[3] > 1e-2 and rel_old[4] > 1e-4
    assert float(((new - want).abs() / want).max()) <= 8 * 2.0 ** -23
