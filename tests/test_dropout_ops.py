"""Op-level parity of the dropout kernels (csrc/batchnorm.hip: dropout_fwd_kernel, dropout_bwd_kernel) through the C ABI.
The keep rule is a counter-based splitmix64 whose every step is exact, so the mask is predictable bit for bit
(step_ref.dropout_keep_ref) and the output is one correctly rounded f32 product: everything forward is compared as bits.
n = 2^20 + 300 lies past kNumCU * 16 * 256 = 1,048,576 elements, where the grid-stride loop takes a second trip."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_ref as S  # noqa: E402
from glue_ref import PREFILL_ULP, SENT, U32, check, check_equal, prefill  # noqa: E402
from test_glue_ops import L, ok, st  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 6144, 2 ** 20 + 300]
MASK_SENT = 0xAB


@functools.lru_cache(maxsize=None)
def keep_ref(seed, n, p):
    return torch.from_numpy(S.dropout_keep_ref(seed, n, p))


def guarded(t):
    """t followed by 8 sentinels, on the device."""
    sent = MASK_SENT if t.dtype == torch.uint8 else SENT
    return torch.cat([t.reshape(-1), torch.full((8,), sent, dtype=t.dtype)]).cuda()


def guard_ok(buf, n, what):
    sent = MASK_SENT if buf.dtype == torch.uint8 else SENT
    assert bool((buf[n:].cpu() == sent).all()), f"{what}: wrote past its end"


def bits(t):
    return t.contiguous().view(torch.int32)


def expected_out(x, keep, p):
    """x * (float) (1 / (1 - p)) where kept -- one f32 product --, +0.0 elsewhere."""
    return torch.where(keep.bool(), x * torch.tensor(float(S.dropout_inv_keep(p))), torch.zeros_like(x))


@pytest.mark.parametrize("n", SIZES)
def test_dropout_fwd_mask_and_output_are_bit_equal_to_the_restated_rule(n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    x[0] = -0.0 if n > 1 else x[0]
    xd = guarded(x)
    for seed in S.DROPOUT_SEEDS:
        for p in S.DROPOUT_PS:
            keep = keep_ref(seed, n, p)
            out, mask = guarded(torch.full((n,), SENT)), guarded(torch.full((n,), MASK_SENT, dtype=torch.uint8))
            ok(L().tt_dropout_fwd(xd.data_ptr(), out.data_ptr(), n, p, seed, None, mask.data_ptr(), st()), "tt_dropout_fwd")
            case = f"n={n} seed={seed:#x} p={p}"
            check_equal("dropout_fwd mask", case, mask[:n].cpu(), keep)
            check_equal("dropout_fwd out", case, bits(out[:n].cpu()), bits(expected_out(x, keep, p)))
            if p == 0:
                assert bool(keep.all()) and torch.equal(bits(out[:n].cpu()), bits(x)), "p = 0 must return x bit for bit"
            guard_ok(out, n, "out"), guard_ok(mask, n, "mask_out"), guard_ok(xd, n, "x")


def test_dropout_fwd_keeps_a_draw_equal_to_p():
    """The edge of the rule: seeds under which one element draws exactly (float) p (step_ref.dropout_seed_drawing).  It is
    kept -- the rule is >= --, also at p = 0 with a draw of 0; random masks meet such a draw once in 2^24 elements."""
    n = 255
    x = torch.rand(n, generator=torch.Generator().manual_seed(9)) + 1.0
    xd = guarded(x)
    for p, u24 in S.DROPOUT_EDGES:
        for index in (0, 5, 254):
            seed = S.dropout_seed_drawing(u24, index)
            keep = torch.from_numpy(S.dropout_keep_ref(seed, n, p))
            assert keep[index] == 1
            out, mask = guarded(torch.full((n,), SENT)), guarded(torch.full((n,), MASK_SENT, dtype=torch.uint8))
            ok(L().tt_dropout_fwd(xd.data_ptr(), out.data_ptr(), n, p, seed, None, mask.data_ptr(), st()), "tt_dropout_fwd")
            case = f"draw == p = {p} at element {index}"
            check_equal("dropout_fwd mask", case, mask[:n].cpu(), keep)
            check_equal("dropout_fwd out", case, bits(out[:n].cpu()), bits(expected_out(x, keep, p)))
            guard_ok(out, n, "out"), guard_ok(mask, n, "mask_out")


@pytest.mark.parametrize("n", [255, 2 ** 20 + 300])
def test_dropout_fwd_replays_a_given_mask(n):
    """mask_in overrides the generator (any non-zero byte keeps); mask_out then holds it as 0 / 1.  Without a mask_out the
    output is the same."""
    gen = torch.Generator().manual_seed(3 * n)
    x = torch.randn(n, generator=gen)
    given = torch.randint(0, 3, (n,), generator=gen).to(torch.uint8) * 127          # 0, 127, 254
    p, seed = 0.5, 0x5EED
    assert not torch.equal(given != 0, keep_ref(seed, n, p).bool())
    xd, gd = guarded(x), guarded(given)
    want = expected_out(x, given != 0, p)
    for with_mask_out in (True, False):
        out, mask = guarded(torch.full((n,), SENT)), guarded(torch.full((n,), MASK_SENT, dtype=torch.uint8))
        ok(L().tt_dropout_fwd(xd.data_ptr(), out.data_ptr(), n, p, seed, gd.data_ptr(), mask.data_ptr() if with_mask_out else None,
                              st()), "tt_dropout_fwd")
        case = f"n={n} replay mask_out={with_mask_out}"
        check_equal("dropout_fwd out", case, bits(out[:n].cpu()), bits(want))
        if with_mask_out:
            check_equal("dropout_fwd mask", case, mask[:n].cpu(), (given != 0).to(torch.uint8))
        else:
            assert bool((mask.cpu() == MASK_SENT).all())
        guard_ok(out, n, "out"), guard_ok(mask, n, "mask_out"), guard_ok(gd, n, "mask_in")
    assert torch.equal(gd[:n].cpu(), given)


@pytest.mark.parametrize("n", [1, 255, 2 ** 20 + 300])
def test_dropout_bwd_accumulates_into_dx(n):
    """dx += mask ? dout * (float) (1 / (1 - p)) : 0 -- one f32 product, then the sum into the prefill (its ulp: PREFILL_ULP);
    a dropped element adds +0.0 and keeps its prefill bit for bit."""
    gen = torch.Generator().manual_seed(5 * n)
    for p in (0.0, 0.5, 0.9):
        dout = torch.randn(n, generator=gen).clamp(-3.0, 3.0) * (1.0 - p)           # |dout / (1 - p)| <= 3: inside the prefill's ulp
        keep = keep_ref(0x5EED, n, p if p else 0.5)                                 # p = 0 with a mask that still drops
        P = prefill((n,), gen)
        dd, md, dx = guarded(dout), guarded(keep), guarded(P)
        ok(L().tt_dropout_bwd(dd.data_ptr(), md.data_ptr(), dx.data_ptr(), n, p, st()), "tt_dropout_bwd")
        got = dx[:n].cpu()
        ref = torch.where(keep.bool(), dout.double() * float(S.dropout_inv_keep(p)), torch.zeros(n, dtype=torch.float64))
        check("dropout_bwd", f"n={n} p={p}", got.double() - P.double(), ref, bound=U32 * ref.abs(), slack=PREFILL_ULP)
        drop = ~keep.bool()
        assert torch.equal(bits(got[drop]), bits(P[drop])), "a dropped element must keep its prefill"
        guard_ok(dx, n, "dx"), guard_ok(dd, n, "dout"), guard_ok(md, n, "mask")


def test_ops_dropout_draws_a_new_predictable_mask_per_call():
    from thinktwice_amd import ops
    saved_seed, saved_masks = list(ops.DROPOUT_SEED), ops.DROPOUT_MASKS
    n, p = 6144, 0.5
    x = torch.rand(n, generator=torch.Generator().manual_seed(1)) + 1.0              # no zero: out != 0 is the mask
    try:
        ops.DROPOUT_MASKS = None
        masks = []
        for _ in range(2):
            calls = ops.DROPOUT_SEED[1] + 1
            seed = (ops.DROPOUT_SEED[0] * 0x100000001B3 + calls * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
            out = ops.dropout(x.cuda(), p).cpu()
            assert ops.DROPOUT_SEED[1] == calls
            keep = torch.from_numpy(S.dropout_keep_ref(seed, n, p))
            check_equal("dropout_fwd out", f"ops.dropout call {calls}", bits(out), bits(expected_out(x, keep, p)))
            masks.append(keep)
        assert not torch.equal(masks[0], masks[1])
    finally:
        ops.DROPOUT_SEED[:] = saved_seed
        ops.DROPOUT_MASKS = saved_masks
