"""Op-level parity of the optimizer kernels (csrc/optim.hip) through the C ABI: the global gradient norm with its clip factor,
and AdamW by both entry points -- tt_adamw_step_dev (the step count on the device) and tt_adamw_step (its host-count twin) --
against the float64 references of tests/step_ref.py within bounds counted from the kernels' roundings.  Sizes: one partial
block, under and over the 1024 blocks of the norm, and 2,097,152 + 257 elements, past 8192 * 256 where the update kernels
take a second grid-stride trip.  The skip-on-NaN bookkeeping is covered by test_train_step.py and test_accumulate.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_ref as S  # noqa: E402
from glue_ref import SENT, check, check_equal  # noqa: E402
from test_glue_ops import L, ok, st  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = 2_097_152 + 257


class Guarded:
    """[8 sentinels | n values | 8 sentinels] on the device; ptr() is the first value (32 bytes in: still 16-byte aligned)."""

    def __init__(self, t):
        self.n = t.numel()
        pad = torch.full((8,), SENT, dtype=t.dtype)
        self.buf = torch.cat([pad, t.reshape(-1), pad]).cuda()

    def ptr(self, off=0):
        return self.buf.data_ptr() + (8 + off) * self.buf.element_size()

    def get(self):
        return self.buf[8:8 + self.n].cpu()

    def set(self, t):
        self.buf[8:8 + self.n].copy_(t)

    def untouched(self, what):
        h = self.buf.cpu()
        assert bool((h[:8] == SENT).all()) and bool((h[-8:] == SENT).all()), f"{what}: wrote outside its buffer"


# ----------------------------------------------------------------------------- gradient norm and clip factor
@pytest.mark.parametrize("n", [1, 255, 257, 262144 + 1, BIG])
def test_grad_norm_and_clip_factor(n):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.37
    if n == 1:
        g[0] = 0.37
    gd = Guarded(g)
    ws = Guarded(torch.full((1024,), float("nan")))
    ref, bound = S.grad_norm_ref(g), S.grad_norm_bound(g)

    def run(max_norm):
        out = Guarded(torch.full((2,), SENT))
        ok(L().tt_grad_norm_clip(gd.ptr(), n, max_norm, ws.ptr(), out.ptr(), st()), "tt_grad_norm_clip")
        out.untouched("out_norm_scale"), ws.untouched("workspace"), gd.untouched("grad")
        return out.get()

    first = run(100.0)
    norm = np.float32(first[0].item())
    up, down = float(np.nextafter(norm, np.float32(np.inf))), float(np.nextafter(norm, np.float32(0)))
    # the norm below max_norm, at it, one ulp to either side of it, and above it
    for what, max_norm in (("far below", 2.0 * float(norm)), ("one ulp below", up), ("at", float(norm)), ("one ulp above", down),
                           ("far above", 0.5 * float(norm))):
        got = run(max_norm)
        assert torch.equal(got[:1], first[:1]), "the norm of the same gradient differs between two runs"
        case = f"n={n} norm {what} max_norm"
        check("grad_norm", case, got[:1], torch.tensor([ref], dtype=torch.float64), bound=torch.tensor([bound], dtype=torch.float64))
        want = S.clip_factor_ref(norm, max_norm)
        check_equal("grad_norm clip factor", case, got[1:], torch.tensor([float(want)]))
    assert float(S.clip_factor_ref(norm, 2.0 * float(norm))) == 1.0 and float(S.clip_factor_ref(norm, 0.5 * float(norm))) < 0.6


# ----------------------------------------------------------------------------- AdamW
STARTS, LRS, WDS, SCALES = (0, 9, 100000), (0.0, 1e-4), (0.0, 1e-7, 0.1), (None, 0.25)
ALL_COMBOS = [(s, lr, wd, gs) for s in STARTS for lr in LRS for wd in WDS for gs in SCALES]
# at the large size one combination per test, each value of every parameter taken once
BIG_COMBOS = [(0, 1e-4, 1e-7, None), (9, 1e-4, 0.1, 0.25), (100000, 0.0, 0.0, 0.25)]
ADAMW_CASES = ([(e, n, None) for e in ("dev", "host") for n in (1, 255)]
               + [(e, BIG, i) for e in ("dev", "host") for i in range(len(BIG_COMBOS))])
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def adamw_state(n, gen):
    """p, m, v with both moments nonzero, and every seventh v exactly zero (the gradients are zero there too: denom = eps)."""
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 0.01 + 1e-6
    v[::7] = 0.0
    return p, m, v


@pytest.mark.parametrize("entry,n,combo", ADAMW_CASES, ids=[f"{e}-n{n}" + ("" if i is None else f"-combo{i}") for e, n, i in ADAMW_CASES])
def test_adamw_three_steps_against_float64(entry, n, combo):
    lib = L()
    for start, lr, wd, gs in (ALL_COMBOS if combo is None else [BIG_COMBOS[combo]]):
        gen = torch.Generator().manual_seed(n % 1000 + start % 100 + int(wd * 1e8))
        p, m, v = adamw_state(n, gen)
        P, M, V, Gd = Guarded(p), Guarded(m), Guarded(v), Guarded(torch.zeros(n))
        steps_dev = torch.tensor([start], dtype=torch.int32).cuda()
        gs_dev = None if gs is None else torch.tensor([gs]).cuda()
        gsp = None if gs_dev is None else gs_dev.data_ptr()
        for k in range(3):
            g = torch.randn(n, generator=gen) * (4.0 if gs else 1.0)
            g[::7] = 0.0
            Gd.set(g.cuda())
            step = start + k + 1
            if entry == "dev":
                ok(lib.tt_adamw_step_dev(P.ptr(), Gd.ptr(), M.ptr(), V.ptr(), n, lr, BETA1, BETA2, EPS, wd, steps_dev.data_ptr(), gsp,
                                         st()), "tt_adamw_step_dev")
                ok(lib.tt_adamw_advance(steps_dev.data_ptr(), gsp, st()), "tt_adamw_advance")
                assert int(steps_dev.item()) == step
            else:
                ok(lib.tt_adamw_step(P.ptr(), Gd.ptr(), M.ptr(), V.ptr(), n, lr, BETA1, BETA2, EPS, wd, step, gsp, st()), "tt_adamw_step")
            # one step from the values the device started it with: the errors of the steps do not pile up
            rp, rm, rv = S.adamw_ref(p, g, m, v, step, lr, BETA1, BETA2, EPS, wd, gs)
            bp, bm, bv = S.adamw_bounds(p, g, m, v, step, lr, BETA1, BETA2, EPS, wd, gs)
            p, m, v = P.get(), M.get(), V.get()
            case = f"n={n} step {step} lr={lr} wd={wd} grad_scale={gs}"
            kern = "adamw_dev_step" if entry == "dev" else "adamw (host step)"
            check(kern + " p", case, p, rp, bound=bp)
            check(kern + " m", case, m, rm, bound=bm)
            check(kern + " v", case, v, rv, bound=bv)
            assert bool((v[::7] == 0).all())
            if lr == 0.0:
                assert torch.equal(p, rp.float()), "lr = 0 must leave the parameters alone"
        for t, what in ((P, "param"), (M, "exp_avg"), (V, "exp_avg_sq"), (Gd, "grad")):
            t.untouched(what)
        assert torch.equal(Gd.get(), g)


def test_flat_adamw_live_ranges_touch_nothing_else():
    """Ranges whose offsets are no multiple of 4 floats: inside them one AdamW step with the clip factor of the whole buffer,
    outside them p, m and v bit-unchanged; the step count advances once, not once per range."""
    from thinktwice_amd.optim import FlatAdamW
    n, ranges = 6000, [(3, 5), (17, 1), (1001, 4099)]
    gen = torch.Generator().manual_seed(6000)
    p, m, v = adamw_state(n, gen)
    g = torch.randn(n, generator=gen) * 3.0                                          # norm ~ 230: clipped at 100
    pd, gd = p.cuda(), g.cuda()
    opt = FlatAdamW(pd, gd, lr=1e-4, weight_decay=0.1, max_grad_norm=100.0)
    opt.m.copy_(m), opt.v.copy_(v)
    opt.steps = 9
    ns = opt.step(live_ranges=ranges).cpu()
    assert opt.steps == 10
    gs = float(ns[1])
    assert 0.3 < gs < 0.6 and np.float32(gs) == S.clip_factor_ref(np.float32(ns[0].item()), 100.0)
    inside = torch.zeros(n, dtype=torch.bool)
    for off, cnt in ranges:
        inside[off:off + cnt] = True
    rp, rm, rv = S.adamw_ref(p, g, m, v, 10, 1e-4, BETA1, BETA2, EPS, 0.1, gs)
    bp, bm, bv = S.adamw_bounds(p, g, m, v, 10, 1e-4, BETA1, BETA2, EPS, 0.1, gs)
    for what, got, before, ref, bound in (("p", pd.cpu(), p, rp, bp), ("m", opt.m.cpu(), m, rm, bm), ("v", opt.v.cpu(), v, rv, bv)):
        check("adamw_dev_step " + what, "FlatAdamW live ranges", got[inside], ref[inside], bound=bound[inside])
        assert torch.equal(got[~inside], before[~inside]), f"{what} changed outside the live ranges"
        assert not torch.equal(got[inside], before[inside])
