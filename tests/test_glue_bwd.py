"""Op-level parity of the backward glue kernels (csrc/glue_bwd.hip) against torch autograd through the float64 forward.

Every gradient destination is pre-filled with a non-zero pattern (the kernels document `+=`) inside a buffer with sentinel
guard rows and, where the entry point takes a stride, guard columns; `got - prefill` is compared with the reference at the
value tolerance plus one ulp of the prefill (tests/glue_ref.py: prefill magnitudes 8..16, cotangents scaled so that every
gradient stays below 4).  Two runs must be bit-identical, except the atomically accumulated `gx` of the deformable columns."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import glue_ref as G  # noqa: E402
from glue_ref import PREFILL_ULP, Win, check, check_equal, vjp  # noqa: E402
from test_glue_ops import HW_IDS, L, LN_CASES, CAT_R, cat_rows_of, deform_offsets, ew_ref, nchw, ok, st, tie_data, twice, up2  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(t):
    return t.contiguous().cuda()


def delta(win):
    """What a kernel added to a prefilled window, in float64."""
    return win.get().double() - win.init().double()


# ----------------------------------------------------------------------------- max-pool backward
MPB = [((2, 7, 10, 8), "vector-path-7x10-overhang", 0), ((1, 1, 1, 4), "vector-path-1x1", 0), ((1, 2, 3, 4), "vector-path-2x3", 0),
       ((1, 5, 5, 12), "vector-path-5x5-C12", 0), ((2, 7, 10, 6), "scalar-path-C6", 0), ((2, 7, 10, 8), "scalar-path-misaligned", 1)]


@pytest.mark.parametrize("shape,cid,shift", MPB, ids=[c for _, c, _ in MPB])
def test_maxpool3x3s2_bwd_routes_to_the_first_maximum_bit_equal(shape, cid, shift):
    """Integer-valued dy and prefill: the sums are exact, so the result is bit-equal to torch's float64 backward.  `shift` = 1
    places x, dy and dx one float past a 16-byte boundary (the vector kernel needs all three aligned)."""
    g = torch.Generator().manual_seed(sum(shape) + shift)
    N, H, W, C = shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = tie_data(shape, g)
    dy = torch.randint(-3, 4, (N, OH, OW, C), generator=g).float()
    P = torch.randint(1, 6, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    ref = vjp(lambda t: F.max_pool2d(nchw(t), 3, 2, 1), [x], nchw(dy))[0]
    assert torch.equal(ref, G.maxpool3x3s2_bwd_first_max(x.double(), dy.double()))

    def place(t):                          # flat device buffer [sentinel * shift | t | 8 sentinels]
        flat = torch.full((t.numel() + shift + 8,), G.SENT)
        flat[shift:shift + t.numel()] = t.reshape(-1)
        return flat.cuda(), flat

    xd, _ = place(x)
    dyd, _ = place(dy)

    def run():
        dxd, host0 = place(P)
        for t in (xd, dyd, dxd):
            assert (t.data_ptr() + 4 * shift) % 16 == 4 * shift
        ok(L().tt_maxpool3x3s2_bwd(xd.data_ptr() + 4 * shift, dyd.data_ptr() + 4 * shift, dxd.data_ptr() + 4 * shift, N, H, W, C, st()))
        return dxd, host0
    (d1, host0), (d2, _) = run(), run()
    assert torch.equal(d1, d2)
    got = d1.cpu()
    n = P.numel()
    check_equal("maxpool3x3s2_bwd", cid, got[shift:shift + n].reshape(shape), (P.double() + ref).float())
    assert torch.equal(got[:shift], host0[:shift]) and torch.equal(got[shift + n:], host0[shift + n:])


# ----------------------------------------------------------------------------- nearest upsample + add backward
UP_SIZES = [(4, 6, 2, 3), (5, 7, 2, 3), (3, 3, 3, 3), (8, 2, 1, 1)]


@pytest.mark.parametrize("size", UP_SIZES, ids=[f"{H}x{W}-from-{h}x{w}" for H, W, h, w in UP_SIZES])
def test_upsample_nearest_add_bwd(size):
    H, W, h, w = size
    N = 2
    for C in (4, 12):
        g = torch.Generator().manual_seed(H * 100 + W + C)
        dd = torch.randn(N, H, W, C, generator=g)
        z = torch.zeros(N, h, w, C)
        dd = dd * G.fit_scale(vjp(lambda s: G.nearest_up(s, H, W), [z], dd)[0])
        ref = vjp(lambda s: G.nearest_up(s, H, W), [z], dd)[0]
        asum = vjp(lambda s: G.nearest_up(s, H, W), [z], dd.abs())[0]
        P = G.prefill((N * h * w, C), g)
        ddd = dev(dd)

        def run():
            ds = Win(N * h * w, C, init=P)
            ok(L().tt_upsample_nearest_add_bwd(ddd.data_ptr(), ds.ptr(), N, H, W, C, h, w, st()))
            return ds
        ds = twice(run)
        n = -(-H // h) * -(-W // w)                               # addends of one source pixel, summed from 0: no further rounding
        check("upsample_nearest_add_bwd", f"{H}x{W}<-{h}x{w} C={C}", delta(ds), ref.reshape(-1, C),
              bound=G.sum_bound(asum.reshape(-1, C), n, 0), slack=PREFILL_ULP)
        ds.untouched("upsample_nearest_add_bwd")
    zz = torch.zeros(64, device="cuda")
    assert L().tt_upsample_nearest_add_bwd(zz.data_ptr(), zz.data_ptr(), 1, 2, 2, 4, 3, 1, st()) != 0      # H < h


# ----------------------------------------------------------------------------- bilinear x2 backward
BL_SIZES = [(1, 1, "1x1-sh0-sw0"), (1, 5, "1x5-sh0"), (3, 1, "3x1-sw0"), (2, 2, "2x2"), (3, 5, "3x5"), (16, 11, "16x11-index-range")]


@pytest.mark.parametrize("H,W,cid", BL_SIZES, ids=[c for _, _, c in BL_SIZES])
def test_bilinear_up2_bwd(H, W, cid):
    N = 2
    for C in (4, 16):
        g = torch.Generator().manual_seed(H * 31 + W + C)
        x = torch.randn(N, H, W, C, generator=g)
        dy = torch.randn(N, 2 * H, 2 * W, C, generator=g)
        dy = dy * G.fit_scale(vjp(up2, [x], dy)[0])
        ref = vjp(up2, [x], dy)[0].reshape(-1, C)
        lim = G.f32_limit(vjp(up2, [x], dy, torch.float32)[0].reshape(-1, C), ref)
        P = G.prefill((N * H * W, C), g)
        dyd, xd = dev(dy), dev(x)

        def run():
            dx = Win(N * H * W, C, init=P)
            ok(L().tt_bilinear_up2_bwd(dyd.data_ptr(), dx.ptr(), N, H, W, C, st()))
            return dx
        dx = twice(run)
        check("bilinear_up2_bwd", f"{cid} C={C}", delta(dx), ref, rel=lim, slack=PREFILL_ULP)
        dx.untouched("bilinear_up2_bwd")
        # adjoint identity <up(x), dy> = <x, up^T(dy)> on the device results (the backward into zeros: no prefill rounding).
        # Forward: 4 addends + 3 roundings (two weights, the product); backward: at most 16 addends (the outputs whose source
        # coordinate lies within one pixel, per axis 4) + the same 3; both against sum |dy| up(|x|).
        up = Win(N * 4 * H * W, C)
        ok(L().tt_bilinear_up2(xd.data_ptr(), up.ptr(), N, H, W, C, 0, st()))
        dx0 = Win(N * H * W, C, init=torch.zeros(N * H * W, C))
        ok(L().tt_bilinear_up2_bwd(dyd.data_ptr(), dx0.ptr(), N, H, W, C, st()))
        lhs = float((up.get().double() * dy.double().reshape(-1, C)).sum())
        rhs = float((x.double().reshape(-1, C) * dx0.get().double()).sum())
        bound = float(G.sum_bound((dy.double().abs() * up2(x.double().abs())).sum(), 4 + 16, 6))
        print(f"PARITY bilinear adjoint {cid} C={C}: |lhs - rhs| {abs(lhs - rhs):.3e} bound {bound:.3e}")
        assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    zz = torch.zeros(64, device="cuda")
    assert L().tt_bilinear_up2_bwd(zz.data_ptr(), zz.data_ptr(), 1, 0, 2, 4, st()) != 0


# ----------------------------------------------------------------------------- spatial mean / mean+max backward
@pytest.mark.parametrize("HW", list(HW_IDS), ids=list(HW_IDS.values()))
def test_spatial_mean_bwd(HW):
    N = 2
    for C in (4, 64, 65, 100):
        for window in (False, True):
            g = torch.Generator().manual_seed(HW * 7 + C)
            cs, coff = (C + 24, 8) if window else (C, 0)
            dpool = torch.randn(N, C, generator=g)
            x0 = torch.zeros(N, HW, C)
            ref = vjp(lambda t: t.mean(1), [x0], dpool)[0].reshape(-1, C)
            lim = G.f32_limit(vjp(lambda t: t.mean(1), [x0], dpool, torch.float32)[0].reshape(-1, C), ref)
            P = G.prefill((N * HW, C), g)
            dpd = dev(dpool)

            def run():
                dx = Win(N * HW, C, cstride=cs, coff=coff, init=P)
                ok(L().tt_spatial_mean_bwd(dpd.data_ptr(), dx.ptr(), N, HW, C, cs, coff, st()))
                return dx
            dx = twice(run)
            check("spatial_mean_bwd", f"HW={HW} C={C}{' window' if window else ''}", delta(dx), ref, rel=lim, slack=PREFILL_ULP)
            dx.untouched("spatial_mean_bwd")
    zz = torch.zeros(64, device="cuda")
    assert L().tt_spatial_mean_bwd(zz.data_ptr(), zz.data_ptr(), 1, 2, 4, 6, 3, st()) != 0         # cstride < coff + C


@pytest.mark.parametrize("HW", list(HW_IDS), ids=list(HW_IDS.values()))
def test_spatial_meanmax_bwd_splits_evenly_among_ties(HW):
    N = 2

    def f(t):
        return 0.5 * t.mean(1) + 0.5 * t.amax(1)
    for C in (4, 64, 65, 100):
        g = torch.Generator().manual_seed(HW * 3 + C)
        x = torch.randn(N, HW, C, generator=g)                    # unique maxima ...
        x[0, :, 0] = 0.0                                          # ... an all-zero plane: an HW-way tie
        x[0, :, 1] = -x[0, :, 1].abs() - 1.0
        x[0, 0, 1] = x[0, HW - 1, 1] = 5.0                        # ... a two-way tie (one-way at HW = 1)
        dpool = torch.randn(N, C, generator=g)
        dpool = dpool * G.fit_scale(vjp(f, [x], dpool)[0])
        ref = vjp(f, [x], dpool)[0].reshape(-1, C)
        lim = G.f32_limit(vjp(f, [x], dpool, torch.float32)[0].reshape(-1, C), ref)
        P = G.prefill((N * HW, C), g)
        xd, dpd = dev(x), dev(dpool)

        def run():
            dx = Win(N * HW, C, init=P)
            ok(L().tt_spatial_meanmax_bwd(xd.data_ptr(), dpd.data_ptr(), dx.ptr(), N, HW, C, st()))
            return dx
        dx = twice(run)
        check("spatial_meanmax_bwd", f"HW={HW} C={C}", delta(dx), ref, rel=lim, slack=PREFILL_ULP)
        dx.untouched("spatial_meanmax_bwd")


# ----------------------------------------------------------------------------- channel gate backward
@pytest.mark.parametrize("C", [4, 64, 68], ids=["C=4", "C=64-full-slab", "C=68-second-slab-of-4"])
@pytest.mark.parametrize("form", ["plain", "out_relu+dres"])
def test_channel_gate_bwd(C, form):
    N = 2
    for HW in (1, 3, 5, 9):
        g = torch.Generator().manual_seed(HW * 13 + C)
        x, res = torch.randn(N, HW, C, generator=g), torch.randn(N, HW, C, generator=g)
        x[:, :, 0], res[:, :, 0] = 0.0, 0.0                       # out = relu(0 * s + 0) = 0 exactly: masked (out > 0), gradient 0
        gate = torch.randn(N, C, generator=g) * 2
        dy = torch.randn(N, HW, C, generator=g)
        xd, gd, rd = dev(x), dev(gate), dev(res)
        relu = form != "plain"
        if relu:                      # the saved output comes from the device forward; the reference masks with the same `out > 0`
            outw = Win(N * HW, C)
            ok(L().tt_channel_gate(xd.data_ptr(), gd.data_ptr(), rd.data_ptr(), outw.ptr(), N, HW, C, G.ACT_SIGMOID, G.ACT_RELU, 0, st()))
            out = outw.get().reshape(N, HW, C)
            assert bool((out[:, :, 0] == 0).all())
            mask = (out > 0)
            outd = dev(out)
        else:
            mask = torch.ones(N, HW, C, dtype=torch.bool)

        def f(x_, g_, r_):
            return (x_ * torch.sigmoid(g_).unsqueeze(1) + r_) * mask.to(x_.dtype)
        dy = dy * G.fit_scale(*vjp(f, [x, gate, res], dy))
        rx, rg, rr = vjp(f, [x, gate, res], dy)
        bx, _, br = vjp(f, [x, gate, res], dy, torch.float32)
        s = torch.sigmoid(gate.double())
        # dgate = s (1 - s) sum_p g x: HW addends; 6 roundings (exp, 1 + e, reciprocal, 1 - s, two products)
        bg = G.sum_bound(s * (1 - s) * (dy.double() * mask * x.double()).abs().sum(1), HW, 6)
        Px, Pg, Pr = G.prefill((N * HW, C), g), G.prefill((N, C), g), G.prefill((N * HW, C), g)
        dyd = dev(dy)

        def run():
            dx, dg, dr = Win(N * HW, C, init=Px), Win(N, C, init=Pg), Win(N * HW, C, init=Pr)
            ok(L().tt_channel_gate_bwd(xd.data_ptr(), gd.data_ptr(), dyd.data_ptr(), dx.ptr(), dg.ptr(), N, HW, C,
                                       outd.data_ptr() if relu else None, dr.ptr() if relu else None, st()))
            return dx, dg, dr
        dx, dg, dr = twice(run)
        case = f"{form} C={C} HW={HW}"
        check("channel_gate_bwd dx", case, delta(dx), rx.reshape(-1, C), rel=G.f32_limit(bx.reshape(-1, C), rx.reshape(-1, C)), slack=PREFILL_ULP)
        check("channel_gate_bwd dgate", case, delta(dg), rg, bound=bg, slack=PREFILL_ULP)
        if relu:
            check("channel_gate_bwd dres", case, delta(dr), rr.reshape(-1, C), rel=G.f32_limit(br.reshape(-1, C), rr.reshape(-1, C)),
                  slack=PREFILL_ULP)
            assert torch.equal(dr.get()[:, 0], dr.init()[:, 0]) and torch.equal(dx.get()[:, 0], dx.init()[:, 0])   # gradient exactly 0
        else:
            assert torch.equal(dr.buf.cpu(), dr.host0)            # no dres requested: not written
        for wbuf in (dx, dg, dr):
            wbuf.untouched("channel_gate_bwd")


# ----------------------------------------------------------------------------- LayerNorm backward
LNB_IDS = {1: "R=1-one-block", 3: "R=3", 4: "R=4", 5: "R=5", 255: "R=255", 256: "R=256-rows_per=1", 257: "rows_per=2-R=257-empty-blocks",
           600: "rows_per=3-R=600-empty-blocks"}
LNB_CASES = [(R, D, (LNB_IDS[R] if D == 65 and "R=" in i else i)) for R, D, i in LN_CASES]


@pytest.mark.parametrize("R,D,cid", LNB_CASES, ids=[i for _, _, i in LNB_CASES])
def test_layernorm_rows_bwd(R, D, cid):
    g = torch.Generator().manual_seed(R * 1000 + D)
    x = G.ln_rows(R, D, g)
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.3
    dout = torch.randn(R, D, generator=g)
    dout[0] *= 2.0 ** -9                                          # the constant row has rstd = 316: keep its dx below the prefill

    def f(x_, ga_, be_):
        return F.layer_norm(x_, (D,), ga_, be_, 1e-5)
    dout = dout * G.fit_scale(*vjp(f, [x, gamma, beta], dout))
    rx, rg, rb = vjp(f, [x, gamma, beta], dout)
    blocks = min(R, 256)
    rows_per = -(-R // blocks)
    if R in (257, 600):
        assert rows_per == (2 if R == 257 else 3) and blocks * rows_per - R >= rows_per     # trailing blocks that own no row
    bx, bg, bb = G.layernorm_bwd_bounds(x.double(), gamma.double(), dout.double(), 1e-5, chain=rows_per + blocks)
    xs, ds, dxs = D + 3, D + 2, D + 4
    xin, din = Win(R, D, cstride=xs, init=x), Win(R, D, cstride=ds, init=dout)
    gd = dev(gamma)
    Px, Pg, Pb = G.prefill((R, D), g), G.prefill((1, D), g), G.prefill((1, D), g)
    nb = int(L().tt_layernorm_rows_bwd_workspace_bytes(R, D))
    assert nb == blocks * 2 * D * 4

    def run():
        dx, dg, db = Win(R, D, cstride=dxs, init=Px), Win(1, D, init=Pg), Win(1, D, init=Pb)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        ok(L().tt_layernorm_rows_bwd(xin.ptr(), gd.data_ptr(), din.ptr(), dx.ptr(), dg.ptr(), db.ptr(), R, D, xs, ds, dxs, 1e-5,
                                     ws.data_ptr(), nb, st()))
        return dx, dg, db
    dx, dg, db = twice(run)
    check("layernorm_rows_bwd dx", cid, delta(dx), rx, bound=bx, slack=PREFILL_ULP)
    check("layernorm_rows_bwd dgamma", cid, delta(dg), rg.reshape(1, D), bound=bg.reshape(1, D), slack=PREFILL_ULP)
    check("layernorm_rows_bwd dbeta", cid, delta(db), rb.reshape(1, D), bound=bb.reshape(1, D), slack=PREFILL_ULP)
    for wbuf in (dx, dg, db):
        wbuf.untouched("layernorm_rows_bwd")
    # a workspace one byte short: an error code, no launch
    dx, dg, db = Win(R, D, cstride=dxs, init=Px), Win(1, D, init=Pg), Win(1, D, init=Pb)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    assert L().tt_layernorm_rows_bwd(xin.ptr(), gd.data_ptr(), din.ptr(), dx.ptr(), dg.ptr(), db.ptr(), R, D, xs, ds, dxs, 1e-5,
                                     ws.data_ptr(), nb - 1, st()) != 0
    for wbuf in (dx, dg, db):
        assert torch.equal(wbuf.buf.cpu(), wbuf.host0)


# ----------------------------------------------------------------------------- tt_ew backward
BWD_ACTS = [G.ACT_NONE, G.ACT_RELU, G.ACT_SIGMOID, G.ACT_SOFTPLUS, G.ACT_SOFTPLUS_CLAMP]


def ew_bwd_call(op, act, R, C, a, b, g, out, dout, da, db, dg):
    """Each of a, b, g, out, dout, da, db, dg: (pointer or None, row stride, channel offset)."""
    return L().tt_ew_bwd(op, act, R, C, a[0], a[1], a[2], b[0], b[1], b[2], g[0], g[1], g[2], out[0], out[1], out[2],
                         dout[0], dout[1], dout[2], da[0], da[1], da[2], db[0], db[1], db[2], dg[0], dg[1], dg[2], st())


NONE = (None, 0, 0)


def spec(w):
    return (w.ptr(), w.cs, w.coff)


def ew_forward_out(op, act, R, C, wa, wb, wg):
    out = Win(R, C, cstride=C + 9, coff=4)
    ok(L().tt_ew(wa.ptr(), wb.ptr() if op != 3 else None, wg.ptr() if op == 2 else None, out.ptr(), R, C, wa.cs, wa.coff,
                 wb.cs, wb.coff, wg.cs, wg.coff, out.cs, out.coff, op, act, 0, st()))
    return out


@pytest.mark.parametrize("R,C", [(1, 1), (7, 5), (64, 96)], ids=["1x1", "7x5", "64x96-24-blocks"])
def test_ew_bwd_every_op_and_activation_in_row_strided_windows(R, C):
    g = torch.Generator().manual_seed(R + C)
    a, b = torch.randn(R, C, generator=g) * 2, torch.randn(R, C, generator=g) * 2
    gt = torch.rand(R, C, generator=g)
    dout = torch.randn(R, C, generator=g) * 0.125                 # |gradient| <= (1 + |a| + |b|) |dout| stays below the prefill
    wa, wb, wg = Win(R, C, cstride=C + 3, coff=1, init=a), Win(R, C, cstride=C + 5, coff=2, init=b), Win(R, C, cstride=C + 7, coff=3, init=gt)
    wd = Win(R, C, cstride=C + 11, coff=5, init=dout)
    Pa, Pb, Pg = (G.prefill((R, C), g) for _ in range(3))
    for op in range(4):
        for act in BWD_ACTS:
            out = ew_forward_out(op, act, R, C, wa, wb, wg)
            refs = vjp(lambda a_, b_, g_: ew_ref(op, act, a_, b_, g_) + 0 * (a_ + b_ + g_), [a, b, gt], dout)
            base = vjp(lambda a_, b_, g_: ew_ref(op, act, a_, b_, g_) + 0 * (a_ + b_ + g_), [a, b, gt], dout, torch.float32)
            assert max(float(r.abs().max()) for r in refs) <= 8.0
            # da / db / dg each absent in turn (and all present): every gradient in its own window, a different coff each
            for drop in ((None,) if op != 2 else (None, 0, 1, 2)):
                def run():
                    ws = [Win(R, C, cstride=C + 2, coff=2, init=Pa), Win(R, C, cstride=C + 4, coff=1, init=Pb), Win(R, C, cstride=C + 6, coff=6, init=Pg)]
                    want = [True, op != 3, op == 2]
                    ptrs = [spec(w) if (want[i] and drop != i) else NONE for i, w in enumerate(ws)]
                    ok(ew_bwd_call(op, act, R, C, spec(wa), spec(wb) if op != 3 else NONE, spec(wg) if op == 2 else NONE, spec(out),
                                   spec(wd), *ptrs))
                    return ws
                ws = twice(run)
                for i, (w, name) in enumerate(zip(ws, ("da", "db", "dg"))):
                    live = [True, op != 3, op == 2][i] and drop != i
                    case = f"{R}x{C} op{op} {G.ACT_NAMES[act]} {name}" + (f" without-d{'abg'[drop]}" if drop is not None else "")
                    if live:
                        check("ew_bwd", case, delta(w), refs[i], rel=G.f32_limit(base[i], refs[i]), slack=PREFILL_ULP)
                        w.untouched("ew_bwd")
                    else:
                        assert torch.equal(w.buf.cpu(), w.host0), case
    # a and b the same tensor: both gradients go into one buffer
    for op in (0, 1):
        out = ew_forward_out(op, G.ACT_SIGMOID, R, C, wa, wa, wg)
        ref = vjp(lambda a_: ew_ref(op, G.ACT_SIGMOID, a_, a_, a_), [a], dout)[0]
        base = vjp(lambda a_: ew_ref(op, G.ACT_SIGMOID, a_, a_, a_), [a], dout, torch.float32)[0]

        def run_same():
            w = Win(R, C, cstride=C + 2, coff=2, init=Pa)
            ok(ew_bwd_call(op, G.ACT_SIGMOID, R, C, spec(wa), spec(wa), NONE, spec(out), spec(wd), spec(w), spec(w), NONE))
            return w
        w = twice(run_same)
        # two accumulations into the prefilled element: two prefill ulps
        check("ew_bwd", f"{R}x{C} op{op} sigmoid a-is-b", delta(w), ref, rel=G.f32_limit(base, ref), slack=2 * PREFILL_ULP)
        w.untouched("ew_bwd")


def test_ew_bwd_refuses_gelu_and_missing_operands():
    z = torch.zeros(8, device="cuda")
    zs = (z.data_ptr(), 1, 0)
    assert ew_bwd_call(3, G.ACT_GELU, 1, 1, zs, NONE, NONE, zs, zs, zs, NONE, NONE) != 0       # GELU needs the pre-activation
    assert ew_bwd_call(3, G.ACT_RELU, 1, 1, zs, NONE, NONE, NONE, zs, zs, NONE, NONE) != 0     # the saved output is missing
    assert ew_bwd_call(0, G.ACT_NONE, 1, 1, zs, NONE, NONE, NONE, zs, zs, NONE, NONE) != 0     # op 0 without b
    assert ew_bwd_call(2, G.ACT_NONE, 1, 1, zs, zs, NONE, NONE, zs, zs, NONE, NONE) != 0       # op 2 without g
    assert ew_bwd_call(4, G.ACT_NONE, 1, 1, zs, zs, NONE, NONE, zs, zs, NONE, NONE) != 0
    assert float(z.abs().sum()) == 0.0


PRE = [-30.0, -20.0, -17.0, -15.0, -10.0, -5.0, 0.0, 5.0, 19.9, 20.1, 25.0]
CLAMP_PRE = [-6.95, -6.85]          # softplus = 9.58e-4 / 1.0588e-3: either side of the clamp at 1e-3


@pytest.mark.parametrize("act", [G.ACT_SIGMOID, G.ACT_SOFTPLUS, G.ACT_SOFTPLUS_CLAMP], ids=["sigmoid", "softplus", "softplus_clamp"])
def test_ew_bwd_activation_derivative_per_element(act):
    """da / dout of op 3 per ELEMENT against float64, relative limit 8 * 2^-23 (a norm-relative check cannot see a derivative
    that is wrong where it is small: the parent commit's `1 - expf(-out)` is off by 4.6e-4 at pre = -10, 0.44 at -17 and returns 0
    from -20 down, all below 6e-8 absolute).

    The kernel differentiates from the SAVED OUTPUT o, so the reference is the float64 derivative as a function of the f32
    value the kernel receives: sigmoid o (1 - o), softplus 1 - exp(-o).  For the softplus forms it is also held to the
    derivative at the pre-activation itself, sigmoid(pre): d log(1 - exp(-o)) / d log o <= 1, so the forward's rounding of o
    costs no more than its own relative error.  That second check is not possible for the sigmoid: o rounds to 1 from
    pre = 17 up and o (1 - o) has lost the derivative in the saved value, whatever the kernel does."""
    pre = torch.tensor(PRE + (CLAMP_PRE if act == G.ACT_SOFTPLUS_CLAMP else []))
    C = pre.numel()
    wa = Win(1, C, init=pre)
    out = ew_forward_out(3, act, 1, C, wa, wa, wa)
    wd = Win(1, C, init=torch.ones(1, C))

    def run():
        da = Win(1, C, cstride=C + 3, coff=2, init=torch.zeros(1, C))
        ok(ew_bwd_call(3, act, 1, C, spec(wa), NONE, NONE, spec(out), spec(wd), spec(da), NONE, NONE))
        return da
    da = twice(run)
    got = da.get().double().reshape(-1)
    o = out.get().double().reshape(-1)
    from_out = o * (1 - o) if act == G.ACT_SIGMOID else -torch.expm1(-o)
    at_pre = torch.sigmoid(pre.double())
    if act == G.ACT_SOFTPLUS_CLAMP:
        clamped = F.softplus(pre.double()) < 1e-3
        assert clamped.tolist() == [True] * 5 + [False] * 6 + [True, False]
        assert bool((got[clamped] == 0).all()), got[clamped]          # below the clamp: gradient exactly 0
        from_out, at_pre = from_out * ~clamped, at_pre * ~clamped
    lim = 8 * 2.0 ** -23
    for name, ref in (("saved-output", from_out),) + ((("pre-activation", at_pre),) if act != G.ACT_SIGMOID else ()):
        rel = ((got - ref).abs() / ref.abs().clamp(min=1e-300)) * (ref != 0)
        print(f"PARITY ew_bwd derivative {G.ACT_NAMES[act]} vs {name}: per-element relative error " + " ".join(f"{v:.1e}" for v in rel.tolist()))
        G._record("ew_bwd act' per element", f"{G.ACT_NAMES[act]} vs {name}", float(rel.max()), lim, "(relative per element)")
        assert bool((rel <= lim).all()), (name, rel.tolist())
        assert bool((got[ref == 0] == 0).all())
    da.untouched("ew_bwd")


def test_ew_bwd_above_the_backward_grid_cap():
    """R * C = 16385 * 1024: 65,540 blocks of 256 against the 65,536-block cap (the last 1,024 elements take the second trip of
    the grid-stride loop).  op 1 (out = (1 - b) a): da = (1 - b) dout, db = -a dout; five f32 tensors of 67 MB."""
    R, C = 16385, 1024
    assert (R * C + 255) // 256 > 65536
    g = torch.Generator().manual_seed(9)
    a, b, dout = (torch.randn(R, C, generator=g) for _ in range(3))
    dout *= 2.0 ** -4                                             # |gradient| <= (1 + |b|) |dout| stays below the prefill
    P = (8.0 + (torch.arange(R * C) % 7).float()).reshape(R, C)
    ad, bd, dd = a.cuda(), b.cuda(), dout.cuda()
    da, db = Win(R, C, init=P), Win(R, C, init=P)
    ok(ew_bwd_call(1, G.ACT_NONE, R, C, (ad.data_ptr(), C, 0), (bd.data_ptr(), C, 0), NONE, NONE, (dd.data_ptr(), C, 0), spec(da), spec(db), NONE))
    for w, name, f in ((da, "da", lambda x, y, d: (1 - y) * d), (db, "db", lambda x, y, d: -x * d)):
        ref = f(a.double(), b.double(), dout.double())
        lim = G.f32_limit(f(a, b, dout), ref)
        got = w.get().double() - P.double()
        assert float(ref.abs().max()) <= 8.0
        check("ew_bwd", f"grid-cap 16385x1024 op1 {name}", got, ref, rel=lim, slack=PREFILL_ULP)
        del ref, got
        w.untouched("ew_bwd")


# ----------------------------------------------------------------------------- concat piece backward
CPB = [(1, 0, "div1"), (4, 0, "div4"), (1, 4, "mod4"), (2, 3, "div2-mod3")]


@pytest.mark.parametrize("div,mod,cid", CPB, ids=[c for _, _, c in CPB])
@pytest.mark.parametrize("data", ["integer", "real"])
def test_concat_piece_bwd(div, mod, cid, data):
    R, C, coff, ostride = CAT_R, 5, 3, 5 + 3 + 4
    g = torch.Generator().manual_seed(div * 10 + mod)
    rows = cat_rows_of(div, mod)
    src_rows = int(rows.max()) + 1
    if data == "integer":
        dout = torch.randint(-9, 10, (R, C), generator=g).float()
        P = torch.randint(1, 9, (src_rows, C), generator=g).float()
    else:
        dout = torch.randn(R, C, generator=g) * 0.3
        P = G.prefill((src_rows, C), g)
    ref = torch.zeros(src_rows, C, dtype=torch.float64).index_add(0, rows, dout.double())
    asum = torch.zeros(src_rows, C, dtype=torch.float64).index_add(0, rows, dout.double().abs())
    din = Win(R, C, cstride=ostride, coff=coff, init=dout)

    def run():
        ds = Win(src_rows, C, cstride=C + 2, init=P)
        ok(L().tt_concat_piece_bwd(din.ptr(), ostride, coff, R, C, div, mod, ds.ptr(), C + 2, src_rows, st()))
        return ds
    ds = twice(run)
    if data == "integer":
        check_equal("concat_piece_bwd", f"{cid} integer", ds.get(), (P.double() + ref).float())
    else:
        n = int(torch.bincount(rows).max())                      # output rows that read one source row, summed from 0
        check("concat_piece_bwd", f"{cid} real", delta(ds), ref, bound=G.sum_bound(asum, n, 0), slack=PREFILL_ULP)
    ds.untouched("concat_piece_bwd")


# ----------------------------------------------------------------------------- broadcast rows backward
@pytest.mark.parametrize("N,HW,C", [(1, 1, 1), (3, 5, 7), (2, 441, 32)], ids=["1x1x1", "3x5x7", "2x441x32"])
def test_broadcast_rows_bwd(N, HW, C):
    g = torch.Generator().manual_seed(N + HW + C)
    dout = torch.randn(N, HW, C, generator=g)
    dout = dout * G.fit_scale(dout.double().sum(1))
    ref, asum = dout.double().sum(1), dout.double().abs().sum(1)
    din = Win(N * HW, C, cstride=C + 6, coff=5, init=dout)
    P = G.prefill((N, C), g)

    def run():
        dv = Win(N, C, cstride=C + 3, coff=2, init=P)             # strided dv
        ok(L().tt_broadcast_rows_bwd(din.ptr(), dv.wptr(), N, HW, C, C + 6, 5, C + 3, st()))
        return dv
    dv = twice(run)
    check("broadcast_rows_bwd", f"{N}x{HW}x{C}", delta(dv), ref, bound=G.sum_bound(asum, HW, 0), slack=PREFILL_ULP)
    dv.untouched("broadcast_rows_bwd")


# ----------------------------------------------------------------------------- deformable columns backward
DEFB = [(1, 2, 2, 18), (2, 5, 7, 27), (2, 5, 7, 18)]
C_IDS = {4: "C=4-one-trip-4-lanes", 8: "C=8", 68: "C=68-second-trip-4-lanes", 132: "C=132-third-trip-ragged"}


@pytest.mark.parametrize("C", list(C_IDS), ids=list(C_IDS.values()))
@pytest.mark.parametrize("kind", ["integer", "random"], ids=["integer-offsets-gx-only", "random-offsets-3sigma"])
@pytest.mark.parametrize("N,H,W,cs", DEFB, ids=[f"{n}x{h}x{w}-offstride{c}" for n, h, w, c in DEFB])
def test_deform_im2col3x3_bwd(C, kind, N, H, W, cs):
    from oracle import model_ref
    g = torch.Generator().manual_seed(H * W + C + cs)
    x = torch.randn(N, H, W, C, generator=g)
    off = deform_offsets(kind, N, H, W, cs, g)
    gcols = torch.randn(N * H * W, 9, C, generator=g)

    def f(x_, o_):
        return model_ref.deform_im2col(nchw(x_), nchw(o_)).permute(0, 3, 4, 2, 1).reshape(N * H * W, 9, C)
    gcols = gcols * G.fit_scale(*vjp(f, [x, off[..., :18]], gcols))
    rx, ro = vjp(f, [x, off[..., :18]], gcols)
    # bounds from the float64 corner restatement (u = 2^-24).  A coordinate py = base + off is rounded once, |py| u, which moves
    # the weights by as much; the weights take two more roundings and each product one:
    #   gx[pixel]  : cnt addends (atomic, any order) + 1, and per addend |g| u (|py| + |px| + 4) for its weight
    #   goff[p,tap]: one wave sums the C channels (G.wave_sum_depth additions per addend), 8 roundings (weights, differences,
    #                products) + the coordinate rounding, against sum_c |g| (|a00| + |a01| + |a10| + |a11|)
    s = G.deform_sample(x, off)
    g64 = gcols.double().reshape(N, H, W, 9, 1, C)
    coord = (s["py"].abs() + s["px"].abs()).unsqueeze(-1)                                          # [N,H,W,9,1]
    wv = (s["w"] * s["valid"]).unsqueeze(-1)                                                       # [N,H,W,9,4,1]
    idx = s["idx"].reshape(-1)
    add_abs = (g64.abs() * wv).expand(N, H, W, 9, 4, C).reshape(-1, C)
    w_err = (g64.abs() * (s["valid"].unsqueeze(-1) * G.U32 * (coord + 4).unsqueeze(-1))).expand(N, H, W, 9, 4, C).reshape(-1, C)
    zeros = torch.zeros(N * H * W, C, dtype=torch.float64)
    cnt = torch.zeros(N * H * W, dtype=torch.float64).index_add(0, idx, s["valid"].reshape(-1).double())
    bgx = (cnt + 1).unsqueeze(1) * G.U32 * zeros.index_add(0, idx, add_abs) + zeros.index_add(0, idx, w_err)
    corner_abs = (g64.abs() * s["a"].abs()).sum((4, 5))                                            # [N,H,W,9]
    bgo = ((G.wave_sum_depth(C) + 8) + 2 * (coord.squeeze(-1) + 2)) * G.U32 * corner_abs
    bgo = torch.stack([bgo, bgo], -1).reshape(N * H * W, 18)
    far = ((s["py"] - s["py"].round()).abs() > 1e-4) & ((s["px"] - s["px"].round()).abs() > 1e-4)  # [N,H,W,9]
    far2 = torch.stack([far, far], -1).reshape(N * H * W, 18)
    if kind == "random":                                          # the reference alone excludes < 1 % of the (pixel, tap) pairs
        assert float((~far).double().mean()) < 0.01
    xd, od, gd = dev(x), dev(off), dev(gcols)
    Px, Po = G.prefill((N * H * W, C), g), G.prefill((N * H * W, 18), g)

    def run():
        gx, go = Win(N * H * W, C, init=Px), Win(N * H * W, 18, cstride=cs, init=Po)
        ok(L().tt_deform_im2col3x3_bwd(xd.data_ptr(), od.data_ptr(), gd.data_ptr(), gx.ptr(), go.ptr(), N, H, W, C, cs, 1, st()))
        return gx, go
    (gx, go), (gx2, go2) = run(), run()
    assert torch.equal(go.buf, go2.buf)                           # goff is bit-identical; gx accumulates through float atomics
    case = f"{N}x{H}x{W} C={C} offstride={cs} {kind}"
    # gx is scattered: each of the cnt addends of an element is an atomic add INTO the prefilled destination and is rounded at the
    # prefill's magnitude, so the accumulation allowance is one prefill ulp per addend, not one per element (measured with one
    # ulp per element: up to 5e-6 absolute at cnt ~ 20, against 1.5e-6).  The launch into zeros below has no such term.
    acc = cnt.unsqueeze(1) * PREFILL_ULP
    check("deform_im2col3x3_bwd gx", case, delta(gx), rx.reshape(-1, C), bound=bgx + acc)
    check("deform_im2col3x3_bwd gx", case + " (second run)", delta(gx2), rx.reshape(-1, C), bound=bgx + acc)
    gx0, go0 = Win(N * H * W, C, init=torch.zeros(N * H * W, C)), Win(N * H * W, 18, cstride=cs, init=Po)
    ok(L().tt_deform_im2col3x3_bwd(xd.data_ptr(), od.data_ptr(), gd.data_ptr(), gx0.ptr(), go0.ptr(), N, H, W, C, cs, 1, st()))
    check("deform_im2col3x3_bwd gx", case + " (into zeros)", gx0.get(), rx.reshape(-1, C), bound=bgx)
    if kind == "random":
        got_o, ref_o = delta(go) * far2, ro.reshape(-1, 18) * far2
        check("deform_im2col3x3_bwd goff", case, got_o, ref_o, bound=bgo, slack=PREFILL_ULP)
    for wbuf in (gx, go, gx2):
        wbuf.untouched("deform_im2col3x3_bwd")                    # goff's columns 18 .. off_cstride - 1 among them


def test_deform_im2col3x3_bwd_refuses_empty_dimensions():
    z = torch.zeros(64, device="cuda")
    p = z.data_ptr()
    for bad in [(0, 2, 2, 4, 18), (1, 0, 2, 4, 18), (1, 2, -1, 4, 18), (1, 2, 2, 0, 18), (1, 2, 2, -4, 18), (1, 2, 2, 4, 17)]:
        n, h, w, c, s_ = bad
        assert L().tt_deform_im2col3x3_bwd(p, p, p, p, p, n, h, w, c, s_, 1, st()) != 0, bad
    assert float(z.abs().sum()) == 0.0


# ----------------------------------------------------------------------------- lift-splat backward
X, Y, Z = 7, 5, 1
LS = [((1, 1, 1, 1, 1, 4), "one-pixel-D=1-C=4"), ((2, 2, 64, 3, 5, 64), "D=64-first-half-only-C=64"), ((1, 2, 65, 2, 3, 80), "D=65-second-half-one-lane"),
      ((1, 1, 128, 2, 2, 256), "D=128-C=256-all-lanes"), ((2, 4, 59, 3, 4, 80), "D=59-24-blocks")]


@pytest.mark.parametrize("dims,cid", LS, ids=[c for _, c in LS])
def test_lift_splat_bwd(dims, cid):
    B, ncam, D, fH, fW, C = dims
    g = torch.Generator().manual_seed(sum(dims))
    npix = B * ncam * fH * fW
    logits = torch.randn(B * ncam, fH, fW, D, generator=g) * 2
    ctx = torch.randn(B * ncam, fH, fW, C, generator=g)
    geom = torch.stack([torch.randint(-2, X + 2, (B, ncam, D, fH, fW), generator=g), torch.randint(-2, Y + 2, (B, ncam, D, fH, fW), generator=g),
                        torch.randint(-1, 2, (B, ncam, D, fH, fW), generator=g)], -1).to(torch.int32)
    special = npix > 2
    if special:
        geom[0, 0, :, 0, 0, 0] = -1                               # pixel 0: every bin out of range
        geom[0, 0, :, 0, 1] = torch.tensor([3, 2, 0], dtype=torch.int32)      # pixel 1: every bin in the cell (x 3, y 2)
    gflat = geom.reshape(B, ncam * D * fH * fW, 3).contiguous()
    gbev = torch.randn(B, Y, X, C, generator=g)

    def f(l_, c_):
        return G.lift_splat_ref(l_, c_, gflat, (X, Y, Z), B, ncam)
    gbev = gbev * G.fit_scale(*vjp(f, [logits, ctx], gbev))
    rl, rc = vjp(f, [logits, ctx], gbev)
    # bounds (u = 2^-24), from the per-pixel cells: p = softmax (exp, D addends, reciprocal, product: D + 6 relative),
    #   dctx[c]  = sum_d p_d g[cell d][c]                 : D addends + the error of p       -> (2 D + 6) u sum_d p_d |g|
    #   dlogit_d = p_d (q_d - sum_d' p_d' q_d'), q = <ctx, g>: C addends in q, D in the sum, p, the final two
    #                                                        -> (2 D + C + 12) u p_d (A_d + sum_d' p_d' A_d'),  A = <|ctx|, |g|>
    gp = geom.permute(0, 1, 3, 4, 2, 5).reshape(npix, D, 3).long()
    okc = (gp[..., 0] >= 0) & (gp[..., 0] < X) & (gp[..., 1] >= 0) & (gp[..., 1] < Y) & (gp[..., 2] >= 0) & (gp[..., 2] < Z)
    bidx = (torch.arange(npix) // (ncam * fH * fW)).view(npix, 1).expand(npix, D)
    cell = (bidx * Y + gp[..., 1].clamp(0, Y - 1)) * X + gp[..., 0].clamp(0, X - 1)
    gsel = gbev.double().reshape(B * Y * X, C)[cell] * okc.unsqueeze(-1)                      # [npix, D, C]
    p = logits.double().reshape(npix, D).softmax(-1)
    bctx = G.sum_bound((p.unsqueeze(-1) * gsel.abs()).sum(1), 2 * D, 6)
    A = (ctx.double().reshape(npix, 1, C).abs() * gsel.abs()).sum(-1)                         # [npix, D]
    blog = G.sum_bound(p * (A + (p * A).sum(1, keepdim=True)), 2 * D + C, 12)
    gin = Win(B * Y * X, C, cstride=C + 16, coff=8, init=gbev)     # the BEV gradient in a channel window
    ld, cd, gd = dev(logits), dev(ctx), gflat.cuda()
    Pl, Pc = G.prefill((npix, D), g), G.prefill((npix, C), g)

    def run():
        dl, dc = Win(npix, D, init=Pl), Win(npix, C, init=Pc)
        ok(L().tt_lift_splat_bwd(B, ncam, D, fH, fW, C, X, Y, Z, ld.data_ptr(), cd.data_ptr(), gd.data_ptr(), gin.ptr(), C + 16, 8,
                                 dl.ptr(), dc.ptr(), st()))
        return dl, dc
    dl, dc = twice(run)
    check("lift_splat_bwd dlogits", cid, delta(dl), rl.reshape(npix, D), bound=blog, slack=PREFILL_ULP)
    check("lift_splat_bwd dctx", cid, delta(dc), rc.reshape(npix, C), bound=bctx, slack=PREFILL_ULP)
    if special:
        assert not bool(okc[0].any()) and bool(okc[1].all()) and int(cell[1].min()) == int(cell[1].max())
        assert torch.equal(dl.get()[0], dl.init()[0]) and torch.equal(dc.get()[0], dc.init()[0])     # nothing reaches pixel 0
    dl.untouched("lift_splat_bwd")
    dc.untouched("lift_splat_bwd")


def test_lift_splat_bwd_refuses_what_its_lanes_cannot_hold():
    z = torch.zeros(1024, device="cuda")
    p = z.data_ptr()
    for D, C, cs, coff in [(129, 4, 4, 0), (4, 6, 8, 0), (4, 4, 8, 2), (4, 260, 260, 0), (4, 4, 6, 0)]:
        assert L().tt_lift_splat_bwd(1, 1, D, 1, 1, C, X, Y, Z, p, p, p, p, cs, coff, p, p, st()) != 0, (D, C, cs, coff)
    assert float(z.abs().sum()) == 0.0
