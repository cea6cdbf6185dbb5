"""Op-level parity of the backward look-module kernels (csrc/look_bwd.hip) against torch autograd through the float64
restatements of tests/look_ref.py, in the pattern of test_glue_bwd.py: every gradient destination is pre-filled (the kernels
document `+=`) inside a buffer with sentinel guard rows and, for the strided value gradient, guard columns; `got - prefill` is
compared with the reference plus one ulp of the prefill; two runs are bit-identical except where f32 atomics accumulate."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import glue_ref as G  # noqa: E402
import look_ref as K  # noqa: E402
from glue_ref import PREFILL_ULP, Win, check, vjp  # noqa: E402
from test_glue_ops import L, ok, st, twice  # noqa: E402
from test_look_ops import NAN, WINDOWS, dev, hw_arg, level_args, max_lens, windowed  # noqa: E402

pytestmark = pytest.mark.gpu


def delta(win):
    """What a kernel added to a prefilled window, in float64."""
    return win.get().double() - win.init().double()


# ----------------------------------------------------------------------------- tt_msda_sample_bwd
@functools.lru_cache(maxsize=None)
def msda_bwd_refs(name, B):
    """Cotangent (scaled so that every gradient stays below 4), float64 gradients, f32-autograd baselines and, for the atomically
    scattered dvalue, per element: the number of addends, sum |addend| and the bound of the addends' own error."""
    c = K.msda_case(name, B)
    hw, BC, R = c["level_hw"], B * 4, B * 480
    g = torch.Generator().manual_seed(90 + B)
    dout = torch.randn(R, 256, generator=g)
    xs = [c["value"], c["offsets"], c["logits"]]

    def f(value, offsets, logits, **kw):
        return K.msda_ref(value, offsets, logits, c["ref"].to(value.dtype), hw, **kw)
    refs = vjp(f, xs, dout)
    s = G.fit_scale(*refs)
    dout = dout * s
    refs = [r * s for r in refs]
    base = vjp(f, xs, dout, torch.float32)
    asum = vjp(f, xs, dout.abs())[0]                              # every weight is >= 0: the same map carries sum |addend|
    cerr = vjp(lambda v, o, l: f(v, o, l, corner_w=K.msda_coord_err(c["offsets"], c["ref"], hw)), xs, dout.abs())[0]
    cnt = K.msda_touch_count(c["offsets"], c["ref"], hw, BC).unsqueeze(-1).expand(BC, -1, 8, 32).reshape(BC, -1, 256)
    return c, dout, refs, base, asum, cerr, cnt


@pytest.mark.parametrize("name", ["lattice", "random"])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_msda_sample_bwd(B, name):
    """dvalue: an element takes cnt atomic addends g w (1 - ly) (1 - lx) in any order.  sum_bound with n = cnt and k = 40: the
    softmax weight (the difference, the exponential, a 32-term positive sum with its 32 exponentials and the division: 34),
    the two complements and the four products of the addend (6); plus, per addend, the rounding of the pixel coordinates
    (look_ref.msda_coord_err) times |g| w.  Into a prefilled destination every atomic add rounds at the prefill's magnitude:
    cnt prefill ulps; the launch into zeros has no such term."""
    c, dout, (rv, ro, rl), (bv, bo, bl), asum, cerr, cnt = msda_bwd_refs(name, B)
    hw, BC, R = c["level_hw"], B * 4, B * 480
    S = c["value"].shape[1]
    bval = (G.sum_bound(asum, cnt, 40) + cerr).reshape(BC * S, 256)
    lim_o, lim_l = G.f32_limit(bo, ro), G.f32_limit(bl, rl)
    g = torch.Generator().manual_seed(B)
    Po, Pl = G.prefill((R, 512), g), G.prefill((R, 256), g)
    od, ld, rd, dd, hwa = dev(c["offsets"]), dev(c["logits"]), dev(c["ref"]), dev(dout), hw_arg(hw)
    x, y = K.msda_pixels(c["offsets"].double(), c["ref"].double(), hw)
    for cs, coff in WINDOWS:
        vd = windowed(c["value"], cs, coff)
        Pv = G.prefill((BC * S, 256), g)

        def run(init_v=Pv):
            dv, do, dl = Win(BC * S, 256, cstride=cs, coff=coff, init=init_v), Win(R, 512, init=Po), Win(R, 256, init=Pl)
            ok(L().tt_msda_sample_bwd(B, vd.data_ptr(), cs, coff, od.data_ptr(), ld.data_ptr(), rd.data_ptr(), hwa, dd.data_ptr(),
                                      dv.ptr(), do.ptr(), dl.ptr(), st()))
            return dv, do, dl
        (dv, do, dl), (dv2, do2, dl2) = run(), run()
        assert torch.equal(do.buf, do2.buf) and torch.equal(dl.buf, dl2.buf)       # dvalue accumulates through float atomics
        case = f"{name} B={B} cstride={cs} coff={coff}"
        check("msda_sample_bwd doffsets", case, delta(do), ro, rel=lim_o, slack=PREFILL_ULP)
        check("msda_sample_bwd dlogits", case, delta(dl), rl, rel=lim_l, slack=PREFILL_ULP)
        acc = cnt.reshape(BC * S, 256) * PREFILL_ULP
        check("msda_sample_bwd dvalue", case, delta(dv), rv.reshape(BC * S, 256), bound=bval + acc)
        check("msda_sample_bwd dvalue", case + " (second run)", delta(dv2), rv.reshape(BC * S, 256), bound=bval + acc)
        dv0 = run(torch.zeros(BC * S, 256))[0]
        check("msda_sample_bwd dvalue", case + " (into zeros)", dv0.get(), rv.reshape(BC * S, 256), bound=bval)
        free = (cnt.reshape(BC * S, 256) == 0)
        assert torch.equal(dv.get()[free], dv.init()[free])                        # no sample touches it: the prefill, bit for bit
        if name == "lattice":
            assert int(free.sum()) >= S * 32
            # the one-sided derivative: samples at exactly integral coordinates (on the map's edge, just outside it, inside it)
            on_x = (x == x.round()) & (x >= -1) & (x <= torch.tensor([w for _, w in hw]).view(1, 1, 4, 1))
            on_y = (y == y.round()) & (y >= -1) & (y <= torch.tensor([h for h, _ in hw]).view(1, 1, 4, 1))
            m = torch.stack([on_x, on_y], -1).reshape(R, 512)
            assert int(((ro != 0) & m).sum()) > 1000
            check("msda_sample_bwd doffsets", case + " integral coordinates", delta(do) * m, ro * m, rel=lim_o, slack=PREFILL_ULP)
        for w in (dv, do, dl, dv2, dv0):
            w.untouched("msda_sample_bwd")


# ----------------------------------------------------------------------------- tt_look_gather_query_bwd
@pytest.mark.parametrize("row_stride", [1543, 1552])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_look_gather_query_bwd(B, row_stride):
    """Five destinations, all atomic scatters of one row's columns: dtemporal / dstatic (rows of the point), dmeas / dflat (rows of
    the sample), the four level maps (bilinear corners).  sum_bound with n = the number of rows (corners) that land on the
    element, counted from query_of_slot and the reference corners; k = 0 for the copied columns and 4 for a corner weight (two
    complements, two products) plus the rounding of the pixel coordinate x = rx W - 0.5 (two roundings: 2 u (|rx| W + 1)) per axis."""
    g = torch.Generator().manual_seed(50 + B)
    qos, ref, t, maps = K.gather_inputs(B, g, torch.float32)
    R, BC = B * 480, B * 4
    live = (qos.reshape(-1) >= 0)
    dout = torch.randn(R, 1543, generator=g)
    dout[:, :7] = 0.0                                             # the waypoint / control columns are detached
    xs = [t["temporal"], t["static"], t["meas"], t["flat"]] + maps

    def f(te, se, me, fl, *mp):
        d = te.dtype
        return K.gather_query_ref(qos, ref.to(d), t["wp"].to(d), t["ctrl"].to(d), te, se, me, fl, list(mp))
    refs = vjp(f, xs, dout)
    s = G.fit_scale(*refs)
    dout = dout * s
    refs = [r * s for r in refs]
    asum = vjp(f, xs, dout.abs())
    # addend counts
    q = qos.reshape(-1).long().clamp(min=0)
    pt, b = q // 15, torch.arange(R) // 480
    n_pt = torch.zeros(8, dtype=torch.float64).index_add(0, pt[live], torch.ones(int(live.sum()), dtype=torch.float64))
    n_b = torch.zeros(B, dtype=torch.float64).index_add(0, b[live], torch.ones(int(live.sum()), dtype=torch.float64))
    counts = [n_pt[:4].view(4, 1), n_pt[4:].view(4, 1), n_b.view(B, 1), n_b.view(B, 1)]
    bounds = [G.sum_bound(a, n, 0) for a, n in zip(asum[:4], counts)]
    r2 = ref.double().reshape(BC, 120, 2)
    gabs = dout.double().abs().reshape(BC, 120, 1543)[:, :, 519:].reshape(BC, 120, 256, 4) * live.reshape(BC, 120, 1, 1)
    for lv, m in enumerate(maps):
        H, W = m.shape[1], m.shape[2]
        idx, _, valid = K.bilinear_corners(r2[..., 0] * W - 0.5, r2[..., 1] * H - 0.5, H, W)          # (BC,120,4)
        valid = valid & live.reshape(BC, 120, 1)
        flat = (torch.arange(BC).view(BC, 1, 1) * H * W + idx)
        cnt = torch.zeros(BC * H * W, dtype=torch.float64).index_add(0, flat[valid], torch.ones(int(valid.sum()), dtype=torch.float64))
        cerr = 2 * G.U32 * ((r2[..., 0].abs() * W + 1) + (r2[..., 1].abs() * H + 1))                   # (BC,120)
        werr = (gabs[..., lv] * cerr.unsqueeze(-1)).unsqueeze(2).expand(BC, 120, 4, 256)
        we = torch.zeros(BC * H * W, 256, dtype=torch.float64).index_add(0, flat[valid], werr[valid])
        counts.append(cnt.view(-1, 1))
        bounds.append(G.sum_bound(asum[4 + lv].reshape(-1, 256), cnt.view(-1, 1), 4) + we)
    names = ["dtemporal", "dstatic", "dmeas", "dflat", "dmap0", "dmap1", "dmap2", "dmap3"]
    shapes = [(4, 128), (4, 128), (B, 128), (B, 256)] + [(BC * m.shape[1] * m.shape[2], 256) for m in maps]
    P = [G.prefill(sh, g) for sh in shapes]
    dwide = torch.full((R, row_stride), NAN)                      # columns 0..6 and the pad columns must not be read
    dwide[:, 7:1543] = dout[:, 7:]
    qd, rd, dd = dev(qos), dev(ref), dev(dwide)
    hwa = hw_arg([(m.shape[1], m.shape[2]) for m in maps])

    def run(zero=False):
        ws = [Win(sh[0], sh[1], init=(torch.zeros(sh) if zero else p)) for sh, p in zip(shapes, P)]
        arr = (ctypes.c_void_p * 4)(*[w.ptr() for w in ws[4:]])
        ok(L().tt_look_gather_query_bwd(B, qd.data_ptr(), rd.data_ptr(), dd.data_ptr(), row_stride, ws[0].ptr(), ws[1].ptr(), ws[2].ptr(),
                                        ws[3].ptr(), arr, hwa, st()))
        return ws
    ws, ws0 = run(), run(zero=True)
    case = f"B={B} row_stride={row_stride}"
    for name, w, w0, r, bnd, n, sh in zip(names, ws, ws0, refs, bounds, counts, shapes):
        kernel = "look_gather_query_bwd " + (name if not name.startswith("dmap") else "dmaps")
        check(kernel, f"{case} {name}", delta(w), r.reshape(sh), bound=bnd + n * PREFILL_ULP)
        check(kernel, f"{case} {name} (into zeros)", w0.get(), r.reshape(sh), bound=bnd)
        free = (n.expand(sh) == 0)
        assert torch.equal(w.get()[free], w.init()[free])         # nothing lands here (-1 rows contribute nothing)
        w.untouched("look_gather_query_bwd")
        w0.untouched("look_gather_query_bwd")
    assert int((~live).sum()) > 80


# ----------------------------------------------------------------------------- tt_sca_reduce_bwd
@pytest.mark.parametrize("B", [1, 2, 3])
def test_sca_reduce_bwd(B):
    """Every row in [B, min(max_len, 120)) takes one add of dout / B: the rounding of the division and one prefill ulp; every other
    row keeps its prefill bit for bit."""
    R = B * 480
    for max_len in max_lens(B):
        g = torch.Generator().manual_seed(B * 100 + max_len)
        dout = torch.randn(B, 1024, generator=g)
        x0 = torch.zeros(R, 256)
        ref = vjp(lambda x: K.sca_reduce_ref(x, max_len, B), [x0], dout)[0]
        P = G.prefill((R, 256), g)
        dd, ml = dev(dout), torch.tensor([max_len], dtype=torch.int32).cuda()

        def run():
            dx = Win(R, 256, init=P)
            ok(L().tt_sca_reduce_bwd(B, dd.data_ptr(), ml.data_ptr(), dx.ptr(), st()))
            return dx
        dx = twice(run)
        check("sca_reduce_bwd", f"B={B} max_len={max_len}", delta(dx), ref, bound=G.U32 * ref.abs(), slack=PREFILL_ULP)
        slot = torch.arange(R) % 120
        outside = (slot < B) | (slot >= min(max_len, 120))
        assert torch.equal(dx.get()[outside], dx.init()[outside])
        assert bool((ref[outside] == 0).all()) and (max_len <= B or bool((ref[~outside] != 0).any()))
        dx.untouched("sca_reduce_bwd")


# ----------------------------------------------------------------------------- error codes
def test_look_bwd_entry_points_refuse_bad_arguments_before_any_launch():
    B = 1
    buf = Win(480, 512)
    z = torch.zeros(480 * 1552 + 4096, device="cuda")
    p, o = z.data_ptr(), buf.ptr()
    maps = [torch.zeros(4, h, w, 256, device="cuda") for h, w in K.GQ_HW]
    arr, hw = level_args(maps)
    hw0 = (ctypes.c_int * 8)(5, 7, 3, 4, 0, 3, 1, 1)
    s, lib = st(), L()

    def mb(B=B, v=p, cs=256, coff=0, off=p, lg=p, ref=p, hw=hw, dout=p, dv=o, do=o, dl=o):
        return lib.tt_msda_sample_bwd(B, v, cs, coff, off, lg, ref, hw, dout, dv, do, dl, s)

    def gb(B=B, qos=p, ref=p, dout=p, rs=1543, dt=o, ds=o, dm=o, df=o, arr=arr, hw=hw):
        return lib.tt_look_gather_query_bwd(B, qos, ref, dout, rs, dt, ds, dm, df, arr, hw, s)
    bad = [mb(B=0), mb(cs=320, coff=65), mb(cs=255), mb(coff=-1), mb(hw=hw0)]
    bad += [mb(**{k: None}) for k in ("v", "off", "lg", "ref", "hw", "dout", "dv", "do", "dl")]
    bad += [gb(B=0), gb(rs=1542), gb(hw=hw0)] + [gb(**{k: None}) for k in ("qos", "ref", "dout", "dt", "ds", "dm", "df", "arr", "hw")]
    bad += [lib.tt_sca_reduce_bwd(0, p, p, o, s), lib.tt_sca_reduce_bwd(B, None, p, o, s), lib.tt_sca_reduce_bwd(B, p, None, o, s),
            lib.tt_sca_reduce_bwd(B, p, p, None, s)]
    assert all(rc != 0 for rc in bad), [i for i, rc in enumerate(bad) if rc == 0]
    torch.cuda.synchronize()
    assert torch.equal(buf.buf.cpu(), buf.host0) and float(z.abs().sum()) == 0.0
