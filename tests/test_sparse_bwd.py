"""Op-level parity of the sparse LiDAR encoder's backward: tt_sp_inverse_rulebook, tt_sp_to_dense / tt_sp_from_dense, the sparse input
gradient (ops.gather_conv_dgrad: the gathered GEMM over the transposed rulebook, accumulating in place) and tt_conv_epilogue_bwd with a
device row count, each against the float64 restatements of tests/sparse_ref.py.

As in tests/test_glue_bwd.py every gradient destination is a prefilled window with sentinel guard rows, `got - prefill` is compared at
the value tolerance plus one ulp of the prefill, rows beyond the live count must come back bit-unchanged, and every kernel runs
twice with bit-identical results.  The input-gradient cases pin the kernel they expect (KERNELS; tests/test_sparse_ref.py replays
the table through tt_conv2d_plan without a device)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sparse_ref as S  # noqa: E402
from glue_ref import PREFILL_ULP, U32, Win, check, check_equal, fit_scale, prefill, sum_bound, vjp  # noqa: E402
from test_glue_ops import L, ok, st, twice  # noqa: E402

pytestmark = pytest.mark.gpu


def delta(win):
    """What a kernel added to a prefilled window, in float64."""
    return win.get().double() - win.init().double()


def i32(v):
    return torch.tensor([v], dtype=torch.int32).cuda()


# ----------------------------------------------------------------------------- tt_sp_inverse_rulebook
# (rulebook of S.INVERSE_CASES, live rows: None = all of them, "over" = a device count above M, which clamps)
INVERSE = [("27 taps", None), ("27 taps pad 011", None), ("3 taps", None), ("27 taps", 0), ("27 taps", 1), ("3 taps", 1),
           ("27 taps", "over"), ("3 taps", "over")]


@pytest.mark.parametrize("name,live", INVERSE, ids=[f"{n}-live-{v}" for n, v in INVERSE])
def test_sp_inverse_rulebook_equals_the_reference(name, live):
    """Rows of nbr beyond the live count hold garbage (negative and far out of range) and must not be read; `inv` has 50 rows more
    than any index referenced, which stay -1, and two guard rows."""
    rb = S.case_rulebook(name)
    nbr, rows_in = rb["nbr"], rb["rows_in"]
    taps = nbr.shape[1]
    S.assert_inverse_unique(nbr, rows_in)
    g = torch.Generator().manual_seed(len(name))
    if live == "over":
        M, count = nbr.shape[0], nbr.shape[0] + 5000
        alloc = nbr.clone()
    else:
        count = nbr.shape[0] if live is None else live
        M = nbr.shape[0] + 29
        alloc = torch.where(torch.rand(M, taps, generator=g) < 0.5, torch.randint(-2 ** 31, 0, (M, taps), generator=g),
                            torch.randint(10 ** 6, 2 ** 31 - 1, (M, taps), generator=g)).to(torch.int32)
        alloc[:count] = nbr[:count]
    if live is None:
        assert (M * taps) % 256 != 0 and (count * taps) % 256 != 0
    rows = rows_in + 50
    want = torch.cat([S.inverse_rulebook(alloc, count, rows), torch.full((2, taps), -77, dtype=torch.int32)])
    nd, md = alloc.cuda(), i32(count)

    def run():
        inv = torch.full((rows + 2, taps), -1, dtype=torch.int32)
        inv[rows:] = -77
        inv = inv.cuda()
        ok(L().tt_sp_inverse_rulebook(nd.data_ptr(), md.data_ptr(), M, taps, inv.data_ptr(), st()), "tt_sp_inverse_rulebook")
        return inv.cpu()
    a, b = run(), run()
    assert torch.equal(a, b)
    check_equal("sp_inverse_rulebook", f"{name} live {count} of {M}", a, want)
    assert bool((a[rows_in:rows] == -1).all())
    if count >= nbr.shape[0]:          # and it is the transposed rulebook: every live entry is found again
        m, t = (nbr >= 0).nonzero(as_tuple=True)
        assert torch.equal(a[nbr[m, t].long(), t].long(), m)


# ----------------------------------------------------------------------------- tt_sp_to_dense / tt_sp_from_dense
DENSE_DIMS = (2, 2, 5, 7)                     # (B, D, H, W)


def dense_coords(live, spare, g):
    """`live` distinct cells in random order, then `spare` other cells (valid coordinates of cells no live row maps to: a kernel
    that read rows beyond the live count would show as non-zero cells / touched rows, never as an access outside the grid)."""
    B, D, H, W = DENSE_DIMS
    cells = torch.randperm(B * D * H * W, generator=g)[:live + spare]
    return torch.stack([cells // (D * H * W), cells // (H * W) % D, cells // W % H, cells % W], 1).to(torch.int32)


DENSE_CASES = [(3, 41), (128, 41), (3, 1), (128, 0)]       # (C, live rows)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C,live", DENSE_CASES, ids=[f"C{c}-live{n}" for c, n in DENSE_CASES])
def test_sp_to_dense_is_bit_equal(C, live, dt):
    from thinktwice_amd import ops
    B, D, H, W = DENSE_DIMS
    g = torch.Generator().manual_seed(C + live)
    max_rows = live + 5
    coords = dense_coords(live, 5, g)
    x = torch.randn(max_rows, C, generator=g).to(dt)
    want = S.sp_to_dense(x, coords, live, (D, H, W), B)
    xd, cd, rd = x.cuda(), coords.cuda(), i32(live)
    a = ops.sp_to_dense(xd, cd, rd, max_rows, (D, H, W), B).cpu()
    b = ops.sp_to_dense(xd, cd, rd, max_rows, (D, H, W), B).cpu()
    assert torch.equal(a, b)
    check_equal("sp_to_dense", f"C={C} live {live} of {max_rows} {str(dt).split('.')[-1]}", a, want)
    assert int((a != 0).sum()) <= live * C         # cells no live row maps to stay zero


@pytest.mark.parametrize("C,live", DENSE_CASES, ids=[f"C{c}-live{n}" for c, n in DENSE_CASES])
def test_sp_from_dense_accumulates_the_live_rows(C, live):
    from thinktwice_amd import ops
    B, D, H, W = DENSE_DIMS
    g = torch.Generator().manual_seed(C + live + 1)
    max_rows = live + 5
    coords = dense_coords(live, 5, g)
    gd = torch.rand(B, H, W, C * D, generator=g) * 8 - 4
    ref = S.sp_from_dense(gd.double(), coords, live, (D, H, W))
    P = prefill((max_rows, C), g)
    gdd, cd, rd = gd.cuda(), coords.cuda(), i32(live)

    def run():
        win = Win(max_rows, C, init=P)
        ops.sp_from_dense(gdd, cd, rd, max_rows, (D, H, W), win.buf[:max_rows])
        return win
    win = twice(run)
    check("sp_from_dense", f"C={C} live {live} of {max_rows}", delta(win)[:live], ref, slack=PREFILL_ULP)
    assert torch.equal(win.get()[live:], win.init()[live:]), "sp_from_dense wrote rows beyond the live count"
    win.untouched("sp_from_dense")


@pytest.mark.parametrize("C", [3, 128])
def test_sp_dense_pair_is_adjoint_on_integers(C):
    """<to_dense(x), g> == <x, from_dense(g)> exactly: small integers, so every product and sum is exact in f32 and in float64."""
    from thinktwice_amd import ops
    B, D, H, W = DENSE_DIMS
    live, max_rows = 41, 46
    g = torch.Generator().manual_seed(C)
    coords = dense_coords(live, 5, g)
    x = torch.randint(-8, 9, (max_rows, C), generator=g).float()
    gd = torch.randint(-8, 9, (B, H, W, C * D), generator=g).float()
    cd, rd = coords.cuda(), i32(live)
    dense = ops.sp_to_dense(x.cuda(), cd, rd, max_rows, (D, H, W), B).cpu()
    rows = torch.zeros(max_rows, C).cuda()
    ops.sp_from_dense(gd.cuda(), cd, rd, max_rows, (D, H, W), rows)
    lhs, rhs = float((dense.double() * gd.double()).sum()), float((x[:live].double() * rows.cpu()[:live].double()).sum())
    assert lhs == rhs and lhs != 0.0, (lhs, rhs)
    assert float(rows[live:].abs().max()) == 0.0


# ----------------------------------------------------------------------------- the sparse input gradient
# The kernel every case of S.DGRAD_CASES is expected to run on: (exact f32, bf16x3), the labels tt_conv2d_plan gives the launch of
# ops.gather_conv_dgrad (tests/test_sparse_ref.py::test_the_kernel_table_is_what_the_chooser_plans asserts them without a device).
F32_32, F32_64, F32_128 = (f"conv_igemm_kernel<float, 128, {n}>" for n in (32, 64, 128))      # the exact-f32 register-staged gather kernel
GLDS_32, GLDS_64 = (f"conv_igemm_glds_kernel<float, {n}, 8, 1, 128, 2, true, true>" for n in (32, 64))   # gathered LDS-DMA, bf16x3
KERNELS = {
    "subm 16->16": (F32_32, "sp_conv_runs_l2_kernel<16>"),
    "subm 32->32": (F32_32, "sp_conv_runs_kernel<1, 8, 1>"),
    "subm 64->64": (F32_64, "sp_conv_runs_kernel<2, 8, 1>"),
    "subm 128->128": (F32_128, "sp_conv_runs_kernel<2, 4, 2>"),
    "subm 8->16 input layer": (F32_32, F32_32),          # 8 output channels: no bf16x3 tile takes them, exact f32 in both modes
    "subm 32->32 small": (F32_32, F32_32),               # below 2048 rows: the small-M route is the exact-f32 kernel in both modes
    "s2 16->32": (F32_32, "sp_conv_runs_l2_kernel<32>"),
    "s2 32->64": (F32_32, GLDS_32),
    "s2p011 64->64": (F32_64, GLDS_64),
    "k311 64->128": (F32_64, GLDS_64),
}


def dgrad_desc(name, x3):
    """The descriptor of the gathered GEMM ops.gather_conv_dgrad launches for a case, with dummy addresses (host only)."""
    from thinktwice_amd import _lib, ops
    from tools import conv_choice_sweep as sweep
    _, Cin, Cout, _, _, _ = S.DGRAD_CASES[name]
    z = S.dgrad_sizes(name)
    M = z["in_alloc"]
    d = ops.conv_desc(x=1, x_shape=(z["out_alloc"], Cout), x_strides=None, w=1, w_shape=(Cin, 1, z["taps"], Cout), out=1, out_shape=(M, Cin),
                      out_strides=None, dtype=_lib.TT_F32, out_dtype=_lib.TT_F32, stride=2 if z["strided"] else 1, shift_n_mod=0,
                      res1=1, res1_shape=(M, Cin), weight_x3=1 if x3 else None, gather=(1, 1, M))
    return sweep.dict_to_desc(sweep.desc_to_dict(d))


def test_the_kernel_table_covers_every_family():
    x3 = " ".join(v[1] for v in KERNELS.values())
    assert "sp_conv_runs_kernel<" in x3 and "sp_conv_runs_l2_kernel<" in x3
    assert "conv_igemm_glds_kernel<float" in x3                                  # the generic gathered LDS-DMA kernel, bf16x3 weights
    assert all(v[0].startswith("conv_igemm_kernel<float") for v in KERNELS.values())   # exact f32: the register-staged gather kernel
    assert set(KERNELS) == set(S.DGRAD_CASES)


DGRAD = [(n, m) for n in S.DGRAD_CASES for m in ("f32", "x3")]


@pytest.mark.parametrize("name,mode", DGRAD, ids=[f"{n}-{m}" for n, m in DGRAD])
def test_sparse_input_gradient_matches_float64_autograd(name, mode):
    """ops.gather_conv_dgrad (what Tape.gather_conv's backward calls) into a prefilled gradient buffer.  bf16x3: within 1e-4 of
    max|ref|, the project's bound for bf16x3 at these K (tests/test_conv.py).  Exact f32: the summation bound with n = the live (tap,
    channel) addends of the row and k = 1 (the accumulator leaves the MFMA chain and is rounded once more when the epilogue adds the
    residual; the part of that rounding that belongs to the prefill is the slack).  dconv rows beyond the live count are NaN
    (uninitialised by contract), rulebook rows beyond it garbage."""
    from thinktwice_amd import ops
    _, Cin, Cout, _, _, _ = S.DGRAD_CASES[name]
    z, rb, R = S.dgrad_sizes(name), S.case_rulebook(name), S.dgrad_reference(name)
    x3 = mode == "x3"
    g = torch.Generator().manual_seed(len(name))
    nbr = torch.randint(-5, 10 ** 6, (z["out_alloc"], z["taps"]), generator=g, dtype=torch.int32)
    nbr[:z["live_out"]] = rb["nbr"]
    dconv = torch.full((z["out_alloc"], Cout), float("nan"))
    dconv[:z["live_out"]] = R["dconv"]
    P = prefill((z["in_alloc"], Cin), g)
    nd, dd, wd, m_out = nbr.cuda(), dconv.cuda(), R["w"].cuda(), i32(z["live_out"])
    in_rows = (i32(z["live_in"]), z["in_alloc"]) if z["strided"] else None
    labels = []

    def run(win=None):
        win = win or Win(z["in_alloc"], Cin, init=P)
        ops.gather_conv_dgrad(dd, nd, m_out, wd, win.buf[:z["in_alloc"]], in_rows, x3)
        labels.append(ops._last_conv_kernel())
        return win
    win = twice(run)
    assert labels[0] == labels[1] == KERNELS[name][x3], labels
    family = labels[0].split("<")[0]
    live = z["live_in"]
    kw = dict(rel=1e-4) if x3 else dict(bound=sum_bound(R["asum"], R["n"].unsqueeze(1).double(), 1))
    check(f"dgrad {mode} {family}", f"{name}: {labels[0]}", delta(win)[:live], R["ref"], slack=PREFILL_ULP, **kw)
    assert torch.equal(win.get()[live:], win.init()[live:]), f"{family} wrote rows beyond the live count"
    win.untouched(family)
    if name == "subm 32->32":       # accumulation: a second call into the same buffer adds the gradient a second time
        first = win.get().double()
        run(win)
        check(f"dgrad {mode} {family}", f"{name}: second call into the same buffer", win.get().double()[:live] - first[:live],
              R["ref"], slack=PREFILL_ULP, **kw)
        win.untouched(family)


# ----------------------------------------------------------------------------- tt_conv_epilogue_bwd as the sparse tape calls it
EPI_M, EPI_LIVE = 1531, 1237
EPI = [(C, act, res) for C in (16, 48, 128, 320) for act in (1, 0) for res in (True, False)]


@pytest.mark.parametrize("C,act,use_res", EPI, ids=[f"C{c}-{'relu' if a else 'none'}-{'res' if r else 'nores'}" for c, a, r in EPI])
def test_conv_epilogue_bwd_with_a_device_row_count(C, act, use_res):
    """conv_epilogue_bwd(gy, out, scale, shift, act, res, None, C=Cout, dres1=<prefilled gradient buffer>, m_dev=...): M = 1531 rows
    over 512 workgroups of three rows each, 1237 live, so 99 workgroups see no live row and must contribute zero partials.
    Pre-activations are at least 1e-3 away from 0 (the ReLU mask is unambiguous, no element is excluded).  dconv rows beyond the
    live count are uninitialised by contract and not compared; dres1 rows beyond it must be untouched.
    Summation depth of dshift / dscale, counted from the kernel: a thread adds ceil(3 / TY) rows, TY = 256 / min(C, 256) row lanes are
    added in order, the finish kernel adds 512 / 16 partials per lane and then its 16 lanes.  dscale's addend g * ((y - shift - res) /
    scale) carries the division and the product (k = 2) and the two subtractions' roundings, scaled by |g / scale|."""
    from thinktwice_amd import ops
    M, live = EPI_M, EPI_LIVE
    g = torch.Generator().manual_seed(C * 4 + act * 2 + use_res)
    pre = (torch.randn(M, C, generator=g).abs() + 1e-3) * (torch.randint(0, 2, (M, C), generator=g) * 2 - 1).float()
    y = torch.relu(pre) if act == 1 else pre
    scale = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    shift = torch.randn(C, generator=g) * 0.3
    res = torch.randn(M, C, generator=g) if use_res else None
    dy = torch.randn(M, C, generator=g)
    dy = dy * fit_scale(dy)
    r = res if use_res else torch.zeros(M, C)
    conv = ((pre.double() - shift.double() - r.double()) / scale.double())[:live]

    def fwd(cv, rs, sc, sh):
        v = cv * sc + sh + rs
        return torch.relu(v) if act == 1 else v
    dconv_ref, dres_ref, dscale_ref, dshift_ref = vjp(fwd, [conv, r[:live], scale, shift], dy[:live])
    gm = dres_ref                                                        # g = dy * act'(pre), float64
    TY = 256 // min(C, 256)
    depth = -(-3 // TY) + TY + 512 // 16 + 16
    sc64, sh64 = scale.double(), shift.double()
    t1 = (pre.double()[:live] - sh64).abs()
    recon = U32 * ((gm / sc64).abs() * (t1 + (pre.double()[:live] - sh64 - r.double()[:live]).abs())).sum(0)
    P = prefill((M, C), g)
    dyd, yd, scd, shd, md = dy.cuda(), y.cuda(), scale.cuda(), shift.cuda(), i32(live)
    rd = res.cuda() if use_res else None

    def run():
        win = Win(M, C, init=P) if use_res else None
        dconv, _, dscale, dshift = ops.conv_epilogue_bwd(dyd, yd, scd, shd, act, rd, None, C=C,
                                                         dres1=win.buf[:M] if use_res else None, m_dev=md)
        outs = [Win(live, C, init=dconv[:live].cpu(), guard=0), Win(1, C, init=dscale.cpu(), guard=0), Win(1, C, init=dshift.cpu(), guard=0)]
        return outs + ([win] if use_res else [])
    outs = twice(run)
    case = f"C={C} {'relu' if act else 'none'}{' res' if use_res else ''} live {live} of {M}"
    check("conv_epilogue_bwd dconv", case, outs[0].get(), dconv_ref, bound=sum_bound(dconv_ref.abs(), 1, 0))
    check("conv_epilogue_bwd dscale", case, outs[1].get()[0], dscale_ref, bound=sum_bound((gm * conv).abs().sum(0), depth, 2) + recon)
    check("conv_epilogue_bwd dshift", case, outs[2].get()[0], dshift_ref, bound=sum_bound(gm.abs().sum(0), depth, 0))
    if use_res:
        win = outs[3]
        check("conv_epilogue_bwd dres1", case, delta(win)[:live], gm, slack=PREFILL_ULP)
        assert torch.equal(win.get()[live:], win.init()[live:]), "conv_epilogue_bwd wrote dres1 rows beyond the live count"
        win.untouched("conv_epilogue_bwd dres1")
