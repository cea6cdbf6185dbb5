"""Op-level parity of the forward glue kernels (csrc/elementwise.hip, csrc/dcn.hip) against float64 references on the CPU.

Every case checks four things (tests/glue_ref.py has the helpers and the tolerance rules): the values -- bit-equal to torch
f32 for data movement and single-rounding ops, otherwise within a measured limit of the float64 reference computed from the
values the device receives --, that nothing outside the output's rows and channel window is written (sentinel guard rows and
columns), that two runs are bit-identical, and that bad arguments come back as an error code before any launch.
The backward kernels are in test_glue_bwd.py."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import glue_ref as G  # noqa: E402
from glue_ref import Win, check, check_equal  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
DT_ID = {F32: "f32", BF16: "bf16", F16: "f16"}
CODE = {F32: 0, BF16: 1, F16: 2}
dt_param = pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])


def L():
    from thinktwice_amd import _lib
    return _lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(rc, what=""):
    assert rc == 0, f"{what} rc={rc}: {L().tt_last_error().decode()}"


def q(x, dt):
    """The f32 values of x as the device receives them in storage type dt."""
    return x.to(dt).float()


def twice(run):
    """run() allocates its buffers, launches and returns the written Win objects: two runs must be bit-identical."""
    a, b = run(), run()
    a = a if isinstance(a, (list, tuple)) else [a]
    b = b if isinstance(b, (list, tuple)) else [b]
    for wa, wb in zip(a, b):
        assert torch.equal(wa.buf, wb.buf), "two runs on the same inputs differ"
    return a if len(a) > 1 else a[0]


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def tie_data(shape, g):
    """Values from {0, 0, 0, 1, 2}: every 3 x 3 window has ties (a post-ReLU map); one window of -inf only when it fits."""
    x = torch.tensor([0.0, 0.0, 0.0, 1.0, 2.0])[torch.randint(0, 5, shape, generator=g)]
    if shape[1] > 2 and shape[2] > 2:
        x[0, :2, :2] = float("-inf")
    return x


# ----------------------------------------------------------------------------- max-pool
MP_F32 = [((2, 7, 10, 8), "7x10-odd-H-overhang"), ((1, 1, 1, 4), "1x1"), ((1, 2, 3, 4), "2x3"), ((1, 5, 5, 12), "5x5-C12")]
MP_16 = [((2, 7, 10, 8), "7x10-odd-H-overhang-C8"), ((1, 1, 1, 8), "1x1-C8"), ((1, 2, 3, 16), "2x3-C16"), ((1, 5, 5, 16), "5x5-C16")]
MP_CASES = [(F32, s, i) for s, i in MP_F32] + [(d, s, i) for d in (BF16, F16) for s, i in MP_16]


@pytest.mark.parametrize("dt,shape,cid", MP_CASES, ids=[f"{DT_ID[d]}-{i}" for d, _, i in MP_CASES])
def test_maxpool3x3s2_is_bit_equal_to_torch(dt, shape, cid):
    g = torch.Generator().manual_seed(sum(shape))
    N, H, W, C = shape
    x = tie_data(shape, g)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    want = nhwc(F.max_pool2d(nchw(x.double()), 3, 2, 1)).to(dt).reshape(-1, C)
    xd = x.to(dt).cuda()

    def run():
        out = Win(N * OH * OW, C, dtype=dt)
        ok(L().tt_maxpool3x3s2(xd.data_ptr(), out.ptr(), N, H, W, C, CODE[dt], st()))
        return out
    out = twice(run)
    check_equal("maxpool3x3s2", f"{DT_ID[dt]} {cid}", out.get(), want)
    out.untouched("maxpool3x3s2")


def test_vector_kernels_refuse_a_channel_count_off_the_vector_width():
    """C % 4 (f32) / C % 8 (16-bit) is required by the 16-byte-vector kernels: why their 16-bit cases use C = 8, 16, 24."""
    x = torch.zeros(64, device="cuda")
    for name in ("tt_maxpool3x3s2", "tt_bilinear_up2"):
        assert getattr(L(), name)(x.data_ptr(), x.data_ptr(), 1, 1, 1, 6, 0, st()) != 0
        assert getattr(L(), name)(x.data_ptr(), x.data_ptr(), 1, 1, 1, 12, 1, st()) != 0
    assert L().tt_upsample_nearest_add(x.data_ptr(), x.data_ptr(), 1, 1, 1, 12, 1, 1, 2, st()) != 0
    assert L().tt_channel_gate(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 1, 1, 4, 2, 0, 1, st()) != 0


# ----------------------------------------------------------------------------- nearest upsample + add
UP_SIZES = [(4, 6, 2, 3), (5, 7, 2, 3), (3, 3, 3, 3), (8, 2, 1, 1)]


@dt_param
@pytest.mark.parametrize("size", UP_SIZES, ids=[f"{H}x{W}-from-{h}x{w}" for H, W, h, w in UP_SIZES])
def test_upsample_nearest_add(dt, size):
    H, W, h, w = size
    N = 2
    for C in ((4, 12) if dt == F32 else (8, 24)):                       # 16-bit: 8 elements per vector
        g = torch.Generator().manual_seed(H * 100 + W + C)
        dst0, src = q(torch.randn(N, H, W, C, generator=g), dt), q(torch.randn(N, h, w, C, generator=g), dt)
        sd = src.to(dt).cuda()

        def run():
            dst = Win(N * H * W, C, dtype=dt, init=dst0)
            ok(L().tt_upsample_nearest_add(dst.ptr(), sd.data_ptr(), N, H, W, C, h, w, CODE[dt], st()))
            return dst
        dst = twice(run)
        case = f"{DT_ID[dt]} {H}x{W}<-{h}x{w} C={C}"
        if dt == F32:         # one add: bit-equal to torch's f32 of the same expression
            want = dst0 + nhwc(F.interpolate(nchw(src), size=(H, W), mode="nearest"))
            check_equal("upsample_nearest_add", case, dst.get(), want.reshape(-1, C))
        else:
            ref = dst0.double() + G.nearest_up(src.double(), H, W)
            check("upsample_nearest_add", case, dst.get(), ref.reshape(-1, C), rel=8 * G.U32, store=dt)
        dst.untouched("upsample_nearest_add")


# ----------------------------------------------------------------------------- bilinear x2, align_corners
BL_SIZES = [(1, 1, "1x1-sh0-sw0"), (1, 5, "1x5-sh0"), (3, 1, "3x1-sw0"), (2, 2, "2x2"), (3, 5, "3x5"), (16, 11, "16x11-two-blocks")]


def up2(x):
    return nhwc(F.interpolate(nchw(x), scale_factor=2, mode="bilinear", align_corners=True))


@dt_param
@pytest.mark.parametrize("H,W,cid", BL_SIZES, ids=[c for _, _, c in BL_SIZES])
def test_bilinear_up2(dt, H, W, cid):
    N = 2
    for C in ((4, 16) if dt == F32 else (16,)):
        g = torch.Generator().manual_seed(H * 31 + W + C)
        x = q(torch.randn(N, H, W, C, generator=g), dt)
        xd = x.to(dt).cuda()
        ref = up2(x.double()).reshape(-1, C)
        lim = G.f32_limit(up2(x).reshape(-1, C), ref)

        def run():
            out = Win(N * 4 * H * W, C, dtype=dt)
            ok(L().tt_bilinear_up2(xd.data_ptr(), out.ptr(), N, H, W, C, CODE[dt], st()))
            return out
        out = twice(run)
        check("bilinear_up2", f"{DT_ID[dt]} {cid} C={C}", out.get(), ref, rel=lim, store=dt)
        out.untouched("bilinear_up2")


@pytest.mark.parametrize("H,W,cid", BL_SIZES, ids=[c for _, _, c in BL_SIZES])
def test_bilinear_up2_pair_format_is_the_split_of_the_f32_result(H, W, cid):
    from thinktwice_amd import weights
    N = 2
    for C in (16, 32):
        g = torch.Generator().manual_seed(H * 17 + W + C)
        xd = torch.randn(N, H, W, C, generator=g).cuda()
        plain = Win(N * 4 * H * W, C)
        ok(L().tt_bilinear_up2(xd.data_ptr(), plain.ptr(), N, H, W, C, 0, st()))

        def run():
            out = Win(N * 4 * H * W, C)
            assert out.ptr() % 64 == 0
            ok(L().tt_bilinear_up2_pair(xd.data_ptr(), out.ptr(), N, H, W, C, st()))
            return out
        out = twice(run)
        want = weights.split_pairs_x3(plain.get().reshape(N, 2 * H, 2 * W, C))
        check_equal("bilinear_up2_pair", f"{cid} C={C}", out.get().view(torch.int32), want.reshape(-1, C).view(torch.int32))
        out.untouched("bilinear_up2_pair")
    assert L().tt_bilinear_up2_pair(xd.data_ptr(), xd.data_ptr(), 1, 1, 1, 8, st()) != 0        # C % 16


# ----------------------------------------------------------------------------- spatial pool (mean / mean+max)
HW_IDS = {1: "HW=1-three-idle-partitions", 3: "HW=3", 4: "HW=4-one-row-each", 5: "HW=5-tail-loop", 31: "HW=31-unrolled-in-3-partitions",
          32: "HW=32-unrolled-once-no-tail", 33: "HW=33-unrolled+tail", 61: "HW=61-unrolled+tail-of-7"}


@dt_param
@pytest.mark.parametrize("HW", list(HW_IDS), ids=list(HW_IDS.values()))
def test_spatial_pool(dt, HW):
    N = 2
    for C in (4, 64, 65, 100):                                   # one slab, a full slab, slab + 1 (`c < C`), a ragged second slab
        g = torch.Generator().manual_seed(HW * 7 + C)
        x = torch.randn(N, HW, C, generator=g)
        x[0, :, 0] = -x[0, :, 0].abs() - 1.0                     # an all-negative plane: the maximum must not start at 0
        x = q(x, dt)
        for mode, window in ((0, False), (0, True), (1, False)):  # the tape asserts a window for mode 0 only
            cs, coff = (C + 24, 8) if window else (C, 0)
            xin = Win(N * HW, C, cstride=cs, coff=coff, dtype=dt, init=x)

            def run():
                out = Win(N, C)
                ok(L().tt_spatial_pool(xin.ptr(), out.ptr(), N, HW, C, cs, coff, mode, CODE[dt], st()))
                return out
            out = twice(run)
            x64 = x.double()
            mean, amean = x64.mean(1), x64.abs().mean(1)
            if mode == 0:
                ref, bound = mean, G.sum_bound(amean, HW, 1)      # HW addends (4 partial sums joined), the division
            else:
                ref = 0.5 * mean + 0.5 * x64.amax(1)
                bound = G.sum_bound(0.5 * amean + 0.5 * x64.amax(1).abs(), HW, 2)      # + the final add
            check(f"spatial_pool mode {mode}", f"{DT_ID[dt]} HW={HW} C={C}{' window' if window else ''}", out.get(), ref, bound=bound)
            out.untouched("spatial_pool")
    z = torch.zeros(64, device="cuda")
    assert L().tt_spatial_pool(z.data_ptr(), z.data_ptr(), 1, 4, 0, 4, 0, 0, 0, st()) != 0         # C <= 0
    assert L().tt_spatial_pool(z.data_ptr(), z.data_ptr(), 1, 4, -4, 4, 0, 0, 0, st()) != 0
    assert L().tt_spatial_pool(z.data_ptr(), z.data_ptr(), 1, 4, 4, 6, 3, 0, 0, st()) != 0         # cstride < coff + C
    assert L().tt_spatial_pool(z.data_ptr(), z.data_ptr(), 1, 4, 4, 4, -1, 0, 0, st()) != 0


# ----------------------------------------------------------------------------- channel gate
@dt_param
@pytest.mark.parametrize("C", [0, 1, 2], ids=["C=4or8-one-vector", "C=64", "C=68or72-ragged"])
def test_channel_gate(dt, C):
    C = ((4, 64, 68) if dt == F32 else (8, 64, 72))[C]
    N = 2
    for HW in (1, 3, 5, 9):
        g = torch.Generator().manual_seed(HW * 13 + C)
        x, res = q(torch.randn(N, HW, C, generator=g), dt), q(torch.randn(N, HW, C, generator=g), dt)
        x[:, :, 0], res[:, :, 0] = 0.0, 0.0                       # x * s + res exactly 0
        gate = torch.randn(N, C, generator=g) * 2
        xd, rd, gd = x.to(dt).cuda(), res.to(dt).cuda(), gate.cuda()
        for gate_act in (G.ACT_SIGMOID, G.ACT_NONE):
            for out_act in (G.ACT_NONE, G.ACT_RELU):
                for use_res in (False, True):
                    def f(x_, g_, r_):
                        v = x_ * G.act_ref(g_, gate_act).unsqueeze(1)
                        return G.act_ref(v + r_ if use_res else v, out_act)
                    ref = f(x.double(), gate.double(), res.double()).reshape(-1, C)
                    lim = G.f32_limit(f(x, gate, res).reshape(-1, C), ref)

                    def run():
                        out = Win(N * HW, C, dtype=dt)
                        ok(L().tt_channel_gate(xd.data_ptr(), gd.data_ptr(), rd.data_ptr() if use_res else None, out.ptr(), N, HW, C,
                                               gate_act, out_act, CODE[dt], st()))
                        return out
                    out = twice(run)
                    case = f"{DT_ID[dt]} C={C} HW={HW} gate={G.ACT_NAMES[gate_act]} out={G.ACT_NAMES[out_act]} res={int(use_res)}"
                    check("channel_gate", case, out.get(), ref, rel=lim, store=dt)
                    out.untouched("channel_gate")


# ----------------------------------------------------------------------------- affine rows
@dt_param
@pytest.mark.parametrize("R,C", [(1, 1), (5, 7), (3, 300)], ids=["1x1", "5x7", "3x300-two-blocks"])
def test_affine_rows(dt, R, C):
    g = torch.Generator().manual_seed(R * 10 + C)
    x = q(torch.randn(R, C, generator=g) * 3, dt)
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    sd, hd = scale.cuda(), shift.cuda()
    xin = Win(R, C, cstride=C + 3, coff=1, dtype=dt, init=x)      # row-strided input and output
    for use_scale in (False, True):
        for use_shift in (False, True):
            for act in range(6):
                def f(x_, s_, h_):
                    v = x_ * s_ if use_scale else x_
                    return G.act_ref(v + h_ if use_shift else v, act)
                ref = f(x.double(), scale.double(), shift.double())
                lim = G.f32_limit(f(x, scale, shift), ref)

                def run():
                    out = Win(R, C, cstride=C + 5, coff=2, dtype=dt)
                    ok(L().tt_affine_rows(xin.wptr(), sd.data_ptr() if use_scale else None, hd.data_ptr() if use_shift else None,
                                          out.wptr(), R, C, C + 3, C + 5, act, CODE[dt], st()))
                    return out
                out = twice(run)
                check("affine_rows", f"{DT_ID[dt]} {R}x{C} scale={int(use_scale)} shift={int(use_shift)} {G.ACT_NAMES[act]}",
                      out.get(), ref, rel=lim, store=dt)
                out.untouched("affine_rows")


# ----------------------------------------------------------------------------- LayerNorm rows
LN_D = [(1, "D=1"), (5, "D=5"), (64, "D=64-one-pass"), (65, "D=65-second-pass-one-lane"), (256, "D=256"), (300, "D=300-ragged-fifth-pass")]
LN_R = [(1, "R=1"), (3, "R=3-partial-block"), (4, "R=4-one-block"), (5, "R=5"), (255, "R=255"), (256, "R=256"), (257, "R=257"), (600, "R=600")]
LN_CASES = [(5, D, i) for D, i in LN_D] + [(R, 65, i) for R, i in LN_R]


@dt_param
@pytest.mark.parametrize("R,D,cid", LN_CASES, ids=[i for _, _, i in LN_CASES])
def test_layernorm_rows(dt, R, D, cid):
    g = torch.Generator().manual_seed(R * 1000 + D)
    x = q(G.ln_rows(R, D, g), dt)
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.3
    gd, bd = gamma.cuda(), beta.cuda()
    xs, os_ = D + 3, D + 6                                        # columns >= D of the output rows are sentinel
    xin = Win(R, D, cstride=xs, dtype=dt, init=x)

    def run():
        out = Win(R, D, cstride=os_, dtype=dt)
        ok(L().tt_layernorm_rows(xin.ptr(), gd.data_ptr(), bd.data_ptr(), out.ptr(), R, D, xs, os_, 1e-5, CODE[dt], st()))
        return out
    out = twice(run)
    ref = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    check("layernorm_rows", f"{DT_ID[dt]} {cid}", out.get(), ref, bound=G.layernorm_bound(x.double(), gamma.double(), beta.double(), 1e-5),
          store=dt)
    out.untouched("layernorm_rows")


# ----------------------------------------------------------------------------- tt_ew
def ew_ref(op, act, a, b, g):
    v = (a + b, (1 - b) * a, (1 - g) * a + g * b, a)[op]
    return G.act_ref(v, act)


EW_ACTS = [G.ACT_NONE, G.ACT_RELU, G.ACT_SIGMOID, G.ACT_SOFTPLUS, G.ACT_SOFTPLUS_CLAMP, G.ACT_GELU]


@dt_param
@pytest.mark.parametrize("R,C", [(1, 1), (7, 5), (64, 96)], ids=["1x1", "7x5", "64x96-24-blocks"])
def test_ew_every_op_and_activation_in_row_strided_windows(dt, R, C):
    g = torch.Generator().manual_seed(R + C)
    a, b = q(torch.randn(R, C, generator=g) * 3, dt), q(torch.randn(R, C, generator=g) * 3, dt)
    gt = q(torch.rand(R, C, generator=g), dt)
    wa = Win(R, C, cstride=C + 3, coff=1, dtype=dt, init=a)       # every operand in its own window, a different coff each
    wb = Win(R, C, cstride=C + 5, coff=2, dtype=dt, init=b)
    wg = Win(R, C, cstride=C + 7, coff=3, dtype=dt, init=gt)
    for op in range(4):
        for act in EW_ACTS:
            def run():
                out = Win(R, C, cstride=C + 9, coff=4, dtype=dt)
                ok(L().tt_ew(wa.ptr(), wb.ptr() if op != 3 else None, wg.ptr() if op == 2 else None, out.ptr(), R, C, C + 3, 1,
                             C + 5, 2, C + 7, 3, C + 9, 4, op, act, CODE[dt], st()))
                return out
            out = twice(run)
            case = f"{DT_ID[dt]} {R}x{C} op{op} {G.ACT_NAMES[act]}"
            if dt == F32 and op in (0, 3) and act in (G.ACT_NONE, G.ACT_RELU):
                check_equal("ew", case, out.get(), ew_ref(op, act, a, b, gt))
            else:
                ref = ew_ref(op, act, a.double(), b.double(), gt.double())
                check("ew", case, out.get(), ref, rel=G.f32_limit(ew_ref(op, act, a, b, gt), ref), store=dt)
            out.untouched("ew")
    z = torch.zeros(8, device="cuda")
    assert L().tt_ew(z.data_ptr(), None, None, z.data_ptr(), 1, 1, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, st()) != 0      # op 0 without b
    assert L().tt_ew(z.data_ptr(), z.data_ptr(), None, z.data_ptr(), 1, 1, 1, 0, 1, 0, 1, 0, 1, 0, 2, 0, 0, st()) != 0   # op 2 without g
    assert L().tt_ew(z.data_ptr(), z.data_ptr(), None, z.data_ptr(), 1, 1, 1, 0, 1, 0, 1, 0, 1, 0, 4, 0, 0, st()) != 0   # op 4


def test_ew_above_the_forward_grid_cap():
    """R * C = 2049 * 1024 elements: 8,196 blocks of 256 against the 8,192-block cap, so the grid-stride loop takes a second trip."""
    R, C = 2049, 1024
    assert R * C > 8192 * 256 and (R * C + 255) // 256 > 8192
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g)
    ad, bd = a.cuda(), b.cuda()

    def run():
        out = Win(R, C)
        ok(L().tt_ew(ad.data_ptr(), bd.data_ptr(), None, out.ptr(), R, C, C, 0, C, 0, 0, 0, C, 0, 0, G.ACT_RELU, 0, st()))
        return out
    out = twice(run)
    check_equal("ew", "grid-cap 2049x1024 op0 relu", out.get(), torch.relu(a + b))
    out.untouched("ew")


# ----------------------------------------------------------------------------- concat rows
def _cat_arrays(pieces, coff):
    n = len(pieces)
    srcs = (ctypes.c_void_p * n)()
    strides, widths, coffs, divs, mods = ((ctypes.c_int * n)() for _ in range(5))
    c = coff
    for i, (src, stride, C, div, mod) in enumerate(pieces):
        srcs[i], strides[i], widths[i], coffs[i], divs[i], mods[i] = src, stride, C, c, div, mod
        c += C
    return srcs, strides, widths, coffs, divs, mods


def cat_call(out_ptr, R, out_stride, nseg, arrs):
    srcs, strides, widths, coffs, divs, mods = arrs
    return L().tt_concat_rows(out_ptr, R, out_stride, nseg, srcs, strides, widths, coffs, divs, mods, st())


CAT_R = 12
# (width, div, mod, has source): the decoder's mappings -- plain copy, a per-sample vector over 4 steps, a per-step embedding
CAT_CASES = {
    "1-piece-div1": [(5, 1, 0, True)],
    "3-pieces-div4-mod4-None": [(4, 4, 0, True), (3, 1, 4, True), (2, 1, 0, False)],
    "8-pieces-div2-mod3": [(1, 1, 0, True), (3, 2, 3, True), (2, 4, 0, True), (4, 1, 4, True), (1, 1, 0, False), (5, 1, 0, True),
                           (2, 2, 3, True), (3, 4, 0, True)],
}


def cat_rows_of(div, mod, R=CAT_R):
    r = torch.arange(R) // div
    return r % mod if mod else r


@pytest.mark.parametrize("cid", list(CAT_CASES), ids=list(CAT_CASES))
def test_concat_rows_is_bit_equal_to_torch(cid):
    g = torch.Generator().manual_seed(len(cid))
    spec = CAT_CASES[cid]
    total, coff = sum(s[0] for s in spec), 3                      # coff > 0, output stride > coff + total width
    srcs, want = [], []
    for C, div, mod, has in spec:
        rows = int(cat_rows_of(div, mod).max()) + 1
        if has:
            v = torch.randint(-9, 10, (rows, C), generator=g).float()
            srcs.append(Win(rows, C, cstride=C + 2, init=v))      # source stride > C
            want.append(v[cat_rows_of(div, mod)])
        else:
            srcs.append(None)
            want.append(torch.zeros(CAT_R, C))
    pieces = [(w.ptr() if w is not None else None, C + 2 if w is not None else 0, C, div, mod) for w, (C, div, mod, _) in zip(srcs, spec)]

    def run():
        out = Win(CAT_R, total, cstride=total + 9, coff=coff)
        ok(cat_call(out.ptr(), CAT_R, total + 9, len(pieces), _cat_arrays(pieces, coff)))
        return out
    out = twice(run)
    check_equal("concat_rows", cid, out.get(), torch.cat(want, 1))
    out.untouched("concat_rows")


def test_concat_rows_refuses_nine_pieces_and_gaps():
    z = torch.zeros(CAT_R * 32, device="cuda")
    nine = [(z.data_ptr(), 1, 1, 1, 0)] * 9
    assert cat_call(z.data_ptr(), CAT_R, 32, 9, _cat_arrays(nine, 0)) != 0
    two = [(z.data_ptr(), 2, 2, 1, 0)] * 2
    arrs = _cat_arrays(two, 0)
    arrs[3][1] = 3                                                # piece 1 starts one column after piece 0 ends
    assert cat_call(z.data_ptr(), CAT_R, 32, 2, arrs) != 0
    assert cat_call(z.data_ptr(), CAT_R, 3, 2, _cat_arrays(two, 0)) != 0        # pieces exceed the output row
    assert float(z.abs().sum()) == 0.0


# ----------------------------------------------------------------------------- broadcast rows
@dt_param
@pytest.mark.parametrize("N,HW,C", [(1, 1, 1), (3, 5, 7), (2, 441, 32)], ids=["1x1x1", "3x5x7", "2x441x32-111-blocks"])
def test_broadcast_rows_is_bit_equal(dt, N, HW, C):
    g = torch.Generator().manual_seed(N + HW + C)
    v = torch.randn(N, C, generator=g).to(dt)
    vin = Win(N, C, cstride=C + 3, coff=2, dtype=dt, init=v)      # strided v

    def run():
        out = Win(N * HW, C, cstride=C + 6, coff=5, dtype=dt)     # a window of the output
        ok(L().tt_broadcast_rows(vin.wptr(), out.ptr(), N, HW, C, C + 3, C + 6, 5, CODE[dt], st()))
        return out
    out = twice(run)
    check_equal("broadcast_rows", f"{DT_ID[dt]} {N}x{HW}x{C}", out.get(), v.unsqueeze(1).expand(N, HW, C).reshape(-1, C).contiguous())
    out.untouched("broadcast_rows")


# ----------------------------------------------------------------------------- copy_nhwc
COPY_PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16), (F32, F16), (F16, F32), (F16, F16)]


@pytest.mark.parametrize("di,do", COPY_PAIRS, ids=[f"{DT_ID[a]}-to-{DT_ID[b]}" for a, b in COPY_PAIRS])
def test_copy_nhwc_every_dtype_pair_with_windows_on_both_sides(di, do):
    N, H, W, C = 2, 3, 4, 5
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(N, H, W, C, generator=g) * 4).to(di)
    xin = Win(N * H * W, C, cstride=C + 3, coff=1, dtype=di, init=x)

    def run():
        out = Win(N * H * W, C, cstride=C + 5, coff=2, dtype=do)
        ok(L().tt_copy_nhwc(xin.ptr(), out.ptr(), N, H, W, C, C + 3, 1, C + 5, 2, 0, CODE[di], CODE[do], st()))
        return out
    out = twice(run)
    check_equal("copy_nhwc", f"{DT_ID[di]}->{DT_ID[do]}", out.get(), x.to(do).reshape(-1, C))
    out.untouched("copy_nhwc")


@pytest.mark.parametrize("S", [1, 2, 5], ids=["1x1", "2x2", "5x5"])
def test_copy_nhwc_rot_flip_is_rot90_of_flip(S):
    N, C = 2, 3
    g = torch.Generator().manual_seed(S)
    x = torch.randn(N, S, S, C, generator=g)
    xin = Win(N * S * S, C, cstride=C + 1, coff=1, init=x)

    def run():
        out = Win(N * S * S, C, cstride=C + 2, coff=0)
        ok(L().tt_copy_nhwc(xin.ptr(), out.ptr(), N, S, S, C, C + 1, 1, C + 2, 0, 1, 0, 0, st()))
        return out
    out = twice(run)
    want = nhwc(torch.rot90(torch.flip(nchw(x), dims=[2]), 1, dims=[2, 3])).reshape(-1, C).contiguous()
    check_equal("copy_nhwc rot_flip", f"{S}x{S}", out.get(), want)
    out.untouched("copy_nhwc")


def test_copy_nhwc_refuses_rot_flip_of_a_non_square_map_and_unknown_dtype_pairs():
    z = torch.zeros(64, device="cuda")
    assert L().tt_copy_nhwc(z.data_ptr(), z.data_ptr(), 1, 2, 3, 1, 1, 0, 1, 0, 1, 0, 0, st()) != 0
    assert L().tt_copy_nhwc(z.data_ptr(), z.data_ptr(), 1, 2, 2, 1, 1, 0, 1, 0, 0, 1, 2, st()) != 0      # bf16 -> f16
    assert float(z.abs().sum()) == 0.0


# ----------------------------------------------------------------------------- layout changes
@dt_param
@pytest.mark.parametrize("C,Cp", [(3, 8), (4, 4)], ids=["C3-padded-to-8", "C4-unpadded"])
def test_nchw_to_nhwc_pad_and_border(dt, C, Cp):
    N, H, W = 2, 3, 5
    g = torch.Generator().manual_seed(C)
    x = torch.randn(N, C, H, W, generator=g)
    xd = x.cuda()
    want = torch.zeros(N, H, W, Cp)
    want[..., :C] = nhwc(x)
    want = want.to(dt)

    def run():
        out = Win(N * H * W, Cp, dtype=dt)
        ok(L().tt_nchw_to_nhwc_pad(xd.data_ptr(), out.ptr(), N, C, H, W, Cp, CODE[dt], st()))
        return out
    out = twice(run)
    check_equal("nchw_to_nhwc_pad", f"{DT_ID[dt]} C={C}->{Cp}", out.get(), want.reshape(-1, Cp))
    out.untouched("nchw_to_nhwc_pad")
    # the interior of a spatially padded buffer: the border is the sentinel region
    Hp, Wp, top, left = H + 3, W + 4, 1, 2

    def run_b():
        out = Win(N * Hp * Wp, Cp, dtype=dt)
        ok(L().tt_nchw_to_nhwc_border(xd.data_ptr(), out.ptr(), N, C, H, W, Cp, Hp, Wp, top, left, CODE[dt], st()))
        return out
    outb = twice(run_b)
    exp = outb.host0.clone()
    inner = exp[:N * Hp * Wp].view(N, Hp, Wp, Cp)
    inner[:, top:top + H, left:left + W] = want
    check_equal("nchw_to_nhwc_border", f"{DT_ID[dt]} C={C}->{Cp}", outb.buf.cpu(), exp)
    z = torch.zeros(64, device="cuda")
    assert L().tt_nchw_to_nhwc_border(z.data_ptr(), z.data_ptr(), 1, 1, 2, 2, 1, 2, 3, 1, 0, 0, st()) != 0     # Hp < H + top
    assert L().tt_nchw_to_nhwc_pad(z.data_ptr(), z.data_ptr(), 1, 4, 2, 2, 3, 0, st()) != 0                    # Cp < C


@dt_param
def test_nhwc_to_nchw_from_a_channel_window(dt):
    N, H, W, C = 2, 3, 5, 6
    g = torch.Generator().manual_seed(8)
    x = torch.randn(N, H, W, C, generator=g).to(dt)
    xin = Win(N * H * W, C, cstride=C + 4, coff=3, dtype=dt, init=x)

    def run():
        out = Win(N * C, H * W)
        ok(L().tt_nhwc_to_nchw(xin.ptr(), out.ptr(), N, C, H, W, C + 4, 3, CODE[dt], st()))
        return out
    out = twice(run)
    check_equal("nhwc_to_nchw", DT_ID[dt], out.get(), nchw(x.float()).reshape(N * C, H * W).contiguous())
    out.untouched("nhwc_to_nchw")


# ----------------------------------------------------------------------------- deformable columns
def deform_offsets(kind, N, H, W, cs, g):
    if kind == "zero":
        return torch.zeros(N, H, W, cs)
    if kind == "integer":
        return torch.randint(-3, 4, (N, H, W, cs), generator=g).float()
    off = torch.randn(N, H, W, cs, generator=g) * 3               # many samples leave the map
    off[0, 0, 0, 0], off[0, 0, 0, 1] = 0.5, 1.25                  # tap 0 of pixel (0, 0): py = -0.5 in (-1, 0), px = 0.25
    off[0, 0, 0, 16], off[0, 0, 0, 17] = H - 1.5, -0.75           # tap 8: py = H - 0.5 in (H - 1, H), px = 0.25
    return off


def oracle_cols(x, off):
    from oracle import model_ref
    N, H, W, C = x.shape
    cols = model_ref.deform_im2col(nchw(x), nchw(off[..., :18]))             # (B,C,9,H,W)
    return cols.permute(0, 3, 4, 2, 1).reshape(N * H * W * 9, C)


DEF_CASES = [(1, 2, 2, 18), (2, 5, 7, 27), (2, 5, 7, 18)]


@dt_param
@pytest.mark.parametrize("kind", ["zero", "integer", "random"], ids=["zero-offsets", "integer-offsets", "random-offsets-3sigma"])
@pytest.mark.parametrize("N,H,W,cs", DEF_CASES, ids=[f"{n}x{h}x{w}-offstride{c}" for n, h, w, c in DEF_CASES])
def test_deform_im2col3x3(dt, kind, N, H, W, cs):
    for C in ((4, 8, 68, 132) if dt == F32 else (8, 72, 136)):
        g = torch.Generator().manual_seed(H * W + C + cs)
        x = q(torch.randn(N, H, W, C, generator=g), dt)
        off = deform_offsets(kind, N, H, W, cs, g)
        xd, od = x.to(dt).cuda(), off.cuda()

        def run():
            cols = Win(N * H * W * 9, C, dtype=dt)
            ok(L().tt_deform_im2col3x3(xd.data_ptr(), od.data_ptr(), cols.ptr(), N, H, W, C, cs, 1, CODE[dt], st()))
            return cols
        cols = twice(run)
        case = f"{DT_ID[dt]} {N}x{H}x{W} C={C} offstride={cs} {kind}"
        if kind == "zero":
            check_equal("deform_im2col3x3", case, cols.get(), G.im2col3x3_zero_pad(x).reshape(-1, C).to(dt))
        else:
            ref = oracle_cols(x.double(), off.double())
            check("deform_im2col3x3", case, cols.get(), ref, rel=G.f32_limit(oracle_cols(x, off), ref), store=dt)
            if kind == "random":
                s = G.deform_sample(x, off)
                assert float(s["py"][0, 0, 0, 0]) == -0.5 and float(s["py"][0, 0, 0, 8]) == H - 0.5
                assert bool((~s["inside"]).any()) and bool(s["inside"].any())
        cols.untouched("deform_im2col3x3")
    z = torch.zeros(64, device="cuda")
    for bad in [(0, 2, 2, 4, 18), (1, 0, 2, 4, 18), (1, 2, -1, 4, 18), (1, 2, 2, 0, 18), (1, 2, 2, -4, 18), (1, 2, 2, 4, 17), (1, 2, 2, 6, 18)]:
        n, h, w, c, s_ = bad
        assert L().tt_deform_im2col3x3(z.data_ptr(), z.data_ptr(), z.data_ptr(), n, h, w, c, s_, 1, 0, st()) != 0, bad
