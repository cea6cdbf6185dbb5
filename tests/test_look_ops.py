"""Op-level parity of the forward look-module kernels (csrc/look_module.hip) against the float64 restatements of tests/look_ref.py.

As in test_glue_ops.py every case checks the values (bit-equal where the kernel only moves data or the case is exact by
construction, otherwise one of glue_ref's two rules), that nothing outside the output's rows is written (sentinel guard rows),
that two launches are bit-identical, and that arguments the host code rejects come back as an error code with nothing written.
The backward kernels are in test_look_bwd.py."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import glue_ref as G  # noqa: E402
import look_ref as K  # noqa: E402
from glue_ref import Win, check, check_equal  # noqa: E402
from test_glue_ops import BF16, CODE, DT_ID, DTYPES, F16, F32, L, ok, st, twice  # noqa: E402,F401
from test_look_ref import PROJ_CASES, projection_case  # noqa: E402

pytestmark = pytest.mark.gpu

B_param = pytest.mark.parametrize("B", [1, 2, 3])
dt_param = pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
WINDOWS = [(256, 0), (320, 32), (512, 256)]
NAN = float("nan")
EPS = 1e-5
ISENT = -77


def dev(t):
    return t.contiguous().cuda()


class IntWin:
    """An int32 device buffer of n elements followed by 8 sentinel elements."""

    def __init__(self, n, fill=ISENT):
        self.n = n
        self.host0 = torch.full((n + 8,), ISENT, dtype=torch.int32)
        self.host0[:n] = fill
        self.buf = self.host0.cuda()

    def ptr(self):
        return self.buf.data_ptr()

    def get(self):
        return self.buf.cpu()[:self.n]

    def untouched(self, what=""):
        assert torch.equal(self.buf.cpu()[self.n:], self.host0[self.n:]), f"{what}: wrote past its end"


def level_args(maps):
    arr = (ctypes.c_void_p * 4)(*[m.data_ptr() for m in maps])
    hw = (ctypes.c_int * 8)(*[v for m in maps for v in (m.shape[1], m.shape[2])])
    return arr, hw


def hw_arg(level_hw):
    return (ctypes.c_int * 8)(*[v for pair in level_hw for v in pair])


# ----------------------------------------------------------------------------- tt_look_project_pack
@pytest.mark.parametrize("kind,seed", PROJ_CASES, ids=[f"{k}{s}" for k, s in PROJ_CASES])
@B_param
def test_look_project_pack(kind, seed, B):
    wp, l2i, ida, hw = projection_case(kind, seed, B)
    packed, qos, count, max_len, bound = K.project_pack_ref(wp, l2i, ida, hw)
    if kind == "random":
        assert int(K.ambiguous_points(wp, l2i, ida, hw).sum()) == 0
    wpd, ld, ad = dev(wp), dev(l2i), dev(ida)

    def run():
        ref, qs, cnt, ml = Win(B * 4 * 120, 2), IntWin(B * 4 * 120), IntWin(B * 4), IntWin(1, fill=999)
        ok(L().tt_look_project_pack(B, wpd.data_ptr(), ld.data_ptr(), ad.data_ptr(), float(hw[0]), float(hw[1]), ref.ptr(), qs.ptr(),
                                    cnt.ptr(), ml.ptr(), st()))
        return ref, qs, cnt, ml
    ref, qs, cnt, ml = twice(run)
    case = f"{kind}{seed} B={B}"
    check_equal("look_project_pack", case + " query_of_slot", qs.get(), qos.reshape(-1))
    check_equal("look_project_pack", case + " count", cnt.get(), count.reshape(-1))
    assert int(ml.get()[0]) == max_len                                             # reset by the call (it held 999), then the maximum
    got = ref.get()
    if kind == "random":
        check("look_project_pack", case + " ref_packed", got, packed.reshape(-1, 2), bound=bound.reshape(-1, 2))
    else:
        check_equal("look_project_pack", case + " ref_packed", got, packed.reshape(-1, 2).float())
    pad = (qos.reshape(-1) < 0)
    assert bool((qs.get()[pad] == -1).all()) and bool((got[pad] == 0).all())
    if kind == "degenerate":
        assert int(cnt.get().abs().sum()) == 0 and int(ml.get()[0]) == 0
    for w in (ref, qs, cnt, ml):
        w.untouched("look_project_pack")


# ----------------------------------------------------------------------------- tt_look_gather_query / tt_look_query_ln
STRIDES = [1543, 1544, 1552, 1799]


@functools.lru_cache(maxsize=None)
def gather_case(B, dt):
    """Inputs (f32; the maps rounded to dt on the host so that the reference reads what the device reads) and the references."""
    g = torch.Generator().manual_seed(20 + B)
    qos, ref, t, maps = K.gather_inputs(B, g, torch.float32)
    maps = [m.to(dt) for m in maps]
    t["ctrl_sp"] = torch.nn.functional.softplus(t["ctrl"])
    gamma, beta = torch.rand(1543, generator=g) + 0.5, torch.randn(1543, generator=g) * 0.3

    def rows(d, raw):
        c = t["ctrl"] if raw else t["ctrl_sp"]
        with torch.no_grad():
            return K.gather_query_ref(qos, ref.to(d), t["wp"].to(d), c.to(d), t["temporal"].to(d), t["static"].to(d), t["meas"].to(d),
                                      t["flat"].to(d), [m.to(d) for m in maps], raw_ctrl=raw)
    r = {(d, raw): rows(d, raw) for d in (torch.float64, torch.float32) for raw in (False, True)}
    return qos, ref, t, maps, gamma, beta, r


def gather_device(B, dt):
    qos, ref, t, maps, gamma, beta, _ = gather_case(B, dt)
    d = {k: dev(v) for k, v in t.items()}
    d.update(qos=dev(qos), ref=dev(ref), maps=[dev(m) for m in maps], gamma=dev(gamma), beta=dev(beta))
    return d


@dt_param
@B_param
def test_look_gather_query(B, dt):
    qos, ref, t, maps, _, _, r = gather_case(B, dt)
    d = gather_device(B, dt)
    arr, hw = level_args(d["maps"])
    r64, r32 = r[(torch.float64, False)], r[(torch.float32, False)]
    lim = G.f32_limit(r32[:, 519:], r64[:, 519:])
    R = B * 4 * 120
    for rs in STRIDES:
        def run():
            out = Win(R, rs)
            ok(L().tt_look_gather_query(B, d["qos"].data_ptr(), d["ref"].data_ptr(), d["wp"].data_ptr(), d["ctrl_sp"].data_ptr(),
                                        d["temporal"].data_ptr(), d["static"].data_ptr(), d["meas"].data_ptr(), d["flat"].data_ptr(),
                                        arr, hw, CODE[dt], out.ptr(), rs, st()))
            return out
        out = twice(run)
        got = out.get()
        case = f"B={B} {DT_ID[dt]} maps row_stride={rs}"
        check_equal("look_gather_query", case + " copied columns", got[:, :519].contiguous(), r32[:, :519].contiguous())
        check("look_gather_query", case + " sampled columns", got[:, 519:1543], r64[:, 519:], rel=lim)        # f32 output: no storage ulp
        assert bool((got[:, 1543:] == 0).all())                                    # the pad columns
        assert bool((got[qos.reshape(-1) < 0] == 0).all())
        out.untouched("look_gather_query")


@pytest.mark.parametrize("raw_ctrl", [0, 1], ids=["ctrl-softplus-given", "raw-ctrl"])
@dt_param
@B_param
def test_look_query_ln(B, dt, raw_ctrl):
    """LayerNorm(1543) of the gathered row.  Sum depth: every thread adds ceil(1543 / 256) = 7 elements, six butterfly steps, then
    the two-level sum of the four wave totals: 7 + 6 + 2 = 15 additions per addend.  The row itself carries the kernel's own
    error: the sampled columns the f32_limit of the gather, the four control columns 8 * 2^-24 (softplus) when raw_ctrl."""
    qos, ref, t, maps, gamma, beta, r = gather_case(B, dt)
    d = gather_device(B, dt)
    arr, hw = level_args(d["maps"])
    r64, r32 = r[(torch.float64, bool(raw_ctrl))], r[(torch.float32, bool(raw_ctrl))]
    e = torch.zeros(1, 1543, dtype=torch.float64)
    e[:, 519:] = G.f32_limit(r32[:, 519:], r64[:, 519:]) * float(r64[:, 519:].abs().max())
    if raw_ctrl:
        e[:, :4] = 8 * G.U32 * float(r64[:, :4].abs().max())
    want = K.layer_norm(r64, gamma.double(), beta.double(), EPS)
    bound = K.layernorm_bound_in(r64, e, gamma.double(), beta.double(), EPS, depth=15)
    R = B * 4 * 120
    cd = d["ctrl"] if raw_ctrl else d["ctrl_sp"]
    for rs in STRIDES:
        def run():
            out = Win(R, rs)
            ok(L().tt_look_query_ln(B, d["qos"].data_ptr(), d["ref"].data_ptr(), d["wp"].data_ptr(), cd.data_ptr(), raw_ctrl,
                                    d["temporal"].data_ptr(), d["static"].data_ptr(), d["meas"].data_ptr(), d["flat"].data_ptr(),
                                    arr, hw, CODE[dt], d["gamma"].data_ptr(), d["beta"].data_ptr(), EPS, out.ptr(), rs, st()))
            return out
        out = twice(run)
        got = out.get()
        check("look_query_ln", f"B={B} {DT_ID[dt]} maps row_stride={rs} raw_ctrl={raw_ctrl}", got[:, :1543], want, bound=bound)
        assert bool((got[:, 1543:] == 0).all())
        pad = qos.reshape(-1) < 0
        assert torch.equal(got[pad][:, :1543], beta.expand(int(pad.sum()), 1543))   # a zero row normalises to beta exactly
        out.untouched("look_query_ln")


# ----------------------------------------------------------------------------- tt_msda_sample / _strided / _ln
@functools.lru_cache(maxsize=None)
def msda_refs(name, B, dt):
    """The case with its value tensor rounded to dt on the host, the float64 reference and the f32 baseline."""
    c = dict(K.msda_case(name, B))
    if dt == F32:
        r64, r32 = K.msda_forward_refs(name, B)
        return c, r64, r32
    c["value"] = c["value"].to(dt).float()
    with torch.no_grad():
        r64 = K.msda_ref(c["value"].double(), c["offsets"].double(), c["logits"].double(), c["ref"].double(), c["level_hw"])
        r32 = K.msda_ref(c["value"], c["offsets"], c["logits"], c["ref"], c["level_hw"])
    return c, r64, r32


def windowed(value, cs, coff, dt=F32, fill=NAN):
    """value (BC,S,256) inside a (BC,S,cs) device tensor, every channel outside [coff, coff + 256) NaN."""
    wide = torch.full(value.shape[:2] + (cs,), fill)
    wide[..., coff:coff + 256] = value
    return wide.to(dt).cuda()


name_param = pytest.mark.parametrize("name", ["lattice", "random"])


@dt_param
@name_param
@B_param
def test_msda_sample(B, name, dt):
    c, r64, r32 = msda_refs(name, B, dt)
    lim = G.f32_limit(r32, r64)
    R = B * 4 * 120
    od, ld, rd, hw = dev(c["offsets"]), dev(c["logits"]), dev(c["ref"]), hw_arg(c["level_hw"])
    for cs, coff in WINDOWS:
        vd = windowed(c["value"], cs, coff, dt)

        def run():
            out = Win(R, 256)
            ok(L().tt_msda_sample_strided(B, vd.data_ptr(), CODE[dt], cs, coff, od.data_ptr(), ld.data_ptr(), rd.data_ptr(), hw,
                                          out.ptr(), st()))
            return out
        out = twice(run)
        check("msda_sample", f"{name} B={B} {DT_ID[dt]} cstride={cs} coff={coff}", out.get(), r64, rel=lim)
        out.untouched("msda_sample")
    vd = dev(c["value"].to(dt))
    out = Win(R, 256)                                                              # the unstrided entry point
    ok(L().tt_msda_sample(B, vd.data_ptr(), CODE[dt], od.data_ptr(), ld.data_ptr(), rd.data_ptr(), hw, out.ptr(), st()))
    check("msda_sample", f"{name} B={B} {DT_ID[dt]} plain entry", out.get(), r64, rel=lim)
    out.untouched("msda_sample")


@dt_param
@name_param
@B_param
def test_msda_sample_ln(B, name, dt):
    """The raw rows as tt_msda_sample; the normalised rows against the float64 LayerNorm of the raw rows the kernel wrote (its input,
    exactly).  Sum depth of a 256-row: one element per thread, six butterfly steps, the two-level sum of four wave totals: 8."""
    c, r64, r32 = msda_refs(name, B, dt)
    lim = G.f32_limit(r32, r64)
    R = B * 4 * 120
    g = torch.Generator().manual_seed(B)
    gamma, beta = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.3
    od, ld, rd, hw, gd, bd = dev(c["offsets"]), dev(c["logits"]), dev(c["ref"]), hw_arg(c["level_hw"]), dev(gamma), dev(beta)
    for cs, coff in WINDOWS:
        vd = windowed(c["value"], cs, coff, dt)

        def run():
            out, out_ln = Win(R, 256), Win(R, 256)
            ok(L().tt_msda_sample_ln(B, vd.data_ptr(), CODE[dt], cs, coff, od.data_ptr(), ld.data_ptr(), rd.data_ptr(), hw, gd.data_ptr(),
                                     bd.data_ptr(), EPS, out.ptr(), out_ln.ptr(), None, st()))
            return out, out_ln
        out, out_ln = twice(run)
        case = f"{name} B={B} {DT_ID[dt]} cstride={cs} coff={coff}"
        raw = out.get()
        check("msda_sample_ln", case + " raw", raw, r64, rel=lim)
        check("msda_sample_ln", case + " normalised", out_ln.get(), K.layer_norm(raw.double(), gamma.double(), beta.double(), EPS),
              bound=G.layernorm_bound(raw.double(), gamma.double(), beta.double(), EPS, depth=8))
        out.untouched("msda_sample_ln")
        out_ln.untouched("msda_sample_ln")


# ----------------------------------------------------------------------------- tt_msda_sample_proj_ln
@name_param
@B_param
def test_msda_sample_proj_ln(B, name):
    """Sample first, project after, against projecting every position and sampling then (float64); non-zero bias and
    (level, camera) shift, so a corner outside the map must take neither."""
    c = K.msda_case(name, B)
    g = torch.Generator().manual_seed(60 + B)
    maps = [torch.randn(B * 4, h, w, 256, generator=g) for h, w in c["level_hw"]]
    W = torch.randn(256, 256, generator=g) / 16
    bias, vshift = torch.randn(256, generator=g), torch.randn(4, 4, 256, generator=g)
    gamma, beta = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.3
    with torch.no_grad():
        r64 = K.msda_proj_ref([m.double() for m in maps], c["offsets"].double(), c["logits"].double(), c["ref"].double(), W.double(),
                              bias.double(), vshift.double())
        r32 = K.msda_proj_ref(maps, c["offsets"], c["logits"], c["ref"], W, bias, vshift)
    lim = G.f32_limit(r32, r64)
    R = B * 4 * 120
    md = [dev(m) for m in maps]
    arr, hw = level_args(md)
    od, ld, rd = dev(c["offsets"]), dev(c["logits"]), dev(c["ref"])
    wd, bd, sd, gd, ed = dev(W.t()), dev(bias), dev(vshift), dev(gamma), dev(beta)

    def run():
        out, out_ln = Win(R, 256), Win(R, 256)
        ok(L().tt_msda_sample_proj_ln(B, arr, hw, od.data_ptr(), ld.data_ptr(), rd.data_ptr(), wd.data_ptr(), bd.data_ptr(), sd.data_ptr(),
                                      gd.data_ptr(), ed.data_ptr(), EPS, out.ptr(), out_ln.ptr(), None, st()))
        return out, out_ln
    out, out_ln = twice(run)
    raw = out.get()
    check("msda_sample_proj_ln", f"{name} B={B} raw", raw, r64, rel=lim)
    check("msda_sample_proj_ln", f"{name} B={B} normalised", out_ln.get(), K.layer_norm(raw.double(), gamma.double(), beta.double(), EPS),
          bound=G.layernorm_bound(raw.double(), gamma.double(), beta.double(), EPS, depth=8))
    out.untouched("msda_sample_proj_ln")
    out_ln.untouched("msda_sample_proj_ln")


# ----------------------------------------------------------------------------- tt_sca_reduce / _ln
def max_lens(B):
    return [0, B - 1, B, B + 1, 64, 119, 120, 500]


def sca_rows(B, max_len, g):
    """Rows the reduction reads are random, every other row (slots < B, slots >= max_len) NaN."""
    x = torch.randn(B * 4, 120, 256, generator=g) * (torch.rand(B * 4, 120, 1, generator=g) * 3 + 0.2)
    slot = torch.arange(120).view(1, 120, 1)
    live = (slot >= B) & (slot < min(max_len, 120))
    return torch.where(live, x, torch.full_like(x, NAN)).reshape(-1, 256), torch.where(live, x, torch.zeros_like(x)).reshape(-1, 256)


@B_param
def test_sca_reduce(B):
    """n = min(max_len, 120) - B addends summed from zero, each divided by B first: k = 1."""
    for max_len in max_lens(B):
        g = torch.Generator().manual_seed(B * 1000 + max_len)
        x_nan, x0 = sca_rows(B, max_len, g)
        want = K.sca_reduce_ref(x0.double(), max_len, B)
        n = max(min(max_len, 120) - B, 0)
        bound = G.sum_bound(K.sca_reduce_ref(x0.double().abs(), max_len, B), n, 1)
        xd, ml = dev(x_nan), torch.tensor([max_len], dtype=torch.int32).cuda()

        def run():
            out = Win(B, 1024)
            ok(L().tt_sca_reduce(B, xd.data_ptr(), ml.data_ptr(), out.ptr(), st()))
            return out
        out = twice(run)
        check("sca_reduce", f"B={B} max_len={max_len}", out.get(), want, bound=bound)
        if max_len <= B:
            assert bool((out.get() == 0).all())
        out.untouched("sca_reduce")


@B_param
def test_sca_reduce_ln(B):
    """The reduction as above, then LayerNorm(1024) in one block of 1024 threads: one element per thread, six butterfly steps, the
    sixteen wave totals added in turn: depth 22.  The row carries the reduction's own summation bound."""
    for max_len in max_lens(B):
        g = torch.Generator().manual_seed(B * 1000 + max_len + 7)
        x_nan, x0 = sca_rows(B, max_len, g)
        gamma, beta = torch.rand(1024, generator=g) + 0.5, torch.randn(1024, generator=g) * 0.3
        red = K.sca_reduce_ref(x0.double(), max_len, B)
        n = max(min(max_len, 120) - B, 0)
        e = G.sum_bound(K.sca_reduce_ref(x0.double().abs(), max_len, B), n, 1)
        want = K.layer_norm(red, gamma.double(), beta.double(), EPS)
        bound = K.layernorm_bound_in(red, e, gamma.double(), beta.double(), EPS, depth=22)
        xd, ml, gd, bd = dev(x_nan), torch.tensor([max_len], dtype=torch.int32).cuda(), dev(gamma), dev(beta)

        def run():
            out = Win(B, 1024)
            ok(L().tt_sca_reduce_ln(B, xd.data_ptr(), ml.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, out.ptr(), st()))
            return out
        out = twice(run)
        check("sca_reduce_ln", f"B={B} max_len={max_len}", out.get(), want, bound=bound)
        if max_len <= B:
            assert torch.equal(out.get(), beta.expand(B, 1024))                    # an exactly zero row normalises to beta
        out.untouched("sca_reduce_ln")


# ----------------------------------------------------------------------------- tt_dec_merge_in
@pytest.mark.parametrize("B", [1, 3])
def test_dec_merge_in(B):
    """LayerNorm(1024) of [future flat | look | zeros | temporal | measurement].  Sum depth: a thread adds its four values in two
    levels (the squares one after the other: 4), six butterfly steps, the two-level sum of four wave totals: 4 + 6 + 2 = 12."""
    g = torch.Generator().manual_seed(70 + B)
    fflat, look, temporal, meas = (torch.randn(*s, generator=g) * 2 + 0.3 for s in ((B * 4, 256), (B, 256), (4, 128), (B, 128)))
    gamma, beta = torch.rand(1024, generator=g) + 0.5, torch.randn(1024, generator=g) * 0.3
    cat = K.merge_in_cat(fflat.double(), look.double(), temporal.double(), meas.double())
    want = K.layer_norm(cat, gamma.double(), beta.double(), EPS)
    bound = G.layernorm_bound(cat, gamma.double(), beta.double(), EPS, depth=12)
    fd, kd, td, md, gd, bd = (dev(t) for t in (fflat, look, temporal, meas, gamma, beta))

    def run():
        out = Win(B * 4, 1024)
        ok(L().tt_dec_merge_in(B, fd.data_ptr(), kd.data_ptr(), td.data_ptr(), md.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, out.ptr(), st()))
        return out
    out = twice(run)
    check("dec_merge_in", f"B={B}", out.get(), want, bound=bound)
    mean, var = cat.mean(1, keepdim=True), cat.var(1, unbiased=False, keepdim=True)
    zero_block = beta.double()[512:768] - mean / torch.sqrt(var + EPS) * gamma.double()[512:768]       # the input there is exactly zero
    check("dec_merge_in", f"B={B} zero block", out.get()[:, 512:768], zero_block, bound=bound[:, 512:768])
    out.untouched("dec_merge_in")


# ----------------------------------------------------------------------------- error codes
def test_look_entry_points_refuse_bad_arguments_before_any_launch():
    """Only arguments the host code is read to reject (TT_REQUIRE before the launch): a null pointer for a checked argument, a row
    stride outside [1543, 1799], a channel window outside the row, B <= 0, a level with H or W < 1.  Nothing is written."""
    B, R = 1, 480
    buf = Win(R, 1799)                                           # large enough for every output of every call below
    z = torch.zeros(R * 1799 + 4096, device="cuda")
    p, o = z.data_ptr(), buf.ptr()
    maps = [torch.zeros(4, h, w, 256, device="cuda") for h, w in K.GQ_HW]
    arr, hw = level_args(maps)
    hw0 = (ctypes.c_int * 8)(5, 7, 3, 0, 2, 3, 1, 1)
    s = st()
    lib = L()
    bad = []

    def gq(B=B, qos=p, ref=p, wp=p, ctrl=p, te=p, se=p, me=p, fl=p, arr=arr, hw=hw, out=o, rs=1544):
        return lib.tt_look_gather_query(B, qos, ref, wp, ctrl, te, se, me, fl, arr, hw, 0, out, rs, s)

    def ql(B=B, qos=p, ref=p, wp=p, ctrl=p, te=p, se=p, me=p, fl=p, arr=arr, hw=hw, ga=p, be=p, out=o, rs=1544):
        return lib.tt_look_query_ln(B, qos, ref, wp, ctrl, 0, te, se, me, fl, arr, hw, 0, ga, be, EPS, out, rs, s)
    for f in (gq, ql):
        bad += [f(rs=1542), f(rs=1800), f(B=0), f(B=-1), f(hw=hw0)]
        bad += [f(**{k: None}) for k in ("qos", "ref", "wp", "ctrl", "te", "se", "me", "fl", "arr", "hw", "out")]
    bad += [ql(ga=None), ql(be=None)]

    def ms(B=B, v=p, cs=256, coff=0, off=p, lg=p, ref=p, hw=hw, out=o):
        return lib.tt_msda_sample_strided(B, v, 0, cs, coff, off, lg, ref, hw, out, s)

    def ml(B=B, v=p, cs=256, coff=0, off=p, lg=p, ref=p, hw=hw, ga=p, be=p, out=o, out_ln=o):
        return lib.tt_msda_sample_ln(B, v, 0, cs, coff, off, lg, ref, hw, ga, be, EPS, out, out_ln, None, s)
    for f in (ms, ml):
        bad += [f(cs=320, coff=65), f(cs=255), f(coff=-1), f(cs=512, coff=257), f(B=0), f(hw=hw0)]
        bad += [f(**{k: None}) for k in ("v", "off", "lg", "ref", "hw", "out")]
    bad += [ml(ga=None), ml(be=None), ml(out_ln=None)]
    bad += [lib.tt_msda_sample(B, None, 0, p, p, p, hw, o, s), lib.tt_msda_sample(0, p, 0, p, p, p, hw, o, s)]

    def pl(B=B, arr=arr, hw=hw, off=p, lg=p, ref=p, w=p, bi=p, vs=p, ga=p, be=p, out=o, out_ln=o):
        return lib.tt_msda_sample_proj_ln(B, arr, hw, off, lg, ref, w, bi, vs, ga, be, EPS, out, out_ln, None, s)
    bad += [pl(B=0), pl(hw=hw0)] + [pl(**{k: None}) for k in ("arr", "hw", "off", "lg", "ref", "w", "bi", "vs", "ga", "be", "out", "out_ln")]
    def pp(B=B, wp=p, l2i=p, ida=p, ref=o, qos=p, cnt=p, ml=p):
        return lib.tt_look_project_pack(B, wp, l2i, ida, 128.0, 256.0, ref, qos, cnt, ml, s)
    bad += [pp(B=0)] + [pp(**{k: None}) for k in ("wp", "l2i", "ida", "ref", "qos", "cnt", "ml")]
    bad += [lib.tt_sca_reduce(0, p, p, o, s), lib.tt_sca_reduce(-2, p, p, o, s), lib.tt_sca_reduce(B, None, p, o, s),
            lib.tt_sca_reduce(B, p, None, o, s), lib.tt_sca_reduce(B, p, p, None, s)]
    bad += [lib.tt_sca_reduce_ln(0, p, p, p, p, EPS, o, s), lib.tt_sca_reduce_ln(B, None, p, p, p, EPS, o, s),
            lib.tt_sca_reduce_ln(B, p, None, p, p, EPS, o, s), lib.tt_sca_reduce_ln(B, p, p, None, p, EPS, o, s),
            lib.tt_sca_reduce_ln(B, p, p, p, None, EPS, o, s), lib.tt_sca_reduce_ln(B, p, p, p, p, EPS, None, s)]
    def mi(B=B, ff=p, lk=p, te=p, me=p, ga=p, be=p, out=o):
        return lib.tt_dec_merge_in(B, ff, lk, te, me, ga, be, EPS, out, s)
    bad += [mi(B=0)] + [mi(**{k: None}) for k in ("ff", "lk", "te", "me", "ga", "be", "out")]
    assert all(rc != 0 for rc in bad), [i for i, rc in enumerate(bad) if rc == 0]
    assert len(lib.tt_last_error()) > 0
    torch.cuda.synchronize()
    assert torch.equal(buf.buf.cpu(), buf.host0) and float(z.abs().sum()) == 0.0
