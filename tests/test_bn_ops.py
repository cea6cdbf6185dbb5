"""Op-level parity of train-mode BatchNorm (csrc/batchnorm.hip) through the C ABI: every case runs tt_bn_stats ->
tt_bn_finalize -> tt_bn_apply -> tt_bn_bwd_reduce -> tt_bn_bwd_apply and holds every output to the float64 references of
tests/step_ref.py within bounds counted from the kernels' roundings (test_step_ref.py pins those references to torch).

The cases (step_ref.BN_CASES) are the smallest shapes that reach each launch arm and loop shape: the scalar kernels by channel
count and by one misaligned tensor at a time, the 16-byte kernels with every tensor in its own channel window, one / two /
25+ / 512 workgroups per group, a device row count from 0 to past the allocation, the guards of bn_finalize_kernel, and
columns whose one-pass variance is badly conditioned.  Every written tensor lies in a guarded window that must stay intact
around it, the workspace starts as NaN (an unwritten partial would show), and two runs must agree bit for bit: the file
documents a fixed summation order."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_ref as S  # noqa: E402
from glue_ref import PREFILL_ULP, SENT, Win, check, check_equal, prefill  # noqa: E402
from test_glue_ops import L, ok, st, twice  # noqa: E402

pytestmark = pytest.mark.gpu

TENSORS = ("z", "out", "res1", "res2", "dy", "y", "dres1", "dres2", "dz")
# the launches a tensor is an argument of (dy is bn_bwd_apply's g)
USED_BY = {"z": {"stats", "apply", "bwd_reduce", "bwd_apply"}, "out": {"apply"}, "res1": {"apply"}, "res2": {"apply"},
           "dy": {"bwd_reduce", "bwd_apply"}, "y": {"bwd_reduce"}, "dres1": {"bwd_reduce"}, "dres2": {"bwd_reduce"},
           "dz": {"bwd_apply"}}
LEAD = 64            # sentinel floats in front of every window buffer (a multiple of 4: keeps the 16-byte alignment)


class SWin(Win):
    """glue_ref.Win inside a flat buffer [LEAD + shift sentinels | rows | guard rows | 8 sentinels]: `shift` = 1 places row 0
    one float past a 16-byte boundary; untouched() also covers the floats in front and behind."""

    def __init__(self, R, C, cstride=None, coff=0, init=None, guard=2, shift=0):
        self.R, self.C, self.cs, self.coff, self.shift = R, C, cstride or C, coff, shift
        host = torch.full((R + guard, self.cs), SENT)
        if init is not None:
            host[:R, coff:coff + C] = init.reshape(R, C).float()
        self.host0 = host.clone()
        self.lead = LEAD + shift
        flat = torch.full((self.lead + host.numel() + 8,), SENT)
        flat[self.lead:self.lead + host.numel()] = host.reshape(-1)
        self.flat = flat.cuda()
        self.buf = self.flat[self.lead:self.lead + host.numel()].view(R + guard, self.cs)
        assert self.buf.data_ptr() % 16 == 4 * shift

    def untouched(self, what=""):
        super().untouched(what)
        flat = self.flat.cpu()
        assert bool((flat[:self.lead] == SENT).all()) and bool((flat[-8:] == SENT).all()), f"{what}: wrote around its buffer"


class Flat:
    """n device elements followed by 8 sentinels."""

    def __init__(self, n, dtype=torch.float32, init=None):
        host = torch.full((n + 8,), SENT, dtype=dtype)
        if init is not None:
            host[:n] = init.reshape(-1).to(dtype)
        self.n, self.buf = n, host.cuda()

    def ptr(self):
        return self.buf.data_ptr()

    def get(self):
        return self.buf.cpu()[:self.n]

    def untouched(self, what=""):
        assert bool((self.buf.cpu()[self.n:] == SENT).all()), f"{what}: wrote past its end"


def layout(c):
    """(cstride, coff, shift) of every tensor: each in a window of its own (cstride != C, coff != 0), offsets and strides
    multiples of 4 where the channel count allows the 16-byte kernels, arbitrary otherwise; then the one tensor a
    misalignment case moves."""
    C, lay = c.C, {}
    for k, t in enumerate(TENSORS):
        if C % 4 == 0:
            coff = 4 * (1 + k % 2)
            lay[t] = (C + coff + 4 * (k % 3), coff, 0)
        else:
            coff = 1 + 2 * (k % 2)
            lay[t] = (C + coff + k % 3, coff, 0)
    if isinstance(c.lay, tuple):
        t, how = c.lay
        cs, coff, _ = lay[t]
        lay[t] = {"shift": (cs, coff, 1), "coff": (cs + 4, coff + 1, 0), "cstride": (cs + 1, coff, 0)}[how]
    return lay


def vec_ok(C, wins, flats):
    """bn_vec_ok restated: the 16-byte kernels need C % 4 == 0, every base pointer on a 16-byte boundary and every stride
    and offset a multiple of 4."""
    wins = [w for w in wins if w is not None]
    return (C % 4 == 0 and all(w.ptr() % 16 == 0 and w.cs % 4 == 0 and w.coff % 4 == 0 for w in wins)
            and all(f.ptr() % 16 == 0 for f in flats))


def run_case(c, d):
    M, C, G = c.M, c.C, c.groups
    lay = layout(c)
    lib = L()
    w = {}

    def win(t, init=None):
        cs, coff, shift = lay[t]
        w[t] = SWin(M, C, cs, coff, init=init, shift=shift)
        return w[t]

    z = win("z", d["z"])
    res = [win(f"res{i + 1}", r) for i, r in enumerate(d["res"])] + [None] * (2 - c.nres)
    out, dy, dz = win("out"), win("dy", d["dy"]), win("dz")
    dres = [win(f"dres{i + 1}", d["P"][i]) for i in range(c.nres)] + [None] * (2 - c.nres)
    m_dev = None if c.live is None else torch.tensor([c.live], dtype=torch.int32).cuda()
    mp = None if m_dev is None else m_dev.data_ptr()
    ws_bytes = lib.tt_bn_workspace_bytes(C, G)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8).cuda()             # every partial starts as a NaN
    stats, sums = Flat(G * (2 * C + 2), torch.float64), Flat(G * 2 * C, torch.float64)
    scale, shift, mean, invstd = (Flat(G * C) for _ in range(4))
    gamma = None if d["gamma"] is None else Flat(C, init=d["gamma"])
    beta = None if d["beta"] is None else Flat(C, init=d["beta"])
    rm = None if d["rm"] is None else Flat(C, init=d["rm"])
    rv = None if d["rv"] is None else Flat(C, init=d["rv"])
    P = lambda x: None if x is None else x.ptr()
    CS = lambda x: 0 if x is None else x.cs
    CO = lambda x: 0 if x is None else x.coff

    ok(lib.tt_bn_stats(z.ptr(), M, C, z.cs, z.coff, mp, G, stats.ptr(), ws.data_ptr(), ws_bytes, st()), "tt_bn_stats")
    ok(lib.tt_bn_finalize(stats.ptr(), C, G, P(gamma), P(beta), c.eps, c.momentum, P(rm), P(rv), scale.ptr(), shift.ptr(),
                          mean.ptr(), invstd.ptr(), st()), "tt_bn_finalize")
    ok(lib.tt_bn_apply(z.ptr(), M, C, z.cs, z.coff, mp, G, scale.ptr(), shift.ptr(), mean.ptr(), P(res[0]), CS(res[0]), CO(res[0]),
                       P(res[1]), CS(res[1]), CO(res[1]), c.act, out.ptr(), out.cs, out.coff, st()), "tt_bn_apply")
    y = win("y", out.get())                          # the forward's output, handed over in a buffer with its own stride
    ws.fill_(0xFF)
    ok(lib.tt_bn_bwd_reduce(dy.ptr(), dy.cs, dy.coff, y.ptr(), y.cs, y.coff, z.ptr(), z.cs, z.coff, M, C, mp, G, mean.ptr(),
                            invstd.ptr(), c.act, P(dres[0]), CS(dres[0]), CO(dres[0]), P(dres[1]), CS(dres[1]), CO(dres[1]),
                            sums.ptr(), ws.data_ptr(), ws_bytes, st()), "tt_bn_bwd_reduce")
    ok(lib.tt_bn_bwd_apply(dy.ptr(), dy.cs, dy.coff, z.ptr(), z.cs, z.coff, M, C, mp, G, sums.ptr(), stats.ptr(), scale.ptr(),
                           mean.ptr(), invstd.ptr(), dz.ptr(), dz.cs, dz.coff, st()), "tt_bn_bwd_apply")
    torch.cuda.synchronize()
    arms = {"stats": vec_ok(C, [z], []),
            "apply": vec_ok(C, [z, res[0], res[1], out], [scale, shift, mean]),
            "bwd_reduce": vec_ok(C, [dy, y, z, dres[0], dres[1]], [mean, invstd]),
            "bwd_apply": vec_ok(C, [dy, z, dz], [scale, mean, invstd])}
    flats = dict(stats=stats, sums=sums, scale=scale, shift=shift, mean=mean, invstd=invstd, rm=rm, rv=rv)
    return dict(w=w, f=flats, arms={k: "vec" if v else "scalar" for k, v in arms.items()})


def bits(t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


@pytest.mark.parametrize("c", S.BN_CASES, ids=[c.id for c in S.BN_CASES])
def test_batchnorm_train_forward_and_backward(c):
    M, C, G = c.M, c.C, c.groups
    d = S.bn_case_data(c)
    d["P"] = [prefill((M, C), torch.Generator().manual_seed(77 + i)) for i in range(c.nres)]
    outs = []

    def run():
        r = run_case(c, d)
        outs.append(r)
        return [x for x in list(r["w"].values()) + list(r["f"].values()) if x is not None]
    if c.data == "bad":                              # NaN results: compared as bits
        a, b = run(), run()
        assert all(torch.equal(bits(x.buf), bits(y.buf)) for x, y in zip(a, b)), "two runs on the same inputs differ"
    else:
        twice(run)
    r = outs[0]
    w, fl, arms = r["w"], r["f"], r["arms"]

    # the arm every launch took, by the restated rule
    if c.arm in ("vec", "scalar"):
        assert set(arms.values()) == {c.arm}, arms
    else:
        assert {k for k, v in arms.items() if v == "scalar"} == USED_BY[c.lay[0]], arms

    z = d["z"].double()
    f = S.bn_forward_ref(z, d["gamma"], d["beta"], c.eps, c.momentum, d["rm"], d["rv"], G, c.live, d["res"], c.act)
    d_fwd = S.bn_sum_depth(M, C, G, c.live, arms["stats"] == "vec")
    d_bwd = S.bn_sum_depth(M, C, G, c.live, arms["bwd_reduce"] == "vec")
    fb = S.bn_forward_bounds(z, f, d["res"], depth=d_fwd)
    n_live = f["rows"][-1][1]
    good = torch.ones(C, dtype=torch.bool)
    if c.data == "bad":
        good[2] = good[5] = False
    case = c.id

    # tt_bn_stats: the f64 sums (each addend through at most n additions), the row count
    stats = fl["stats"].get().view(G, 2 * C + 2)
    nn = torch.tensor([float(n) for n in f["n"]], dtype=torch.float64).view(G, 1)
    dd = nn.clamp(max=d_fwd)                         # additions an addend passes through (step_ref.bn_sum_depth)
    s1 = torch.stack([z[a:b].sum(0) for a, b in f["rows"]])
    s2 = torch.stack([(z[a:b] ** 2).sum(0) for a, b in f["rows"]])
    a1 = torch.stack([z[a:b].abs().sum(0) for a, b in f["rows"]])
    nb = S.bn_launch_blocks(M, G)                    # workgroups per group = partial rows bn_finish_kernel adds
    kern = f"bn_stats {arms['stats']} finish nb{'<25' if nb < 25 else '=512' if nb == 512 else '>=25'}"
    check(kern, case + " sum", stats[:, :C][:, good], s1[:, good], bound=(dd * S.U64 * a1 + S.TINY)[:, good])
    check(kern, case + " sum of squares", stats[:, C:2 * C][:, good], s2[:, good], bound=(dd * S.U64 * s2 + S.TINY)[:, good])
    check_equal("bn_finish row count", case, stats[:, 2 * C:], torch.cat([nn, torch.zeros(G, 1, dtype=torch.float64)], 1))

    # tt_bn_finalize
    for name in ("mean", "invstd", "scale"):
        got = fl[name].get().view(G, C)
        assert bool(torch.isfinite(got[:, good]).all()), name
        check("bn_finalize " + name, case, got[:, good], f[name][:, good], bound=fb[name][:, good])
    check_equal("bn_finalize shift", case, fl["shift"].get().view(G, C), f["shift"].float().expand(G, C).contiguous())
    if c.running:
        for name, key, init in (("running_mean", "rm", d["rm"]), ("running_var", "rv", d["rv"])):
            got = fl[key].get()
            if n_live == 0:                          # nothing to apply: bit-unchanged
                check_equal("bn_finalize " + name, case + " no live row", got, init)
                continue
            check("bn_finalize " + name, case, got[good], f[name][good], bound=fb[name][good])
            if not bool(good.all()):                 # a non-finite statistic must not reach the running buffers
                check_equal("bn_finalize " + name, case + " guarded channels", got[~good], init[~good])

    # tt_bn_apply
    out = w["out"].get()
    check(f"bn_apply {arms['apply']}", case, out[:n_live][:, good], f["out"][:n_live][:, good], bound=fb["out"][:n_live][:, good])
    assert bool((out[n_live:] == SENT).all()), "tt_bn_apply wrote a row past the device row count"
    if c.data == "const" and c.nres == 0 and c.act == S.ACT_NONE:
        check_equal(f"bn_apply {arms['apply']}", case + " constant column returns beta", out[:, 0], d["beta"][0].expand(M).contiguous())

    # backward, from the y the device wrote
    b = S.bn_backward_ref(d["dy"], out.double(), z, f, c.act)
    bb = S.bn_backward_bounds(z, f, fb, b, depth=d_bwd)
    check_equal(f"bn_bwd_reduce {arms['bwd_reduce']} g", case, w["dy"].get()[:, good], b["g"].float()[:, good])
    for i in range(c.nres):
        got = w[f"dres{i + 1}"].get()
        check(f"bn_bwd_reduce {arms['bwd_reduce']} dres", case + f" dres{i + 1}", (got.double() - d["P"][i].double())[:n_live][:, good],
              b["dres"][:n_live][:, good], slack=PREFILL_ULP)
        assert torch.equal(got[n_live:], d["P"][i][n_live:]), "tt_bn_bwd_reduce touched a row past the device row count"
    sums = fl["sums"].get().view(G, 2 * C)
    check(f"bn_bwd_reduce {arms['bwd_reduce']} sum g", case, sums[:, :C][:, good], b["sg"][:, good], bound=bb["sg"][:, good])
    check(f"bn_bwd_reduce {arms['bwd_reduce']} sum g xhat", case, sums[:, C:][:, good], b["sgx"][:, good], bound=bb["sgx"][:, good])
    dz = w["dz"].get()
    check(f"bn_bwd_apply {arms['bwd_apply']}", case, dz[:n_live][:, good], b["dz"][:n_live][:, good], bound=bb["dz"][:n_live][:, good])
    assert bool((dz[n_live:] == SENT).all()), "tt_bn_bwd_apply wrote a row past the device row count"
    if M == 1:                                       # one row: xhat = 0 and g - sum g = 0, exactly
        assert bool((dz == 0).all())
        assert torch.equal(fl["rv"].get(), ((1.0 - torch.tensor(c.momentum)) * d["rv"]).float())    # + momentum * 0: the biased value

    for t, x in w.items():
        x.untouched(f"{case} {t}")
    for t, x in fl.items():
        if x is not None:
            x.untouched(f"{case} {t}")
