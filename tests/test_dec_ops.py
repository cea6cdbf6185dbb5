"""Op-level parity of the decoder's spatial kernels and row chains (csrc/dec_spatial.hip: tt_dec_gru, tt_dec_flatten,
tt_dec_bev_update; csrc/dec_chain.hip: tt_mlp_chain, tt_mlp_chain_wide) against the float64 restatements of tests/dec_ref.py.

Every compared tensor is held, element by element, to dec_ref.rule: 4 x the error of the CPU emulation of the promised bf16x3
arithmetic against float64, at least 8 * 2^-24, relative to max|ref64| -- computed on the CPU from the reference alone
(test_dec_ref.py asserts that every such limit is below 1e-4 and above plain f32's error).  The spatial kernels are called
through the C entries, so the tests own every buffer: scratch sized by the tt_dec_*_scratch_floats queries (and filled with NaN
where a test says so), outputs in sentinel buffers with guard rows behind the last sample or map.  With
TT_GLUE_PARITY_OUT=<file> the worst error per kernel and output is written there (profiles/decoder_ops_parity.txt)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dec_ref as D  # noqa: E402
from dec_ref import BEV_Q, C, GRU_P, HW, MIDS, PIX, Win, check_equal, check_rule  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")


def L():
    from thinktwice_amd import _lib
    return _lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(rc, what):
    assert rc == 0, f"{what} rc={rc}: {L().tt_last_error().decode()}"


def done():
    from thinktwice_amd import ops
    torch.cuda.synchronize()
    assert ops.device_faults() == 0


def rows_of(maps):
    """[N, 32, 21, 21] -> the kernels' channel-last rows [N, 441, 32] on the device."""
    return maps.permute(0, 2, 3, 1).reshape(maps.shape[0], PIX, C).contiguous().cuda()


def scratch_of(floats, fill):
    return torch.full((int(floats),), fill, dtype=torch.float32, device="cuda")


_PREP = {}


def prep(kind, sd):
    """decoder_fused.prep_* of a state dict, once per (kernel, state dict)."""
    from thinktwice_amd import decoder_fused as DF
    key = (kind, id(sd))
    if key not in _PREP:
        _PREP[key] = {"gru": lambda: DF.prep_gru(sd, GRU_P, "cuda"), "flat": lambda: DF.prep_flatten(sd, "cuda"),
                      "bev": lambda: DF.prep_bev_update(sd, BEV_Q, "cuda")}[kind]()
    return _PREP[key]


# ----------------------------------------------------------------------------- tt_dec_gru
def gru_run(c, fill=0.0, sample=None, scratch=None):
    """One launch on the case's samples (or on sample `sample` alone) -> (fut Win of B * 4 * 441 rows + guard, scratch)."""
    w = prep("gru", c["sd"])
    inp6, state = c["inp6"], c["state"]
    if sample is not None:
        inp6, state = inp6[sample:sample + 1], state[sample:sample + 1]
    B = state.shape[0]
    inp6_d, state_d = inp6.contiguous().cuda(), rows_of(state)
    if scratch is None:
        scratch = scratch_of(L().tt_dec_gru_scratch_floats(B), fill)
    fut = Win(B * 4 * PIX, C, guard=8)
    ok(L().tt_dec_gru(B, inp6_d.data_ptr(), state_d.data_ptr(), fut.ptr(), scratch.data_ptr(), w["w0"], w["wx"], w["b0"], w["w2"],
                      w["b2"], w["wd0"].data_ptr(), w["bd0"].data_ptr(), w["wd2"].data_ptr(), w["bd2"].data_ptr(), st()), "tt_dec_gru")
    torch.cuda.synchronize()
    fut.untouched("tt_dec_gru fut")
    return fut, scratch


def gru_maps(fut, B):
    return fut.get().view(B, 4, HW, HW, C).permute(0, 1, 4, 2, 3)          # [B, 4, 32, 21, 21]


@pytest.mark.parametrize("name", D.GRU_CASES)
def test_gru_matches_float64(name):
    """Every time step to its own limit, one comparison per border class (corners 0 2 6 8, edges 1 3 5 7, inside 4); exactly
    B * 4 * 441 * 32 floats written (the sentinel is far over any limit, the guard rows stay)."""
    c = D.gru_case(name)
    fut, _ = gru_run(c)
    got = gru_maps(fut, c["B"])
    assert bool(torch.isfinite(got).all())
    cls = D.border_classes()
    for t in range(4):
        for k in range(9):
            m = cls == k
            check_rule(f"dec_gru.fut[step {t + 1}]", f"{name} class {k}", got[:, t][:, :, m], c["ref"][t][:, :, m], c["limit"][t],
                       c["scale"][t])
    done()


def test_gru_scratch_contents_never_reach_fut():
    """NaN in the scratch (gates, states, the rows beyond pixel 440, the flag words before they are zeroed) changes no bit."""
    c = D.gru_case("B2")
    a, _ = gru_run(c, fill=0.0)
    b, _ = gru_run(c, fill=NAN)
    check_equal("dec_gru.fut", "NaN scratch == zero scratch", b.get(), a.get())
    done()


def test_gru_samples_are_independent():
    c = D.gru_case("B5")
    whole = gru_maps(gru_run(c)[0], 5)
    for b in range(5):
        alone = gru_maps(gru_run(c, sample=b)[0], 1)
        check_equal("dec_gru.fut", f"sample {b} of 5 == alone", whole[b:b + 1].contiguous(), alone.contiguous())
    done()


def test_gru_second_launch_on_the_same_scratch():
    """The flag words are zeroed again on the stream; stale gates and states of the first launch are overwritten before use."""
    c = D.gru_case("B2")
    a, scratch = gru_run(c, fill=NAN)
    b, _ = gru_run(c, scratch=scratch)
    check_equal("dec_gru.fut", "second launch == first", b.get(), a.get())
    done()


# ----------------------------------------------------------------------------- tt_dec_flatten
def flat_run(sd, maps, mids=True, fill=0.0):
    """-> (out Win [n, 256], mids Win [n, 9472] | None), guards checked."""
    w = prep("flat", sd)
    n = maps.shape[0]
    maps_d = rows_of(maps)
    out = Win(n, 256, guard=2)
    mid = Win(n, MIDS, guard=1) if mids else None
    scratch = scratch_of(L().tt_dec_flatten_scratch_floats(n), fill)
    ok(L().tt_dec_flatten(n, maps_d.data_ptr(), out.ptr(), mid.ptr() if mids else None, scratch.data_ptr(), w["w"], w["b"],
                          w["bn_scale"].data_ptr(), w["bn_shift"].data_ptr(), st()), "tt_dec_flatten")
    torch.cuda.synchronize()
    out.untouched("tt_dec_flatten out")
    if mids:
        mid.untouched("tt_dec_flatten mids")
    return out, mid


@pytest.mark.parametrize("name", D.FLAT_CASES)
def test_flatten_matches_float64(name):
    """1 map; 4 and 32: exact fits of the tail's groups of 4, 8, 16, 32 maps; 5, 17, 33: a last group of one map; signed inputs;
    a map that is all negative; a map whose maximum sits in a corner pixel."""
    c = D.flat_case(name)
    out, mid = flat_run(c["sd"], c["maps"])
    got = D.mids_of(mid.get()) + [out.get()]
    for i, what in enumerate(D.FLAT_OUT):
        assert bool(torch.isfinite(got[i]).all())
        check_rule("dec_flatten." + what, name, got[i], c["ref"][i], c["limit"][i], c["scale"][i])
    done()


def test_flatten_without_mids_and_with_nan_scratch_is_bit_equal():
    """mids = null switches stages 10 and 15 of the tail to scratch for their staged block output; NaN in the scratch (every
    intermediate of the tail) changes no bit."""
    c = D.flat_case("maps5")
    out, mid = flat_run(c["sd"], c["maps"])
    bare, _ = flat_run(c["sd"], c["maps"], mids=False)
    check_equal("dec_flatten.flat", "mids = null == with mids", bare.get(), out.get())
    out_n, mid_n = flat_run(c["sd"], c["maps"], fill=NAN)
    bare_n, _ = flat_run(c["sd"], c["maps"], mids=False, fill=NAN)
    check_equal("dec_flatten.flat", "NaN scratch == zero scratch", out_n.get(), out.get())
    check_equal("dec_flatten.mids", "NaN scratch == zero scratch", mid_n.get(), mid.get())
    check_equal("dec_flatten.flat", "mids = null, NaN scratch", bare_n.get(), out.get())
    done()


def test_flatten_maps_are_independent():
    """Map i of the 33-map launch against the same map alone: the tail packs rows of several maps into one tile, and a row's K
    order does not depend on its neighbours."""
    c = D.flat_case("maps33")
    out, mid = flat_run(c["sd"], c["maps"])
    whole, whole_mid = out.get(), mid.get()
    for i in range(33):
        o, m = flat_run(c["sd"], c["maps"][i:i + 1])
        check_equal("dec_flatten.flat", f"map {i} of 33 == alone", whole[i:i + 1].contiguous(), o.get())
        check_equal("dec_flatten.mids", f"map {i} of 33 == alone", whole_mid[i:i + 1].contiguous(), m.get())
    done()


# ----------------------------------------------------------------------------- tt_dec_bev_update
BEV_ROW = PIX * C


def bev_g(c, rows=None):
    """G of the case through ops.mlp_chain(..., n_split=5), as decoder_fused issues it -> Win [B, 1152]."""
    from thinktwice_amd import ops
    w = prep("bev", c["sd"])
    hb = c["hb"] if rows is None else c["hb"][rows]
    g = Win(hb.shape[0], 1152, guard=2)
    ops.mlp_chain(hb.contiguous().cuda(), [{"lin": w["G"], "src": -1, "out": (g.buf, 0)}], n_split=5)
    torch.cuda.synchronize()
    g.untouched("G")
    return g


def bev_run(c, g_rows, out_stride=BEV_ROW, out2_stride=0, fill=0.0, sample=None, scratch=None):
    """g_rows: device [B, 1152].  -> (out Win of B rows of 441 * 32 floats at row stride out_stride, out2 Win | None, scratch)."""
    w = prep("bev", c["sd"])
    bev = c["bev"] if sample is None else c["bev"][sample:sample + 1]
    B = bev.shape[0]
    bev_d = rows_of(bev)
    assert g_rows.shape == (B, 1152) and g_rows.is_contiguous()
    out = Win(B, BEV_ROW, cstride=out_stride, guard=1)
    out2 = Win(B, BEV_ROW, cstride=out2_stride, guard=1) if out2_stride else None
    if scratch is None:
        scratch = scratch_of(L().tt_dec_bev_update_scratch_floats(B), fill)
    ok(L().tt_dec_bev_update(B, bev_d.data_ptr(), g_rows.data_ptr(), out.ptr(), out_stride, out2.ptr() if out2 else None, out2_stride,
                             scratch.data_ptr(), w["w0"].data_ptr(), w["b0"].data_ptr(), w["w2"], w["b2"].data_ptr(), st()),
       "tt_dec_bev_update")
    torch.cuda.synchronize()
    out.untouched("tt_dec_bev_update out")
    if out2:
        out2.untouched("tt_dec_bev_update out2")
    return out, out2, scratch


def g_dev(g):
    return g.buf[:g.R].contiguous()


@pytest.mark.parametrize("name", D.BEV_CASES)
def test_bev_update_matches_float64(name):
    c = D.bev_case(name)
    B = c["B"]
    g = bev_g(c)
    check_rule("dec_bev_update.G", name, g.get(), c["ref"][0], c["limit"][0], c["scale"][0])
    out, _, _ = bev_run(c, g_dev(g))
    got = out.get().view(B, HW, HW, C).permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all())
    cls = D.border_classes()
    for k in range(9):
        m = cls == k
        check_rule("dec_bev_update.out", f"{name} class {k}", got[:, :, m], c["ref"][1][:, :, m], c["limit"][1], c["scale"][1])
    done()


def test_bev_update_strided_and_second_output():
    """out at a sample stride of 441 * 32 + 64 floats and the second copy at 4 * 441 * 32 (the stacked per-layer layout of the
    composite decoder): both bit-equal to the plain launch, the gaps between the samples and the guards untouched."""
    c = D.bev_case("B3")
    g = g_dev(bev_g(c))
    plain, _, _ = bev_run(c, g)
    out, out2, _ = bev_run(c, g, out_stride=BEV_ROW + 64, out2_stride=4 * BEV_ROW)
    check_equal("dec_bev_update.out", "out_bstride 441*32+64 == plain", out.get(), plain.get())
    check_equal("dec_bev_update.out2", "out2_bstride 4*441*32 == out", out2.get(), out.get())
    only2, second, _ = bev_run(c, g, out2_stride=BEV_ROW)
    check_equal("dec_bev_update.out2", "out2 plain stride == out", second.get(), only2.get())
    done()


def test_bev_update_scratch_samples_and_second_launch():
    c = D.bev_case("B3")
    g = g_dev(bev_g(c))
    a, _, _ = bev_run(c, g, fill=0.0)
    b, _, scratch = bev_run(c, g, fill=NAN)
    check_equal("dec_bev_update.out", "NaN scratch == zero scratch", b.get(), a.get())
    again, _, _ = bev_run(c, g, scratch=scratch)
    check_equal("dec_bev_update.out", "second launch == first", again.get(), a.get())
    for s in range(3):
        alone, _, _ = bev_run(c, g[s:s + 1].contiguous(), sample=s)
        check_equal("dec_bev_update.out", f"sample {s} of 3 == alone", alone.get(), a.get()[s:s + 1].contiguous())
    g_alone = bev_g(c, rows=[1])
    check_equal("dec_bev_update.G", "row 1 of 3 == alone", g_alone.get(), g[1:2].cpu())
    done()


# ----------------------------------------------------------------------------- row chains
FORMS = (("rows", False, None), ("wide-g1", True, 1), ("wide-g16", True, 16))
form_param = pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])


def chain_run(c, form, out_coff=0, n_split=1):
    """The case's stages in one forced form; every written output in a Win of row stride N + 8 at column out_coff, + guard rows.
    -> the Win of every stage with "out" (guards checked)."""
    from thinktwice_amd import ops
    _, wide, groups = form
    R = c["R"]
    xd = c["x"].cuda()
    stages, wins = [], []
    for s in c["stages"]:
        lin = ops.ChainLinear(s["w"], s.get("bias"), act=s.get("act", 0), side_k=s.get("side_k", 0))
        d = {"lin": lin, "src": s["src"]}
        if s.get("side") is not None:
            d["side"] = s["side"].cuda()
        if s.get("res") is not None:
            d["res"] = (s["res"].cuda(), s["res_coff"])
        if s.get("out"):
            N = s["w"].shape[0]
            win = Win(R, N, cstride=N + 8, coff=out_coff, guard=2)
            d["out"] = (win.buf, out_coff)
            wins.append(win)
        stages.append(d)
    ops.mlp_chain(xd, stages, n_split=n_split, groups=groups, wide=wide)
    torch.cuda.synchronize()
    assert ops.chain_faults() == 0
    for i, win in enumerate(wins):
        win.untouched(f"chain output {i}")
    return wins


def chain_check(c, form, name, out_coff=0, n_split=1):
    wins = chain_run(c, form, out_coff, n_split)
    kernel = "mlp_chain_wide" if form[1] else "mlp_chain"
    for i, win in enumerate(wins):
        got = win.get()
        assert bool(torch.isfinite(got).all())
        check_rule(kernel, f"{name} {form[0]} coff {out_coff}" + (f" n_split {n_split}" if n_split > 1 else ""), got, c["ref"][i],
                   c["limit"][i], c["scale"][i])
    return wins


SINGLE_IDS = [n for n in D.CHAIN_CASES if n.startswith("single")]


@form_param
@pytest.mark.parametrize("name", SINGLE_IDS)
def test_chain_single_stage_matches_float64(name, form):
    """Fewer K steps than the weight ring (kChainPF = 4; PF = 2, 4, 8 of the wide form) and than the wide form's K slices (waves with
    no step), step counts that are no multiple of the ring, all three wide_stage<PF> arms, 1, 2 and 4 row blocks per workgroup
    with dead ones (R = 65, 96, 129), K = 20 below Kp = 32 with the sentinel in the padding columns of x."""
    c = D.chain_case(name)
    for coff in (0, 4):
        chain_check(c, form, name, out_coff=coff)
    done()


@form_param
@pytest.mark.parametrize("name", [n for n in D.CHAIN_CASES if not n.startswith(("single", "split"))])
def test_chain_stages_match_float64(name, form):
    """64 -> 100 (ReLU) -> 8 with a ragged, zero-padded middle; residual (stride N + 12, offset 8) and side input (2 and 8 of 12
    columns) at 45 and 129 rows (the wide form's preloaded and in-loop epilogue operands); each of the six activations.
    (The ragged middle in the row form is the case that found mlp_chain_kernel storing a kept stage's columns 112 .. 127 -- the
    rest of its last 32-column block -- behind the 112-column LDS row, over the next row's first 16 columns: errors of half the
    output's maximum, the worst in rows 28 and 36 of the two cases.)"""
    chain_check(D.chain_case(name), form, name)
    done()


@form_param
def test_chain_column_split_is_bit_equal(form):
    """N = 96 is three column blocks: with n_split = 2 and 4 a workgroup of the row form has none."""
    c = D.chain_case("split-N96")
    one = chain_check(c, form, "split-N96")[0].get()
    for n_split in (2, 4):
        got = chain_check(c, form, "split-N96", n_split=n_split)[0].get()
        check_equal("mlp_chain_wide" if form[1] else "mlp_chain", f"split-N96 {form[0]} n_split {n_split} == 1", got, one)
    done()
