"""A bottleneck's conv3 and the next block's conv1 in one launch (csrc/conv_x3_join.hip, tt_conv2d_fwd_next, ops.conv2d(nxt=...))
against the two tt_conv2d_fwd launches it replaces -- other kernels, the same sums: both outputs bit for bit -- and against torch on
the CPU in float64 within the bound tests/test_conv_patch.py holds bf16x3 layers to.

Shapes: 3 images of 37 x 41 = 4,551 rows (more than the 4,096 rows below which a layer runs the latency kernel, no multiple of 256 or
32: the last workgroup and its last wave are partial) for the five (K1, Cout, N2) forms, and 3 x 64 x 64 = 12,288 rows (whole tiles)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FORMS = [(64, 256, 64), (64, 256, 128), (128, 512, 128), (128, 512, 256), (256, 1024, 256)]
RAGGED, FULL = (3, 37, 41), (3, 64, 64)
# variant: pair-format input?, folded-BN affine?, residual: None / "own" (a tensor of its own) / "window" (its own stride and offset)
VARIANTS = {"pair affine window": (True, True, "window"), "f32 plain own": (False, False, "own"), "pair affine none": (True, True, None)}
GUARD = 4096


def _waves(form):
    return 4 if form[2] == 256 else 8


def _label(form, pair):
    # (both test sizes are below kJoinMinRows, the rows from which callers route the join: the label says so)
    return f"conv_x3_join_kernel<{form[0]}, {form[2]}, {_waves(form)}>" + (" pre-split A" if pair else "") + " below kJoinMinRows"


def _unpair(t):
    """pair-format tensor [.., C] -> the f32 values hi + lo"""
    b = t.contiguous().view(torch.bfloat16).reshape(*t.shape[:-1], t.shape[-1] // 16, 2, 16).float()
    return (b[..., 0, :] + b[..., 1, :]).reshape(t.shape)


@functools.lru_cache(maxsize=None)
def _case(form, shape, variant):
    """Inputs (on the device) and the two-launch reference of a case: computed once, never modified."""
    from thinktwice_amd import ops, weights
    k1, cout, n2 = form
    N, H, W = shape
    pair, affine, res = VARIANTS[variant]
    g = torch.Generator().manual_seed(7000 + k1 + 3 * n2 + H + 17 * len(variant))
    y = torch.randn(N, H, W, k1, generator=g)
    w1 = torch.randn(cout, 1, 1, k1, generator=g) / k1 ** 0.5
    w2 = torch.randn(n2, 1, 1, cout, generator=g) / cout ** 0.5
    cpu = dict(y=y, w1=w1, w2=w2, s1=None, b1=None, s2=None, b2=None, res=None)
    if affine:
        cpu.update(s1=torch.rand(cout, generator=g) + 0.5, b1=0.1 * torch.randn(cout, generator=g),
                   s2=torch.rand(n2, generator=g) + 0.5, b2=0.1 * torch.randn(n2, generator=g))
    rcoff = 0
    if res:
        rcs, rcoff = (cout + 32, 16) if res == "window" else (cout, 0)
        cpu["res"] = torch.randn(N, H, W, rcs, generator=g)
    dev = {k: (v.cuda() if v is not None else None) for k, v in cpu.items()}
    dev["yp"] = weights.split_pairs_x3(dev["y"])
    w1x3, w2x3 = weights.split_pairs_x3(dev["w1"]), weights.split_pairs_x3(dev["w2"])
    kw1 = dict(scale=dev["s1"], shift=dev["b1"], act=1, w_x3=w1x3, res1=dev["res"], res1_coff=rcoff, in_pair=pair)
    nxt = (dev["w2"], w2x3, dev["s2"], dev["b2"], 1)
    xin = dev["yp"] if pair else dev["y"]
    x_ref = ops.conv2d(xin, dev["w1"], **kw1)
    k_a = ops._last_conv_kernel()
    z_ref = ops.conv2d(x_ref, dev["w2"], scale=dev["s2"], shift=dev["b2"], act=1, w_x3=w2x3, out_pair=True)
    k_b = ops._last_conv_kernel()
    assert "conv_igemm_glds_kernel<float" in k_a and ", true>" in k_a and "conv_igemm_glds_kernel<float" in k_b and ", true>" in k_b, (k_a, k_b)
    torch.cuda.synchronize()
    return dict(form=form, shape=shape, pair=pair, cpu=cpu, rcoff=rcoff, dev=dev, xin=xin, kw1=kw1, nxt=nxt, x_ref=x_ref, z_ref=z_ref,
                label=_label(form, pair))


def _run(k, **kw):
    from thinktwice_amd import ops
    x, z = ops.conv2d(k["xin"], k["dev"]["w1"], nxt=k["nxt"], **k["kw1"], **kw)
    assert ops._last_conv_kernel() == k["label"], ops._last_conv_kernel()
    return x, z


CASES = [(f, RAGGED, v) for f in FORMS for v in VARIANTS] + [((64, 256, 64), FULL, "pair affine window"), ((128, 512, 128), FULL, "f32 plain own")]


@pytest.mark.parametrize("form,shape,variant", CASES, ids=[f"{f[0]}-{f[1]}-{f[2]} {s[1]}x{s[2]} {v}" for f, s, v in CASES])
def test_both_outputs_equal_the_two_launches(form, shape, variant):
    k = _case(form, shape, variant)
    x, z = _run(k)
    assert x.shape == k["x_ref"].shape and z.shape == k["z_ref"].shape
    assert torch.equal(x, k["x_ref"])
    assert torch.equal(z.view(torch.int32), k["z_ref"].view(torch.int32))
    x2, z2 = _run(k)                               # and a second run gives the same bits
    assert torch.equal(x2, x) and torch.equal(z2.view(torch.int32), z.view(torch.int32))


@pytest.mark.parametrize("form", FORMS, ids=[f"{f[0]}-{f[1]}-{f[2]}" for f in FORMS])
def test_accuracy_against_torch_on_the_cpu_in_float64(form):
    k = _case(form, RAGGED, "pair affine window")
    c = k["cpu"]
    k1, cout, n2 = form
    y = c["y"].double().reshape(-1, k1)
    x64 = y @ c["w1"].double().reshape(cout, k1).t() * c["s1"].double() + c["b1"].double()
    x64 = torch.relu(x64 + c["res"].double().reshape(-1, c["res"].shape[-1])[:, k["rcoff"]:k["rcoff"] + cout])
    z64 = torch.relu(x64 @ c["w2"].double().reshape(n2, cout).t() * c["s2"].double() + c["b2"].double())
    x, z = _run(k)
    for name, got, ref, want in (("x", x, k["x_ref"], x64), ("z", _unpair(z), _unpair(k["z_ref"]), z64)):
        err = float((got.cpu().double().reshape(want.shape) - want).abs().max()) / float(want.abs().max())
        ref_err = float((ref.cpu().double().reshape(want.shape) - want).abs().max()) / float(want.abs().max())
        print(f"{form} {name}: max abs err / max = {err:.3e} (the two launches: {ref_err:.3e})")
        assert err < 1e-4, (name, err)
        assert err <= ref_err, (name, err, ref_err)        # the two are bit-equal: a larger error is a bug


@pytest.mark.parametrize("form", FORMS, ids=[f"{f[0]}-{f[1]}-{f[2]}" for f in FORMS])
def test_outputs_are_fully_written_and_nothing_else_is(form):
    """Outputs pre-filled with NaN come back without one; 4,096 guard floats before and after each output keep their pattern."""
    k = _case(form, RAGGED, "pair affine window")
    N, H, W = k["shape"]
    bufs = []
    for c in (form[1], form[2]):
        n = N * H * W * c
        b = torch.full((GUARD + n + GUARD,), -1234.5, dtype=torch.float32, device="cuda")
        b[GUARD:GUARD + n] = float("nan")
        bufs.append((b, n, b[GUARD:GUARD + n].view(N, H, W, c)))
    _run(k, out=bufs[0][2], nxt_out=bufs[1][2])
    torch.cuda.synchronize()
    for b, n, _ in bufs:
        assert bool((b[:GUARD] == -1234.5).all()) and bool((b[GUARD + n:] == -1234.5).all())
    assert not bool(torch.isnan(bufs[0][2]).any()) and torch.equal(bufs[0][2], k["x_ref"])
    assert torch.equal(bufs[1][2].view(torch.int32), k["z_ref"].view(torch.int32))


def _desc(k):
    """The (tt_conv_desc, tt_conv_next) ops.conv2d(nxt=...) builds for a case, on the case's own tensors (whatever is launched stays
    inside them)."""
    from thinktwice_amd import _lib, ops
    k1, cout, n2 = k["form"]
    N, H, W = k["shape"]
    d, n, v = ops._ConvDesc(), ops._ConvNext(), k["dev"]
    k["keep"] = (torch.empty(N, H, W, cout, device="cuda"), torch.empty(N, H, W, n2, device="cuda"))
    d.in_ = k["xin"].data_ptr(); d.N = N; d.H = H; d.W = W; d.Cin = k1; d.in_cstride = k1
    d.weight = v["w1"].data_ptr(); d.Cout = cout; d.KH = d.KW = d.stride = d.dil = 1
    d.out = k["keep"][0].data_ptr(); d.OH = H; d.OW = W; d.out_cstride = cout
    d.scale = v["s1"].data_ptr(); d.shift = v["b1"].data_ptr()
    d.res1 = v["res"].data_ptr(); d.res1_cstride = v["res"].shape[-1]; d.res1_coff = k["rcoff"]
    d.act = 1; d.dtype = d.out_dtype = _lib.TT_F32
    d.weight_x3 = k["kw1"]["w_x3"].data_ptr(); d.in_pair = 1
    n.next_weight = v["w2"].data_ptr(); n.next_weight_x3 = k["nxt"][1].data_ptr(); n.next_cout = n2
    n.next_scale = v["s2"].data_ptr(); n.next_shift = v["b2"].data_ptr(); n.next_act = 1
    n.next_out = k["keep"][1].data_ptr(); n.next_out_cstride = n2; n.next_out_pair = 1
    return d, n


# field changes that leave every pointer and size of the descriptor valid, and the word tt_last_error must name
REFUSALS = [(dict(act=2), "act"), (dict(next_act=3), "next_act"), (dict(next_out_pair=0), "next_out_pair"), (dict(out_pair=1), "out_pair"),
            (dict(pad=1), "pad"), (dict(res1_up_h=37, res1_up_w=41), "res1_up"), (dict(next_out_coff=8), "next_out_coff"),
            (dict(in_coff=4), "in_coff"), (dict(res2="res"), "res2"), (dict(shift_n="b1"), "shift_n"), (dict(out2="x"), "out2"),
            (dict(N=1, H=64, W=64, OH=64, OW=64), "N*OH*OW")]


@pytest.mark.parametrize("change,word", REFUSALS, ids=[w.replace("*", "x") for _, w in REFUSALS])
def test_refusals_name_the_field(change, word):
    from thinktwice_amd import _lib
    k = _case((64, 256, 64), RAGGED, "pair affine window")
    d, n = _desc(k)
    for f, val in change.items():
        if val == "res":
            d.res2 = k["dev"]["res"].data_ptr(); d.res2_cstride = k["dev"]["res"].shape[-1]
        elif val == "b1":
            d.shift_n = k["dev"]["b1"].data_ptr(); d.shift_n_mod = 1
        elif val == "x":
            d.out2 = k["keep"][0].data_ptr(); d.out2_cstride = k["form"][1]
        else:
            setattr(n if f.startswith("next_") else d, f, val)
    L = _lib.lib()
    assert L.tt_conv2d_fwd_next(ctypes.byref(d), ctypes.byref(n), _lib.cur_stream(k["xin"].device)) != 0
    err = L.tt_last_error().decode()
    print(err)
    assert word in err, err
    torch.cuda.synchronize()


def test_the_unchanged_descriptor_launches():
    """... so the refusals above are refusals of the change, not of the helper's descriptor."""
    from thinktwice_amd import _lib
    k = _case((64, 256, 64), RAGGED, "pair affine window")
    d, n = _desc(k)
    _lib.check(_lib.lib().tt_conv2d_fwd_next(ctypes.byref(d), ctypes.byref(n), _lib.cur_stream(k["xin"].device)), "tt_conv2d_fwd_next")
    torch.cuda.synchronize()
    assert torch.equal(k["keep"][0], k["x_ref"]) and torch.equal(k["keep"][1].view(torch.int32), k["z_ref"].view(torch.int32))
