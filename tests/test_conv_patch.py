"""The pair-format 3 x 3 convolution on halo patches (csrc/conv_x3_patch.hip, chosen by conv_choose.cpp for in_pair layers from
kPatchMinRows output rows on) against the same layer on the f32 input -- another kernel (the per-tap tile that splits its operand
itself), the same sums: bit for bit -- and against torch on the CPU within the bound tests/test_conv_up2.py holds bf16x3 layers to.

Each case fixes everything but one image dimension and asks tt_conv2d_plan for the smallest value at which the pair-format layer
takes the new kernel AND the f32-input reference layer runs bf16x3 arithmetic (with fewer than 64 output channels it does so from
65,536 rows on; below, it would be the exact-f32 kernel, which is no bit-equal reference): the sizes follow the thresholds."""
import functools
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_spec = importlib.util.spec_from_file_location("conv_choice_sweep", os.path.join(ROOT, "tools", "conv_choice_sweep.py"))
sweep = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sweep)

LABEL = {64: "conv_x3_run3_kernel<64, patch> pre-split A", 32: "conv_x3_run3_kernel<32, patch> pre-split A"}

# name: N, H, W (None: the searched dimension), Cin, Cout, channels of the input buffer (> Cin: a window at channel 32), out_pair,
# and what the searched size must not be a multiple of
CASES = {
    "two images": dict(N=2, H=None, W=40, cin=32, cout=64),              # the halo must not reach into the neighbouring image
    "ragged": dict(N=1, H=None, W=37, cin=64, cout=64, odd=8),           # partial tiles right and bottom, rows no multiple of 256
    "seg head": dict(N=1, H=None, W=130, cin=64, cout=12),               # output channel stride 12, zero-page weight rows, unstored columns
    "cout 8": dict(N=1, H=None, W=96, cin=64, cout=8),
    "cout 32 out_pair": dict(N=1, H=None, W=72, cin=32, cout=32, out_pair=True),
    "four chunks": dict(N=1, H=None, W=80, cin=128, cout=32),
    "W = 1": dict(N=1, H=None, W=1, cin=32, cout=64),
    "H = 1": dict(N=1, H=1, W=None, cin=32, cout=64),
    "window": dict(N=1, H=None, W=48, cin=64, cout=64, cs=128),          # in_cstride = Cin + 64, in_coff = 32
}
ACCURACY = ["two images", "ragged", "seg head"]


def _label(c, H, W, in_pair):
    from thinktwice_amd import _lib
    L = _lib.lib()
    win = dict(cs=c["cs"], in_coff=32) if c.get("cs") else {}
    row, _ = sweep.describe(sweep.D("patch", c["N"], H, W, c["cin"], c["cout"], k=3, x3=True, in_pair=in_pair,
                                    out_pair=bool(c.get("out_pair")) and in_pair, **win), L)
    return sweep.plan_label(L, sweep.dict_to_desc(row))


def _size(c):
    """(H, W): the smallest searched dimension (both conditions are monotone in it), moved on to the next value the case allows."""
    def hw(v):
        return (v, c["W"]) if c["H"] is None else (c["H"], v)

    def ok(v):
        return _label(c, *hw(v), True) == LABEL[64 if c["cout"] == 64 else 32] and ", true>" in _label(c, *hw(v), False)
    lo, hi = 0, 1
    while not ok(hi):
        lo, hi = hi, 2 * hi
        assert hi < 1 << 22
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    if c.get("odd"):
        while hi % c["odd"] == 0 or (c["N"] * hi * c["W"]) % 256 == 0:
            hi += 1
    assert ok(hi)
    return hw(hi)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of a case (on the device) and the f32-input reference: computed once, never modified."""
    from thinktwice_amd import ops, weights
    c = CASES[name]
    H, W = _size(c)
    N, cin, cout, cs = c["N"], c["cin"], c["cout"], c.get("cs") or c["cin"]
    coff = 32 if c.get("cs") else 0
    g = torch.Generator().manual_seed(4000 + 13 * W + cin + cout)
    x = torch.randn(N, H, W, cs, generator=g)
    wt = torch.randn(cout, 3, 3, cin, generator=g) / (9 * cin) ** 0.5
    scale = torch.rand(cout, generator=g) + 0.5
    shift = 0.1 * torch.randn(cout, generator=g)
    dev = dict(x=x.cuda(), w=wt.cuda(), scale=scale.cuda(), shift=shift.cuda())
    dev["xp"] = weights.split_pairs_x3(dev["x"])          # per 16 channels: [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15]
    kw = dict(pad=1, scale=dev["scale"], shift=dev["shift"], act=1, w_x3=weights.split_pairs_x3(dev["w"]), in_coff=coff, cin=cin)
    ref = ops.conv2d(dev["x"], dev["w"], **kw)
    assert "pre-split" not in ops._last_conv_kernel() and ", true>" in ops._last_conv_kernel(), ops._last_conv_kernel()
    torch.cuda.synchronize()
    return dict(c=c, shape=(N, H, W), cpu=(x[..., coff:coff + cin], wt, scale, shift), dev=dev, kw=kw, ref=ref,
                label=LABEL[64 if cout == 64 else 32])


@pytest.mark.parametrize("name", list(CASES))
def test_the_patch_kernel_equals_the_layer_on_the_f32_input(name):
    from thinktwice_amd import ops, weights
    k = _case(name)
    N, H, W = k["shape"]
    print(f"{name}: N={N} H={H} W={W} rows={N * H * W}")
    if k["c"].get("out_pair"):
        got = ops.conv2d(k["dev"]["xp"], k["dev"]["w"], in_pair=True, out_pair=True, **k["kw"])
        assert ops._last_conv_kernel() == k["label"]
        assert torch.equal(got.view(torch.int32), weights.split_pairs_x3(k["ref"]).view(torch.int32))
    got = ops.conv2d(k["dev"]["xp"], k["dev"]["w"], in_pair=True, **k["kw"])
    assert ops._last_conv_kernel() == k["label"]
    assert tuple(got.shape) == (N, H, W, k["c"]["cout"])
    assert torch.equal(got, k["ref"])


@pytest.mark.parametrize("name", ACCURACY)
def test_accuracy_against_torch_on_the_cpu(name):
    from thinktwice_amd import ops
    k = _case(name)
    x, wt, scale, shift = k["cpu"]
    y = F.conv2d(x.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), padding=1)
    want = torch.relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    got = ops.conv2d(k["dev"]["xp"], k["dev"]["w"], in_pair=True, **k["kw"]).cpu()
    assert ops._last_conv_kernel() == k["label"]
    err = float((got - want).abs().max()) / float(want.abs().max())
    ref_err = float((k["ref"].cpu() - want).abs().max()) / float(want.abs().max())
    print(f"{name} {k['shape']}: max abs err / max = {err:.3e} (the kernel it replaces: {ref_err:.3e})")
    assert err < 1e-4, err
    assert err <= ref_err, (err, ref_err)         # the two are bit-equal: a larger error is a bug


@pytest.mark.parametrize("out_pair", [False, True])
def test_no_store_outside_the_output(out_pair):
    """Partial tiles on both edges: the bytes in front of and behind the output buffer keep their pattern."""
    from thinktwice_amd import ops, weights
    k = _case("ragged")
    N, H, W = k["shape"]
    cout = k["c"]["cout"]
    n_out, guard = N * H * W * cout, 4096
    buf = torch.full((guard + n_out + guard,), -1234.5, dtype=torch.float32, device="cuda")
    out = buf[guard:guard + n_out].view(N, H, W, cout)
    ops.conv2d(k["dev"]["xp"], k["dev"]["w"], in_pair=True, out_pair=out_pair, out=out, **k["kw"])
    assert ops._last_conv_kernel() == k["label"]
    torch.cuda.synchronize()
    assert bool((buf[:guard] == -1234.5).all()) and bool((buf[guard + n_out:] == -1234.5).all())
    want = weights.split_pairs_x3(k["ref"]) if out_pair else k["ref"]
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
