"""The bf16x3 3 x 3 convolution that reads its input through the bilinear x2 upsampling (ops.conv2d(in_up2=True), tt_conv_desc.in_up2,
csrc/conv_x3_up2.hip) against the two launches it replaces -- ops.bilinear_up2(x, out_pair=True) then the same layer with
in_pair=True -- bit for bit, and against torch on the CPU within the bound tests/test_conv.py holds every bf16x3 layer to."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

COUT = 64
# (N, h, w, Cin): source shapes; the output is [N, 2h, 2w, 64]
SHAPES = [
    (2, 20, 40, 32),      # one channel chunk; two images: the halo must not reach into the neighbour image
    (1, 33, 37, 64),      # odd sizes, partial tiles at the right and bottom edge, 4,884 rows (no multiple of 256)
    (3, 8, 100, 128),     # the model's four chunks, a wide short image
    (1, 1, 2100, 32),     # h == 1 (sh == 0), a single tile row
    (1, 2100, 1, 32),     # w == 1
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs of a shape (on the device) and the two-launch reference, f32 and pair-format output: computed once, never modified."""
    from thinktwice_amd import ops, weights
    N, h, w, Cin = shape
    g = torch.Generator().manual_seed(1000 + 7 * h + w + Cin)
    x = torch.randn(N, h, w, Cin, generator=g)
    wt = torch.randn(COUT, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5
    scale = torch.rand(COUT, generator=g) + 0.5
    shift = 0.1 * torch.randn(COUT, generator=g)
    dev = dict(x=x.cuda(), w=wt.cuda(), scale=scale.cuda(), shift=shift.cuda())
    dev["w_x3"] = weights.split_pairs_x3(dev["w"])
    up = ops.bilinear_up2(dev["x"], out_pair=True)
    kw = dict(pad=1, scale=dev["scale"], shift=dev["shift"], act=1, w_x3=dev["w_x3"])
    ref = ops.conv2d(up, dev["w"], in_pair=True, **kw)
    ref_pair = ops.conv2d(up, dev["w"], in_pair=True, out_pair=True, **kw)
    torch.cuda.synchronize()
    return dict(cpu=(x, wt, scale, shift), dev=dev, kw=kw, ref=ref, ref_pair=ref_pair)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_launch_equals_the_two_launches(shape):
    from thinktwice_amd import ops
    c = _case(shape)
    got = ops.conv2d(c["dev"]["x"], c["dev"]["w"], in_up2=True, **c["kw"])
    assert ops._last_conv_kernel() == "conv_x3_run3_kernel<64, up2>"
    N, h, w, _ = shape
    assert tuple(got.shape) == (N, 2 * h, 2 * w, COUT)
    assert torch.equal(got, c["ref"])
    got_pair = ops.conv2d(c["dev"]["x"], c["dev"]["w"], in_up2=True, out_pair=True, **c["kw"])
    assert torch.equal(got_pair.view(torch.int32), c["ref_pair"].view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES[:3], ids=IDS[:3])
def test_accuracy_against_torch_on_the_cpu(shape):
    from thinktwice_amd import ops
    c = _case(shape)
    x, wt, scale, shift = c["cpu"]
    up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
    y = F.conv2d(up, wt.permute(0, 3, 1, 2), padding=1)
    want = torch.relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    got = ops.conv2d(c["dev"]["x"], c["dev"]["w"], in_up2=True, **c["kw"]).cpu()
    err = float((got - want).abs().max()) / float(want.abs().max())
    print(f"{shape}: max abs err / max = {err:.3e}")
    assert err < 1e-4, err


@pytest.mark.parametrize("out_pair", [False, True])
def test_no_store_outside_the_output(out_pair):
    """Partial tiles on both edges: the bytes in front of and behind the output buffer keep their pattern."""
    from thinktwice_amd import ops
    shape = SHAPES[1]
    c = _case(shape)
    N, h, w, _ = shape
    n_out, guard = N * 2 * h * 2 * w * COUT, 4096
    buf = torch.full((guard + n_out + guard,), -1234.5, dtype=torch.float32, device="cuda")
    out = buf[guard:guard + n_out].view(N, 2 * h, 2 * w, COUT)
    ops.conv2d(c["dev"]["x"], c["dev"]["w"], in_up2=True, out_pair=out_pair, out=out, **c["kw"])
    torch.cuda.synchronize()
    assert bool((buf[:guard] == -1234.5).all()) and bool((buf[guard + n_out:] == -1234.5).all())
    want = c["ref_pair"] if out_pair else c["ref"]
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


def _refused(**over):
    """The error text of a launch with one thing outside the contract."""
    from thinktwice_amd import _lib, ops, weights
    a = dict(N=1, h=40, w=64, cin=32, cout=64, kw={})
    a.update(over)
    x = torch.randn(a["N"], a["h"], a["w"], a["cin"], device="cuda")
    wt = torch.randn(a["cout"], 3, 3, a["cin"], device="cuda")
    kw = {k: (v(a) if callable(v) else v) for k, v in a["kw"].items()}
    with pytest.raises(_lib.TTError) as e:
        ops.conv2d(x, wt, pad=1, w_x3=weights.split_pairs_x3(wt), in_up2=True, **kw)
    return str(e.value)


def test_refusals_name_their_reason():
    assert "Cin" in _refused(cin=48)
    assert "Cout" in _refused(cout=32)
    assert "4096" in _refused(h=16, w=32)                     # 32 x 64 = 2048 rows
    assert "4096" in _refused(h=32, w=32)                     # exactly 4096 rows
    assert "residual" in _refused(kw=dict(res1=lambda a: torch.zeros(a["N"], 2 * a["h"], 2 * a["w"], a["cout"], device="cuda")))


def test_in_up2_with_in_pair_is_refused():
    """ops.conv2d asserts on the combination, so the descriptor is built here: the library's own message."""
    import ctypes
    from thinktwice_amd import _lib, ops, weights
    x = torch.randn(1, 40, 64, 32, device="cuda")
    wt = torch.randn(64, 3, 3, 32, device="cuda")
    w3 = weights.split_pairs_x3(wt)
    out = torch.empty(1, 80, 128, 64, device="cuda")
    d = ops._ConvDesc()
    d.in_ = x.data_ptr(); d.N = 1; d.H = 80; d.W = 128; d.Cin = 32; d.in_cstride = 32
    d.weight = wt.data_ptr(); d.weight_x3 = w3.data_ptr(); d.Cout = 64; d.KH = d.KW = 3; d.stride = 1; d.pad = 1; d.dil = 1
    d.out = out.data_ptr(); d.OH = 80; d.OW = 128; d.out_cstride = 64; d.shift_n_mod = 1
    d.in_up2 = 1; d.in_pair = 1
    L = _lib.lib()
    assert L.tt_conv2d_fwd(ctypes.byref(d), None) != 0
    msg = L.tt_last_error().decode()
    assert "in_up2" in msg and "in_pair" in msg, msg
