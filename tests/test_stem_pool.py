"""The bf16x3 stem from the NCHW image to the max-pooled map in one launch (csrc/conv_x3_stem.hip, tt_stem_pool_x3, ops.stem_pool)
against the three launches it replaces -- tt_nchw_to_nhwc_border, the row-run stem on the bf16x3 LDS-DMA tile, tt_maxpool3x3s2: other
kernels, the same sums, every element bit for bit -- and against torch on the CPU in float64 within the bound tests/test_conv.py and
tests/test_conv_join.py hold the f32 bf16x3 layers to.

The three launches run the bf16x3 tile only above 4,096 output rows (below, tt_conv2d_fwd takes the exact-f32 latency kernel, which has
other sums, and callers keep the three launches: ops.stem_pool_ok).  The shapes here are far smaller, so the reference batch is the
case's images followed by filler images up to 4,097 stem rows; a row of the tile depends on its own image alone, and the label of the
reference launch is asserted.

Shapes (B, T, N, 3, H, W), the smallest that reach each way of going wrong:
  (1, 1, 1, 3, 36, 68)   pooled 9 x 17: no multiple of the 7 x 8 tile, partial tiles on both axes;
  (1, 1, 2, 3, 26, 38)   stem 13 x 19 is odd, pooled 7 x 10: the last window hangs over the stem map;
  (1, 1, 1, 3, 16, 288)  pooled 4 x 72: nine column tiles in a row; also with the persistent grid held to 1 and to 2 workgroups;
  (2, 2, 2, 3, 20, 24)   a strided view of a larger tensor (non-unit b / t / n strides): the sweep-major order."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = {"36x68": (1, 1, 1, 3, 36, 68), "26x38": (1, 1, 2, 3, 26, 38), "16x288": (1, 1, 1, 3, 16, 288), "strided 20x24": (2, 2, 2, 3, 20, 24)}
GUARD = 4096
SENTINEL = -12345.5


def _sweep_major(img):
    """(B, T, N, 3, H, W) -> (T*B*N, 3, H, W): image (s*B + b)*N + n = img[b, T-1-s, n]"""
    B, T, N = img.shape[:3]
    return torch.stack([img[b, T - 1 - s, n] for s in range(T) for b in range(B) for n in range(N)])


@functools.lru_cache(maxsize=None)
def _case(name, variant="plain"):
    """Inputs (on the device) and the three-launch reference of a case: computed once, never modified."""
    from thinktwice_amd import ops, weights
    B, T, N, _, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(900 + H + 3 * W + 7 * len(variant))
    if name.startswith("strided"):
        base = torch.randn(2 * B - 1, 2 * T, 2 * N, 3, H, W, generator=g)
        view = lambda t: t[::2, 1::2, ::2]                      # noqa: E731  b, t and n strides twice the dense ones, t offset by one
    else:
        base = torch.randn(B, T, N, 3, H, W, generator=g)
        view = lambda t: t                                      # noqa: E731
    if variant == "nan":
        view(base)[0, 0, 0, 1, H // 2 + 1, W // 2 - 3] = float("nan")
    w = torch.randn(64, 3, 7, 7, generator=g) * (3 * 49) ** -0.5
    scale, shift = torch.rand(64, generator=g) + 0.5, 0.1 * torch.randn(64, generator=g)
    if variant == "negative":
        shift[5] = -100.0
    wr = torch.zeros(64, 7, 1, 32)
    wr[:, :, 0, :28] = F.pad(w.permute(0, 2, 3, 1), (0, 1)).reshape(64, 7, 28)          # lss._ResNet50's row-run form
    dev = dict(base=base.cuda(), wr=wr.cuda(), scale=scale.cuda(), shift=shift.cuda())
    dev["img"] = view(dev["base"])
    dev["w_x3"] = weights.split_pairs_x3(dev["wr"])
    assert tuple(dev["img"].shape) == SHAPES[name]
    # the three launches, over the case's images and fillers up to 4,097 stem rows
    imgs = _sweep_major(dev["img"]).contiguous()
    NI, rows = imgs.shape[0], (H // 2) * (W // 2)
    total = max(NI, -(-4097 // rows))
    fill = torch.randn(total - NI, 3, H, W, generator=g).cuda()
    xpad = torch.zeros(total, H + 6, W + 8, 4, device="cuda")
    ops.nchw_to_nhwc_border(torch.cat([imgs, fill]), xpad, 3, 3)
    y = ops.conv2d(xpad, dev["wr"], stride=2, pad=0, scale=dev["scale"], shift=dev["shift"], act=1, in_cstride=4,
                   out_hw=(H // 2, W // 2), w_x3=dev["w_x3"])
    label = ops._last_conv_kernel()
    assert label.startswith("conv_igemm_glds_kernel<float, 64, 8, 1, 128, 2, false, true"), label
    ref = ops.maxpool3x3s2(y)[:NI].clone()
    torch.cuda.synchronize()
    return dict(name=name, cpu=dict(img=view(base), w=w, scale=scale, shift=shift), dev=dev, ref=ref, NI=NI)


def _fused(k, **kw):
    from thinktwice_amd import ops
    d = k["dev"]
    return ops.stem_pool(d["img"], d["w_x3"], d["scale"], d["shift"], **kw)


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_element_equals_the_three_launches(name):
    k = _case(name)
    B, T, N, _, H, W = SHAPES[name]
    out = _fused(k)
    assert tuple(out.shape) == (B * T * N, (H + 3) // 4, (W + 3) // 4, 64) == tuple(k["ref"].shape)
    assert torch.equal(out, k["ref"])
    assert torch.equal(_fused(k), out)                            # and a second run gives the same bits


@pytest.mark.parametrize("workgroups", [1, 2])
def test_more_tiles_than_one_persistent_pass(workgroups):
    k = _case("16x288")                                           # 9 tiles
    assert torch.equal(_fused(k, max_workgroups=workgroups), k["ref"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_accuracy_against_torch_on_the_cpu_in_float64(name):
    k = _case(name)
    c = k["cpu"]
    x = _sweep_major(c["img"]).double()
    want = F.max_pool2d(F.relu(F.conv2d(x, c["w"].double(), None, 2, 3) * c["scale"].double().view(1, -1, 1, 1) +
                               c["shift"].double().view(1, -1, 1, 1)), 3, 2, 1).permute(0, 2, 3, 1)
    top = float(want.abs().max())
    err = float((_fused(k).cpu().double() - want).abs().max()) / top
    ref_err = float((k["ref"].cpu().double() - want).abs().max()) / top
    print(f"{name}: max abs err / max = {err:.3e} (the three launches: {ref_err:.3e})")
    assert err < 1e-4, err
    assert err == ref_err, (err, ref_err)                         # the two are bit-equal


def test_a_channel_with_negative_pre_activations_is_exact_zeros():
    k = _case("36x68", "negative")
    out = _fused(k)
    assert torch.equal(out, k["ref"])
    assert int(torch.count_nonzero(out[..., 5])) == 0 and not bool(torch.signbit(out[..., 5]).any())
    assert int(torch.count_nonzero(out[..., 6])) > 0


def test_a_nan_pixel_gives_what_the_three_launches_give():
    k = _case("36x68", "nan")
    assert bool(torch.isnan(k["dev"]["img"]).any())
    out, ref = _fused(k), k["ref"]
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    assert torch.equal(torch.nan_to_num(out), torch.nan_to_num(ref))


def test_guard_floats_behind_the_output_stay():
    from thinktwice_amd import _lib
    k = _case("26x38")
    d, img = k["dev"], k["dev"]["img"]
    B, T, N, _, H, W = img.shape
    n = k["ref"].numel()
    buf = torch.full((n + GUARD,), SENTINEL, device="cuda")
    s = img.stride()
    _lib.check(_lib.lib().tt_stem_pool_x3(img.data_ptr(), s[0], s[1], s[2], s[3], s[4], s[5], B, T, N, H, W, _lib.TT_F32,
                                          d["w_x3"].data_ptr(), 64, 7, 32, d["scale"].data_ptr(), d["shift"].data_ptr(),
                                          buf.data_ptr(), n, 0, _lib.cur_stream(img.device)), "tt_stem_pool_x3")
    torch.cuda.synchronize()
    assert torch.equal(buf[:n].view(k["ref"].shape), k["ref"])
    assert bool((buf[n:] == SENTINEL).all())
