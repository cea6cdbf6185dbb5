"""The camera trunk with the bf16x3 stem as one launch (ops.stem_pool, ops.STEM_POOL / TT_STEM_POOL) against the same trunk with the
border copy, the row-run stem and the max pool as three launches: the four ResNet stage outputs bit for bit on `_ResNet50` alone at
B = 1, T = 2, N = 2, 64 x 96 (6,144 stem pixels: above the 4,096 from which the three launches run the bf16x3 tile), and through
`LSS.forward` (the synthetic rig: 4 cameras) the launch records, the bordered buffers and the routes that keep the three launches."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

HW = (64, 96)
FUSED = "conv_x3_stem_pool_kernel"


@functools.lru_cache(maxsize=None)
def _setup():
    from thinktwice_amd import config, params, synth
    cfg = config.model_config(final_dim=HW)
    sd = params.init_params(cfg, seed=3, parts=("img_encoder",))
    batch = synth.make_batch(1, img_hw=HW, num_points=16)
    return cfg, sd, batch


@functools.lru_cache(maxsize=None)
def _lss(dtype):
    from thinktwice_amd.lss import LSS
    cfg, sd, _ = _setup()
    enc = dict(cfg["img_encoder"])
    enc.pop("type")
    return LSS(**enc, dtype=dtype).load_state_dict(sd)


def _forward(dtype="f32x3", tape=False, fresh=False):
    """(LSS, [(shape label, kernel label)] of every recorded launch of one forward); `fresh`: on a module of its own (a train-mode
    forward moves the running statistics)"""
    from thinktwice_amd import autodiff, ops
    m, batch = (_lss.__wrapped__ if fresh else _lss)(dtype), _setup()[2]
    m._xpad.clear()
    ops.CONV_PROFILE, ops.CONV_KERNELS = [], []
    try:
        if tape:
            with autodiff.Tape(x3=True):
                m(batch["img"].cuda(), batch["img_metas"], channel_last=True)
        else:
            m(batch["img"].cuda(), batch["img_metas"], channel_last=True)
        torch.cuda.synchronize()
        return m, [(r[3], k) for r, k in zip(ops.CONV_PROFILE, ops.CONV_KERNELS)]
    finally:
        ops.CONV_PROFILE, ops.CONV_KERNELS = None, None


def test_stage_outputs_equal_with_one_launch_and_with_three(monkeypatch):
    from thinktwice_amd import lss, ops
    monkeypatch.setattr(ops, "STEM_POOL", True)
    _, sd, _ = _setup()
    net = lss._ResNet50(sd, "img_encoder.img_backbone", "f32x3", "cuda")
    img = torch.randn(1, 2, 2, 3, *HW, generator=torch.Generator().manual_seed(11)).cuda()
    assert net.stem_pool_ok(img)
    on = net(img, image=True)
    xpad = torch.zeros(4, HW[0] + 6, HW[1] + 8, 4, device="cuda")
    for s in range(2):
        ops.nchw_to_nhwc_border(img[0, 1 - s].contiguous(), xpad[2 * s:2 * s + 2], 3, 3)
    off = net(xpad, bordered=True)
    assert [tuple(t.shape) for t in on] == [(4, 16, 24, 256), (4, 8, 12, 512), (4, 4, 6, 1024), (4, 2, 3, 2048)]
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    monkeypatch.setattr(ops, "STEM_POOL", False)
    assert not net.stem_pool_ok(img)


def test_the_forward_records_the_one_launch_and_allocates_no_bordered_copy(monkeypatch):
    from thinktwice_amd import ops
    monkeypatch.setattr(ops, "STEM_POOL", True)
    m, rec = _forward()
    assert [k for _, k in rec].count(FUSED) == 1
    assert [s for s, k in rec if k == FUSED] == ["M=12288 N=64 K=224 stem+pool k7x7s2"]
    assert not [s for s, _ in rec if "k7x1s2" in s]
    assert m._xpad == {}
    monkeypatch.setattr(ops, "STEM_POOL", False)
    m, rec = _forward()
    assert FUSED not in [k for _, k in rec] and len([s for s, _ in rec if "k7x1s2" in s]) == 1 and len(m._xpad) == 1


@pytest.mark.parametrize("route", ["tape", "BN_TRAIN", "bfloat16"])
def test_the_other_routes_keep_their_launches(monkeypatch, route):
    from thinktwice_amd import layers, ops
    monkeypatch.setattr(ops, "STEM_POOL", True)
    if route == "BN_TRAIN":
        monkeypatch.setattr(layers, "BN_TRAIN", True)
    _, rec = _forward(dtype=torch.bfloat16 if route == "bfloat16" else "f32x3", tape=route == "tape", fresh=route == "BN_TRAIN")
    assert rec and FUSED not in [k for _, k in rec] and not [s for s, _ in rec if "stem+pool" in s]
    stem = [s for s, _ in rec if "K=224 k7x1s2" in s or "K=448 k7x1s2" in s or " k7x7s2" in s]
    assert len(stem) == 1, stem
