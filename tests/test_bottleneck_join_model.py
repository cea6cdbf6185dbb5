"""The ResNet-50 trunk with a bottleneck's conv3 and the next block's conv1 in one launch (thinktwice_amd/lss.py, ops.BNECK_JOIN)
against the same trunk with two launches: all four stage outputs bit for bit, the joins counted from the launch records.

8 images of 512 x 512: layer 1 has 131,072 rows and layer 2 32,768 = kJoinMinRows, the smallest size (for 8 square images) at which the
layer-1, layer-1 -> 2 and layer-2 joins are all taken."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

HW, NI = (512, 512), 8
JOINS = ["M=131072 N=256->64 K=64 join k1x1s1"] * 2 + ["M=131072 N=256->128 K=64 join k1x1s1"] + ["M=32768 N=512->128 K=128 join k1x1s1"] * 3


@functools.lru_cache(maxsize=None)
def _trunk():
    from thinktwice_amd import config, lss, params, weights
    cfg = config.model_config(final_dim=HW)
    sd = params.init_params(cfg, seed=3, parts=("img_encoder",))
    net = lss._ResNet50(sd, "img_encoder.img_backbone", "f32x3", "cuda")
    img = torch.randn(NI, 3, *HW, generator=torch.Generator().manual_seed(11))
    return net, weights.to_channel_last(img, torch.float32).cuda()


def _run(tape=False):
    """(stage outputs, [(shape label, kernel label)] of every convolution launch)"""
    from thinktwice_amd import autodiff, ops
    net, x = _trunk()
    ops.CONV_PROFILE, ops.CONV_KERNELS = [], []
    try:
        if tape:
            with autodiff.Tape(x3=True):
                outs = net(x)
        else:
            outs = net(x)
        torch.cuda.synchronize()
        return outs, [(r[3], k) for r, k in zip(ops.CONV_PROFILE, ops.CONV_KERNELS)]
    finally:
        ops.CONV_PROFILE, ops.CONV_KERNELS = None, None


def test_stage_outputs_equal_with_and_without_the_joins(monkeypatch):
    from thinktwice_amd import ops
    monkeypatch.setattr(ops, "BNECK_JOIN", True)
    on, rec_on = _run()
    monkeypatch.setattr(ops, "BNECK_JOIN", False)
    off, rec_off = _run()
    joined = [(s, k) for s, k in rec_on if " join " in s]
    print("\n".join(f"{s}: {k}" for s, k in joined))
    assert [s for s, _ in joined] == JOINS
    assert all(k.startswith("conv_x3_join_kernel<") and "below" not in k for _, k in joined)
    assert not [s for s, k in rec_off if " join " in s or "join" in k]
    assert len(rec_off) == len(rec_on) + len(JOINS)            # each join replaces two launches
    assert [tuple(t.shape) for t in on] == [(NI, 128, 128, 256), (NI, 64, 64, 512), (NI, 32, 32, 1024), (NI, 16, 16, 2048)]
    for a, b in zip(on, off):
        assert torch.equal(a, b)


def test_the_taped_forward_records_no_join(monkeypatch):
    from thinktwice_amd import ops
    monkeypatch.setattr(ops, "BNECK_JOIN", True)
    _, rec = _run(tape=True)
    assert rec and not [s for s, k in rec if " join " in s or "join" in k]
