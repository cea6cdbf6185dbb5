"""tt_stem_pool_x3's refusals (csrc/conv_x3_stem.hip): every argument check comes before the first device call, so each is reachable
without a device; and the caller's rule ops.stem_pool_ok on plain CPU tensors."""
import pytest
import torch

P = 0x10000       # a stand-in for every pointer: the checks look at null-ness and alignment only

OK = dict(img=P, stride_b=0, stride_t=0, stride_n=3 * 36 * 68, stride_c=36 * 68, stride_h=68, stride_w=1, B=1, T=1, N=1, H=36, W=68,
          img_dtype=None, weight_x3=P, w_cout=64, w_kh=7, w_k=32, scale=P, shift=P, out=P, out_floats=9 * 17 * 64, max_workgroups=0)

REFUSALS = [
    (dict(H=35, stride_c=35 * 68), "H=35"),
    (dict(W=67, stride_h=67, stride_c=36 * 67), "W=67"),
    (dict(w_cout=32), "weight_x3 shape [32][7][1][32]"),
    (dict(w_kh=3), "weight_x3 shape [64][3][1][32]"),
    (dict(w_k=64), "weight_x3 shape [64][7][1][64]"),
    (dict(weight_x3=P + 8), "weight_x3 must be 16-byte aligned"),
    (dict(weight_x3=None), "weight_x3 is null"),
    (dict(stride_w=2), "stride_w=2"),
    (dict(stride_h=70), "stride_h=70"),
    (dict(stride_c=36 * 68 + 4), "stride_c=2452"),
    (dict(out_floats=9 * 17 * 64 - 1), "out_floats=9791"),
    (dict(out=P + 4), "out must be 16-byte aligned"),
    (dict(img_dtype="TT_BF16"), "img_dtype="),
    (dict(img_dtype="TT_F16"), "img_dtype="),
    (dict(scale=None), "scale / shift"),
    (dict(img=None), "img / out"),
    (dict(max_workgroups=-1), "max_workgroups=-1"),
    (dict(N=0), "N=0"),
]


@pytest.mark.parametrize("change,field", REFUSALS, ids=[f for _, f in REFUSALS])
def test_refusals_without_a_device(change, field):
    from thinktwice_amd import _lib
    L = _lib.lib()
    a = dict(OK, **change)
    a["img_dtype"] = getattr(_lib, a["img_dtype"] or "TT_F32")
    rc = L.tt_stem_pool_x3(a["img"], a["stride_b"], a["stride_t"], a["stride_n"], a["stride_c"], a["stride_h"], a["stride_w"], a["B"], a["T"],
                           a["N"], a["H"], a["W"], a["img_dtype"], a["weight_x3"], a["w_cout"], a["w_kh"], a["w_k"], a["scale"], a["shift"],
                           a["out"], a["out_floats"], a["max_workgroups"], None)
    assert rc != 0
    err = L.tt_last_error().decode()
    assert err.startswith("tt_stem_pool_x3: ") and field in err, err


def test_the_arguments_follow_the_header():
    from thinktwice_amd import _lib
    assert [n for _, n in _lib.prototypes()["tt_stem_pool_x3"].params] == list(OK) + ["stream"]


def test_the_callers_rule(monkeypatch):
    from thinktwice_amd import autodiff, layers, ops
    w = torch.zeros(64, 7, 1, 32)
    img = torch.zeros(1, 2, 2, 3, 64, 96)                       # 4 images x 32 x 48 = 6,144 stem rows
    monkeypatch.setattr(ops, "STEM_POOL", True)
    monkeypatch.setattr(layers, "BN_TRAIN", False)
    monkeypatch.setattr(autodiff, "TAPE", None)
    assert ops.stem_pool_ok(img, w)
    assert ops.stem_pool_ok(img[:, 1:], w[:]) is False          # 3,072 rows: the three launches run the exact-f32 kernel there
    assert ops.stem_pool_ok(torch.zeros(1, 1, 1, 3, 128, 128), w) is False and ops.stem_pool_ok(torch.zeros(1, 1, 1, 3, 128, 130), w)
    assert not ops.stem_pool_ok(img, None)
    assert not ops.stem_pool_ok(img.bfloat16(), w)
    assert not ops.stem_pool_ok(img[..., :95], w) and not ops.stem_pool_ok(img[..., :63, :], w)     # odd, and no longer contiguous
    assert not ops.stem_pool_ok(img[..., ::2], w)
    assert ops.stem_pool_ok(torch.zeros(3, 4, 4, 3, 64, 96)[::2, 1::2, ::2], w)                     # b / t / n strides are free
    monkeypatch.setattr(layers, "BN_TRAIN", True)
    assert not ops.stem_pool_ok(img, w)
    monkeypatch.setattr(layers, "BN_TRAIN", False)
    monkeypatch.setattr(autodiff, "TAPE", object())
    assert not ops.stem_pool_ok(img, w)
    monkeypatch.setattr(autodiff, "TAPE", None)
    monkeypatch.setattr(ops, "STEM_POOL", False)
    assert not ops.stem_pool_ok(img, w)
