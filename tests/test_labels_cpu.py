"""CPU half of the label decode (thinktwice_amd.labels): the restatement tests/labels_ref.py against golden F19 -- which the
reference's own LoadDepth / LoadSeg produced --, the contents of tt_seg_decode_conf for the config's tag list, the restatement
on hand-made masks, and every refusal that has to come before a launch.  The device half is tests/test_label_decode.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import labels_ref as R  # noqa: E402
from label_cases import IDXS, decision_cases, mask_cases  # noqa: E402
from thinktwice_amd import labels as L, synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f19_label_decode.npz")


# ------------------------------------------------------------------------------------------------------------ golden F19
def test_restatement_is_bit_equal_to_golden_f19():
    g = np.load(GOLDEN)
    n, h, w = (int(v) for v in g["shape"])
    assert g["seg_label_idxs"].tolist() == IDXS and g["seg"].dtype == np.uint8 and g["depth"].dtype == np.float32
    d, t, c = synth.raw_label_bytes(int(g["seed"][0]), n, h, w)
    assert np.array_equal(R.decode_depth(d).view(np.uint32), g["depth"].view(np.uint32))
    seg = R.decode_seg_batch(t, c, IDXS)
    assert seg.dtype == np.float32 and np.array_equal(seg, g["seg"].astype(np.float32))
    # what the fixture pins: every light type, the 20-pixel rule, the tag 1 -> class 0 quirk, tags outside the list
    assert all((g["seg"] == k).any() for k in range(11))
    assert (g["seg"][t == 18] == 0).any() and (t == 1).any() and not g["seg"][t == 1].any() and not g["seg"][t == 22].any()


def test_synthetic_label_bytes_are_seeded_and_have_blobs_of_both_kinds():
    a, b = synth.raw_label_bytes(5, 2, 60, 90), synth.raw_label_bytes(5, 2, 60, 90)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    d, t, c = a
    assert d.shape == c.shape == (2, 60, 90, 3) and t.shape == (2, 60, 90) and d.dtype == t.dtype == c.dtype == np.uint8
    sizes = [len(r) for n in range(2) for r in R.components(t[n] == 18)[0]]
    assert min(sizes) < 20 <= max(sizes)
    assert not np.array_equal(synth.raw_label_bytes(6, 2, 60, 90)[1], t)


# ------------------------------------------------------------------------------------------------------------- the conf
def test_conf_of_the_config_list():
    conf = L.seg_decode_conf(IDXS)
    want = np.zeros(256, dtype=np.uint8)
    for idx, tag in enumerate(IDXS[:-1]):
        want[tag] = idx
    assert list(conf.class_of_tag) == want.tolist() and conf.class_of_tag[1] == 0 and conf.class_of_tag[12] == 7
    assert (conf.light_tag, conf.light_base, conf.min_pixels, conf.val_low) == (18, 8, 20, 140)
    assert (conf.green_lo, conf.green_hi, conf.red_lo, conf.red_hi) == (70, 100, 150, 180)
    assert list(conf.sat_low_of_avg) == [int(a * 1.1) for a in range(256)]
    assert conf.sat_low_of_avg[100] == 110 and conf.sat_low_of_avg[231] == 254 and conf.sat_low_of_avg[232] == 255 and conf.sat_low_of_avg[233] == 256
    sdiv, hdiv = R.hsv_tables()
    assert list(conf.hsv.sdiv) == sdiv.tolist() and list(conf.hsv.hdiv) == hdiv.tolist()
    assert [np.array_equal(a, b) for a, b in zip(L.hsv_tables(), (sdiv, hdiv))] == [True, True]
    assert (sdiv[0], sdiv[1], sdiv[255], hdiv[0], hdiv[1], hdiv[255]) == (0, 1044480, 4096, 0, 122880, 482)
    assert ctypes.sizeof(L.SegDecodeConf) == 3360 and ctypes.sizeof(L.HsvTables) == 2048      # the header's comments
    none = L.seg_decode_conf(IDXS, traffic_light_tag=None)
    assert none.light_tag == -1 and none.class_of_tag[18] == 8
    assert L.seg_decode_conf([3, 18, 5]).light_base == 1 and L.seg_decode_conf([3, 5]).light_tag == -1


def test_conf_refuses_bad_lists():
    for bad in ([1, 4, 4], [1, 256], [-1, 2], [1.5, 2], [True, 2]):
        with pytest.raises(ValueError):
            L.seg_decode_conf(bad)
    with pytest.raises(ValueError):
        L.seg_decode_conf(IDXS, traffic_light_tag=256)
    with pytest.raises(ValueError):
        L.seg_decode_conf(list(range(255)) + [255], traffic_light_tag=255)          # classes 255..257


# --------------------------------------------------------------------------------------------------- restatement sanity
def test_restatement_on_hand_made_masks():
    cases = mask_cases(37, 53)
    rgb = np.zeros((37, 53, 3), dtype=np.uint8)                     # S = 0, V = 0: every classified component is type 0

    def seg(mask):
        return R.decode_seg(np.where(mask, 18, 0).astype(np.uint8), rgb, IDXS)

    assert not seg(cases["empty"]).any() and (seg(cases["full"]) == 8).all()
    for one in ("checkerboard", "spiral", "serpentine", "comb", "frame"):
        assert len(R.components(cases[one])[0]) == 1 and np.array_equal(seg(cases[one]) == 8, cases[one]), one
    assert [len(r) for r in R.components(cases["nineteen and twenty"])[0]] == [19, 20, 20, 19]
    s = seg(cases["nineteen and twenty"])
    assert not s[1].any() and (s[3, 1:21] == 8).all() and not s[17:36, 40].any() and (s[16:36, 44] == 8).all()
    assert len(R.components(cases["one pixel apart"])[0]) == 4 and len(R.components(cases["corner diagonals"])[0]) == 2
    four = np.zeros((5, 5), dtype=bool)
    four[0, 0] = four[1, 1] = four[0, 2] = True                     # joined through corners only: 8-connectivity
    four[4, 4] = True
    assert [len(r) for r in R.components(four)[0]] == [3, 1]


def test_restatement_decision_rule_and_hsv_spot_values():
    tags, rgb, expected = decision_cases()
    want = R.decode_seg_batch(tags, rgb, IDXS)
    for i, k in enumerate(sorted(expected)):
        assert set(np.unique(want[0, i][tags[0, i] == 18])) == {8.0 + expected[k]}, k
        assert set(np.unique(want[0, i][tags[0, i] != 18])) == {1.0}                 # tag 4 -> class 1
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [50, 50, 50]], dtype=np.uint8)
    assert R.rgb2hsv_u8(px).tolist() == [[0, 255, 255], [60, 255, 255], [120, 255, 255], [0, 0, 255], [0, 0, 0], [0, 0, 50]]
    hsv = np.array([[70, 110, 140], [69, 110, 140], [100, 255, 255], [101, 255, 255], [70, 109, 140], [70, 110, 139]],
                   dtype=np.uint8)[:, None, :]
    assert R.in_range(hsv, np.array([70, 110, 140]), np.array([100, 255, 255])).ravel().tolist() == [255, 0, 255, 0, 0, 0]
    assert not R.in_range(hsv, np.array([70, 264, 140]), np.array([100, 255, 255])).any()


# ---------------------------------------------------------------------------------------------------------- ValueErrors
class _Recorder:
    def __init__(self, launched):
        self.launched = launched

    def __getattr__(self, name):
        return lambda *a: self.launched.append(name) or 0


def test_bad_arguments_raise_before_anything_is_launched(monkeypatch):
    launched = []
    monkeypatch.setattr(L, "lib", lambda: _Recorder(launched))
    conf = L.seg_decode_conf(IDXS)
    tags, rgb = torch.zeros(2, 3, 5, 7, dtype=torch.uint8), torch.zeros(2, 3, 5, 7, 3, dtype=torch.uint8)
    raw = torch.zeros(2, 2, 3, 5, 7, 3, dtype=torch.uint8)
    dec = L.RawLabelDecoder(IDXS)
    for call in (lambda: L.decode_depth(rgb), lambda: L.rgb2hsv_u8(rgb), lambda: L.decode_seg(tags, rgb, conf),
                 lambda: dec(raw, rgb, tags)):
        with pytest.raises(ValueError, match="on the device"):     # CPU tensors
            call()
    assert launched == []


@pytest.mark.gpu
def test_bad_shapes_raise_before_anything_is_launched_on_the_device(monkeypatch):
    launched = []
    monkeypatch.setattr(L, "lib", lambda: _Recorder(launched))
    conf = L.seg_decode_conf(IDXS)
    tags = torch.zeros(2, 3, 5, 7, dtype=torch.uint8, device="cuda")
    rgb = torch.zeros(2, 3, 5, 7, 3, dtype=torch.uint8, device="cuda")
    raw = torch.zeros(2, 2, 3, 5, 7, 3, dtype=torch.uint8, device="cuda")
    dec = L.RawLabelDecoder(IDXS)
    bad = [lambda: L.decode_depth(rgb.float()), lambda: L.decode_depth(rgb[..., :2]), lambda: L.decode_depth(rgb[:, :, ::2]),
           lambda: L.decode_depth(rgb[:0]), lambda: L.rgb2hsv_u8(tags), lambda: L.rgb2hsv_u8(rgb[:, :, :, ::2]),
           lambda: L.decode_seg(tags[0], rgb[0], conf), lambda: L.decode_seg(tags, rgb[:, :2], conf),
           lambda: L.decode_seg(tags, rgb, None), lambda: L.decode_seg(tags.float(), rgb, conf),
           lambda: L.decode_seg(tags, rgb.transpose(2, 3).contiguous().transpose(2, 3), conf),
           lambda: L.decode_seg(tags.transpose(2, 3).contiguous().transpose(2, 3), rgb, conf),
           lambda: L.decode_seg(tags, rgb, conf, workspace=torch.zeros(10, dtype=torch.uint8, device="cuda")),
           lambda: dec(raw[:, 0], rgb, tags), lambda: dec(raw, rgb[:1], tags), lambda: dec(raw, rgb, tags[:, :, :4]),
           lambda: dec(raw.transpose(1, 2), rgb, tags)]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
    assert launched == []
    L.decode_seg(tags, raw[:, -1], conf)                            # the strided key sweep is accepted
    assert launched == ["tt_decode_seg_u8"]


def test_c_entries_refuse_bad_arguments_on_the_host():
    """The C ABI's own checks (host code only: every call here is refused before it touches the device)."""
    from thinktwice_amd import _lib
    lib = _lib.lib()
    dummy = (ctypes.c_float * 4)(1, 1, 1, 1)        # a non-null, 8-byte aligned pointer no valid call would get this far with
    conf = L.seg_decode_conf(IDXS)
    need = 2 * 37 * 53 * 24
    assert lib.tt_decode_seg_workspace_bytes(2, 37, 53) == need == L.workspace_bytes(2, 37, 53)
    assert lib.tt_decode_seg_workspace_bytes(0, 37, 53) == 0 and lib.tt_decode_seg_workspace_bytes(1, 65536, 32768) == 0

    def call(tags=dummy, b=1, n=2, h=37, w=53, rgb=dummy, stride=2 * 37 * 53 * 3, c=conf, ws=dummy, nbytes=need, out=dummy):
        return lib.tt_decode_seg_u8(tags, b, n, h, w, rgb, stride, None if c is None else ctypes.byref(c), ws, nbytes, out, None)

    assert call(nbytes=need - 1) == -1 and b"workspace" in lib.tt_last_error()
    for kw in (dict(tags=None), dict(rgb=None), dict(c=None), dict(ws=None), dict(out=None), dict(b=0), dict(n=-1), dict(h=0),
               dict(w=0), dict(h=65536, w=32768, nbytes=1 << 60), dict(stride=2 * 37 * 53 * 3 - 1), dict(b=65536, n=1, nbytes=1 << 60)):
        assert call(**kw) == -1, kw
    for tag in (-2, 256):
        bad = L.seg_decode_conf(IDXS)
        bad.light_tag = tag
        assert call(c=bad) == -1 and b"traffic-light tag" in lib.tt_last_error()
    bad = L.seg_decode_conf(IDXS)
    bad.light_base = 254
    assert call(c=bad) == -1 and b"base class" in lib.tt_last_error()
    tab = L.HsvTables()
    assert lib.tt_decode_depth_u8(None, 4, dummy, None) == -1 and lib.tt_decode_depth_u8(dummy, 0, dummy, None) == -1
    assert lib.tt_decode_depth_u8(dummy, 4, None, None) == -1
    assert lib.tt_rgb2hsv_u8(dummy, 4, None, dummy, None) == -1 and lib.tt_rgb2hsv_u8(dummy, -1, ctypes.byref(tab), dummy, None) == -1
    assert lib.tt_rgb2hsv_u8(None, 4, ctypes.byref(tab), dummy, None) == -1
