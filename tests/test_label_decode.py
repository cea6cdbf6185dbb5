"""The label inputs of the training image pipeline decoded on the device from the dataset's raw bytes (thinktwice_amd.labels,
csrc/labels.hip: tt_decode_depth_u8, tt_rgb2hsv_u8, tt_decode_seg_u8) against the numpy / scipy restatement of the reference's
LoadDepth / LoadSeg (tests/labels_ref.py), which golden F19 pins to the reference's own module.

Everything is compared BIT FOR BIT, no tolerance anywhere: the depth is one IEEE division and one IEEE product of exact f32
operands, the rest is integer arithmetic whose result does not depend on the order of the atomics.  The labelling cases use the
smallest images whose 64 x 16 tiles' edges fall inside (37 x 53: rows only), on (64 x 64) and one past (65 x 129) the image
edge."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import labels_ref as R  # noqa: E402
from label_cases import IDXS, SIZES, batch_isolation_case, decision_cases, mask_cases  # noqa: E402
from thinktwice_amd import calib, labels as L, synth  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f19_label_decode.npz")


@functools.lru_cache(maxsize=None)
def _conf():
    return L.seg_decode_conf(IDXS)


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()                   # (a copy: the shared references are read-only arrays)


def _device(tags, rgb, conf=None, **kw):
    """tags [B, N, H, W], rgb [B, N, H, W, 3] numpy -> the device's class map as numpy."""
    out = L.decode_seg(_cuda(tags), _cuda(rgb), conf or _conf(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _full_size():
    """(depth_rgb, tags, rgb, restated seg) of one 900 x 1600 camera: computed once, never modified."""
    d, t, c = synth.raw_label_bytes(19, 1, 900, 1600)
    ref = R.decode_seg_batch(t, c, IDXS)
    for a in (d, t, c, ref):
        a.setflags(write=False)
    return d, t, c, ref


# ----------------------------------------------------------------------------------------------------------------- depth
def test_depth_of_every_24_bit_code_is_bit_equal_to_numpy_float32():
    code = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([code & 255, (code >> 8) & 255, code >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    got = L.decode_depth(torch.from_numpy(rgb).cuda()).cpu().numpy()
    want = R.decode_depth(rgb)
    assert got.dtype == want.dtype == np.float32 and got.shape == (4096, 4096)
    assert int((got.view(np.uint32) != want.view(np.uint32)).sum()) == 0
    assert got[0, 0] == 0.0 and got[-1, -1] == 1000.0


def test_depth_of_odd_sizes_and_unaligned_views():
    """The scalar tail (sizes that are no multiple of four pixels) and a pointer the four-pixel path cannot take."""
    rng = np.random.default_rng(5)
    for shape in ((1, 1, 3), (3, 7, 3), (2, 37, 53, 3)):
        rgb = rng.integers(0, 256, shape, dtype=np.uint8)
        got = L.decode_depth(torch.from_numpy(rgb).cuda()).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), R.decode_depth(rgb).view(np.uint32))
    flat = torch.from_numpy(rng.integers(0, 256, 3 * 1001 + 3, dtype=np.uint8)).cuda()
    view = flat[3:].view(1001, 3)                                # 3 bytes past an aligned allocation
    assert view.data_ptr() % 4 == 3 and view.is_contiguous()
    got = L.decode_depth(view.view(1, 1001, 3)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), R.decode_depth(view.cpu().numpy().reshape(1, 1001, 3)).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- HSV
def test_hsv_of_every_rgb_triple_is_equal_to_the_restatement():
    code = torch.arange(1 << 24, dtype=torch.int32, device="cuda")
    rgb = torch.stack([code & 255, (code >> 8) & 255, code >> 16], dim=-1).to(torch.uint8)
    got = L.rgb2hsv_u8(rgb).cpu().numpy()
    rgb = rgb.cpu().numpy()
    bad = 0
    for i in range(0, 1 << 24, 1 << 21):
        bad += int((got[i:i + (1 << 21)] != R.rgb2hsv_u8(rgb[i:i + (1 << 21)])).sum())
    assert bad == 0 and got[:, 0].max() == 179


# ------------------------------------------------------------------------------------------------------------- class map
@pytest.mark.parametrize("hw", [(1, 1), (37, 53)])
def test_class_map_without_a_traffic_light_tag(hw):
    """Random tags, most of them absent from the list (-> 0); tag 18 is in neither list, so it is a plain tag here."""
    H, W = hw
    rng = np.random.default_rng(H)
    tags = rng.integers(0, 256, (2, 3, H, W), dtype=np.uint8)
    tags[0, 0, 0, 0] = 18
    rgb = rng.integers(0, 256, (2, 3, H, W, 3), dtype=np.uint8)
    for idxs, tl in (([1, 4, 5, 6, 7, 8, 10, 12], 18), (IDXS, None), ([255, 0, 18, 3], 200)):
        conf = L.seg_decode_conf(idxs, traffic_light_tag=tl)
        assert conf.light_tag == -1
        want = R.decode_seg_batch(tags, rgb, idxs, traffic_light_tag=tl)
        assert np.array_equal(_device(tags, rgb, conf), want)
        assert set(np.unique(want)) <= set(range(len(idxs)))


# ------------------------------------------------------------------------------------------------------------- labelling
@pytest.mark.parametrize("hw", SIZES)
def test_labelling_cases_are_equal_to_the_restatement(hw):
    H, W = hw
    cases = mask_cases(H, W)
    names = sorted(cases)
    rng = np.random.default_rng(H * W)
    tags = np.where(np.stack([cases[k] for k in names]), 18, rng.choice([0, 1, 4, 12, 22], (len(names), H, W))).astype(np.uint8)[None]
    rgb = rng.integers(0, 256, (1, len(names), H, W, 3), dtype=np.uint8)
    got, want = _device(tags, rgb), R.decode_seg_batch(tags, rgb, IDXS)
    wrong = {k: int((got[0, i] != want[0, i]).sum()) for i, k in enumerate(names) if not np.array_equal(got[0, i], want[0, i])}
    assert not wrong, f"{H} x {W}: pixels that differ per case: {wrong}"
    # the cases are what they claim to be (a restatement that labelled nothing would agree with a device that did the same)
    of = {k: want[0, i] for i, k in enumerate(names)}
    assert not of["empty"][cases["empty"]].any() and len(np.unique(of["full"])) == 1 and of["full"][0, 0] >= 8
    for one in ("checkerboard", "spiral", "serpentine", "comb", "frame"):
        v = np.unique(of[one][cases[one]])
        assert len(v) == 1 and v[0] >= 8, one
    assert (of["nineteen and twenty"][1, 1:20] == 0).all() and (of["nineteen and twenty"][3, 1:21] >= 8).all()
    assert (of["corner diagonals"][cases["corner diagonals"]] >= 8).all()
    assert (of["noise"][cases["noise"]] == 0).any()


def test_decision_rule():
    tags, rgb, expected = decision_cases()
    want = R.decode_seg_batch(tags, rgb, IDXS)
    names = sorted(expected)
    for i, k in enumerate(names):                                  # the painted counts give what the case's name says
        assert set(np.unique(want[0, i][tags[0, i] == 18])) == {8.0 + expected[k]}, k
    got = _device(tags, rgb)
    wrong = [k for i, k in enumerate(names) if not np.array_equal(got[0, i], want[0, i])]
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------------- batch isolation
def test_images_next_to_each_other_in_memory_never_share_a_component():
    tags, rgb = batch_isolation_case()
    want = R.decode_seg_batch(tags, rgb, IDXS)
    assert np.array_equal(_device(tags, rgb), want)
    assert (want[tags == 18] == 0).any() and (want[tags == 18] >= 8).any()


def test_rgb_is_read_in_place_from_the_key_sweep_of_a_raw_tensor():
    tags, rgb = batch_isolation_case()
    rng = np.random.default_rng(2)
    raw = torch.from_numpy(np.stack([rng.integers(0, 256, rgb.shape, dtype=np.uint8), rgb], axis=1)).cuda()      # [B, T = 2, N, H, W, 3]
    view = raw[:, -1]
    assert not view.is_contiguous()
    t = torch.from_numpy(tags).cuda()
    a = L.decode_seg(t, view, _conf())
    b = L.decode_seg(t, view.contiguous(), _conf())
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), R.decode_seg_batch(tags, rgb, IDXS))


# ------------------------------------------------------------------------------------------------- full size, golden F19
def test_one_full_size_image():
    _, t, c, want = _full_size()
    got = _device(t[None], c[None])[0]
    assert int((got != want).sum()) == 0
    assert all((want == k).any() for k in (8, 9, 10)) and (want[t == 18] == 0).any()


def test_golden_f19_on_the_device():
    g = np.load(GOLDEN)
    n, h, w = (int(v) for v in g["shape"])
    d, t, c = synth.raw_label_bytes(int(g["seed"][0]), n, h, w)
    raw = torch.from_numpy(np.stack([c[::-1].copy(), c])[None]).cuda()          # [1, T = 2, N, h, w, 3]: the key sweep is the last
    depth, seg = L.RawLabelDecoder(g["seg_label_idxs"].tolist())(raw, _cuda(d[None]), _cuda(t[None]))
    assert depth.dtype == seg.dtype == torch.float32 and depth.shape == seg.shape == (1, n, h, w)
    assert np.array_equal(depth[0].cpu().numpy().view(np.uint32), g["depth"].view(np.uint32))
    assert np.array_equal(seg[0].cpu().numpy(), g["seg"].astype(np.float32))


# ----------------------------------------------------------------------------------------------------------- determinism
def test_calls_repeat_bit_for_bit_whatever_the_workspace_holds():
    cases = mask_cases(65, 129)
    rng = np.random.default_rng(9)
    tags = np.where(np.stack([cases["noise"], cases["spiral"], cases["u shapes"]]), 18, 4).astype(np.uint8)[None]
    rgb = rng.integers(0, 256, tags.shape + (3,), dtype=np.uint8)
    t, c = torch.from_numpy(tags).cuda(), torch.from_numpy(rgb).cuda()
    need = L.workspace_bytes(3, 65, 129)
    first = L.decode_seg(t, c, _conf())
    assert torch.equal(first, L.decode_seg(t, c, _conf()))
    for fill in (0xFF, 0x00):
        assert torch.equal(first, L.decode_seg(t, c, _conf(), workspace=torch.full((need,), fill, dtype=torch.uint8, device="cuda")))
    assert np.array_equal(first.cpu().numpy(), R.decode_seg_batch(tags, rgb, IDXS))


# ----------------------------------------------------------------------------------------------------------- error codes
def test_c_entries_return_errors_and_a_short_workspace_launches_nothing():
    from thinktwice_amd import _lib
    lib = _lib.lib()
    B, N, H, W = 1, 2, 37, 53
    tags = torch.full((B, N, H, W), 18, dtype=torch.uint8, device="cuda")
    rgb = torch.zeros(B, N, H, W, 3, dtype=torch.uint8, device="cuda")
    need = int(lib.tt_decode_seg_workspace_bytes(B * N, H, W))
    assert need == L.workspace_bytes(B * N, H, W) == B * N * H * W * 24
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.full((B, N, H, W), -7.0, device="cuda")
    conf = L.seg_decode_conf(IDXS)

    def call(tags_p=tags.data_ptr(), b=B, n=N, h=H, w=W, rgb_p=rgb.data_ptr(), stride=N * H * W * 3, conf_p=ctypes.byref(conf),
             ws_p=ws.data_ptr(), ws_bytes=need, out_p=out.data_ptr()):
        return lib.tt_decode_seg_u8(tags_p, b, n, h, w, rgb_p, stride, conf_p, ws_p, ws_bytes, out_p, None)

    assert call(ws_bytes=need - 1) == -1 and b"workspace" in lib.tt_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "the refused call wrote to its output"
    for kw in (dict(tags_p=None), dict(rgb_p=None), dict(conf_p=None), dict(ws_p=None), dict(out_p=None), dict(b=0), dict(n=0),
               dict(h=0), dict(w=-1), dict(h=65536, w=32768), dict(stride=N * H * W * 3 - 1), dict(ws_p=ws.data_ptr() + 4)):
        assert call(**kw) == -1, kw
    for tag in (-2, 256):
        bad = L.seg_decode_conf(IDXS)
        bad.light_tag = tag
        assert call(conf_p=ctypes.byref(bad)) == -1 and b"traffic-light tag" in lib.tt_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert lib.tt_decode_seg_workspace_bytes(0, H, W) == 0 and lib.tt_decode_seg_workspace_bytes(1, 65536, 32768) == 0
    tab = L.HsvTables()
    assert lib.tt_decode_depth_u8(None, 4, out.data_ptr(), None) == -1 and lib.tt_decode_depth_u8(rgb.data_ptr(), 0, out.data_ptr(), None) == -1
    assert lib.tt_rgb2hsv_u8(rgb.data_ptr(), 4, None, rgb.data_ptr(), None) == -1
    assert lib.tt_rgb2hsv_u8(rgb.data_ptr(), -1, ctypes.byref(tab), rgb.data_ptr(), None) == -1
    assert call() == 0                                              # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert bool((out >= 8.0).all())


# ------------------------------------------------------------------------------------------------------------ end to end
def test_pipeline_fed_by_the_decoder_equals_the_pipeline_fed_by_the_restatement():
    from thinktwice_amd.preprocess import IdaSampler, TrainImagePipeline
    d, t, c, seg_ref = _full_size()
    conf = dict(calib.IDA_AUG_CONF, final_dim=(128, 256), resize_lim=(0.16, 0.18))
    raw = torch.from_numpy(np.stack([synth.raw_camera_frames(3, T=1, N=1)[0], c])[None]).cuda()        # [1, 2, 1, 900, 1600, 3]
    depth, seg = L.RawLabelDecoder(IDXS)(raw, _cuda(d[None]), _cuda(t[None]))
    pipe = TrainImagePipeline(conf)
    params = IdaSampler(conf, seed=4).sample(1, 1)
    a = pipe(raw, depth, seg, params=params)
    b = pipe(raw, _cuda(R.decode_depth(d)[None]), _cuda(seg_ref[None]), params=params)
    for k in ("img", "depth", "seg"):
        assert torch.equal(a[k], b[k]), k
    assert a["seg"].shape == (1, 1, 128, 256) and float(a["seg"].max()) >= 8
