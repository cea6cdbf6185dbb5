"""The training image pipeline (IDAImageTransform(is_train=True): a resize / crop / flip draw per camera, shared by both sweeps
and by the camera's depth and segmentation label maps) -- thinktwice_amd.preprocess.IdaSampler / ida_mat / TrainImagePipeline /
fill_batch and the kernels behind tt_preprocess_images_ida / tt_preprocess_labels_ida, against golden F18 (the reference's
own pipeline at seed 18) and the torch-CPU restatement tests/train_pipeline_ref.py that F18 pins.

Bounds.  Restatement vs F18 (the same torch ops): max 1e-5, mean 1e-7, the figures tests/test_preprocess.py uses for F17.
Kernel vs F18 / restatement: max 2e-3, mean 2e-5, the project's bound for this arithmetic (the reference round-trips the
undistortion map through its [-1, 1] normalisation in f32).  Both are for normalised images, whose value range is about
1 / 0.225 = 4.4; a label map of value range R (depth 100 m, segmentation ids 11) gets the same bounds as fractions of its
range: 1e-5 * R / 4.4 and 1e-7 * R / 4.4 for the restatement, and for the kernel 2e-3 * 0.229 * 255 / 255 = 4.6e-4 * R
(max) and 4.6e-6 * R (mean), i.e. 0.046 m / 4.6e-4 m for depth and 5.1e-3 / 5.1e-5 for segmentation."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_pipeline_ref as R  # noqa: E402
from thinktwice_amd import calib  # noqa: E402

RANGE = {"depth": 100.0, "seg": 11.0}
IMG_RANGE = 4.4
GPU_MAX, GPU_MEAN = 2e-3, 2e-5
GPU_LABEL_MAX, GPU_LABEL_MEAN = 4.6e-4, 4.6e-6          # x RANGE
FD = (calib.FINAL_H, calib.FINAL_W)


def _P(rh, rw, cy, cx, flip, resize=None):
    from thinktwice_amd.preprocess import IdaParams
    return IdaParams(rh / 900.0 if resize is None else resize, rh, rw, cy, cx, bool(flip))


# ------------------------------------------------------------------------------------------------ CPU
def test_sampler_and_ida_mat_reproduce_the_reference_draws_golden_f18():
    from thinktwice_amd.preprocess import IdaSampler, ida_mat
    g = R.f18()
    assert int(g["seed"][0]) == 18
    got = IdaSampler(calib.IDA_AUG_CONF, seed=18).sample(1, 4)[0]
    np.testing.assert_array_equal(np.asarray([[p.resize, p.resized_h, p.resized_w, p.crop_y, p.crop_x, int(p.flip)] for p in got],
                                             dtype=np.float64), g["params"])
    assert [p.flip for p in got] == [False, True, True, True] and [p.crop_x for p in got] == [59, 1, 2, 19]
    mats = np.stack([ida_mat(p, FD) for p in got])
    assert mats.dtype == np.float32 and g["ida_mats"].shape == (2, 4, 4, 4)
    for t in range(2):                                               # both sweeps carry the camera's draw
        np.testing.assert_array_equal(g["ida_mats"][t], mats)


def test_sampler_in_evaluation_equivalent_form_gives_the_evaluation_matrix():
    from thinktwice_amd.preprocess import IdaSampler, ida_mat
    conf = dict(calib.IDA_AUG_CONF, resize_lim=(0.56, 0.56), rand_flip=False)
    for p in IdaSampler(conf, seed=5).sample(2, 4)[1]:
        assert (p.resize, p.resized_h, p.resized_w, p.crop_y, p.crop_x, p.flip) == (0.56, 504, 896, 56, 0, False)
        np.testing.assert_array_equal(ida_mat(p, FD), calib.eval_ida_mat())


def test_sampler_draws_the_flip_only_when_rand_flip_is_set():
    """The reference's `rand_flip and np.random.choice(...)` short-circuits: without rand_flip three draws per camera."""
    from thinktwice_amd.preprocess import IdaSampler
    s = IdaSampler(dict(calib.IDA_AUG_CONF, rand_flip=False), seed=18)
    s.sample(1, 4)
    twin = np.random.RandomState(18)
    twin.uniform(size=12)
    assert s.rng.uniform() == twin.uniform()


def test_restatement_matches_reference_pipeline_golden_f18():
    raw, depth, seg, params, out = R.seed18()
    e = R.errors_against_f18(out["img"].numpy(), out["depth"].numpy(), out["seg"].numpy())
    print("restatement vs F18:", e)
    assert e["img"][0] <= 1e-5 and e["img"][1] <= 1e-7, e
    assert e["img_image_mean"] <= 2e-6, e
    for k, rng in RANGE.items():
        assert e[k][0] <= 1e-5 * rng / IMG_RANGE and e[k][1] <= 1e-7 * rng / IMG_RANGE, (k, e)
        assert e[f"{k}_image_mean"] <= 2e-6 * rng / IMG_RANGE, (k, e)


def test_label_maps_are_seeded_and_in_range():
    from thinktwice_amd import synth
    d, s = synth.raw_label_maps(18, N=2, h=60, w=110)
    d2, s2 = synth.raw_label_maps(18, N=2, h=60, w=110)
    assert np.array_equal(d, d2) and np.array_equal(s, s2)
    assert d.dtype == s.dtype == np.float32 and d.shape == s.shape == (2, 60, 110)
    assert d.min() >= 0 and d.max() <= 100 and len(np.unique(d)) > d.size // 2                 # not quantised
    assert set(np.unique(s)) <= set(range(12)) and (s[:, :25, :25] == s[:, :1, :1]).all() and (s[:, 0, 25] != s[:, 0, 24]).any()


BAD = [(504, 896, 57, 0), (504, 896, 0, 1), (562, 1000, 115, 0), (562, 1000, 114, 105), (504, 896, -1, 0), (562, 1000, 0, -1),
       (0, 896, 0, 0), (504, 0, 0, 0), (-504, -896, 0, 0)]


@pytest.mark.parametrize("bad", BAD)
def test_invalid_parameters_raise_before_anything_is_launched(bad, monkeypatch):
    from thinktwice_amd import preprocess
    launched = []

    class Recorder:
        def __getattr__(self, name):
            return lambda *a: launched.append(name) or 0

    monkeypatch.setattr(preprocess, "lib", lambda: Recorder())
    pipe = preprocess.TrainImagePipeline(calib.IDA_AUG_CONF, device="cpu", undistort=False)
    raw = torch.zeros(1, 1, 2, 4, 6, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        pipe(raw, depth=torch.zeros(1, 2, 4, 6), params=[[_P(504, 896, 56, 0, 0), _P(*bad, 0)]])
    with pytest.raises(ValueError):
        pipe(raw)                                                    # neither params nor sampler
    with pytest.raises(ValueError):
        pipe(raw, params=[[_P(504, 896, 56, 0, 0)]])                 # one set for two cameras
    assert launched == []


def test_c_entries_refuse_invalid_parameter_sets_before_any_launch():
    """The C ABI's own argument check (host code only: it returns before touching the device)."""
    from thinktwice_amd import _lib
    from thinktwice_amd.preprocess import IdaSet
    import re
    L = _lib.lib()
    assert int(re.search(r"#define TT_IDA_MAX_SETS (\d+)", open(_lib.HEADER).read()).group(1)) == _lib.TT_IDA_MAX_SETS
    assert ctypes.sizeof(IdaSet) == 20
    dummy = (ctypes.c_float * 4)(1, 1, 1, 1)                          # a non-null pointer no valid call would get this far with
    for bad in BAD + [(504, 896, 56, 0, 2)]:
        sets = (IdaSet * 2)(IdaSet(504, 896, 56, 0, 0), IdaSet(*bad))
        rc = L.tt_preprocess_images_ida(dummy, 1, 2, 2, 900, 1600, dummy, dummy, sets, 448, 896, dummy, dummy, dummy, 4, 0, None, None)
        assert rc == -1 and b"set 1" in L.tt_last_error(), (bad, rc, L.tt_last_error())
        rc = L.tt_preprocess_labels_ida(dummy, 1, 2, 900, 1600, dummy, dummy, sets, 448, 896, dummy, None)
        assert rc == -1 and b"set 1" in L.tt_last_error(), (bad, rc, L.tt_last_error())
    big = (IdaSet * 1)(IdaSet(504, 896, 56, 0, 0))
    assert L.tt_preprocess_labels_ida(dummy, _lib.TT_IDA_MAX_SETS // 4 + 1, 4, 900, 1600, dummy, dummy, big, 448, 896, dummy, None) == -1
    assert L.tt_preprocess_labels_ida(dummy, 1, 1, 900, 1600, dummy, dummy, None, 448, 896, dummy, None) == -1


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _frames(seed):
    from thinktwice_amd import synth
    d, s = synth.raw_label_maps(seed)
    return torch.from_numpy(synth.raw_camera_frames(seed)), torch.from_numpy(d), torch.from_numpy(s)


@functools.lru_cache(maxsize=None)
def _pipe(undistort=True):
    from thinktwice_amd.preprocess import TrainImagePipeline
    return TrainImagePipeline(calib.IDA_AUG_CONF, undistort=undistort)


def _batch(seeds):
    fr = [_frames(s) for s in seeds]
    return tuple(torch.stack([f[i] for f in fr]).cuda() for i in range(3))


# eight distinct sets: (504, 896) where crop_x can only be 0; (562, 1000) with the crop at the left edge and touching the right
# (104 + 896 = 1000) and the bottom (114 + 448 = 562) edge; each with and without flip, a different one on every camera
EDGE_SETS = [[_P(504, 896, 0, 0, 0), _P(504, 896, 56, 0, 1), _P(562, 1000, 114, 0, 0), _P(562, 1000, 114, 104, 1)],
             [_P(562, 1000, 114, 0, 1), _P(562, 1000, 114, 104, 0), _P(504, 896, 30, 0, 1), _P(562, 1000, 0, 50, 0)]]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
def test_evaluation_parameters_reproduce_the_evaluation_kernel_bit_for_bit():
    from thinktwice_amd.preprocess import ImagePreprocessor
    raw, _, _ = _batch((18,))
    params = [[_P(504, 896, 56, 0, 0, resize=0.56)] * 4]
    pp = ImagePreprocessor()
    out = _pipe()(raw, params=params)
    assert out["img"].shape == (1, 2, 4, 3, 448, 896)
    assert torch.equal(_bits(out["img"]), _bits(pp(raw)))
    cl = _pipe()(raw, params=params, channel_last_dtype=torch.float32)["img"]
    assert cl.shape == (8, 448, 896, 4)
    assert torch.equal(_bits(cl), _bits(pp(raw, channel_last_dtype=torch.float32)))
    for dt in (torch.bfloat16, torch.float16):                       # and the 16-bit forms the LSS trunk consumes
        assert torch.equal(_pipe()(raw, params=params, channel_last_dtype=dt)["img"].view(torch.int16),
                           pp(raw, channel_last_dtype=dt).view(torch.int16))
    np.testing.assert_array_equal(out["ida_mats"].numpy(), np.broadcast_to(calib.eval_ida_mat(), (1, 2, 4, 4, 4)))


@pytest.mark.gpu
def test_flip_mirrors_the_output_columns_and_nothing_else():
    raw, depth, seg = _batch((18,))
    plain = [[p._replace(flip=False) for p in R.f18_params()]]
    flipped = [[p._replace(flip=True) for p in R.f18_params()]]
    a = _pipe()(raw, depth, seg, params=plain)
    b = _pipe()(raw, depth, seg, params=flipped)
    for k in ("img", "depth", "seg"):
        assert torch.equal(_bits(b[k]), _bits(torch.flip(a[k], [-1]))), k
        assert not torch.equal(a[k], b[k])


@pytest.mark.gpu
def test_seed_18_matches_reference_pipeline_golden_f18_and_the_restatement():
    from thinktwice_amd.preprocess import IdaSampler
    raw, depth, seg = _batch((18,))
    _, _, _, params, ref = R.seed18()
    out = _pipe()(raw, depth, seg, sampler=IdaSampler(calib.IDA_AUG_CONF, 18))
    assert out["params"] == [params]
    np.testing.assert_array_equal(out["ida_mats"][0].numpy(), R.f18()["ida_mats"])
    got = {k: out[k][0].cpu() for k in ("img", "depth", "seg")}
    e = R.errors_against_f18(*(got[k].numpy() for k in ("img", "depth", "seg")))
    r = {k: (float((got[k] - ref[k]).abs().max()), float((got[k] - ref[k]).abs().mean())) for k in got}
    print("kernels vs F18 (max, mean):", e)
    print("kernels vs restatement (max, mean):", r)
    for name, x in (("F18", e), ("restatement", r)):
        assert x["img"][0] <= GPU_MAX and x["img"][1] <= GPU_MEAN, (name, x)
        for k, rng in RANGE.items():
            assert x[k][0] <= GPU_LABEL_MAX * rng and x[k][1] <= GPU_LABEL_MEAN * rng, (name, k, x)
    assert e["img_image_mean"] <= 2 * GPU_MEAN, e
    for k, rng in RANGE.items():
        assert e[f"{k}_image_mean"] <= 2 * GPU_LABEL_MEAN * rng, (k, e)


@pytest.mark.gpu
def test_crops_at_the_edges_of_the_resized_image_match_the_restatement():
    raw, depth, seg = _batch((18, 19))
    out = _pipe()(raw, depth, seg, params=EDGE_SETS)
    mx, my = calib.undistort_rectify_map()
    for b in range(2):
        ref = R.restate(raw[b].cpu(), EDGE_SETS[b], mx, my, depth[b].cpu(), seg[b].cpu())
        for k, (tmax, tmean) in (("img", (GPU_MAX, GPU_MEAN)), ("depth", (GPU_LABEL_MAX * 100, GPU_LABEL_MEAN * 100)),
                                 ("seg", (GPU_LABEL_MAX * 11, GPU_LABEL_MEAN * 11))):
            d = (out[k][b].cpu() - ref[k]).abs()
            cam = d.transpose(0, 1) if k == "img" else d                # camera first
            for n in range(4):                                           # every set on its own: one bad edge must not average out
                emax, emean = float(cam[n].max()), float(cam[n].mean())
                print(f"sample {b} camera {n} {k}: max {emax:.3e} mean {emean:.3e}")
                assert emax <= tmax and emean <= tmean, (b, n, k, EDGE_SETS[b][n], emax, emean)


@pytest.mark.gpu
def test_table_is_indexed_by_sample_and_camera_and_shared_by_the_sweeps():
    raw, depth, seg = _batch((18, 19))
    both = _pipe()(raw, depth, seg, params=EDGE_SETS)
    for b in range(2):
        one = _pipe()(raw[b:b + 1].contiguous(), depth[b:b + 1].contiguous(), seg[b:b + 1].contiguous(), params=[EDGE_SETS[b]])
        for k in ("img", "depth", "seg"):
            assert torch.equal(_bits(both[k][b]), _bits(one[k][0])), (b, k)
        assert torch.equal(both["ida_mats"][b], one["ida_mats"][0]) and torch.equal(both["ida_mats"][b, 0], both["ida_mats"][b, 1])
    # the two sweeps of a camera use one set: sweep 1's frames run as sweep 0 give sweep 1's output
    swapped = _pipe()(raw.flip(1).contiguous(), params=EDGE_SETS)["img"]
    assert torch.equal(_bits(swapped[:, 0]), _bits(both["img"][:, 1])) and torch.equal(_bits(swapped[:, 1]), _bits(both["img"][:, 0]))


@pytest.mark.gpu
def test_output_forms_agree():
    from thinktwice_amd import ops
    raw, _, _ = _batch((18,))
    params = [R.f18_params()]
    nchw = _pipe()(raw, params=params)["img"].view(8, 3, 448, 896)
    cl = _pipe()(raw, params=params, channel_last_dtype=torch.float32)["img"]
    assert cl.shape == (8, 448, 896, 4) and float(cl[..., 3].abs().max()) == 0.0
    assert torch.equal(_bits(cl[..., :3].permute(0, 3, 1, 2)), _bits(nchw))
    for dt in (torch.bfloat16, torch.float16):
        got = _pipe()(raw, params=params, channel_last_dtype=dt)["img"]
        assert got.shape == (8, 448, 896, 8) and got.dtype == dt
        assert torch.equal(got.view(torch.int16), ops.nchw_to_nhwc_pad(nchw, dt, 8).view(torch.int16))      # the library's rounding
    cl6 = _pipe()(raw, params=params, channel_last_dtype=torch.float32, c_pad=6)["img"]
    assert torch.equal(_bits(cl6[..., :3]), _bits(cl[..., :3])) and float(cl6[..., 3:].abs().max()) == 0.0


@pytest.mark.gpu
def test_pipeline_output_feeds_forward_train():
    """Hand-over only: sampler -> TrainImagePipeline -> fill_batch -> forward_train returns its 23 finite loss terms."""
    from thinktwice_amd import model as tm, params, synth
    from thinktwice_amd.preprocess import IdaSampler, TrainImagePipeline, fill_batch
    hw = (128, 256)
    conf = dict(calib.IDA_AUG_CONF, final_dim=hw, resize_lim=(0.16, 0.18))
    raw, depth, seg = _batch((18, 19))
    out = TrainImagePipeline(conf)(raw, depth, seg, sampler=IdaSampler(conf, seed=3))
    assert out["img"].shape == (2, 2, 4, 3, 128, 256) and out["depth"].shape == out["seg"].shape == (2, 4, 128, 256)
    batch = synth.make_batch(2, img_hw=hw, num_points=4096)
    batch.update(synth.make_train_targets(2, img_hw=hw))
    fill_batch(batch, out)
    assert batch["img"] is out["img"] and batch["depth"] is out["depth"] and batch["seg"] is out["seg"]
    for b in range(2):
        for t in range(2):
            assert torch.equal(batch["img_metas"][b][t]["ida_mats"], out["ida_mats"][b, t])
    m, cfg = tm.build_thinktwice(final_dim=hw, dtype=torch.float32)
    m.load_state_dict(params.init_params(cfg, seed=0))
    losses = m.forward_train(batch)
    torch.cuda.synchronize()
    assert len(losses) == 23
    for k, v in losses.items():
        assert bool(torch.isfinite(v).all()), (k, v)
