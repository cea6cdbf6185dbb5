"""The inference-only routes of the convolutions -- pair format, in_up2, the joined stage, the one-launch stem, res1_up, the split-K
query -- are chosen by the predicates of thinktwice_amd/ops.py, which ask the library (tt_conv2d_plan) instead of restating its
contracts.  Two recorded tables pin that nothing moved when they began to ask:

  tests/route_cases.json   (host) tools/route_sweep.py at the commit before: every predicate's answer over a grid on both sides of
                           every threshold and at the numbers of every call site of lss.py at B = 1, 2 and 8;
  tests/route_labels.json  (MI355X) `python tests/test_routes.py --record` at that commit: the ordered launch records of the
                           ResNet-50 trunk at the smallest shapes that sit on the thresholds, in three modes.
"""
import contextlib
import functools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
LABELS = os.path.join(ROOT, "tests", "route_labels.json")

KNOBS = ("PAIR", "BNECK_JOIN", "SEG_UP2", "STEM_POOL", "SEG_CHAIN")
MODES = ("inference", "train_no_grad", "tape")
# (B, T, N, H, W).  Four images of 256 x 512: 131,072 stem rows, layer 1 at exactly 32,768 (the join is routed at its threshold),
# layer 2 at 8,192, layer 3 at 2,048 (pair format off).  One image of 64 x 128: 2,048 stem rows (the one-launch stem off)
IMAGES = {"4 x 256 x 512": (1, 2, 2, 256, 512), "1 x 64 x 128": (1, 1, 1, 64, 128)}


def test_every_recorded_answer_is_reproduced():
    """A case may only flip from yes to no, only off the model's call sites, and only where the library refuses the canonical
    descriptor of the form (tt_conv2d_plan != 0): there the old yes promised a launch that would have raised."""
    from tools import route_sweep
    from thinktwice_amd import ops
    cases = json.load(open(os.path.join(ROOT, "tests", "route_cases.json")))["cases"]
    assert len(cases) > 3000 and sum(c[3] is not None for c in cases) == 270
    for fn in ("pair_ok", "up2_ok", "join_ok", "stem_pool_ok", "res1_up_ok", "auto_splitk_asks"):
        assert {c[2] for c in cases if c[0] == fn} == {True, False}, fn          # both answers of every predicate are in the table
    flipped = []
    for fn, args, want, site in cases:
        got = route_sweep.ask(fn, args)
        if got != want:
            assert want and not got and site is None and fn in ("pair_ok", "up2_ok"), (fn, args, want, got, site)
            rows, cin, cout = args[:3]
            refusal = ops.plan_label(*ops.canonical_desc(fn[:-3], rows, cin, cout, *args[3:]))
            assert refusal.startswith("ERROR: tt_conv2d_fwd: "), (fn, args, refusal)
            flipped.append((fn, args, refusal))
    print(f"{len(flipped)} yes -> no, cout {sorted({a[2] for _, a, _ in flipped})}: {sorted({r for _, _, r in flipped})[:4]}")


@functools.lru_cache(maxsize=None)
def _net():
    from thinktwice_amd import config, lss, params
    sd = params.init_params(config.model_config(final_dim=(256, 512)), seed=3, parts=("img_encoder",))
    return lss._ResNet50(sd, "img_encoder.img_backbone", "f32x3", "cuda")


@functools.lru_cache(maxsize=None)
def _image(name):
    B, T, N, H, W = IMAGES[name]
    return torch.randn(B, T, N, 3, H, W, generator=torch.Generator().manual_seed(11)).cuda()


@contextlib.contextmanager
def _state(mode, knobs):
    from thinktwice_amd import autodiff, layers, ops
    saved = [getattr(ops, k) for k in KNOBS], layers.BN_TRAIN
    for k in KNOBS:
        setattr(ops, k, knobs)
    layers.BN_TRAIN = mode == "train_no_grad"
    ops.CONV_PROFILE, ops.CONV_KERNELS = [], []
    try:
        with (autodiff.Tape(x3=True) if mode == "tape" else contextlib.nullcontext()):
            yield
    finally:
        for k, v in zip(KNOBS, saved[0]):
            setattr(ops, k, v)
        layers.BN_TRAIN = saved[1]
        ops.CONV_PROFILE, ops.CONV_KERNELS = None, None


def _run(name, mode, knobs=True):
    """(stage outputs, [[shape label, kernel label]] of every recorded launch) of the trunk on IMAGES[name]; the stem as
    LSS.forward picks it: the plain 7 x 7 layer under a tape, else the one launch where stem_pool_ok says so, else the row-run
    layer over the bordered copy.  Images in sweep-major order on every path."""
    from thinktwice_amd import ops
    net, img = _net(), _image(name)
    B, T, N, _, H, W = img.shape
    flat = torch.cat([img[b, T - 1 - s] for s in range(T) for b in range(B)]).contiguous()
    with _state(mode, knobs):
        if mode == "tape":
            outs = net(ops.nchw_to_nhwc_pad(flat, torch.float32, net.cin_pad))
        elif net.stem_pool_ok(img):
            outs = net(img, image=True)
        else:
            xpad = torch.zeros(B * T * N, H + 6, W + 8, net.cin_pad, device="cuda")
            outs = net(ops.nchw_to_nhwc_border(flat, xpad, 3, 3), bordered=True)
        torch.cuda.synchronize()
        return outs, [[r[3], k] for r, k in zip(ops.CONV_PROFILE, ops.CONV_KERNELS)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_the_trunk_launches_the_recorded_kernels(mode):
    want = json.load(open(LABELS))
    for name in IMAGES:
        outs, rec = _run(name, mode)
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(rec, want[f"{mode}: {name}"])) if g != w]
        assert not bad and len(rec) == len(want[f"{mode}: {name}"]), (name, len(rec), len(want[f"{mode}: {name}"]), bad[:5])
        if mode != "tape":          # every knob off: the same bits from the plain launches
            off, rec_off = _run(name, mode, knobs=False)
            assert len(rec_off) >= len(rec) and not [k for _, k in rec_off if "pre-split" in k or "join" in k or "stem_pool" in k]
            for a, b in zip(outs, off):
                assert torch.equal(a, b), (name, mode)
    if mode == "inference":         # the shapes sit where the docstring says: the routed join at its threshold, the stem on both sides
        big, small = (_run(name, mode)[1] for name in IMAGES)
        assert ["M=131072 N=64 K=224 stem+pool k7x7s2", "conv_x3_stem_pool_kernel"] in big
        assert [s for s, k in big if " join " in s and "below" not in k][:1] == ["M=32768 N=256->64 K=64 join k1x1s1"]
        assert not [s for s, k in big if "M=2048 " in s and "pre-split" in k]
        assert not [s for s, _ in small if "stem+pool" in s] and [s for s, _ in small if s.startswith("M=2048 N=64 K=224 k7x1s2")]


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], "usage: python tests/test_routes.py --record [FILE]   (on an MI355X, at the commit to record)"
    table = {f"{mode}: {name}": _run(name, mode)[1] for mode in MODES for name in IMAGES}
    open((sys.argv[2:] + [LABELS])[0], "w").write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in table.items()) + "\n}\n")
    print({k: len(v) for k, v in table.items()})
