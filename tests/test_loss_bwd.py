"""Op-level parity of the two map-loss gradients (csrc/losses.hip: tt_loss_seg_focal_bwd, tt_loss_depth_bce_bwd) and of their
forward reductions, through LossReducer, against torch autograd over the float64 restatements of tests/sparse_ref.py.

The gradient buffer LossReducer allocates is pre-filled with the sentinel, so that an element the kernel leaves unwritten shows:
the padding columns [C, row_stride), the ignored / background pixels and the no-foreground map must come back exactly 0.  One shape of
each loss has more than 256 x 256 = 65,536 pixels, the grid of the kernels, and so reaches the second trip of their grid-stride loops.

Tolerance of the gradients: the elementwise rule of glue_ref.f32_limit on the gradient tensor (4 x torch's own f32 autograd error
against float64 on the same inputs, at least 8 * 2^-24, relative to max|ref|) plus the roundings of the kernel's f32 closing formula
of the coefficient, counted next to each loss below."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sparse_ref as S  # noqa: E402
from glue_ref import SENT, U32, check, f32_limit, sum_bound, vjp  # noqa: E402

pytestmark = pytest.mark.gpu

UPSTREAM = [None, 0.37]
C, ROW = 12, 16                       # 12 classes in 16-wide rows
PAD_LOGIT = 50.0                      # what the padding columns of the logits hold: read by mistake, it would dominate every softmax
# coefficient of the seg gradient, f32 in the kernel: coef = upstream * 5 * (2 (1 - e) e u + (1 - e)^2) / cnt with e = expf(-u).  Roundings:
# u as stored by the forward (1), expf (2), 1 - e (1, entering twice: 2), the two products of the first summand (2), the square (1), the
# sum (1), * 5 (1), * upstream (1), / cnt (1), and coef * (p - onehot) (1): 13; both summands are positive, so nothing cancels.  16 allows
# for the second-order terms.
SEG_COEF_ROUNDINGS = 16
# coefficient of the depth gradient: upstream / divisor (1), * upstream (1), coef * (sigmoid - onehot) (1)
DEPTH_COEF_ROUNDINGS = 3


def sentinel_outputs(monkeypatch):
    """LossReducer allocates its gradient with torch.empty_like: hand it a sentinel-filled buffer instead."""
    monkeypatch.setattr(torch, "empty_like", lambda t, **kw: torch.full_like(t, SENT))


def up_tensor(up):
    return None if up is None else torch.tensor([up], dtype=torch.float32).cuda()


def up_value(up):
    return 1.0 if up is None else float(torch.tensor(up, dtype=torch.float32))


# ----------------------------------------------------------------------------- seg focal
SEG_SHAPES = [(2, 8, 12), (3, 304, 304)]         # (BN, H, W) at factor 2: 48 pixels; 69,312 pixels (second trip of the grid-stride loop)


@functools.lru_cache(maxsize=None)
def seg_case(BN, H, W):
    g = torch.Generator().manual_seed(BN * H + W)
    h, w = H // 2, W // 2
    logits = torch.randn(BN, h, w, ROW, generator=g) * 2
    logits[..., C:] = PAD_LOGIT
    labels = torch.randint(0, C, (1, BN, H, W), generator=g).float()
    labels[torch.rand(1, BN, H, W, generator=g) < 0.1] = 255.0
    labels[0, -1, -2:, -8:] = 255.0                                   # the very last sampled pixels are ignored ones
    x = logits[..., :C]
    fn = lambda t: S.seg_focal(t, labels, 2)[0]                       # noqa: E731
    one = torch.ones(())
    g64, g32 = vjp(fn, [x], one)[0], vjp(fn, [x], one, torch.float32)[0]
    loss, u, cnt = S.seg_focal(x.double(), labels, 2)
    keep = labels.view(BN, H, W)[:, ::2, ::2] != 255
    assert cnt == int(keep.sum()) and not bool(keep.view(-1)[-4:].any()) and (BN * h * w > 65536) == (H > 100)
    if H > 100:
        assert bool(keep.view(-1)[65536:].any())                      # contributing pixels in the second trip too
    # forward bound: a pixel's m + logf(s) - v[label] in f32 (s: C expf terms), then double sums; per pixel (C + 8) roundings on
    # |m| + |log s| + |v_label| + 1 (the relative error of s is an absolute error of log s); the stored u is rounded once more
    xd = x.double()
    m, lse = xd.max(-1).values, torch.logsumexp(xd, -1)
    vl = xd.gather(-1, labels.view(BN, H, W)[:, ::2, ::2].long().clamp(0, C - 1).unsqueeze(-1)).squeeze(-1)
    du = (C + 8) * U32 * float(((m.abs() + (lse - m).abs() + vl.abs() + 1) * keep).sum() / cnt) + U32 * float(u)
    uu = u.detach().clone().requires_grad_(True)
    ((1 - torch.exp(-uu)) ** 2 * 5 * uu).backward()
    dloss = float(uu.grad.abs()) * du + 8 * U32 * float(loss)         # closing formula: expf, 1 - pt, the square, three products, the sign
    return dict(logits=logits, labels=labels, g64=g64, g32=g32, loss=float(loss), u=float(u), cnt=cnt, keep=keep, du=du, dloss=dloss)


@pytest.mark.parametrize("up", UPSTREAM, ids=["upstream-none", "upstream-0.37"])
@pytest.mark.parametrize("shape", SEG_SHAPES, ids=[f"{b}x{h}x{w}" for b, h, w in SEG_SHAPES])
def test_seg_focal_forward_and_gradient(shape, up, monkeypatch):
    from thinktwice_amd import losses
    BN, H, W = shape
    R = seg_case(*shape)
    red = losses.LossReducer("cuda")
    ld, lab, upd = R["logits"].cuda(), R["labels"].cuda(), up_tensor(up)
    sentinel_outputs(monkeypatch)

    def run():
        val = red.seg_focal(ld, lab, C, 2).cpu().clone()
        aux = red.seg_aux.cpu().clone()
        return val, aux, red.seg_focal_bwd(ld, lab, C, 2, upstream=upd).cpu()
    (val, aux, d), again = run(), run()
    for a, b in zip((val, aux, d), again):
        assert torch.equal(a, b), "two runs on the same inputs differ"
    case = f"{BN}x{H}x{W} factor 2 upstream {up}"
    check("loss_seg_focal", case + " loss", val.reshape(1), torch.tensor([R["loss"]]), slack=R["dloss"])
    check("loss_seg_focal", case + " mean CE", aux[:1], torch.tensor([R["u"]]), slack=R["du"])
    assert float(aux[1]) == R["cnt"]
    assert d.shape == R["logits"].shape
    assert bool((d[..., C:] == 0).all()), "padding columns of the gradient are not exactly 0"
    assert bool((d[~R["keep"]] == 0).all()), "ignored pixels of the gradient are not exactly 0"
    ref = R["g64"] * up_value(up)
    check("loss_seg_focal_bwd", case, d[..., :C], ref, rel=f32_limit(R["g32"], R["g64"]) + SEG_COEF_ROUNDINGS * U32)
    assert float(ref[R["keep"]].abs().min()) > 0 and bool((d[..., :C][R["keep"]] != 0).all())


# ----------------------------------------------------------------------------- depth BCE
D_BOUND, D, DROW = [1.0, 41.0, 0.5], 80, 88
# (BN, H, W, factor): the model's factor 16; and one cell per pixel, 66,560 cells: tt_loss_depth_bce accepts factor 1, so the second trip
# of the grid-stride loop is reached without a large depth map
DEPTH_SHAPES = [(2, 64, 128, 16), (1, 260, 256, 1)]
# cells of image 0, row 0 and the returns placed in them (all exact in f32) -> the bin + 1 they must fall into (0 = background)
EDGES = [((7.25, 3.0, 12.0, 0.0), 5), ((0.5,), 0), ((1.0,), 1), ((40.5,), 80), ((41.0,), 0), ((-2.0, 5.0), 0), ((), 0), ((40.75, 0.0), 80)]


@functools.lru_cache(maxsize=None)
def depth_case(BN, H, W, f, foreground=True):
    g = torch.Generator().manual_seed(BN * H + W + f)
    h, w = H // f, W // f
    logits = torch.randn(BN, h, w, DROW, generator=g) * 2
    logits[..., D:] = PAD_LOGIT
    gt = torch.zeros(1, BN, H, W)
    if foreground:
        gt = torch.rand(1, BN, H, W, generator=g) * 44.4 + 0.6            # returns between 0.6 and 45 m: some beyond the last bin
        gt[torch.rand(1, BN, H, W, generator=g) < (0.7 if f == 1 else 0.97)] = 0.0
        for i, (vals, _) in enumerate(EDGES):
            if f == 1 and len(vals) > 1:
                vals = vals[:1]                                          # one pixel per cell: the first return alone
            gt[0, 0, :f, i * f:(i + 1) * f] = 0.0
            for k, v in enumerate(vals):
                gt[0, 0, (k * 5) % f, i * f + (k * 3) % f] = v
    x = logits[..., :D]
    fn = lambda t: S.depth_bce(t, gt, D_BOUND, f)[0]                      # noqa: E731
    one = torch.ones(())
    g64, g32 = vjp(fn, [x], one)[0], vjp(fn, [x], one, torch.float32)[0]
    loss, div, bins = S.depth_bce(x.double(), gt, D_BOUND, f)
    if foreground:
        for i, (vals, want) in enumerate(EDGES):
            if f == 1 and len(vals) > 1:
                want = int((vals[0] - 0.5) / 0.5) if 1.0 <= vals[0] < 41.0 else 0
            assert int(bins[0, 0, i]) == want, (i, vals, int(bins[0, 0, i]), want)
        assert (BN * h * w > 65536) == (f == 1) and (f != 1 or bool((bins.view(-1)[65536:] >= 1).any()))
    # forward bound: a cell's D terms max(x, 0) - [bin] x + log1pf(expf(-|x|)) summed in f32 (six roundings on a term, D additions), the
    # cells in double, then the division and the cast
    xd, fg = x.double(), (bins >= 1).unsqueeze(-1)
    onehot = torch.nn.functional.one_hot(bins, D + 1)[..., 1:]
    terms = (xd.clamp_min(0) + (xd * onehot).abs() + torch.log1p(torch.exp(-xd.abs()))) * fg
    return dict(logits=logits, gt=gt, g64=g64, g32=g32, loss=float(loss), div=div, fg=bins >= 1,
                dloss=float(sum_bound(terms.sum() / div, D, 8)))


@pytest.mark.parametrize("up", UPSTREAM, ids=["upstream-none", "upstream-0.37"])
@pytest.mark.parametrize("shape", DEPTH_SHAPES, ids=[f"{b}x{h}x{w}-f{f}" for b, h, w, f in DEPTH_SHAPES])
def test_depth_bce_forward_and_gradient(shape, up, monkeypatch):
    """The cell-minimum rule (several returns in a cell, zeros ignored) and the depths exactly on the edges: 0.5 -> background,
    1.0 -> bin 0, 40.5 -> bin 79, 41.0 -> background, a negative value -> background (EDGES; asserted on the reference's bins)."""
    from thinktwice_amd import losses
    BN, H, W, f = shape
    R = depth_case(*shape)
    red = losses.LossReducer("cuda")
    ld, gtd, upd = R["logits"].cuda(), R["gt"].cuda(), up_tensor(up)
    sentinel_outputs(monkeypatch)

    def run():
        val = red.depth_bce(ld, gtd, D_BOUND, f).cpu().clone()
        aux = red.depth_aux.cpu().clone()
        return val, aux, red.depth_bce_bwd(ld, gtd, D_BOUND, f, upstream=upd).cpu()
    (val, aux, d), again = run(), run()
    for a, b in zip((val, aux, d), again):
        assert torch.equal(a, b), "two runs on the same inputs differ"
    case = f"{BN}x{H}x{W} factor {f} upstream {up}"
    check("loss_depth_bce", case + " loss", val.reshape(1), torch.tensor([R["loss"]]), slack=R["dloss"])
    assert float(aux[0]) == R["div"] > 8
    assert bool((d[..., D:] == 0).all()), "padding columns of the gradient are not exactly 0"
    assert bool((d[~R["fg"]] == 0).all()), "background cells of the gradient are not exactly 0"
    ref = R["g64"] * up_value(up)
    check("loss_depth_bce_bwd", case, d[..., :D], ref, rel=f32_limit(R["g32"], R["g64"]) + DEPTH_COEF_ROUNDINGS * U32)
    assert bool((d[..., :D][R["fg"]] != 0).all())


def test_depth_bce_without_foreground_has_divisor_one_and_a_zero_gradient(monkeypatch):
    from thinktwice_amd import losses
    R = depth_case(2, 64, 128, 16, foreground=False)
    assert R["div"] == 1 and R["loss"] == 0.0 and float(R["g64"].abs().max()) == 0.0
    red = losses.LossReducer("cuda")
    ld, gtd = R["logits"].cuda(), R["gt"].cuda()
    sentinel_outputs(monkeypatch)
    val = red.depth_bce(ld, gtd, D_BOUND, 16).cpu()
    assert float(val) == 0.0 and float(red.depth_aux.cpu()[0]) == 1.0
    for up in UPSTREAM:
        d = red.depth_bce_bwd(ld, gtd, D_BOUND, 16, upstream=up_tensor(up)).cpu()
        assert bool((d == 0).all()), "a map without foreground must give an all-zero gradient"
