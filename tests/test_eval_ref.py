"""The label conventions tests/eval_ref.py restates equal the oracle's (oracle/train_ref.py::seg_loss / depth_loss): which pixel
is a seg cell's label, and which depth bin a cell belongs to.  CPU only.  Shapes: B*N = 3, 10 x 14 at factor 2 and 32 x 48 at
factor 16, with cells that are all zero, out of range, or exactly on a bin edge."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import eval_ref as E  # noqa: E402

D_BOUND = (1.0, 41.0, 0.5)
D = int((D_BOUND[1] - D_BOUND[0]) / D_BOUND[2])
SHAPES = [(10, 14, 2), (32, 48, 16)]


@pytest.mark.parametrize("H, W, f", SHAPES)
def test_the_seg_label_of_a_cell_is_the_oracles_nearest_resize(H, W, f):
    rng = np.random.default_rng(H)
    B, N = 1, 3
    lab = rng.integers(0, 12, (B, N, H, W)).astype(np.float32)
    lab[0, 1, ::3, ::5] = 255
    gt = torch.from_numpy(lab)
    # oracle/train_ref.py::seg_loss, its first statement
    want = F.interpolate(gt.view(1, B * N, H, W).float(), size=(H // f, W // f), mode="nearest")[0].long().numpy()
    got = E.seg_cell_labels(lab.reshape(B * N, H, W), f)
    assert got.shape == want.shape == (B * N, H // f, W // f)
    assert np.array_equal(got.astype(np.int64), want)


def _oracle_onehot(gt_depth, d_bound, factor):
    """oracle/train_ref.py::depth_loss up to the one-hot (the statements are its own)."""
    B, N, H, W = gt_depth.shape
    Dn = int((d_bound[1] - d_bound[0]) / d_bound[2])
    g = gt_depth.view(B * N, H // factor, factor, W // factor, factor, 1).permute(0, 1, 3, 5, 2, 4).contiguous()
    g = g.view(-1, factor * factor)
    g = torch.min(torch.where(g == 0.0, 1e5 * torch.ones_like(g), g), dim=-1).values
    g = g.view(B * N, H // factor, W // factor)
    g = (g - (d_bound[0] - d_bound[2])) / d_bound[2]
    g = torch.where((g < Dn + 1) & (g >= 0.0), g, torch.zeros_like(g))
    return F.one_hot(g.long(), num_classes=Dn + 1).view(-1, Dn + 1)[:, 1:].float()


@pytest.mark.parametrize("H, W, f", SHAPES)
def test_the_depth_bin_of_a_cell_is_the_oracles_one_hot(H, W, f):
    rng = np.random.default_rng(W)
    B, N = 1, 3
    h, w = H // f, W // f
    gt = np.zeros((B, N, H, W), np.float32)
    gt[rng.random(gt.shape) < 0.3] = 0
    vals = rng.uniform(0.2, 45.0, gt.shape).astype(np.float32)
    mask = rng.random(gt.shape) < 0.2
    gt[mask] = vals[mask]
    cells = gt.reshape(B * N, h, f, w, f)
    cells[0, 0, :, 0, :] = 0.0                                   # all zero: background
    cells[0, 0, :, 1, :] = 0.0
    cells[0, 0, 0, 1, 0] = 0.3                                   # below the first bin: (0.3 - 0.5) / 0.5 < 0 -> background
    cells[1, 0, :, 0, :] = 60.0                                  # beyond the last bin: background
    cells[1, 0, :, 1, :] = 0.0
    cells[1, 0, f - 1, 1, f - 1] = 1.0                           # exactly on an edge: bin 1 (channel 0)
    cells[2, 0, :, 0, :] = 0.0
    cells[2, 0, 0, 0, 0] = 41.0                                  # (41 - 0.5) / 0.5 = 81 = D + 1: out of range -> background
    cells[2, 0, :, 1, :] = 0.0
    cells[2, 0, 0, 1, 1] = 40.5                                  # the last bin's edge: bin 80
    cells[2, 0, 1, 1, 1] = 40.75
    gt = cells.reshape(B, N, H, W)
    onehot = _oracle_onehot(torch.from_numpy(gt), D_BOUND, f).numpy()
    bins = E.depth_cell_bins(gt.reshape(B * N, H, W), f, D_BOUND[0], D_BOUND[2], D).reshape(-1)
    assert bins[0] == 0 and bins[1] == 0 and bins[h * w] == 0 and bins[h * w + 1] == 1
    assert bins[2 * h * w] == 0 and bins[2 * h * w + 1] == 80
    want = np.where(onehot.max(1) > 0, onehot.argmax(1) + 1, 0)
    assert np.array_equal(bins, want)
    assert (bins > 0).sum() > 0 and (bins == 0).sum() > 0


def test_argmax_ties_go_to_the_lowest_index_and_nan_is_flagged():
    rows = np.array([[1.0, 3.0, 3.0, 2.0], [0.0, -0.0, -1.0, -1.0], [np.nan, 5.0, 1.0, 0.0], [-np.inf, -np.inf, -np.inf, -np.inf]],
                    np.float32)
    idx, nan = E.argmax_lowest(rows)
    assert idx[:2].tolist() == [1, 0] and idx[3] == 0 and nan.tolist() == [False, False, True, False]


def test_sequential_sums_are_not_pairwise():
    v = np.array([1e16, 1.0, -1e16, 1.0] * 64, np.float64)
    want = 0.0
    for x in v:
        want = want + x
    assert E.seq_sum(v) == want
    assert E.seq_sum(v[:3], 2.0) == ((2.0 + 1e16) + 1.0) - 1e16
