"""Float64 references of the sparse LiDAR backward and the two map losses (tests/test_sparse_bwd.py, tests/test_loss_bwd.py), and
the rulebooks those tests run on.  Everything here runs on the CPU; tests/test_sparse_ref.py checks each piece against torch itself.

  * `rulebook`: tests/test_conv.py::_grid_rulebook generalised to a kernel, stride and padding per axis (the encoder's four
    geometries, GEOM); rows in (b, z, y, x) cell order, output coordinates returned.  On the two geometries _grid_rulebook
    knows, the same generator gives the same rulebook (asserted in test_sparse_ref.py);
  * `gather_matmul`: the sparse convolution as gather + matmul (differentiable: torch.autograd gives the input gradient);
  * `inverse_rulebook`, `assert_subm_symmetry`, `assert_inverse_unique`: the transposed rulebook of a strided layer and the two
    facts the product's input gradient relies on;
  * `sp_to_dense`, `sp_from_dense`: the dense layout (B, H, W, C * D), channel c * D + z, as index expressions;
  * `seg_focal`, `depth_bce`: the two map losses in float64 torch ops (oracle/train_ref.py's seg_loss / depth_loss; the depth bin
    in float32 exactly as the reference computes it).
"""
import functools

import torch
import torch.nn.functional as F

from test_conv import _grid_rulebook  # noqa: F401  (the builder this one generalises; compared in test_sparse_ref.py)

# the encoder's sparse geometries (thinktwice_amd/lidarnet.py SparseEncoder_fp32): kernel, stride, padding per (z, y, x) axis
GEOM = {
    "subm": dict(kernel=(3, 3, 3), stride=(1, 1, 1), pad=(1, 1, 1), subm=True),       # SubMConv3d: outputs = inputs
    "s2": dict(kernel=(3, 3, 3), stride=(2, 2, 2), pad=(1, 1, 1), subm=False),        # SparseConv3d, stride 2
    "s2p011": dict(kernel=(3, 3, 3), stride=(2, 2, 2), pad=(0, 1, 1), subm=False),    # the last down layer
    "k311": dict(kernel=(3, 1, 1), stride=(2, 1, 1), pad=(0, 0, 0), subm=False),      # conv_out
}


def occupancy(B, D, H, W, occ, g):
    """The occupancy draw of _grid_rulebook (same generator state -> same grid)."""
    return torch.rand(B, D, H, W, generator=g) < occ


def rulebook(vol, kernel=(3, 3, 3), stride=(1, 1, 1), pad=(1, 1, 1), subm=False):
    """vol bool [B, D, H, W] -> (nbr int32 [M, taps], out_coords int32 [M, 4] (b, z, y, x), rows_in).  Input row = rank of the
    cell among the occupied ones in (b, z, y, x) order; tap t = (kz * KY + ky) * KX + kx reads cell out * stride - pad + k.
    subm: the outputs are the inputs (stride 1, pad = kernel // 2); else every output cell whose window holds an input."""
    B, D, H, W = vol.shape
    (kz, ky, kx), (sz, sy, sx), (pz, py, px) = kernel, stride, pad
    rows_in = int(vol.sum())
    idx = torch.full((B, D, H, W), -1, dtype=torch.int64)
    idx[vol] = torch.arange(rows_in)
    padded = F.pad(idx, (px, px, py, py, pz, pz), value=-1)
    if subm:
        assert stride == (1, 1, 1) and pad == (kz // 2, ky // 2, kx // 2)
        oc = vol.nonzero()
    else:
        hit = F.max_pool3d(F.pad(vol.float()[:, None], (px, px, py, py, pz, pz)), kernel, stride)[:, 0] > 0
        assert tuple(hit.shape[1:]) == tuple((n + 2 * p - k) // s + 1 for n, p, k, s in zip((D, H, W), pad, kernel, stride))
        oc = hit.nonzero()
    b, z, y, x = oc.unbind(1)
    taps = [padded[b, z * sz + a, y * sy + c, x * sx + d] for a in range(kz) for c in range(ky) for d in range(kx)]
    return torch.stack(taps, 1).to(torch.int32), oc.to(torch.int32), rows_in


def out_dims(dims, kernel, stride, pad, subm=False):
    return tuple(dims) if subm else tuple((n + 2 * p - k) // s + 1 for n, p, k, s in zip(dims, pad, kernel, stride))


def gather_matmul(feats, nbr, w):
    """feats [R_in, Cin], nbr [M, taps] (-1 = no input), w [Cout, 1, taps, Cin] -> [M, Cout], in feats' dtype."""
    M, Cout = nbr.shape[0], w.shape[0]
    hit = (nbr >= 0).unsqueeze(-1)
    gathered = torch.where(hit, feats[nbr.clamp_min(0).long()], torch.zeros((), dtype=feats.dtype))
    return gathered.reshape(M, -1) @ w.reshape(Cout, -1).t()


def dense_conv3d(feats, vol, w, kernel, stride, pad):
    """The same layer as F.conv3d over the scattered grid: -> [B, Cout, oD, oH, oW]."""
    B, D, H, W = vol.shape
    Cout, Cin = w.shape[0], w.shape[-1]
    dense = torch.zeros(B, D, H, W, Cin, dtype=feats.dtype)
    dense[vol] = feats
    return F.conv3d(dense.permute(0, 4, 1, 2, 3), w.reshape(Cout, *kernel, Cin).permute(0, 4, 1, 2, 3), None, stride, pad)


def inverse_rulebook(nbr, live, rows):
    """inv int32 [rows, taps]: inv[j][t] = m for the live rows m < live with nbr[m][t] == j, -1 elsewhere (tt_sp_inverse_rulebook)."""
    M, taps = nbr.shape
    live = max(0, min(int(live), M))
    inv = torch.full((rows, taps), -1, dtype=torch.int32)
    sub = nbr[:live].long()
    m, t = (sub >= 0).nonzero(as_tuple=True)
    inv[sub[m, t], t] = m.to(torch.int32)
    return inv


def assert_subm_symmetry(nbr):
    """nbr[m][t] == j  <=>  nbr[j][taps - 1 - t] == m: what lets a submanifold layer's input gradient reuse the layer's own
    rulebook with the weight flipped along the taps.  (Stated for every entry, so both directions are covered.)"""
    taps = nbr.shape[1]
    sub = nbr.long()
    m, t = (sub >= 0).nonzero(as_tuple=True)
    assert m.numel() > 0
    assert torch.equal(sub[sub[m, t], taps - 1 - t], m), "submanifold rulebook is not tap-symmetric"


def assert_inverse_unique(nbr, rows_in):
    """At most one output row m for every (input row j, tap t): what lets the transposed rulebook hold one index per entry."""
    taps = nbr.shape[1]
    sub = nbr.long()
    m, t = (sub >= 0).nonzero(as_tuple=True)
    assert m.numel() > 0 and int(sub.max()) < rows_in
    key = sub[m, t] * taps + t
    assert key.unique().numel() == key.numel(), "two output rows read the same input row through the same tap"


def sp_to_dense(x, coords, live, dims, B):
    """x [R, C], coords [R, 4] (b, z, y, x), the first `live` rows -> (B, H, W, C * D), channel c * D + z; other cells zero."""
    D, H, W = dims
    C = x.shape[1]
    c = coords[:live].long()
    dense = torch.zeros(B, H, W, C, D, dtype=x.dtype)
    dense[c[:, 0], c[:, 2], c[:, 3], :, c[:, 1]] = x[:live]
    return dense.reshape(B, H, W, C * D)


def sp_from_dense(g, coords, live, dims):
    """The rows of the dense gradient g (B, H, W, C * D) at the first `live` coordinates -> [live, C]."""
    D, H, W = dims
    B = g.shape[0]
    c = coords[:live].long()
    return g.reshape(B, H, W, -1, D)[c[:, 0], c[:, 2], c[:, 3], :, c[:, 1]]


# ----------------------------------------------------------------------------- the two map losses
def seg_focal(logits, labels, factor=2):
    """logits [BN, h, w, C] (the class columns only), labels [B, N, H, W] float class ids (255 = ignore) sampled at
    (y * factor, x * factor) -> (10 * 0.5 * (1 - e^-u)^2 * u, u = mean cross entropy over the contributing pixels, their count)."""
    B, N, H, W = labels.shape
    BN, h, w, C = logits.shape
    assert (BN, h, w) == (B * N, H // factor, W // factor)
    gt = labels.reshape(BN, H, W)[:, :h * factor:factor, :w * factor:factor].long()
    keep = gt != 255
    ce = torch.logsumexp(logits, -1) - logits.gather(-1, gt.clamp(0, C - 1).unsqueeze(-1)).squeeze(-1)
    cnt = int(keep.sum())
    u = (ce * keep).sum() / cnt
    pt = torch.exp(-u)
    return (1 - pt) ** 2 * 0.5 * u * 10, u, cnt


def depth_bins(gt_depth, d_bound, factor):
    """[B, N, H, W] f32 metres -> long [BN, h, w]: 0 = background, 1 .. D = depth bin + 1.  Float32 throughout, the expression of
    oracle/train_ref.py depth_loss (per cell the smallest non-zero return; (g - (d0 - step)) / step; outside [0, D + 1) -> 0)."""
    B, N, H, W = gt_depth.shape
    D = int((d_bound[1] - d_bound[0]) / d_bound[2])
    g = gt_depth.float().view(B * N, H // factor, factor, W // factor, factor).permute(0, 1, 3, 2, 4).reshape(-1, factor * factor)
    g = torch.min(torch.where(g == 0.0, 1e5 * torch.ones_like(g), g), dim=-1).values.view(B * N, H // factor, W // factor)
    g = (g - (d_bound[0] - d_bound[2])) / d_bound[2]
    g = torch.where((g < D + 1) & (g >= 0.0), g, torch.zeros_like(g))
    return g.long()


def depth_bce(logits, gt_depth, d_bound, factor=16):
    """logits [BN, h, w, D] (the bin columns only) -> (sum over the foreground cells and bins of BCE-with-logits against the one-hot
    bin / max(1, #foreground), that divisor, the bins [BN, h, w])."""
    D = logits.shape[-1]
    bins = depth_bins(gt_depth, d_bound, factor)
    fg = bins >= 1
    onehot = F.one_hot(bins, D + 1)[..., 1:].to(logits.dtype)
    div = max(1, int(fg.sum()))
    loss = (F.binary_cross_entropy_with_logits(logits, onehot, reduction="none") * fg.unsqueeze(-1)).sum() / div
    return loss, div, bins


# ----------------------------------------------------------------------------- the rulebooks of tests/test_sparse_bwd.py
# Input-gradient cases: name -> (geometry, Cin -> Cout of the FORWARD layer, grid (B, D, H, W), occupancy, rows allocated for the
# level whose gradient is written: "l2" = kSpL2MinRows + 37 (the weight-resident kernel is chosen by allocated rows), else live + n).
# Grids as the forward tests use them (tests/test_conv.py, tests/test_sp_conv_l2.py).
DGRAD_CASES = {
    "subm 16->16": ("subm", 16, 16, (2, 10, 60, 60), 0.10, "l2"),
    "subm 32->32": ("subm", 32, 32, (2, 10, 60, 60), 0.10, 300),
    "subm 64->64": ("subm", 64, 64, (2, 6, 40, 44), 0.65, 300),
    "subm 128->128": ("subm", 128, 128, (3, 3, 30, 34), 0.85, 300),
    "subm 8->16 input layer": ("subm", 8, 16, (2, 10, 60, 60), 0.10, 300),      # 5 point features padded to 8 by lidarnet._sp_weight
    "subm 32->32 small": ("subm", 32, 32, (1, 4, 20, 20), 0.50, 37),           # < 2048 rows: the small-M route
    "s2 16->32": ("s2", 16, 32, (2, 11, 60, 60), 0.10, "l2"),
    "s2 32->64": ("s2", 32, 64, (2, 11, 60, 60), 0.10, 300),
    "s2p011 64->64": ("s2p011", 64, 64, (2, 5, 44, 40), 0.65, 300),
    "k311 64->128": ("k311", 64, 128, (2, 5, 30, 34), 0.65, 300),
}
# further rulebooks of the inverse-rulebook cases: name -> (geometry, grid, occupancy)
INVERSE_CASES = {
    "27 taps": ("s2", (2, 5, 12, 13), 0.30),
    "27 taps pad 011": ("s2p011", (1, 5, 9, 11), 0.50),
    "3 taps": ("k311", (2, 5, 7, 9), 0.60),
}


@functools.lru_cache(maxsize=None)
def case_rulebook(name):
    """-> dict(nbr [live_out, taps], coords, rows_in, vol, geom) of a DGRAD_CASES / INVERSE_CASES entry."""
    if name in DGRAD_CASES:
        geom, _, _, dims, occ, _ = DGRAD_CASES[name]
    else:
        geom, dims, occ = INVERSE_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    vol = occupancy(*dims, occ, g)
    nbr, coords, rows_in = rulebook(vol, **GEOM[geom])
    return dict(nbr=nbr, coords=coords, rows_in=rows_in, vol=vol, geom=GEOM[geom])


def all_rulebook_names():
    return list(DGRAD_CASES) + list(INVERSE_CASES)


def min_l2_rows():
    """kSpL2MinRows of csrc/conv_choose.h: allocated rows from which the 16- / 32-channel layers take the weight-resident kernel."""
    import os
    import re
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    return int(re.search(r"kSpL2MinRows\s*=\s*(\d+)", open(os.path.join(root, "thinktwice_amd", "csrc", "conv_choose.h")).read()).group(1))


def dgrad_sizes(name):
    """Live and allocated rows of the two levels of a DGRAD_CASES entry, and the launch of its input gradient:
    dict(live_out, out_alloc, live_in, in_alloc, taps, strided)."""
    geom, _, _, _, _, alloc = DGRAD_CASES[name]
    rb = case_rulebook(name)
    live_out, live_in = rb["nbr"].shape[0], rb["rows_in"]
    in_alloc = max(min_l2_rows(), live_in) + 37 if alloc == "l2" else live_in + alloc
    strided = not GEOM[geom]["subm"]
    return dict(live_out=live_out, out_alloc=live_out + 41 if strided else in_alloc, live_in=live_in, in_alloc=in_alloc,
                taps=rb["nbr"].shape[1], strided=strided)


@functools.lru_cache(maxsize=None)
def dgrad_reference(name):
    """The float64 input gradient of a DGRAD_CASES entry, computed once: dict(w f32 [Cout,1,taps,Cin], dconv f32 [live_out, Cout]
    (scaled by a power of two so that |ref| <= 4), ref / asum float64 [live_in, Cin] (vjp of gather_matmul; the same with |dconv|
    and |w|: the sum of the absolute addends), n [live_in] the number of live (tap, channel) addends of every row)."""
    _, Cin, Cout, _, _, _ = DGRAD_CASES[name]
    rb = case_rulebook(name)
    nbr, rows_in = rb["nbr"], rb["rows_in"]
    taps = nbr.shape[1]
    g = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    w = torch.randn(Cout, 1, taps, Cin, generator=g) * (taps * Cin) ** -0.5
    if "input layer" in name:
        w[..., 5:] = 0.0                      # lidarnet._sp_weight pads the five point features with zero weights
    dconv = torch.randn(nbr.shape[0], Cout, generator=g)
    x0 = torch.zeros(rows_in, Cin)

    def grad(wt, dy):
        leaf = x0.double().requires_grad_(True)
        gather_matmul(leaf, nbr, wt.double()).backward(dy.double())
        return leaf.grad

    ref = grad(w, dconv)
    s = 1.0
    while float(ref.abs().max()) * s > 4.0:
        s *= 0.5
    dconv = dconv * s
    n = torch.zeros(rows_in, dtype=torch.long)
    hit = nbr >= 0
    n.index_add_(0, nbr[hit].long(), torch.ones(int(hit.sum()), dtype=torch.long))
    return dict(w=w, dconv=dconv, ref=ref * s, asum=grad(w.abs(), dconv.abs()), n=n * Cout)
