"""csrc/sp_conv_l2.hip: the weight-resident gather kernel of the 16- / 32-channel sparse 3x3x3 convolutions (bf16x3).

The kernel is chosen from kSpL2MinRows ALLOCATED rows on (csrc/conv_choose.h), so every case here allocates that many rows and
keeps only a few thousand of them live: the rulebook rows beyond the live count hold garbage and must be neither read as
neighbours nor written.  Rulebooks come from tests/test_conv.py::_grid_rulebook (imported, not copied)."""
import functools
import os
import re

import pytest
import torch

from test_conv import _grid_rulebook

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MIN_ROWS = int(re.search(r"kSpL2MinRows\s*=\s*(\d+)", open(os.path.join(ROOT, "thinktwice_amd", "csrc", "conv_choose.h")).read()).group(1))
FILL = 123.0
NEW, OLD = "sp_conv_runs_l2_kernel", "sp_conv_runs_kernel"


def _run(feats, nbr, live, M, w, *, scale=None, shift=None, res=None, act=0, stride=1, seed=0, window=None):
    """ops.gather_conv over an allocation of M rows whose first `live` rows are `nbr` and whose other rows are garbage.
    window = (cstride, coff): the layer reads channels [coff, coff + Cin) of a wider [rows, cstride] buffer.
    -> (output [M, Cout] on the CPU, label of the kernel that ran)."""
    from thinktwice_amd import _lib, ops, weights
    g = torch.Generator().manual_seed(1000 + seed)
    alloc = torch.randint(-5, 10 ** 6, (M, 27), generator=g, dtype=torch.int32)
    alloc[:nbr.shape[0]] = nbr
    Cout = w.shape[0]
    wd = w.cuda()
    out = torch.full((M, Cout), FILL, device="cuda")
    fd = feats.cuda()
    L = _lib.lib()
    real = L.tt_conv2d_fwd
    wide = None
    if window is not None:
        cs, coff = window
        wide = torch.randn(feats.shape[0], cs, generator=g)
        wide[:, coff:coff + feats.shape[1]] = feats
        wide = wide.cuda()

        def spy(d, stream):      # ops.gather_conv describes a dense [rows, Cin] input: point the descriptor at the window
            d._obj.in_, d._obj.in_cstride, d._obj.in_coff = wide.data_ptr(), cs, coff
            return real(d, stream)
        L.tt_conv2d_fwd = spy
    try:
        ops.gather_conv(fd, alloc.cuda(), torch.tensor([live], dtype=torch.int32).cuda(), wd,
                        scale=None if scale is None else scale.cuda(), shift=None if shift is None else shift.cuda(), act=act,
                        res=None if res is None else res.cuda(), w_x3=weights.split_pairs_x3(wd), out=out, stride=stride)
        torch.cuda.synchronize()
    finally:
        L.tt_conv2d_fwd = real
    return out.cpu(), ops._last_conv_kernel()


def _reference(feats, nbr, w, scale, shift, res, act):
    """gather + matmul in f32 on the CPU, as tests/test_conv.py restates the sparse conv"""
    live, Cout = nbr.shape[0], w.shape[0]
    gathered = torch.where((nbr >= 0).unsqueeze(-1), feats[nbr.clamp_min(0).long()], torch.zeros(()))
    ref = gathered.reshape(live, -1) @ w.reshape(Cout, -1).t()
    if scale is not None:
        ref = ref * scale
    if shift is not None:
        ref = ref + shift
    if res is not None:
        ref = ref + res[:live]
    return torch.relu(ref) if act == 1 else ref


@functools.lru_cache(maxsize=None)
def _level2():
    """32 -> 32, stride 1, occupancy 0.10 on (2, 10, 60, 60): ~7,200 live rows, not a multiple of 32"""
    g = torch.Generator().manual_seed(65)
    nbr, rows_in = _grid_rulebook(2, 10, 60, 60, 0.10, 1, g)
    if nbr.shape[0] % 32 == 0:
        nbr = nbr[:-1]
    feats = torch.randn(rows_in, 32, generator=g)
    w = torch.randn(32, 1, 27, 32, generator=g) * (27 * 32) ** -0.5
    scale = torch.rand(32, generator=g) + 0.5
    shift = torch.randn(32, generator=g) * 0.3
    res = torch.randn(MIN_ROWS + 37, 32, generator=g)
    return nbr, feats, w, scale, shift, res


@pytest.mark.parametrize("use_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", [0, 1], ids=["linear", "relu"])
def test_bit_identical_to_the_run_staged_kernel(use_res, act):
    """The same live rows through both kernels: allocation live + 300 takes the run-staged kernel, allocation kSpL2MinRows + 37 the
    weight-resident one.  Cell-ordered SubM rulebook, Cin = 32: the two add a row's non-zero products in the same order."""
    nbr, feats, w, scale, shift, res = _level2()
    live = nbr.shape[0]
    assert 2048 <= live and live + 300 < MIN_ROWS and live % 32 != 0
    kw = dict(scale=scale, shift=shift, act=act)
    old, k_old = _run(feats, nbr, live, live + 300, w, res=res[:live + 300] if use_res else None, **kw)
    new, k_new = _run(feats, nbr, live, MIN_ROWS + 37, w, res=res if use_res else None, **kw)
    assert k_old.startswith(OLD + "<"), k_old
    assert k_new.startswith(NEW + "<"), k_new
    assert torch.equal(old[:live], new[:live])
    assert bool((old[live:] == FILL).all()) and bool((new[live:] == FILL).all())


CASES = {
    # name: (Cin, Cout, stride, occupancy, dims)
    "16to16 isolated": (16, 16, 1, 0.02, (2, 10, 100, 100)),      # ~1 pair per row: most taps are skipped wave-wide
    "16to32 stride2": (16, 32, 2, 0.10, (2, 11, 60, 60)),
    "32to64 stride2": (32, 64, 2, 0.10, (2, 11, 60, 60)),         # two column tiles
    "32to32 shuffled": (32, 32, 1, 0.10, (2, 10, 60, 60)),        # rows of the rulebook and of the input in random order
    "32to32 live1": (32, 32, 1, 0.10, (1, 4, 20, 20)),
    "32to32 live0": (32, 32, 1, 0.10, (1, 4, 20, 20)),
    "32to32 window": (32, 32, 1, 0.10, (2, 6, 40, 40)),           # in_cstride 48 > Cin, in_coff 8
    "16to64 window": (16, 64, 1, 0.10, (2, 6, 40, 40)),           # in_cstride 40, in_coff 20
}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_f32_restatement(name):
    """Every allocation >= kSpL2MinRows with a few thousand live rows; err < 1e-4 of the output's max: the project's bound for
    bf16x3 at these K (tests/test_conv.py)."""
    Cin, Cout, stride, occ, dims = CASES[name]
    g = torch.Generator().manual_seed(len(name) * 131 + Cin + Cout)
    nbr, rows_in = _grid_rulebook(*dims, occ, stride, g)
    feats = torch.randn(rows_in, Cin, generator=g)
    if "shuffled" in name:
        pin = torch.randperm(rows_in, generator=g)            # input row j moves to row pin[j]
        f2 = torch.empty_like(feats)
        f2[pin] = feats
        feats = f2
        nbr = torch.where(nbr >= 0, pin[nbr.clamp_min(0).long()].to(torch.int32), nbr)
        nbr = nbr[torch.randperm(nbr.shape[0], generator=g)]
    live = {"live1": 1, "live0": 0}.get(name.split()[-1], nbr.shape[0])
    nbr = nbr[:live]
    # allocations of 40,000 / 70,000 rows launch the full persistent grid (128 x 2 / 256 workgroups), most of which find no live
    # group; the others launch 65 workgroups
    M = {"32to64 stride2": 40000, "32to32 shuffled": 70000}.get(name, max(MIN_ROWS, live) + 37)
    assert M >= MIN_ROWS and M >= live
    w = torch.randn(Cout, 1, 27, Cin, generator=g) * (27 * Cin) ** -0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(Cout, generator=g) * 0.3
    res = torch.randn(M, Cout, generator=g)
    window = {"32to32 window": (48, 8), "16to64 window": (40, 20)}.get(name)
    got, kern = _run(feats, nbr, live, M, w, scale=scale, shift=shift, res=res, act=1, stride=stride, window=window)
    assert kern == f"{NEW}<{Cin}>", kern
    assert bool((got[live:] == FILL).all())                   # rows beyond the live count are not written
    if live:
        ref = _reference(feats, nbr, w, scale, shift, res, 1)
        err = float((got[:live] - ref).abs().max() / ref.abs().max())
        print(f"{name}: live {live} of {M}, err {err:.3e}")
        assert err < 1e-4, err
