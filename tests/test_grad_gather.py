"""tt_grad_gather (csrc/grad_gather.hip): one launch gathers many separately allocated f32 arrays into one flat buffer,
    flat[dst_off_i .. + count_i)  (=|+=)  scale * src_i
against torch, BIT-EQUAL: the library is built with -ffp-contract=off, so `scale * src` and the sum are two separately
rounded operations like torch's `t = src * scale; dst + t`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

_NAN_BITS = 0x7FC0BEEF       # a quiet-NaN bit pattern with a payload


def _segments(seed, dev):
    """Seeded random segment set: counts of 1, 3 and 4097 and one above 2^22 among random ones; destination offsets that are odd
    multiples of 4 bytes; sources that are views at odd element offsets of a larger allocation as well as aligned ones; gaps
    (of 0 .. 9 elements, and one of several pieces' width) between the segments.  -> (srcs, dst_offs, flat_numel)."""
    g = torch.Generator().manual_seed(seed)
    counts = [1, 3, 4097, (1 << 22) + 5] + [int(c) for c in torch.randint(1, 70, (40,), generator=g)] + \
             [int(c) for c in torch.randint(100, 40000, (12,), generator=g)] + [64] * 16 + [4096, 8192, 2, 5]
    counts = [counts[i] for i in torch.randperm(len(counts), generator=g).tolist()]
    srcs, offs, off = [], [], 3                                   # (first destination offset: an odd multiple of 4 bytes)
    for i, n in enumerate(counts):
        shift = int(torch.randint(0, 4, (1,), generator=g)) if i % 3 else 1      # source view offsets 0 .. 3 elements
        base = torch.randn(n + 8, generator=g).to(dev)
        srcs.append(base[shift:shift + n])
        offs.append(off)
        gap = int(torch.randint(0, 10, (1,), generator=g))
        off += n + (3 * 4096 + 1 if i == 7 else gap)
    assert any(o % 2 == 1 for o in offs) and any(s.storage_offset() % 2 == 1 for s in srcs)
    assert any(b - (a + s.numel()) > 0 for a, b, s in zip(offs, offs[1:], srcs))
    return srcs, offs, off + 11


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("scale", [None, 0.37])
@pytest.mark.parametrize("seed", [0, 1])
def test_grad_gather_is_bit_equal_to_torch_and_leaves_gaps_alone(seed, scale, accumulate):
    from thinktwice_amd import ops
    dev = torch.device("cuda")
    srcs, offs, total = _segments(seed, dev)
    g = torch.Generator().manual_seed(100 + seed)
    before = torch.randn(total, generator=g).to(dev)
    covered = torch.zeros(total, dtype=torch.bool, device=dev)
    for s, o in zip(srcs, offs):
        covered[o:o + s.numel()] = True
    before.view(torch.int32)[~covered] = _NAN_BITS                # gaps: a NaN bit pattern that must come back untouched
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=dev)
    want = before.clone()
    for s, o in zip(srcs, offs):
        t = s * sc if sc is not None else s * 1.0                  # two separately rounded operations
        want[o:o + s.numel()] = (before[o:o + s.numel()] + t) if accumulate else t
    flat = before.clone()
    # handed over in shuffled order: the table is sorted by destination offset on the host
    perm = torch.randperm(len(srcs), generator=g).tolist()
    table = ops.GradSegTable(dev).upload([srcs[i] for i in perm], [offs[i] for i in perm], total)
    assert table.nseg == len(srcs)
    ops.grad_gather(table, flat, scale=sc, accumulate=bool(accumulate))
    torch.cuda.synchronize()
    got, exp = flat.view(torch.int32), want.view(torch.int32)
    bad = (got != exp).nonzero().flatten()
    assert bad.numel() == 0, (int(bad.numel()), bad[:8].tolist())
    assert bool((got[~covered] == _NAN_BITS).all())


def test_grad_gather_with_an_empty_table_returns_zero_and_launches_nothing():
    from thinktwice_amd import _lib, ops
    dev = torch.device("cuda")
    flat = torch.full((1000,), 7.0, device=dev)
    # the C entry itself: nseg == 0 -> 0, whatever the pointers (nothing is dereferenced, nothing launched)
    assert _lib.lib().tt_grad_gather(None, 0, _lib.ptr(flat), None, 0, _lib.cur_stream(dev)) == 0
    table = ops.GradSegTable(dev).upload([], [], flat.numel())
    assert table.nseg == 0
    ops.grad_gather(table, flat)
    torch.cuda.synchronize()
    assert bool((flat == 7.0).all())


def test_grad_gather_table_refuses_overlap_and_out_of_range_segments():
    """The kernel trusts its table: the host wrapper checks it (inside the flat buffer, no overlap) before anything is launched."""
    from thinktwice_amd import _lib, ops
    dev = torch.device("cuda")
    a, b = torch.zeros(10, device=dev), torch.zeros(10, device=dev)
    with pytest.raises(_lib.TTError):
        ops.GradSegTable(dev).upload([a, b], [0, 5], 100)
    with pytest.raises(_lib.TTError):
        ops.GradSegTable(dev).upload([a, b], [0, 95], 100)
    with pytest.raises(_lib.TTError):
        ops.GradSegTable(dev).upload([a.double()], [0], 100)
