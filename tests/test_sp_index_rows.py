"""The row-wise rulebook and the bitmap output sets of csrc/lidar.hip (tt_sp_volume_build, tt_sp_strided_outputs, tt_sp_rulebook)
against a torch restatement on the CPU of the definitions in that file's comments: the output set of a strided conv is the set of
cells some input reaches through some tap, row ids are the rank in cell order (b, z, y, x), nbr comes from the dense volume.  Every
tensor is compared with torch.equal.

Shapes: batch 2 with dims that are neither powers of two nor multiples of the stride; x = 33 and 71 put a bitmap word across x rows
and batches.  (5, 9, 11) and (4, 10, 33) fit one 8192-cell tile of the compaction; (11, 45, 71) gives every geometry at least two
tiles (8280 .. 70290 output cells) and tens of thousands of rows, so the carry across workgroups of the compaction and the
256-row blocks of the rulebook are exercised.  Guard words follow nbr, out_coords and vol; every strided case runs twice."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
SMALL = [(5, 9, 11), (4, 10, 33)]
LARGE = (11, 45, 71)
GEOMS = {"3x3x3 s1 p1": ((3, 3, 3), (1, 1, 1), (1, 1, 1)),
         "3x3x3 s2 p1": ((3, 3, 3), (2, 2, 2), (1, 1, 1)),
         "3x3x3 s2 p011": ((3, 3, 3), (2, 2, 2), (0, 1, 1)),
         "3x1x1 s211 p0": ((3, 1, 1), (2, 1, 1), (0, 0, 0)),
         "3x3x3 s122 p1 (generic)": ((3, 3, 3), (1, 2, 2), (1, 1, 1))}
OCCS = ["5%", "60%", "full", "last cell", "empty", "dead rows", "clamped"]
GUARD, FILL = 64, -7


def _ci(*v):
    return (ctypes.c_int * len(v))(*v)


def _level(dims, occ, seed):
    """-> (coords [max_rows, 4] int32 in cell order, live count).  "dead rows": the allocation is much larger than the live count
    and its dead rows hold coordinates of OTHER cells, so a kernel that read them would change the result, not fault."""
    g = torch.Generator().manual_seed(seed)
    if occ == "full":
        grid = torch.ones(B, *dims, dtype=torch.bool)
    elif occ == "last cell":
        grid = torch.zeros(B, *dims, dtype=torch.bool)
        grid[-1, -1, -1, -1] = True
    elif occ == "empty":
        grid = torch.zeros(B, *dims, dtype=torch.bool)
    else:
        grid = torch.rand(B, *dims, generator=g) < {"5%": 0.05, "60%": 0.6, "dead rows": 0.3, "clamped": 0.6}[occ]
    live = grid.nonzero().to(torch.int32)
    spare = 700 if occ == "dead rows" else 37
    junk = torch.stack([torch.randint(0, n, (spare,), generator=g, dtype=torch.int32) for n in (B, *dims)], 1)
    return torch.cat([live, junk]).contiguous(), live.shape[0]


def _out_dims(dims, geom):
    k, s, p = geom
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip(dims, k, s, p))


def _taps(k):
    return [(kz, ky, kx) for kz in range(k[0]) for ky in range(k[1]) for kx in range(k[2])]


def _ref_volume(coords, n, dims):
    vol = torch.full((B, *dims), -1, dtype=torch.int32)
    c = coords[:n].long()
    vol[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = torch.arange(n, dtype=torch.int32)
    return vol


def _ref_outputs(coords, n, geom, od, max_out):
    """-> (out coords of the rows below max_out, clamped live count, output volume, unclamped count)"""
    k, s, p = geom
    flags = torch.zeros((B, *od), dtype=torch.bool)
    c = coords[:n].long()
    for kz, ky, kx in _taps(k):
        nz, ny, nx = c[:, 1] + p[0] - kz, c[:, 2] + p[1] - ky, c[:, 3] + p[2] - kx
        ok = (nz >= 0) & (ny >= 0) & (nx >= 0) & (nz % s[0] == 0) & (ny % s[1] == 0) & (nx % s[2] == 0)
        oz, oy, ox = nz // s[0], ny // s[1], nx // s[2]
        ok &= (oz < od[0]) & (oy < od[1]) & (ox < od[2])
        flags[c[ok, 0], oz[ok], oy[ok], ox[ok]] = True
    oc = flags.nonzero().to(torch.int32)               # nonzero() lists cells in (b, z, y, x) order: the rank is the row id
    rows = min(oc.shape[0], max_out)
    vol = torch.full((B, *od), -1, dtype=torch.int32)
    o = oc[:rows].long()
    vol[o[:, 0], o[:, 1], o[:, 2], o[:, 3]] = torch.arange(rows, dtype=torch.int32)
    return oc[:rows], rows, vol, oc.shape[0]


def _ref_rulebook(out_coords, rows, geom, in_vol, dims):
    k, s, p = geom
    o = out_coords[:rows].long()
    cols = []
    for kz, ky, kx in _taps(k):
        z, y, x = o[:, 1] * s[0] - p[0] + kz, o[:, 2] * s[1] - p[1] + ky, o[:, 3] * s[2] - p[2] + kx
        ok = (z >= 0) & (z < dims[0]) & (y >= 0) & (y < dims[1]) & (x >= 0) & (x < dims[2])
        r = in_vol[o[:, 0], z.clamp(0, dims[0] - 1), y.clamp(0, dims[1] - 1), x.clamp(0, dims[2] - 1)]
        cols.append(torch.where(ok, r, torch.full_like(r, -1)))
    return torch.stack(cols, 1).reshape(-1)


def _buf(n, shift):
    """n int32 words followed by GUARD guard words, all FILL; shift = 1 starts the buffer 4 bytes off a 16-byte boundary"""
    return torch.full((n + GUARD + shift,), FILL, dtype=torch.int32, device="cuda")[shift:]


def _dev_ints(t, shift):
    d = _buf(t.numel(), shift)
    d[:t.numel()] = t.reshape(-1).cuda()
    return d


def _gpu_volume(cd, rows, max_rows, dims, shift):
    from thinktwice_amd import ops
    from thinktwice_amd._lib import check, lib, ptr
    cells = B * dims[0] * dims[1] * dims[2]
    vol = _buf(cells, shift)
    check(lib().tt_sp_volume_build(ptr(cd), ptr(rows), max_rows, B, _ci(*dims), ptr(vol), ops.cur_stream(cd.device)),
          "tt_sp_volume_build")
    return vol


def _gpu_rulebook(out_coords, out_rows, max_out, geom, in_dims, in_vol, shift):
    from thinktwice_amd import ops
    from thinktwice_amd._lib import check, lib, ptr
    KV = geom[0][0] * geom[0][1] * geom[0][2]
    nbr = _buf(max_out * KV, shift)
    check(lib().tt_sp_rulebook(ptr(out_coords), ptr(out_rows), max_out, _ci(*geom[0], *geom[1], *geom[2]), _ci(*in_dims),
                               ptr(in_vol), ptr(nbr), ops.cur_stream(nbr.device)), "tt_sp_rulebook")
    torch.cuda.synchronize()
    return nbr.cpu()


def _gpu_outputs(cd, rows, max_in, geom, od, max_out, shift):
    from thinktwice_amd import ops
    from thinktwice_amd._lib import check, lib, ptr
    cells = B * od[0] * od[1] * od[2]
    ws_bytes = int(lib().tt_sp_strided_outputs_workspace_bytes(cells))
    ws = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device="cuda")       # the workspace arrives dirty
    ovol, ocoords = _buf(cells, shift), _buf(max_out * 4, shift)
    orows = torch.full((1,), FILL, dtype=torch.int32, device="cuda")
    check(lib().tt_sp_strided_outputs(ptr(cd), ptr(rows), max_in, B, _ci(*geom[0], *geom[1], *geom[2]), _ci(*od), ptr(ws), ws_bytes,
                                      ptr(ovol), ptr(ocoords), ptr(orows), max_out, ops.cur_stream(cd.device)),
          "tt_sp_strided_outputs")
    torch.cuda.synchronize()
    return ovol, ocoords, orows


def _check_case(dims, geom, occ, shift=0):
    coords, n = _level(dims, occ, seed=5)
    max_in = coords.shape[0]
    cd = _dev_ints(coords, shift)
    rows = torch.tensor([n], dtype=torch.int32).cuda()
    ref_vol = _ref_volume(coords, n, dims)
    in_cells = ref_vol.numel()
    vol = _gpu_volume(cd, rows, max_in, dims, shift)
    vol_h = vol.cpu()
    assert torch.equal(vol_h[:in_cells].view(B, *dims), ref_vol)
    assert bool((vol_h[in_cells:] == FILL).all())

    if geom[1] == (1, 1, 1):       # the SubM use: the level's own rows, its dead rows included in the allocation
        nbr = _gpu_rulebook(cd, rows, max_in, geom, dims, vol, shift)
        ref = _ref_rulebook(coords, n, geom, ref_vol, dims)
        assert torch.equal(nbr[:ref.numel()], ref)
        assert bool((nbr[ref.numel():] == FILL).all())          # dead rows and the guard stay unwritten

    od = _out_dims(dims, geom)
    cells = B * od[0] * od[1] * od[2]
    active = _ref_outputs(coords, n, geom, od, cells)[3]
    max_out = max(active - 1, 1) if occ == "clamped" else active + 9
    ref_coords, ref_rows, ref_ovol, _ = _ref_outputs(coords, n, geom, od, max_out)
    assert occ != "clamped" or ref_rows == active - 1
    first = None
    for _ in range(2):
        ovol, ocoords, orows = _gpu_outputs(cd, rows, max_in, geom, od, max_out, shift)
        got = (ovol.cpu(), ocoords.cpu(), orows.cpu())
        assert int(got[2]) == ref_rows
        assert torch.equal(got[1][:ref_rows * 4], ref_coords.reshape(-1))
        assert bool((got[1][ref_rows * 4:] == FILL).all())
        assert torch.equal(got[0][:cells].view(B, *od), ref_ovol)         # -1 in empty cells and in cells past the clamp
        assert bool((got[0][cells:] == FILL).all())
        if first is not None:
            assert all(torch.equal(a, b) for a, b in zip(first, got))
        first = got
    nbr = _gpu_rulebook(ocoords, orows, max_out, geom, dims, vol, shift)
    ref = _ref_rulebook(ref_coords, ref_rows, geom, ref_vol, dims)
    assert torch.equal(nbr[:ref.numel()], ref)
    assert bool((nbr[ref.numel():] == FILL).all())


@pytest.mark.parametrize("occ", OCCS)
@pytest.mark.parametrize("geom", list(GEOMS), ids=list(GEOMS))
@pytest.mark.parametrize("dims", SMALL, ids=lambda d: "x".join(map(str, d)))
def test_small_grids(dims, geom, occ):
    _check_case(dims, GEOMS[geom], occ)


@pytest.mark.parametrize("occ", ["5%", "60%", "dead rows", "clamped"])
@pytest.mark.parametrize("geom", list(GEOMS), ids=list(GEOMS))
def test_several_workgroups(geom, occ):
    _check_case(LARGE, GEOMS[geom], occ)


@pytest.mark.parametrize("occ", ["5%", "clamped"])
def test_bitmap_above_the_direct_count_size(occ):
    """538,200 output cells = 66 tiles of 8192: above the 64 tiles up to which the compaction counts the bitmap itself, so the
    per-workgroup totals come from the count launch (the model's first strided level, 19 M cells, takes this path too)"""
    _check_case((23, 90, 130), GEOMS["3x3x3 s1 p1"], occ)


@pytest.mark.parametrize("geom", list(GEOMS), ids=list(GEOMS))
def test_arrays_off_a_16_byte_boundary(geom):
    """coords, vol, out_coords and nbr 4 bytes past a 16-byte boundary: the kernels' scalar load / store forms"""
    _check_case(SMALL[1], GEOMS[geom], "60%", shift=1)
