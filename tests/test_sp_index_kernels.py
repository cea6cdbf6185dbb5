"""The index kernels of the sparse LiDAR levels (csrc/lidar.hip): tt_sp_volume_build, tt_sp_strided_outputs and tt_sp_rulebook
against a torch restatement on the CPU, compared with torch.equal -- same row order, same -1s, same live count.  Small odd grids:
B = 2 with dims (5, 13, 17)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

B, DIMS = 2, (5, 13, 17)
SUBM = ((3, 3, 3), (1, 1, 1), (1, 1, 1))
DOWN = ((3, 3, 3), (2, 2, 2), (0, 1, 1))
OUTC = ((3, 1, 1), (2, 1, 1), (0, 0, 0))


def _ci(*v):
    return (ctypes.c_int * len(v))(*v)


def _level(occ, seed, spare=50):
    """Cell-ordered coords (b, z, y, x) of a random occupancy grid in an allocation of live + spare rows.  The rows beyond the live
    count hold valid coordinates of OTHER cells: a kernel that read them would change the result, not fault."""
    g = torch.Generator().manual_seed(seed)
    vol = torch.rand(B, *DIMS, generator=g) < occ
    live = vol.nonzero().to(torch.int32)
    junk = torch.stack([torch.randint(0, n, (spare,), generator=g, dtype=torch.int32) for n in (B, *DIMS)], 1)
    return torch.cat([live, junk]).contiguous(), live.shape[0]


def _out_dims(dims, geom):
    k, s, p = geom
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip(dims, k, s, p))


def _ref_volume(coords, n, dims):
    vol = torch.full((B, *dims), -1, dtype=torch.int32)
    c = coords[:n].long()
    vol[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = torch.arange(n, dtype=torch.int32)
    return vol


def _ref_outputs(coords, n, geom, od, max_out):
    """active outputs o: some input i and tap k with i = o * s - p + k; rows in cell order, clamped to max_out"""
    k, s, p = geom
    flags = torch.zeros((B, *od), dtype=torch.bool)
    c = coords[:n].long()
    for kz in range(k[0]):
        for ky in range(k[1]):
            for kx in range(k[2]):
                nz, ny, nx = c[:, 1] + p[0] - kz, c[:, 2] + p[1] - ky, c[:, 3] + p[2] - kx
                ok = (nz >= 0) & (ny >= 0) & (nx >= 0) & (nz % s[0] == 0) & (ny % s[1] == 0) & (nx % s[2] == 0)
                oz, oy, ox = nz // s[0], ny // s[1], nx // s[2]
                ok &= (oz < od[0]) & (oy < od[1]) & (ox < od[2])
                flags[c[ok, 0], oz[ok], oy[ok], ox[ok]] = True
    oc = flags.nonzero().to(torch.int32)
    rows = min(oc.shape[0], max_out)
    vol = torch.full((B, *od), -1, dtype=torch.int32)
    o = oc[:rows].long()
    vol[o[:, 0], o[:, 1], o[:, 2], o[:, 3]] = torch.arange(rows, dtype=torch.int32)
    return oc[:rows], rows, vol


def _ref_rulebook(out_coords, rows, geom, in_vol, dims):
    k, s, p = geom
    o = out_coords[:rows].long()
    taps = []
    for kz in range(k[0]):
        for ky in range(k[1]):
            for kx in range(k[2]):
                z, y, x = o[:, 1] * s[0] - p[0] + kz, o[:, 2] * s[1] - p[1] + ky, o[:, 3] * s[2] - p[2] + kx
                ok = (z >= 0) & (z < dims[0]) & (y >= 0) & (y < dims[1]) & (x >= 0) & (x < dims[2])
                r = in_vol[o[:, 0], z.clamp(0, dims[0] - 1), y.clamp(0, dims[1] - 1), x.clamp(0, dims[2] - 1)]
                taps.append(torch.where(ok, r, torch.full_like(r, -1)))
    return torch.stack(taps, 1) if rows else torch.empty(0, len(taps), dtype=torch.int32)


def _gpu_volume(coords, n, max_rows, dims):
    from thinktwice_amd import ops
    from thinktwice_amd._lib import check, lib, ptr
    cd = coords.cuda()
    rows = torch.tensor([n], dtype=torch.int32).cuda()
    vol = torch.empty(B * dims[0] * dims[1] * dims[2], dtype=torch.int32, device="cuda")
    check(lib().tt_sp_volume_build(ptr(cd), ptr(rows), max_rows, B, _ci(*dims), ptr(vol), ops.cur_stream(cd.device)),
          "tt_sp_volume_build")
    return cd, rows, vol


def _gpu_rulebook(out_coords, out_rows, max_out, geom, in_dims, in_vol):
    from thinktwice_amd import ops
    from thinktwice_amd._lib import check, lib, ptr
    KV = geom[0][0] * geom[0][1] * geom[0][2]
    nbr = torch.full((max_out, KV), -7, dtype=torch.int32, device="cuda")
    check(lib().tt_sp_rulebook(ptr(out_coords), ptr(out_rows), max_out, _ci(*geom[0], *geom[1], *geom[2]), _ci(*in_dims),
                               ptr(in_vol), ptr(nbr), ops.cur_stream(nbr.device)), "tt_sp_rulebook")
    torch.cuda.synchronize()
    return nbr.cpu()


@pytest.mark.parametrize("occ", [0.3, 0.0], ids=["occupied", "empty"])
def test_volume_and_subm_rulebook(occ):
    coords, n = _level(occ, 3)
    max_rows = coords.shape[0]
    cd, rows, vol = _gpu_volume(coords, n, max_rows, DIMS)
    ref_vol = _ref_volume(coords, n, DIMS)
    assert torch.equal(vol.cpu().view(B, *DIMS), ref_vol)
    nbr = _gpu_rulebook(cd, rows, max_rows, SUBM, DIMS, vol)
    assert torch.equal(nbr[:n], _ref_rulebook(coords, n, SUBM, ref_vol, DIMS))
    assert bool((nbr[n:] == -7).all())                 # rows beyond the live count are not written


@pytest.mark.parametrize("geom,occ,clamp", [(DOWN, 0.1, False), (DOWN, 0.0, False), (DOWN, 0.3, True), (OUTC, 0.2, False),
                                            (OUTC, 0.2, True)],
                         ids=["stride2", "stride2 empty", "stride2 clamped", "out conv", "out conv clamped"])
def test_strided_outputs_and_their_rulebook(geom, occ, clamp):
    from thinktwice_amd import ops
    from thinktwice_amd._lib import check, lib, ptr
    coords, n = _level(occ, 11)
    max_in = coords.shape[0]
    od = _out_dims(DIMS, geom)
    cells = B * od[0] * od[1] * od[2]
    active = _ref_outputs(coords, n, geom, od, cells)[1]
    max_out = max(active // 2, 1) if clamp else active + 9
    assert not clamp or max_out < active
    ref_coords, ref_rows, ref_ovol = _ref_outputs(coords, n, geom, od, max_out)
    cd, rows, vol = _gpu_volume(coords, n, max_in, DIMS)
    ws_bytes = int(lib().tt_sp_strided_outputs_workspace_bytes(cells))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    ovol = torch.empty(cells, dtype=torch.int32, device="cuda")
    ocoords = torch.full((max_out, 4), -7, dtype=torch.int32, device="cuda")
    orows = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    check(lib().tt_sp_strided_outputs(ptr(cd), ptr(rows), max_in, B, _ci(*geom[0], *geom[1], *geom[2]), _ci(*od), ptr(ws), ws_bytes,
                                      ptr(ovol), ptr(ocoords), ptr(orows), max_out, ops.cur_stream(cd.device)),
          "tt_sp_strided_outputs")
    torch.cuda.synchronize()
    assert int(orows) == ref_rows
    assert torch.equal(ocoords.cpu()[:ref_rows], ref_coords)
    assert bool((ocoords.cpu()[ref_rows:] == -7).all())
    assert torch.equal(ovol.cpu().view(B, *od), ref_ovol)
    nbr = _gpu_rulebook(ocoords, orows, max_out, geom, DIMS, vol)
    assert torch.equal(nbr[:ref_rows], _ref_rulebook(ref_coords, ref_rows, geom, _ref_volume(coords, n, DIMS), DIMS))
    assert bool((nbr[ref_rows:] == -7).all())
