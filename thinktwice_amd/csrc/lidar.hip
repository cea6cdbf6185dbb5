// LiDAR branch kernels: hard voxelisation + mean VFE + sparse 3-D convolution.
//
// Replaces, for LidarNet.forward (backbones/lidarnet.py:87-96):
//   mmcv Voxelization (hard, deterministic)  -> tt_lidar_voxelize   (stable radix sort by voxel id,
//                                               run heads by scan, first <=max_points points per voxel
//                                               IN POINT ORDER, mean over them = HardSimpleVFE)
//   spconv SubMConv3d / SparseConv3d          -> tt_sp_volume_build / tt_sp_strided_outputs /
//                                               tt_sp_rulebook, then tt_conv2d_fwd in gather mode
//                                               (MFMA gathered GEMM, fused BN1d + ReLU + residual)
//   SparseConvTensor.dense() + view           -> tt_sp_to_dense (channel index c*D + z, channel-last)
// No host synchronisation: active-row counts stay in device memory; kernels are launched over an
// upper bound and exit early.
#include <hipcub/hipcub.hpp>

#include "tt_common.h"

namespace tt {

constexpr unsigned long long kInvalidKey = ~0ull;

struct Dims3 { int z, y, x; };

__global__ void lidar_keys_kernel(const float* __restrict__ pts, int B, int Np, int nfeat, float x0, float y0,
                                  float z0, float vx, float vy, float vz, int gx, int gy, int gz, int zlimit,
                                  unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * Np) return;
    const int b = (int)(i / Np);
    const float* p = pts + i * nfeat;
    // mmcv hard voxelize: c = floor((p - range_min) / voxel_size); drop if outside the grid
    const int cx = (int)floorf((p[0] - x0) / vx);
    const int cy = (int)floorf((p[1] - y0) / vy);
    const int cz = (int)floorf((p[2] - z0) / vz);
    const bool ok = cx >= 0 && cx < gx && cy >= 0 && cy < gy && cz >= 0 && cz < gz && cz < zlimit;
    keys[i] = ok ? ((((unsigned long long)b * gz + cz) * gy + cy) * gx + cx) : kInvalidKey;
    vals[i] = (unsigned)i;
}

__global__ void mark_heads_kernel(const unsigned long long* __restrict__ keys, long long n, int* __restrict__ flags,
                                  int* __restrict__ n_valid) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    const bool valid = k != kInvalidKey;
    flags[i] = (valid && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
    if (valid && (i == n - 1 || keys[i + 1] == kInvalidKey)) *n_valid = (int)(i + 1);
}

__global__ void voxel_heads_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ flags,
                                   const int* __restrict__ scan, long long n, int gx, int gy, int gz,
                                   int* __restrict__ coords, int* __restrict__ first, int* __restrict__ num_voxels) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flags[i]) {
        const int v = scan[i];
        unsigned long long k = keys[i];
        const int x = (int)(k % gx); k /= gx;
        const int y = (int)(k % gy); k /= gy;
        const int z = (int)(k % gz); k /= gz;
        coords[v * 4 + 0] = (int)k;
        coords[v * 4 + 1] = z;
        coords[v * 4 + 2] = y;
        coords[v * 4 + 3] = x;
        first[v] = (int)i;
    }
    if (i == n - 1) *num_voxels = scan[i] + flags[i];
}

__global__ void vfe_mean_kernel(const float* __restrict__ pts, const unsigned* __restrict__ vals,
                                const int* __restrict__ first, const int* __restrict__ num_voxels,
                                const int* __restrict__ n_valid, int nfeat, int max_points, long long max_rows,
                                float* __restrict__ feats) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long v = t / nfeat;
    const int f = (int)(t % nfeat);
    const int M = *num_voxels;
    if (v >= M || v >= max_rows) return;
    const int s = first[v];
    const int e = (v + 1 < M) ? first[v + 1] : *n_valid;
    const int cnt = min(e - s, max_points);
    float sum = 0.f;
    for (int j = 0; j < cnt; ++j) sum += pts[(long long)vals[s + j] * nfeat + f];
    feats[v * nfeat + f] = sum / (float)cnt;     // HardSimpleVFE: sum / num_points
}


// ----------------------------------------------------------------------------- max_voxels cap (first-appearance order)
// mmcv's hard voxelisation creates voxels in the order their first point appears and stops creating new ones at
// `max_voxels` per sample (points of later voxels are dropped; configs/thinktwice.py:161-165 (120000, 160000), call site
// backbones/lidarnet.py:88).  The sorted pipeline above emits voxels in CELL order; the capped variant ranks every voxel by
// the index of its first point (stable sort: the head of a run is its earliest point), keeps rank < max_voxels, and only
// then drops the voxels beyond the sparse grid's z extent (the cap counts them, like mmcv does).
__global__ void cap_head_points_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ flags,
                                       const int* __restrict__ scan_h, const unsigned* __restrict__ vals, long long n,
                                       int* __restrict__ head_pos, int* __restrict__ pt_flag, int* __restrict__ n_heads) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flags[i]) {
        head_pos[scan_h[i]] = (int)i;
        pt_flag[vals[i]] = 1;
    }
    if (i == n - 1) *n_heads = scan_h[i] + flags[i];
}

__global__ void cap_keep_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ flags,
                                const unsigned* __restrict__ vals, const int* __restrict__ scan_p, long long n, int Np, int gx,
                                int gy, int gz, int zlimit, int max_voxels, int* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int k = 0;
    if (flags[i]) {
        unsigned long long key = keys[i];
        key /= gx; key /= gy;
        const int z = (int)(key % gz);
        const long long p = vals[i];
        const long long b = p / Np;
        const int rank = scan_p[p] - scan_p[b * Np];          // voxels of this sample created before this one
        k = (rank < max_voxels && z < zlimit) ? 1 : 0;
    }
    keep[i] = k;
}

__global__ void cap_emit_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ keep,
                                const int* __restrict__ scan_k, const int* __restrict__ scan_h,
                                const int* __restrict__ head_pos, const int* __restrict__ n_heads,
                                const int* __restrict__ n_valid, long long n, int gx, int gy, int gz, int* __restrict__ coords,
                                int* __restrict__ first, int* __restrict__ last, int* __restrict__ num_voxels) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (keep[i]) {
        const int v = scan_k[i], h = scan_h[i];
        unsigned long long k = keys[i];
        const int x = (int)(k % gx); k /= gx;
        const int y = (int)(k % gy); k /= gy;
        const int z = (int)(k % gz); k /= gz;
        coords[v * 4 + 0] = (int)k;
        coords[v * 4 + 1] = z;
        coords[v * 4 + 2] = y;
        coords[v * 4 + 3] = x;
        first[v] = (int)i;
        last[v] = (h + 1 < *n_heads) ? head_pos[h + 1] : *n_valid;
    }
    if (i == n - 1) *num_voxels = scan_k[i] + keep[i];
}

__global__ void vfe_mean_capped_kernel(const float* __restrict__ pts, const unsigned* __restrict__ vals,
                                       const int* __restrict__ first, const int* __restrict__ last,
                                       const int* __restrict__ num_voxels, int nfeat, int max_points, long long max_rows,
                                       float* __restrict__ feats) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long v = t / nfeat;
    const int f = (int)(t % nfeat);
    if (v >= *num_voxels || v >= max_rows) return;
    const int s = first[v];
    const int cnt = min(last[v] - s, max_points);
    float sum = 0.f;
    for (int j = 0; j < cnt; ++j) sum += pts[(long long)vals[s + j] * nfeat + f];
    feats[v * nfeat + f] = sum / (float)cnt;
}

// ----------------------------------------------------------------------------- dense index volumes
// Each resolution level keeps vol[b][z][y][x] = feature row or -1.  The synthetic / real LiDAR grids of this
// model are small enough (<= 148 M cells at the input level for B = 8) that a dense volume beats a hash
// table: neighbour look-ups of spatially ordered rows coalesce, output-site generation is a bitmap of the output
// cells (atomicOr marks, popcount + compact), and row ids come out in cell order (deterministic).
struct ConvGeom { int kz, ky, kx, sz, sy, sx, pz, py, px; };

__device__ __forceinline__ long long lin_cell(int b, int z, int y, int x, Dims3 d) {
    return (((long long)b * d.z + z) * d.y + y) * d.x + x;
}

__global__ void volume_scatter_kernel(const int* __restrict__ coords, const int* __restrict__ num_rows,
                                      long long max_rows, Dims3 d, int* __restrict__ vol) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *num_rows || i >= max_rows) return;
    vol[lin_cell(coords[i * 4], coords[i * 4 + 1], coords[i * 4 + 2], coords[i * 4 + 3], d)] = (int)i;
}

// The index kernels below size their grids by the chip (kIndexBlocks workgroups of 256 threads fill every CU) and walk the
// live rows / the cells in a grid-stride or a block-contiguous loop: the row counts stay on the device.
constexpr int kIndexThreads = 256;
constexpr int kIndexBlocks = kNumCU * 8;
constexpr int kDirectCountTiles = 64;     // bitmaps of up to this many 8192-cell tiles are counted inside the compaction

// one row's (b, z, y, x); `vec`: the array is 16-byte aligned
__device__ __forceinline__ int4 load_coord(const int* __restrict__ coords, long long row, bool vec) {
    if (vec) return reinterpret_cast<const int4*>(coords)[row];
    return make_int4(coords[row * 4], coords[row * 4 + 1], coords[row * 4 + 2], coords[row * 4 + 3]);
}

__device__ __forceinline__ void store_int4(int* __restrict__ p, int4 v, bool vec) {
    if (vec) {
        *reinterpret_cast<int4*>(p) = v;
    } else {
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}

// sum over the workgroup's 256 threads, returned to every thread (red: 4 ints of LDS, reusable after the call)
__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// SparseConv3d active outputs: o is active iff some input i and tap k satisfy i = o*s - p + k.  Per dimension those o are
// the consecutive values ceil((i + p - K + 1) / s) .. floor((i + p) / s), clipped to the output grid: one thread per input
// row sets their bits in a bitmap of the output cells (bit c & 31 of word c >> 5).  The rows come in cell order, so the
// lanes of a wave mostly aim at the same few words: wave_or merges them and issues one atomicOr per run of lanes.

// bits[w] |= m of every lane (w = ~0u with m = 0: nothing).  Lanes next to each other with the same w are merged into the
// first lane of their run (OR is idempotent, so any lanes with equal w may be merged); that lane issues the atomic.
// All 64 lanes call it together.
__device__ __forceinline__ void wave_or(unsigned* __restrict__ bits, unsigned w, unsigned m) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned ow = __shfl_down(w, off), om = __shfl_down(m, off);     // past lane 63: the lane's own values
        m |= ow == w ? om : 0u;
    }
    const unsigned pw = __shfl_up(w, 1);
    if (((threadIdx.x & 63) == 0 || pw != w) && m) atomicOr(bits + w, m);
}

// nz, ny: ceil(kz / sz), ceil(ky / sy) = the most oz / oy one input reaches (wave-uniform trip counts around wave_or)
__global__ __launch_bounds__(kIndexThreads) void mark_output_bits_kernel(
    const int* __restrict__ in_coords, const int* __restrict__ in_rows, long long max_in, ConvGeom g, Dims3 od, int nz, int ny,
    unsigned* __restrict__ bits, bool vec) {
    const long long n = min((long long)*in_rows, max_in);
    for (long long base = (long long)blockIdx.x * kIndexThreads; base < n; base += (long long)gridDim.x * kIndexThreads) {
        const long long i = base + threadIdx.x;
        const bool live = i < n;
        const int4 c = live ? load_coord(in_coords, i, vec) : make_int4(0, 0, 0, 0);
        const int az = c.y + g.pz, ay = c.z + g.py, ax = c.w + g.px;
        const int z0 = az - g.kz + 1 > 0 ? (az - g.kz + g.sz) / g.sz : 0, z1 = min(az / g.sz, od.z - 1);
        const int y0 = ay - g.ky + 1 > 0 ? (ay - g.ky + g.sy) / g.sy : 0, y1 = min(ay / g.sy, od.y - 1);
        const int x0 = ax - g.kx + 1 > 0 ? (ax - g.kx + g.sx) / g.sx : 0, x1 = min(ax / g.sx, od.x - 1);
        for (int dz = 0; dz < nz; ++dz)
            for (int dy = 0; dy < ny; ++dy) {
                const int oz = z0 + dz, oy = y0 + dy;
                unsigned w0 = ~0u, m0 = 0, w1 = ~0u, m1 = 0;             // the x run's first word and its last, if another
                if (live && oz <= z1 && oy <= y1 && x0 <= x1) {
                    const unsigned line = ((unsigned)(c.x * od.z + oz) * od.y + oy) * od.x;    // cells < 2^31 (host check)
                    const unsigned first = line + x0, last = line + x1;
                    w0 = first >> 5;
                    const unsigned wl = last >> 5;
                    m0 = ~((1u << (first & 31)) - 1u);
                    const unsigned upto = (2u << (last & 31)) - 1u;      // bits 0 .. last & 31
                    if (wl == w0) {
                        m0 &= upto;
                    } else {
                        w1 = wl;
                        m1 = upto;
                        for (unsigned w = w0 + 1; w < wl; ++w) atomicOr(bits + w, ~0u);    // a run over three or more words
                    }
                }
                wave_or(bits, w0, m0);
                wave_or(bits, w1, m1);
            }
    }
}

// The bitmap is cut into tiles of 256 words (8192 cells); workgroup g owns the tiles [g * tiles_per_block, ...) of it.
// totals[g] = set bits of workgroup g's tiles.
__global__ __launch_bounds__(kIndexThreads) void count_output_bits_kernel(const unsigned* __restrict__ bits, int tiles_per_block,
                                                                          int ntiles, int* __restrict__ totals) {
    __shared__ int red[4];
    const int t0 = min((int)blockIdx.x * tiles_per_block, ntiles), t1 = min(t0 + tiles_per_block, ntiles);
    int cnt = 0;
    for (int t = t0; t < t1; ++t) cnt += __popc(bits[(long long)t * kIndexThreads + threadIdx.x]);
    cnt = block_sum(cnt, red);
    if (threadIdx.x == 0) totals[blockIdx.x] = cnt;
}

// Row id of an active cell = number of active cells before it in cell order (b, z, y, x) = totals of the workgroups before
// this one + set bits before it in this workgroup's tiles.  One pass writes vol for EVERY cell (row, or -1 for an empty
// cell and for rows at or beyond max_out), out_coords of the rows below max_out and the clamped live count.
__global__ __launch_bounds__(kIndexThreads) void compact_output_bits_kernel(
    const unsigned* __restrict__ bits, const int* __restrict__ totals, int tiles_per_block, int ntiles, unsigned cells, Dims3 od,
    int max_out, int* __restrict__ vol, int* __restrict__ out_coords, int* __restrict__ out_rows, bool vec_vol, bool vec_coords) {
    __shared__ int red[4];
    __shared__ unsigned s_word[kIndexThreads];
    __shared__ int s_rank[kIndexThreads];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = min((int)blockIdx.x * tiles_per_block, ntiles), t1 = min(t0 + tiles_per_block, ntiles);
    int before = 0, all = 0;
    if (totals) {
        for (int i = tid; i < (int)gridDim.x; i += kIndexThreads) {
            const int v = totals[i];
            all += v;
            before += i < (int)blockIdx.x ? v : 0;
        }
    } else {      // a small bitmap (kDirectCountTiles): every workgroup counts the words before its own, no count launch
        const uint4* bits4 = reinterpret_cast<const uint4*>(bits);            // the workspace is 16-byte aligned (host check)
        const int n4 = (blockIdx.x == 0 ? ntiles : t0) * (kIndexThreads / 4), before4 = t0 * (kIndexThreads / 4);
#pragma unroll 4
        for (int i = tid; i < n4; i += kIndexThreads) {
            const uint4 w = bits4[i];
            const int v = __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
            all += v;
            before += i < before4 ? v : 0;
        }
    }
    before = block_sum(before, red);
    if (blockIdx.x == 0) {
        all = block_sum(all, red);
        if (tid == 0) *out_rows = min(all, max_out);
    }
    for (int t = t0; t < t1; ++t) {
        const unsigned word = bits[(long long)t * kIndexThreads + tid];
        int incl = __popc(word);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        __syncthreads();                     // the previous tile's readers of s_word / s_rank / red are done
        if (lane == 63) red[wave] = incl;
        __syncthreads();
        int wave_base = 0;
        for (int w = 0; w < wave; ++w) wave_base += red[w];
        s_word[tid] = word;
        s_rank[tid] = before + wave_base + incl - __popc(word);
        before += red[0] + red[1] + red[2] + red[3];
        __syncthreads();
        // four cells per thread and step: a wave stores 1 KB of vol in one piece
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = k * kIndexThreads + tid;                 // group of four cells within the tile
            const unsigned cell = (unsigned)t * (kIndexThreads * 32) + (unsigned)q * 4;
            if (cell >= cells) continue;
            const unsigned ww = s_word[q >> 3];
            const int sh = (q & 7) * 4;
            int row = s_rank[q >> 3] + __popc(ww & ((1u << sh) - 1u));
            const unsigned four = (ww >> sh) & 15u;
            int v[4] = {-1, -1, -1, -1};
            if (four && row < max_out) {
                const unsigned ry = cell / (unsigned)od.x, rz = ry / (unsigned)od.y, rb = rz / (unsigned)od.z;
                int4 c = make_int4((int)rb, (int)(rz - rb * od.z), (int)(ry - rz * od.y), (int)(cell - ry * od.x));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (((four >> j) & 1u) && row < max_out) {
                        v[j] = row;
                        store_int4(out_coords + (long long)row * 4, c, vec_coords);
                        ++row;
                    }
                    if (++c.w == od.x) {                                   // the next cell in (b, z, y, x) order
                        c.w = 0;
                        if (++c.z == od.y) {
                            c.z = 0;
                            if (++c.y == od.z) { c.y = 0; ++c.x; }
                        }
                    }
                }
            }
            if (vec_vol && cell + 3 < cells) {
                *reinterpret_cast<int4*>(vol + cell) = make_int4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (cell + j < cells) vol[cell + j] = v[j];
            }
        }
    }
}

// rulebook: nbr[o][k] = input row at (o*s - p + k) or -1, tap k = (kz * KY + ky) * KX + kx.
// A workgroup takes 256 output rows at a time: their coordinates go through LDS (one 16-byte load per row), and the work
// item is one (row, kz, ky) with its KX taps -- adjacent words of the volume in, adjacent words of nbr out, and item it of
// the block lands at nbr + (base * KV + it * KX), so a wave's stores cover one contiguous piece of nbr.  Every look-up is
// issued unconditionally (an absent or out-of-grid tap reads vol[0] and keeps -1) before the first store, so the loads of
// a thread's items are in flight together.  KX = 3 (host: the input has at least 3 cells in x) fetches an item's three
// words with ONE 12-byte load, from the x window shifted into the row at the grid's edge, three items to a pass.
// KZ = KY = KX = 0 is the generic form with run-time extents.  Measurements: profiles/sp_index.txt.
struct __attribute__((aligned(4))) VolWords3 { int w[3]; };

template <int KZ, int KY, int KX>
__global__ __launch_bounds__(kIndexThreads) void rulebook_rows_kernel(
    const int* __restrict__ out_coords, const int* __restrict__ out_rows, long long max_out, ConvGeom g, Dims3 id,
    const int* __restrict__ vol, int* __restrict__ nbr, bool vec) {
    __shared__ int4 s_coord[kIndexThreads];
    constexpr bool kFixed = KZ > 0;
    const int ky_n = kFixed ? KY : g.ky, kx_n = kFixed ? KX : g.kx;
    const int per_row = (kFixed ? KZ : g.kz) * ky_n;           // items per row
    const int KV = per_row * kx_n;
    const int tid = threadIdx.x;
    const long long n = min((long long)*out_rows, max_out);
    for (long long base = (long long)blockIdx.x * kIndexThreads; base < n; base += (long long)gridDim.x * kIndexThreads) {
        const int rows = (int)min((long long)kIndexThreads, n - base);
        __syncthreads();
        if (tid < rows) s_coord[tid] = load_coord(out_coords, base + tid, vec);
        __syncthreads();
        const int items = rows * per_row;
        int* __restrict__ dst = nbr + base * KV;
        auto look_up = [&](int it, int kx) -> int {          // tap kx of item it, it < items
            const int r = it / per_row, j = it - r * per_row;
            const int kz = j / ky_n, ky = j - kz * ky_n;
            const int4 c = s_coord[r];
            const int z = c.y * g.sz - g.pz + kz, y = c.z * g.sy - g.py + ky, x = c.w * g.sx - g.px + kx;
            const bool ok = (unsigned)z < (unsigned)id.z && (unsigned)y < (unsigned)id.y && (unsigned)x < (unsigned)id.x;
            const int r_in = vol[ok ? lin_cell(c.x, z, y, x, id) : 0];
            return ok ? r_in : -1;
        };
        if constexpr (kFixed && KX == 3) {
            // kPass items of a thread at a time: their loads in flight together, and few enough registers for 8 waves a SIMD
            constexpr int kPass = 3;
            static_assert(KZ * KY % kPass == 0, "whole passes");
#pragma unroll 1
            for (int u0 = 0; u0 < KZ * KY; u0 += kPass) {
                VolWords3 win[kPass];
                unsigned taps[kPass];      // bits 0 .. 2: tap kx lies in the grid; bits 4 .. 7: 8 + (x of tap 0 - window start)
#pragma unroll
                for (int u = 0; u < kPass; ++u) {
                    const int it = min((u0 + u) * kIndexThreads + tid, items - 1);
                    const int r = it / per_row, j = it - r * per_row;
                    const int kz = j / KY, ky = j - kz * KY;
                    const int4 c = s_coord[r];
                    const int z = c.y * g.sz - g.pz + kz, y = c.z * g.sy - g.py + ky, x0 = c.w * g.sx - g.px;
                    const bool zy_ok = (unsigned)z < (unsigned)id.z && (unsigned)y < (unsigned)id.y;
                    const int xs = min(max(x0, 0), id.x - 3);                         // window [xs, xs + 3) lies in the row
                    win[u] = *reinterpret_cast<const VolWords3*>(vol + (zy_ok ? lin_cell(c.x, z, y, xs, id) : 0));
                    unsigned t = (unsigned)(min(max(x0 - xs, -8), 7) + 8) << 4;       // beyond +-2 no tap lies in the row
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) t |= (zy_ok && (unsigned)(x0 + kx) < (unsigned)id.x ? 1u : 0u) << kx;
                    taps[u] = t;
                }
#pragma unroll
                for (int u = 0; u < kPass; ++u) {
                    const int it = (u0 + u) * kIndexThreads + tid;
                    if (it < items) {
                        const int shift = (int)(taps[u] >> 4) - 8;
                        VolWords3 out;
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            const int d = kx + shift;                                 // a tap inside the row has d in 0 .. 2
                            const int r_in = d == 0 ? win[u].w[0] : d == 1 ? win[u].w[1] : win[u].w[2];
                            out.w[kx] = (taps[u] >> kx) & 1u ? r_in : -1;
                        }
                        *reinterpret_cast<VolWords3*>(dst + (long long)it * 3) = out;
                    }
                }
            }
        } else if constexpr (kFixed) {
            int v[KZ * KY][KX];
#pragma unroll
            for (int u = 0; u < KZ * KY; ++u) {
                const int it = min(u * kIndexThreads + tid, items - 1);
#pragma unroll
                for (int kx = 0; kx < KX; ++kx) v[u][kx] = look_up(it, kx);
            }
#pragma unroll
            for (int u = 0; u < KZ * KY; ++u) {
                const int it = u * kIndexThreads + tid;
                if (it < items) {
#pragma unroll
                    for (int kx = 0; kx < KX; ++kx) dst[(long long)it * KX + kx] = v[u][kx];
                }
            }
        } else {
            for (int it = tid; it < items; it += kIndexThreads)
                for (int kx = 0; kx < kx_n; ++kx) dst[(long long)it * kx_n + kx] = look_up(it, kx);
        }
    }
}

// Tap-occupancy mask of every output row of a rulebook (bit t = tap t has an input row), 0xFFFFFFFF for rows beyond
// the live count so that they sort last; vals = row index.  `pairs` (nullable) accumulates the number of existing
// (output row, tap) pairs = the real multiply count of the sparse convolution.
__global__ void sp_row_masks_kernel(const int* __restrict__ nbr, const int* __restrict__ rows_n, long long max_rows, int KV,
                                    unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                                    unsigned long long* __restrict__ pairs) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned cnt = 0;
    if (o < max_rows) {
        unsigned m = 0xFFFFFFFFu;
        if (o < *rows_n) {
            m = 0;
            for (int t = 0; t < KV; ++t) m |= (nbr[o * KV + t] >= 0 ? 1u : 0u) << t;
            cnt = __popc(m);
        }
        keys[o] = m;
        vals[o] = (unsigned)o;
    }
    if (pairs) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(pairs, (unsigned long long)cnt);
    }
}

template <typename T>
__global__ void sp_to_dense_kernel(const T* __restrict__ f, const int* __restrict__ coords,
                                   const int* __restrict__ rows_n, long long max_rows, int C, Dims3 d,
                                   T* __restrict__ dense) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = t / C;
    const int c = (int)(t % C);
    if (r >= *rows_n || r >= max_rows) return;
    const int b = coords[r * 4], z = coords[r * 4 + 1], y = coords[r * 4 + 2], x = coords[r * 4 + 3];
    dense[(((long long)b * d.y + y) * d.x + x) * ((long long)C * d.z) + (long long)c * d.z + z] = f[r * C + c];
}

}  // namespace tt

using namespace tt;

static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

extern "C" long long tt_lidar_voxelize_workspace_bytes(long long num_points_total) {
    size_t sort_bytes = 0, scan_bytes = 0;
    const int n = (int)num_points_total;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (unsigned long long*)nullptr,
                                       (unsigned long long*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, n);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (int*)nullptr, (int*)nullptr, n);
    size_t tot = 0;
    tot += 2 * align256(sizeof(unsigned long long) * n);   // keys in/out
    tot += 2 * align256(sizeof(unsigned) * n);             // vals in/out
    tot += 2 * align256(sizeof(int) * n);                  // flags, scan
    tot += align256(sizeof(int) * (n + 1));                // first
    tot += align256(sizeof(int) * 4);                      // n_valid
    tot += align256(sort_bytes > scan_bytes ? sort_bytes : scan_bytes);
    return (long long)tot;
}

extern "C" int tt_lidar_voxelize(const float* points, int B, int Np, int nfeat, const float* pc_range_lo,
                                 const float* voxel_size, const int* grid_xyz, int z_limit, int max_points,
                                 void* workspace, long long workspace_bytes, float* voxel_feats, int* coords,
                                 int* num_voxels, void* stream) {
    TT_REQUIRE(points && pc_range_lo && voxel_size && grid_xyz && workspace && voxel_feats && coords && num_voxels,
               "tt_lidar_voxelize: null");
    const long long n = (long long)B * Np;
    TT_REQUIRE(n > 0 && n < (1ll << 30), "tt_lidar_voxelize: bad point count");
    TT_REQUIRE(workspace_bytes >= tt_lidar_voxelize_workspace_bytes(n), "tt_lidar_voxelize: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    auto take = [&](size_t bytes) { char* p = w; w += align256(bytes); return p; };
    auto* keys_in = (unsigned long long*)take(sizeof(unsigned long long) * n);
    auto* keys_out = (unsigned long long*)take(sizeof(unsigned long long) * n);
    auto* vals_in = (unsigned*)take(sizeof(unsigned) * n);
    auto* vals_out = (unsigned*)take(sizeof(unsigned) * n);
    auto* flags = (int*)take(sizeof(int) * n);
    auto* scan = (int*)take(sizeof(int) * n);
    auto* first = (int*)take(sizeof(int) * (n + 1));
    auto* n_valid = (int*)take(sizeof(int) * 4);
    void* tmp = w;
    size_t tmp_bytes = (size_t)(workspace_bytes - (w - (char*)workspace));
    (void)hipMemsetAsync(n_valid, 0, sizeof(int), st);
    (void)hipMemsetAsync(num_voxels, 0, sizeof(int), st);
    const unsigned blocks = (unsigned)div_up(n, 256);
    hipLaunchKernelGGL(lidar_keys_kernel, dim3(blocks), dim3(256), 0, st, points, B, Np, nfeat, pc_range_lo[0],
                       pc_range_lo[1], pc_range_lo[2], voxel_size[0], voxel_size[1], voxel_size[2], grid_xyz[0],
                       grid_xyz[1], grid_xyz[2], z_limit, keys_in, vals_in);
    size_t sb = tmp_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(tmp, sb, keys_in, keys_out, vals_in, vals_out, (int)n, 0, 64, st) !=
        hipSuccess) {
        set_error("tt_lidar_voxelize: radix sort failed");
        return -2;
    }
    hipLaunchKernelGGL(mark_heads_kernel, dim3(blocks), dim3(256), 0, st, keys_out, n, flags, n_valid);
    sb = tmp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(tmp, sb, flags, scan, (int)n, st) != hipSuccess) {
        set_error("tt_lidar_voxelize: scan failed");
        return -2;
    }
    hipLaunchKernelGGL(voxel_heads_kernel, dim3(blocks), dim3(256), 0, st, keys_out, flags, scan, n, grid_xyz[0],
                       grid_xyz[1], grid_xyz[2], coords, first, num_voxels);
    hipLaunchKernelGGL(vfe_mean_kernel, dim3((unsigned)div_up(n * nfeat, 256)), dim3(256), 0, st, points, vals_out,
                       first, num_voxels, n_valid, nfeat, max_points, n, voxel_feats);
    return check_launch("tt_lidar_voxelize");
}


extern "C" long long tt_lidar_voxelize_capped_workspace_bytes(long long num_points_total) {
    const long long n = num_points_total;
    return tt_lidar_voxelize_workspace_bytes(n) + (long long)(8 * align256(sizeof(int) * (n + 1)));
}

extern "C" int tt_lidar_voxelize_capped(const float* points, int B, int Np, int nfeat, const float* pc_range_lo,
                                        const float* voxel_size, const int* grid_xyz, int z_limit, int max_points,
                                        int max_voxels, void* workspace, long long workspace_bytes, float* voxel_feats,
                                        int* coords, int* num_voxels, void* stream) {
    TT_REQUIRE(points && pc_range_lo && voxel_size && grid_xyz && workspace && voxel_feats && coords && num_voxels,
               "tt_lidar_voxelize_capped: null");
    const long long n = (long long)B * Np;
    TT_REQUIRE(n > 0 && n < (1ll << 30) && max_voxels > 0, "tt_lidar_voxelize_capped: bad sizes");
    TT_REQUIRE(workspace_bytes >= tt_lidar_voxelize_capped_workspace_bytes(n), "tt_lidar_voxelize_capped: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    auto take = [&](size_t bytes) { char* p = w; w += align256(bytes); return p; };
    auto* keys_in = (unsigned long long*)take(sizeof(unsigned long long) * n);
    auto* keys_out = (unsigned long long*)take(sizeof(unsigned long long) * n);
    auto* vals_in = (unsigned*)take(sizeof(unsigned) * n);
    auto* vals_out = (unsigned*)take(sizeof(unsigned) * n);
    auto* flags = (int*)take(sizeof(int) * n);
    auto* scan_h = (int*)take(sizeof(int) * n);
    auto* first = (int*)take(sizeof(int) * (n + 1));
    auto* n_valid = (int*)take(sizeof(int) * 4);
    auto* head_pos = (int*)take(sizeof(int) * (n + 1));
    auto* pt_flag = (int*)take(sizeof(int) * (n + 1));
    auto* scan_p = (int*)take(sizeof(int) * (n + 1));
    auto* keep = (int*)take(sizeof(int) * (n + 1));
    auto* scan_k = (int*)take(sizeof(int) * (n + 1));
    auto* last = (int*)take(sizeof(int) * (n + 1));
    auto* n_heads = (int*)take(sizeof(int) * (n + 1));
    void* tmp = w;
    size_t tmp_bytes = (size_t)(workspace_bytes - (w - (char*)workspace));
    (void)hipMemsetAsync(n_valid, 0, sizeof(int), st);
    (void)hipMemsetAsync(num_voxels, 0, sizeof(int), st);
    (void)hipMemsetAsync(n_heads, 0, sizeof(int), st);
    (void)hipMemsetAsync(pt_flag, 0, sizeof(int) * n, st);
    const unsigned blocks = (unsigned)div_up(n, 256);
    // keys over the WHOLE voxel grid (z_limit = grid z): the cap counts the voxels beyond the sparse grid too
    hipLaunchKernelGGL(lidar_keys_kernel, dim3(blocks), dim3(256), 0, st, points, B, Np, nfeat, pc_range_lo[0],
                       pc_range_lo[1], pc_range_lo[2], voxel_size[0], voxel_size[1], voxel_size[2], grid_xyz[0],
                       grid_xyz[1], grid_xyz[2], grid_xyz[2], keys_in, vals_in);
    size_t sb = tmp_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(tmp, sb, keys_in, keys_out, vals_in, vals_out, (int)n, 0, 64, st) != hipSuccess) {
        set_error("tt_lidar_voxelize_capped: radix sort failed");
        return -2;
    }
    hipLaunchKernelGGL(mark_heads_kernel, dim3(blocks), dim3(256), 0, st, keys_out, n, flags, n_valid);
    auto scan = [&](const int* in, int* out) {
        size_t b = tmp_bytes;
        return hipcub::DeviceScan::ExclusiveSum(tmp, b, in, out, (int)n, st) == hipSuccess;
    };
    if (!scan(flags, scan_h)) { set_error("tt_lidar_voxelize_capped: scan failed"); return -2; }
    hipLaunchKernelGGL(cap_head_points_kernel, dim3(blocks), dim3(256), 0, st, keys_out, flags, scan_h, vals_out, n, head_pos,
                       pt_flag, n_heads);
    if (!scan(pt_flag, scan_p)) { set_error("tt_lidar_voxelize_capped: scan failed"); return -2; }
    hipLaunchKernelGGL(cap_keep_kernel, dim3(blocks), dim3(256), 0, st, keys_out, flags, vals_out, scan_p, n, Np, grid_xyz[0],
                       grid_xyz[1], grid_xyz[2], z_limit, max_voxels, keep);
    if (!scan(keep, scan_k)) { set_error("tt_lidar_voxelize_capped: scan failed"); return -2; }
    hipLaunchKernelGGL(cap_emit_kernel, dim3(blocks), dim3(256), 0, st, keys_out, keep, scan_k, scan_h, head_pos, n_heads,
                       n_valid, n, grid_xyz[0], grid_xyz[1], grid_xyz[2], coords, first, last, num_voxels);
    hipLaunchKernelGGL(vfe_mean_capped_kernel, dim3((unsigned)div_up(n * nfeat, 256)), dim3(256), 0, st, points, vals_out,
                       first, last, num_voxels, nfeat, max_points, n, voxel_feats);
    return check_launch("tt_lidar_voxelize_capped");
}

static ConvGeom geom_of(const int* g) { return ConvGeom{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8]}; }

extern "C" int tt_sp_volume_build(const int* coords, const int* num_rows, long long max_rows, int batch,
                                  const int* dims_zyx, int* vol, void* stream) {
    TT_REQUIRE(coords && num_rows && dims_zyx && vol, "tt_sp_volume_build: null");
    hipStream_t st = (hipStream_t)stream;
    Dims3 d{dims_zyx[0], dims_zyx[1], dims_zyx[2]};
    const long long cells = (long long)batch * d.z * d.y * d.x;
    (void)hipMemsetAsync(vol, 0xFF, sizeof(int) * cells, st);
    hipLaunchKernelGGL(volume_scatter_kernel, dim3((unsigned)div_up(max_rows, 256)), dim3(256), 0, st, coords,
                       num_rows, max_rows, d, vol);
    return check_launch("tt_sp_volume_build");
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// workgroups of a grid-stride index kernel over at most `rows` rows: one per 256 rows, no more than fill the chip
static unsigned index_blocks(long long rows) {
    const long long b = (rows + kIndexThreads - 1) / kIndexThreads;
    return (unsigned)(b < 1 ? 1 : b < kIndexBlocks ? b : kIndexBlocks);
}

// workspace of tt_sp_strided_outputs: the bitmap of the output cells in whole tiles of 256 words, then one total per workgroup
static long long sp_bitmap_tiles(long long out_cells) { return (out_cells + kIndexThreads * 32 - 1) / (kIndexThreads * 32); }

extern "C" long long tt_sp_strided_outputs_workspace_bytes(long long out_cells) {
    return (long long)(align256(sizeof(unsigned) * kIndexThreads * sp_bitmap_tiles(out_cells)) +
                       align256(sizeof(int) * kIndexBlocks));
}

extern "C" int tt_sp_strided_outputs(const int* in_coords, const int* in_rows, long long max_in, int batch,
                                     const int* kernel_stride_pad, const int* out_dims_zyx, void* workspace,
                                     long long workspace_bytes, int* out_vol, int* out_coords, int* out_rows,
                                     long long max_out, void* stream) {
    TT_REQUIRE(in_coords && in_rows && kernel_stride_pad && out_dims_zyx && workspace && out_vol && out_coords &&
                   out_rows, "tt_sp_strided_outputs: null");
    hipStream_t st = (hipStream_t)stream;
    ConvGeom g = geom_of(kernel_stride_pad);
    Dims3 od{out_dims_zyx[0], out_dims_zyx[1], out_dims_zyx[2]};
    const long long cells = (long long)batch * od.z * od.y * od.x;
    TT_REQUIRE(cells > 0 && cells < (1ll << 31), "tt_sp_strided_outputs: bad grid (%lld cells)", cells);
    TT_REQUIRE(g.kz > 0 && g.ky > 0 && g.kx > 0 && g.sz > 0 && g.sy > 0 && g.sx > 0 && g.pz >= 0 && g.py >= 0 && g.px >= 0,
               "tt_sp_strided_outputs: bad geometry");
    TT_REQUIRE(workspace_bytes >= tt_sp_strided_outputs_workspace_bytes(cells) && aligned16(workspace),
               "tt_sp_strided_outputs: workspace");
    const int ntiles = (int)sp_bitmap_tiles(cells);
    const size_t bitmap_bytes = sizeof(unsigned) * kIndexThreads * (size_t)ntiles;
    unsigned* bits = (unsigned*)workspace;
    int* totals = (int*)((char*)workspace + align256(bitmap_bytes));
    const int blocks = ntiles < kIndexBlocks ? ntiles : kIndexBlocks;
    const int tiles_per_block = div_up(ntiles, blocks);
    (void)hipMemsetAsync(bits, 0, bitmap_bytes, st);
    hipLaunchKernelGGL(mark_output_bits_kernel, dim3(index_blocks(max_in)), dim3(kIndexThreads), 0, st, in_coords, in_rows,
                       max_in, g, od, (g.kz + g.sz - 1) / g.sz, (g.ky + g.sy - 1) / g.sy, bits, aligned16(in_coords));
    if (ntiles > kDirectCountTiles)
        hipLaunchKernelGGL(count_output_bits_kernel, dim3(blocks), dim3(kIndexThreads), 0, st, bits, tiles_per_block, ntiles,
                           totals);
    else
        totals = nullptr;
    const int clamp = (int)(max_out < 0 ? 0 : max_out < 0x7fffffffll ? max_out : 0x7fffffffll);
    hipLaunchKernelGGL(compact_output_bits_kernel, dim3(blocks), dim3(kIndexThreads), 0, st, bits, totals, tiles_per_block,
                       ntiles, (unsigned)cells, od, clamp, out_vol, out_coords, out_rows, aligned16(out_vol),
                       aligned16(out_coords));
    return check_launch("tt_sp_strided_outputs");
}

extern "C" int tt_sp_rulebook(const int* out_coords, const int* out_rows, long long max_out,
                              const int* kernel_stride_pad, const int* in_dims_zyx, const int* in_vol, int* nbr,
                              void* stream) {
    TT_REQUIRE(out_coords && out_rows && kernel_stride_pad && in_dims_zyx && in_vol && nbr, "tt_sp_rulebook: null");
    ConvGeom g = geom_of(kernel_stride_pad);
    Dims3 id{in_dims_zyx[0], in_dims_zyx[1], in_dims_zyx[2]};
    TT_REQUIRE(g.kz > 0 && g.ky > 0 && g.kx > 0 && (long long)g.kz * g.ky * g.kx < (1 << 20),
               "tt_sp_rulebook: bad kernel extents");
    const dim3 grid(index_blocks(max_out)), block(kIndexThreads);
    const bool vec = aligned16(out_coords);
    hipStream_t st = (hipStream_t)stream;
    // the model's two geometries with compile-time tap loops; anything else with run-time extents
    if (g.kz == 3 && g.ky == 3 && g.kx == 3 && id.x >= 3)
        hipLaunchKernelGGL((rulebook_rows_kernel<3, 3, 3>), grid, block, 0, st, out_coords, out_rows, max_out, g, id, in_vol, nbr,
                           vec);
    else if (g.kz == 3 && g.ky == 1 && g.kx == 1)
        hipLaunchKernelGGL((rulebook_rows_kernel<3, 1, 1>), grid, block, 0, st, out_coords, out_rows, max_out, g, id, in_vol, nbr,
                           vec);
    else
        hipLaunchKernelGGL((rulebook_rows_kernel<0, 0, 0>), grid, block, 0, st, out_coords, out_rows, max_out, g, id, in_vol, nbr,
                           vec);
    return check_launch("tt_sp_rulebook");
}

extern "C" int tt_sp_to_dense(const void* feats, const int* coords, const int* num_rows, long long max_rows, int C,
                              const int* dims_zyx, void* dense, int dtype, void* stream) {
    TT_REQUIRE(feats && coords && num_rows && dims_zyx && dense, "tt_sp_to_dense: null");
    Dims3 d{dims_zyx[0], dims_zyx[1], dims_zyx[2]};
    const dim3 grid((unsigned)div_up(max_rows * C, 256));
    if (dtype == TT_F32)
        hipLaunchKernelGGL(sp_to_dense_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)feats,
                           coords, num_rows, max_rows, C, d, (float*)dense);
    else   // bf16 and IEEE half alike: a 2-byte row copy
        hipLaunchKernelGGL(sp_to_dense_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream,
                           (const uint16_t*)feats, coords, num_rows, max_rows, C, d, (uint16_t*)dense);
    return check_launch("tt_sp_to_dense");
}

extern "C" long long tt_sp_tile_plan_workspace_bytes(long long max_rows) {
    size_t sort_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr,
                                       (unsigned*)nullptr, (int)max_rows);
    return (long long)(2 * align256(sizeof(unsigned) * max_rows) + align256(sort_bytes));
}

extern "C" int tt_sp_tile_plan(const int* nbr, const int* num_rows, long long max_rows, int KV, void* workspace,
                               long long workspace_bytes, int* row_perm, unsigned* row_mask_sorted,
                               unsigned long long* pairs_or_null, void* stream) {
    TT_REQUIRE(nbr && num_rows && workspace && row_perm && row_mask_sorted, "tt_sp_tile_plan: null");
    TT_REQUIRE(KV >= 1 && KV <= 31 && max_rows > 0 && max_rows < (1ll << 31), "tt_sp_tile_plan: KV=%d max_rows=%lld", KV,
               max_rows);
    TT_REQUIRE(workspace_bytes >= tt_sp_tile_plan_workspace_bytes(max_rows), "tt_sp_tile_plan: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    unsigned* keys = (unsigned*)w;
    unsigned* vals = (unsigned*)(w + align256(sizeof(unsigned) * max_rows));
    void* tmp = w + 2 * align256(sizeof(unsigned) * max_rows);
    size_t tmp_bytes = (size_t)(workspace_bytes - 2 * (long long)align256(sizeof(unsigned) * max_rows));
    hipLaunchKernelGGL(sp_row_masks_kernel, dim3((unsigned)div_up(max_rows, 256)), dim3(256), 0, st, nbr, num_rows, max_rows,
                       KV, keys, vals, pairs_or_null);
    if (hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys, row_mask_sorted, vals, (unsigned*)row_perm, (int)max_rows, 0,
                                           32, st) != hipSuccess) {
        set_error("tt_sp_tile_plan: radix sort failed");
        return -2;
    }
    return check_launch("tt_sp_tile_plan");
}
