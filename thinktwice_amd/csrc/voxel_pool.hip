// The op-boundary voxel pool ("splat") for gfx950 (wave64): kernels and entries.
//
//  tt_voxel_pool_fwd / _fwd_ws   op-boundary drop-in for the reference CUDA kernel
//                                (ops/voxel_pooling/src/voxel_pooling_forward_cuda.cu:9-36): the single-pass atomic kernels
//                                (rows, scalar), the two-phase reduce and the per-launch counting sort.
//  tt_voxel_pool_plan_build / _fwd_planned   the same sums over a plan sorted once, for static geometry.
//  tt_voxel_pool_bwd             VoxelPooling.backward (ops/voxel_pooling/voxel_pooling.py:57-69).
//
// Which of them a call runs on, with which grids and workspace offsets, is decided in voxel_pool_choose.cpp; every entry
// here validates, asks the chooser and launches what it answers.  The fused lift-splat of the forward is lift_splat.hip.
//
// Design (HBM-bound): the reference walks one point per THREAD
// (64 lanes 1 KiB apart => every load and atomic uncoalesced).  Here one WAVE
// owns a point row: 64 lanes x float4 = one fully coalesced 1 KiB row load,
// rows of out-of-range points are never fetched, consecutive points that fall
// in the same BEV cell are summed in registers and flushed with one atomic per
// channel (wave-level pre-reduction), and 4 row loads are kept in flight per wave.
#include <stdlib.h>

#include <hipcub/hipcub.hpp>

#include "tt_common.h"
#include "voxel_pool_choose.h"

namespace tt {

// ---------------------------------------------------------------------------
// forward, C % 4 == 0.  NV = float4 chunks per lane = ceil(C / 256).
// ---------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(256) void voxel_pool_rows_kernel(
    long long total_points, int num_points, int C, int X, int Y, int Z,
    const int32_t* __restrict__ geom, const float* __restrict__ feats,
    float* __restrict__ out, int32_t* __restrict__ pos_memo) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long nchunks = (total_points + 63) >> 6;
    const int c4 = C >> 2;

    for (long long chunk = wave; chunk < nchunks; chunk += nwaves) {
        const long long p = chunk * 64 + lane;
        int cell = -1;
        if (p < total_points) {
            const int x = geom[p * 3 + 0];
            const int y = geom[p * 3 + 1];
            const int z = geom[p * 3 + 2];
            if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) {
                const int b = (int)(p / num_points);
                cell = (b * Y + y) * X + x;
                if (pos_memo) {
                    pos_memo[p * 3 + 0] = b;
                    pos_memo[p * 3 + 1] = y;
                    pos_memo[p * 3 + 2] = x;
                }
            }
        }
        unsigned long long mask = __ballot(cell >= 0);
        int cur = -1;
        float4 acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);

        while (mask) {
            // up to 4 valid points per round: issue all row loads first.
            int idx[4];
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (mask) {
                    idx[j] = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    cnt = j + 1;
                } else {
                    idx[j] = 0;
                }
            }
            float4 row[4][NV];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < cnt) {
                    const float4* src =
                        reinterpret_cast<const float4*>(feats + (chunk * 64 + idx[j]) * (long long)C);
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const int ch = lane + 64 * v;
                        row[j][v] = (ch < c4) ? src[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < cnt) {
                    const int c = __builtin_amdgcn_readlane(cell, idx[j]);
                    if (c != cur) {
                        if (cur >= 0) {
#pragma unroll
                            for (int v = 0; v < NV; ++v) {
                                const int ch = lane + 64 * v;
                                if (ch < c4) {
                                    float* dst = out + (long long)cur * C + ch * 4;
                                    unsafeAtomicAdd(dst + 0, acc[v].x);
                                    unsafeAtomicAdd(dst + 1, acc[v].y);
                                    unsafeAtomicAdd(dst + 2, acc[v].z);
                                    unsafeAtomicAdd(dst + 3, acc[v].w);
                                }
                            }
                        }
                        cur = c;
#pragma unroll
                        for (int v = 0; v < NV; ++v) acc[v] = row[j][v];
                    } else {
#pragma unroll
                        for (int v = 0; v < NV; ++v) {
                            acc[v].x += row[j][v].x;
                            acc[v].y += row[j][v].y;
                            acc[v].z += row[j][v].z;
                            acc[v].w += row[j][v].w;
                        }
                    }
                }
            }
        }
        if (cur >= 0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int ch = lane + 64 * v;
                if (ch < c4) {
                    float* dst = out + (long long)cur * C + ch * 4;
                    unsafeAtomicAdd(dst + 0, acc[v].x);
                    unsafeAtomicAdd(dst + 1, acc[v].y);
                    unsafeAtomicAdd(dst + 2, acc[v].z);
                    unsafeAtomicAdd(dst + 3, acc[v].w);
                }
            }
        }
    }
}


// ---------------------------------------------------------------------------
// forward v2: atomics-free two-phase reduce (needs a workspace).
//   phase 1: one workgroup per chunk of kChunk consecutive points of ONE sample.  The BEV cells the
//            chunk touches get slots (wave-ballot compaction of an LDS presence table); the chunk's
//            in-range points are counting-sorted by slot in LDS; then one WAVE per slot streams its
//            point rows (coalesced 1 KiB loads, 4 in flight) into registers and writes the partial
//            row and the cell->slot table to the workspace with plain stores.
//   phase 2: one wave per (sample, cell): sums that cell's slots over the sample's chunks in chunk
//            order and adds them to the caller's output -- no global atomics, deterministic up to the
//            LDS accumulation order inside a chunk.
// Cells beyond the slot budget (never the case for Lift-Splat geometry; random indices in tests do
// hit it) fall back to global atomics inside phase 1.
// ---------------------------------------------------------------------------
// Point rows are read exactly once: a non-temporal 16 B load keeps them from displacing the index / partial lines in
// L2 and MALL (measured 0.61 -> 0.75 of HBM peak on the planned path, profiles/r02_voxel_pool_*).
typedef float vp_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 vp_load_row16(const float4* p, bool nt) {
    if (nt) {
        const vp_f4 t = __builtin_nontemporal_load(reinterpret_cast<const vp_f4*>(p));
        return make_float4(t.x, t.y, t.z, t.w);
    }
    return *p;
}

struct __attribute__((packed, aligned(4))) VpPoint { int x, y, z; };

// NV = float4 chunks per lane (ceil(C / 256)), RF = point rows in flight per wave (1 KiB loads each)
template <int NV, int RF, bool NT>
__global__ __launch_bounds__(512) void voxel_pool_p1_kernel(
    int num_points, int C, int X, int Y, int Z, int chunks_per_sample, int smax,
    const int32_t* __restrict__ geom, const float* __restrict__ feats, float* __restrict__ out,
    int32_t* __restrict__ pos_memo, float* __restrict__ partial, int* __restrict__ slot_table) {
    __shared__ int table[kMaxCells];           // cell -> slot (-1 none)
    __shared__ short cell_of[kChunk];          // point -> cell (-1 out of range)
    __shared__ unsigned short sorted[kChunk];  // point indices grouped by slot
    __shared__ int cnt[kMaxCells + 1];         // per-slot count, then exclusive offsets
    __shared__ int cursor[kMaxCells];
    __shared__ int nslots_sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cells = X * Y;
    const int chunk = blockIdx.x;
    const int b = chunk / chunks_per_sample;
    const int cis = chunk - b * chunks_per_sample;
    const long long p0 = (long long)b * num_points + (long long)cis * kChunk;
    const int npts = min(kChunk, num_points - cis * kChunk);
    for (int i = tid; i < cells; i += 512) table[i] = -1;
    __syncthreads();
    // pass A: cell per point, presence, pos_memo.  All of a thread's points are fetched (one 12 B load each) before the first
    // is used: one memory round trip per chunk instead of kChunk / 512
    {
        constexpr int kPA = kChunk / 512;
        const VpPoint* gp = reinterpret_cast<const VpPoint*>(geom) + p0;
        VpPoint pt[kPA];
#pragma unroll
        for (int k = 0; k < kPA; ++k) {
            const int i = tid + 512 * k;
            pt[k].x = -1; pt[k].y = -1; pt[k].z = -1;
            if (i < npts) pt[k] = gp[i];
        }
#pragma unroll
        for (int k = 0; k < kPA; ++k) {
            const int i = tid + 512 * k;
            if (i < npts) {
                const int x = pt[k].x, y = pt[k].y, z = pt[k].z;
                int c = -1;
                if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) {
                    c = y * X + x;
                    table[c] = -2;
                    if (pos_memo) {
                        const long long p = p0 + i;
                        pos_memo[p * 3] = b;
                        pos_memo[p * 3 + 1] = y;
                        pos_memo[p * 3 + 2] = x;
                    }
                }
                cell_of[i] = (short)c;
            }
        }
    }
    __syncthreads();
    if (wave == 0) {   // slot assignment by ballot compaction (cell order)
        int base = 0;
        for (int c0 = 0; c0 < cells; c0 += 64) {
            const int c = c0 + lane;
            const bool hit = (c < cells) && (table[c] == -2);
            const unsigned long long m = __ballot(hit);
            if (hit) table[c] = base + __popcll(m & ((1ull << lane) - 1ull));
            base += __popcll(m);
        }
        if (lane == 0) nslots_sh = base;
    }
    __syncthreads();
    const int ns = nslots_sh;
    for (int i = tid; i <= ns; i += 512) cnt[i] = 0;
    __syncthreads();
    for (int i = tid; i < npts; i += 512) {
        const int c = cell_of[i];
        if (c >= 0) atomicAdd(&cnt[table[c]], 1);
    }
    __syncthreads();
    if (wave == 0) {   // exclusive scan of the slot counts
        int carry = 0;
        for (int s0 = 0; s0 < ns; s0 += 64) {
            const int sidx = s0 + lane;
            const int v = (sidx < ns) ? cnt[sidx] : 0;
            int incl = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            if (sidx < ns) {
                cnt[sidx] = carry + incl - v;
                cursor[sidx] = carry + incl - v;
            }
            carry += __shfl(incl, 63);
        }
        if (lane == 0) cnt[ns] = carry;
    }
    __syncthreads();
    for (int i = tid; i < npts; i += 512) {
        const int c = cell_of[i];
        if (c >= 0) sorted[atomicAdd(&cursor[table[c]], 1)] = (unsigned short)i;
    }
    __syncthreads();
    // slot_table layout [b][cell][chunk_in_sample]: phase 2 reads a cell's chunks contiguously
    for (int c = tid; c < cells; c += 512) {
        const int sl = table[c];
        slot_table[((long long)b * cells + c) * chunks_per_sample + cis] = (sl >= 0 && sl < smax) ? sl : -1;
    }
    // pass B: one wave per slot, register accumulation, no atomics for slots < smax (no barrier after it: a wave leaves
    // as soon as its slots are done)
    const int c4 = C >> 2;
    for (int sl = wave; sl < ns; sl += 8) {
        const int beg = cnt[sl], end = cnt[sl + 1];
        float4 acc[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = beg; k < end; k += RF) {
            float4 row[RF][NV];
#pragma unroll
            for (int j = 0; j < RF; ++j)
                if (k + j < end) {
                    const float4* src = reinterpret_cast<const float4*>(feats + (p0 + sorted[k + j]) * (long long)C);
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const int ch = lane + 64 * v;
                        row[j][v] = (ch < c4) ? vp_load_row16(src + ch, NT) : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
#pragma unroll
            for (int j = 0; j < RF; ++j)
                if (k + j < end) {
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        acc[v].x += row[j][v].x; acc[v].y += row[j][v].y;
                        acc[v].z += row[j][v].z; acc[v].w += row[j][v].w;
                    }
                }
        }
        if (sl < smax) {
            float4* dst = reinterpret_cast<float4*>(partial + ((long long)chunk * smax + sl) * C);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int ch = lane + 64 * v;
                if (ch < c4) dst[ch] = acc[v];
            }
        } else {   // over the workspace budget: one atomic row per (chunk, cell)
            const int cell = cell_of[sorted[beg]];
            float* d = out + ((long long)b * cells + cell) * C;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int ch = lane + 64 * v;
                if (ch < c4) {
                    unsafeAtomicAdd(d + ch * 4 + 0, acc[v].x);
                    unsafeAtomicAdd(d + ch * 4 + 1, acc[v].y);
                    unsafeAtomicAdd(d + ch * 4 + 2, acc[v].z);
                    unsafeAtomicAdd(d + ch * 4 + 3, acc[v].w);
                }
            }
        }
    }
}

__global__ __launch_bounds__(64) void voxel_pool_p2_kernel(int C, int cells, int chunks_per_sample, int smax,
                                                           const float* __restrict__ partial,
                                                           const int* __restrict__ slot_table,
                                                           float* __restrict__ out) {
    const int bc = blockIdx.x;                  // b * cells + cell
    const int b = bc / cells;
    const int lane = threadIdx.x;
    const int c4 = C >> 2;
    float4 acc[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    bool any = false;
    const int* tab = slot_table + (long long)bc * chunks_per_sample;
    for (int k0 = 0; k0 < chunks_per_sample; k0 += 64) {
        const int k = k0 + lane;
        const int s = (k < chunks_per_sample) ? tab[k] : -1;
        unsigned long long m = __ballot(s >= 0);
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const int sj = __builtin_amdgcn_readlane(s, j);
            const long long chunk = (long long)b * chunks_per_sample + k0 + j;
            const float4* src = reinterpret_cast<const float4*>(partial + (chunk * smax + sj) * C);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int ch = lane + 64 * v;
                if (ch < c4) {
                    const float4 t = src[ch];
                    acc[v].x += t.x; acc[v].y += t.y; acc[v].z += t.z; acc[v].w += t.w;
                }
            }
            any = true;
        }
    }
    if (!any) return;
    float4* dst = reinterpret_cast<float4*>(out + (long long)bc * C);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int ch = lane + 64 * v;
        if (ch < c4) {
            float4 o = dst[ch];
            o.x += acc[v].x; o.y += acc[v].y; o.z += acc[v].z; o.w += acc[v].w;
            dst[ch] = o;
        }
    }
}

// Generic fallback (any C): one thread per (point, channel).  Correctness path
// for odd channel counts only.
__global__ __launch_bounds__(256) void voxel_pool_scalar_kernel(
    long long total_points, int num_points, int C, int X, int Y, int Z,
    const int32_t* __restrict__ geom, const float* __restrict__ feats,
    float* __restrict__ out, int32_t* __restrict__ pos_memo) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long p = t / C;
    const int c = (int)(t % C);
    if (p >= total_points) return;
    const int x = geom[p * 3 + 0], y = geom[p * 3 + 1], z = geom[p * 3 + 2];
    if (x < 0 || x >= X || y < 0 || y >= Y || z < 0 || z >= Z) return;
    const int b = (int)(p / num_points);
    if (pos_memo && c == 0) {
        pos_memo[p * 3 + 0] = b;
        pos_memo[p * 3 + 1] = y;
        pos_memo[p * 3 + 2] = x;
    }
    unsafeAtomicAdd(out + ((long long)(b * Y + y) * X + x) * C + c, feats[p * C + c]);
}

// ---------------------------------------------------------------------------
// backward: pure gather, one float4 per thread.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void voxel_pool_bwd_kernel(
    long long total_points, int C, int X, int Y, const int32_t* __restrict__ pos_memo,
    const float* __restrict__ grad_out, float* __restrict__ grad_in) {
    const int c4 = C >> 2;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long p = t / c4;
    const int ch = (int)(t % c4);
    if (p >= total_points) return;
    const int b = pos_memo[p * 3 + 0];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b != -1) {
        const int y = pos_memo[p * 3 + 1], x = pos_memo[p * 3 + 2];
        v = reinterpret_cast<const float4*>(grad_out + ((long long)(b * Y + y) * X + x) * C)[ch];
    }
    reinterpret_cast<float4*>(grad_in + p * C)[ch] = v;
}

__global__ __launch_bounds__(256) void voxel_pool_bwd_scalar_kernel(
    long long total_points, int C, int X, int Y, const int32_t* __restrict__ pos_memo,
    const float* __restrict__ grad_out, float* __restrict__ grad_in) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long p = t / C;
    const int c = (int)(t % C);
    if (p >= total_points) return;
    const int b = pos_memo[p * 3 + 0];
    float v = 0.f;
    if (b != -1) {
        const int y = pos_memo[p * 3 + 1], x = pos_memo[p * 3 + 2];
        v = grad_out[((long long)(b * Y + y) * X + x) * C + c];
    }
    grad_in[p * C + c] = v;
}

// ---------------------------------------------------------------------------
// Planned forward for STATIC geometry (a fixed camera rig: geom_xyz is the same every frame).  The plan sorts the
// in-range points by (sample, BEV cell) once (CSR: `order` = point indices grouped by cell, `cell_start`) and cuts
// every cell's run into segments of kSeg rows.  A forward is then pure streaming with no index work:
//   segments kernel : one wave per segment, kSegRF point rows (1 KiB each) in flight, register accumulation, one
//                     partial row per segment to the workspace (plain stores);
//   cells kernel    : one wave per (sample, cell) adds its segments' partial rows, in order, to the caller's output.
// No atomics, deterministic; HBM traffic = the in-range rows + 4 B per row of indices + 2 x 1/kSeg of the rows.
// ---------------------------------------------------------------------------
constexpr int kSegRF = 16;

__global__ void vp_plan_keys_kernel(long long total, int num_points, int X, int Y, int Z, const int32_t* __restrict__ geom,
                                    unsigned* __restrict__ keys, unsigned* __restrict__ vals, unsigned invalid_key) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const int x = geom[p * 3], y = geom[p * 3 + 1], z = geom[p * 3 + 2];
    unsigned k = invalid_key;
    if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) k = (unsigned)((p / num_points) * (long long)(X * Y) + y * X + x);
    keys[p] = k;
    vals[p] = (unsigned)p;
}

// cell_start[k] = first sorted position with key >= k (k = 0 .. nkeys), by binary search; one thread per key
__global__ void vp_plan_starts_kernel(const unsigned* __restrict__ sorted_keys, long long total, int nkeys,
                                      int* __restrict__ cell_start) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nkeys) return;
    long long lo = 0, hi = total;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (sorted_keys[mid] < (unsigned)k) lo = mid + 1;
        else hi = mid;
    }
    cell_start[k] = (int)lo;
}

// seg_off[k] = number of segments of the cells before k (exclusive scan of ceil(count / kSeg)), k = 0 .. nkeys;
// a single workgroup (nkeys is a few thousand)
__global__ __launch_bounds__(1024) void vp_plan_segments_kernel(const int* __restrict__ cell_start, int nkeys,
                                                                int* __restrict__ seg_off) {
    __shared__ int carry_sh;
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_sh = 0;
    __syncthreads();
    for (int k0 = 0; k0 < nkeys; k0 += 1024) {
        const int k = k0 + tid;
        const int v = (k < nkeys) ? (cell_start[k + 1] - cell_start[k] + kSeg - 1) / kSeg : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = carry_sh;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (k < nkeys) seg_off[k] = before + incl - v;
        __syncthreads();
        if (tid == 1023) carry_sh = before + incl;
        __syncthreads();
    }
    if (tid == 0) seg_off[nkeys] = carry_sh;
}

// Segments are numbered per GROUP of `cpg` cells: group `grp` owns segment ids [grp * segcap, (grp + 1) * segcap) and the
// entries [grp * (cpg + 1), (grp + 1) * (cpg + 1)) of cell_start (absolute positions in `order`) and seg_off (segments of the
// group's cells before cell k).  The static plan is ONE group of batch x cells keys (a global scan at build time); the
// per-launch sort of the generic path (vp_cs_*) makes one group per sample, so that no scan crosses samples.
template <int NV, int RF, bool NT>
__global__ __launch_bounds__(256) void vp_planned_segments_kernel(int C, int cpg, int segcap, int ngroups,
                                                                  const int* __restrict__ order,
                                                                  const int* __restrict__ cell_start,
                                                                  const int* __restrict__ seg_off,
                                                                  const float* __restrict__ feats,
                                                                  float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int g = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);      // segment
    const int grp = g / segcap;
    if (grp >= ngroups) return;
    const int gl = g - grp * segcap;
    seg_off += (long long)grp * (cpg + 1);
    cell_start += (long long)grp * (cpg + 1);
    if (gl >= seg_off[cpg]) return;
    // the cell of segment gl: last k with seg_off[k] <= gl (binary search over the group's cells)
    int lo = 0, hi = cpg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_off[mid] <= gl) lo = mid;
        else hi = mid;
    }
    const int beg = cell_start[lo] + (gl - seg_off[lo]) * kSeg;
    const int end = min(beg + kSeg, cell_start[lo + 1]);
    const int my = (beg + lane < end) ? order[beg + lane] : 0;
    const int c4 = C >> 2;
    float4 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < end - beg; k += RF) {
        float4 row[RF][NV];
#pragma unroll
        for (int j = 0; j < RF; ++j)
            if (k + j < end - beg) {
                const long long pt = (unsigned)__builtin_amdgcn_readlane(my, (k + j) & 63);
                const float4* src = reinterpret_cast<const float4*>(feats + pt * (long long)C);
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const int ch = lane + 64 * v;
                    row[j][v] = (ch < c4) ? vp_load_row16(src + ch, NT) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
#pragma unroll
        for (int j = 0; j < RF; ++j)
            if (k + j < end - beg) {
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    acc[v].x += row[j][v].x; acc[v].y += row[j][v].y;
                    acc[v].z += row[j][v].z; acc[v].w += row[j][v].w;
                }
            }
    }
    float4* dst = reinterpret_cast<float4*>(partial + (long long)g * C);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int ch = lane + 64 * v;
        if (ch < c4) dst[ch] = acc[v];
    }
}

// One workgroup of 4 waves per (sample, cell): wave w sums segments s0 + w, s0 + w + 4, ... with 4 partial rows in flight,
// then the four wave sums are combined in a fixed order through LDS (deterministic).
template <int NV>
__global__ __launch_bounds__(256) void vp_planned_cells_kernel(int C, int cpg, int segcap, const int* __restrict__ seg_off,
                                                               const float* __restrict__ partial, float* __restrict__ out) {
    __shared__ float4 red[3][NV * 64];
    const int key = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = key / cpg, cell = key - grp * cpg;
    seg_off += (long long)grp * (cpg + 1);
    const int s0 = grp * segcap + seg_off[cell], s1 = grp * segcap + seg_off[cell + 1];
    if (s0 == s1) return;
    const int c4 = C >> 2;
    float4 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int sg = s0 + wave; sg < s1; sg += 16) {
        float4 t[4][NV];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int sj = sg + 4 * j;
            const float4* src = reinterpret_cast<const float4*>(partial + (long long)min(sj, s1 - 1) * C);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int ch = lane + 64 * v;
                t[j][v] = (ch < c4) ? src[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (sg + 4 * j < s1) {
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    acc[v].x += t[j][v].x; acc[v].y += t[j][v].y; acc[v].z += t[j][v].z; acc[v].w += t[j][v].w;
                }
            }
    }
    if (wave > 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) red[wave - 1][v * 64 + lane] = acc[v];
    }
    __syncthreads();
    if (wave > 0) return;
    float4* dst = reinterpret_cast<float4*>(out + (long long)key * C);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int ch = lane + 64 * v;
        if (ch < c4) {
            float4 o = dst[ch];
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const float4 r = red[w][v * 64 + lane];
                acc[v].x += r.x; acc[v].y += r.y; acc[v].z += r.z; acc[v].w += r.w;
            }
            o.x += acc[v].x; o.y += acc[v].y; o.z += acc[v].z; o.w += acc[v].w;
            dst[ch] = o;
        }
    }
}

// ---------------------------------------------------------------------------
// v3 (round 5): the planned path for ARBITRARY geometry.  The static plan above needs the in-range points sorted by
// (sample, cell); a general radix sort of 4 M (key, point) pairs takes 2.2 ms -- nine times the operator.  But the keys are
// only `cells` (441) wide per sample, so the sort is a counting sort in three small kernels per launch:
//   vp_cs_count   : one workgroup per 8192 points.  Every wave ranks its 512 points by cell with wave ballots (a slice of 64
//                   consecutive frustum points falls into 1-4 cells: 1-4 ballots), per-(wave, cell) counts in LDS (u16), a
//                   column scan over the 16 waves, and out go one packed (cell, rank within the chunk) word per point and the
//                   chunk's count per cell.  pos_memo is written here.
//   vp_cs_scan    : one workgroup per SAMPLE: per cell the prefix over the sample's <= 64 chunks (held in registers), the
//                   exclusive scans of the cell totals (positions in `order`) and of ceil(total / 64) (segments); rewrites the
//                   table as absolute start positions per (chunk, cell).  Nothing crosses samples: sample b's rows live at
//                   order[b * Np ...) and its segments at [b * segcap, ...).
//   vp_cs_scatter : one thread per point: order[table[chunk][cell] + rank] = point.
// The order inside a cell is ascending point index -- what the stable radix sort of the static plan produces -- so the two paths
// add the same rows in the same order: bit-identical outputs.  Then the planned streaming kernels run as they are.
// Traffic on top of the rows: geom 12 B + 4 B written + 4 B read per point, 4 B per in-range point, < 1 MB of tables.
// ---------------------------------------------------------------------------
constexpr int kCsRankBits = 13;          // rank within a chunk < 8192

__global__ __launch_bounds__(kCsWaves * 64) void vp_cs_count_kernel(int num_points, int X, int Y, int Z, int cps,
                                                                    const int32_t* __restrict__ geom,
                                                                    int32_t* __restrict__ pos_memo,
                                                                    unsigned* __restrict__ keyrank, int* __restrict__ table) {
    // LDS: per wave a running count per cell (u16) and a 64-bit LANE MASK per cell (which lanes of the current slice fall into it)
    extern __shared__ unsigned long long cs_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cells = X * Y, cells_p = (cells + 63) & ~63;
    unsigned long long* cs_mask = cs_lds;                                                     // [kCsWaves][cells_p]
    unsigned short* cs_cnt = reinterpret_cast<unsigned short*>(cs_lds + kCsWaves * cells_p);  // [kCsWaves][cells_p]
    const int chunk = blockIdx.x;
    const int b = chunk / cps, cis = chunk - b * cps;
    const long long p0 = (long long)b * num_points + (long long)cis * kCsChunk;
    const int npts = min(kCsChunk, num_points - cis * kCsChunk);
    for (int i = tid; i < kCsWaves * cells_p; i += kCsWaves * 64) {
        cs_cnt[i] = 0;
        cs_mask[i] = 0ull;
    }
    constexpr int kSlices = kCsChunk / kCsWaves / 64;        // 8 slices of 64 consecutive points per wave
    const VpPoint* gp = reinterpret_cast<const VpPoint*>(geom) + p0;
    VpPoint pt[kSlices];
#pragma unroll
    for (int sl = 0; sl < kSlices; ++sl) {               // one round trip for all of a lane's points
        const int i = wave * (kSlices * 64) + sl * 64 + lane;
        pt[sl].x = -1; pt[sl].y = -1; pt[sl].z = -1;
        if (i < npts) pt[sl] = gp[i];
    }
    __syncthreads();
    unsigned short* mine = cs_cnt + wave * cells_p;
    unsigned long long* mmask = cs_mask + wave * cells_p;
    unsigned kr[kSlices];
#pragma unroll
    for (int sl = 0; sl < kSlices; ++sl) {
        const int i = wave * (kSlices * 64) + sl * 64 + lane;
        const int x = pt[sl].x, y = pt[sl].y, z = pt[sl].z;
        int key = -1;
        if (i < npts && x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) {
            key = y * X + x;
            if (pos_memo) {
                const long long p = p0 + i;
                pos_memo[p * 3] = b;
                pos_memo[p * 3 + 1] = y;
                pos_memo[p * 3 + 2] = x;
            }
        }
        // Rank of a point among the EARLIER points of the same cell in this wave's 512, without a loop over the slice's
        // distinct cells (a slice of 64 consecutive frustum points falls into ~20 cells: the ballot-per-cell form took 40 us per
        // launch, profiles/r05_voxel_pool_kernel_stats_a.csv): every lane ORs its bit into the cell's lane mask (an atomic OR is
        // order-independent: deterministic), reads the mask back -- the lanes of its cell -- and the cell's running count; the
        // lowest lane of each cell then advances the count and clears the mask.  A wave's LDS operations execute in program
        // order, and the region is the wave's own: no barrier.
        int rank = 0;
        if (key >= 0) {
            __hip_atomic_fetch_or(&mmask[key], 1ull << lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (key >= 0) {
            const unsigned long long m = mmask[key];
            const int base = mine[key];
            rank = base + (int)__popcll(m & ((1ull << lane) - 1ull));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // every lane has its mask and base before anyone rewrites them
            if ((int)__builtin_ctzll(m) == lane) {
                mine[key] = (unsigned short)(base + __popcll(m));
                mmask[key] = 0ull;
            }
        }
        kr[sl] = key >= 0 ? (((unsigned)key << kCsRankBits) | (unsigned)rank) : 0xFFFFFFFFu;
    }
    __syncthreads();
    // column scan over the waves: count of (wave, cell) -> rows of the cell in the waves before; the chunk's total to the table
    for (int c = tid; c < cells; c += kCsWaves * 64) {
        int run = 0;
#pragma unroll
        for (int w = 0; w < kCsWaves; ++w) {
            const int v = cs_cnt[w * cells_p + c];
            cs_cnt[w * cells_p + c] = (unsigned short)run;
            run += v;
        }
        table[(long long)chunk * cells + c] = run;
    }
    __syncthreads();
#pragma unroll
    for (int sl = 0; sl < kSlices; ++sl) {
        const int i = wave * (kSlices * 64) + sl * 64 + lane;
        if (i < npts) {
            unsigned v = kr[sl];
            if (v != 0xFFFFFFFFu) v += mine[v >> kCsRankBits];
            keyrank[p0 + i] = v;
        }
    }
}

__global__ __launch_bounds__(1024) void vp_cs_scan_kernel(int num_points, int cells, int cps, int* __restrict__ table,
                                                          int* __restrict__ cell_start, int* __restrict__ seg_off) {
    __shared__ int wsum[2][16];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int v[kCsMaxChunksPerSample];
    int total = 0;
    int* tab = table + (long long)b * cps * cells + t;
#pragma unroll
    for (int c = 0; c < kCsMaxChunksPerSample; ++c) v[c] = (t < cells && c < cps) ? tab[(long long)c * cells] : 0;
#pragma unroll
    for (int c = 0; c < kCsMaxChunksPerSample; ++c) total += v[c];
    const int segs = (total + kSeg - 1) / kSeg;
    // exclusive scans over the sample's cells (thread = cell): rows and segments
    int irow = total, iseg = segs;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(irow, o), s2 = __shfl_up(iseg, o);
        if (lane >= o) { irow += a; iseg += s2; }
    }
    if (lane == 63) { wsum[0][wave] = irow; wsum[1][wave] = iseg; }
    __syncthreads();
    int brow = 0, bseg = 0;
    for (int w = 0; w < wave; ++w) { brow += wsum[0][w]; bseg += wsum[1][w]; }
    const int row0 = b * num_points + brow + irow - total;        // absolute position in `order` of this cell's first row
    if (t < cells) {
        cell_start[(long long)b * (cells + 1) + t] = row0;
        seg_off[(long long)b * (cells + 1) + t] = bseg + iseg - segs;
        int run = row0;
#pragma unroll
        for (int c = 0; c < kCsMaxChunksPerSample; ++c)
            if (c < cps) {
                tab[(long long)c * cells] = run;
                run += v[c];
            }
    }
    if (t == cells - 1) {
        cell_start[(long long)b * (cells + 1) + cells] = row0 + total;
        seg_off[(long long)b * (cells + 1) + cells] = bseg + iseg;
    }
}

__global__ __launch_bounds__(256) void vp_cs_scatter_kernel(long long total, int num_points, int cells, int cps,
                                                            const unsigned* __restrict__ keyrank,
                                                            const int* __restrict__ table, int* __restrict__ order) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const unsigned v = keyrank[p];
    if (v == 0xFFFFFFFFu) return;
    const int b = (int)(p / num_points);
    const int cis = (int)((p - (long long)b * num_points) / kCsChunk);
    const int key = (int)(v >> kCsRankBits), rank = (int)(v & ((1u << kCsRankBits) - 1u));
    order[table[((long long)b * cps + cis) * cells + key] + rank] = (int)p;
}

// The two streaming kernels of the planned forward over the groups of a CSR plan (see vp_planned_segments_kernel).
static void launch_planned(int C, const VpCsrLayout& L, const VpLaunch* seg, const VpLaunch* cel, int nv, const char* csr_base,
                           const float* input_features, float* output_features, float* partial, hipStream_t st) {
    const int* order = reinterpret_cast<const int*>(csr_base + L.order);
    const int* cell_start = reinterpret_cast<const int*>(csr_base + L.cell_start);
    const int* seg_off = reinterpret_cast<const int*>(csr_base + L.seg_off);
    const int cpg = (int)L.cpg, segcap = (int)L.segcap;
    if (nv == 1) {
        hipLaunchKernelGGL((vp_planned_segments_kernel<1, 32, true>), dim3(seg->grid), dim3(seg->block), seg->lds, st, C, cpg, segcap,
                           L.ngroups, order, cell_start, seg_off, input_features, partial);
        hipLaunchKernelGGL(vp_planned_cells_kernel<1>, dim3(cel->grid), dim3(cel->block), cel->lds, st, C, cpg, segcap, seg_off, partial,
                           output_features);
    } else {
        hipLaunchKernelGGL((vp_planned_segments_kernel<4, 4, true>), dim3(seg->grid), dim3(seg->block), seg->lds, st, C, cpg, segcap,
                           L.ngroups, order, cell_start, seg_off, input_features, partial);
        hipLaunchKernelGGL(vp_planned_cells_kernel<4>, dim3(cel->grid), dim3(cel->block), cel->lds, st, C, cpg, segcap, seg_off, partial,
                           output_features);
    }
}

}  // namespace tt

using namespace tt;

// Validate -> choose: everything a forward does before it touches the device (tt_voxel_pool_fwd_plan stops here).  *launches:
// whether there is anything to launch (no points: the call returns 0).
static int pool_prepare(const VoxelPoolCall& k, int num_voxel_z, VoxelPoolChoice& c, bool* launches) {
    c = voxel_pool_choose(k);
    *launches = true;
    if (c.arm == VP_SORT || c.arm == VP_TWO_PHASE) {
        TT_REQUIRE(k.geom && k.feats && k.out, "tt_voxel_pool_fwd_ws: null pointer");
        return 0;
    }
    TT_REQUIRE(k.B >= 0 && k.Np >= 0 && k.C > 0, "tt_voxel_pool_fwd: bad sizes B=%d Np=%d C=%d", k.B, k.Np, k.C);
    TT_REQUIRE(k.X > 0 && k.Y > 0 && num_voxel_z > 0, "tt_voxel_pool_fwd: bad voxel grid");
    *launches = c.nlaunch > 0;
    if (!*launches) return 0;
    TT_REQUIRE(k.geom && k.feats && k.out, "tt_voxel_pool_fwd: null pointer");
    return 0;
}

static int pool_run(VoxelPoolCall k, int num_voxel_z, const int32_t* geom_xyz, const float* input_features, float* output_features,
                    int32_t* pos_memo, void* workspace, void* stream) {
    // > 64 KiB of dynamic LDS needs the opt-in (441 cells: 70 KiB, 1024: 160 KiB = the whole CU, which the opt-in asks for).  A
    // device that refuses it takes the next arm down instead -- the one launcher with a fallback, so no error text
    static_assert(kCsWaves * kCsMaxCells * (sizeof(unsigned short) + sizeof(unsigned long long)) <= 160 * 1024, "VP_SORT LDS");
    VoxelPoolChoice c;
    bool launches;
    if (int rc = pool_prepare(k, num_voxel_z, c, &launches)) return rc;
    if (c.arm == VP_SORT && lds_opt_in(reinterpret_cast<const void*>(vp_cs_count_kernel), 160 * 1024, nullptr) != 0) {
        k.lds_granted = false;
        if (int rc = pool_prepare(k, num_voxel_z, c, &launches)) return rc;
    }
    if (!launches) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int B = k.B, Np = k.Np, C = k.C, X = k.X, Y = k.Y, Z = num_voxel_z, cells = X * Y;
    const long long total = (long long)B * Np;
    char* w = static_cast<char*>(workspace);
    const VpLaunch* l = c.launch;
    switch (c.arm) {
        case VP_SORT: {
            unsigned* keyrank = reinterpret_cast<unsigned*>(w + c.keyrank);
            int* table = reinterpret_cast<int*>(w + c.table);
            hipLaunchKernelGGL(vp_cs_count_kernel, dim3(l[0].grid), dim3(l[0].block), l[0].lds, st, Np, X, Y, Z, c.cps, geom_xyz,
                               pos_memo, keyrank, table);
            hipLaunchKernelGGL(vp_cs_scan_kernel, dim3(l[1].grid), dim3(l[1].block), l[1].lds, st, Np, cells, c.cps, table,
                               reinterpret_cast<int*>(w + c.csr.cell_start), reinterpret_cast<int*>(w + c.csr.seg_off));
            hipLaunchKernelGGL(vp_cs_scatter_kernel, dim3(l[2].grid), dim3(l[2].block), l[2].lds, st, total, Np, cells, c.cps, keyrank,
                               table, reinterpret_cast<int*>(w + c.csr.order));
            launch_planned(C, c.csr, l + 3, l + 4, c.nv, w, input_features, output_features, reinterpret_cast<float*>(w + c.partial), st);
            return check_launch("tt_voxel_pool_fwd_ws");
        }
        case VP_TWO_PHASE: {
            float* partial = reinterpret_cast<float*>(w + c.partial);
            int* slot_table = reinterpret_cast<int*>(w + c.slot_table);
#define TT_P1(NV, RF)                                                                                                          \
    hipLaunchKernelGGL((voxel_pool_p1_kernel<NV, RF, true>), dim3(l[0].grid), dim3(l[0].block), l[0].lds, st, Np, C, X, Y, Z, c.cps, \
                       kSlotBudget, geom_xyz, input_features, output_features, pos_memo, partial, slot_table)
            if (c.nv == 1) {
                TT_P1(1, 16);
            } else {
                TT_P1(4, 4);
            }
#undef TT_P1
            hipLaunchKernelGGL(voxel_pool_p2_kernel, dim3(l[1].grid), dim3(l[1].block), l[1].lds, st, C, cells, c.cps, kSlotBudget,
                               partial, slot_table, output_features);
            return check_launch("tt_voxel_pool_fwd_ws");
        }
        case VP_ROWS:
#define LAUNCH(NV)                                                                                                              \
    hipLaunchKernelGGL(voxel_pool_rows_kernel<NV>, dim3(l[0].grid), dim3(l[0].block), l[0].lds, st, total, Np, C, X, Y, Z, geom_xyz, \
                       input_features, output_features, pos_memo)
            switch (c.nv) {
                case 1: LAUNCH(1); break;
                case 2: LAUNCH(2); break;
                case 3: LAUNCH(3); break;
                default: LAUNCH(4); break;
            }
#undef LAUNCH
            break;
        default:
            hipLaunchKernelGGL(voxel_pool_scalar_kernel, dim3(l[0].grid), dim3(l[0].block), l[0].lds, st, total, Np, C, X, Y, Z,
                               geom_xyz, input_features, output_features, pos_memo);
            break;
    }
    return check_launch("tt_voxel_pool_fwd");
}

static VoxelPoolCall pool_call(int B, int Np, int C, int X, int Y, const void* geom, const void* feats, const void* out,
                               const void* ws, long long ws_bytes, bool ws_entry) {
    VoxelPoolCall k;
    k.B = B; k.Np = Np; k.C = C; k.X = X; k.Y = Y; k.geom = geom; k.feats = feats; k.out = out;
    k.ws = ws_entry ? ws : nullptr; k.ws_bytes = ws_entry ? ws_bytes : 0; k.ws_entry = ws_entry; k.lds_granted = true;
    return k;
}

extern "C" int tt_voxel_pool_fwd(int batch_size, int num_points, int num_channels,
                                 int num_voxel_x, int num_voxel_y, int num_voxel_z,
                                 const int32_t* geom_xyz, const float* input_features,
                                 float* output_features, int32_t* pos_memo, void* stream) {
    return pool_run(pool_call(batch_size, num_points, num_channels, num_voxel_x, num_voxel_y, geom_xyz, input_features, output_features,
                              nullptr, 0, false),
                    num_voxel_z, geom_xyz, input_features, output_features, pos_memo, nullptr, stream);
}

extern "C" long long tt_voxel_pool_workspace_bytes(int batch_size, int num_points, int num_channels,
                                                   int num_voxel_x, int num_voxel_y) {
    return voxel_pool_workspace_bytes(batch_size, num_points, num_channels, num_voxel_x, num_voxel_y);
}

extern "C" int tt_voxel_pool_fwd_ws(int batch_size, int num_points, int num_channels, int num_voxel_x,
                                    int num_voxel_y, int num_voxel_z, const int32_t* geom_xyz,
                                    const float* input_features, float* output_features, int32_t* pos_memo,
                                    void* workspace, long long workspace_bytes, void* stream) {
    return pool_run(pool_call(batch_size, num_points, num_channels, num_voxel_x, num_voxel_y, geom_xyz, input_features, output_features,
                              workspace, workspace_bytes, true),
                    num_voxel_z, geom_xyz, input_features, output_features, pos_memo, workspace, stream);
}

extern "C" int tt_voxel_pool_fwd_plan(int batch_size, int num_points, int num_channels, int num_voxel_x, int num_voxel_y,
                                      int num_voxel_z, const int32_t* geom_xyz, const float* input_features,
                                      float* output_features, int32_t* pos_memo, void* workspace, long long workspace_bytes,
                                      int ws_entry, char* label, int label_bytes) {
    (void)pos_memo;
    VoxelPoolChoice c;
    bool launches;
    if (int rc = pool_prepare(pool_call(batch_size, num_points, num_channels, num_voxel_x, num_voxel_y, geom_xyz, input_features,
                                        output_features, workspace, workspace_bytes, ws_entry != 0),
                              num_voxel_z, c, &launches))
        return rc;
    TT_REQUIRE(label && label_bytes > 0, "tt_voxel_pool_fwd_plan: no room for the label");
    vp_label(c.launch, launches ? c.nlaunch : 0, c.nv, c.rf, nullptr, c.ws_bytes, label, (size_t)label_bytes);
    return 0;
}

extern "C" int tt_voxel_pool_bwd(int batch_size, int num_points, int num_channels,
                                 int num_voxel_x, int num_voxel_y, const int32_t* pos_memo,
                                 const float* grad_out_bhwc, float* grad_in, void* stream) {
    const long long total = (long long)batch_size * num_points;
    if (total == 0) return 0;
    TT_REQUIRE(pos_memo && grad_out_bhwc && grad_in, "tt_voxel_pool_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int C = num_channels;
    if (C % 4 == 0) {
        const long long threads = total * (C / 4);
        hipLaunchKernelGGL(voxel_pool_bwd_kernel, dim3((unsigned)div_up(threads, 256)), dim3(256), 0,
                           st, total, C, num_voxel_x, num_voxel_y, pos_memo, grad_out_bhwc, grad_in);
    } else {
        const long long threads = total * C;
        hipLaunchKernelGGL(voxel_pool_bwd_scalar_kernel, dim3((unsigned)div_up(threads, 256)),
                           dim3(256), 0, st, total, C, num_voxel_x, num_voxel_y, pos_memo,
                           grad_out_bhwc, grad_in);
    }
    return check_launch("tt_voxel_pool_bwd");
}

// ---- static-geometry plan ------------------------------------------------------------------------------------

extern "C" long long tt_voxel_pool_plan_bytes(int batch_size, int num_points, int num_voxel_x, int num_voxel_y) {
    return (long long)vp_static_plan_layout(batch_size, num_points, num_voxel_x, num_voxel_y).end;
}

// The build's workspace: keys | vals | keys_sorted (u32 [total] each, vp_align'ed) | the radix sort's own
static size_t plan_sort_bytes(long long total) {
    size_t sort_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr,
                                       (unsigned*)nullptr, (int)total);
    return sort_bytes;
}

extern "C" long long tt_voxel_pool_plan_workspace_bytes(int batch_size, int num_points) {
    const long long total = (long long)batch_size * num_points;
    return (long long)(3 * vp_align(4 * total) + vp_align(plan_sort_bytes(total)));
}

extern "C" int tt_voxel_pool_plan_build(int batch_size, int num_points, int num_voxel_x, int num_voxel_y, int num_voxel_z,
                                        const int32_t* geom_xyz, void* workspace, long long workspace_bytes, void* plan,
                                        long long plan_bytes, void* stream) {
    TT_REQUIRE(geom_xyz && workspace && plan, "tt_voxel_pool_plan_build: null pointer");
    const long long total = (long long)batch_size * num_points;
    const long long nkeys = (long long)batch_size * num_voxel_x * num_voxel_y;
    TT_REQUIRE(total > 0 && total < (1ll << 31) && nkeys < (1ll << 30), "tt_voxel_pool_plan_build: sizes");
    const VpCsrLayout L = vp_static_plan_layout(batch_size, num_points, num_voxel_x, num_voxel_y);
    TT_REQUIRE(workspace_bytes >= tt_voxel_pool_plan_workspace_bytes(batch_size, num_points) && plan_bytes >= (long long)L.end,
               "tt_voxel_pool_plan_build: buffers too small");
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    const size_t col = vp_align(4 * total);
    unsigned* keys = (unsigned*)w;
    unsigned* vals = (unsigned*)(w + col);
    unsigned* keys_sorted = (unsigned*)(w + 2 * col);
    void* tmp = w + 3 * col;
    size_t tmp_bytes = (size_t)(workspace_bytes - 3 * (long long)col);
    char* pl = (char*)plan;
    int* order = (int*)(pl + L.order);
    int* cell_start = (int*)(pl + L.cell_start);
    int* seg_off = (int*)(pl + L.seg_off);
    hipLaunchKernelGGL(vp_plan_keys_kernel, dim3((unsigned)div_up(total, 256)), dim3(256), 0, st, total, num_points,
                       num_voxel_x, num_voxel_y, num_voxel_z, geom_xyz, keys, vals, (unsigned)nkeys);
    int bits = 1;
    while ((1ll << bits) <= nkeys) ++bits;
    if (hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys, keys_sorted, vals, (unsigned*)order, (int)total, 0, bits,
                                           st) != hipSuccess) {
        set_error("tt_voxel_pool_plan_build: radix sort failed");
        return -2;
    }
    hipLaunchKernelGGL(vp_plan_starts_kernel, dim3((unsigned)div_up(nkeys + 1, 256)), dim3(256), 0, st, keys_sorted, total,
                       (int)nkeys, cell_start);
    hipLaunchKernelGGL(vp_plan_segments_kernel, dim3(1), dim3(1024), 0, st, cell_start, (int)nkeys, seg_off);
    return check_launch("tt_voxel_pool_plan_build");
}

extern "C" long long tt_voxel_pool_planned_workspace_bytes(int batch_size, int num_points, int num_channels,
                                                           int num_voxel_x, int num_voxel_y) {
    return vp_static_plan_layout(batch_size, num_points, num_voxel_x, num_voxel_y).partial_bytes(num_channels);
}

extern "C" int tt_voxel_pool_fwd_planned(int batch_size, int num_points, int num_channels, int num_voxel_x,
                                         int num_voxel_y, const void* plan, const float* input_features,
                                         float* output_features, void* workspace, long long workspace_bytes, void* stream) {
    TT_REQUIRE(plan && input_features && output_features && workspace, "tt_voxel_pool_fwd_planned: null pointer");
    const int C = num_channels;
    TT_REQUIRE(C % 4 == 0 && C <= 1024 && !(reinterpret_cast<uintptr_t>(input_features) & 15) &&
                   !(reinterpret_cast<uintptr_t>(output_features) & 15), "tt_voxel_pool_fwd_planned: C %% 4, 16 B alignment");
    const VpCsrLayout L = vp_static_plan_layout(batch_size, num_points, num_voxel_x, num_voxel_y);
    TT_REQUIRE(workspace_bytes >= L.partial_bytes(C), "tt_voxel_pool_fwd_planned: workspace too small");
    int nv, rf;
    VpLaunch l[2];
    vp_planned_launches(C, L, &nv, &rf, l);
    launch_planned(C, L, l, l + 1, nv, (const char*)plan, input_features, output_features, (float*)workspace, (hipStream_t)stream);
    return check_launch("tt_voxel_pool_fwd_planned");
}

