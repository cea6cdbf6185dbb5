// The Lift-Splat of the forward for gfx950 (wave64): kernels and entries.
//
//  tt_frustum_voxel_index        LSS.get_geometry + voxel index (backbones/lss.py:474-512,629-631).
//  tt_lift_splat_fwd / _fwd_ws   fused depth-softmax (x) context -> BEV (lss.py:583-615 + splat): a per-pixel atomic kernel,
//                                the strip kernel with atomics, and the strip kernel + lift_splat_cells_kernel (workspace form).
//
// Which of them a call runs on, with which grids, dynamic LDS and workspace offsets, is decided in voxel_pool_choose.cpp
// (lift_splat_choose); the entries here validate, ask the chooser and launch what it answers.  The op-boundary voxel pool is
// voxel_pool.hip.
#include "tt_common.h"
#include "voxel_pool_choose.h"

namespace tt {

// ---------------------------------------------------------------------------
// frustum -> ego -> voxel index.  Products and sums are written as separate
// IEEE roundings in k order (no FMA contraction) so the oracle can restate the
// exact same arithmetic.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float dot4_seq(const float* m, float a, float b, float c, float d) {
#pragma clang fp contract(off)
    float s = __fmul_rn(m[0], a);
    s = __fadd_rn(s, __fmul_rn(m[1], b));
    s = __fadd_rn(s, __fmul_rn(m[2], c));
    s = __fadd_rn(s, __fmul_rn(m[3], d));
    return s;
}

__global__ __launch_bounds__(256) void frustum_voxel_index_kernel(
    int B, int ncam, int D, int fH, int fW, const float* __restrict__ frustum,
    const float* __restrict__ mats, float lox, float loy, float loz, float sx, float sy, float sz,
    int32_t* __restrict__ geom_xyz, float* __restrict__ geom_f32) {
#pragma clang fp contract(off)
    const long long per_cam = (long long)D * fH * fW;
    const long long total = (long long)B * ncam * per_cam;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long bc = t / per_cam;
    const long long q = t % per_cam;
    const float* iida = mats + bc * 32;
    const float* comb = iida + 16;
    const float4 f = reinterpret_cast<const float4*>(frustum)[q];
    float p0 = dot4_seq(iida + 0, f.x, f.y, f.z, f.w);
    float p1 = dot4_seq(iida + 4, f.x, f.y, f.z, f.w);
    float p2 = dot4_seq(iida + 8, f.x, f.y, f.z, f.w);
    float p3 = dot4_seq(iida + 12, f.x, f.y, f.z, f.w);
    p0 = __fmul_rn(p0, p2);
    p1 = __fmul_rn(p1, p2);
    const float gx = dot4_seq(comb + 0, p0, p1, p2, p3);
    const float gy = dot4_seq(comb + 4, p0, p1, p2, p3);
    const float gz = dot4_seq(comb + 8, p0, p1, p2, p3);
    if (geom_f32) {
        geom_f32[t * 3 + 0] = gx;
        geom_f32[t * 3 + 1] = gy;
        geom_f32[t * 3 + 2] = gz;
    }
    // (geom - lo) / size, truncated toward zero like Tensor.int() (lss.py:630-631)
    geom_xyz[t * 3 + 0] = (int)__fdiv_rn(__fsub_rn(gx, lox), sx);
    geom_xyz[t * 3 + 1] = (int)__fdiv_rn(__fsub_rn(gy, loy), sy);
    geom_xyz[t * 3 + 2] = (int)__fdiv_rn(__fsub_rn(gz, loz), sz);
}

// ---------------------------------------------------------------------------
// fused lift-splat: one wave per image pixel (b, cam, h, w).
//   prob[d] = softmax_d(depth_logits[pix, :]);  out[cell(pix,d), :] += prob[d] * ctx[pix, :]
// Consecutive depth bins of one ray that fall in the same BEV cell are merged
// (sum of probabilities) before touching memory.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void lift_splat_kernel(
    int B, int ncam, int D, int fH, int fW, int C, int X, int Y, int Z,
    const T* __restrict__ depth_logits, const T* __restrict__ ctx,
    const int32_t* __restrict__ geom, float* __restrict__ out, int out_cstride, int out_coff,
    int rot_flip) {
    const int lane = threadIdx.x & 63;
    const long long pix = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long npix = (long long)B * ncam * fH * fW;
    if (pix >= npix) return;
    const int hw = (int)(pix % ((long long)fH * fW));
    const int bc = (int)(pix / ((long long)fH * fW));
    const int b = bc / ncam;
    const int cam = bc % ncam;

    // ---- softmax over D (D <= 128: two bins per lane)
    const T* lg = depth_logits + pix * D;
    float l0 = (lane < D) ? Elem<T>::ld(lg + lane) : -INFINITY;
    float l1 = (lane + 64 < D) ? Elem<T>::ld(lg + lane + 64) : -INFINITY;
    float m = fmaxf(l0, l1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float e0 = (lane < D) ? expf(l0 - m) : 0.f;
    float e1 = (lane + 64 < D) ? expf(l1 - m) : 0.f;
    float s = e0 + e1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float inv = 1.f / s;
    e0 *= inv;
    e1 *= inv;

    // ---- cell per depth bin
    const long long per_cam = (long long)D * fH * fW;
    const int32_t* g = geom + ((long long)b * ncam * per_cam + (long long)cam * per_cam) * 3;
    int cell0 = -1, cell1 = -1;
    if (lane < D) {
        const int32_t* q = g + ((long long)lane * fH * fW + hw) * 3;
        const int x = q[0], y = q[1], z = q[2];
        if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) cell0 = y * X + x;
    }
    if (lane + 64 < D) {
        const int32_t* q = g + ((long long)(lane + 64) * fH * fW + hw) * 3;
        const int x = q[0], y = q[1], z = q[2];
        if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) cell1 = y * X + x;
    }

    // ---- context row in registers (C <= 1024: up to 4 float4-chunks per lane)
    const int c4 = C >> 2;
    float4 cv[4];
    const T* crow = ctx + pix * C;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int ch = lane + 64 * v;
        if (ch < c4) {
            cv[v].x = Elem<T>::ld(crow + ch * 4 + 0);
            cv[v].y = Elem<T>::ld(crow + ch * 4 + 1);
            cv[v].z = Elem<T>::ld(crow + ch * 4 + 2);
            cv[v].w = Elem<T>::ld(crow + ch * 4 + 3);
        } else {
            cv[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }

    int cur = -1;
    float w = 0.f;
    auto flush = [&](int cell, float wsum) {
        int y = cell / X, x = cell % X;
        int oi = y, oj = x;
        if (rot_flip) {  // rot90(flip(bev,[2]),1,[2,3]): out[i][j] = bev[Y-1-j][X-1-i]
            oi = X - 1 - x;
            oj = Y - 1 - y;
        }
        const int OW = rot_flip ? Y : X;
        const int OH = rot_flip ? X : Y;
        float* dst = out + (((long long)b * OH + oi) * OW + oj) * out_cstride + out_coff;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int ch = lane + 64 * v;
            if (ch < c4) {
                unsafeAtomicAdd(dst + ch * 4 + 0, wsum * cv[v].x);
                unsafeAtomicAdd(dst + ch * 4 + 1, wsum * cv[v].y);
                unsafeAtomicAdd(dst + ch * 4 + 2, wsum * cv[v].z);
                unsafeAtomicAdd(dst + ch * 4 + 3, wsum * cv[v].w);
            }
        }
    };
    for (int d = 0; d < D; ++d) {
        const int src_lane = d & 63;
        const int c = (d < 64) ? __builtin_amdgcn_readlane(cell0, src_lane)
                               : __builtin_amdgcn_readlane(cell1, src_lane);
        const float pr = __uint_as_float(
            (d < 64) ? __builtin_amdgcn_readlane(__float_as_uint(e0), src_lane)
                     : __builtin_amdgcn_readlane(__float_as_uint(e1), src_lane));
        if (c != cur) {
            if (cur >= 0) flush(cur, w);
            cur = c;
            w = 0.f;
        }
        w += pr;
    }
    if (cur >= 0) flush(cur, w);
}


// ---------------------------------------------------------------------------
// fused lift-splat v2: workgroup-level pre-reduction.  One workgroup owns a full-height strip of
// kStripW image columns of one camera: all its rays share (almost) the same azimuth, so the strip's
// 28 x kStripW x 80 frustum points fall into only ~10-30 BEV cells.  The block
//   1. softmaxes every pixel's depth logits into LDS and tags each (pixel, depth) with its cell,
//   2. gives the touched cells LDS slots (ballot compaction) and builds W[slot][pixel] = sum of the
//      depth probabilities that pixel sends to that cell,
//   3. forms sum_pixel W[slot][pixel] * context[pixel, :] with one wave per slot (context rows are
//      coalesced 1 KiB loads, L2 resident) and issues ONE atomic row per (strip, cell)
// -- ~13x fewer global atomics than the one-wave-per-pixel kernel above.
// With a workspace (tt_lift_splat_fwd_ws) there are no atomics at all: step 2 builds W with one thread per pixel
// walking its ray in depth order, step 3 stores the (strip, cell) partial rows to ws_rows[block][slot][C] and the
// block's cell -> slot table to slot_of[block][cell]; lift_splat_cells_kernel then adds every cell's partial rows to
// the output in block order.  Same inputs => bit-identical output.
// The strip's limits (kStripW, kMaxStripPix, kMaxSlots, kMaxD, kStageC) and the dynamic LDS layout are in voxel_pool_choose.h.
// ---------------------------------------------------------------------------

struct __attribute__((packed, aligned(4))) GeomPoint { int x, y, z; };

template <typename T>
__global__ __launch_bounds__(256) void lift_splat_strip_kernel(
    int B, int ncam, int D, int fH, int fW, int C, int X, int Y, int Z, const T* __restrict__ depth_logits,
    const T* __restrict__ ctx, const int32_t* __restrict__ geom, float* __restrict__ out, int out_cstride,
    int out_coff, int rot_flip, float* __restrict__ ws_rows, unsigned char* __restrict__ slot_of) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ls_smem[];
    __shared__ int nslots_sh;
    const int cells = X * Y;
    const int CW = min(C, kStageC);                 // channels per staged chunk of the context rows
    const int PD = lift_splat_prob_stride(D);
    float* Wt = reinterpret_cast<float*>(ls_smem);                          // [p][slot]
    int* table = reinterpret_cast<int*>(Wt + kWS * kMaxStripPix);
    int* slot_cell = table + cells;
    float* prob = reinterpret_cast<float*>(table + lift_splat_table_words(cells));      // [p][PD]
    short* tag = reinterpret_cast<short*>(prob + kMaxStripPix * PD);        // [d][npx]: cell, then slot
    float* ctxs = prob;                                                     // [p][CW], once prob / tag are spent
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int strips = (fW + kStripW - 1) / kStripW;
    // workgroup -> strip: hardware deals consecutive workgroups to the 8 XCDs in turn; give every XCD a CONTIGUOUS range of
    // strips, so that the neighbouring image columns that share 128 B lines of geom_xyz (10.7 points per line, 2 per strip
    // row) are fetched through the same L2
    const int nblk = gridDim.x, xcd = blockIdx.x & 7, full = nblk >> 3, rem = nblk & 7;
    const int vb = xcd * full + min(xcd, rem) + (blockIdx.x >> 3);
    const int bc = vb / strips;            // b * ncam + cam
    const int strip = vb % strips;
    const int b = bc / ncam, cam = bc % ncam;
    const int w0 = strip * kStripW;
    const int sw = min(kStripW, fW - w0);
    const int npx = fH * sw;                        // pixels in this strip: p -> (h = p / sw, w = w0 + p % sw)

    // context rows of one channel chunk: global -> registers (issued early, under other work) -> LDS as f32
    constexpr int kS = kMaxStripPix * (kStageC / 4) / 256;         // 8 float4 pieces per thread at the limits
    float4 cv[kS];
    auto ctx_fetch = [&](int c0) {
        const int cw4 = min(kStageC, C - c0) >> 2, tot = npx * cw4;
#pragma unroll
        for (int k = 0; k < kS; ++k) {
            const int i = k * 256 + tid;
            cv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < tot) {
                const int p = i / cw4, j = i - p * cw4;
                const int h = p / sw, w = w0 + p - h * sw;
                const T* crow = ctx + (((long long)bc * fH + h) * fW + w) * C + c0 + j * 4;
                if constexpr (sizeof(T) == 4) {
                    cv[k] = *reinterpret_cast<const float4*>(crow);
                } else {
                    cv[k].x = Elem<T>::ld(crow + 0); cv[k].y = Elem<T>::ld(crow + 1);
                    cv[k].z = Elem<T>::ld(crow + 2); cv[k].w = Elem<T>::ld(crow + 3);
                }
            }
        }
    };
    auto ctx_commit = [&](int c0) {
        const int cw4 = min(kStageC, C - c0) >> 2, tot = npx * cw4;
#pragma unroll
        for (int k = 0; k < kS; ++k) {
            const int i = k * 256 + tid;
            if (i < tot) {
                const int p = i / cw4, j = i - p * cw4;
                reinterpret_cast<float4*>(ctxs + p * CW)[j] = cv[k];
            }
        }
    };

    for (int i = tid; i < cells; i += 256) table[i] = -1;
    for (int i = tid; i < kWS * kMaxStripPix; i += 256) Wt[i] = 0.f;
    // depth logits of the strip: coalesced 16 B pieces -> registers now, LDS after the geometry pass
    constexpr int kL = kMaxStripPix * (kMaxD / 4) / 256;          // 8 pieces per thread at the limits
    const bool logits16 = (D & 3) == 0 && sizeof(T) == 4;
    float4 lv[kL];
    if (logits16) {
        const int d4 = D >> 2, tot4 = npx * d4;
#pragma unroll
        for (int k = 0; k < kL; ++k) {
            const int i = k * 256 + tid;
            lv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < tot4) {
                const int p = i / d4, j = i - p * d4;
                const int h = p / sw, w = w0 + p - h * sw;
                lv[k] = reinterpret_cast<const float4*>(depth_logits + (((long long)bc * fH + h) * fW + w) * D)[j];
            }
        }
    }
    __syncthreads();
    const long long per_cam = (long long)D * fH * fW;
    const GeomPoint* g = reinterpret_cast<const GeomPoint*>(geom) + ((long long)b * ncam + cam) * per_cam;
    // 1a. cell tags: every thread takes (depth, pixel) pairs, one 12 B load per point, a batch of loads before the first use
    {
        constexpr int kG = 18;
        const int tot = D * npx;
        for (int i0 = 0; i0 < tot; i0 += 256 * kG) {
            GeomPoint gp[kG];
#pragma unroll
            for (int k = 0; k < kG; ++k) {
                const int i = i0 + k * 256 + tid;
                gp[k].x = -1; gp[k].y = -1; gp[k].z = -1;
                if (i < tot) {
                    const int d = i / npx, p = i - d * npx;
                    const int h = p / sw, w = w0 + p - h * sw;
                    gp[k] = g[(long long)d * fH * fW + (long long)h * fW + w];
                }
            }
#pragma unroll
            for (int k = 0; k < kG; ++k) {
                const int i = i0 + k * 256 + tid;
                if (i < tot) {
                    const int d = i / npx, p = i - d * npx;
                    const int x = gp[k].x, y = gp[k].y, z = gp[k].z;
                    int c = -1;
                    if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) {
                        c = y * X + x;
                        table[c] = -2;
                    }
                    tag[i] = (short)c;
                }
            }
        }
    }
    // 1b. softmax over depth: logits -> LDS (coalesced rows), then four adjacent lanes per pixel (depth bins q, q+4, ...)
    // with two quad-shuffle steps per reduction
    {
        if (logits16) {
            const int d4 = D >> 2, tot4 = npx * d4;
#pragma unroll
            for (int k = 0; k < kL; ++k) {
                const int i = k * 256 + tid;
                if (i < tot4) {
                    const int p = i / d4, j = i - p * d4;
                    reinterpret_cast<float4*>(prob + p * PD)[j] = lv[k];
                }
            }
        } else {
            for (int i = tid; i < npx * D; i += 256) {
                const int p = i / D, d = i - p * D;
                const int h = p / sw, w = w0 + p - h * sw;
                prob[p * PD + d] = Elem<T>::ld(depth_logits + (((long long)bc * fH + h) * fW + w) * D + d);
            }
        }
        __syncthreads();
        const int p = tid >> 2, q = tid & 3;
        if (p < npx) {                              // whole quads take the branch together
            float* pr = prob + p * PD;
            float m = -INFINITY;
            for (int d = q; d < D; d += 4) m = fmaxf(m, pr[d]);
            m = fmaxf(m, __shfl_xor(m, 1));
            m = fmaxf(m, __shfl_xor(m, 2));
            float ssum = 0.f;
            for (int d = q; d < D; d += 4) {
                const float e = expf(pr[d] - m);
                pr[d] = e;
                ssum += e;
            }
            ssum += __shfl_xor(ssum, 1);
            ssum += __shfl_xor(ssum, 2);
            const float inv = 1.f / ssum;
            for (int d = q; d < D; d += 4) pr[d] *= inv;
        }
    }
    __syncthreads();
    // 2. slots
    if (wave == 0) {
        int base = 0;
        for (int c0 = 0; c0 < cells; c0 += 64) {
            const int c = c0 + lane;
            const bool hit = (c < cells) && (table[c] == -2);
            const unsigned long long mk = __ballot(hit);
            if (hit) {
                const int sidx = base + __popcll(mk & ((1ull << lane) - 1ull));
                table[c] = sidx;
                if (sidx < kMaxSlots) slot_cell[sidx] = c;
            }
            base += __popcll(mk);
        }
        if (lane == 0) nslots_sh = base;
    }
    __syncthreads();
    const int ns = nslots_sh;
    auto out_row = [&](int cell) {
        const int y = cell / X, x = cell % X;
        int oi = y, oj = x;
        if (rot_flip) { oi = X - 1 - x; oj = Y - 1 - y; }
        const int OW = rot_flip ? Y : X, OH = rot_flip ? X : Y;
        return out + (((long long)b * OH + oi) * OW + oj) * out_cstride + out_coff;
    };
    if (slot_of) {
        for (int i = tid; i < cells; i += 256) {
            const int t = table[i];
            slot_of[(long long)vb * cells + i] = (unsigned char)((t >= 0 && t < kMaxSlots) ? t : 255);
        }
    }
    // cell tags -> slot tags (over-budget cells keep their cell as -(cell + 2))
    {
        constexpr int kT = 4;
        const int tot = D * npx;
        for (int i0 = 0; i0 < tot; i0 += 256 * kT) {
            int c[kT], t[kT];
#pragma unroll
            for (int k = 0; k < kT; ++k) {
                const int i = i0 + k * 256 + tid;
                c[k] = (i < tot) ? (int)tag[i] : -1;
            }
#pragma unroll
            for (int k = 0; k < kT; ++k) t[k] = table[c[k] < 0 ? 0 : c[k]];
#pragma unroll
            for (int k = 0; k < kT; ++k) {
                const int i = i0 + k * 256 + tid;
                if (i < tot && c[k] >= 0) tag[i] = (short)(t[k] < kMaxSlots ? t[k] : -(c[k] + 2));
            }
        }
    }
    ctx_fetch(0);           // first chunk of context rows: in flight under the W build
    __syncthreads();
    // W[pixel][slot] += prob, one thread per pixel walking its ray front to back.  ds_add_f32 is used as a fire-and-forget
    // add (no read-modify-write round trip per depth bin): every address has exactly one writer thread and the LDS executes a
    // wave's operations in program order, so the sum is formed in depth order -- deterministic.  Pairs whose slot is over
    // budget go straight to global atomics below.
    if (tid < npx) {
        constexpr int kW = 8;
        for (int d0 = 0; d0 < D; d0 += kW) {
            int sg[kW];
            float pr[kW];
#pragma unroll
            for (int k = 0; k < kW; ++k) {
                const int d = min(d0 + k, D - 1);
                sg[k] = tag[d * npx + tid];
                pr[k] = prob[tid * PD + d];
            }
#pragma unroll
            for (int k = 0; k < kW; ++k)
                if (d0 + k < D && sg[k] >= 0) atomicAdd(&Wt[tid * kWS + sg[k]], pr[k]);
        }
    }
    __syncthreads();
    if (ns > kMaxSlots) {   // rare (never with Lift-Splat geometry): per-(pixel,depth) atomics for the excess cells
        for (int i = wave; i < npx * D; i += 4) {
            const int tg = tag[i];
            if (tg >= -1) continue;
            const int c = -tg - 2;
            const int d = i / npx, p = i - d * npx;
            const float wgt = prob[p * PD + d];
            const int h = p / sw, w = w0 + p % sw;
            const T* crow = ctx + (((long long)bc * fH + h) * fW + w) * C;
            float* dst = out_row(c);
            for (int ch = lane; ch < C; ch += 64) unsafeAtomicAdd(dst + ch, wgt * Elem<T>::ld(crow + ch));
        }
    }
    const int nsl = min(ns, kMaxSlots);
    // 3. rows[slot][:] = sum_p W[p][slot] * ctx[p][:] as a small dense product, kStageC channels at a time: the strip's
    // context rows are staged in LDS (f32); a task = (4 slots, one float4 column): 2 x 16 B of LDS per 16 FMAs, only live
    // slots get tasks, pixels in index order
    for (int c0 = 0; c0 < C; c0 += kStageC) {
        const int cw4 = min(kStageC, C - c0) >> 2;
        __syncthreads();        // prob / tag (first chunk) or the previous chunk's rows are no longer read
        ctx_commit(c0);
        __syncthreads();
        if (c0 + kStageC < C) ctx_fetch(c0 + kStageC);     // next chunk's rows fly under this chunk's product
        const int ntask = (kStageC / 4) * ((nsl + 3) >> 2);
        for (int task = tid; task < ntask; task += 256) {
            const int j = task & (kStageC / 4 - 1), sgp = task / (kStageC / 4);
            if (j >= cw4) continue;
            float4 acc[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
            for (int p = 0; p < npx; ++p) {
                const float4 wq = *reinterpret_cast<const float4*>(Wt + p * kWS + sgp * 4);
                const float4 x = reinterpret_cast<const float4*>(ctxs + p * CW)[j];
                acc[0].x += wq.x * x.x; acc[0].y += wq.x * x.y; acc[0].z += wq.x * x.z; acc[0].w += wq.x * x.w;
                acc[1].x += wq.y * x.x; acc[1].y += wq.y * x.y; acc[1].z += wq.y * x.z; acc[1].w += wq.y * x.w;
                acc[2].x += wq.z * x.x; acc[2].y += wq.z * x.y; acc[2].z += wq.z * x.z; acc[2].w += wq.z * x.w;
                acc[3].x += wq.w * x.x; acc[3].y += wq.w * x.y; acc[3].z += wq.w * x.z; acc[3].w += wq.w * x.w;
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int slot = sgp * 4 + v;
                if (slot >= nsl) continue;
                if (ws_rows) {
                    reinterpret_cast<float4*>(ws_rows + ((long long)vb * kMaxSlots + slot) * C + c0)[j] = acc[v];
                } else {
                    float* dst = out_row(slot_cell[slot]) + c0 + j * 4;
                    unsafeAtomicAdd(dst + 0, acc[v].x);
                    unsafeAtomicAdd(dst + 1, acc[v].y);
                    unsafeAtomicAdd(dst + 2, acc[v].z);
                    unsafeAtomicAdd(dst + 3, acc[v].w);
                }
            }
        }
    }
}

// second pass of the atomics-free lift-splat: one wave per (sample, BEV cell) finds the strips that produced a partial
// row for the cell (slot_of[block][cell], the blocks of one sample are contiguous) and adds them in block order.
__global__ __launch_bounds__(256) void lift_splat_cells_kernel(int B, int blocks_per_sample, int C, int X, int Y,
                                                               const float* __restrict__ ws_rows,
                                                               const unsigned char* __restrict__ slot_of,
                                                               float* __restrict__ out, int out_cstride, int out_coff,
                                                               int rot_flip) {
    const int lane = threadIdx.x & 63;
    const int cells = X * Y;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long long)B * cells) return;
    const int b = (int)(wid / cells), cell = (int)(wid % cells);
    const int c4 = C >> 2;
    float4 acc[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    bool any = false;
    for (int k0 = 0; k0 < blocks_per_sample; k0 += 64) {
        const int k = k0 + lane;
        int s = 255;
        if (k < blocks_per_sample) s = slot_of[((long long)b * blocks_per_sample + k) * cells + cell];
        unsigned long long mk = __ballot(s != 255);
        while (mk) {
            const int l = __ffsll((long long)mk) - 1;
            mk &= mk - 1;
            const int sl = __shfl(s, l);
            const float4* wr = reinterpret_cast<const float4*>(
                ws_rows + (((long long)b * blocks_per_sample + k0 + l) * kMaxSlots + sl) * C);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int ch = lane + 64 * v;
                if (ch < c4) {
                    const float4 r = wr[ch];
                    acc[v].x += r.x; acc[v].y += r.y; acc[v].z += r.z; acc[v].w += r.w;
                }
            }
            any = true;
        }
    }
    if (!any) return;
    const int y = cell / X, x = cell % X;
    int oi = y, oj = x;
    if (rot_flip) { oi = X - 1 - x; oj = Y - 1 - y; }
    const int OW = rot_flip ? Y : X, OH = rot_flip ? X : Y;
    float4* dst = reinterpret_cast<float4*>(out + (((long long)b * OH + oi) * OW + oj) * out_cstride + out_coff);
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

template <typename T>
static int launch_lift_splat(const LiftSplatChoice& c, int batch_size, int num_cams, int D, int fH, int fW, int C, int X, int Y, int Z,
                             const void* depth_logits, const void* context, const int32_t* geom_xyz, float* out, int out_cstride,
                             int out_coff, int rot_flip, void* ws, hipStream_t st) {
    const VpLaunch* l = c.launch;
    if (c.arm == LS_PIXEL) {
        hipLaunchKernelGGL(lift_splat_kernel<T>, dim3(l[0].grid), dim3(l[0].block), l[0].lds, st, batch_size, num_cams, D, fH, fW, C,
                           X, Y, Z, (const T*)depth_logits, (const T*)context, geom_xyz, out, out_cstride, out_coff, rot_flip);
        return 0;
    }
    float* ws_rows = c.arm == LS_STRIP_CELLS ? (float*)ws : nullptr;
    unsigned char* slot_of = c.arm == LS_STRIP_CELLS ? (unsigned char*)ws + c.slot_of : nullptr;
    if (lds_opt_in(reinterpret_cast<const void*>(lift_splat_strip_kernel<T>), c.lds_opt_in, "lift_splat_strip_kernel")) return -1;
    hipLaunchKernelGGL(lift_splat_strip_kernel<T>, dim3(l[0].grid), dim3(l[0].block), l[0].lds, st, batch_size, num_cams, D, fH, fW,
                       C, X, Y, Z, (const T*)depth_logits, (const T*)context, geom_xyz, out, out_cstride, out_coff, rot_flip,
                       ws_rows, slot_of);
    if (c.arm == LS_STRIP_CELLS)
        hipLaunchKernelGGL(lift_splat_cells_kernel, dim3(l[1].grid), dim3(l[1].block), l[1].lds, st, batch_size, num_cams * c.strips,
                           C, X, Y, ws_rows, slot_of, out, out_cstride, out_coff, rot_flip);
    return 0;
}

}  // namespace tt

using namespace tt;

extern "C" int tt_frustum_voxel_index(int batch_size, int num_cams, int D, int fH, int fW,
                                      const float* frustum, const float* mats,
                                      const float* voxel_lo, const float* voxel_size,
                                      int32_t* geom_xyz, float* geom_f32_or_null, void* stream) {
    TT_REQUIRE(frustum && mats && voxel_lo && voxel_size && geom_xyz,
               "tt_frustum_voxel_index: null pointer");
    const long long total = (long long)batch_size * num_cams * D * fH * fW;
    if (total == 0) return 0;
    // voxel_lo / voxel_size are HOST pointers (3 floats each): module constants.
    hipLaunchKernelGGL(frustum_voxel_index_kernel, dim3((unsigned)div_up(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, batch_size, num_cams, D, fH, fW, frustum, mats,
                       voxel_lo[0], voxel_lo[1], voxel_lo[2], voxel_size[0], voxel_size[1],
                       voxel_size[2], geom_xyz, geom_f32_or_null);
    return check_launch("tt_frustum_voxel_index");
}

extern "C" long long tt_lift_splat_workspace_bytes(int batch_size, int num_cams, int D, int fH, int fW, int C,
                                                   int num_voxel_x, int num_voxel_y) {
    return lift_splat_choose(batch_size, num_cams, D, fH, fW, C, num_voxel_x, num_voxel_y, true).ws_bytes;
}

// Validate -> choose: everything a launch does before it touches the device (tt_lift_splat_fwd_plan stops here).  *type: the
// storage type as the kernel's template argument is printed; *launches: whether there is anything to launch (no pixels: 0).
static int lift_splat_prepare(int batch_size, int num_cams, int D, int fH, int fW, int C, int num_voxel_x, int num_voxel_y,
                              const void* depth_logits, const void* context, int dtype, const int32_t* geom_xyz, const float* out,
                              int out_cstride, int out_coff, const void* ws, long long ws_bytes, LiftSplatChoice& c,
                              const char** type, bool* launches) {
    TT_REQUIRE(depth_logits && context && geom_xyz && out, "tt_lift_splat_fwd: null pointer");
    TT_REQUIRE(D > 0 && D <= 128, "tt_lift_splat_fwd: D=%d unsupported (1..128)", D);
    TT_REQUIRE(C > 0 && C % 4 == 0 && C <= 1024, "tt_lift_splat_fwd: C=%d unsupported", C);
    TT_REQUIRE(out_cstride % 4 == 0 && out_coff % 4 == 0 || !ws, "tt_lift_splat_fwd: workspace form needs 16 B aligned rows");
    *launches = (long long)batch_size * num_cams * fH * fW != 0;
    if (!*launches) return 0;
    c = lift_splat_choose(batch_size, num_cams, D, fH, fW, C, num_voxel_x, num_voxel_y, ws != nullptr);
    if (c.arm == LS_STRIP_CELLS)
        TT_REQUIRE(ws_bytes >= c.ws_bytes, "tt_lift_splat_fwd_ws: workspace %lld B < %lld B", ws_bytes, c.ws_bytes);
    *type = dtype == TT_F32 ? "float" : dtype == TT_BF16 ? "unsigned short" : dtype == TT_F16 ? "tt::f16_t" : nullptr;
    TT_REQUIRE(*type, "tt_lift_splat_fwd: bad dtype %d", dtype);
    return 0;
}

// `ws` (tt_lift_splat_workspace_bytes, contents don't matter) selects the atomics-free, bit-reproducible form; without
// it (or for shapes outside the strip kernel's limits) the partial rows are added with f32 atomics.
extern "C" int tt_lift_splat_fwd_ws(int batch_size, int num_cams, int D, int fH, int fW, int C,
                                    int num_voxel_x, int num_voxel_y, int num_voxel_z,
                                    const void* depth_logits, const void* context, int dtype,
                                    const int32_t* geom_xyz, float* out, int out_cstride, int out_coff,
                                    int rot_flip, void* ws, long long ws_bytes, void* stream) {
    LiftSplatChoice c;
    const char* type;
    bool launches;
    if (int rc = lift_splat_prepare(batch_size, num_cams, D, fH, fW, C, num_voxel_x, num_voxel_y, depth_logits, context, dtype,
                                    geom_xyz, out, out_cstride, out_coff, ws, ws_bytes, c, &type, &launches))
        return rc;
    if (!launches) return 0;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    switch (dtype) {
        case TT_F32:
            rc = launch_lift_splat<float>(c, batch_size, num_cams, D, fH, fW, C, num_voxel_x, num_voxel_y, num_voxel_z, depth_logits,
                                          context, geom_xyz, out, out_cstride, out_coff, rot_flip, ws, st);
            break;
        case TT_BF16:
            rc = launch_lift_splat<uint16_t>(c, batch_size, num_cams, D, fH, fW, C, num_voxel_x, num_voxel_y, num_voxel_z, depth_logits,
                                             context, geom_xyz, out, out_cstride, out_coff, rot_flip, ws, st);
            break;
        default:
            rc = launch_lift_splat<f16_t>(c, batch_size, num_cams, D, fH, fW, C, num_voxel_x, num_voxel_y, num_voxel_z, depth_logits,
                                          context, geom_xyz, out, out_cstride, out_coff, rot_flip, ws, st);
            break;
    }
    return rc ? rc : check_launch("tt_lift_splat_fwd");
}

extern "C" int tt_lift_splat_fwd(int batch_size, int num_cams, int D, int fH, int fW, int C,
                                 int num_voxel_x, int num_voxel_y, int num_voxel_z,
                                 const void* depth_logits, const void* context, int dtype,
                                 const int32_t* geom_xyz, float* out, int out_cstride, int out_coff,
                                 int rot_flip, void* stream) {
    return tt_lift_splat_fwd_ws(batch_size, num_cams, D, fH, fW, C, num_voxel_x, num_voxel_y, num_voxel_z, depth_logits,
                                context, dtype, geom_xyz, out, out_cstride, out_coff, rot_flip, nullptr, 0, stream);
}

extern "C" int tt_lift_splat_fwd_plan(int batch_size, int num_cams, int D, int fH, int fW, int C,
                                      int num_voxel_x, int num_voxel_y, int num_voxel_z,
                                      const void* depth_logits, const void* context, int dtype,
                                      const int32_t* geom_xyz, float* out, int out_cstride, int out_coff,
                                      int rot_flip, void* ws, long long ws_bytes, char* label, int label_bytes) {
    (void)num_voxel_z;
    (void)rot_flip;
    LiftSplatChoice c{};
    const char* type = nullptr;
    bool launches;
    if (int rc = lift_splat_prepare(batch_size, num_cams, D, fH, fW, C, num_voxel_x, num_voxel_y, depth_logits, context, dtype,
                                    geom_xyz, out, out_cstride, out_coff, ws, ws_bytes, c, &type, &launches))
        return rc;
    TT_REQUIRE(label && label_bytes > 0, "tt_lift_splat_fwd_plan: no room for the label");
    vp_label(c.launch, launches ? c.nlaunch : 0, 0, 0, type, c.arm == LS_STRIP_CELLS ? c.ws_bytes : 0, label, (size_t)label_bytes);
    return 0;
}
