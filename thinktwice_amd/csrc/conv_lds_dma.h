// The LDS-DMA conv pipeline: the pieces every kernel of the family shares, each defined once.
//
// conv_igemm_glds.hip, conv_x3_pipe.hip, conv_h2.hip and sp_conv_runs.hip (and the staged weight gradient of conv_bwd.hip) move
// their operands the same way: 1 KiB `global_load_lds_dwordx4` pieces into unpadded LDS rows, an XOR swizzle applied to the DMA
// SOURCE address, one precomputed pointer + one tap-validity mask per activation slot, a zero page for padding, channel-chunk-outer /
// tap-inner K order, XCD-aware tile order, counted `s_waitcnt vmcnt(N)` + raw `s_barrier`, inline-asm fragment reads.  A kernel
// derived from the pipeline consists of its schedule; the layout it schedules is here, parametrised by row width, element type,
// wave count and K tile -- never by which kernel calls.
#pragma once
#include "conv_common.h"

namespace tt {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Fragment reads are INLINE ASM: hipcc treats every ds_read of the dynamic LDS array as aliasing the in-flight LDS-DMA and would
// insert `s_waitcnt vmcnt(0)` in front of it (draining the tiles of prefetch every iteration); asm reads are invisible to that
// pass, ordering is by the counted vmcnt + barrier of the kernel's loop (MI355X_MICROARCH.md "Two waves per SIMD" item 7).
__device__ __forceinline__ u32x4 lds_read(unsigned addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
// ... with a compile-time byte offset
template <int OFF>
__device__ __forceinline__ u32x4 lds_read_at(unsigned addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}

// The counted wait: at most N of this wave's loads (LDS-DMA pieces, in issue order) are still outstanding.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit count");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// One 1 KiB DMA piece: 64 lanes x 16 B from per-lane global addresses to the wave-uniform LDS address `lds` (it goes to M0: keep
// it in scalar registers instead of deriving it from threadIdx through a VALU add + v_readfirstlane per load) + lane * 16.
template <typename E>
__device__ __forceinline__ void dma_piece(const E* src, unsigned lds) {
    __builtin_amdgcn_global_load_lds(src, (lds_ptr_t)(uintptr_t)lds, 16, 0, 0);
}

// LDS rows are unpadded (the DMA writes wave-uniform base + lane * 16); bank conflicts are removed by storing 16 B chunk c of row r
// at chunk slot c ^ swz(r): f(r) = (r >> 2) & 3 for 64 B rows, (r >> 1) & 7 for 128 B rows, r & 15 for 256 B rows -- every 16-lane
// group of ds_read_b128 then touches 16 distinct slots of the 256 B bank row.
template <int ROWB>
__device__ __forceinline__ int swz(int row) {
    static_assert(ROWB == 64 || ROWB == 128 || ROWB == 256, "64 B, 128 B or 256 B rows");
    return ROWB == 64 ? (row >> 2) & 3 : ROWB == 128 ? (row >> 1) & 7 : row & 15;
}

// Byte offset of (row, 16 B chunk) inside a stage of ROWB-byte rows: what a kernel's fragment-offset table holds for every K step
// (registers instead of 3 VALU per read per step; ds_read_b128 per lane: row = lane & 31 of the 32-row block, K half = lane >> 5).
// Flipping bit 4 / bit 5 of the result addresses chunk ^ 1 / chunk ^ 2 of the same row (the swizzle being an XOR): the second half
// of an f32 fragment, the lo half of a pair-format one.  (The loops that fill a table stay in the kernels: filled through a
// reference by a shared function, the hand-pipelined loops came out of the register allocator differently.)
template <int ROWB>
__device__ __forceinline__ unsigned frag_off(int row, unsigned chunk) {
    return row * ROWB + ((chunk ^ swz<ROWB>(row)) << 4);
}

// XCD-aware tile order (bijective for any grid size): hardware places block b on XCD b % 8; the tiles are dealt so that consecutive
// ones -- which share an activation row block / their halo rows -- run on ONE XCD (its L2).  `nblk` = the tiles that have work (the
// sparse kernels pass their live count: dealt over the allocation, whole XCDs end up holding nothing but dead tiles); the caller
// has returned for blockIdx.x >= nblk.
__device__ __forceinline__ int xcd_tile(int nblk) {
    const int b = blockIdx.x, xcd = b & 7, q = nblk >> 3, r = nblk & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// ---- dense activation slots.  Everything about a slot that does not change over the K loop is folded into ONE pointer (the
// chunk's address for tap (0,0), channel 0, possibly outside the image) and ONE bitmask (bit t = tap t of this row is inside the
// image; KH*KW <= 31 or 32, dispatchers -- the hand-pipelined kernels rely on bit 31 never being set).  Per K tile a slot then costs
// a 64-bit add of a wave-uniform tap offset, a bit test and a select -- the per-tile im2col arithmetic was ~2/3 of the kernel's VALU
// issue (SQ_INSTS_VALU 5.6 per MFMA, profiles/r01_conv_sq_counters.txt).
struct RowWindow {
    int n, h0, w0;      // image, input coordinate of tap (0, 0)
};
__device__ __forceinline__ RowWindow row_window(const ConvArgs& p, int m) {
    const int n = m / (p.OH * p.OW);
    const int r = m - n * (p.OH * p.OW);
    const int oh = r / p.OW, ow = r - oh * p.OW;
    return RowWindow{n, oh * p.stride - p.pad, ow * p.stride - p.pad};
}
__device__ __forceinline__ unsigned tap_mask(const ConvArgs& p, int h0, int w0) {
    unsigned mk = 0;
    int tbit = 0;
    for (int kh = 0; kh < p.KH; ++kh) {
        const int ih = h0 + kh * p.dil;
        for (int kw = 0; kw < p.KW; ++kw, ++tbit) {
            const int iw = w0 + kw * p.dil;
            if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) mk |= 1u << tbit;
        }
    }
    return mk;
}
// Slot of 16 B chunk g of the [rows][ROWB] activation tile whose first row is output row m0 (g = piece * 64 + lane).  Rows beyond
// Mlim get an empty mask: every tap reads the zero page.
template <int ROWB, typename E>
__device__ __forceinline__ void dense_slot(const ConvArgs& p, const E* in, int g, int m0, int Mlim, const E*& ptr, unsigned& mask) {
    constexpr int CPR = ROWB / 16, VEC = 16 / (int)sizeof(E);
    const int row = g / CPR, pos = g % CPR;
    const int c = (pos ^ swz<ROWB>(row)) * VEC;          // element offset of the global chunk inside the K tile
    const int m = m0 + row;
    const bool ok = m < Mlim;
    const RowWindow w = row_window(p, ok ? m : 0);
    ptr = in + (long long)w.n * p.in_nstride + p.in_coff + ((long long)w.h0 * p.W + w.w0) * p.in_cstride + c;
    mask = ok ? tap_mask(p, w.h0, w.w0) : 0u;
}

// ---- K walk of the compiler-scheduled tiles.  K order: channel chunk OUTER, filter tap INNER (Cin % BK == 0: one tap per K tile).
// The KH*KW taps of one BK-channel chunk re-read the same (tile + halo) pixels back to back, so the re-reads hit the XCD's 4 MiB L2
// (64 resident tiles x ~700 px x 128 B lines = ~2 MiB with the XCD-contiguous tile order).  With taps outer the reuse distance was
// the whole channel extent (~8 MiB per XCD for Cin = 256) and 8 of 9 reads fell through to the Infinity Cache.  Summation order
// differs from (tap, channel) only in f32 rounding.
// The activation and the weight stream walk the same sequence; with an asymmetric ring the activation walker runs one tile ahead
// of the weight walker, so each keeps its own position.
struct KWalk {
    int kh, kw, ci;     // running (kh, kw, ci) of the next tile to issue
};
template <int BK>
__device__ __forceinline__ void advance(KWalk& w, const ConvArgs& p) {
    if (++w.kw == p.KW) {
        w.kw = 0;
        if (++w.kh == p.KH) {
            w.kh = 0;
            w.ci += BK;
        }
    }
}
// The DMA of one tile, one piece at a time ("spread"): when all eight waves issue their pieces of the next tile together right
// after the barrier, the CU's one texture path (64 B/clk: 16 clk per 1 KiB piece) queues 64 pieces and every wave sits ~1000 cycles
// in instruction issue before its first MFMA.  Spread over the sub-steps of the tile -- one piece group behind each group of MFMAs
// -- the queue never fills.  `begin` takes the walker's position (wave-uniform, SALU) and advances it; `emit` issues one slot.
struct DmaCtx {
    unsigned st;        // LDS address of the stage
    int tap;            // activations: bit of the slot masks
    long long off;      // element offset from the slot pointers
    bool on;            // false: past the last tile, nothing is issued
};
template <int BK>
__device__ __forceinline__ DmaCtx dma_begin_a(const ConvArgs& p, KWalk& w, unsigned st, bool on) {
    DmaCtx c{0u, 0, 0, on};
    if (!on) return c;
    c.st = st;
    c.tap = w.kh * p.KW + w.kw;
    c.off = ((long long)(w.kh * p.dil) * p.W + w.kw * p.dil) * p.in_cstride + w.ci;
    advance<BK>(w, p);
    return c;
}
// WROW: elements of a weight row per element of K (1; 2 for the (hi, lo) f16 pair rows of the h2 kernels)
template <int BK, int WROW>
__device__ __forceinline__ DmaCtx dma_begin_b(const ConvArgs& p, KWalk& w, unsigned st, bool on) {
    DmaCtx c{0u, 0, 0, on};
    if (!on) return c;
    c.st = st;
    c.off = (long long)WROW * ((long long)(w.kh * p.KW + w.kw) * p.Cin + w.ci);
    advance<BK>(w, p);
    return c;
}
template <typename E>
__device__ __forceinline__ void dma_emit_a(const DmaCtx& c, const E* ptr, unsigned mask, const E* zp, int piece) {
    dma_piece(((mask >> c.tap) & 1u) ? ptr + c.off : zp, c.st + (unsigned)piece * 1024u);
}
template <typename E>
__device__ __forceinline__ void dma_emit_b(const DmaCtx& c, const E* ptr, bool ok, const E* zp, int piece) {
    dma_piece(ok ? ptr + c.off : zp, c.st + (unsigned)piece * 1024u);
}

// ---- host side: the tail of every launcher of the family.  Zero page and LDS opt-in for the current device (`lds_max` = the
// largest request any launch of `kern` makes, so the opt-in happens once), the ConvArgs bookkeeping and the launch of kern(a, zero
// page, tiles_m, tiles_n, extra...).  Returns 1, or -1 with the error text set (naming `who` and the device); never another kernel.
template <typename K, typename... Extra>
static int launch_lds_dma(K kern, dim3 grid, dim3 block, size_t lds, size_t lds_max, const char* who, ConvArgs& a, hipStream_t st,
                          int tiles_m, int tiles_n, int splits, Extra... extra) {
    const void* zp = zero_page(who);
    if (!zp || lds_opt_in(reinterpret_cast<const void*>(kern), lds_max, who)) return -1;
    a.tiles_n = tiles_n;
    a.splits = splits;
    if (splits <= 1) a.ws = nullptr;       // split-K: a.ws / a.ws_slices are the caller's
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, zp, tiles_m, tiles_n, extra...);
    return 1;
}

}  // namespace tt
