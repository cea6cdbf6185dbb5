// Which kernels a voxel pool (voxel_pool.hip) or a fused lift-splat (lift_splat.hip) runs on: the constants host and kernels share,
// the workspace / plan layouts, and the choice the launchers make for a call (voxel_pool_choose.cpp).  The .hip files include this
// for the constants and the LDS-size helpers; everything else is host-only.
//
// 16-byte alignment, per arm.  "falls" = a pointer that is not aligned sends the call to the next arm down, "refused" = an error,
// "-" = not looked at.  The rules are the ones each arm grew up with and are kept as they are:
//
//   arm                                   input_features   output_features   workspace
//   SORT       (tt_voxel_pool_fwd_ws)     falls            falls             falls
//   TWO_PHASE  (tt_voxel_pool_fwd_ws)     falls            falls             -          (its float4 partial rows are plain global stores)
//   ROWS       (both entries)             falls            -                 -          (the output only takes scalar atomics)
//   SCALAR     (both entries)             -                -                 -
//   static plan (tt_voxel_pool_fwd_planned) refused        refused           -
//   lift-splat (every arm)                -                -                 -          (the workspace form refuses out_cstride / out_coff
//                                                                                        that are no multiple of 4 floats instead)
#pragma once
#include <stddef.h>

#include "tt_common.h"

namespace tt {

// ---- two-phase pool (voxel_pool_p1_kernel / _p2_kernel)
constexpr int kChunk = 2048;             // consecutive points of one sample per workgroup
constexpr int kMaxCells = 2048;          // BEV cells of its LDS tables (and of the lift-splat strip kernel's)
constexpr int kSlotBudget = 64;          // workspace rows per chunk (Lift-Splat chunks touch <= ~40 cells); the rest go to atomics
// ---- planned streaming kernels (vp_planned_*): a cell's run of rows is cut into segments of kSeg
constexpr int kSeg = 64;
// ---- per-launch counting sort (vp_cs_*)
constexpr int kCsChunk = 8192;
constexpr int kCsWaves = 16;
constexpr int kCsMaxCells = 1024;
constexpr int kCsMaxChunksPerSample = 64;
// ---- lift-splat strip kernel
constexpr int kStripW = 2;
constexpr int kMaxStripPix = 64;         // fH * kStripW <= 64
constexpr int kMaxSlots = 64;
constexpr int kMaxD = 128;
constexpr int kStageC = 128;
constexpr int kWS = kMaxSlots + 4;       // W row stride: 16 B rows, = 4 mod 8 words

// dynamic LDS of vp_cs_count_kernel: per wave and (64-padded) cell a u16 running count and a 64-bit lane mask
inline size_t vp_cs_count_lds(int cells) {
    return (size_t)kCsWaves * ((cells + 63) & ~63) * (sizeof(unsigned short) + sizeof(unsigned long long));
}

// dynamic LDS of lift_splat_strip_kernel: W f32 [kMaxStripPix][kWS] | table int [cells] | slot_cell int [kMaxSlots] | a region that
// holds { prob f32 [kMaxStripPix][PD], tag short [D][npx] } until W is built and the staged context rows
// f32 [kMaxStripPix][min(C, kStageC)] afterwards  (50 KiB at the thinktwice.py shapes: three workgroups per CU)
__host__ __device__ inline int lift_splat_prob_stride(int D) {      // 16 B rows, = 4 mod 8 words: 16 rows on 16 bank quads
    int pd = (D + 3) & ~3;
    if ((pd & 4) == 0) pd += 4;
    return pd;
}
__host__ __device__ inline int lift_splat_table_words(int cells) { return (cells + kMaxSlots + 3) & ~3; }
inline size_t lift_splat_strip_lds(int D, int C, int cells) {
    const size_t a = (size_t)kMaxStripPix * lift_splat_prob_stride(D) * 4 + (size_t)kMaxStripPix * D * 2;
    const size_t c = (size_t)kMaxStripPix * (C < kStageC ? C : kStageC) * 4;
    const size_t b = (size_t)kWS * kMaxStripPix * 4 + (size_t)lift_splat_table_words(cells) * 4 + (a > c ? a : c);
    return (b + 15) / 16 * 16;
}

inline size_t vp_align(size_t v) { return (v + 255) / 256 * 256; }

// ---- launches ------------------------------------------------------------------------------------------------
enum VpKernel {
    VPK_ROWS,           // voxel_pool_rows_kernel<NV>
    VPK_SCALAR,         // voxel_pool_scalar_kernel
    VPK_P1,             // voxel_pool_p1_kernel<NV, RF, true>
    VPK_P2,             // voxel_pool_p2_kernel
    VPK_CS_COUNT,       // vp_cs_count_kernel
    VPK_CS_SCAN,        // vp_cs_scan_kernel
    VPK_CS_SCATTER,     // vp_cs_scatter_kernel
    VPK_SEGMENTS,       // vp_planned_segments_kernel<NV, RF, true>
    VPK_CELLS,          // vp_planned_cells_kernel<NV>
    LSK_PIXEL,          // lift_splat_kernel<T>
    LSK_STRIP,          // lift_splat_strip_kernel<T>
    LSK_CELLS,          // lift_splat_cells_kernel
};

struct VpLaunch {
    int kernel;         // VpKernel
    unsigned grid;      // workgroups
    int block;          // threads per workgroup
    size_t lds;         // dynamic LDS bytes
};

// ---- CSR plan: `order` (point indices grouped by cell) | cell_start | seg_off, each vp_align'ed, over `ngroups` groups of `cpg`
// cells (see vp_planned_segments_kernel).  The static plan is one group of batch x cells keys over all the points, the per-launch
// sort one group per sample.  segcap: a group's segments, <= floor(rows / kSeg) + one ragged one per cell.
struct VpCsrLayout {
    int ngroups;
    long long cpg, segcap;
    size_t order, cell_start, seg_off, end;     // byte offsets; `end` = first byte after seg_off
    // one partial row per segment (upper bound): the workspace of the two streaming kernels
    long long partial_bytes(int C) const { return ngroups * segcap * (long long)C * 4; }
};
VpCsrLayout vp_csr_layout(size_t base, int ngroups, long long rows_per_group, long long cells_per_group);
inline VpCsrLayout vp_static_plan_layout(int B, int Np, int X, int Y) {
    return vp_csr_layout(0, 1, (long long)B * Np, (long long)B * X * Y);
}
// The two streaming kernels over a CSR plan: <1, 32, true> + cells<1> up to 256 channels, else <4, 4, true> + cells<4>
// (32 rows in flight per wave, non-temporal row loads: measured against 8 / 16 rows and plain loads, profiles/r02_voxel_pool_*).
void vp_planned_launches(int C, const VpCsrLayout& L, int* nv, int* rf, VpLaunch out[2]);

// ---- the op-boundary pool -----------------------------------------------------------------------------------
enum VoxelPoolArm {
    VP_ROWS,            // single-pass atomic kernel, one wave per point row
    VP_SCALAR,          // single-pass atomic kernel, one thread per (point, channel): any C, any alignment
    VP_TWO_PHASE,       // "v2": per-chunk cell sums in LDS order, then an ordered per-cell gather
    VP_SORT,            // "v3": per-launch counting sort, then the planned streaming kernels
};

struct VoxelPoolCall {
    int B, Np, C, X, Y;
    const void* geom;               // the pointers are tested for null-ness (launcher) and 16-byte alignment (chooser), never read
    const void* feats;
    const void* out;
    const void* ws;
    long long ws_bytes;
    bool ws_entry;                  // tt_voxel_pool_fwd_ws (false: tt_voxel_pool_fwd, which has no workspace)
    bool lds_granted;               // the device lets vp_cs_count_kernel take its > 64 KiB of dynamic LDS
};

struct VoxelPoolChoice {
    int arm;                        // VoxelPoolArm
    int nv, rf;                     // template arguments: float4 chunks per lane, point rows in flight per wave
    int nlaunch;
    VpLaunch launch[5];
    long long ws_bytes;             // workspace bytes the arm needs (atomic arms: 0)
    int cps;                        // chunks per sample (of kChunk / kCsChunk points)
    // workspace layout, byte offsets.  VP_TWO_PHASE: partial | slot_table.  VP_SORT: keyrank | table | csr | partial.
    size_t partial, slot_table, keyrank, table;
    VpCsrLayout csr;
};

VoxelPoolChoice voxel_pool_choose(const VoxelPoolCall& c);
// tt_voxel_pool_workspace_bytes: the most any arm would take for these sizes (0: only the atomic kernels take them)
long long voxel_pool_workspace_bytes(int B, int Np, int C, int X, int Y);

// ---- the fused lift-splat -----------------------------------------------------------------------------------
enum LiftSplatArm {
    LS_PIXEL,           // one wave per pixel, atomics
    LS_STRIP_ATOMIC,    // one workgroup per image strip, one atomic row per (strip, cell)
    LS_STRIP_CELLS,     // strip kernel -> partial rows in the workspace -> lift_splat_cells_kernel: no atomics
};

struct LiftSplatChoice {
    int arm;            // LiftSplatArm
    int nlaunch;
    VpLaunch launch[2];
    size_t lds_opt_in;  // LS_STRIP_*: the largest request the strip kernel's limits allow (asked for once per device)
    long long ws_bytes; // what the workspace form of this shape takes: ws_rows | slot_of (0: the shape has no workspace form)
    size_t slot_of;     // byte offset of slot_of (ws_rows is at 0)
    int strips;         // image strips per camera
};
LiftSplatChoice lift_splat_choose(int B, int ncam, int D, int fH, int fW, int C, int X, int Y, bool has_ws);

// Launches joined by " + ", each "<kernel with its template arguments as rocprofv3 prints it> grid <x> block <n> lds <dynamic
// bytes>", then " ws <bytes the arm needs>".  `type`: the storage type of a lift-splat kernel ("float", ...), else null.
void vp_label(const VpLaunch* launch, int nlaunch, int nv, int rf, const char* type, long long ws_bytes, char* out, size_t bytes);

}  // namespace tt
