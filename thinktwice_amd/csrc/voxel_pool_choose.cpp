// The dispatch of tt_voxel_pool_fwd / _fwd_ws / _fwd_planned and tt_lift_splat_fwd / _fwd_ws, stated once: from a call's sizes,
// pointer alignment and workspace to the arm, its template arguments, every launch (kernel, grid, block, dynamic LDS) and the byte
// offsets of the workspace.  Plain host arithmetic (no HIP call), so tt_voxel_pool_fwd_plan / tt_lift_splat_fwd_plan and the size
// queries answer without a device and the rules are testable on any machine (tests/test_voxel_pool_choice.py).  The launchers in
// voxel_pool.hip / lift_splat.hip only map a choice onto its kernels; a rule that is not here does not exist.
//
// The arm decides which sums are formed in which order, i.e. the bits of the output: no number here moves without a new record
// in tests/voxel_pool_choice_cases.json.
#include <stdint.h>

#include "voxel_pool_choose.h"

namespace tt {

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// every kernel but the scalar one moves rows as float4 pieces, at most 4 per lane
bool rows_ok(int C) { return C % 4 == 0 && C <= 1024; }

// ---- VP_TWO_PHASE: from 4 chunks on, cells that fit voxel_pool_p1_kernel's LDS tables
bool two_phase_ok(long long total, int C, int X, int Y) {
    return rows_ok(C) && (long long)X * Y <= kMaxCells && total >= 4 * kChunk;
}

// workspace: partial f32 [nchunks][kSlotBudget][C] | slot_table int [B][cells][cps]
void two_phase_layout(int B, int Np, int C, int X, int Y, VoxelPoolChoice* c) {
    c->cps = (Np + kChunk - 1) / kChunk;
    const long long nchunks = (long long)c->cps * B;
    const long long part = nchunks * kSlotBudget * C * 4;
    const long long tab = (long long)B * X * Y * c->cps * 4;
    c->partial = 0;
    c->slot_table = (size_t)((part + 255) / 256 * 256);
    c->ws_bytes = part + tab + 256;
}

// ---- VP_SORT: from 4 chunks on, cells that fit vp_cs_count_kernel's LDS, a sample's chunks in vp_cs_scan_kernel's registers,
// point indices in an int.  TT_VP_SORT=0 is the A/B knob (bench.py names the kernel by it).
bool sort_ok(long long total, int Np, int C, int X, int Y) {
    static const bool on = env_flag("TT_VP_SORT", true);
    const long long cps = ((long long)Np + kCsChunk - 1) / kCsChunk;
    return on && rows_ok(C) && (long long)X * Y <= kCsMaxCells && cps <= kCsMaxChunksPerSample && total >= 4 * kCsChunk &&
           total < (1ll << 31);
}

// workspace: keyrank u32 [total] | table int [B][cps][cells] | csr (one group per sample) | partial f32 [B][segcap][C]
void sort_layout(int B, int Np, int C, int cells, VoxelPoolChoice* c) {
    const size_t total = (size_t)B * Np;
    c->cps = (Np + kCsChunk - 1) / kCsChunk;
    size_t off = 0;
    c->keyrank = off; off += vp_align(4 * total);
    c->table = off; off += vp_align(4 * (size_t)B * c->cps * cells);
    c->csr = vp_csr_layout(off, B, Np, cells);
    c->partial = c->csr.end;
    c->ws_bytes = (long long)(c->partial + vp_align((size_t)c->csr.partial_bytes(C)));
}

}  // namespace

VpCsrLayout vp_csr_layout(size_t base, int ngroups, long long rows_per_group, long long cells_per_group) {
    VpCsrLayout L;
    L.ngroups = ngroups;
    L.cpg = cells_per_group;
    L.segcap = rows_per_group / kSeg + cells_per_group + 1;
    L.order = base;
    L.cell_start = L.order + vp_align(4 * (size_t)ngroups * rows_per_group);
    L.seg_off = L.cell_start + vp_align(4 * (size_t)ngroups * (cells_per_group + 1));
    L.end = L.seg_off + vp_align(4 * (size_t)ngroups * (cells_per_group + 1));
    return L;
}

void vp_planned_launches(int C, const VpCsrLayout& L, int* nv, int* rf, VpLaunch out[2]) {
    *nv = C <= 256 ? 1 : 4;
    *rf = C <= 256 ? 32 : 4;
    out[0] = {VPK_SEGMENTS, (unsigned)div_up(L.segcap * L.ngroups, 4), 256, 0};        // 4 waves per workgroup, a wave per segment
    out[1] = {VPK_CELLS, (unsigned)((int)L.cpg * L.ngroups), 256, 0};
}

long long voxel_pool_workspace_bytes(int B, int Np, int C, int X, int Y) {
    const long long total = (long long)B * Np;
    VoxelPoolChoice c{};
    long long need = 0;
    if (two_phase_ok(total, C, X, Y)) {
        two_phase_layout(B, Np, C, X, Y, &c);
        need = c.ws_bytes;
    }
    if (sort_ok(total, Np, C, X, Y)) {
        sort_layout(B, Np, C, X * Y, &c);
        if (c.ws_bytes > need) need = c.ws_bytes;
    }
    return need;
}

VoxelPoolChoice voxel_pool_choose(const VoxelPoolCall& k) {
    const long long total = (long long)k.B * k.Np;
    const int cells = k.X * k.Y;
    VoxelPoolChoice c{};
    if (k.ws_entry && k.ws && aligned16(k.feats) && aligned16(k.out)) {
        if (aligned16(k.ws) && k.lds_granted && sort_ok(total, k.Np, k.C, k.X, k.Y)) {
            sort_layout(k.B, k.Np, k.C, cells, &c);
            if (k.ws_bytes >= c.ws_bytes) {
                c.arm = VP_SORT;
                c.launch[0] = {VPK_CS_COUNT, (unsigned)(c.cps * k.B), kCsWaves * 64, vp_cs_count_lds(cells)};
                c.launch[1] = {VPK_CS_SCAN, (unsigned)k.B, 1024, 0};
                c.launch[2] = {VPK_CS_SCATTER, (unsigned)div_up(total, 256), 256, 0};
                vp_planned_launches(k.C, c.csr, &c.nv, &c.rf, c.launch + 3);
                c.nlaunch = 5;
                return c;
            }
            c = VoxelPoolChoice{};
        }
        if (two_phase_ok(total, k.C, k.X, k.Y)) {
            two_phase_layout(k.B, k.Np, k.C, k.X, k.Y, &c);
            if (k.ws_bytes >= c.ws_bytes) {
                c.arm = VP_TWO_PHASE;
                // 16 rows in flight per wave (0.302 / 0.287 / 0.277 ms per launch for 4 / 8 / 16, profiles/r02_voxel_pool_*)
                c.nv = k.C <= 256 ? 1 : 4;
                c.rf = k.C <= 256 ? 16 : 4;
                c.launch[0] = {VPK_P1, (unsigned)(c.cps * k.B), 512, 0};
                c.launch[1] = {VPK_P2, (unsigned)(k.B * cells), 64, 0};
                c.nlaunch = 2;
                return c;
            }
            c = VoxelPoolChoice{};
        }
    }
    if (rows_ok(k.C) && aligned16(k.feats)) {
        c.arm = VP_ROWS;
        c.nv = (k.C / 4 + 63) / 64;
        // a wave takes 64 points at a time; ~8 such chunks per wave keeps 2048+ blocks on big inputs and still fills the chip on
        // small ones
        long long blocks = ((total + 63) / 64 + 4 * 8 - 1) / (4 * 8);
        if (blocks < 1) blocks = 1;
        if (blocks > kNumCU * 16) blocks = kNumCU * 16;
        c.launch[0] = {VPK_ROWS, (unsigned)blocks, 256, 0};
    } else {
        c.arm = VP_SCALAR;
        c.launch[0] = {VPK_SCALAR, (unsigned)div_up(total * k.C, 256), 256, 0};
    }
    c.nlaunch = total == 0 ? 0 : 1;
    return c;
}

LiftSplatChoice lift_splat_choose(int B, int ncam, int D, int fH, int fW, int C, int X, int Y, bool has_ws) {
    LiftSplatChoice c{};
    if (!(fH * kStripW <= kMaxStripPix && D <= kMaxD && X * Y <= kMaxCells)) {
        c.arm = LS_PIXEL;
        c.launch[0] = {LSK_PIXEL, (unsigned)div_up((long long)B * ncam * fH * fW, 4), 256, 0};      // a wave per pixel
        c.nlaunch = 1;
        return c;
    }
    c.strips = div_up(fW, kStripW);
    const long long blocks = (long long)B * ncam * c.strips;
    // workspace: ws_rows f32 [blocks][kMaxSlots][C] | slot_of u8 [blocks][cells]
    c.slot_of = vp_align((size_t)blocks * kMaxSlots * C * sizeof(float));
    c.ws_bytes = (long long)c.slot_of + (long long)vp_align((size_t)blocks * X * Y);
    c.lds_opt_in = lift_splat_strip_lds(kMaxD, kStageC, kMaxCells);
    c.arm = has_ws ? LS_STRIP_CELLS : LS_STRIP_ATOMIC;
    c.launch[0] = {LSK_STRIP, (unsigned)(B * ncam * c.strips), 256, lift_splat_strip_lds(D, C, X * Y)};
    c.launch[1] = {LSK_CELLS, (unsigned)div_up((long long)B * X * Y, 4), 256, 0};                   // a wave per (sample, cell)
    c.nlaunch = has_ws ? 2 : 1;
    return c;
}

void vp_label(const VpLaunch* launch, int nlaunch, int nv, int rf, const char* type, long long ws_bytes, char* out, size_t bytes) {
    size_t n = 0;
    out[0] = 0;
    for (int i = 0; i < nlaunch && n < bytes; ++i) {
        char name[64];
        switch (launch[i].kernel) {
            case VPK_ROWS: snprintf(name, sizeof name, "voxel_pool_rows_kernel<%d>", nv); break;
            case VPK_SCALAR: snprintf(name, sizeof name, "voxel_pool_scalar_kernel"); break;
            case VPK_P1: snprintf(name, sizeof name, "voxel_pool_p1_kernel<%d, %d, true>", nv, rf); break;
            case VPK_P2: snprintf(name, sizeof name, "voxel_pool_p2_kernel"); break;
            case VPK_CS_COUNT: snprintf(name, sizeof name, "vp_cs_count_kernel"); break;
            case VPK_CS_SCAN: snprintf(name, sizeof name, "vp_cs_scan_kernel"); break;
            case VPK_CS_SCATTER: snprintf(name, sizeof name, "vp_cs_scatter_kernel"); break;
            case VPK_SEGMENTS: snprintf(name, sizeof name, "vp_planned_segments_kernel<%d, %d, true>", nv, rf); break;
            case VPK_CELLS: snprintf(name, sizeof name, "vp_planned_cells_kernel<%d>", nv); break;
            case LSK_PIXEL: snprintf(name, sizeof name, "lift_splat_kernel<%s>", type); break;
            case LSK_STRIP: snprintf(name, sizeof name, "lift_splat_strip_kernel<%s>", type); break;
            default: snprintf(name, sizeof name, "lift_splat_cells_kernel"); break;
        }
        const int w = snprintf(out + n, bytes - n, "%s%s grid %u block %d lds %zu", i ? " + " : "", name, launch[i].grid,
                               launch[i].block, launch[i].lds);
        if (w < 0) return;
        n += (size_t)w;
    }
    if (n < bytes) snprintf(out + n, bytes - n, "%sws %lld", n ? " " : "", ws_bytes);
}

}  // namespace tt
