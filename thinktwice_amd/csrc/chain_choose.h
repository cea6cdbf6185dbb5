// Which form a decoder row chain (dec_chain.hip) runs in, and where its intermediates go: the constants and the stage struct host
// and kernels share, the argument checks of both entries, and the choice (chain_choose.cpp).  dec_chain.hip includes this for the
// constants and ChainStage; everything else is host-only.
#pragma once
#include <stddef.h>

#include "tt_common.h"

namespace tt {

constexpr int kChainMaxStages = 12;
constexpr int kChainWaves = 8;
constexpr int kChainNBW = 2;      // accumulator blocks per wave per pass

struct ChainStage {
    const void* w;        // fragment-major pair-format weights of the [N padded to 32][Kp] matrix
    const float* bias;    // [N] or null
    const float* res;     // optional residual rows (global f32): v += res[m * res_stride + res_coff + n]
    const float* side;    // optional extra input columns (global f32 [R][side_stride]): v += sum_j side[m][j] * side_w[n][j]
    const float* side_w;  // [N][side_k] f32
    float* out;           // optional global f32 output: out[m * out_stride + out_coff + n]
    int K, Kp, N, act;
    int in_sel;           // -1: the chain input x; s >= 0: the LDS output of stage s
    int res_stride, res_coff, side_stride, side_k;
    int out_stride, out_coff;
    int lds_off;          // byte offset of this stage's LDS output (pair format); -1: not kept
    int lds_stride;       // bytes per row of that buffer (Kp_next * 4 + 16: an odd number of 16 B slots, conflict-free)
};

enum ChainForce {
    CHAIN_AUTO,           // by the rows (ops.mlp_chain without wide=)
    CHAIN_ROWS,           // tt_mlp_chain, n_split as given
    CHAIN_WIDE,           // tt_mlp_chain_wide, `groups` a hint that is clamped to what can be co-resident (ops.mlp_chain wide=True)
    CHAIN_WIDE_AS_GIVEN,  // tt_mlp_chain_wide with exactly `groups` column groups, refused beyond the bounds (the launch entry)
};

struct ChainChoice {
    bool wide;
    int rb;                                 // 32-row blocks per workgroup (wide: 1, 2 or 4)
    long long row_groups;                   // gridDim.x: workgroups along the rows
    int n_groups, n_split;                  // gridDim.y of the wide / the row form (the other is 1)
    int nbw;                                // row form: 32-column blocks per wave per pass
    // row form: LDS placement of every stage output a later stage reads (lds_off -1: not kept)
    int lds_off[kChainMaxStages], lds_stride[kChainMaxStages];
    size_t lds_total;                       // dynamic LDS of the launch
    // wide form: workspace placement of the same outputs (keep_off -1: not kept; keep_stride: 16-column steps per row block),
    // and where the workgroups of a row block meet
    long long keep_off[kChainMaxStages];
    int keep_stride[kChainMaxStages], sync_before[kChainMaxStages], nsync;
    long long workspace_bytes;
};

// The argument and stage checks of both entries (-1 and the error text under the entry's name `who`).  x is only tested for
// null-ness and alignment.
int chain_validate(const char* who, const void* x, long long R, int x_stride, int nstages, const tt_chain_stage* st);
// The header's stage -> the kernels' (lds_off = -1: the launcher fills the placement in from the choice)
ChainStage chain_stage(const tt_chain_stage& d);

// Whether a chain of R rows runs the wide form (needs nothing else: callers order their stages by it).
bool chain_is_wide(long long R, int force, int max_workgroups);
// The whole choice, 0 or -1 with the error text the launch entry gives.  Stages must have passed chain_validate.  max_workgroups:
// what tt_mlp_chain_wide_max_workgroups() answers for the device; < 0 = not known yet, only with CHAIN_WIDE_AS_GIVEN, whose
// caller then applies chain_wide_fits itself once it has the device.
int chain_choose(long long R, int nstages, const tt_chain_stage* st, int n_split, int groups_hint, int force, int max_workgroups,
                 ChainChoice* out);
int chain_wide_fits(const ChainChoice& c, int max_workgroups);

}  // namespace tt
