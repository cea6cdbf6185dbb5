// Which kernel a convolution runs on: the arguments every conv kernel takes (ConvArgs), the choice tt_conv2d_fwd makes for a layer
// (ConvChoice) and the one host function that makes it (conv_choose, conv_choose.cpp).  Host-only: no kernel includes anything from
// here but ConvArgs, and the choice travels beside ConvArgs, never inside it.
#pragma once
#include <stddef.h>

#include "tt_common.h"

namespace tt {

struct ConvArgs {
    const void* in;
    const void* weight;
    void* out;
    const float* scale;
    const float* shift;
    const float* shift_n;
    const void* res1;
    const void* res2;
    const int* gather;   // GATHER mode: [M][KH*KW] input row per (output row, tap), -1 = none
    const int* m_dev;    // optional device-side row count (rows >= *m_dev are skipped)
    const int* row_perm;         // GATHER, optional: tile slot -> actual output row (rows sorted by tap mask)
    const unsigned* row_mask;    //   "       the sorted masks (bit t = tap t present), 0xFFFFFFFF beyond the live rows
    float* ws;           // split-K: f32 [M][Cout] partial-sum workspace (pre-zeroed), else null
    long long in_nstride, out_nstride;
    int N, H, W, Cin, in_cstride, in_coff;
    int Cout, KH, KW, stride, pad, dil;
    int OH, OW, out_cstride, out_coff;
    int pixel_shuffle2, shift_n_mod;
    int res1_cstride, res1_coff, res2_cstride, res2_coff;
    int act, out_dtype;
    int M, K;            // GEMM sizes
    int cin_fast;        // 1 if Cin % BK == 0 (tap uniform per K tile)
    int out_fast;        // 1 if plain [M][out_cstride] addressing
    int vec_epi;         // 1: LDS-staged epilogue with 16 B stores (channel counts / offsets aligned)
    int res_vec;         // 1: residual chunks are 8/16 B aligned (vector loads)
    int splits;          // split-K factor (gridDim.y)
    int tiles_n;
    int m_begin;         // first output row of this launch (tail-split launches of the LDS-DMA kernel), else 0
    int ws_slices;       // split-K: > 0 = every split stores into its own [M][Cout] slice of ws (ordered finalize)
    int flags;           // bit 4: non-temporal f32 output stores (every launch of the product); bit 5: the activations are pre-split bf16 (hi, lo) pairs (tt_conv_desc.in_pair);
                         // bit 6: write the output in that pair format (tt_conv_desc.out_pair); bit 7: res1 is f32 beside 16-bit operands (tt_conv_desc.res1_f32);
                         // bit 8: `in` is the [N][H/2][W/2][Cin] f32 map read through the bilinear x2 upsampling (tt_conv_desc.in_up2)
    int res1_up_h, res1_up_w;   // > 0: res1 is a [N][res1_up_h][res1_up_w][..] map read through nearest upsampling (tt_conv_desc)
    float* out2;         // optional second, f32, row-linear copy of the output (tt_conv_desc.out2): [M][out2_cstride] at out2_coff
    int out2_cstride, out2_coff;
    long long* trace;    // measurement aid (tt_conv_set_trace): 4 wall-clock stamps (10 ns ticks) per workgroup of the LDS-DMA kernel
                         // -- entry, first K tile landed, K loop done, epilogue done -- at trace[blockIdx.x * 4]; null in the product
};

// Kernel families, in the priority order of conv_choose.
enum ConvFamily {
    CONV_H2,        // conv_h2.hip        conv_h2_kernel<bn, waves_m, waves_n, SA, SB>        (stages = 10 SA + SB)
    CONV_H2_PIPE,   // conv_h2.hip        conv_h2_pipe_kernel
    CONV_SMALL,     // conv_small.hip     conv_small_kernel<T>
    CONV_SP_RUNS_L2,  // sp_conv_l2.hip   sp_conv_runs_l2_kernel<Cin>                          (bkb = 4 Cin: bytes of a weight row)
    CONV_SP_RUNS,   // sp_conv_runs.hip   sp_conv_runs_kernel<bn / (32 waves_n), waves_m, waves_n>
    CONV_X3_PIPE,   // conv_x3_pipe.hip   conv_x3_pipe_kernel<4, 1, bn, apair>
    CONV_X3_RUN3,   // conv_x3_pipe.hip   conv_x3_run3_kernel<bn, apair>
    CONV_X3_UP2,    // conv_x3_up2.hip    conv_x3_up2_kernel (input read through the bilinear x2 upsampling, tt_conv_desc.in_up2)
    CONV_X3_PATCH,  // conv_x3_patch.hip  conv_x3_patch_kernel<bn / 32> (pair-format 3 x 3 input staged as halo patches by LDS-DMA)
    CONV_X3_JOIN,   // conv_x3_join.hip   conv_x3_join_kernel<bkb / 4, bn, waves_m> (this 1 x 1 layer and the next one in one launch, tt_conv2d_fwd_next)
    CONV_GLDS,      // conv_igemm_glds.hip conv_igemm_glds_kernel<T, bn, waves_m, waves_n, bkb, stages, gather, x3, apair>
    CONV_IGEMM,     // conv_igemm.hip     conv_igemm_kernel<T, 128, bn, waves_m, waves_n, gather>
};

// Fewest allocated rows at which a 16- / 32-channel 3x3x3 rulebook conv takes the weight-resident kernel (conv_choose.cpp).
constexpr int kSpL2MinRows = 16384;

// Fewest output rows at which a pair-format 3 x 3 layer takes the halo-patch kernel (conv_choose.cpp, choose_x3_patch).
constexpr int kPatchMinRows = 16384;

// Joined stage (tt_conv2d_fwd_next, tt_conv_next; conv_choose.cpp, choose_join).  kJoinFloorRows: fewest output rows the kernel's contract takes
// (its pair-format output needs more than kSmallMaxRows).  kJoinMinRows: fewest rows at which every routed form beats its two
// launches.  The rule is stated here: a launch below it still runs the joined kernel, and its label -- tt_conv2d_plan_next's too -- ends
// in " below kJoinMinRows"; ops.join_ok routes by that label and keeps no number of its own.
// kSmallMaxRows: most output rows of the latency kernel (choose_small), hence the floor of pair format, in_up2 and the joined stage.
// Both numbers are the header's (include/thinktwice_hip.h), where the Python side reads them too.
constexpr int kSmallMaxRows = TT_CONV_SMALL_ROWS;
constexpr int kJoinFloorRows = kSmallMaxRows + 1;
constexpr int kJoinMinRows = TT_CONV_JOIN_MIN_ROWS;

// What conv2d_run knows about a layer beside its validated ConvArgs.
struct ConvFacts {
    int dtype;                  // operand storage type (TT_F32 / TT_BF16 / TT_F16)
    const void* weight_x3;      // tt_conv_desc.weight_x3 / weight_h2: tested for presence and 16-byte alignment, never read
    const void* weight_h2;
    bool out2, res1_up, res1_f32;
    bool assume_ws;             // tt_conv2d_splitk_slices: choose as if a split-K workspace of any size were given
    const ConvArgs* join;       // tt_conv2d_fwd_next: the joined stage as the validated layer it would be alone (null: none)
    const void* join_weight_x3; //   "   its weight_x3
};

struct ConvChoice {
    int family;                 // ConvFamily
    int bn;                     // tile width along Cout
    int waves_m, waves_n, bkb, stages;      // the tile variant: what the family's template takes (see ConvFamily)
    bool gather, x3, apair;     // x3: bf16x3 arithmetic, the launch reads weight_x3; apair: pre-split activations (in_pair)
    int main_rows;              // > 0: tail split -- the main launch covers this many 256-row tiles, the rest runs as 256 x 64 tiles
    int splits;                 // K ranges (gridDim.y), 1 = no split-K
    int slices;                 // split-K: workspace slices the ordered form writes (0: the atomic form); under assume_ws: slices to provide
    bool below_min;             // CONV_X3_JOIN: fewer than kJoinMinRows rows (the label says so)
};

// The kernel tt_conv2d_fwd runs a validated layer on.  0, or -1 with the error text set where the layer's operands name an arithmetic
// (weight_h2, pair format) whose kernel does not take the shape.  Touches no device.
int conv_choose(const ConvArgs& a, const ConvFacts& f, ConvChoice* c);
// The 256 x 64 tiles that follow the main launch of a tail split (c.main_rows > 0).
ConvChoice conv_tail_choice(const ConvChoice& c);
// What tt_conv_last_kernel reports after the launch of `c`: the kernel's name with its template arguments spelled as rocprofv3 prints them.
void conv_label(const ConvChoice& c, int dtype, char* out, size_t bytes);

}  // namespace tt
