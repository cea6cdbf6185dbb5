// The dispatch of tt_conv2d_fwd, stated once: from a validated layer to the kernel family, tile variant and split it runs with.
// Plain host arithmetic (no HIP call), so tt_conv2d_plan / tt_conv2d_splitk_slices answer without a device and the rules are
// testable on any machine (tests/test_conv_choice.py).  The launchers in the kernel files only map a choice onto its template
// instantiation; a rule that is not here does not exist.
#include <stdint.h>

#include "conv_choose.h"

namespace tt {
namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

void set_tile(ConvChoice* c, int family, int bn, int waves_m, int waves_n, int bkb, int stages) {
    c->family = family;
    c->bn = bn;
    c->waves_m = waves_m;
    c->waves_n = waves_n;
    c->bkb = bkb;
    c->stages = stages;
}

// ---- "h2" arithmetic (conv_h2.hip): dense, Cin % 64 == 0, KH*KW <= 31
bool choose_h2(const ConvArgs& a, ConvChoice* c) {
    if (a.gather || a.m_dev || a.ws || a.pixel_shuffle2 || a.Cin % 64 != 0 || a.KH * a.KW > 31 || a.K < 64) return false;
    // long K, 128-wide column tiles: the hand-pipelined one-wave-per-SIMD kernel.  TT_H2_PIPE=0 (test hook: tests/test_conv.py
    // compares the two kernels bit for bit): the compiler-scheduled kernel everywhere
    static const bool pipe = env_flag("TT_H2_PIPE", true);
    if (pipe && a.Cout % 128 == 0 && a.K >= 1152) set_tile(c, CONV_H2_PIPE, 128, 4, 1, 128, 32);
    // 128-wide: 8 waves of 64 x 64 on a 3 + 2 ring (160 KiB); measured against four waves of 128 x 64 (+15 %) and a 2 + 2 ring (-0.5 %:
    // kept out, one variant less): profiles/r06_h2_microbench.txt.  64-wide: 8 waves of 32 x 64, 3 + 3 ring (four waves: +20 %)
    else if (a.Cout > 64) set_tile(c, CONV_H2, 128, 4, 2, 128, 32);
    else set_tile(c, CONV_H2, 64, 8, 1, 128, 33);
    return true;
}

// ---- latency-bound small-M variant (conv_small.hip: 32 x 32 tile, intra-block split-K)
bool choose_small(const ConvArgs& a, ConvChoice* c) {
    if (a.gather || a.m_dev || a.M > kSmallMaxRows) return false;
    if ((long long)div_up(a.M, 32) * div_up(a.Cout, 32) > 4096) return false;
    set_tile(c, CONV_SMALL, 32, 1, 1, 32, 1);
    return true;
}

// Tail split of a 256x256-tile launch.  With T tiles on 256 CUs (one workgroup per CU: 128 KiB of LDS) the launch
// takes ceil(T / 256) rounds; when the last round is less than a quarter full (the 512 -> 512 DepthNet layers: 784
// tiles = 3 rounds + 16 tiles, i.e. 23 % of the launch spent on 2 % of the work) the row tiles of that remainder are
// peeled off into a second launch of 256x64 tiles (4x as many, 1/4 the work each) that fills the chip.
// Returns the number of row tiles the MAIN launch should cover (0: no split).
int tail_split_rows(const ConvArgs& a) {
    if (a.Cout % 256 != 0) return 0;
    const int tiles_m = div_up(a.M, 256), tiles_n = a.Cout / 256;
    const long long T = (long long)tiles_m * tiles_n;
    const int rounds = (int)((T + kNumCU - 1) / kNumCU);
    const int last = (int)(T - (long long)kNumCU * (rounds - 1));
    if (rounds < 2 || rounds > 8 || last > kNumCU / 4) return 0;
    const int peel = div_up(last, tiles_n);            // row tiles moved to the tail launch
    return peel < tiles_m ? tiles_m - peel : 0;
}

// Split-K form of the 64-wide bf16x3 tile: few rows, long K (batch-1 ticks: ResNet layer 4 at M = 3,136, K = 2048 / 4608 --
// 13 row tiles are a twentieth of the chip, so those layers ran the exact-f32 register-staged kernel with a K split, 2.0 ms per
// tick).  Column blocks of 64 give tiles_m x Cout / 64 workgroups; the K tiles are dealt over up to 16 ranges of >= 8 tiles until
// ~512 workgroups (two per CU) are in flight.  The workspace must hold one [M][Cout] slice per non-empty K range.
bool choose_x3_splitk(const ConvArgs& a, bool assume_ws, ConvChoice* c) {
    if (a.gather || a.m_dev || a.M < 512 || a.M > 8192 || a.Cout < 64 || a.KH * a.KW > 32) return false;
    if (a.Cin % 32 != 0 || a.K < 1024 || a.pixel_shuffle2) return false;
    const int tiles = div_up(a.M, 256) * div_up(a.Cout, 64);
    const int nk = a.K / 32;
    if (tiles >= 256) return false;
    int sp = 512 / tiles;
    if (sp > nk / 8) sp = nk / 8;
    if (sp > 16) sp = 16;
    if (sp < 2) return false;
    const int slices = div_up(nk, div_up(nk, sp));
    if (slices < 2 || (!assume_ws && a.ws_slices < slices)) return false;
    set_tile(c, CONV_GLDS, 64, 8, 1, 128, 2);
    c->x3 = true;
    c->splits = sp;
    c->slices = slices;
    return true;
}

// ---- weight-resident sparse 3x3x3 conv (sp_conv_l2.hip): bf16x3 gathered conv with 27 taps, Cin 16 / 32, Cout 16 / 32 / 64, any
// rulebook and stride.  A persistent launch loads 27 x 32 x Cin x 4 B of weights (110 KB at Cin = 32) into every CU's LDS once, which
// only pays over many 32-row groups: from kSpL2MinRows allocated rows on (at most 65,536: the batch-1 allocation of the 16-channel
// level must take this kernel).  Below it the run-staged kernel and the gathered LDS-DMA tiles keep their layers.
// Measured crossover (profiles/sp_conv_l2.txt; us per launch, old -> new): 32 -> 32 SubM at 17 K / 64 K / 260 K rows 26.9 -> 18.8,
// 30.0 -> 21.8, 99.3 -> 68.3; 16 -> 16 at 64 K rows 22.9 -> 11.8.  The new kernel already wins at the lowest size tried, so the
// threshold sits at the 16,384 rows it was first set to.  The routed shapes of the B = 8 forward, serialised (ms over the calls,
// old -> new): 32 -> 32 SubM x 4 2.43 -> 1.65; 32 -> 64 stride 2 0.80 -> 0.68; 16 -> 16 SubM x 4 (M = 523 K) 0.55 -> 0.31;
// 16 -> 32 stride 2 0.37 -> 0.22.  Every shape wins, so none is sent back to its old kernel.
bool choose_sp_runs_l2(const ConvArgs& a, ConvChoice* c) {
    if (!a.gather || a.row_perm || a.KH != 1 || a.KW != 27 || a.pixel_shuffle2 || a.M < kSpL2MinRows) return false;
    if ((a.Cin != 16 && a.Cin != 32) || (a.Cout != 16 && a.Cout != 32 && a.Cout != 64)) return false;
    // 16 B loads of the neighbour rows, the vector epilogue's f32 stores
    if ((a.in_cstride & 3) || (a.in_coff & 3) || !aligned16(a.in) || !a.vec_epi || a.out_dtype != TT_F32) return false;
    set_tile(c, CONV_SP_RUNS_L2, 32, 8, 1, a.Cin * 4, 1);
    c->gather = c->x3 = true;
    return true;
}

// ---- run-staged sparse 3x3x3 conv (sp_conv_runs.hip): bf16x3 gathered conv with 27 taps in [kz][ky][kx] order, Cin a multiple
// of 32, Cout 32 / 64 / 128
bool choose_sp_runs(const ConvArgs& a, ConvChoice* c) {
    if (!a.gather || a.row_perm || a.KH != 1 || a.KW != 27) return false;
    // strided sparse convs (the caller states stride 2): the inputs of a (dz, dy) group sit on every other line, the
    // contiguous range is ~4x the tile and is walked in mostly-empty chunks (measured 0.74 -> 4.1 ms): gather kernel
    if (a.stride != 1) return false;
    if (a.Cin % 32 != 0 || a.Cin > 128 || a.M < 2048 || a.pixel_shuffle2) return false;
    if ((a.in_cstride & 3) || (a.in_coff & 3)) return false;
    if (a.Cout == 32) set_tile(c, CONV_SP_RUNS, 32, 8, 1, 128, 2);            // <NCB, WR, WC> = <1, 8, 1>
    else if (a.Cout == 64) set_tile(c, CONV_SP_RUNS, 64, 8, 1, 128, 2);       //                 <2, 8, 1>
    else if (a.Cout == 128) set_tile(c, CONV_SP_RUNS, 128, 4, 2, 128, 2);     //                 <2, 4, 2>
    else return false;
    c->gather = c->x3 = true;
    return true;
}

// the hand-pipelined bf16x3 tiles (conv_x3_pipe.hip) take: dense, Cout a multiple of the tile width, at most 31 taps
bool x3_pipe_ok(const ConvArgs& a, int bn) {
    return !(a.gather || a.m_dev || (bn != 256 && bn != 128) || a.Cout % bn != 0 || a.Cin % 32 != 0 || a.KH * a.KW > 31 || a.K < 64);
}

// ---- pair-format 3 x 3 "same" convolution on halo patches (conv_x3_patch.hip): the kernel's whole contract.  Anything outside it
// keeps its per-tap tile: a routing decision, not an error.  TT_X3_PATCH=0 (the A/B knob): the per-tap tiles everywhere.
// Threshold kPatchMinRows = 16,384 rows, for both column-block forms.  Measured crossover (profiles/conv_patch.txt; us per launch,
// serialised, minimum of 10, per-tap tile -> patch kernel), Cin = 64 over 128-pixel-wide images:
//   rows       64 -> 64 (pair output)   64 -> 12        64 -> 32
//   16,384     31.2 -> 22.9             22.5 -> 18.8    25.6 -> 17.2
//   32,768     33.5 -> 22.1             28.7 -> 18.9    27.1 -> 18.3
//   65,536     35.8 -> 27.5             27.5 -> 20.1    25.6 -> 20.8
//   131,072    51.5 -> 39.4             39.8 -> 25.8    38.0 -> 25.4
//   262,144    81.2 -> 64.0             64.9 -> 44.4    61.4 -> 42.0
//   524,288    150.1 -> 113.5           111.2 -> 73.2   106.2 -> 73.3
// The patch kernel already wins at the lowest size tried, so there is no crossover above the floor: the threshold sits at the
// 16,384 rows it was first set to (it may not sit at or below 8,192: tests/conv_choice_cases.json records the per-tap tiles up to
// there).  The model's shapes at B = 8 (ms): seg head 1.324 -> 0.883, layer1 conv2 0.457 -> 0.374 per call; at B = 1: 0.179 -> 0.117,
// 0.081 -> 0.060.  Both forms win at the model's shapes and in the headline, so both are routed.
bool choose_x3_patch(const ConvArgs& a, ConvChoice* c) {
    static const bool on = env_flag("TT_X3_PATCH", true);
    if (!on || !(a.flags & 32) || a.M < kPatchMinRows) return false;
    if (a.KH != 3 || a.KW != 3 || a.stride != 1 || a.pad != 1 || a.dil != 1 || a.OH != a.H || a.OW != a.W) return false;
    if (a.Cin % 32 != 0 || !(a.Cout == 64 || (a.Cout >= 8 && a.Cout <= 32)) || !a.vec_epi || a.out_dtype != TT_F32) return false;
    if (a.res1 || a.res2 || a.shift_n || a.out2 || a.ws || a.pixel_shuffle2 || a.gather || a.m_dev) return false;
    if ((long long)a.H * a.W * a.in_cstride >= (1ll << 30)) return false;        // 32-bit byte offsets inside an image
    // 64-wide with K >= 1152 (128+ input channels): the one such layer of the model is unet_layer0.1, which has its own patch kernel
    // (in_up2); its two-launch form (TT_SEG_UP2=0) stays the per-tap tile it is compared against (tests/test_conv_up2_choice.py)
    if (a.Cout == 64 && a.K >= 1152) return false;
    set_tile(c, CONV_X3_PATCH, a.Cout == 64 ? 64 : 32, 8, 1, 128, 3);
    return true;
}

// ---- bf16x3 arithmetic on f32 storage (conv_igemm_glds.hip's X3 tiles and the kernels derived from them).  false when the shape is
// outside the LDS-DMA kernels' contract (the layer then runs the exact f32 path on the plain weights).
bool choose_x3(const ConvArgs& a, ConvChoice* c) {
    c->x3 = true;
    if (a.gather) {
        if (choose_sp_runs_l2(a, c)) return true;   // 3x3x3 rulebooks with 16 / 32 channels over many rows: weights resident in LDS
        if (choose_sp_runs(a, c)) return true;      // 3x3x3 rulebooks with 32+ channels: run-staged kernel
        const bool cin_ok = a.Cin >= 16 && (a.Cin & (a.Cin - 1)) == 0;
        if (!cin_ok || a.M < 2048 || a.Cout < 16 || a.Cout > 128) return false;
        set_tile(c, CONV_GLDS, a.Cout <= 32 ? 32 : (a.Cout <= 64 ? 64 : 128), 8, 1, 128, 2);
        c->gather = true;
        return true;
    }
    if (a.m_dev || a.M < 2048 || a.KH * a.KW > 32) return false;
    if (a.Cin % 32 != 0 || a.K < 64) return false;       // 128 B rows = 32 f32 of one tap per K tile, >= 2 tiles
    // pre-split activations (tt_conv_desc.in_pair): 16-channel pair groups must line up with the 32-channel K tiles
    const bool apair = (a.flags & 32) != 0;
    if (apair && (a.in_coff % 16 != 0 || a.in_cstride % 16 != 0)) return false;
    c->apair = apair;
    if (choose_x3_patch(a, c)) return true;
    // few output channels over many rows (the segmentation head: 3 x 3, 64 -> 12 at 224 x 448 per image; the deformable conv's
    // offset head: 3 x 3, 512 -> 18; seg_res_to_image_feature's 64 -> 16): a 256 x 32 tile, two workgroups per CU.  Below 2^16
    // rows the exact-f32 register-staged kernel keeps them
    if (a.Cout < 64) {
        if (a.Cout > 32 || a.Cout < 8) return false;
        if (!apair && a.M < (1 << 16)) return false;
        set_tile(c, CONV_GLDS, 32, 8, 1, 128, 2);
        return true;
    }
    // Tile width along N.  The widest wave tile the layer allows is the most efficient per tile (the operand split costs
    // 8/TN VALU per MFMA; measured ~1.0 / 0.85 / 0.63 relative MFMA rate for the 256 / 128 / 64 wide tiles), but a
    // launch with fewer workgroups than the chip holds (batch-1 ticks: 49 row tiles x 2 on 256 CUs) is bound by its
    // rounds, not by the per-tile rate: pick the width with the smallest  rounds x (BN / rate).
    const int tiles_m = div_up(a.M, 256);
    auto cost = [&](int bn, double rate) {      // the busiest CU runs ceil(tiles / 256) tiles at the tile's measured rate
        const long long tiles = (long long)tiles_m * div_up(a.Cout, bn);
        return (double)((tiles + kNumCU - 1) / kNumCU) * bn / rate;
    };
    const bool wide = a.Cout % 256 == 0 || a.Cout > 512;
    const int main_rows = tail_split_rows(a);
    // 256-wide with a tail split: the main launch's full rounds + the peeled row tiles as 256 x 64 tiles
    auto cost256 = [&]() {
        if (!main_rows) return cost(256, 1.0);
        const long long tn = a.Cout / 256;
        const long long main_tiles = (long long)main_rows * tn, tail_tiles = (long long)(tiles_m - main_rows) * tn * 4;
        return (double)((main_tiles + kNumCU - 1) / kNumCU) * 256 / 1.0 + (double)((tail_tiles + kNumCU - 1) / kNumCU) * 64 / 0.63;
    };
    const double c256 = wide ? cost256() : 1e30;
    // (long-K layers run the 128-wide tile on the hand-pipelined kernel: 404 vs 423 TF/s for the 256-wide one, profiles/r04_run3_ab.txt)
    const double c128 = a.Cout > 64 ? cost(128, (a.K >= 1152 && a.Cout % 128 == 0) ? 0.95 : 0.85) : 1e30;
    const double c64 = cost(64, 0.63);
    const int bn = (c256 <= c128 && c256 <= c64) ? 256 : (c128 <= c64 ? 128 : 64);
    // Long-K layers (K >= 1152: every 3 x 3 of the trunks) on the 256- and 128-wide tiles: four hand-pipelined waves, one per SIMD
    // (csrc/conv_x3_pipe.hip: MFMA pipe 77 % busy against 58 %, profiles/r04_conv_sq_counters_noepilogue.txt).  Short K keeps the
    // 8-wave tile: there the tile's prologue + epilogue dominate and eight waves issue the output stores faster than four
    // (K = 1024: 0.203 vs 0.216 ms, K = 256 N = 1280: 0.52 vs 0.77 ms; profiles/r04_pipe_ab_first.txt).
    // TT_X3_PIPE=0 (test hook: tests/test_conv.py compares the two families bit for bit): the compiler-scheduled tiles everywhere
    static const bool pipe = env_flag("TT_X3_PIPE", true);
    if (pipe && a.K >= 1152 && bn != 64 && x3_pipe_ok(a, bn)) {
        // 3 x 3 stride-1 "same" convolutions over a dense batch: the run-staged form (one staged pixel run per filter row serves
        // its three taps).  TT_X3_RUN3=0 (test hook: tests/test_conv.py compares the two forms bit for bit): the per-tap form everywhere
        static const bool run3 = env_flag("TT_X3_RUN3", true);
        const bool runs = run3 && a.KW == 3 && a.KH <= 5 && a.stride == 1 && a.dil == 1 && a.pad == 1 && a.OH == a.H && a.OW == a.W &&
                          (a.N == 1 || a.in_nstride == (long long)a.H * a.W * a.in_cstride);
        // wave grid 4 x 1: 64 x 256 (64 x 128 on the 128-wide tile) per wave -- every activation fragment is split by ONE wave (the
        // 2 x 2 grid of 128 x 128 waves measured slower, profiles/r04_pipe_ab_grids.txt)
        set_tile(c, runs ? CONV_X3_RUN3 : CONV_X3_PIPE, bn, 4, 1, 128, 23);
    } else if (bn == 256) {
        set_tile(c, CONV_GLDS, 256, 4, 2, 128, 23);      // 8 x (64 x 128), 3 + 2 stages = 160 KiB
    } else {
        // Narrow tiles: two LDS stages (a third costs the 64-wide tile its second workgroup per CU: N=64 K=576 2.13 -> 2.66 ms), eight
        // waves (four waves of 64 x 64 on the 64-wide tile: 3-15 % slower, profiles/r05_x3_64wide_waves_ab.txt; pre-split activations:
        // 1-5 % slower there too, profiles/r06_pair_format.txt)
        set_tile(c, CONV_GLDS, bn, 8, 1, 128, 2);        // 8 x (32 x 128) / 8 x (32 x 64)
    }
    if (bn == 256) c->main_rows = main_rows;
    return true;
}

// ---- bf16x3 3 x 3 convolution that reads its input through the bilinear x2 upsampling (conv_x3_up2.hip, tt_conv_desc.in_up2): the
// kernel's whole contract.  a.H / a.W are the upsampled size.  More than kSmallMaxRows rows, as for in_pair: up to there a layer runs
// the latency kernel.  Measured against the two launches it replaces in profiles/seg_up2_fusion.txt.
int choose_up2(const ConvArgs& a, const ConvFacts& f, ConvChoice* c) {
    TT_REQUIRE(f.dtype == TT_F32 && a.out_dtype == TT_F32 && f.weight_x3 && aligned16(f.weight_x3) && !f.weight_h2,
               "tt_conv2d_fwd: in_up2 goes with a bf16x3 layer (f32 storage, a 16-byte aligned weight_x3)");
    TT_REQUIRE(!a.gather && !a.m_dev && !a.ws && !a.pixel_shuffle2 && !(a.flags & 32) && !a.res1 && !a.res2 && !a.shift_n && !f.out2,
               "tt_conv2d_fwd: in_up2 takes no in_pair, residual, per-image shift, out2, split-K workspace, gather or pixel shuffle");
    TT_REQUIRE(a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.dil == 1 && a.H % 2 == 0 && a.W % 2 == 0 && a.OH == a.H &&
                   a.OW == a.W,
               "tt_conv2d_fwd: in_up2 is a 3 x 3 / stride 1 / pad 1 layer over an even H x W (got %d x %d, k %d x %d s %d p %d d %d)", a.H,
               a.W, a.KH, a.KW, a.stride, a.pad, a.dil);
    static_assert(kSmallMaxRows == 4096, "the refusal below spells the number");
    TT_REQUIRE(a.Cin % 32 == 0 && a.Cout == 64 && a.M > kSmallMaxRows && a.vec_epi,
               "tt_conv2d_fwd: in_up2 layer outside the kernel's contract (Cin %% 32 == 0, Cout == 64, more than 4096 rows, aligned "
               "output: M=%d Cin=%d Cout=%d)", a.M, a.Cin, a.Cout);
    const long long img = (long long)(a.H / 2) * (a.W / 2) * a.Cin;
    TT_REQUIRE(a.in_cstride == a.Cin && a.in_coff == 0 && a.in_nstride == img && img < (1ll << 30),
               "tt_conv2d_fwd: in_up2 reads a contiguous [N][H/2][W/2][Cin] source of less than 2^30 elements per image");
    set_tile(c, CONV_X3_UP2, 64, 8, 1, 128, 3);
    c->x3 = true;
    return 0;
}

// ---- a 1 x 1 bf16x3 layer with a joined stage (conv_x3_join.hip, tt_conv2d_fwd_next): the kernel's whole contract.  A call
// that names a next stage (tt_conv_next) runs here or is refused -- it never becomes two launches.  `a` / f.join are the two stages as the layers
// they would be alone; each is put to conv_choose by itself, since the joined kernel reproduces the sums of the bf16x3 LDS-DMA tiles
// (k ascending in 16-wide steps, bf16x3.h's one-accumulator order) and of nothing else.
// Forms <Cin, next_cout, waves>: <64, 64, 8> <64, 128, 8> <128, 128, 8> <128, 256, 4> <256, 256, 4>; a workgroup covers 32 rows per wave.
// Threshold kJoinMinRows = 32,768 rows, one value for every form.  Measured crossover (profiles/bottleneck_join.txt; us, serialised,
// minimum of 10, the two launches -> the joined one; one image 128 pixels wide, residual and ReLU):
//   rows       64 -> 256 -> 64   64 -> 256 -> 128   128 -> 512 -> 128   128 -> 512 -> 256   256 -> 1024 -> 256
//   4,608      33.0 -> 30.2      33.2 -> 35.2       44.8 -> 63.3        44.6 -> 67.0        71.8 -> 133.4
//   8,192      33.0 -> 30.7      32.9 -> 37.1       46.6 -> 64.4        46.4 -> 68.0        78.8 -> 134.0
//   16,384     36.0 -> 31.7      35.9 -> 35.8       58.3 -> 66.9        59.2 -> 72.5        102.0 -> 138.0
//   32,768     45.7 -> 33.4      46.8 -> 40.0       76.1 -> 69.2        86.8 -> 78.8        165.6 -> 154.2
//   65,536     65.0 -> 38.5      71.3 -> 46.5       125.1 -> 83.0       143.8 -> 146.9      303.9 -> 322.3
//   131,072    112.3 -> 78.0     128.1 -> 93.5      248.4 -> 166.2      282.2 -> 288.6      567.9 -> 596.2
//   262,144    202.4 -> 155.2    245.2 -> 183.8     456.1 -> 309.6      521.0 -> 524.9      1091.6 -> 1152.2
// The three eight-wave forms win from 32,768 rows on (64 -> 256 -> 64 already from the floor, by 2 - 4 us); below, 64 -> 256 -> 128 and
// 128 -> 512 -> 128 lose.  The two four-wave forms (one wave per SIMD) win at 32,768 rows only and lose at the model's row counts
// (B = 8: 819 -> 835 and 497 -> 586 us; B = 1: 125 -> 132 and 95 -> 136): callers leave them to two launches (ops.JOIN_ROUTED); the
// kernel keeps them.  The model's routed shapes (us): B = 8 1074 -> 805, 1297 -> 961, 710 -> 501; B = 1 160 -> 137, 202 -> 158, 108 -> 72.
// A call below the threshold is still run here, down to kJoinFloorRows, and its label says " below kJoinMinRows": callers route by
// that label (ops.join_ok asks tt_conv2d_plan_next), so the number stands in conv_choose.h alone.
int choose_join(const ConvArgs& a, const ConvFacts& f, ConvChoice* c) {
    const ConvArgs& n = *f.join;
    TT_REQUIRE(f.dtype == TT_F32 && a.out_dtype == TT_F32 && f.weight_x3 && aligned16(f.weight_x3) && !f.weight_h2,
               "tt_conv2d_fwd: next_out goes with a bf16x3 layer (dtype / out_dtype TT_F32, a 16-byte aligned weight_x3)");
    TT_REQUIRE(f.join_weight_x3 && aligned16(f.join_weight_x3), "tt_conv2d_fwd: next_weight_x3 must be given and 16-byte aligned");
    TT_REQUIRE(a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0 && a.OH == a.H && a.OW == a.W,
               "tt_conv2d_fwd: next_out needs a 1 x 1 / stride 1 / pad 0 layer (got k %d x %d s %d p %d)", a.KH, a.KW, a.stride, a.pad);
    TT_REQUIRE(!a.gather && !a.m_dev && !a.ws && !a.pixel_shuffle2 && !a.res2 && !a.shift_n && !f.out2 && !f.res1_up && !(a.flags & (64 | 256)),
               "tt_conv2d_fwd: next_out takes no res2, shift_n, out2, res1_up, out_pair, in_up2, splitk_ws, gather_idx or pixel_shuffle2");
    TT_REQUIRE((a.Cin == 64 || a.Cin == 128 || a.Cin == 256) && a.Cout == 4 * a.Cin,
               "tt_conv2d_fwd: next_out needs Cin = 64, 128 or 256 and Cout = 4 Cin (got Cin=%d Cout=%d)", a.Cin, a.Cout);
    TT_REQUIRE(n.Cout == a.Cin || (n.Cout == 2 * a.Cin && a.Cin <= 128),
               "tt_conv2d_fwd: next_cout = %d has no joined kernel beside Cin = %d (64 or 128 / 128 or 256 / 256)", n.Cout, a.Cin);
    TT_REQUIRE(a.act == TT_ACT_NONE || a.act == TT_ACT_RELU, "tt_conv2d_fwd: next_out needs act none or ReLU (got %d)", a.act);
    TT_REQUIRE(n.act == TT_ACT_NONE || n.act == TT_ACT_RELU, "tt_conv2d_fwd: next_act must be none or ReLU (got %d)", n.act);
    TT_REQUIRE(a.M >= kJoinFloorRows, "tt_conv2d_fwd: next_out needs N*OH*OW of at least %d rows (got %d)", kJoinFloorRows, a.M);
    TT_REQUIRE(a.in_nstride == (long long)a.H * a.W * a.in_cstride && (!(a.flags & 32) || (a.in_cstride % 16 == 0 && a.in_coff % 16 == 0)),
               "tt_conv2d_fwd: next_out needs a row-linear `in` (in_nstride 0 or H*W*in_cstride; in_pair: in_cstride / in_coff multiples of 16)");
    TT_REQUIRE(a.out_fast && a.vec_epi && a.res_vec, "tt_conv2d_fwd: next_out needs a row-linear `out` and 16-byte aligned out / res1 rows");
    TT_REQUIRE((n.flags & 64) && n.out_fast && n.vec_epi,
               "tt_conv2d_fwd: next_out_pair must be 1, with a row-linear next_out and next_cout / next_out_cstride / next_out_coff multiples of 16");
    // each stage alone: a bf16x3 LDS-DMA tile without split-K, or no joined form
    ConvFacts f1 = f, f2{};
    f1.join = nullptr;
    f1.join_weight_x3 = nullptr;
    f2.dtype = TT_F32;
    f2.weight_x3 = f.join_weight_x3;
    ConvChoice s1, s2;
    if (conv_choose(a, f1, &s1) || conv_choose(n, f2, &s2)) return -1;
    auto same_sums = [](const ConvChoice& s) { return s.family == CONV_GLDS && s.x3 && !s.gather && s.splits <= 1; };
    TT_REQUIRE(same_sums(s1), "tt_conv2d_fwd: next_out: this layer alone (M=%d Cin=%d Cout=%d) would not run on a bf16x3 LDS-DMA tile", a.M,
               a.Cin, a.Cout);
    TT_REQUIRE(same_sums(s2), "tt_conv2d_fwd: next_out: the next layer alone (M=%d %d -> next_cout=%d) would not run on a bf16x3 LDS-DMA tile",
               n.M, n.Cin, n.Cout);
    const int nw = (n.Cout == 256) ? 4 : 8;
    set_tile(c, CONV_X3_JOIN, n.Cout, nw, 1, a.Cin * 4, 2);      // (bkb = 4 Cin: bytes of a weight row of this layer)
    c->x3 = true;
    c->apair = (a.flags & 32) != 0;
    c->below_min = a.M < kJoinMinRows;
    return 0;
}

// ---- the LDS-DMA kernel on exact-f32 and 16-bit operands (conv_igemm_glds.hip)
bool choose_glds(const ConvArgs& a, int dtype, ConvChoice* c) {
    constexpr int min_tiles = 2;      // K = 64 1x1 layers: 0.43 -> 0.27 ms against the register-staged kernel
    if (a.gather) {
        // sparse 3D conv as a gathered GEMM (rulebook rows): whole 128 B+ activation rows per DMA lane group
        const bool cin_ok = a.Cin >= 16 && (a.Cin & (a.Cin - 1)) == 0;   // power of two: taps tile the 128 B rows
        if (dtype == TT_F32 || !cin_ok || a.M < 2048 || a.Cout < 16 || a.Cout > 128) return false;
        if (a.Cout <= 32) set_tile(c, CONV_GLDS, 32, 8, 1, 128, 2);
        else if (a.Cout <= 64) set_tile(c, CONV_GLDS, 64, 8, 1, 128, 2);
        else set_tile(c, CONV_GLDS, 128, 4, 2, 128, 2);
        c->gather = true;
        return true;
    }
    if (a.m_dev || a.M < 2048 || a.Cout < 64 || a.KH * a.KW > 32) return false;
    if (dtype == TT_F32) {
        if (a.Cin % 16 != 0 || div_up(a.K, 16) < min_tiles) return false;
        if (a.Cout > 64) set_tile(c, CONV_GLDS, 128, 4, 2, 64, 3);
        else set_tile(c, CONV_GLDS, 64, 8, 1, 64, 3);
        return true;
    }
    if (a.Cin % 32 != 0 || div_up(a.K, 32) < min_tiles) return false;
    // Tile selection (profiles/r01_conv_microbench_tiles.txt).  Three things set the rate of these kernels:
    //  * L2->LDS bytes per FLOP = workgroup tile: 256x128 -> 85 FLOP/B, 256x256 -> 128 FLOP/B;
    //  * whether a DMA lane group consumes WHOLE 128 B cache lines: with 64 B rows every activation line is
    //    fetched twice from L2 (the other half is needed one K tile later and the 32 KiB L1 cannot hold a tile);
    //    128 B rows in 2 stages beat 64 B rows in 3 stages by 10-17 % on every layer whose LDS budget allows it;
    //  * LDS fragment bytes per MFMA = per-wave register tile (64x64: 1 KiB, 128x64: 0.75 KiB) -- second order.
    // Auto: Cout % 256 == 0 -> 256x256 tile of eight 128x64 waves (128 B rows if Cin % 64 == 0); short K -> four
    // 128x64 waves on 256x128; Cout <= 64 -> 256x64 tile with 128 B rows; else eight 64x64 waves on 256x128.
    // Retired after measurement (same file): 16-wave 256x256, 8x1 wave grid, 128 B rows x 3 stages (1 workgroup/CU),
    // 128 B x 2 stages on the 256x128 tile.
    if (a.Cout > 64) {
        const long long tiles256 = (long long)div_up(a.M, 256) * (a.Cout / 256);
        if (a.Cout % 256 == 0 && tiles256 >= 200) {
            if (a.Cin % 64 == 0) {
                set_tile(c, CONV_GLDS, 256, 2, 4, 128, 2);
                c->main_rows = tail_split_rows(a);
            } else {
                set_tile(c, CONV_GLDS, 256, 2, 4, 64, 3);          // 8 waves x 128x64
            }
        } else if (a.K <= 512) {
            set_tile(c, CONV_GLDS, 128, 2, 2, 64, 3);              // 4 waves x 128x64
        } else {
            set_tile(c, CONV_GLDS, 128, 4, 2, 64, 3);              // 8 waves x 64x64
        }
        return true;
    }
    // Cout <= 64 (the 224x448 UNet / stem-level layers): 128 B rows in 2 stages (80 KiB, 2 workgroups / CU)
    // measured +17 % over 64 B rows x 3 stages (1.61 vs 1.89 ms on M=6.4M K=1152)
    if (a.Cin % 64 == 0) set_tile(c, CONV_GLDS, 64, 8, 1, 128, 2);
    else set_tile(c, CONV_GLDS, 64, 8, 1, 64, 3);
    return true;
}

// ---- the register-staged kernel (conv_igemm.hip) takes everything; with a workspace, few tiles and a long K it splits K
int choose_igemm(const ConvArgs& a, int dtype, bool ws, bool assume_ws, ConvChoice* c) {
    if (a.Cout > 64) set_tile(c, CONV_IGEMM, 128, 2, 2, 64, 2);
    else if (a.Cout > 32) set_tile(c, CONV_IGEMM, 64, 2, 2, 64, 2);
    else set_tile(c, CONV_IGEMM, 32, 4, 1, 64, 2);
    if (dtype != TT_F32) c->bkb = 128;
    c->gather = a.gather != nullptr;
    const int tiles = div_up(a.M, 128) * div_up(a.Cout, c->bn);
    const int nk = div_up(a.K, c->bkb / (dtype == TT_F32 ? 4 : 2));
    if (ws && !a.m_dev && tiles < 128 && nk >= 8) {
        int sp = div_up(512, tiles);
        if (sp > nk / 2) sp = nk / 2;
        if (sp > 64) sp = 64;
        c->splits = sp < 1 ? 1 : sp;
    }
    if (c->splits <= 1) return 0;
    c->slices = c->splits;
    if (!assume_ws) {
        c->slices = 0;
        if (a.ws_slices > 0) {
            // ordered form: the non-empty splits (the K tiles are dealt in runs of ceil(nk / splits)) store into their own slices
            const int eff = div_up(nk, div_up(nk, c->splits));
            TT_REQUIRE(a.ws_slices >= eff, "tt_conv2d_fwd: split-K workspace holds %d slices, %d needed", a.ws_slices, eff);
            c->slices = eff;
        }
    }
    return 0;
}

}  // namespace

int conv_choose(const ConvArgs& a, const ConvFacts& f, ConvChoice* c) {
    *c = ConvChoice{};
    c->splits = 1;
    const bool ws = a.ws || f.assume_ws;
    if (f.join) return choose_join(a, f, c);            // tt_conv_next: the joined kernel or an error
    if (a.flags & 256) return choose_up2(a, f, c);      // in_up2: its own kernel or an error
    if (f.weight_h2) {
        // half storage x (hi, lo) weights: the only kernel with this arithmetic -- a shape outside its contract is an error, not a
        // silent change of precision
        TT_REQUIRE(aligned16(f.weight_h2), "tt_conv2d_fwd: weight_h2 must be 16-byte aligned");
        TT_REQUIRE(choose_h2(a, c), "tt_conv2d_fwd: weight_h2 layer outside the h2 kernel's contract (Cin=%d KH*KW=%d)", a.Cin,
                   a.KH * a.KW);
        return 0;
    }
    TT_REQUIRE(!f.out2 || a.vec_epi, "tt_conv2d_fwd: out2 needs the vector epilogue (aligned channel counts)");
    TT_REQUIRE(!f.res1_up || a.vec_epi, "tt_conv2d_fwd: an upsampled res1 needs the vector epilogue (aligned channel counts)");
    TT_REQUIRE(!f.res1_f32 || (a.vec_epi && a.res_vec), "tt_conv2d_fwd: an f32 res1 needs the vector epilogue and aligned residual rows");
    TT_REQUIRE(!(f.dtype == TT_F32 && a.out_dtype != TT_F32 && a.res1) || (a.vec_epi && a.res_vec),
               "tt_conv2d_fwd: a 16-bit output of an f32 layer with a residual needs the vector epilogue");
    if (a.flags & (32 | 64)) {      // in_pair / out_pair: bf16x3 on the LDS-DMA kernels or nothing
        TT_REQUIRE(a.vec_epi && aligned16(f.weight_x3) && a.K % 16 == 0,
                   "tt_conv2d_fwd: in_pair / out_pair need the vector epilogue and a 16-byte aligned weight_x3");
        TT_REQUIRE(choose_x3(a, c), "tt_conv2d_fwd: pair-format layer outside the LDS-DMA bf16x3 kernel's contract (M=%d Cin=%d Cout=%d)",
                   a.M, a.Cin, a.Cout);
        return 0;
    }
    if (!ws && !f.out2 && !f.res1_up && !f.res1_f32 && choose_small(a, c)) return 0;
    const bool x3 = f.weight_x3 && f.dtype == TT_F32;
    // few rows, long K, bf16x3 operand: the 64-wide x3 tile, K split
    if (ws && x3 && a.K % 16 == 0 && aligned16(f.weight_x3) && choose_x3_splitk(a, f.assume_ws, c)) return 0;
    if (!ws && x3) {
        TT_REQUIRE(aligned16(f.weight_x3) && a.K % 16 == 0, "tt_conv2d_fwd: weight_x3 needs 16-byte alignment and K %% 16 == 0 (K = %d)",
                   a.K);
        if (choose_x3(a, c)) return 0;
        *c = ConvChoice{};
        c->splits = 1;
    }
    if (!ws && choose_glds(a, f.dtype, c)) return 0;
    return choose_igemm(a, f.dtype, ws, f.assume_ws, c);
}

ConvChoice conv_tail_choice(const ConvChoice& c) {
    ConvChoice t{};
    set_tile(&t, CONV_GLDS, 64, 8, 1, 128, 2);
    t.x3 = c.x3;
    t.apair = c.apair;
    t.splits = 1;
    return t;
}

void conv_label(const ConvChoice& c, int dtype, char* out, size_t bytes) {
    const char* tn = dtype == TT_F32 ? "float" : "16-bit";
    const char* pre = c.apair ? " pre-split A" : "";
    const char* tail = c.main_rows > 0 ? " + tail" : "";
    switch (c.family) {
        case CONV_H2: snprintf(out, bytes, "conv_h2_kernel<%d, %d, %d, %d, %d>", c.bn, c.waves_m, c.waves_n, c.stages / 10, c.stages % 10); break;
        case CONV_H2_PIPE: snprintf(out, bytes, "conv_h2_pipe_kernel"); break;
        case CONV_SMALL: snprintf(out, bytes, "conv_small_kernel"); break;
        case CONV_SP_RUNS_L2: snprintf(out, bytes, "sp_conv_runs_l2_kernel<%d>", c.bkb / 4); break;
        case CONV_SP_RUNS: snprintf(out, bytes, "sp_conv_runs_kernel<%d, %d, %d>", c.bn / (32 * c.waves_n), c.waves_m, c.waves_n); break;
        case CONV_X3_PIPE: snprintf(out, bytes, "conv_x3_pipe_kernel<%s>%s%s", c.bn == 128 ? "4, 1, 128" : "4, 1", pre, tail); break;
        case CONV_X3_RUN3: snprintf(out, bytes, "conv_x3_run3_kernel<%d>%s%s", c.bn, pre, tail); break;
        case CONV_X3_UP2: snprintf(out, bytes, "conv_x3_run3_kernel<%d, up2>", c.bn); break;     // (run-staged family: one patch, nine taps)
        case CONV_X3_PATCH: snprintf(out, bytes, "conv_x3_run3_kernel<%d, patch>%s", c.bn, pre); break;          // (the same family)
        case CONV_X3_JOIN: snprintf(out, bytes, "conv_x3_join_kernel<%d, %d, %d>%s%s", c.bkb / 4, c.bn, c.waves_m, pre, c.below_min ? " below kJoinMinRows" : ""); break;
        case CONV_GLDS:
            snprintf(out, bytes, "conv_igemm_glds_kernel<%s, %d, %d, %d, %d, %d, %s, %s>%s%s", tn, c.bn, c.waves_m, c.waves_n, c.bkb,
                     c.stages, c.gather ? "true" : "false", c.x3 ? "true" : "false", pre, c.splits > 1 ? " split-K" : tail);
            break;
        default: snprintf(out, bytes, "conv_igemm_kernel<%s, 128, %d>%s", tn, c.bn, c.splits > 1 ? " split-K" : ""); break;
    }
}

}  // namespace tt
