// Which kernel a weight gradient runs on: the choice tt_conv2d_wgrad / tt_conv2d_wgrad_x3 / tt_gather_conv_wgrad make for a layer
// (WgradChoice) and the host functions that make it (wgrad_choose.cpp).  Host-only: no kernel includes anything from here.
#pragma once
#include <stddef.h>

#include "tt_common.h"

namespace tt {

// Kernel families of conv_bwd.hip.
enum WgradFamily {
    WGRAD_TILE64,   // conv_wgrad_kernel / gather_wgrad_kernel: a workgroup owns a 64 x 64 tile, its four waves are added through LDS
    WGRAD_WAVE,     // conv_wgrad_wide_kernel<bi, bj> / gather_wgrad_wide_kernel<bi, bj>: every wave owns a (32 bi) x (32 bj) tile
    WGRAD_LDS,      // conv_wgrad_lds_kernel<bi, bj>: LDS-staged bf16x3, a workgroup owns a (64 bi) x (64 bj) tile (dense layers only)
};

// What the dense launch knows about a layer (the gathered one needs nothing but M, the channels and the taps).
struct WgradLayer {
    const void* x;              // tested for 16-byte alignment, never read
    const void* dy;
    int N, H, W, Cin, x_cstride, x_coff;
    int OH, OW, Cout, dy_cstride, dy_coff;
    int KH, KW, stride, pad, cin_pad;
    bool x3;                    // tt_conv2d_wgrad_x3: the LDS-staged kernel where its contract holds
};

struct WgradChoice {
    int family;                 // WgradFamily
    int bi, bj;                 // the family's template arguments: tile in 32- (WGRAD_LDS: 64-) channel blocks along Cout / Cin
    int tiles;                  // gridDim.x: (Cout tiles) x ci_tiles x taps
    int splits;                 // gridDim.y: ranges of output rows (gathered: of live row pairs)
    int slices;                 // partial-sum slices of the workspace the reduce kernel adds: splits, x 4 in WGRAD_WAVE (one per wave)
    int rows_per_split;         // dense: output rows (n, oh) per split
    int ci_tiles;               // tiles along cin_pad
    size_t lds_bytes;           // dynamic LDS of the launch (WGRAD_LDS: its two stages)
    int N, OH, OW, H, W;        // the geometry the kernel is launched with: a 1 x 1 layer's regrouped pseudo-rows, else the caller's
    bool regrouped;
};

// tile of one wave in 32-channel blocks per side (the f32 kernels; 2 x 2 = WGRAD_TILE64)
void wgrad_blocks(int Cout, int Cin, int* bi, int* bj);
// The kernel a validated dense / gathered layer runs on.  Touch no device.
WgradChoice wgrad_choose(const WgradLayer& l);
WgradChoice gather_wgrad_choose(long long M, int Cout, int Cin, int cin_pad, int taps);
// Partial-sum slices the caller's workspace must hold (tt_conv2d_wgrad_workspace_bytes: it knows neither x3 nor OW).
int wgrad_workspace_slices(int N, int OH, int Cout, int Cin, int taps);
// "kernel<bi, bj> grid X x Y lds B reduce S[ as N=.. OH=.. OW=.. H=.. W=..]": the kernel's name with its template arguments as
// rocprofv3 prints them, the grid in workgroups, dynamic LDS bytes, the slices reduced and, where it was regrouped, the geometry.
void wgrad_label(const WgradChoice& c, bool gathered, char* out, size_t bytes);

}  // namespace tt
