// The dispatch of tt_conv2d_wgrad / tt_conv2d_wgrad_x3 / tt_gather_conv_wgrad, stated once: from a validated layer to the kernel
// family, its template arguments, the grid, the row split, the slices the reduce kernel adds and the geometry of the launch.  Plain
// host arithmetic (no HIP call), so tt_conv2d_wgrad_plan / tt_gather_conv_wgrad_plan and the workspace queries answer without a
// device and the rules are testable on any machine (tests/test_wgrad_choice.py).  The launchers in conv_bwd.hip only map a choice
// onto its template instantiation; a rule that is not here does not exist.
//
// The split decides which partial sums are added in which order, i.e. the bits of the gradient: no number here moves without a
// new record in tests/wgrad_choice_cases.json.
#include <stdint.h>

#include "wgrad_choose.h"

namespace tt {

// tile of one wave in 32-channel blocks per side: 4 (128 channels) where the side has >= 128, 1 where it has <= 32 (the
// segmentation / depth heads, the stem's 3 input channels: a 64-wide tile would multiply mostly zeros), else 2.  2 x 2 is the
// 64 x 64 workgroup-tile kernel, everything else the per-wave-tile kernel.
void wgrad_blocks(int Cout, int Cin, int* bi, int* bj) {
    *bi = Cout >= 128 ? 4 : (Cout <= 32 ? 1 : 2);
    *bj = Cin >= 128 ? 4 : (Cin <= 32 ? 1 : 2);
}

namespace {

// "workgroups per CU -> splits": enough row ranges that `tiles` workgroups per range put per_cu workgroups on every CU
long long splits_for(long long per_cu, long long tiles) { return (per_cu * kNumCU + tiles - 1) / tiles; }

// Row ranges of the f32 kernels over `tiles` workgroups each: aim at >= 4 workgroups per CU, 2 for the 128-wide wave tiles (one
// wave per SIMD each, and every split costs four partial slices); at most `most` (what the rows allow), at least 1, at most 1024.
int f32_splits(int bi, int bj, long long tiles, long long most) {
    long long s = splits_for(bi * bj >= 8 ? 2 : 4, tiles);
    if (s > most) s = most;
    if (s < 1) s = 1;
    if (s > 1024) s = 1024;
    return (int)s;
}

// The f32 choice of a dense layer, over the caller's geometry.  It is also what sizes the workspace (wgrad_workspace_slices), so it
// may depend on nothing but N, OH, the channel counts and the taps.  (It counts its tiles over Cin, the grid over cin_pad: the two
// differ only where cin_pad pads past a tile boundary.)
void choose_f32(int N, int OH, int Cout, int Cin, int taps, WgradChoice* c) {
    wgrad_blocks(Cout, Cin, &c->bi, &c->bj);
    c->family = (c->bi == 2 && c->bj == 2) ? WGRAD_TILE64 : WGRAD_WAVE;
    const long long tiles = (long long)div_up(Cout, 32 * c->bi) * div_up(Cin, 32 * c->bj) * taps;
    c->splits = f32_splits(c->bi, c->bj, tiles, N * OH / 4);      // every wave of a workgroup gets at least one row
    c->slices = c->splits * (c->family == WGRAD_TILE64 ? 1 : 4);  // the per-wave-tile kernel: one slice per wave
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- LDS-staged bf16x3 kernel (conv_wgrad_lds_kernel): >= 64 channels on both sides (iteration 962 -> 820 ms against the f32-MFMA
// wave-tile form), 16-byte DMA slots (channel counts, strides, offsets in multiples of 4 floats, aligned bases), rows of >= 16 pixels.
// `cap`: the slices of the caller's workspace.  The workspace query knows neither x3 nor OW, so it answers for the f32 choice, and
// this kernel's splits are CLAMPED to that answer -- where the clamp binds, the gradient's bits depend on it.
bool choose_lds(const WgradLayer& l, int cap, WgradChoice* c) {
    if (!l.x3 || l.Cout < 64 || l.Cin < 64) return false;
    if (l.Cout % 4 || l.Cin % 4 || l.x_cstride % 4 || l.x_coff % 4 || l.dy_cstride % 4 || l.dy_coff % 4) return false;
    if (!aligned16(l.x) || !aligned16(l.dy)) return false;
    // the kernel walks image rows in 32-pixel segments: a 1x1 / stride-1 / unpadded layer (linear layers over rows: OW = 1) is the
    // same sum over ANY regrouping of its pixels, so short rows are merged into pseudo-rows of >= 128 pixels -- m rows each, m the
    // smallest divisor of the row count that reaches 128 pixels; without one the layer keeps its rows
    if (l.KH == 1 && l.KW == 1 && l.stride == 1 && l.pad == 0 && l.OW < 128) {
        const long long prow = (long long)l.N * l.OH;
        long long m = (128 + l.OW - 1) / l.OW;
        while (m < prow && prow % m) ++m;
        if (m <= prow && prow % m == 0) {
            c->N = 1;
            c->OW = c->W = (int)(l.OW * m);
            c->OH = c->H = (int)(prow / m);
            c->regrouped = true;
        }
    }
    // other layers with rows shorter than 16 pixels (the 1 x 9 grouped deformable-conv GEMM) keep the f32 kernels
    if (c->OW < 16) return false;
    c->family = WGRAD_LDS;
    c->bi = l.Cout >= 256 ? 4 : (l.Cout >= 128 ? 2 : 1);
    c->bj = l.Cin >= 256 ? 4 : (l.Cin >= 128 ? 2 : 1);
    c->ci_tiles = div_up(l.cin_pad, 64 * c->bj);
    const long long tiles = (long long)div_up(l.Cout, 64 * c->bi) * c->ci_tiles * l.KH * l.KW;
    const int rows = c->N * c->OH;
    const long long per_cu = c->bi * c->bj >= 16 ? 2 : (c->bi * c->bj >= 4 ? 3 : 4);     // resident workgroups (LDS) x ~1.5 rounds
    long long sp = splits_for(per_cu, tiles);
    if (sp > cap) sp = cap;
    if (sp > rows) sp = rows;
    if (sp < 1) sp = 1;
    c->tiles = (int)tiles;
    c->rows_per_split = div_up(rows, sp);
    c->splits = c->slices = div_up(rows, c->rows_per_split);      // the non-empty row ranges
    c->lds_bytes = (size_t)2 * 32 * (64 * c->bi + 64 * c->bj) * 4;      // two stages of 32 pixels x (dy tile + x tile) channels
    return true;
}

}  // namespace

int wgrad_workspace_slices(int N, int OH, int Cout, int Cin, int taps) {
    WgradChoice c{};
    choose_f32(N, OH, Cout, Cin, taps, &c);
    return c.slices;
}

WgradChoice wgrad_choose(const WgradLayer& l) {
    const int taps = l.KH * l.KW;
    WgradChoice caller{};
    caller.N = l.N; caller.OH = l.OH; caller.OW = l.OW; caller.H = l.H; caller.W = l.W;
    WgradChoice c = caller;
    if (choose_lds(l, wgrad_workspace_slices(l.N, l.OH, l.Cout, l.Cin, taps), &c)) return c;
    c = caller;       // the f32 kernels always walk the caller's own rows
    choose_f32(l.N, l.OH, l.Cout, l.Cin, taps, &c);
    c.ci_tiles = div_up(l.cin_pad, 32 * c.bj);
    c.tiles = div_up(l.Cout, 32 * c.bi) * c.ci_tiles * taps;
    c.rows_per_split = div_up(l.N * l.OH, c.splits);
    return c;
}

// The gathered layer: the f32 tile rule over cin_pad; the LIVE row pairs are divided over the splits inside the kernel (device
// count), the host only bounds the splits by the allocated rows: 64 rows per split at least.
WgradChoice gather_wgrad_choose(long long M, int Cout, int Cin, int cin_pad, int taps) {
    WgradChoice c{};
    wgrad_blocks(Cout, Cin, &c.bi, &c.bj);
    c.family = (c.bi == 2 && c.bj == 2) ? WGRAD_TILE64 : WGRAD_WAVE;
    c.ci_tiles = div_up(cin_pad, 32 * c.bj);
    c.tiles = div_up(Cout, 32 * c.bi) * c.ci_tiles * taps;
    c.splits = f32_splits(c.bi, c.bj, c.tiles, (M + 63) / 64);
    c.slices = c.splits * (c.family == WGRAD_TILE64 ? 1 : 4);
    return c;
}

void wgrad_label(const WgradChoice& c, bool gathered, char* out, size_t bytes) {
    char name[64];
    if (c.family == WGRAD_TILE64) snprintf(name, sizeof name, gathered ? "gather_wgrad_kernel" : "conv_wgrad_kernel");
    else snprintf(name, sizeof name, "%s<%d, %d>", gathered ? "gather_wgrad_wide_kernel" : c.family == WGRAD_LDS ? "conv_wgrad_lds_kernel" : "conv_wgrad_wide_kernel", c.bi, c.bj);
    int n = snprintf(out, bytes, "%s grid %d x %d lds %zu reduce %d", name, c.tiles, c.splits, c.lds_bytes, c.slices);
    if (c.regrouped && n > 0 && (size_t)n < bytes)
        snprintf(out + n, bytes - n, " as N=%d OH=%d OW=%d H=%d W=%d", c.N, c.OH, c.OW, c.H, c.W);
}

}  // namespace tt
