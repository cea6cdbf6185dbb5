// bf16x3 3 x 3 / stride 1 / pad 1 / dilation 1 "same" convolution over a PAIR-FORMAT input (tt_conv_desc.in_pair), Cout = 64 (two
// column blocks) or 8 .. 32 (one): the halo-patch form of conv_x3_patch.h with the patch produced by LDS-DMA.
//
// The per-tap tiles of conv_igemm_glds.hip send every input pixel from L2 to LDS nine times, once per tap (the seg head: 14.8 GB for
// a 1.64 GB tensor).  Here the 128 bytes a pair-format tensor holds for (pixel, 32-channel chunk) ARE the patch row the taps read, so
// a chunk's 10 x 34 patch is 43 DMA pieces of eight consecutive patch pixels (wave w issues pieces w, w + 8, ...), the patch-column
// swizzle applied on the source address, pixels outside the image (and the four pixels that pad the patch to whole pieces) from the
// zero page.  No interpolation, no VALU split; every pixel crosses L2 -> LDS 340 / 256 = 1.33 times.
// The patch is single-buffered like conv_x3_up2.hip's: a chunk's pieces are issued behind the barrier that ends the previous chunk's
// taps and waited for (vmcnt 0) at tap 0; two workgroups per CU cover each other's waits.
// Same sums as the tiles it replaces (conv_x3_patch.h), bit for bit; padding contributes exact zeros in both forms.
// Contract (conv_choose.cpp, choose_x3_patch): in_pair, Cin % 32 == 0, in_coff / in_cstride multiples of 16, an image of less than
// 2^30 elements, vector epilogue, f32 or out_pair output; no residual, out2, per-image shift, split-K, pixel shuffle, gather, m_dev.
#include "conv_x3_patch.h"

namespace tt {

template <int NCB>
__global__ __launch_bounds__(patch::NT, 4) void conv_x3_patch_kernel(const ConvArgs p, const void* zero_page, int tiles, int /*tiles_n*/,
                                                                     int tiles_x, int tiles_y) {
#if defined(__HIP_DEVICE_COMPILE__)
    using namespace patch;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x >= tiles) return;
    const Tile tl = tile_of(tiles, tiles_x, tiles_y);
    const int H = p.H, W = p.W, C = p.Cin;

    const float* __restrict__ img = reinterpret_cast<const float*>(p.in) + (long long)tl.n * p.in_nstride + p.in_coff;
    const float* __restrict__ wgt = reinterpret_cast<const float*>(p.weight);
    const float* zp = reinterpret_cast<const float*>(zero_page);
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);

    // ---- production: piece q = wave + 8 r covers patch pixels 8 q .. 8 q + 7 (row-major over the 10 x 34 patch); lane l brings the
    // 16 B that land at chunk slot l & 7 of pixel 8 q + (l >> 3): source chunk (l & 7) ^ swz(patch column)
    constexpr int ROUNDS = (PIECES + NW - 1) / NW;      // 6; the last round has pieces for waves 0 .. 2 only
    constexpr unsigned OUTSIDE = ~0u;
    unsigned src[ROUNDS];          // byte offset of the lane's 16 B inside the image window, channel chunk 0; OUTSIDE: the zero page
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int lin = (wave + NW * r) * 8 + (lane >> 3);
        const int py = lin / PW, px = lin - py * PW;
        const int iy = tl.oy0 - 1 + py, ix = tl.ox0 - 1 + px;
        const bool inside = lin < PH * PW && iy >= 0 && iy < H && ix >= 0 && ix < W;
        const int chunk = (lane & 7) ^ swz<ROWB>(px);
        src[r] = inside ? ((unsigned)((iy * W + ix) * p.in_cstride) + (unsigned)chunk * 4u) * 4u : OUTSIDE;
    }
    auto produce = [&](int ci) {
        const char* cb = reinterpret_cast<const char*>(img + ci);      // wave-uniform
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int q = wave_s + NW * r;
            if (NW * (r + 1) <= PIECES || q < PIECES)
                dma_piece(src[r] != OUTSIDE ? reinterpret_cast<const float*>(cb + src[r]) : zp, lds_base + (unsigned)q * 1024u);
        }
    };

    f32x16 acc[1][NCB];
    zero_acc(acc);
    patch_k_loop<NCB, 0>(p, wgt, zp, lds_base, wave, lane, C, acc, produce);
    patch_epilogue<NCB>(p, acc, smem, wave, lane, tl);
#endif
}

template <int NCB>
static int launch_patch(ConvArgs& a, hipStream_t st, int tiles, int tiles_x, int tiles_y) {
    constexpr size_t lds = (size_t)patch::Lds<NCB>::BYTES;
    return launch_lds_dma(conv_x3_patch_kernel<NCB>, dim3((unsigned)tiles), dim3(patch::NT), lds, lds, "conv_x3_patch_kernel", a, st, tiles,
                          1, 1, tiles_x, tiles_y);
}

// c.family = CONV_X3_PATCH, c.bn = 64 / 32: two / one column blocks.  a.weight = the pre-split weights.  1, or < 0 on failure.
int launch_conv_x3_patch(const ConvChoice& c, ConvArgs& a, hipStream_t st) {
    const int tiles_x = div_up(a.OW, patch::TW), tiles_y = div_up(a.OH, patch::TH);
    const long long tiles = (long long)a.N * tiles_x * tiles_y;
    TT_REQUIRE(tiles < (1ll << 31), "tt_conv2d_fwd: patch-form layer of %lld tiles", tiles);
    TT_REQUIRE(c.bn == 64 || c.bn == 32, "tt_conv2d_fwd: no conv_x3_patch_kernel for a %d-wide tile", c.bn);
    return c.bn == 64 ? launch_patch<2>(a, st, (int)tiles, tiles_x, tiles_y) : launch_patch<1>(a, st, (int)tiles, tiles_x, tiles_y);
}

}  // namespace tt
