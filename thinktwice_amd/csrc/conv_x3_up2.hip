// bf16x3 3 x 3 / stride 1 / pad 1 convolution, Cout = 64, whose input is read THROUGH a bilinear x2 upsampling (align_corners=True):
// `in` is the low-resolution f32 map [N][h][w][Cin], the logical input that map after nn.Upsample(scale_factor=2, bilinear,
// align_corners=True), the output [N][2h][2w][64] (tt_conv_desc.in_up2; UNet.unet_layer0 -> unet_layer0.1 of the camera branch).
// The upsampled tensor -- 4 x the source, one reader -- never reaches global memory, and the nine taps of a channel chunk read one
// staged patch instead of nine DMA'd row tiles.
//
// Same arithmetic as tt_bilinear_up2_pair followed by the pair-format X3 body of conv_igemm_glds.hip, bit for bit: the interpolation
// and the operand split are the two functions of bilinear_up2.h (the split itself: bf16x3.h); the sums run channel chunk outer, taps (kh, kw) ascending inside it,
// two 16-channel k-steps per (chunk, tap), per k-step a_lo*b_hi, a_hi*b_lo, a_hi*b_hi on v_mfma_f32_32x32x16_bf16 into one f32
// accumulator; the epilogue is the shared one.
//
// The tile, the LDS layout, the weight stream and the nine taps are the halo-patch form's (conv_x3_patch.h, two column blocks);
// this file is its production: the workgroup writes the 10 x 34 halo patch of INTERPOLATED pixels into LDS in pair format (128 B per
// pixel: the bytes a pair-format tensor holds for that chunk), each thread up to three (pixel, 8-channel group) items: four source
// vectors from global memory, up2_pair8, two 16 B LDS stores at the swizzled chunk slots.  Patch pixels outside the image are the
// convolution's zero padding: zeroed once, never written again.  What an item needs beside the chunk offset is kept in four
// registers (source offset, the two weights, LDS address with the clamp / inside bits in its low four bits).
// Contract (conv_choose.cpp, choose_up2): f32 contiguous source, Cin % 32 == 0, Cout == 64, vector epilogue, no residuals, no split-K.
#include "bilinear_up2.h"
#include "conv_x3_patch.h"

namespace tt {

namespace up2 {
using namespace patch;
constexpr int ITEMS = PH * PW * 4, ROUNDS = (ITEMS + NT - 1) / NT;     // (pixel, 8-channel group) items of a patch; per thread
constexpr int LDS_BYTES = Lds<2>::BYTES;
static_assert(ROUNDS == 3, "three production rounds per chunk");
}  // namespace up2

__global__ __launch_bounds__(up2::NT, 4) void conv_x3_up2_kernel(const ConvArgs p, const void* zero_page, int tiles, int /*tiles_n*/,
                                                                 int tiles_x, int tiles_y) {
#if defined(__HIP_DEVICE_COMPILE__)
    using namespace up2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x >= tiles) return;
    const Tile tl = tile_of(tiles, tiles_x, tiles_y);
    const int n = tl.n, oy0 = tl.oy0, ox0 = tl.ox0;
    const int OH = p.OH, OW = p.OW, h = OH >> 1, w = OW >> 1, C = p.Cin;

    const float* __restrict__ img = reinterpret_cast<const float*>(p.in) + (long long)n * h * w * C;
    const float* __restrict__ wgt = reinterpret_cast<const float*>(p.weight);
    const float* zp = reinterpret_cast<const float*>(zero_page);
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;

    // ---- production items: item = tid + 512 r -> patch pixel item >> 2 = (py, px), 8-channel group item & 3 of the chunk
    unsigned it_off[ROUNDS];       // byte offset of (y0, x0, group) inside the image, channel chunk 0 (the image base stays scalar)
    unsigned it_dst[ROUNDS];       // byte offset of the hi half in smem | bit 0: x1 != x0, bit 1: y1 != y0, bit 2: inside the image
    float it_ly[ROUNDS], it_lx[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int item = tid + NT * r;
        const bool valid = item < ITEMS;
        const int pix = valid ? item >> 2 : 0, g = item & 3;
        const int py = pix / PW, px = pix - py * PW;
        const int oy = oy0 - 1 + py, ox = ox0 - 1 + px;
        const bool inside = valid && oy >= 0 && oy < OH && ox >= 0 && ox < OW;
        const Up2Tap t = up2_tap(h, w, inside ? oy : 0, inside ? ox : 0);
        it_off[r] = (unsigned)((t.y0 * w + t.x0) * C + g * 8) * 4u;
        it_ly[r] = t.ly;
        it_lx[r] = t.lx;
        // hi half: 16 B chunk 4 (g >> 1) + (g & 1) of the pixel's 128 B (k-step g >> 1, lane half g & 1 of the fragment reads), the lo
        // half two chunks on (address ^ 32)
        const unsigned dst = (unsigned)(py * PW * ROWB) + frag_off<ROWB>(px, 4u * (g >> 1) + (g & 1));
        it_dst[r] = dst | (t.x1 != t.x0 ? 1u : 0u) | (t.y1 != t.y0 ? 2u : 0u) | (inside ? 4u : 0u);
        if (valid && !inside) {                    // zero padding (and the pixels beyond a partial tile's image edge)
            *reinterpret_cast<uint4*>(smem + dst) = make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint4*>(smem + (dst ^ 32u)) = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    const unsigned dxB = (unsigned)C * 4u, dyB = (unsigned)(w * C) * 4u;
    auto produce = [&](int ci) {
        const char* cb = reinterpret_cast<const char*>(img + ci);      // wave-uniform: the loads take it as their scalar base
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            // (the empty asms keep the four addresses from being hoisted out of the chunk loop as 64-bit pointers: 24 registers)
            unsigned d = it_dst[r], o00 = it_off[r];
            asm volatile("" : "+v"(d), "+v"(o00));
            if (d & 4u) {
                const unsigned o01 = o00 + ((d & 1u) ? dxB : 0u);
                const unsigned o10 = o00 + ((d & 2u) ? dyB : 0u), o11 = o10 + ((d & 1u) ? dxB : 0u);
                uint4 hi, lo;
                up2_pair8(reinterpret_cast<const float*>(cb + o00), reinterpret_cast<const float*>(cb + o01),
                          reinterpret_cast<const float*>(cb + o10), reinterpret_cast<const float*>(cb + o11), it_ly[r], it_lx[r], hi, lo);
                *reinterpret_cast<uint4*>(smem + (d & ~15u)) = hi;
                *reinterpret_cast<uint4*>(smem + ((d & ~15u) ^ 32u)) = lo;
            }
        }
    };

    f32x16 acc[1][2];
    zero_acc(acc);
    patch_k_loop<2, 1>(p, wgt, zp, lds_base, wave, lane, C, acc, produce);
    patch_epilogue<2>(p, acc, smem, wave, lane, tl);
#endif
}

// c.family = CONV_X3_UP2.  a.H / a.W are the logical (upsampled) input size = the output size; a.weight = the pre-split weights.
// 1, or < 0 on failure.
int launch_conv_x3_up2(const ConvChoice& c, ConvArgs& a, hipStream_t st) {
    (void)c;
    const int tiles_x = div_up(a.OW, up2::TW), tiles_y = div_up(a.OH, up2::TH);
    const long long tiles = (long long)a.N * tiles_x * tiles_y;
    TT_REQUIRE(tiles < (1ll << 31), "tt_conv2d_fwd: in_up2 layer of %lld tiles", tiles);
    return launch_lds_dma(conv_x3_up2_kernel, dim3((unsigned)tiles), dim3(up2::NT), (size_t)up2::LDS_BYTES, (size_t)up2::LDS_BYTES,
                          "conv_x3_up2_kernel", a, st, (int)tiles, 1, 1, tiles_x, tiles_y);
}

}  // namespace tt
