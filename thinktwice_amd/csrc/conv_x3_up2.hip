// bf16x3 3 x 3 / stride 1 / pad 1 convolution, Cout = 64, whose input is read THROUGH a bilinear x2 upsampling (align_corners=True):
// `in` is the low-resolution f32 map [N][h][w][Cin], the logical input that map after nn.Upsample(scale_factor=2, bilinear,
// align_corners=True), the output [N][2h][2w][64] (tt_conv_desc.in_up2; UNet.unet_layer0 -> unet_layer0.1 of the camera branch).
// The upsampled tensor -- 4 x the source, one reader -- never reaches global memory, and the nine taps of a channel chunk read one
// staged patch instead of nine DMA'd row tiles.
//
// Same arithmetic as tt_bilinear_up2_pair followed by the pair-format X3 body of conv_igemm_glds.hip, bit for bit: the interpolation
// and the operand split are the two functions of bilinear_up2.h; the sums run channel chunk outer, taps (kh, kw) ascending inside it,
// two 16-channel k-steps per (chunk, tap), per k-step a_lo*b_hi, a_hi*b_lo, a_hi*b_hi on v_mfma_f32_32x32x16_bf16 into one f32
// accumulator; the epilogue is the shared one.
//
// A workgroup of eight waves owns 8 rows x 32 columns of output pixels of ONE image; wave r owns output row r (32 pixels x 64
// channels: two 32 x 32 accumulator blocks).  Per 32-channel chunk:
//   * production: the workgroup writes the 10 x 34 halo patch of INTERPOLATED pixels into LDS in pair format (128 B per pixel:
//     the bytes a pair-format tensor holds for that chunk), each thread up to three (pixel, 8-channel group) items: four source
//     vectors from global memory, up2_pair8, two 16 B LDS stores at the swizzled chunk slots.  Patch pixels outside the image are the
//     convolution's zero padding: zeroed once, never written again.  What an item needs beside the chunk offset is kept in four
//     registers (source offset, the two weights, LDS address with the clamp / inside bits in its low four bits).
//   * the nine taps read their activation fragments from that patch at per-lane addresses: pixel (r + kh, x + kw).  The swizzle is
//     taken from the patch COLUMN (frag_off of the column, + row * 34 * 128): a tap shift in kh then is a constant ds_read offset and
//     the six (kw, k-step) addresses of a lane serve all nine taps.
//   * weights stream per (chunk, tap) through LDS-DMA, 8 KiB per tap (one 1 KiB piece per wave), three-slot ring, two taps ahead;
//     one counted vmcnt + barrier per tap.
// The patch is single-buffered (a barrier in front of every production): with 68 KiB of LDS two workgroups share a CU and one's
// production runs beside the other's MFMAs.
// Contract (conv_choose.cpp, choose_up2): f32 contiguous source, Cin % 32 == 0, Cout == 64, vector epilogue, no residuals, no split-K.
#include "bilinear_up2.h"
#include "conv_lds_dma.h"

namespace tt {

namespace up2 {
constexpr int TH = 8, TW = 32;                    // output pixels of a tile
constexpr int PH = TH + 2, PW = TW + 2;           // the halo patch
constexpr int ROWB = 128, BK = 32;                // bytes / channels of a patch pixel = one channel chunk
constexpr int NT = 512, NW = 8;
constexpr int ITEMS = PH * PW * 4, ROUNDS = (ITEMS + NT - 1) / NT;     // (pixel, 8-channel group) items of a patch; per thread
constexpr int PATCH_BYTES = PH * PW * ROWB;       // 43,520
constexpr int W_BYTES = 64 * ROWB, W_SLOTS = 3;   // 8 KiB per tap, three slots
constexpr int W_OFF = PATCH_BYTES;
constexpr int LOOP_BYTES = PATCH_BYTES + W_SLOTS * W_BYTES;            // 68,096
constexpr int EPI_BYTES = NW * 32 * (64 + 4) * 4;                      // conv_epilogue's staging: 69,632
constexpr int LDS_BYTES = LOOP_BYTES > EPI_BYTES ? LOOP_BYTES : EPI_BYTES;
static_assert(ROUNDS == 3, "three production rounds per chunk");
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU: one's patch production runs beside the other's MFMAs");
static_assert(2 * PW * ROWB < 65536 && W_SLOTS * W_BYTES < 65536, "tap and ring-slot shifts are ds_read offsets (16 bits)");
}  // namespace up2

// ds_read_b128 with a compile-time byte offset (inline asm for the reason conv_lds_dma.h gives for lds_read)
template <int OFF>
__device__ __forceinline__ u32x4 lds_read_at(unsigned addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}

__global__ __launch_bounds__(up2::NT, 4) void conv_x3_up2_kernel(const ConvArgs p, const void* zero_page, int tiles, int /*tiles_n*/,
                                                                 int tiles_x, int tiles_y) {
#if defined(__HIP_DEVICE_COMPILE__)
    using namespace up2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x >= tiles) return;
    const int L = xcd_tile(tiles);                 // consecutive tiles (neighbours in x: shared halo, shared source rows) on one XCD
    const int tpi = tiles_x * tiles_y;
    const int n = L / tpi, trem = L - n * tpi;
    const int tile_y = trem / tiles_x, tile_x = trem - tile_y * tiles_x;
    const int oy0 = tile_y * TH, ox0 = tile_x * TW;
    const int OH = p.OH, OW = p.OW, h = OH >> 1, w = OW >> 1, C = p.Cin;

    const float* __restrict__ img = reinterpret_cast<const float*>(p.in) + (long long)n * h * w * C;
    const float* __restrict__ wgt = reinterpret_cast<const float*>(p.weight);
    const float* zp = reinterpret_cast<const float*>(zero_page);
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);

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

    // ---- weight stream: tile kt = (chunk, tap), 64 rows x 128 B; this wave's piece = rows 8 wave .. + 7
    const float* b_ptr;
    {
        const int g = wave * 64 + lane;
        const int row = g >> 3, pos = g & 7;
        b_ptr = wgt + (long long)row * p.K + (pos ^ swz<ROWB>(row)) * 4;
    }
    const int nch = C / BK, nk = nch * 9;
    int w_kt = 0, w_tap = 0;                       // walker of the next tile to issue (wave-uniform)
    long long w_off = 0;
    auto issue_w = [&](int slot) {
        dma_piece(w_kt < nk ? b_ptr + w_off : zp, lds_base + (unsigned)(W_OFF + slot * W_BYTES) + (unsigned)wave_s * 1024u);
        ++w_kt;
        if (++w_tap == 9) {
            w_tap = 0;
            w_off += BK - 8ll * C;
        } else {
            w_off += C;
        }
    };

    // ---- fragment addresses.  A: patch pixel (wave + kh, x + kw), x = lane & 31; lane half hf owns channels 8 hf .. + 7 of the
    // k-step: hi chunk 4 kc + hf, lo chunk ^ 2.  B: weight row j * 32 + (lane & 31) of the tap's 64, same chunks.
    // Held per lane: the k-step-0 hi address of each kw, and of the weight row lane & 31.  The swizzle being an XOR, the lo half is
    // the address ^ 32 and k-step 1 the address ^ 64; weight rows 32 .. 63 (the second column block) have the swizzle of rows 0 .. 31
    // and lie 4 KiB on: an offset.
    const unsigned hf = lane >> 5;
    unsigned fa[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) fa[kw] = lds_base + (unsigned)(wave * PW * ROWB) + frag_off<ROWB>((lane & 31) + kw, hf);
    const unsigned fb = lds_base + (unsigned)W_OFF + frag_off<ROWB>(lane & 31, hf);

    f32x16 acc[1][2];
    zero_acc(acc);

    issue_w(0);
    issue_w(1);
    auto mfma_k = [&](const u32x4& ah, const u32x4& al, const u32x4 (&bh)[2], const u32x4 (&bl)[2]) {
        const uint4 ahv = __builtin_bit_cast(uint4, ah), alv = __builtin_bit_cast(uint4, al);
        // term-major: consecutive MFMAs write different accumulators; per accumulator the order is lo*hi, hi*lo, hi*hi
#pragma unroll
        for (int j = 0; j < 2; ++j) Mfma<uint16_t>::run(alv, __builtin_bit_cast(uint4, bh[j]), acc[0][j]);
#pragma unroll
        for (int j = 0; j < 2; ++j) Mfma<uint16_t>::run(ahv, __builtin_bit_cast(uint4, bl[j]), acc[0][j]);
#pragma unroll
        for (int j = 0; j < 2; ++j) Mfma<uint16_t>::run(ahv, __builtin_bit_cast(uint4, bh[j]), acc[0][j]);
    };
    // One filter tap t = 3 kh + kw of the current chunk; kh, kw and the ring slot t % 3 are compile-time (kh and the slot are
    // ds_read offsets).
    auto tap = [&](auto t_c) {
        constexpr int t = decltype(t_c)::value;
        constexpr int kh = t / 3, kw = t % 3, slot = t % 3;
        constexpr int OA = kh * PW * ROWB, OB = slot * W_BYTES;
        // this tap's weights have landed for this wave once only the next tap's piece is outstanding (the production's loads are
        // consumed); the barrier publishes them -- and, at tap 0, the patch -- and frees the ring slot of tap t - 1
        wait_vmcnt<1>();
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        issue_w((t + 2) % 3);
        u32x4 ah[2], al[2], bh[2][2], bl[2][2];
        auto read_k = [&](int kc) {
            const unsigned a = fa[kw] ^ (kc ? 64u : 0u), b = fb ^ (kc ? 64u : 0u);
            ah[kc] = lds_read_at<OA>(a);
            al[kc] = lds_read_at<OA>(a ^ 32u);
            bh[kc][0] = lds_read_at<OB>(b);
            bl[kc][0] = lds_read_at<OB>(b ^ 32u);
            bh[kc][1] = lds_read_at<OB + 32 * ROWB>(b);
            bl[kc][1] = lds_read_at<OB + 32 * ROWB>(b ^ 32u);
        };
        // the wait ties to the registers the MFMAs read: no MFMA can be scheduled above it
        auto landed = [&](int kc) {
            asm volatile("" : "+v"(ah[kc]), "+v"(al[kc]), "+v"(bh[kc][0]), "+v"(bl[kc][0]), "+v"(bh[kc][1]), "+v"(bl[kc][1]));
        };
        read_k(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        read_k(1);                 // in flight under the first k-step's MFMAs
        landed(0);
        mfma_k(ah[0], al[0], bh[0], bl[0]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        landed(1);
        mfma_k(ah[1], al[1], bh[1], bl[1]);
    };
    for (int c = 0; c < nch; ++c) {
        // every wave is done with the previous chunk's patch (c = 0: nothing to wait for; the zero fill above is published by the
        // barrier of tap 0, like the production)
        if (c > 0) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        produce(c * BK);
        tap(std::integral_constant<int, 0>{});
        tap(std::integral_constant<int, 1>{});
        tap(std::integral_constant<int, 2>{});
        tap(std::integral_constant<int, 3>{});
        tap(std::integral_constant<int, 4>{});
        tap(std::integral_constant<int, 5>{});
        tap(std::integral_constant<int, 6>{});
        tap(std::integral_constant<int, 7>{});
        tap(std::integral_constant<int, 8>{});
    }
    wait_vmcnt<0>();               // the two zero-page pieces issued beyond the last tap: landed before the epilogue reuses LDS
    // wave r's 32 pixels are consecutive output rows of the GEMM: the shared epilogue takes them as one 32 x 64 block whose row limit
    // is the end of the image row (a partial tile's columns beyond it, and its rows beyond the image, store nothing)
    const int oy = oy0 + wave;
    const bool row_ok = oy < OH;
    const int m0 = row_ok ? (n * OH + oy) * OW + ox0 : 0;
    const int mlim = row_ok ? (n * OH + oy) * OW + (ox0 + TW < OW ? ox0 + TW : OW) : 0;
    conv_epilogue<float, 1, 2, 32, 64>(p, acc, smem, wave, lane, 0, 0, m0, 0, mlim);
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
