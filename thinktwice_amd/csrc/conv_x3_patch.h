// The halo-patch form of the bf16x3 3 x 3 / stride 1 / pad 1 convolution: what conv_x3_up2.hip (patch interpolated from a low-resolution
// f32 map) and conv_x3_patch.hip (patch DMA'd from a pair-format tensor) share, stated once.  A kernel of the form consists of its
// patch production; the tile, the LDS layout, the weight stream, the fragment addresses, the nine taps and the epilogue call are here.
//
// A workgroup of eight waves owns 8 rows x 32 columns of output pixels of ONE image; wave r owns output row r (32 pixels x 32 NCB
// channels: NCB 32 x 32 accumulator blocks).  Per 32-channel chunk:
//   * production (the kernel's): the 10 x 34 halo patch of input pixels in LDS, pair format, 128 B per pixel = the bytes a pair-format
//     tensor holds for (pixel, chunk): 16 B chunk c of patch pixel (py, px) at (py * 34 + px) * 128 + ((c ^ swz(px)) << 4).  Patch
//     pixels outside the image are the convolution's zero padding.
//   * the nine taps read their activation fragments from that patch at per-lane addresses: pixel (r + kh, x + kw).  The swizzle is
//     taken from the patch COLUMN (frag_off of the column, + row * 34 * 128): a tap shift in kh then is a constant ds_read offset and
//     the six (kw, k-step) addresses of a lane serve all nine taps.
//   * weights stream per (chunk, tap) through LDS-DMA, 32 NCB rows x 128 B per tap (one 1 KiB piece per wave, the first 4 NCB waves),
//     three-slot ring, two taps ahead; one counted vmcnt + barrier per tap.  Weight rows at or beyond Cout read the zero page.
// The patch is single-buffered (a barrier in front of every production): two workgroups share a CU and one's production runs beside
// the other's MFMAs.
// Sums: channel chunk outer, taps (kh, kw) ascending inside it, two 16-channel k-steps per (chunk, tap), per k-step a_lo*b_hi,
// a_hi*b_lo, a_hi*b_hi on v_mfma_f32_32x32x16_bf16 into one f32 accumulator (bf16x3.h) -- the order of the pair-format X3 body of
// conv_igemm_glds.hip, bit for bit.
#pragma once
#include "conv_lds_dma.h"

namespace tt {

namespace patch {
constexpr int TH = 8, TW = 32;                    // output pixels of a tile
constexpr int PH = TH + 2, PW = TW + 2;           // the halo patch
constexpr int ROWB = 128, BK = 32;                // bytes / channels of a patch pixel = one channel chunk
constexpr int NT = 512, NW = 8;
constexpr int PIECES = (PH * PW * ROWB + 1023) / 1024;                 // 1 KiB DMA pieces of eight consecutive patch pixels: 43
constexpr int PATCH_BYTES = PIECES * 1024;        // 44,032: the patch padded to whole pieces
constexpr int W_SLOTS = 3, W_OFF = PATCH_BYTES;
template <int NCB>
struct Lds {
    static constexpr int W_BYTES = 32 * NCB * ROWB;                    // a tap's weights: 4 / 8 KiB
    static constexpr int LOOP_BYTES = PATCH_BYTES + W_SLOTS * W_BYTES; // 56,320 / 68,608
    static constexpr int EPI_BYTES = NW * 32 * (32 * NCB + 4) * 4;     // conv_epilogue's staging: 36,864 / 69,632
    static constexpr int BYTES = LOOP_BYTES > EPI_BYTES ? LOOP_BYTES : EPI_BYTES;
    static_assert(2 * BYTES <= 160 * 1024, "two workgroups per CU: one's patch production runs beside the other's MFMAs");
    static_assert(2 * PW * ROWB < 65536 && W_SLOTS * W_BYTES < 65536, "tap and ring-slot shifts are ds_read offsets (16 bits)");
};

// The tile of this workgroup: image n, first output pixel (oy0, ox0).  Consecutive tiles (neighbours in x: shared halo, shared source
// rows) run on one XCD.
struct Tile {
    int n, oy0, ox0;
};
__device__ __forceinline__ Tile tile_of(int tiles, int tiles_x, int tiles_y) {
    const int L = xcd_tile(tiles);
    const int tpi = tiles_x * tiles_y;
    const int n = L / tpi, trem = L - n * tpi;
    const int tile_y = trem / tiles_x, tile_x = trem - tile_y * tiles_x;
    return Tile{n, tile_y * TH, tile_x * TW};
}
}  // namespace patch

// The K loop of a tile: for every chunk, produce(first channel of the chunk) and the nine taps.  `wgt`: the pre-split weights
// [Cout][9 C]; `C` = Cin.  TAP0_VM: the loads of this wave that may still be in flight when tap 0 of a chunk reads the patch -- 1 (the
// next tap's weight piece) where the production has consumed its own loads, 0 where the production IS loads (LDS-DMA pieces, issued
// behind the two weight pieces in flight).  Returns with nothing outstanding: the epilogue may reuse LDS.
template <int NCB, int TAP0_VM, typename Produce>
__device__ __forceinline__ void patch_k_loop(const ConvArgs& p, const float* __restrict__ wgt, const float* zp, unsigned lds_base, int wave,
                                             int lane, int C, f32x16 (&acc)[1][NCB], Produce produce) {
    using namespace patch;
    constexpr int W_BYTES = Lds<NCB>::W_BYTES;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);

    // ---- weight stream: tile kt = (chunk, tap), 32 NCB rows x 128 B; this wave's piece = rows 8 wave .. + 7
    const float* b_ptr;
    bool b_ok;
    {
        const int g = wave * 64 + lane;
        const int row = g >> 3, pos = g & 7;
        b_ptr = wgt + (long long)row * p.K + (pos ^ swz<ROWB>(row)) * 4;
        b_ok = NCB == 2 || row < p.Cout;           // (two column blocks: Cout == 64)
    }
    const int nch = C / BK, nk = nch * 9;
    int w_kt = 0, w_tap = 0;                       // walker of the next tile to issue (wave-uniform)
    long long w_off = 0;
    auto issue_w = [&](int slot) {
        if (NCB == 2 || wave_s < 4 * NCB)
            dma_piece((w_kt < nk && b_ok) ? b_ptr + w_off : zp, lds_base + (unsigned)(W_OFF + slot * W_BYTES) + (unsigned)wave_s * 1024u);
        ++w_kt;
        if (++w_tap == 9) {
            w_tap = 0;
            w_off += BK - 8ll * C;
        } else {
            w_off += C;
        }
    };

    // ---- fragment addresses.  A: patch pixel (wave + kh, x + kw), x = lane & 31; lane half hf owns channels 8 hf .. + 7 of the
    // k-step: hi chunk 4 kc + hf, lo chunk ^ 2.  B: weight row j * 32 + (lane & 31) of the tap's 32 NCB, same chunks.
    // Held per lane: the k-step-0 hi address of each kw, and of the weight row lane & 31.  The swizzle being an XOR, the lo half is
    // the address ^ 32 and k-step 1 the address ^ 64; weight rows 32 .. 63 (the second column block) have the swizzle of rows 0 .. 31
    // and lie 4 KiB on: an offset.
    const unsigned hf = lane >> 5;
    unsigned fa[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) fa[kw] = lds_base + (unsigned)(wave * PW * ROWB) + frag_off<ROWB>((lane & 31) + kw, hf);
    const unsigned fb = lds_base + (unsigned)W_OFF + frag_off<ROWB>(lane & 31, hf);

    issue_w(0);
    issue_w(1);
    auto mfma_k = [&](const u32x4& ah, const u32x4& al, const u32x4 (&bh)[NCB], const u32x4 (&bl)[NCB]) {
        const uint4 ahv = __builtin_bit_cast(uint4, ah), alv = __builtin_bit_cast(uint4, al);
        // term-major: consecutive MFMAs write different accumulators; per accumulator the one-accumulator order of bf16x3.h
#pragma unroll
        for (int j = 0; j < NCB; ++j) Mfma<uint16_t>::run(alv, __builtin_bit_cast(uint4, bh[j]), acc[0][j]);
#pragma unroll
        for (int j = 0; j < NCB; ++j) Mfma<uint16_t>::run(ahv, __builtin_bit_cast(uint4, bl[j]), acc[0][j]);
#pragma unroll
        for (int j = 0; j < NCB; ++j) Mfma<uint16_t>::run(ahv, __builtin_bit_cast(uint4, bh[j]), acc[0][j]);
    };
    // One filter tap t = 3 kh + kw of the current chunk; kh, kw and the ring slot t % 3 are compile-time (kh and the slot are
    // ds_read offsets).
    auto tap = [&](auto t_c) {
        constexpr int t = decltype(t_c)::value;
        constexpr int kh = t / 3, kw = t % 3, slot = t % 3;
        constexpr int OA = kh * PW * ROWB, OB = slot * W_BYTES;
        // this tap's weights have landed for this wave once only the next tap's piece is outstanding (tap 0: TAP0_VM); the barrier
        // publishes them -- and, at tap 0, the patch -- and frees the ring slot of tap t - 1
        wait_vmcnt<t == 0 ? TAP0_VM : 1>();
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        issue_w((t + 2) % 3);
        u32x4 ah[2], al[2], bh[2][NCB], bl[2][NCB];
        auto read_k = [&](int kc) {
            const unsigned a = fa[kw] ^ (kc ? 64u : 0u), b = fb ^ (kc ? 64u : 0u);
            ah[kc] = lds_read_at<OA>(a);
            al[kc] = lds_read_at<OA>(a ^ 32u);
            bh[kc][0] = lds_read_at<OB>(b);
            bl[kc][0] = lds_read_at<OB>(b ^ 32u);
            if constexpr (NCB == 2) {
                bh[kc][1] = lds_read_at<OB + 32 * ROWB>(b);
                bl[kc][1] = lds_read_at<OB + 32 * ROWB>(b ^ 32u);
            }
        };
        // the wait ties to the registers the MFMAs read: no MFMA can be scheduled above it
        auto landed = [&](int kc) {
            if constexpr (NCB == 2)
                asm volatile("" : "+v"(ah[kc]), "+v"(al[kc]), "+v"(bh[kc][0]), "+v"(bl[kc][0]), "+v"(bh[kc][1]), "+v"(bl[kc][1]));
            else
                asm volatile("" : "+v"(ah[kc]), "+v"(al[kc]), "+v"(bh[kc][0]), "+v"(bl[kc][0]));
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
        // every wave is done with the previous chunk's patch (c = 0: nothing to wait for; what the kernel wrote into the patch before
        // the loop is published by the barrier of tap 0, like the production)
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
}

// wave r's 32 pixels are consecutive output rows of the GEMM: the shared epilogue takes them as one 32 x 32 NCB block whose row limit
// is the end of the image row (a partial tile's columns beyond it, and its rows beyond the image, store nothing; so do the columns at
// or beyond Cout)
template <int NCB>
__device__ __forceinline__ void patch_epilogue(const ConvArgs& p, f32x16 (&acc)[1][NCB], unsigned char* smem, int wave, int lane,
                                               const patch::Tile& t) {
    const int oy = t.oy0 + wave;
    const bool row_ok = oy < p.OH;
    const int m0 = row_ok ? (t.n * p.OH + oy) * p.OW + t.ox0 : 0;
    const int mlim = row_ok ? (t.n * p.OH + oy) * p.OW + (t.ox0 + patch::TW < p.OW ? t.ox0 + patch::TW : p.OW) : 0;
    conv_epilogue<float, 1, NCB, 32, 32 * NCB>(p, acc, smem, wave, lane, 0, 0, m0, 0, mlim);
}

}  // namespace tt
