// A ResNet bottleneck's conv3 and the NEXT block's conv1 as ONE launch over a row tile (tt_conv2d_fwd_next; label conv_x3_join_kernel):
//
//   x = act1(s1 * (W1 . y) + b1 + res1)    1 x 1, K1 -> 4 K1, f32 output (written: the next block's identity / downsample read it)
//   z = act2(s2 * (W2 . x) + b2)           1 x 1, 4 K1 -> N2, pair-format output (tt_conv_desc.out_pair: the next block's 3 x 3 reads it)
//
// As two tt_conv2d_fwd launches the second one reads all of x back (1.64 GB per layer-1 block at B = 8) to produce a tensor four or
// eight times narrower.  Here a WAVE owns 32 rows from the load of y to the store of z:
//   * y (K1 channels, pair format or f32 split once on load) stays in the wave's registers as stage 1's A fragments;
//   * stage 1 is computed one 32-column block of x at a time.  The block goes through the wave's private 4.5 KiB of LDS exactly as
//     in the convolutions' vector epilogue (affine applied in the MFMA C layout, then whole 128-byte row segments: residual, ReLU,
//     non-temporal store) -- and the finished values are written back to the same LDS words, from where the wave reads them in the
//     MFMA A layout, splits them (bf16x3.h) and multiplies them into stage 2's accumulators, which stay live over the whole walk;
//   * per column block the workgroup streams one weight tile through a two-slot LDS-DMA ring: the 32 rows of W1 (K1 wide) and the
//     32-wide K slice of all N2 rows of W2, in the 128-byte-row sub-tile layout and swizzle of conv_lds_dma.h.  One barrier per block.
// Nothing is shared between workgroups.
//
// Both outputs are, bit for bit, those of the two launches: per accumulator k ascends in 16-wide steps with the three products in the
// one-accumulator order of bf16x3.h (stage 2's k order is stage 1's column order: the blocks are walked in ascending order), and the
// epilogue expressions are conv_common.h's.  The entry (conv_choose.cpp, choose_join) refuses every case in which either stage alone
// would run on a kernel with other sums.
//
// LDS accesses of the loop are inline asm (conv_lds_dma.h: the compiler would put `s_waitcnt vmcnt(0)` in front of each one while
// LDS-DMA is in flight, which here would also drain the output stores).  vmcnt discipline: per block a wave issues its DMA pieces
// FIRST and its four output stores LAST, so `vmcnt(4)` at the next block's top has the pieces (and the residual reads) landed while
// the stores stay in flight; a wave whose 32 rows are not all inside M predicates its stores and waits for vmcnt(0) instead.
#include <utility>

#include "conv_lds_dma.h"

namespace tt {
namespace {

__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void pin(u32x4& v) { asm volatile("" : "+v"(v)); }
template <int OFF>
__device__ __forceinline__ void lds_write_f32_at(unsigned addr, float v) {
    asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_write4_at(unsigned addr, const u32x4& v) {
    asm volatile("ds_write_b128 %0, %1 offset:%2\n\ts_nop 1" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}

constexpr int kJoinCB = 32;                    // columns of x per block = K elements of a stage-2 step pair
constexpr int kJoinLdc = kJoinCB + 4;          // LDS row stride (floats) of the wave's block: the conv epilogue's WTN + 4
constexpr int kJoinBlockBytes = 32 * kJoinLdc * 4;

// the affine in the C layout (lane = column, register r = row (r & 3) + 8 (r >> 2) + 4 half): stage_scaled's expression
template <int... R>
__device__ __forceinline__ void stage_block(unsigned addr, const f32x16& acc, float sc, float sh, std::integer_sequence<int, R...>) {
    (lds_write_f32_at<((R & 3) + 8 * (R >> 2)) * kJoinLdc * 4>(addr, acc[R] * sc + sh), ...);
}

}  // namespace

template <int K1, int N2, int NW>
__global__ __launch_bounds__(NW * 64, NW / 4) void conv_x3_join_kernel(const ConvArgs p, const void* /*zero_page*/, int /*tiles_m*/,
                                                                       int /*tiles_n*/, const ConvArgs p2) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int CB = kJoinCB, LDC = kJoinLdc;
    constexpr int K2 = 4 * K1, NCB = K2 / CB, KS1 = K1 / 16, NJ = N2 / 32;
    constexpr int P1 = K1 / 8, P2 = N2 / 8;           // 1 KiB pieces of a block's W1 rows / W2 slice
    constexpr int PPW = (P1 + P2) / NW;               // pieces per wave
    constexpr int TILE = (P1 + P2) * 1024;
    static_assert((P1 + P2) % NW == 0 && K1 % 32 == 0 && (N2 == 64 || N2 == 128 || N2 == 256), "whole pieces per wave, whole 128-byte sub-tiles, column block pairs");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, half = lane >> 5;        // MFMA operand layout: lane = (row or column, 16 B half of a k-step)
    const int Mlim = p.M;
    const int m0 = (int)blockIdx.x * (32 * NW);
    const int mb = m0 + wave * 32;
    const bool full = mb + 32 <= Mlim;                // wave-uniform
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned blk = lds_base + 2u * TILE + (unsigned)wave * kJoinBlockBytes;

    // ---- stage 1's A operand: the wave's 32 rows of y, in registers for the whole walk
    uint4 ah[KS1], al[KS1];
    {
        const int m = mb + r;                          // rows beyond M read row M - 1: their sums are never stored
        const float* row = reinterpret_cast<const float*>(p.in) + (long long)(m < Mlim ? m : Mlim - 1) * p.in_cstride + p.in_coff;
        if (p.flags & 32) {      // pair format: hi chunk `half`, lo chunk `half` + 2 of each 64-byte group
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) {
                ah[ks] = *reinterpret_cast<const uint4*>(row + ks * 16 + half * 4);
                al[ks] = *reinterpret_cast<const uint4*>(row + ks * 16 + 8 + half * 4);
            }
        } else {                 // f32: lane half h owns floats 8h .. 8h + 7 of the 16-wide k-step
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) {
                const uint4 r0 = *reinterpret_cast<const uint4*>(row + ks * 16 + half * 8);
                const uint4 r1 = *reinterpret_cast<const uint4*>(row + ks * 16 + half * 8 + 4);
                split8(r0, r1, ah[ks], al[ks]);
            }
        }
    }

    // ---- DMA slots: piece q = wave + NW j of a block's tile.  q < P1: 8 rows x 128 B of W1 sub-tile q / 4 (rows = the block's 32
    // columns, sub-tile t = K elements 32 t .. 32 t + 31); else 8 rows x 128 B of the W2 slice (rows = stage 2's columns, K elements =
    // the block's 32 columns).  Lane l brings the 16 B that land at chunk slot l & 7 of its row: source chunk (l & 7) ^ swz(row).
    const float* dsrc[PPW];
    int dstep[PPW];              // elements from one block's piece to the next block's
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int q = wave + NW * j;
        if (q < P1) {
            const int g = q * 64 + lane, t = g >> 8, row = (g & 255) >> 3, pos = g & 7;
            dsrc[j] = reinterpret_cast<const float*>(p.weight) + (long long)row * K1 + t * 32 + ((pos ^ swz<128>(row)) << 2);
            dstep[j] = CB * K1;
        } else {
            const int g = (q - P1) * 64 + lane, row = g >> 3, pos = g & 7;
            dsrc[j] = reinterpret_cast<const float*>(p2.weight) + (long long)row * K2 + ((pos ^ swz<128>(row)) << 2);
            dstep[j] = CB;
        }
    }
    auto issue_tile = [&](int cb) {
        const unsigned st = lds_base + (unsigned)(cb & 1) * TILE;
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            dma_piece(dsrc[j], st + (unsigned)(wave + NW * j) * 1024u);
            dsrc[j] += dstep[j];
        }
    };

    // ---- stage 1's epilogue geometry: a row of the block is 8 chunks of 16 B, the 64 lanes cover 8 rows per pass, 4 passes
    const int prow = lane >> 3, pcol = (lane & 7) * 4;
    const unsigned pass_addr = blk + (unsigned)(prow * LDC + pcol) * 4u;
    const unsigned stage_addr = blk + (unsigned)(4 * half * LDC + r) * 4u;
    const unsigned a_addr = blk + (unsigned)(r * LDC + half * 8) * 4u;
    const bool has_res = p.res1 != nullptr, relu1 = p.act == TT_ACT_RELU;
    // wave-uniform addresses of the wave's first row, per-lane element offsets of the four passes (loads of rows beyond M read row M - 1)
    float* const obase = reinterpret_cast<float*>(p.out) + (long long)mb * p.out_cstride + p.out_coff;
    const float* const rbase = has_res ? reinterpret_cast<const float*>(p.res1) + (long long)mb * p.res1_cstride + p.res1_coff : nullptr;
    int ooff[4], roff[4];
    bool row_ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int m = mb + q * 8 + prow;
        row_ok[q] = m < Mlim;
        const int dr = (row_ok[q] ? m : Mlim - 1) - mb;
        ooff[q] = dr * p.out_cstride + pcol;
        roff[q] = dr * p.res1_cstride + pcol;
    }
    // residual and folded-BN affine of ONE block: loaded a block ahead, behind the adds that read the previous values
    float4 res[4];
    float sc = 1.f, sh = 0.f;
    auto load_epi = [&](int cb) {
        sc = p.scale ? p.scale[cb * CB + r] : 1.f;
        sh = p.shift ? p.shift[cb * CB + r] : 0.f;
        if (has_res) {
#pragma unroll
            for (int q = 0; q < 4; ++q) res[q] = *reinterpret_cast<const float4*>(rbase + roff[q] + cb * CB);
        }
    };

    // fragment offsets inside a 32-row x 128-byte sub-tile: k-step parity 0 / 1, hi chunk; the lo chunk is ^ 32.  Rows 32 j + r of
    // the W2 slice have the swizzle of row r, so one pair serves every sub-tile of both operands
    const unsigned fo[2] = {frag_off<128>(r, (unsigned)half), frag_off<128>(r, 4u + (unsigned)half)};

    f32x16 acc2[N2 / 64][1][2];
#pragma unroll
    for (int g = 0; g < N2 / 64; ++g) zero_acc(acc2[g]);

    typedef float f4v __attribute__((ext_vector_type(4)));
    issue_tile(0);
    asm volatile("" ::: "memory");
    load_epi(0);
    // the A fragments are used here, in front of the loop: left to their first MFMA, the compiler's wait for them sits inside the loop
    // as vmcnt(0) and drains every block's stores
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
        asm volatile("" ::"v"(ah[ks].x), "v"(al[ks].x));
    }
#pragma unroll 1
    for (int cb = 0; cb < NCB; ++cb) {
        // the block's tile has landed for this wave; its output stores of the previous block may still be in flight
        if (cb > 0 && full) wait_vmcnt<4>();
        else wait_vmcnt<0>();
        asm volatile("s_barrier" ::: "memory");       // publishes tile cb; every wave is done reading tile cb - 1
        if (cb + 1 < NCB) issue_tile(cb + 1);
        asm volatile("" ::: "memory");
        const unsigned w1 = lds_base + (unsigned)(cb & 1) * TILE, w2 = w1 + P1 * 1024u;

        // ---- stage 1: one 32 x 32 block of x, K1 / 16 k-steps on the resident A fragments
        f32x16 acc1;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc1[e] = 0.f;
        u32x4 bh[2], bl[2];
        bh[0] = lds_read(w1 + fo[0]);
        bl[0] = lds_read(w1 + (fo[0] ^ 32u));
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            const int b = ks & 1;
            lds_wait();
            pin(bh[b]);
            pin(bl[b]);
            if (ks + 1 < KS1) {
                const unsigned o = (unsigned)((ks + 1) >> 1) * 4096u + fo[(ks + 1) & 1];
                bh[b ^ 1] = lds_read(w1 + o);
                bl[b ^ 1] = lds_read(w1 + (o ^ 32u));
            }
            mfma3(ah[ks], al[ks], __builtin_bit_cast(uint4, bh[b]), __builtin_bit_cast(uint4, bl[b]), acc1);
        }

        // ---- its epilogue: affine in the C layout -> LDS -> row segments: residual, ReLU, store; the values go back to LDS
        stage_block(stage_addr, acc1, sc, sh, std::make_integer_sequence<int, 16>{});
        u32x4 t[4];
        t[0] = lds_read_at<0 * 8 * LDC * 4>(pass_addr);
        t[1] = lds_read_at<1 * 8 * LDC * 4>(pass_addr);
        t[2] = lds_read_at<2 * 8 * LDC * 4>(pass_addr);
        t[3] = lds_read_at<3 * 8 * LDC * 4>(pass_addr);
        lds_wait();
#pragma unroll
        for (int q = 0; q < 4; ++q) pin(t[q]);
        f4v v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float x[4] = {__uint_as_float(t[q].x), __uint_as_float(t[q].y), __uint_as_float(t[q].z), __uint_as_float(t[q].w)};
            if (has_res) {
                x[0] += res[q].x; x[1] += res[q].y; x[2] += res[q].z; x[3] += res[q].w;
            }
            if (relu1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = x[e] > 0.f ? x[e] : 0.f;
            }
            v[q] = f4v{x[0], x[1], x[2], x[3]};
        }
        lds_write4_at<0 * 8 * LDC * 4>(pass_addr, __builtin_bit_cast(u32x4, v[0]));
        lds_write4_at<1 * 8 * LDC * 4>(pass_addr, __builtin_bit_cast(u32x4, v[1]));
        lds_write4_at<2 * 8 * LDC * 4>(pass_addr, __builtin_bit_cast(u32x4, v[2]));
        lds_write4_at<3 * 8 * LDC * 4>(pass_addr, __builtin_bit_cast(u32x4, v[3]));
        // stage 2's A fragments: row r, floats 8 half .. 8 half + 7 of the two 16-wide k-steps (the LDS executes a wave's accesses in
        // order), and its first weight pair
        u32x4 xa[2][2];
        xa[0][0] = lds_read_at<0>(a_addr);
        xa[0][1] = lds_read_at<16>(a_addr);
        xa[1][0] = lds_read_at<64>(a_addr);
        xa[1][1] = lds_read_at<80>(a_addr);
        bh[0] = lds_read(w2 + fo[0]);
        bl[0] = lds_read(w2 + (fo[0] ^ 32u));
        // the next block's residual and affine travel under this block's stores and stage 2 (the adds above have released the registers)
        if (cb + 1 < NCB) load_epi(cb + 1);
        asm volatile("" ::: "memory");
        // the four output stores: the wave's last vector-memory operations of the block (see the head comment)
        if (full) {
#pragma unroll
            for (int q = 0; q < 4; ++q) __builtin_nontemporal_store(v[q], reinterpret_cast<f4v*>(obase + ooff[q] + cb * CB));
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (row_ok[q]) __builtin_nontemporal_store(v[q], reinterpret_cast<f4v*>(obase + ooff[q] + cb * CB));
        }
        asm volatile("" ::: "memory");

        // ---- stage 2: the block is K elements 32 cb .. 32 cb + 31 = two k-steps over every column block; per accumulator the
        // one-accumulator order of bf16x3.h
        uint4 xh[2], xl[2];
        constexpr int NS = 2 * NJ;                    // sub-steps: (k-step, column block)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ks = s / NJ, j = s % NJ, b = s & 1;
            lds_wait();
            pin(bh[b]);
            pin(bl[b]);
            if (s == 0) {
                pin(xa[0][0]); pin(xa[0][1]); pin(xa[1][0]); pin(xa[1][1]);
                split8(xa[0][0], xa[0][1], xh[0], xl[0]);
                split8(xa[1][0], xa[1][1], xh[1], xl[1]);
            }
            if (s + 1 < NS) {
                const unsigned o = (unsigned)((s + 1) % NJ) * 4096u + fo[(s + 1) / NJ];
                bh[b ^ 1] = lds_read(w2 + o);
                bl[b ^ 1] = lds_read(w2 + (o ^ 32u));
            }
            mfma3(xh[ks], xl[ks], __builtin_bit_cast(uint4, bh[b]), __builtin_bit_cast(uint4, bl[b]), acc2[j >> 1][0][j & 1]);
        }
    }

    // ---- stage 2's epilogue: the convolutions' own (pair-format stores), 64 columns at a time through 8.5 KiB per wave
    __syncthreads();                                  // every wave is done with the ring and its block
    float* sC = reinterpret_cast<float*>(smem) + (tid >> 6) * (32 * (64 + 4));
    // (spelled out: left to the unroller, the 256-wide form kept its accumulators in scratch)
    auto epi2 = [&](auto g) { conv_epilogue_vec<float, 8, 1, 2, 32, 64, false>(p2, acc2[decltype(g)::value], sC, lane, tid >> 6, decltype(g)::value, m0, 0, Mlim); };
    epi2(std::integral_constant<int, 0>{});
    if constexpr (N2 >= 128) epi2(std::integral_constant<int, 1>{});
    if constexpr (N2 >= 256) {
        epi2(std::integral_constant<int, 2>{});
        epi2(std::integral_constant<int, 3>{});
    }
#endif
}

template <int K1, int N2, int NW>
static int launch_join(ConvArgs& a, const ConvArgs& a2, hipStream_t st) {
    constexpr size_t ring = 2 * (size_t)(K1 / 8 + N2 / 8) * 1024 + (size_t)NW * kJoinBlockBytes;
    constexpr size_t epi = (size_t)NW * 32 * (64 + 4) * 4;
    constexpr size_t lds = ring > epi ? ring : epi;
    const int tiles_m = div_up(a.M, 32 * NW);
    return launch_lds_dma(conv_x3_join_kernel<K1, N2, NW>, dim3((unsigned)tiles_m), dim3(NW * 64), lds, lds, "conv_x3_join_kernel", a, st,
                          tiles_m, 1, 1, a2);
}

// c.family = CONV_X3_JOIN, c.bn = N2, c.waves_m = waves per workgroup.  a / a2: the two stages (a.weight, a2.weight = their pre-split
// weights).  1, or < 0 on failure; never another kernel.
int launch_conv_x3_join(const ConvChoice& c, ConvArgs& a, const ConvArgs& a2, hipStream_t st) {
    const int k1 = a.Cin, n2 = a2.Cout, nw = c.waves_m;
    if (k1 == 64 && n2 == 64 && nw == 8) return launch_join<64, 64, 8>(a, a2, st);
    if (k1 == 64 && n2 == 128 && nw == 8) return launch_join<64, 128, 8>(a, a2, st);
    if (k1 == 128 && n2 == 128 && nw == 8) return launch_join<128, 128, 8>(a, a2, st);
    if (k1 == 128 && n2 == 256 && nw == 4) return launch_join<128, 256, 4>(a, a2, st);
    if (k1 == 256 && n2 == 256 && nw == 4) return launch_join<256, 256, 4>(a, a2, st);
    TT_REQUIRE(false, "tt_conv2d_fwd: no conv_x3_join_kernel<%d, %d, %d>", k1, n2, nw);
}

}  // namespace tt
