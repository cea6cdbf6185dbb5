// Sparse 3-D convolution (3x3x3 rulebook, bf16x3 arithmetic) for the 16- and 32-channel levels: WEIGHT-RESIDENT gather kernel.
//
// At Cin <= 32 a row has one to six neighbours of 64 / 128 B each: the layer is a gather and an HBM problem, not MFMA work, and the
// 256-row tile pipeline of sp_conv_runs.hip spends its time on structure the result does not need (per tile a rulebook DMA, a range
// reduction, nine or more stages that each restage the stage's weights from L2 and end in vmcnt(0) + a barrier, an epilogue nothing
// overlaps: profiles/r03_sparse_runs_ablation.txt).  Here
//   * the pair-format weights of one 32-column output tile -- 27 taps x 32 couts x Cin, hi and lo: 110.6 KB at Cin = 32 -- are
//     DMA'd into LDS ONCE per workgroup and stay there for the whole launch (one vmcnt(0) + one barrier, the only ones);
//   * the launch is persistent, one workgroup of eight waves per CU, and the 32-row groups are dealt statically: a wave owns groups
//     first + k * stride up to the live count it read once.  No queue, no atomics, no flag: nothing can wait on another workgroup,
//     and after the prologue barrier nothing waits on another wave;
//   * per group a lane reads its row's 27 rulebook entries (lanes l and l + 32 hold the same row, lane >> 5 is the K half) and, tap
//     by tap in ascending order, loads its 8-float K half of the neighbour row straight from global memory into registers (lanes
//     without a neighbour read the zero page), two taps ahead of the MFMAs; a tap no row of the wave has is skipped (wave-uniform ballot);
//   * the epilogue is the shared vector epilogue on the wave's own LDS slab (behind the weight block, never aliasing it).
// Bounded by the gathered bytes (pairs x Cin x 4 B through L2) beside ~27 x Cin / 16 x 3 MFMAs per group; the weight stream is gone.
//
// Arithmetic: exactly sp_conv_runs.hip's -- operands split into bf16 hi + lo in registers (pack_bf16x2, residual exact in f32),
// al*bh + ah*bl + ah*bh on v_mfma_f32_32x32x16_bf16 into one f32 accumulator, taps ascending, k-steps ascending.  On a cell-ordered
// SubM rulebook with Cin = 32 the run-staged kernel adds a row's non-zero products in this same sequence and everything else it
// adds is an exact zero: the two kernels are bit-identical there (tests/test_sp_conv_l2.py).
#include "conv_lds_dma.h"

namespace tt {

namespace {
constexpr int kL2Taps = 27;
constexpr int kL2Waves = 8;
constexpr int kL2Slab = 32 * (32 + 4) * 4;      // a wave's epilogue slab: 32 rows x (32 + 4) f32
}  // namespace

template <int CIN>
__global__ __launch_bounds__(kL2Waves * 64, 1) void sp_conv_runs_l2_kernel(const ConvArgs p, const float* __restrict__ zp) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int KS = CIN / 16;                    // k-steps of 16 channels per tap
    constexpr int ROWB = CIN * 4;                   // bytes of one (cout, tap) weight row in pair format
    constexpr int WB = kL2Taps * 32 * ROWB;         // the resident weight block
    constexpr int NP = WB / 1024;                   // its 1 KiB DMA pieces
    constexpr int RPP = 1024 / ROWB, CPR = ROWB / 16;
    static_assert(CIN == 16 || CIN == 32, "one or two k-steps");
    static_assert(WB % 1024 == 0, "whole DMA pieces");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const int n0 = (int)blockIdx.y * 32;
    int Mlim = p.M;
    if (p.m_dev) {
        const int md = *p.m_dev;
        Mlim = md < Mlim ? md : Mlim;
    }
    // ---- the static deal over the LIVE 32-row groups: round robin over all waves of the launch.  (An XCD-contiguous deal -- every
    // XCD walking one contiguous eighth of the groups -- measured the same on the layer and on the step, profiles/sp_conv_l2.txt:
    // one deal is kept.)
    const int ngroups = (Mlim + 31) >> 5;
    int first = (int)blockIdx.x * kL2Waves;
    const int end = ngroups, stride = (int)gridDim.x * kL2Waves;
    if (first >= end) return;                       // workgroup-uniform: no wave of this workgroup has a group
    first += wave_s;

    const float* __restrict__ in = reinterpret_cast<const float*>(p.in) + p.in_coff;
    const float* __restrict__ wgt = reinterpret_cast<const float*>(p.weight);

    // ---- prologue: the column tile's weights, [tap][cout 0..31][ROWB] with the chunk swizzle of conv_lds_dma.h applied to the
    // DMA source.  Couts beyond Cout (Cout = 16) re-read the last row: their columns are never stored.
    {
        const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
        const int d_row = lane / CPR, d_pos = lane % CPR;
        for (int i = wave_s; i < NP; i += kL2Waves) {
            const int r = i * RPP + d_row;          // r = tap * 32 + n
            const int t = r >> 5, n = r & 31;
            const int nn = n0 + n < p.Cout ? n0 + n : p.Cout - 1;
            dma_piece(wgt + (long long)nn * p.K + t * CIN + ((d_pos ^ swz<ROWB>(n)) << 2), lds_base + (unsigned)i * 1024u);
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);             // vmcnt(0): this wave's pieces have landed
    __syncthreads();                                // ... and everyone's.  The last barrier of the kernel.

    float* const sC = reinterpret_cast<float*>(smem + WB + wave * kL2Slab);
    const unsigned kb = lane >> 5;                  // K half of this lane's MFMA operands
    unsigned boff[KS];                              // byte offset of this lane's hi fragment of k-step ks inside a tap's block
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) boff[ks] = frag_off<ROWB>(lane & 31, 4u * ks + kb);
    constexpr unsigned LO = kPairLo;                // chunk ^ 2: the lo half of a pair-format fragment (bf16x3.h)

    // Every load of the main loop is UNCONDITIONAL -- a lane without work reads a harmless address and drops the value: a load inside
    // a divergent branch may or may not have been issued, so the compiler must assume it was not and waits for the newest loads
    // (vmcnt(3) .. (0) in front of every tap), which drains the prefetch.
    // Rulebook entries of this lane's row of group g.  Rows at or beyond the live count hold garbage: such a lane reads the last live
    // row (Mlim >= 1 here) and takes "no neighbour".
    auto load_ent = [&](int g, int (&e)[kL2Taps]) {
        const int m = g * 32 + (lane & 31);
        const bool live = g < end && m < Mlim;
        const int* __restrict__ rb = p.gather + (long long)(live ? m : Mlim - 1) * kL2Taps;
#pragma unroll
        for (int t = 0; t < kL2Taps; ++t) e[t] = rb[t];
#pragma unroll
        for (int t = 0; t < kL2Taps; ++t) e[t] = live ? e[t] : -1;
    };
    // this lane's K half (8 floats per k-step) of neighbour row `ent`; without a neighbour: of the zero page
    auto load_a = [&](int ent, float4 (&a)[KS][2]) {
        const float* __restrict__ row = ent >= 0 ? in + (long long)ent * p.in_cstride : zp;
        const float4* __restrict__ s = reinterpret_cast<const float4*>(row) + 2 * kb;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            a[ks][0] = s[4 * ks];
            a[ks][1] = s[4 * ks + 1];
        }
    };

    int e[kL2Taps];
    load_ent(first, e);
    for (int g = first; g < end; g += stride) {
        f32x16 acc[1][1];
        zero_acc(acc);
        float4 a[3][KS][2];                         // taps t, t + 1, t + 2 in flight
        load_a(e[0], a[0]);
        load_a(e[1], a[1]);
        int en[kL2Taps];                            // the next group's entries land under this group's taps
        load_ent(g + stride, en);
#pragma unroll
        for (int t = 0; t < kL2Taps; ++t) {
            if (t + 2 < kL2Taps) load_a(e[t + 2], a[(t + 2) % 3]);
            if (__builtin_amdgcn_ballot_w64(e[t] >= 0) == 0ull) continue;      // no row of this wave has the tap
            const unsigned char* wt = smem + t * (32 * ROWB);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint4 bh = *reinterpret_cast<const uint4*>(wt + boff[ks]);
                const uint4 bl = *reinterpret_cast<const uint4*>(wt + (boff[ks] ^ LO));
                uint4 ah, al;
                split8(a[t % 3][ks][0], a[t % 3][ks][1], ah, al);
                mfma3(ah, al, bh, bl, acc[0][0]);
            }
        }
        // the wave's own slab: neighbouring waves are mid-loop, nothing here synchronises with them
        if (p.act != 99)                            // (99: profiling aid, main loop only -- as conv_epilogue)
            conv_epilogue_vec<float, 4, 1, 1, 32, 32, true>(p, acc, sC, lane, 0, 0, g * 32, n0, Mlim);
#pragma unroll
        for (int t = 0; t < kL2Taps; ++t) e[t] = en[t];
    }
#endif
}

template <int CIN>
static int launch_l2(ConvArgs& a, hipStream_t st) {
    constexpr size_t smem = (size_t)kL2Taps * 32 * CIN * 4 + (size_t)kL2Waves * kL2Slab;      // 147,456 B at Cin = 32
    static_assert(smem <= 160 * 1024, "the CU's LDS");
    auto kern = sp_conv_runs_l2_kernel<CIN>;
    const void* zp = zero_page("sp_conv_runs_l2_kernel");      // 256 B of zeros: what a lane without a neighbour loads
    if (!zp || lds_opt_in(reinterpret_cast<const void*>(kern), smem, "sp_conv_runs_l2_kernel")) return -1;
    // persistent: one workgroup per CU over all column tiles, never more workgroups than 256-row blocks of the allocation
    const int ncol = div_up(a.Cout, 32);
    int gx = div_up(a.M, kL2Waves * 32);
    if (gx > kNumCU / ncol) gx = kNumCU / ncol;
    a.tiles_n = ncol;
    a.splits = 1;
    a.ws = nullptr;
    a.m_begin = 0;
    hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)ncol), dim3(kL2Waves * 64), smem, st, a, reinterpret_cast<const float*>(zp));
    return 1;
}

// `a.weight` = pre-split pair-format weights [Cout][27][Cin].  1, or < 0 on failure.
int launch_sp_conv_l2(const ConvChoice& c, ConvArgs& a, hipStream_t st) {
    if (a.Cin == 32 && c.bkb == 128) return launch_l2<32>(a, st);
    if (a.Cin == 16 && c.bkb == 64) return launch_l2<16>(a, st);
    TT_REQUIRE(false, "tt_conv2d_fwd: no sp_conv_runs_l2_kernel for Cin = %d", a.Cin);
}

}  // namespace tt
