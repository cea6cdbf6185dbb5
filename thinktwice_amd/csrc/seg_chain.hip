// seg_res_to_image_feature.0 / .3 (backbones/lss.py:409-416: 1 x 1, n_class -> 64, BN, ReLU; 1 x 1, 64 -> 16, BN, ReLU) as ONE
// launch over the rows of the full-resolution segmentation map:
//
//   y = act1(s1 * (W1 . x) + b1)   16 (zero-padded K1) -> 64
//   z = act2(s2 * (W2 . y) + b2)   64 -> N2
//
// As two tt_conv2d_fwd launches the 64-channel map y is written to HBM and read back (1.64 GB each way at B = 8) around 1,792
// MACs per row.  Here a WAVE owns 32 rows from the load of x to the store of z: y goes through the wave's private 8.5 KiB of LDS
// (the MFMA C layout has a lane own a column, the A layout a row), so the kernel has no barrier, no cross-wave traffic and moves
// K1 + N2 floats per row.  Both weight matrices stay in registers over a wave's whole grid-stride walk.
//
// The result is, bit for bit, that of the two launches: per stage the MFMAs, their K order and the epilogue expressions are those
// of the kernel conv_choose picks for that layer at this row count (tt_seg_feedback_chain asks it):
//   SMALL  (R <= 4096)   conv_small_kernel on both: exact f32, K steps of 8 dealt over four partial sums added ((p0 + p1) + p2) + p3
//   F32    (R < 65536)   conv_igemm_kernel<float> on both: exact f32, one chain over K
//   X3     (else)        conv_igemm_kernel<float> on stage 1, the 256 x 32 bf16x3 tile of conv_igemm_glds.hip on stage 2: y split
//                        into bf16 (hi, lo) and multiplied in the one-accumulator order of bf16x3.h, per 16-wide k-step
#include "conv_common.h"

namespace tt {
namespace {

enum { CHAIN_SMALL = 0, CHAIN_F32 = 1, CHAIN_X3 = 2 };

constexpr int kN1 = 64;          // width of the intermediate
constexpr int kLd1 = kN1 + 4;    // LDS row strides (floats) of the y and z blocks: the conv epilogue's WTN + 4
constexpr int kLd2 = 32 + 4;

struct SegChainArgs {
    const float* x;
    const float* w1; const float* scale1; const float* shift1;
    const float* w2; const void* w2_x3; const float* scale2; const float* shift2;
    float* out;
    long long R;
    int x_stride, K1, N2, act1, act2, out_stride, out_coff, nblocks;
};

// the wave's LDS traffic so far has completed, and the compiler moves no memory access across (the block is wave-private: the LDS
// executes a wave's operations in order, so this is all the synchronisation the lane-to-lane hand-over needs)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ float act01(float v, int act) { return act == TT_ACT_RELU ? (v > 0.f ? v : 0.f) : v; }

__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

template <int MODE>
__global__ __launch_bounds__(256) void seg_chain_kernel(const SegChainArgs p) {
    __shared__ __attribute__((aligned(16))) float smem[4 * 32 * kLd1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = lane & 31, half = lane >> 5;      // MFMA operand layout: lane = (row or column, 16 B half of a K step of 8)
    float* sC = smem + wave * 32 * kLd1;
    const uint4 zero4 = make_uint4(0, 0, 0, 0);

    // ---- both weight matrices and the folded-BN affines, in registers for the whole walk
    uint4 b1[2][2];                                   // [column block][K step of 8]
    float sc1[2], sh1[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = j * 32 + row;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int k = s * 8 + half * 4;
            b1[j][s] = k < p.K1 ? *reinterpret_cast<const uint4*>(p.w1 + col * p.K1 + k) : zero4;
        }
        sc1[j] = p.scale1 ? p.scale1[col] : 1.f;
        sh1[j] = p.shift1 ? p.shift1[col] : 0.f;
    }
    const bool col_ok = row < p.N2;
    uint4 b2[8];                                      // X3: [k-step] hi, [4 + k-step] lo; else [K step of 8]
    if constexpr (MODE == CHAIN_X3) {
        // pair format: per 16 K elements 64 B = [hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15]
        const uint4* wr = reinterpret_cast<const uint4*>(p.w2_x3) + row * (kN1 / 4);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            b2[ks] = col_ok ? wr[ks * 4 + half] : zero4;
            b2[4 + ks] = col_ok ? wr[ks * 4 + 2 + half] : zero4;
        }
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s)
            b2[s] = col_ok ? *reinterpret_cast<const uint4*>(p.w2 + row * kN1 + s * 8 + half * 4) : zero4;
    }
    const float sc2 = (col_ok && p.scale2) ? p.scale2[row] : 1.f;
    const float sh2 = (col_ok && p.shift2) ? p.shift2[row] : 0.f;

    // output pass geometry: a row of N2 floats is N2 / 4 16-byte chunks, the 64 lanes cover 64 / (N2 / 4) rows per pass
    const int cpr = p.N2 >> 2, rpp = 64 / cpr, npass = 32 / rpp;
    const int o_row = lane / cpr, o_col = (lane % cpr) * 4;

    auto load_x = [&](int blk, uint4 (&xa)[2]) {
        const long long m = (long long)blk * 32 + row;
        const bool ok = blk < p.nblocks && m < p.R;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int k = s * 8 + half * 4;
            xa[s] = (ok && k < p.K1) ? *reinterpret_cast<const uint4*>(p.x + m * p.x_stride + k) : zero4;
        }
    };

    const int stride = gridDim.x * 4;
    int blk = blockIdx.x * 4 + wave;
    uint4 xa[2], xn[2];
    load_x(blk, xa);
    for (; blk < p.nblocks; blk += stride) {
        load_x(blk + stride, xn);                     // the next block's rows travel under this block's arithmetic

        // ---- stage 1: exact f32, v_mfma_f32_32x32x2_f32 in steps of 8 K elements
        f32x16 acc1[2];
        if constexpr (MODE == CHAIN_SMALL) {
            // conv_small_kernel: wave w of its workgroup owns K steps w, w + 4, ...; K1 <= 16 is steps 0 and 1, the other two partial
            // sums are zeros
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x16 p0, p1;
                zero16(p0);
                zero16(p1);
                Mfma<float>::run(xa[0], b1[j][0], p0);
                Mfma<float>::run(xa[1], b1[j][1], p1);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc1[j][r] = p0[r] + p1[r] + 0.f + 0.f;
            }
        } else {
            zero16(acc1[0]);
            zero16(acc1[1]);
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 2; ++j) Mfma<float>::run(xa[s], b1[j][s], acc1[j]);
        }
        wave_lds_sync();                              // the previous block's z reads are done
        // C layout: lane = column, register r = row (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                sC[((r & 3) + 8 * (r >> 2) + 4 * half) * kLd1 + j * 32 + row] = act01(acc1[j][r] * sc1[j] + sh1[j], p.act1);
        wave_lds_sync();

        // ---- stage 2
        f32x16 acc2;
        const float* ya = sC + row * kLd1 + half * 4;
        if constexpr (MODE == CHAIN_X3) {
            zero16(acc2);
            uint4 r0[4], r1[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {          // lane half h owns floats 8h .. 8h + 7 of the 16-wide k-step
                r0[ks] = *reinterpret_cast<const uint4*>(ya + ks * 16 + half * 4);
                r1[ks] = *reinterpret_cast<const uint4*>(ya + ks * 16 + half * 4 + 4);
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                uint4 ah, al;
                split8(r0[ks], r1[ks], ah, al);
                mfma3(ah, al, b2[ks], b2[4 + ks], acc2);
            }
        } else {
            uint4 a[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) a[s] = *reinterpret_cast<const uint4*>(ya + s * 8);
            if constexpr (MODE == CHAIN_SMALL) {
                f32x16 pw[4];
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    zero16(pw[w]);
                    Mfma<float>::run(a[w], b2[w], pw[w]);
                    Mfma<float>::run(a[w + 4], b2[w + 4], pw[w]);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[r] = pw[0][r] + pw[1][r] + pw[2][r] + pw[3][r];
            } else {
                zero16(acc2);
#pragma unroll
                for (int s = 0; s < 8; ++s) Mfma<float>::run(a[s], b2[s], acc2);
            }
        }
        wave_lds_sync();                              // y has been read: its LDS block takes z
#pragma unroll
        for (int r = 0; r < 16; ++r) sC[((r & 3) + 8 * (r >> 2) + 4 * half) * kLd2 + row] = acc2[r] * sc2 + sh2;
        wave_lds_sync();
        // one 16-byte store per lane and pass: whole rows of z, written once and read by a later launch (non-temporal, as the
        // convolutions' f32 outputs)
        typedef float f4v __attribute__((ext_vector_type(4)));
        for (int ps = 0; ps < npass; ++ps) {
            const int rl = ps * rpp + o_row;
            const long long m = (long long)blk * 32 + rl;
            if (m >= p.R) continue;
            const float4 t = *reinterpret_cast<const float4*>(sC + rl * kLd2 + o_col);
            const f4v v = {act01(t.x, p.act2), act01(t.y, p.act2), act01(t.z, p.act2), act01(t.w, p.act2)};
            __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(p.out + m * p.out_stride + p.out_coff + o_col));
        }
        xa[0] = xn[0];
        xa[1] = xn[1];
    }
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// The kernel family tt_conv2d_fwd runs one stage of the chain on, as a 1 x 1 convolution over R rows: CHAIN_SMALL / CHAIN_F32 /
// CHAIN_X3, or -1 with the error text set for anything else (a dispatch rule this file does not know).
int stage_mode(long long R, int K, int N, const void* w_x3) {
    ConvArgs a{};
    a.N = 1; a.H = 1; a.W = 1; a.OH = 1; a.OW = 1;
    a.KH = a.KW = a.stride = a.dil = 1;
    a.Cin = K; a.in_cstride = K; a.Cout = N; a.out_cstride = N;
    a.M = (int)R; a.K = K;
    a.in_nstride = K; a.out_nstride = N;
    a.shift_n_mod = 1;
    a.out_dtype = TT_F32;
    a.out_fast = a.vec_epi = a.res_vec = 1;
    a.flags = 16;
    ConvFacts f{};
    f.dtype = TT_F32;
    f.weight_x3 = (K % 16 == 0) ? w_x3 : nullptr;
    ConvChoice c;
    if (conv_choose(a, f, &c)) return -1;
    if (c.splits > 1) { set_error("tt_seg_feedback_chain: a split-K stage (K=%d N=%d) has no chain form", K, N); return -1; }
    if (c.family == CONV_SMALL) return CHAIN_SMALL;
    if (c.family == CONV_IGEMM && !c.x3) return CHAIN_F32;
    if (c.family == CONV_GLDS && c.x3 && !c.apair && c.bn == 32 && c.bkb == 128) return CHAIN_X3;
    set_error("tt_seg_feedback_chain: the convolution dispatch runs the %d -> %d stage over %lld rows on a kernel the chain does not "
              "reproduce", K, N, R);
    return -1;
}

}  // namespace
}  // namespace tt

using namespace tt;

extern "C" int tt_seg_feedback_chain(const float* x, long long R, int x_stride, int K1, const float* w1, const float* scale1,
                                     const float* shift1, int act1, const float* w2, const void* w2_x3, int N2,
                                     const float* scale2, const float* shift2, int act2, float* out, int out_stride,
                                     int out_coff, void* stream) {
    TT_REQUIRE(x && w1 && w2 && w2_x3 && out, "tt_seg_feedback_chain: null pointer");
    TT_REQUIRE(R > 0 && R <= 0x7fffffffll - 64, "tt_seg_feedback_chain: bad row count %lld", R);
    TT_REQUIRE(K1 == 16 || K1 == 12, "tt_seg_feedback_chain: K1 = %d (16, or 12 read as 16 with zeros; the intermediate is 64 wide)", K1);
    TT_REQUIRE(N2 == 8 || N2 == 16 || N2 == 32, "tt_seg_feedback_chain: N2 = %d (8, 16 or 32)", N2);
    TT_REQUIRE(x_stride >= K1 && x_stride % 4 == 0 && out_stride % 4 == 0 && out_coff % 4 == 0 && out_coff >= 0 &&
                   out_coff + N2 <= out_stride,
               "tt_seg_feedback_chain: x_stride=%d out_stride=%d out_coff=%d must be multiples of 4 that hold the K1=%d / N2=%d "
               "channels", x_stride, out_stride, out_coff, K1, N2);
    TT_REQUIRE(aligned16(x) && aligned16(w1) && aligned16(w2) && aligned16(w2_x3) && aligned16(out),
               "tt_seg_feedback_chain: x / w1 / w2 / w2_x3 / out must be 16-byte aligned");
    TT_REQUIRE((act1 == TT_ACT_NONE || act1 == TT_ACT_RELU) && (act2 == TT_ACT_NONE || act2 == TT_ACT_RELU),
               "tt_seg_feedback_chain: activations are none or ReLU (got %d, %d)", act1, act2);
    // the arithmetic of each stage is the one its tt_conv2d_fwd launch would use at this row count
    const int m1 = stage_mode(R, K1, kN1, nullptr), m2 = stage_mode(R, kN1, N2, w2_x3);
    if (m1 < 0 || m2 < 0) return -1;
    TT_REQUIRE((m1 == CHAIN_SMALL) == (m2 == CHAIN_SMALL) && m1 != CHAIN_X3,
               "tt_seg_feedback_chain: stage kernels %d / %d over %lld rows have no chain form", m1, m2, R);
    SegChainArgs a{x, w1, scale1, shift1, w2, w2_x3, scale2, shift2, out, R, x_stride, K1, N2, act1, act2, out_stride, out_coff,
                   div_up(R, 32)};
    // three workgroups of four waves per CU (the kernel's registers allow three waves per SIMD); a wave walks its 32-row blocks
    // with the grid's stride
    int grid = div_up(a.nblocks, 4);
    if (grid > kNumCU * 3) grid = kNumCU * 3;
    hipStream_t st = (hipStream_t)stream;
    if (m2 == CHAIN_SMALL) hipLaunchKernelGGL(seg_chain_kernel<CHAIN_SMALL>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else if (m2 == CHAIN_F32) hipLaunchKernelGGL(seg_chain_kernel<CHAIN_F32>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(seg_chain_kernel<CHAIN_X3>, dim3((unsigned)grid), dim3(256), 0, st, a);
    return check_launch("tt_seg_feedback_chain");
}
