// The ResNet stem of the bf16x3 modes as ONE launch from the NCHW image to the max-pooled map (tt_stem_pool_x3; label
// conv_x3_stem_pool_kernel):
//
//   out = max_pool2d(relu(scale * conv7x7s2p3(img) + shift), 3, 2, 1)       f32 (NI, ceil(H / 4), ceil(W / 4), 64), channel-last
//
// As three launches (tt_nchw_to_nhwc_border into a zero-bordered 4-channel copy, the row-run stem convolution, tt_maxpool3x3s2) the
// full-resolution 64-channel stem map is written once and read once (2 x 1.64 GB at 64 images of 448 x 896) and the bordered copy
// likewise (2 x 0.42 GB); the network needs 0.31 GB in and 0.41 GB out.  Here a workgroup owns a 7 x 8 tile of POOLED pixels of one
// image and everything under it:
//   * the 35 x 40 input pixels below the tile's 15 x 17 stem pixels are read from the three NCHW planes by plain row loads (zero
//     outside the image: the border the copy holds physically), split ONCE per pixel into the bf16 (hi, lo) pair of bf16x3.h and kept
//     in LDS as 8-byte (R, G, B, 0) pixels per half, so an A fragment of the row-run form -- pixels 2h, 2h + 1 of a half filter row
//     times 4 channels -- is one aligned 16-byte read per half and the K loop holds no VALU split;
//   * the 255 stem pixels are 8 row blocks of 32: a wave owns two of them times ONE 32-channel column block, whose pair-format
//     weights (14 k-steps x (hi, lo) = 112 registers) stay in its registers over all tiles of the persistent loop.  The K loop is
//     84 MFMAs on LDS reads alone;
//   * affine + ReLU in the MFMA C layout into an f32 LDS patch, a barrier, the 3 x 3 / stride 2 maximum with a 16-byte channel
//     group per lane, stored non-temporally as whole 256-byte pixels.
// The next tile's input pixels are loaded into registers in front of the K loop and written to LDS behind it, before the pool.
// Workgroups share nothing; a stem pixel under two tiles is computed by both.
//
// Same bits as the three launches: per stem pixel K ascends over the 7 filter rows in two 16-wide k-steps each, the operands are the
// split8 pairs ((R, G), (B, 0)) of the same values -- 0.0f where the bordered copy holds zeros --, the three products go into one
// accumulator in the order of bf16x3.h (al * bh, ah * bl, ah * bh), the affine is stage_scaled's expression, the ReLU apply_act's and
// the maximum folds with fmaxf from -INFINITY over the window positions inside the stem map like maxpool3x3s2_kernel.
#include "conv_common.h"

namespace tt {
namespace {

constexpr int kPH = 7, kPW = 8;                          // pooled pixels of a tile
constexpr int kSH = 2 * kPH + 1, kSW = 2 * kPW + 1;      // stem pixels under them: 15 x 17
constexpr int kRows = kSH * kSW;                         // 255 rows of the implicit GEMM = 8 blocks of 32 (row 255 is a copy of 254)
constexpr int kIH = 2 * kSH + 5, kIW = 2 * kSW + 6;      // input pixels under those: 35 x 40 (a filter row's run is 8 pixels wide)
constexpr int kInPix = kIH * kIW;                        // 1400
constexpr int kInHalf = kInPix * 8;                      // bytes of the hi (and of the lo) pixels
constexpr int kLdc = 72;                                 // floats per row of the stem patch: 4 rows further = 32 banks further
constexpr int kStemBytes = 256 * kLdc * 4;
constexpr int kThreads = 512;                            // 8 waves
constexpr int kInPerThread = (kInPix + kThreads - 1) / kThreads;          // 3
constexpr int kPoolTasks = kPH * kPW * 16;                                // (pooled pixel, 4-channel group)
constexpr int kPoolPerThread = (kPoolTasks + kThreads - 1) / kThreads;    // 2
constexpr size_t kStemLds = 2 * (size_t)kInHalf + kStemBytes;             // 96,128 B
static_assert(kRows <= 256 && kRows > 224, "eight 32-row blocks");

struct StemPoolArgs {
    const float* img;
    long long sb, st, sn;        // element strides of b, t, n
    int B, T, N, H, W;
    int SH, SW, PH, PW;          // stem map, pooled map
    int tiles_y, tiles_x, ntiles;
    const float* w;              // pair format [64][7][1][32]
    const float* scale;
    const float* shift;
    float* out;
};

}  // namespace

__global__ __launch_bounds__(kThreads) void conv_x3_stem_pool_kernel(const StemPoolArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const in_hi = smem;                                    // [35][40] x 8 B, lo halves kInHalf further
    float* const stem = reinterpret_cast<float*>(smem + 2 * kInHalf);     // [256][kLdc]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, half = lane >> 5;
    const int nb = wave & 1;                                              // the wave's 32-channel column block
    const int mb0 = (wave >> 1) * 2;                                      // its two row blocks: mb0, mb0 + 1

    // ---- the wave's weights: column nb * 32 + r, every k-step's hi chunk `half` and lo chunk `half` + 2 of the 64-byte groups
    uint4 bh[14], bl[14];
    {
        const float* wrow = p.w + (long long)(nb * 32 + r) * (7 * 32);
#pragma unroll
        for (int ks = 0; ks < 14; ++ks) {
            bh[ks] = *reinterpret_cast<const uint4*>(wrow + ks * 16 + half * 4);
            bl[ks] = *reinterpret_cast<const uint4*>(wrow + ks * 16 + 8 + half * 4);
        }
    }
    const float sc = p.scale[nb * 32 + r], sh = p.shift[nb * 32 + r];

    // ---- A fragments: row m = stem pixel (m / 17, m % 17) of the tile; filter row ky, k-step s: input pixels (2 sy + ky,
    // 2 sx + 4 s + 2 half), + 1 -- 16 bytes of the hi pixels, the lo ones kInHalf further
    unsigned a_off[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int m = (mb0 + i) * 32 + r;
        m = m < kRows ? m : kRows - 1;
        const int sy = m / kSW, sx = m - sy * kSW;
        a_off[i] = (unsigned)(((2 * sy) * kIW + 2 * sx + 2 * half) * 8);
    }

    // persistent walk: workgroup b takes tiles b, b + grid, ... (dealing neighbouring tiles to one XCD measured no different)
    const int grid = (int)gridDim.x;
    const int slot = (int)blockIdx.x;
    const int tiles_per_img = p.tiles_y * p.tiles_x;
    const long long plane = (long long)p.H * p.W;

    // a tile's input pixels into registers: pixel q = tid + 512 k of the 35 x 40 patch, three planes; bit k of px_ok = inside the
    // image (outside, the load reads pixel (0, 0) and store_patch writes 0.0f: nothing here uses a loaded value, so the loads stay in
    // flight under the K loop)
    float px[kInPerThread][3];
    unsigned px_ok = 0;
    auto load_patch = [&](int tile) {
        const int i = tile / tiles_per_img, rem = tile - i * tiles_per_img;
        const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
        const int s = i / (p.B * p.N), bn = i - s * (p.B * p.N);
        const int b = bn / p.N, n = bn - b * p.N;
        const float* src = p.img + b * p.sb + (long long)(p.T - 1 - s) * p.st + n * p.sn;
        const int iy0 = 4 * kPH * ty - 5, ix0 = 4 * kPW * tx - 5;
        px_ok = 0;
#pragma unroll
        for (int k = 0; k < kInPerThread; ++k) {
            const int q = tid + k * kThreads;
            const int row = q / kIW, col = q - row * kIW;
            const int y = iy0 + row, x = ix0 + col;
            const bool ok = q < kInPix && y >= 0 && y < p.H && x >= 0 && x < p.W;
            const float* g = src + (long long)(ok ? y : 0) * p.W + (ok ? x : 0);
            px_ok |= ok ? 1u << k : 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) px[k][c] = g[c * plane];
        }
    };
    // ... and from there into LDS, split (bf16x3.h: the pairs (R, G) and (B, 0) of split8)
    auto store_patch = [&]() {
#pragma unroll
        for (int k = 0; k < kInPerThread; ++k) {
            const int q = tid + k * kThreads;
            if (q < kInPix) {
                const bool ok = (px_ok >> k) & 1u;
                const float x[4] = {ok ? px[k][0] : 0.f, ok ? px[k][1] : 0.f, ok ? px[k][2] : 0.f, 0.f};
                uint32_t h[2], l[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    h[e] = pack_bf16x2(x[2 * e], x[2 * e + 1]);
                    l[e] = pack_bf16x2(x[2 * e] - hi0_f32(h[e]), x[2 * e + 1] - hi1_f32(h[e]));
                }
                *reinterpret_cast<uint2*>(in_hi + q * 8) = make_uint2(h[0], h[1]);
                *reinterpret_cast<uint2*>(in_hi + kInHalf + q * 8) = make_uint2(l[0], l[1]);
            }
        }
    };

    int tile = slot;
    if (tile < p.ntiles) load_patch(tile);
    // the weights are used here, in front of the loop: left to their first MFMA, the compiler's waits for them sit inside the loop
#pragma unroll
    for (int ks = 0; ks < 14; ++ks) {
        asm volatile("" ::"v"(bh[ks].x), "v"(bl[ks].x));
    }
    if (tile < p.ntiles) store_patch();
    while (tile < p.ntiles) {
        __syncthreads();                          // the patch is published; every wave is done with the previous tile's stem patch
        const int next = tile + grid;
        if (next < p.ntiles) load_patch(next);    // in flight under the K loop

        // ---- K loop: 7 filter rows x 2 k-steps; term-major over the two row blocks, per accumulator the order of bf16x3.h
        f32x16 acc[2];
        zero_acc(acc);
#pragma unroll
        for (int ks = 0; ks < 14; ++ks) {
            const unsigned o = (unsigned)((ks >> 1) * (kIW * 8) + (ks & 1) * 32);
            uint4 ah[2], al[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = *reinterpret_cast<const uint4*>(in_hi + a_off[i] + o);
                al[i] = *reinterpret_cast<const uint4*>(in_hi + kInHalf + a_off[i] + o);
            }
            Mfma<uint16_t>::run(al[0], bh[ks], acc[0]);
            Mfma<uint16_t>::run(al[1], bh[ks], acc[1]);
            Mfma<uint16_t>::run(ah[0], bl[ks], acc[0]);
            Mfma<uint16_t>::run(ah[1], bl[ks], acc[1]);
            Mfma<uint16_t>::run(ah[0], bh[ks], acc[0]);
            Mfma<uint16_t>::run(ah[1], bh[ks], acc[1]);
        }

        // ---- affine (stage_scaled's expression) and ReLU (apply_act's) in the C layout: lane = column, register e = row
        // (e & 3) + 8 (e >> 2) + 4 half of the block
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (mb0 + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
                const float v = acc[i][e] * sc + sh;
                stem[row * kLdc + nb * 32 + r] = v > 0.f ? v : 0.f;
            }
        __syncthreads();                          // the stem patch is complete; every wave is done with the input patch
        // the next tile's pixels go to LDS in FRONT of the pool: behind it, the wait for them would also wait for the pool's stores
        if (next < p.ntiles) store_patch();

        // ---- 3 x 3 / stride 2 / pad 1 maximum: pooled pixel (py, px) of the tile reads stem rows 2 py .. 2 py + 2 of the patch,
        // the positions outside the stem map skipped
        {
            const int i = tile / tiles_per_img, rem = tile - i * tiles_per_img;
            const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
            const int py0 = kPH * ty, px0 = kPW * tx;
            const int sy0 = 2 * py0 - 1, sx0 = 2 * px0 - 1;
            typedef float f4v __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int k = 0; k < kPoolPerThread; ++k) {
                const int q = tid + k * kThreads;
                const int pp = q >> 4, cg = q & 15;
                const int pyl = pp >> 3, pxl = pp & 7;
                const int py = py0 + pyl, pxg = px0 + pxl;
                // a position outside the stem map reads the window's centre instead, which is inside it for every pooled pixel of
                // the map: the fold over the in-range positions with one of them repeated, and no branch around an LDS read
                float4 v[9];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const int sg = sy0 + 2 * pyl + dy;
                    const int sl = (sg < 0 || sg >= p.SH) ? 2 * pyl + 1 : 2 * pyl + dy;
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int cgl = sx0 + 2 * pxl + dx;
                        const int cl = (cgl < 0 || cgl >= p.SW) ? 2 * pxl + 1 : 2 * pxl + dx;
                        v[dy * 3 + dx] = *reinterpret_cast<const float4*>(stem + (sl * kSW + cl) * kLdc + cg * 4);
                    }
                }
                float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
                for (int e = 0; e < 9; ++e) {
                    m[0] = fmaxf(m[0], v[e].x);
                    m[1] = fmaxf(m[1], v[e].y);
                    m[2] = fmaxf(m[2], v[e].z);
                    m[3] = fmaxf(m[3], v[e].w);
                }
                if (q < kPoolTasks && py < p.PH && pxg < p.PW) {
                    float* o = p.out + (((long long)i * p.PH + py) * p.PW + pxg) * 64 + cg * 4;
                    __builtin_nontemporal_store(f4v{m[0], m[1], m[2], m[3]}, reinterpret_cast<f4v*>(o));
                }
            }
        }
        tile = next;
    }
#endif
}

}  // namespace tt

extern "C" int tt_stem_pool_x3(const float* img, long long stride_b, long long stride_t, long long stride_n, long long stride_c,
                               long long stride_h, long long stride_w, int B, int T, int N, int H, int W, int img_dtype,
                               const void* weight_x3, int w_cout, int w_kh, int w_k, const float* scale, const float* shift,
                               float* out, long long out_floats, int max_workgroups, void* stream) {
    using namespace tt;
    TT_REQUIRE(img_dtype == TT_F32, "tt_stem_pool_x3: img_dtype=%d: f32 storage only (the 16-bit stems keep their three launches)", img_dtype);
    TT_REQUIRE(img && out, "tt_stem_pool_x3: img / out is null");
    TT_REQUIRE(B > 0 && T > 0 && N > 0 && H > 0 && W > 0, "tt_stem_pool_x3: B=%d T=%d N=%d H=%d W=%d must be positive", B, T, N, H, W);
    TT_REQUIRE(H % 2 == 0, "tt_stem_pool_x3: H=%d must be even", H);
    TT_REQUIRE(W % 2 == 0, "tt_stem_pool_x3: W=%d must be even", W);
    TT_REQUIRE(stride_w == 1 && stride_h == W && stride_c == (long long)H * W,
               "tt_stem_pool_x3: stride_c=%lld stride_h=%lld stride_w=%lld: the inner (3, H, W) block must be contiguous", stride_c,
               stride_h, stride_w);
    TT_REQUIRE(stride_b >= 0 && stride_t >= 0 && stride_n >= 0, "tt_stem_pool_x3: stride_b / stride_t / stride_n must not be negative");
    TT_REQUIRE(weight_x3, "tt_stem_pool_x3: weight_x3 is null");
    TT_REQUIRE(w_cout == 64 && w_kh == 7 && w_k == 32, "tt_stem_pool_x3: weight_x3 shape [%d][%d][1][%d]: the row-run stem is [64][7][1][32]",
               w_cout, w_kh, w_k);
    TT_REQUIRE(((uintptr_t)weight_x3 & 15) == 0, "tt_stem_pool_x3: weight_x3 must be 16-byte aligned");
    TT_REQUIRE(scale && shift, "tt_stem_pool_x3: scale / shift is null");
    TT_REQUIRE(((uintptr_t)out & 15) == 0, "tt_stem_pool_x3: out must be 16-byte aligned");
    const long long NI = (long long)B * T * N;
    const int SH = H / 2, SW = W / 2, PH = (SH + 1) / 2, PW = (SW + 1) / 2;
    TT_REQUIRE(out_floats >= NI * PH * PW * 64, "tt_stem_pool_x3: out_floats=%lld is too small for (%lld, %d, %d, 64)", out_floats, NI, PH,
               PW);
    TT_REQUIRE(max_workgroups >= 0, "tt_stem_pool_x3: max_workgroups=%d must not be negative", max_workgroups);
    StemPoolArgs a;
    a.img = img;
    a.sb = stride_b; a.st = stride_t; a.sn = stride_n;
    a.B = B; a.T = T; a.N = N; a.H = H; a.W = W;
    a.SH = SH; a.SW = SW; a.PH = PH; a.PW = PW;
    a.tiles_y = div_up(PH, kPH);
    a.tiles_x = div_up(PW, kPW);
    const long long ntiles = NI * a.tiles_y * a.tiles_x;
    TT_REQUIRE(ntiles < (1ll << 31) && (long long)H * W < (1ll << 31), "tt_stem_pool_x3: %lld tiles / %d x %d pixels overflow an int", ntiles, H, W);
    a.ntiles = (int)ntiles;
    a.w = reinterpret_cast<const float*>(weight_x3);
    a.scale = scale;
    a.shift = shift;
    a.out = out;
    if (lds_opt_in(reinterpret_cast<const void*>(conv_x3_stem_pool_kernel), kStemLds, "tt_stem_pool_x3")) return -1;
    // persistent: one workgroup per CU (96 KiB of LDS each), the weights loaded once per wave
    int grid = (int)(ntiles < kNumCU ? ntiles : kNumCU);
    if (max_workgroups > 0 && max_workgroups < grid) grid = max_workgroups;
    hipLaunchKernelGGL(conv_x3_stem_pool_kernel, dim3((unsigned)grid), dim3(kThreads), kStemLds, (hipStream_t)stream, a);
    return check_launch("tt_stem_pool_x3");
}
