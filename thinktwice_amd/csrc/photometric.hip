// Colour augmentation of training frames: ImageTransformMulti(aug=True) and its imgaug `augmenter(iteration)`
// (datasets/pipelines/transform.py:142-216) as a table-driven device stage.  The host (thinktwice_amd/photometric.py) draws
// one program per sample and compiles it into steps (tt_aug_op of thinktwice_hip.h, which states every step's arithmetic);
// the kernels here execute the tables and nothing else: no transcendental function, no fused multiply-add.
//
// One templated pair of kernels serves both entries, a source functor (uint8 load | IDA gather + astype(uint8)) and a sink
// functor (uint8 store | /255, Normalize, NCHW f32 and / or channel-last padded):
//   stage A  the point steps up to the blur -- the whole program for a sample without one, which goes to the sink; with a
//            blur a packed 4-byte pixel goes to the scratch image.  blockIdx.y is the image, so the program is block-uniform
//            and its tables are staged in LDS once per block.
//   stage B  (launched only when some program has a blur; blocks of a sample without one return at once) a 64 x 16 tile with
//            a 2-pixel reflect-101 halo in LDS, horizontal 5-tap pass into an f32 LDS tile, vertical pass, rint, clip, the
//            remaining point steps, the sink.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "preprocess_ida.h"

namespace tt {

constexpr int kAugOpWords = (int)sizeof(tt_aug_op) / 4;
constexpr int kAugProgWords = (int)sizeof(tt_aug_program) / 4;
constexpr int kAugHeadWords = 2;                       // num_ops, blur_index
constexpr int kBlurTW = 64, kBlurTH = 16, kBlurR = 2;   // stage B's tile and halo
static_assert(sizeof(tt_aug_op) == 856 && sizeof(tt_aug_program) == 6856, "tt_aug_program layout (photometric.py mirrors it)");
static_assert(kAugHeadWords * 4 + TT_AUG_MAX_OPS * sizeof(tt_aug_op) == sizeof(tt_aug_program), "tt_aug_program has no padding");

// the field value of element idx: high 32 bits of the dropout kernel's splitmix64 mix (batchnorm.hip)
__device__ __forceinline__ uint32_t aug_field(unsigned long long seed, unsigned long long idx) {
    unsigned long long zz = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
    zz = (zz ^ (zz >> 30)) * 0xBF58476D1CE4E5B9ull;
    zz = (zz ^ (zz >> 27)) * 0x94D049BB133111EBull;
    zz ^= zz >> 31;
    return (uint32_t)(zz >> 32);
}

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// one point step on the grey levels v[3] of pixel (y, x) of an H x W image; `op` is block-uniform (LDS)
__device__ __forceinline__ void aug_point(const tt_aug_op& op, int H, int W, int y, int x, int v[3]) {
    switch (op.kind) {
        case TT_AUG_LUT:
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = op.lut[c][v[c]];
            break;
        case TT_AUG_NOISE: {
            uint32_t u = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c == 0 || op.per_channel)
                    u = aug_field(op.seed, ((unsigned long long)(op.per_channel ? c : 0) * H + y) * W + x);
                int k = -TT_AUG_NOISE_K;
#pragma unroll
                for (int j = 0; j < 2 * TT_AUG_NOISE_K; ++j) k += u >= op.cum[j] ? 1 : 0;
                v[c] = clip8(v[c] + k);
            }
            break;
        }
        case TT_AUG_DROPOUT: {
            uint32_t u = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c == 0 || op.per_channel)
                    u = aug_field(op.seed, ((unsigned long long)(op.per_channel ? c : 0) * H + y) * W + x);
                if (u < op.threshold) v[c] = 0;
            }
            break;
        }
        case TT_AUG_COARSE: {
            const int cy = y * op.grid_h / H, cx = x * op.grid_w / W;     // (H, W <= 32768: the products fit)
            uint32_t u = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c == 0 || op.per_channel)
                    u = aug_field(op.seed, ((unsigned long long)(op.per_channel ? c : 0) * op.grid_h + cy) * op.grid_w + cx);
                if (u < op.threshold) v[c] = 0;
            }
            break;
        }
        case TT_AUG_GRAY: {
            const int g = (4899 * v[0] + 9617 * v[1] + 1868 * v[2] + 8192) >> 14;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = clip8((int)rintf((float)v[c] + op.alpha * (float)(g - v[c])));
            break;
        }
        default:
            break;
    }
}

// ---- sources: grey levels 0..255 of pixel (y, x) of image n ----
struct AugU8Src {
    const uint8_t* in;
    int H, W;
    __device__ __forceinline__ void load(int n, int y, int x, int v[3]) const {
        const uint8_t* p = in + (((long long)n * H + y) * W + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = p[c];
    }
};

// preprocess_ida_kernel's gather, then the reference's astype(np.uint8) between its two transforms
struct AugIdaSrc {
    IdaArgs a;
    IdaTable tab;
    const uint8_t* raw;
    const float* mapx;
    const float* mapy;
    __device__ __forceinline__ void load(int n, int oy, int ox, int v[3]) const {
        const IdaTaps k = ida_taps(tab.s[(n / a.per_sample) * a.N + n % a.N], a.H, a.W, a.OW, oy, ox);
        const uint8_t* img = raw + (long long)n * a.H * a.W * 3;
        float p00[3], p01[3], p10[3], p11[3];
        undist_px(img, mapx, mapy, a.H, a.W, k.y0, k.x0, p00);
        undist_px(img, mapx, mapy, a.H, a.W, k.y0, k.x1, p01);
        undist_px(img, mapx, mapy, a.H, a.W, k.y1, k.x0, p10);
        undist_px(img, mapx, mapy, a.H, a.W, k.y1, k.x1, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = (1.f - k.lx) * p00[c] + k.lx * p01[c];
            const float bot = (1.f - k.lx) * p10[c] + k.lx * p11[c];
            v[c] = clip8((int)((1.f - k.ly) * top + k.ly * bot));
        }
    }
};

// ---- sinks ----
struct AugU8Sink {
    uint8_t* out;
    int H, W;
    __device__ __forceinline__ void store(int n, int y, int x, const int v[3]) const {
        uint8_t* p = out + (((long long)n * H + y) * W + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = (uint8_t)v[c];
    }
};

// preprocess_ida_kernel's normalisation and output forms
template <typename T>
struct AugNormSink {
    T* out;
    float* out_nchw;
    int OH, OW, Cp, pixel16;
    float mean[3], inv_std[3];
    __device__ __forceinline__ void store(int n, int oy, int ox, const int g[3]) const {
        const long long t = ((long long)n * OH + oy) * OW + ox;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = ((float)g[c] / 255.f - mean[c]) * inv_std[c];
            if (out_nchw) out_nchw[(((long long)n * 3 + c) * OH + oy) * OW + ox] = v[c];
        }
        if (!out) return;
        if (pixel16) {
            constexpr int kN = 16 / (int)sizeof(T);
            union { T e[kN]; uint4 q; } px;
#pragma unroll
            for (int c = 0; c < kN; ++c) Elem<T>::st(px.e + c, c < 3 ? v[c] : 0.f);
            *reinterpret_cast<uint4*>(out + t * kN) = px.q;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) Elem<T>::st(out + t * Cp + c, v[c]);
            for (int c = 3; c < Cp; ++c) Elem<T>::st(out + t * Cp + c, 0.f);
        }
    }
};

// The block's program: steps [first, last) of program `g` into LDS.  The counts are clamped here as well, so that a device
// copy that differs from the checked host copy cannot index outside the staged words.
struct AugRange {
    int num_ops, blur;      // blur: index of the BLUR step or -1
};

__device__ __forceinline__ AugRange aug_range(const uint32_t* __restrict__ g) {
    AugRange r;
    r.num_ops = min(max((int)g[0], 0), TT_AUG_MAX_OPS);
    const int bi = (int)g[1];
    r.blur = (bi >= 0 && bi < r.num_ops) ? bi : -1;
    return r;
}

__device__ __forceinline__ void aug_stage_program(uint32_t* s_words, const uint32_t* __restrict__ g, int first, int last) {
    for (int i = kAugHeadWords + first * kAugOpWords + (int)threadIdx.x; i < kAugHeadWords + last * kAugOpWords; i += (int)blockDim.x)
        s_words[i] = g[i];
    __syncthreads();
}

template <typename Src, typename Sink>
__global__ __launch_bounds__(256) void aug_point_kernel(Src src, Sink sink, const tt_aug_program* __restrict__ progs,
                                                        int per_sample, int H, int W, uint32_t* __restrict__ scratch) {
    __shared__ __align__(16) uint32_t s_words[kAugProgWords];
    const int n = (int)blockIdx.y;
    const uint32_t* g = reinterpret_cast<const uint32_t*>(progs + n / per_sample);
    const AugRange r = aug_range(g);
    const int end = r.blur >= 0 ? r.blur : r.num_ops;
    aug_stage_program(s_words, g, 0, end);
    const tt_aug_program& P = *reinterpret_cast<const tt_aug_program*>(s_words);
    const int HW = H * W;
    for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < HW; p += (int)(gridDim.x * blockDim.x)) {
        const int y = p / W, x = p - y * W;
        int v[3];
        src.load(n, y, x, v);
        for (int k = 0; k < end; ++k) aug_point(P.ops[k], H, W, y, x, v);
        if (r.blur >= 0)
            scratch[(long long)n * HW + p] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
        else
            sink.store(n, y, x, v);
    }
}

// reflect-101 (i < 0 -> -i, i >= n -> 2n - 2 - i; exact within 2 of the image for n >= 3), then clamped so that the halo of a
// partial tile's pixels outside the image, which nobody uses, still reads inside it
__device__ __forceinline__ int reflect101(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}

template <typename Sink>
__global__ __launch_bounds__(256) void aug_blur_kernel(Sink sink, const tt_aug_program* __restrict__ progs, int per_sample,
                                                       int H, int W, const uint32_t* __restrict__ scratch) {
    constexpr int kIW = kBlurTW + 2 * kBlurR, kIH = kBlurTH + 2 * kBlurR;
    __shared__ __align__(16) uint32_t s_words[kAugProgWords];
    __shared__ uint32_t s_in[kIH][kIW];
    __shared__ float s_h[3][kIH][kBlurTW];
    const int n = (int)blockIdx.z;
    const uint32_t* g = reinterpret_cast<const uint32_t*>(progs + n / per_sample);
    const AugRange r = aug_range(g);
    if (r.blur < 0) return;                                     // (block-uniform)
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * kBlurTW, y0 = (int)blockIdx.y * kBlurTH;
    const uint32_t* img = scratch + (long long)n * H * W;
    for (int i = tid; i < kIH * kIW; i += 256) {
        const int rr = i / kIW, cc = i - rr * kIW;
        s_in[rr][cc] = img[(long long)reflect101(y0 + rr - kBlurR, H) * W + reflect101(x0 + cc - kBlurR, W)];
    }
    aug_stage_program(s_words, g, r.blur, r.num_ops);           // (its barrier covers s_in too)
    const tt_aug_program& P = *reinterpret_cast<const tt_aug_program*>(s_words);
    float t[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) t[k] = P.ops[r.blur].taps[k];
    for (int i = tid; i < kIH * kBlurTW; i += 256) {
        const int rr = i / kBlurTW, cc = i - rr * kBlurTW;
        uint32_t px[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) px[k] = s_in[rr][cc + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = t[0] * (float)((px[0] >> (8 * c)) & 255u) + t[1] * (float)((px[1] >> (8 * c)) & 255u);
#pragma unroll
            for (int k = 2; k < 5; ++k) acc = acc + t[k] * (float)((px[k] >> (8 * c)) & 255u);
            s_h[c][rr][cc] = acc;
        }
    }
    __syncthreads();
    const int tx = tid % kBlurTW;
    for (int ty = tid / kBlurTW; ty < kBlurTH; ty += 256 / kBlurTW) {
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = t[0] * s_h[c][ty][tx] + t[1] * s_h[c][ty + 1][tx];
#pragma unroll
            for (int k = 2; k < 5; ++k) acc = acc + t[k] * s_h[c][ty + k][tx];
            v[c] = clip8((int)rintf(acc));
        }
        for (int k = r.blur + 1; k < r.num_ops; ++k) aug_point(P.ops[k], H, W, y, x, v);
        sink.store(n, y, x, v);
    }
}

}  // namespace tt

using namespace tt;

// every program on the host, before anything is launched; *any_blur: whether stage B is needed
static int aug_check(const char* what, const tt_aug_program* host, const tt_aug_program* dev, int B, long long num_images, int H,
                     int W, const void* scratch, long long scratch_bytes, bool* any_blur) {
    TT_REQUIRE(host, "%s: null host program pointer", what);
    TT_REQUIRE(dev, "%s: null device program pointer", what);
    TT_REQUIRE(H > 0 && W > 0 && H <= 32768 && W <= 32768, "%s: image size %d x %d outside 1..32768", what, H, W);
    TT_REQUIRE(num_images > 0 && num_images <= 65535, "%s: %lld images in one call, at most 65535", what, num_images);
    *any_blur = false;
    for (int b = 0; b < B; ++b) {
        const tt_aug_program& p = host[b];
        TT_REQUIRE(p.num_ops >= 0 && p.num_ops <= TT_AUG_MAX_OPS, "%s: sample %d: num_ops %d outside 0..%d", what, b, p.num_ops,
                   TT_AUG_MAX_OPS);
        int blur = -1;
        for (int k = 0; k < p.num_ops; ++k) {
            const tt_aug_op& op = p.ops[k];
            switch (op.kind) {
                case TT_AUG_LUT:
                case TT_AUG_DROPOUT:
                    break;
                case TT_AUG_NOISE:
                    for (int j = 1; j < 2 * TT_AUG_NOISE_K; ++j)
                        TT_REQUIRE(op.cum[j - 1] <= op.cum[j], "%s: sample %d step %d: noise thresholds decrease at %d", what, b, k, j);
                    break;
                case TT_AUG_COARSE:
                    TT_REQUIRE(op.grid_h >= 1 && op.grid_h <= H && op.grid_w >= 1 && op.grid_w <= W,
                               "%s: sample %d step %d: grid %d x %d outside 1..%d x 1..%d", what, b, k, op.grid_h, op.grid_w, H, W);
                    break;
                case TT_AUG_GRAY:
                    TT_REQUIRE(op.alpha >= 0.f && op.alpha <= 1.f, "%s: sample %d step %d: alpha %g outside [0, 1]", what, b, k,
                               (double)op.alpha);     // (false for NaN)
                    break;
                case TT_AUG_BLUR: {
                    TT_REQUIRE(blur < 0, "%s: sample %d: steps %d and %d are both blurs, at most one", what, b, blur, k);
                    blur = k;
                    double sum = 0;
                    for (int j = 0; j < 5; ++j) {
                        TT_REQUIRE(isfinite(op.taps[j]) && op.taps[j] >= 0.f, "%s: sample %d step %d: tap %d is %g", what, b, k, j,
                                   (double)op.taps[j]);
                        sum += op.taps[j];
                    }
                    TT_REQUIRE(fabs(sum - 1.0) <= 1e-5, "%s: sample %d step %d: taps sum to %.9g", what, b, k, sum);
                    TT_REQUIRE(H >= 3 && W >= 3, "%s: sample %d step %d: a blur needs H, W >= 3, got %d x %d", what, b, k, H, W);
                    break;
                }
                default:
                    TT_REQUIRE(false, "%s: sample %d step %d: unknown kind %d", what, b, k, op.kind);
            }
            if (op.kind == TT_AUG_NOISE || op.kind == TT_AUG_DROPOUT || op.kind == TT_AUG_COARSE)
                TT_REQUIRE(op.per_channel == 0 || op.per_channel == 1, "%s: sample %d step %d: per_channel must be 0 or 1", what, b, k);
        }
        TT_REQUIRE(p.blur_index == blur, "%s: sample %d: blur_index %d, the blur is step %d", what, b, p.blur_index, blur);
        if (blur >= 0) *any_blur = true;
    }
    if (*any_blur) {
        const long long need = tt_photometric_scratch_bytes((int)num_images, H, W);
        TT_REQUIRE(scratch && scratch_bytes >= need, "%s: a program has a blur: need %lld bytes of scratch, got %lld", what, need,
                   scratch ? scratch_bytes : 0LL);
        TT_REQUIRE(((uintptr_t)scratch & 3) == 0, "%s: scratch must be 4-byte aligned", what);
    }
    return 0;
}

template <typename Src, typename Sink>
static void aug_launch(const Src& src, const Sink& sink, const tt_aug_program* dev, int num_images, int per_sample, int H, int W,
                       bool any_blur, void* scratch, hipStream_t stream) {
    // enough blocks per image to fill the device, few enough that staging the program stays a small share of a block's work
    const int gx = std::min(div_up((long long)H * W, 256), std::max(32, div_up(8192, num_images)));
    hipLaunchKernelGGL((aug_point_kernel<Src, Sink>), dim3(gx, num_images), dim3(256), 0, stream, src, sink, dev, per_sample, H, W,
                       (uint32_t*)scratch);
    if (any_blur)
        hipLaunchKernelGGL((aug_blur_kernel<Sink>), dim3(div_up(W, kBlurTW), div_up(H, kBlurTH), num_images), dim3(256), 0, stream,
                           sink, dev, per_sample, H, W, (const uint32_t*)scratch);
}

extern "C" long long tt_photometric_scratch_bytes(int num_images, int H, int W) {
    if (num_images <= 0 || H <= 0 || W <= 0) return 0;
    return (long long)num_images * H * W * 4;
}

extern "C" int tt_photometric_u8(const uint8_t* in_u8, int B, int per_sample, int H, int W, const tt_aug_program* programs_host,
                                 const tt_aug_program* programs_dev, void* scratch, long long scratch_bytes, uint8_t* out_u8,
                                 void* stream) {
    TT_REQUIRE(in_u8 && out_u8 && in_u8 != out_u8, "tt_photometric_u8: null or aliased images");
    TT_REQUIRE(B > 0 && per_sample > 0, "tt_photometric_u8: bad sizes");
    bool any_blur;
    if (int rc = aug_check("tt_photometric_u8", programs_host, programs_dev, B, (long long)B * per_sample, H, W, scratch,
                           scratch_bytes, &any_blur))
        return rc;
    const AugU8Src src{in_u8, H, W};
    const AugU8Sink sink{out_u8, H, W};
    aug_launch(src, sink, programs_dev, B * per_sample, per_sample, H, W, any_blur, scratch, (hipStream_t)stream);
    return check_launch("tt_photometric_u8");
}

template <typename T>
static void aug_launch_ida(const AugIdaSrc& src, const IdaArgs& a, void* out_nhwc, float* out_nchw, const tt_aug_program* dev,
                           bool any_blur, void* scratch, hipStream_t stream) {
    AugNormSink<T> sink;
    sink.out = (T*)out_nhwc; sink.out_nchw = out_nchw;
    sink.OH = a.OH; sink.OW = a.OW; sink.Cp = a.Cp; sink.pixel16 = a.pixel16;
    for (int c = 0; c < 3; ++c) { sink.mean[c] = a.mean[c]; sink.inv_std[c] = a.inv_std[c]; }
    aug_launch(src, sink, dev, a.NI, a.per_sample, a.OH, a.OW, any_blur, scratch, stream);
}

extern "C" int tt_preprocess_images_ida_aug(const uint8_t* raw_hwc, int B, int T, int N, int H, int W, const float* mapx,
                                            const float* mapy, const tt_ida_set* sets, int out_h, int out_w,
                                            const float* mean3, const float* std3, void* out_nhwc, int out_channels_padded,
                                            int out_dtype, float* out_nchw_or_null, const tt_aug_program* programs_host,
                                            const tt_aug_program* programs_dev, void* scratch, long long scratch_bytes,
                                            void* stream) {
    // tt_preprocess_images_ida's checks
    TT_REQUIRE(raw_hwc && mapx && mapy && mean3 && std3 && (out_nhwc || out_nchw_or_null), "tt_preprocess_images_ida_aug: null");
    TT_REQUIRE(B > 0 && T > 0 && N > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0, "tt_preprocess_images_ida_aug: bad sizes");
    TT_REQUIRE(out_channels_padded >= 3, "tt_preprocess_images_ida_aug: need >= 3 output channels");
    TT_REQUIRE(out_dtype == TT_F32 || out_dtype == TT_BF16 || out_dtype == TT_F16, "tt_preprocess_images_ida_aug: bad dtype");
    TT_REQUIRE((long long)B * N <= TT_IDA_MAX_SETS, "tt_preprocess_images_ida_aug: B * N = %lld parameter sets, at most %d",
               (long long)B * N, TT_IDA_MAX_SETS);
    AugIdaSrc src;
    if (int rc = ida_fill("tt_preprocess_images_ida_aug", sets, B * N, out_h, out_w, &src.tab)) return rc;
    const long long total = (long long)B * T * N * out_h * out_w;
    TT_REQUIRE((long long)B * T * N <= INT_MAX && (total + 255) / 256 <= INT_MAX, "tt_preprocess_images_ida_aug: too many pixels");
    bool any_blur;
    if (int rc = aug_check("tt_preprocess_images_ida_aug", programs_host, programs_dev, B, (long long)B * T * N, out_h, out_w,
                           scratch, scratch_bytes, &any_blur))
        return rc;
    IdaArgs& a = src.a;
    a.NI = B * T * N; a.H = H; a.W = W; a.per_sample = T * N; a.N = N;
    a.OH = out_h; a.OW = out_w; a.Cp = out_channels_padded;
    a.pixel16 = out_channels_padded * (out_dtype == TT_F32 ? 4 : 2) == 16 && ((uintptr_t)out_nhwc & 15) == 0;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.inv_std[c] = 1.f / std3[c]; }
    src.raw = raw_hwc; src.mapx = mapx; src.mapy = mapy;
    if (out_dtype == TT_F32)
        aug_launch_ida<float>(src, a, out_nhwc, out_nchw_or_null, programs_dev, any_blur, scratch, (hipStream_t)stream);
    else if (out_dtype == TT_BF16)
        aug_launch_ida<uint16_t>(src, a, out_nhwc, out_nchw_or_null, programs_dev, any_blur, scratch, (hipStream_t)stream);
    else
        aug_launch_ida<f16_t>(src, a, out_nhwc, out_nchw_or_null, programs_dev, any_blur, scratch, (hipStream_t)stream);
    return check_launch("tt_preprocess_images_ida_aug");
}
