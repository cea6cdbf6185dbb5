// The dataset's PNG files on the device (thinktwice_hip.h, tt_png_decode_u8): inflate, then unfilter, one launch each.
//
// inflate    one 64-lane workgroup per image runs png_inflate.h's inflate_zlib: the decode is wave-uniform, the byte moves
//            (input staging, match copies, table fill, window flush) are spread over the lanes.  A zlib stream has no restart
//            points: the parallelism is across the images of the call and inside the copies.
// unfilter   one 64-lane workgroup per image.  Sub, Average and Paeth are serial along a row and Up, Average and Paeth need
//            the row above, so 64 consecutive rows run as a skewed wavefront: at step s lane k reconstructs pixel x = s - k of
//            row r0 + k.  Its left neighbour is its own previous result, the pixel above is what lane k - 1 produced one step
//            earlier (one __shfl_up of a packed pixel), the upper-left one is the `up` it held one step before.  Lane 63 keeps
//            its row in LDS for lane 0 of the next band: different threads of one wave, ordered by the barrier between bands
//            and, inside a band, by lane 63 writing x = s - 63 only after lane 0 has read x = s.
// Neither kernel waits for another workgroup, and every loop is bounded by the image's sizes or the stream's length.
// tt_png_decode_u8_verified (csrc/png_verify.hip) puts the checksum launches between the two and reuses this file's argument
// checks and unfilter (png_launch.h): the unfilter skips every image whose status is not TT_PNG_OK, the checksum codes included.
#include <limits.h>

#include <algorithm>

#include "tt_common.h"          // (first: png_inflate.h's barrier is the HIP runtime's)
#include "png_inflate.h"
#include "png_launch.h"

namespace tt {

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ packed, long long packed_bytes,
                                                         const tt_png_image* __restrict__ images, uint8_t* __restrict__ ws,
                                                         int32_t* __restrict__ status) {
    __shared__ tt_png::State S;
    const int img = (int)blockIdx.x, lane = (int)threadIdx.x;
    const tt_png_image im = images[img];
    const long long off = png_slot_offset(images, img);
    const int skew = (int)(im.stream_offset & 3);                // `packed` is 16-byte aligned: read from the word the stream starts in
    const long long word0 = im.stream_offset - skew;
    const int st = tt_png::inflate_zlib(S, packed + word0, skew, skew + (int)im.stream_bytes, packed_bytes - word0, ws + off,
                                        (int)png_expect(im), lane, kWave);
    if (lane == 0) status[img] = st;
}

__device__ __forceinline__ uint32_t png_recon_px(int ft, int C, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (ch < C) {
            const int sh = 8 * ch;
            r |= (uint32_t)tt_png::recon(ft, (int)((x >> sh) & 255u), (int)((a >> sh) & 255u), (int)((b >> sh) & 255u),
                                         (int)((c >> sh) & 255u)) << sh;
        }
    }
    return r;
}

__global__ __launch_bounds__(64) void png_unfilter_kernel(const tt_png_image* __restrict__ images, const uint8_t* __restrict__ ws,
                                                          uint8_t* __restrict__ out_base, int32_t* __restrict__ status) {
    __shared__ uint32_t s_prev[TT_PNG_MAX_WIDTH];               // the band's last row, one packed pixel per x
    const int img = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (status[img] != TT_PNG_OK) return;                       // (uniform) the inflate failed: the destination stays as it is
    const tt_png_image im = images[img];
    const int H = im.height, W = im.width, C = im.channels;
    const long long row_bytes = (long long)W * C, stride = row_bytes + 1;
    const uint8_t* filt = ws + png_slot_offset(images, img);
    uint8_t* dst = out_base + im.dst_offset;

    bool bad = false;
    for (int r = lane; r < H; r += kWave) bad |= filt[r * stride] > 4;
    if (__ballot(bad)) {
        if (lane == 0) status[img] = TT_PNG_BAD_FILTER;
        return;
    }

    for (int r0 = 0; r0 < H; r0 += kWave) {
        const int row = r0 + lane;
        const bool valid = row < H;
        const int ft = valid ? filt[row * stride] : 0;
        const uint8_t* src = filt + (valid ? row : 0) * stride + 1;
        uint8_t* d = dst + (valid ? row : 0) * row_bytes;
        uint32_t mine = 0, a = 0, c = 0;
        for (int s = 0; s < W + kWave - 1; ++s) {
            const int x = s - lane;
            uint32_t up = __shfl_up(mine, 1, kWave);
            if (lane == 0) up = (r0 > 0 && s < W) ? s_prev[s] : 0u;
            if (valid && x >= 0 && x < W) {
                const long long o = (long long)x * C;
                uint32_t px = src[o];
                if (C == 3) px |= ((uint32_t)src[o + 1] << 8) | ((uint32_t)src[o + 2] << 16);
                mine = png_recon_px(ft, C, px, a, up, c);
                d[o] = (uint8_t)mine;
                if (C == 3) {
                    d[o + 1] = (uint8_t)(mine >> 8);
                    d[o + 2] = (uint8_t)(mine >> 16);
                }
                a = mine;
                c = up;
                if (lane == kWave - 1) s_prev[x] = mine;
            }
        }
        __syncthreads();
    }
}

// every check of the entry that needs only the table's sizes; 0 or the expected byte count
long long png_sizes_ok(const tt_png_image& im) {
    if (im.channels != 1 && im.channels != 3) return 0;
    if (im.width <= 0 || im.height <= 0 || im.width > TT_PNG_MAX_WIDTH) return 0;
    const long long e = png_expect(im);
    return e <= INT_MAX ? e : 0;
}

}  // namespace tt

using namespace tt;

extern "C" long long tt_png_workspace_bytes(const tt_png_image* images_host, int num_images) {
    if (!images_host || num_images < 1 || num_images > TT_PNG_MAX_IMAGES) return 0;
    long long total = 0;
    for (int i = 0; i < num_images; ++i) {
        if (!png_sizes_ok(images_host[i])) return 0;
        total += png_slot(images_host[i]);
    }
    return total;
}

// every refusal of tt_png_decode_u8 but the workspace's size: 0, or -1 with the error text set
int tt::png_check_args(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                          const tt_png_image* images_dev, int num_images, void* workspace, uint8_t* out_base, long long out_bytes,
                          int32_t* status_dev) {
    TT_REQUIRE(packed_dev && images_host && images_dev && workspace && out_base && status_dev, "tt_png_decode_u8: null pointer");
    TT_REQUIRE(num_images >= 1 && num_images <= TT_PNG_MAX_IMAGES, "tt_png_decode_u8: %d images, 1..%d", num_images,
               TT_PNG_MAX_IMAGES);
    TT_REQUIRE(packed_bytes > 0 && out_bytes > 0, "tt_png_decode_u8: %lld packed bytes, %lld output bytes", packed_bytes, out_bytes);
    TT_REQUIRE(((uintptr_t)packed_dev & 15) == 0, "tt_png_decode_u8: the packed buffer must be 16-byte aligned");
    TT_REQUIRE(((uintptr_t)images_dev & 7) == 0 && ((uintptr_t)status_dev & 3) == 0, "tt_png_decode_u8: misaligned table or status");
    TT_REQUIRE(((uintptr_t)workspace & (kPngSlotAlign - 1)) == 0, "tt_png_decode_u8: the workspace must be 256-byte aligned");
    struct Range {
        long long lo, hi;
    };
    Range dst[TT_PNG_MAX_IMAGES];
    for (int i = 0; i < num_images; ++i) {
        const tt_png_image& im = images_host[i];
        TT_REQUIRE(im.channels == 1 || im.channels == 3, "tt_png_decode_u8: image %d has %d channels, 1 or 3", i, im.channels);
        TT_REQUIRE(im.width > 0 && im.height > 0, "tt_png_decode_u8: image %d is %d x %d", i, im.height, im.width);
        TT_REQUIRE(im.width <= TT_PNG_MAX_WIDTH, "tt_png_decode_u8: image %d is %d pixels wide, at most %d", i, im.width,
                   TT_PNG_MAX_WIDTH);
        TT_REQUIRE(png_sizes_ok(im), "tt_png_decode_u8: image %d: %d x (1 + %d x %d) scanline bytes, at most 2^31 - 1", i, im.height,
                   im.width, im.channels);
        TT_REQUIRE(im.stream_bytes >= 6 && im.stream_bytes <= INT_MAX - 16,
                   "tt_png_decode_u8: image %d: a stream of %lld bytes, 6 .. 2^31 - 17", i, im.stream_bytes);
        TT_REQUIRE(im.stream_offset >= 0 && im.stream_offset <= packed_bytes && im.stream_bytes <= packed_bytes - im.stream_offset,
                   "tt_png_decode_u8: image %d: stream [%lld, +%lld) outside the %lld packed bytes", i, im.stream_offset,
                   im.stream_bytes, packed_bytes);
        const long long bytes = (long long)im.height * im.width * im.channels;
        TT_REQUIRE(im.dst_offset >= 0 && im.dst_offset <= out_bytes && bytes <= out_bytes - im.dst_offset,
                   "tt_png_decode_u8: image %d: destination [%lld, +%lld) outside the %lld output bytes", i, im.dst_offset, bytes,
                   out_bytes);
        dst[i].lo = im.dst_offset;
        dst[i].hi = im.dst_offset + bytes;
    }
    std::sort(dst, dst + num_images, [](const Range& p, const Range& q) { return p.lo < q.lo; });
    for (int i = 1; i < num_images; ++i)
        TT_REQUIRE(dst[i].lo >= dst[i - 1].hi, "tt_png_decode_u8: the destinations [%lld, %lld) and [%lld, %lld) overlap", dst[i - 1].lo,
                   dst[i - 1].hi, dst[i].lo, dst[i].hi);
    return 0;
}

extern "C" int tt_png_decode_u8_phases(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                                       const tt_png_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                                       uint8_t* out_base, long long out_bytes, int32_t* status_dev, int phases, void* stream) {
    TT_REQUIRE(phases == 1 || phases == 2, "tt_png_decode_u8: %d phases, 1 or 2", phases);
    if (png_check_args(packed_dev, packed_bytes, images_host, images_dev, num_images, workspace, out_base, out_bytes, status_dev))
        return -1;
    const long long need = tt_png_workspace_bytes(images_host, num_images);
    TT_REQUIRE(need > 0 && workspace_bytes >= need, "tt_png_decode_u8: need %lld bytes of workspace, got %lld", need, workspace_bytes);

    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)num_images), dim3(kWave), 0, st, packed_dev, packed_bytes, images_dev,
                       (uint8_t*)workspace, status_dev);
    if (phases >= 2)
        hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)num_images), dim3(kWave), 0, st, images_dev, (const uint8_t*)workspace,
                           out_base, status_dev);
    return check_launch("tt_png_decode_u8");
}

extern "C" int tt_png_decode_u8(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                                const tt_png_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                                uint8_t* out_base, long long out_bytes, int32_t* status_dev, void* stream) {
    return tt_png_decode_u8_phases(packed_dev, packed_bytes, images_host, images_dev, num_images, workspace, workspace_bytes,
                                   out_base, out_bytes, status_dev, 2, stream);
}

void tt::png_launch_unverified(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_dev, int num_images,
                               uint8_t* workspace, uint8_t* out_base, int32_t* status_dev, bool inflate, hipStream_t st) {
    if (inflate)
        hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)num_images), dim3(kWave), 0, st, packed_dev, packed_bytes, images_dev,
                           workspace, status_dev);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)num_images), dim3(kWave), 0, st, images_dev, (const uint8_t*)workspace,
                       out_base, status_dev);
}
