// JPEG files written on the device (thinktwice_hip.h, tt_jpeg_encode_u8): the launches around csrc/jpeg_core.h, which holds the
// transform of a block, the entropy coding of a restart interval and the file's headers as plain functions.  Stream-ordered, no
// workgroup waits for another:
//
// transform one lane per 8 x 8 block, 64 blocks of ONE image per workgroup (its quantisation tables in LDS) -> int16
//           coefficients, zig-zag order, blocks in scan order, in the image's region of the workspace
// entropy   one 64-lane workgroup per restart interval -> the interval's own worst-case slot, its size to sizes[interval]
// layout    one lane per image: the headers, the sizes' running sum -> where each interval goes, file_sizes_dev
// compact   one 256-lane workgroup per interval copies it into the file
//
// The workspace: file_slots.h's (per image a region [coefficients | one slot per interval], then sizes and int_at per interval).
#include "tt_common.h"          // (first: the core's barrier and atomics are the HIP runtime's)
#include "jpeg_core.h"
#include "file_encode_launch.h"

namespace tt {

namespace jpg = tt_jpeg;
namespace slots = tt_slots;
using JpgSlots = jpg::SlotFormat;

__global__ __launch_bounds__(jpg::kLanes) void jpeg_transform_kernel(const uint8_t* __restrict__ pixels, const tt_jpeg_enc_image* __restrict__ images,
                                                                     int num_images, uint8_t* __restrict__ ws) {
    __shared__ uint16_t q[128];
    const slots::Where w = slots::find<JpgSlots>(images, num_images, slots::kByUnit, blockIdx.x);
    if (w.image < 0) return;
    const tt_jpeg_enc_image im = images[w.image];
    const jpg::Geom g = JpgSlots::geom(im);
    const int lane = (int)threadIdx.x;
    jpg::fill_quant(q, im.quality, jpg::Lanes{lane, lane + 1});
    __syncthreads();
    const long long b = w.local * jpg::kLanes + lane;
    if (b >= g.blocks) return;
    int16_t out[64];
    jpg::transform_block(pixels + im.pixel_offset, im.height, im.width, g, b, q, out);
    uint4* dst = reinterpret_cast<uint4*>(ws + w.region_at + b * 128);            // (the region is 256-byte aligned)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint4 v;
        v.x = (uint16_t)out[8 * i + 0] | ((uint32_t)(uint16_t)out[8 * i + 1] << 16);
        v.y = (uint16_t)out[8 * i + 2] | ((uint32_t)(uint16_t)out[8 * i + 3] << 16);
        v.z = (uint16_t)out[8 * i + 4] | ((uint32_t)(uint16_t)out[8 * i + 5] << 16);
        v.w = (uint16_t)out[8 * i + 6] | ((uint32_t)(uint16_t)out[8 * i + 7] << 16);
        dst[i] = v;
    }
}

__global__ __launch_bounds__(jpg::kLanes) void jpeg_entropy_kernel(const tt_jpeg_enc_image* __restrict__ images, int num_images,
                                                                   uint8_t* __restrict__ ws, int32_t* __restrict__ sizes) {
    __shared__ jpg::State S;
    const slots::Where w = slots::find<JpgSlots>(images, num_images, slots::kByPart, blockIdx.x);
    if (w.image < 0) return;
    const tt_jpeg_enc_image im = images[w.image];
    const slots::Region<JpgSlots> r = slots::region<JpgSlots>(im);
    const int k = (int)w.local, lane = (int)threadIdx.x;
    const int16_t* coefs = reinterpret_cast<const int16_t*>(ws + w.region_at) + jpg::interval_first_block(r.g, im.restart_rows, k) * 64;
    const long long got = jpg::encode_interval(S, coefs, jpg::interval_blocks(r.g, im.restart_rows, k), r.g.bpm,
                                               slots::slot_at(ws + w.region_at, r, k), slots::slot_cap(r, k),
                                               k == r.g.nint - 1 ? jpg::kEoi : jpg::kRst0 + (k & 7), jpg::Lanes{lane, lane + 1});
    if (lane == 0) sizes[blockIdx.x] = (int32_t)got;
}

__global__ __launch_bounds__(jpg::kLanes) void jpeg_layout_kernel(const tt_jpeg_enc_image* __restrict__ images, int num_images,
                                                                  const int32_t* __restrict__ sizes, long long* __restrict__ int_at,
                                                                  uint8_t* __restrict__ files, long long* __restrict__ file_sizes) {
    const int img = (int)(blockIdx.x * jpg::kLanes + threadIdx.x);
    if (img >= num_images) return;
    const slots::Where w = slots::find<JpgSlots>(images, num_images, slots::kByImage, img);
    const tt_jpeg_enc_image im = images[img];
    const slots::Region<JpgSlots> r = slots::region<JpgSlots>(im);
    long long at = jpg::write_header(files + im.file_offset, im.height, im.width, im.quality, r.g);
    for (int k = 0; k < r.g.nint; ++k) {
        const long long cap = slots::slot_cap(r, k);
        long long n = sizes[w.first_part + k];
        n = n < 0 ? 0 : n > cap ? cap : n;                                        // (a size the entropy pass cannot write)
        int_at[w.first_part + k] = at;
        at += n;
    }
    file_sizes[img] = at;
}

__global__ __launch_bounds__(kCopyLanes) void jpeg_compact_kernel(const tt_jpeg_enc_image* __restrict__ images, int num_images,
                                                                  const uint8_t* __restrict__ ws, const int32_t* __restrict__ sizes,
                                                                  const long long* __restrict__ int_at, uint8_t* __restrict__ files) {
    compact_block<JpgSlots>(images, num_images, ws, sizes, int_at, files);
}

// The format's own refusals of image i.
static int jpeg_image_check(const tt_jpeg_enc_image& im, int i) {
    TT_REQUIRE(im.channels == 1 || im.channels == 3, "tt_jpeg_encode_u8: image %d has %d channels, 1 or 3", i, im.channels);
    TT_REQUIRE(im.height >= 1 && im.width >= 1 && im.height <= jpg::kMaxDim && im.width <= jpg::kMaxDim,
               "tt_jpeg_encode_u8: image %d is %d x %d pixels, 1..%d", i, im.height, im.width, jpg::kMaxDim);
    TT_REQUIRE(im.quality >= 1 && im.quality <= 100, "tt_jpeg_encode_u8: image %d has quality %d, 1..100", i, im.quality);
    TT_REQUIRE(im.subsampling == TT_JPEG_444 || im.subsampling == TT_JPEG_420, "tt_jpeg_encode_u8: image %d: unknown subsampling %d", i,
               im.subsampling);
    TT_REQUIRE(im.restart_rows >= 1, "tt_jpeg_encode_u8: image %d has restart_rows %d", i, im.restart_rows);
    TT_REQUIRE(JpgSlots::bound(im) > 0, "tt_jpeg_encode_u8: image %d: %d MCU rows per restart interval make a DRI value above 65535", i,
               im.restart_rows);
    return 0;
}

}  // namespace tt

using namespace tt;

extern "C" int tt_jpeg_encode_u8_phases(const uint8_t* pixels_dev, long long pixel_bytes, const tt_jpeg_enc_image* images_host,
                                        const tt_jpeg_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                                        uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, int phases, void* stream) {
    if (check_file_table<JpgSlots>("tt_jpeg_encode_u8", "tt_jpeg_encode_bound", pixels_dev, pixel_bytes, images_host, images_dev, num_images,
                                   workspace, files_dev, files_bytes, file_sizes_dev, jpeg_image_check))
        return -1;
    slots::Totals T;
    TT_REQUIRE(slots::totals<JpgSlots>(images_host, num_images, T), "tt_jpeg_encode_u8: more than 2^31 - 1 intervals or block groups");
    TT_REQUIRE(workspace_bytes >= T.end, "tt_jpeg_encode_u8: need %lld bytes of workspace, got %lld", T.end, workspace_bytes);

    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    int32_t* sizes = (int32_t*)(ws + T.sizes);
    long long* int_at = (long long*)(ws + T.part_at);
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)T.units), dim3(jpg::kLanes), 0, st, pixels_dev, images_dev, num_images, ws);
    if (phases < 2) return check_launch("tt_jpeg_encode_u8");
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)T.parts), dim3(jpg::kLanes), 0, st, images_dev, num_images, ws, sizes);
    if (phases < 3) return check_launch("tt_jpeg_encode_u8");
    hipLaunchKernelGGL(jpeg_layout_kernel, dim3((unsigned)div_up(num_images, jpg::kLanes)), dim3(jpg::kLanes), 0, st, images_dev, num_images,
                       sizes, int_at, files_dev, file_sizes_dev);
    hipLaunchKernelGGL(jpeg_compact_kernel, dim3((unsigned)T.parts), dim3(kCopyLanes), 0, st, images_dev, num_images, ws, sizes, int_at,
                       files_dev);
    return check_launch("tt_jpeg_encode_u8");
}

extern "C" long long tt_jpeg_encode_bound(const tt_jpeg_enc_image* images_host, int num_images) {
    return slots::bound_sum<JpgSlots>(images_host, num_images);
}

extern "C" long long tt_jpeg_encode_workspace_bytes(const tt_jpeg_enc_image* images_host, int num_images) {
    slots::Totals T;
    return slots::totals<JpgSlots>(images_host, num_images, T) ? T.end : 0;
}

extern "C" int tt_jpeg_encode_u8(const uint8_t* pixels_dev, long long pixel_bytes, const tt_jpeg_enc_image* images_host,
                                 const tt_jpeg_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                                 uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, void* stream) {
    return tt_jpeg_encode_u8_phases(pixels_dev, pixel_bytes, images_host, images_dev, num_images, workspace, workspace_bytes, files_dev,
                                    files_bytes, file_sizes_dev, 3, stream);
}
