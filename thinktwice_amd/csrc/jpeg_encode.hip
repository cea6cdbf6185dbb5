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
// The workspace: per image a region [coefficients | one slot per interval], each part rounded up to 256 bytes; then sizes
// (int32 per interval) and int_at (int64 per interval).
#include <limits.h>

#include "tt_common.h"          // (first: the core's barrier and atomics are the HIP runtime's)
#include "jpeg_core.h"

namespace tt {

namespace jpg = tt_jpeg;

constexpr long long kJpgAlign = 256;
static inline __host__ __device__ long long jpg_up(long long n) { return (n + kJpgAlign - 1) / kJpgAlign * kJpgAlign; }

// One image's part of the workspace.
struct JpgRegion {
    jpg::Geom g;
    long long slot_full, slot_last;     // the slot of a full interval, of the last
    long long slots_at;                 // of the first slot in the region (the coefficients come first)
    long long bytes;                    // of the region
    long long groups;                   // transform workgroups: 64 blocks each
};

static inline __host__ __device__ JpgRegion jpg_region(const tt_jpeg_enc_image& im) {
    JpgRegion r;
    r.g = jpg::geom(im.height, im.width, im.channels, im.subsampling, im.restart_rows);
    r.slot_full = jpg::interval_slot_bytes(jpg::interval_blocks(r.g, im.restart_rows, 0));
    r.slot_last = jpg::interval_slot_bytes(jpg::interval_blocks(r.g, im.restart_rows, r.g.nint - 1));
    r.slots_at = jpg_up(r.g.blocks * 128);
    r.bytes = r.slots_at + jpg_up((r.g.nint - 1) * r.slot_full + r.slot_last);
    r.groups = (r.g.blocks + jpg::kLanes - 1) / jpg::kLanes;
    return r;
}

// Where an image, or the image of a transform workgroup or of an interval, lies: the running sums over the table, the same in
// every lane.
struct JpgWhere {
    int image;
    long long region_at;                // of the image's region in the workspace
    long long first_interval;           // the image's first entry in sizes / int_at
    long long local;                    // the workgroup or interval within the image
};

enum { kJpgByImage = 0, kJpgByGroup = 1, kJpgByInterval = 2 };

static inline __host__ __device__ JpgWhere jpg_find(const tt_jpeg_enc_image* images, int num_images, int by, long long index) {
    JpgWhere w{0, 0, 0, 0};
    long long count = 0;
    for (int i = 0; i < num_images; ++i) {
        const JpgRegion r = jpg_region(images[i]);
        const long long mine = by == kJpgByImage ? 1 : by == kJpgByGroup ? r.groups : r.g.nint;
        if (index < count + mine) {
            w.image = i;
            w.local = index - count;
            return w;
        }
        count += mine;
        w.region_at += r.bytes;
        w.first_interval += r.g.nint;
    }
    w.image = -1;
    return w;
}

__global__ __launch_bounds__(jpg::kLanes) void jpeg_transform_kernel(const uint8_t* __restrict__ pixels, const tt_jpeg_enc_image* __restrict__ images,
                                                                     int num_images, uint8_t* __restrict__ ws) {
    __shared__ uint16_t q[128];
    const JpgWhere w = jpg_find(images, num_images, kJpgByGroup, blockIdx.x);
    if (w.image < 0) return;
    const tt_jpeg_enc_image im = images[w.image];
    const jpg::Geom g = jpg::geom(im.height, im.width, im.channels, im.subsampling, im.restart_rows);
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
    const JpgWhere w = jpg_find(images, num_images, kJpgByInterval, blockIdx.x);
    if (w.image < 0) return;
    const tt_jpeg_enc_image im = images[w.image];
    const JpgRegion r = jpg_region(im);
    const int k = (int)w.local, lane = (int)threadIdx.x;
    const bool last = k == r.g.nint - 1;
    const int16_t* coefs = reinterpret_cast<const int16_t*>(ws + w.region_at) + jpg::interval_first_block(r.g, im.restart_rows, k) * 64;
    const long long got = jpg::encode_interval(S, coefs, jpg::interval_blocks(r.g, im.restart_rows, k), r.g.bpm,
                                               ws + w.region_at + r.slots_at + k * r.slot_full, last ? r.slot_last : r.slot_full,
                                               last ? jpg::kEoi : jpg::kRst0 + (k & 7), jpg::Lanes{lane, lane + 1});
    if (lane == 0) sizes[blockIdx.x] = (int32_t)got;
}

__global__ __launch_bounds__(jpg::kLanes) void jpeg_layout_kernel(const tt_jpeg_enc_image* __restrict__ images, int num_images,
                                                                  const int32_t* __restrict__ sizes, long long* __restrict__ int_at,
                                                                  uint8_t* __restrict__ files, long long* __restrict__ file_sizes) {
    const int img = (int)(blockIdx.x * jpg::kLanes + threadIdx.x);
    if (img >= num_images) return;
    const JpgWhere w = jpg_find(images, num_images, kJpgByImage, img);
    const tt_jpeg_enc_image im = images[img];
    const JpgRegion r = jpg_region(im);
    long long at = jpg::write_header(files + im.file_offset, im.height, im.width, im.quality, r.g);
    for (int k = 0; k < r.g.nint; ++k) {
        const long long cap = k == r.g.nint - 1 ? r.slot_last : r.slot_full;
        long long n = sizes[w.first_interval + k];
        n = n < 0 ? 0 : n > cap ? cap : n;                                        // (a size the entropy pass cannot write)
        int_at[w.first_interval + k] = at;
        at += n;
    }
    file_sizes[img] = at;
}

constexpr int kJpgCopyLanes = 256;

__global__ __launch_bounds__(kJpgCopyLanes) void jpeg_compact_kernel(const tt_jpeg_enc_image* __restrict__ images, int num_images,
                                                                     const uint8_t* __restrict__ ws, const int32_t* __restrict__ sizes,
                                                                     const long long* __restrict__ int_at, uint8_t* __restrict__ files) {
    const JpgWhere w = jpg_find(images, num_images, kJpgByInterval, blockIdx.x);
    if (w.image < 0) return;
    const tt_jpeg_enc_image im = images[w.image];
    const JpgRegion r = jpg_region(im);
    const long long cap = w.local == r.g.nint - 1 ? r.slot_last : r.slot_full;
    long long n = sizes[blockIdx.x];
    if (n > cap) n = cap;
    const long long at = int_at[blockIdx.x];
    if (n < 0 || at < 0 || at > im.file_capacity - n) return;                    // (not what the layout kernel wrote: nothing is copied)
    const uint8_t* src = ws + w.region_at + r.slots_at + w.local * r.slot_full;
    uint8_t* dst = files + im.file_offset + at;
    for (long long i = threadIdx.x; i < n; i += kJpgCopyLanes) dst[i] = src[i];
}

struct JpgLayout {
    long long intervals, groups, regions;       // of all images: intervals, transform workgroups, bytes of the regions
    long long sizes, int_at, total;
};

// 0 where the table is refused for its sizes or parameters
static long long jpg_image_ok(const tt_jpeg_enc_image& im) {
    if ((im.channels != 1 && im.channels != 3) || im.height < 1 || im.width < 1 || im.height > jpg::kMaxDim || im.width > jpg::kMaxDim) return 0;
    if (im.quality < 1 || im.quality > 100 || (im.subsampling != TT_JPEG_444 && im.subsampling != TT_JPEG_420) || im.restart_rows < 1) return 0;
    const jpg::Geom g = jpg::geom(im.height, im.width, im.channels, im.subsampling, im.restart_rows);
    if (g.dri > 65535) return 0;
    return jpg::file_bound(g);
}

static bool jpg_layout(const tt_jpeg_enc_image* images, int num_images, JpgLayout& L) {
    L = JpgLayout{};
    if (!images || num_images < 1 || num_images > TT_PNG_MAX_IMAGES) return false;
    for (int i = 0; i < num_images; ++i) {
        if (!jpg_image_ok(images[i])) return false;
        const JpgRegion r = jpg_region(images[i]);
        L.intervals += r.g.nint;
        L.groups += r.groups;
        L.regions += r.bytes;
    }
    if (L.intervals > INT_MAX || L.groups > INT_MAX) return false;
    L.sizes = L.regions;
    L.int_at = L.sizes + jpg_up(4 * L.intervals);
    L.total = L.int_at + jpg_up(8 * L.intervals);
    return true;
}

static int jpeg_encode(const uint8_t* pixels_dev, long long pixel_bytes, const tt_jpeg_enc_image* images_host,
                       const tt_jpeg_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes, uint8_t* files_dev,
                       long long files_bytes, long long* file_sizes_dev, int phases, void* stream) {
    TT_REQUIRE(pixels_dev && images_host && images_dev && workspace && files_dev && file_sizes_dev, "tt_jpeg_encode_u8: null pointer");
    TT_REQUIRE(num_images >= 1 && num_images <= TT_PNG_MAX_IMAGES, "tt_jpeg_encode_u8: %d images, 1..%d", num_images, TT_PNG_MAX_IMAGES);
    TT_REQUIRE(((uintptr_t)images_dev & 7) == 0 && ((uintptr_t)files_dev & 3) == 0 && ((uintptr_t)file_sizes_dev & 7) == 0 &&
                   ((uintptr_t)workspace & (kJpgAlign - 1)) == 0,
               "tt_jpeg_encode_u8: misaligned table, files, file sizes or workspace (8, 4, 8, 256 bytes)");
    TT_REQUIRE(pixel_bytes >= 0 && files_bytes >= 0, "tt_jpeg_encode_u8: %lld pixel bytes, %lld file bytes", pixel_bytes, files_bytes);
    for (int i = 0; i < num_images; ++i) {
        const tt_jpeg_enc_image& im = images_host[i];
        TT_REQUIRE(im.channels == 1 || im.channels == 3, "tt_jpeg_encode_u8: image %d has %d channels, 1 or 3", i, im.channels);
        TT_REQUIRE(im.height >= 1 && im.width >= 1 && im.height <= jpg::kMaxDim && im.width <= jpg::kMaxDim,
                   "tt_jpeg_encode_u8: image %d is %d x %d pixels, 1..%d", i, im.height, im.width, jpg::kMaxDim);
        TT_REQUIRE(im.quality >= 1 && im.quality <= 100, "tt_jpeg_encode_u8: image %d has quality %d, 1..100", i, im.quality);
        TT_REQUIRE(im.subsampling == TT_JPEG_444 || im.subsampling == TT_JPEG_420, "tt_jpeg_encode_u8: image %d: unknown subsampling %d", i,
                   im.subsampling);
        TT_REQUIRE(im.restart_rows >= 1, "tt_jpeg_encode_u8: image %d has restart_rows %d", i, im.restart_rows);
        const long long bound = jpg_image_ok(im);
        TT_REQUIRE(bound > 0, "tt_jpeg_encode_u8: image %d: %d MCU rows per restart interval make a DRI value above 65535", i, im.restart_rows);
        const long long image = (long long)im.height * im.width * im.channels;
        TT_REQUIRE(im.pixel_offset >= 0 && im.pixel_offset <= pixel_bytes && image <= pixel_bytes - im.pixel_offset,
                   "tt_jpeg_encode_u8: image %d: pixels [%lld, +%lld) outside the %lld pixel bytes", i, im.pixel_offset, image, pixel_bytes);
        TT_REQUIRE((im.file_offset & 3) == 0, "tt_jpeg_encode_u8: image %d: file_offset %lld is not a multiple of 4", i, im.file_offset);
        TT_REQUIRE(im.file_capacity >= bound, "tt_jpeg_encode_u8: image %d: a slot of %lld bytes, tt_jpeg_encode_bound is %lld", i,
                   im.file_capacity, bound);
        TT_REQUIRE(im.file_offset >= 0 && im.file_offset <= files_bytes && im.file_capacity <= files_bytes - im.file_offset,
                   "tt_jpeg_encode_u8: image %d: slot [%lld, +%lld) outside the %lld file bytes", i, im.file_offset, im.file_capacity,
                   files_bytes);
        for (int j = 0; j < i; ++j)
            TT_REQUIRE(im.file_offset >= images_host[j].file_offset + images_host[j].file_capacity ||
                           images_host[j].file_offset >= im.file_offset + im.file_capacity,
                       "tt_jpeg_encode_u8: the slots of images %d and %d overlap", j, i);
    }
    JpgLayout L;
    TT_REQUIRE(jpg_layout(images_host, num_images, L), "tt_jpeg_encode_u8: more than 2^31 - 1 intervals or block groups");
    TT_REQUIRE(workspace_bytes >= L.total, "tt_jpeg_encode_u8: need %lld bytes of workspace, got %lld", L.total, workspace_bytes);

    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    int32_t* sizes = (int32_t*)(ws + L.sizes);
    long long* int_at = (long long*)(ws + L.int_at);
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)L.groups), dim3(jpg::kLanes), 0, st, pixels_dev, images_dev, num_images, ws);
    if (phases < 2) return check_launch("tt_jpeg_encode_u8");
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)L.intervals), dim3(jpg::kLanes), 0, st, images_dev, num_images, ws, sizes);
    if (phases < 3) return check_launch("tt_jpeg_encode_u8");
    hipLaunchKernelGGL(jpeg_layout_kernel, dim3((unsigned)div_up(num_images, jpg::kLanes)), dim3(jpg::kLanes), 0, st, images_dev, num_images,
                       sizes, int_at, files_dev, file_sizes_dev);
    hipLaunchKernelGGL(jpeg_compact_kernel, dim3((unsigned)L.intervals), dim3(kJpgCopyLanes), 0, st, images_dev, num_images, ws, sizes, int_at,
                       files_dev);
    return check_launch("tt_jpeg_encode_u8");
}

}  // namespace tt

using namespace tt;

extern "C" long long tt_jpeg_encode_bound(const tt_jpeg_enc_image* images_host, int num_images) {
    if (!images_host || num_images < 1 || num_images > TT_PNG_MAX_IMAGES) return 0;
    long long total = 0;
    for (int i = 0; i < num_images; ++i) {
        const long long bound = jpg_image_ok(images_host[i]);
        if (!bound) return 0;
        total += bound;
    }
    return total;
}

extern "C" long long tt_jpeg_encode_workspace_bytes(const tt_jpeg_enc_image* images_host, int num_images) {
    JpgLayout L;
    return jpg_layout(images_host, num_images, L) ? L.total : 0;
}

extern "C" int tt_jpeg_encode_u8(const uint8_t* pixels_dev, long long pixel_bytes, const tt_jpeg_enc_image* images_host,
                                 const tt_jpeg_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                                 uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, void* stream) {
    return jpeg_encode(pixels_dev, pixel_bytes, images_host, images_dev, num_images, workspace, workspace_bytes, files_dev, files_bytes,
                       file_sizes_dev, 3, stream);
}

extern "C" int tt_jpeg_encode_u8_phases(const uint8_t* pixels_dev, long long pixel_bytes, const tt_jpeg_enc_image* images_host,
                                        const tt_jpeg_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                                        uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, int phases, void* stream) {
    return jpeg_encode(pixels_dev, pixel_bytes, images_host, images_dev, num_images, workspace, workspace_bytes, files_dev, files_bytes,
                       file_sizes_dev, phases, stream);
}
