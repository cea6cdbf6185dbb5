// PNG files written on the device (thinktwice_hip.h, tt_png_encode_u8): the launches around csrc/png_deflate.h, which holds
// the filter pass, the deflate and the file's layout as plain functions.  Stream-ordered, no workgroup waits for another:
//
// filter    one 64-lane workgroup per row -> the filtered scanlines, in the image's region of the workspace
// deflate   one 64-lane workgroup per segment of R rows -> the segment's own worst-case slot, its size to sizes[segment]
// layout    one lane per image: the sizes' running sum -> the ttSG offsets, every fixed byte of the file, file_sizes_dev,
//           and where each segment goes
// compact   one 256-lane workgroup per segment copies it into the IDAT payload
// checksums the tile plan over the device's sizes (checksum_launch.h), Adler-32 tiles over the scanlines, their fold writes
//           the stream's last four bytes; then CRC-32 tiles over IHDR, ttSG and IDAT (type bytes and body) and their fold
//           writes the three CRC fields.  The host sizes the tile table for the largest file; a tile the device's plan does
//           not fill is refused by the tile kernel's own range check or sums bytes nobody reads.
//
// The workspace: per image a region [scanlines | one slot per segment], each part rounded up to 256 bytes; then sizes
// (int32 per segment), seg_at (int64 per segment), payload (int64 per image), first_tile, the tile table, the partials.
#include <limits.h>

#include "tt_common.h"          // (first: png_deflate.h's barrier and atomics are the HIP runtime's)
#include "png_deflate.h"
#include "checksum_launch.h"

namespace tt {

namespace enc = tt_pngenc;

constexpr long long kEncAlign = 256;
static inline __host__ __device__ long long enc_up(long long n) { return (n + kEncAlign - 1) / kEncAlign * kEncAlign; }

// One image's part of the workspace.
struct EncRegion {
    enc::FileGeom g;
    long long n_full, n_last;           // filtered bytes of a full segment, of the last
    long long slot_full, slot_last;     // their slots
    long long slots_at;                 // of the first slot in the region (the scanlines come first)
    long long bytes;                    // of the region
};

static inline __host__ __device__ EncRegion enc_region(const tt_png_enc_image& im) {
    EncRegion r;
    r.g = enc::file_geom(im.height, im.width, im.channels, im.rows_per_segment);
    r.n_full = r.g.rows * r.g.stride;
    r.n_last = enc::segment_rows(r.g, im.height, r.g.nseg - 1) * r.g.stride;
    r.slot_full = enc::segment_slot_bytes(r.n_full);
    r.slot_last = enc::segment_slot_bytes(r.n_last);
    r.slots_at = enc_up(r.g.expect);
    r.bytes = r.slots_at + enc_up((r.g.nseg - 1) * r.slot_full + r.slot_last);
    return r;
}

// Where an image, or the image of a row or of a segment, lies: the running sums over the table, the same in every lane.
struct EncWhere {
    int image;
    long long region_at;                // of the image's region in the workspace
    long long first_segment;            // the image's first entry in sizes / seg_at
    long long local;                    // the row or segment within the image
};

enum { kByImage = 0, kByRow = 1, kBySegment = 2 };

static inline __host__ __device__ EncWhere enc_find(const tt_png_enc_image* images, int num_images, int by, long long index) {
    EncWhere w{0, 0, 0, 0};
    long long count = 0;
    for (int i = 0; i < num_images; ++i) {
        const EncRegion r = enc_region(images[i]);
        const long long mine = by == kByImage ? 1 : by == kByRow ? images[i].height : r.g.nseg;
        if (index < count + mine) {
            w.image = i;
            w.local = index - count;
            return w;
        }
        count += mine;
        w.region_at += r.bytes;
        w.first_segment += r.g.nseg;
    }
    w.image = -1;
    return w;
}

__global__ __launch_bounds__(enc::kLanes) void png_filter_kernel(const uint8_t* __restrict__ pixels, const tt_png_enc_image* __restrict__ images,
                                                                 int num_images, uint8_t* __restrict__ ws) {
    __shared__ enc::FilterState F;
    const EncWhere w = enc_find(images, num_images, kByRow, blockIdx.x);
    if (w.image < 0) return;
    const tt_png_enc_image im = images[w.image];
    const long long row = (long long)im.width * im.channels;
    const uint8_t* cur = pixels + im.pixel_offset + w.local * row;
    const int lane = (int)threadIdx.x;
    enc::filter_row(F, cur, w.local ? cur - row : nullptr, (int)row, im.channels, im.filter, ws + w.region_at + w.local * (row + 1),
                    enc::Lanes{lane, lane + 1});
}

__global__ __launch_bounds__(enc::kLanes) void png_deflate_kernel(const tt_png_enc_image* __restrict__ images, int num_images,
                                                                  uint8_t* __restrict__ ws, int32_t* __restrict__ sizes) {
    __shared__ enc::State S;
    const EncWhere w = enc_find(images, num_images, kBySegment, blockIdx.x);
    if (w.image < 0) return;
    const tt_png_enc_image im = images[w.image];
    const EncRegion r = enc_region(im);
    const bool last = w.local == r.g.nseg - 1;
    const int lane = (int)threadIdx.x;
    enc::Stats stats;
    const long long got = enc::deflate_segment(S, ws + w.region_at + w.local * r.n_full, (int)(last ? r.n_last : r.n_full),
                                               ws + w.region_at + r.slots_at + w.local * r.slot_full, last ? r.slot_last : r.slot_full,
                                               enc::Lanes{lane, lane + 1}, stats);
    if (lane == 0) sizes[blockIdx.x] = (int32_t)got;
}

__global__ __launch_bounds__(enc::kLanes) void png_layout_kernel(const tt_png_enc_image* __restrict__ images, int num_images,
                                                                 const int32_t* __restrict__ sizes, long long* __restrict__ seg_at,
                                                                 long long* __restrict__ payload, uint8_t* __restrict__ files,
                                                                 long long* __restrict__ file_sizes) {
    const int img = (int)(blockIdx.x * enc::kLanes + threadIdx.x);
    if (img >= num_images) return;
    const EncWhere w = enc_find(images, num_images, kByImage, img);
    const tt_png_enc_image im = images[img];
    const enc::FileGeom g = enc::file_geom(im.height, im.width, im.channels, im.rows_per_segment);
    const long long bytes = enc::write_container(files + im.file_offset, im.height, im.width, im.channels, im.rows_per_segment, g,
                                                 sizes + w.first_segment, seg_at + w.first_segment);
    file_sizes[img] = bytes;
    payload[img] = bytes - g.idat_at - 12 - 12;
}

constexpr int kCopyLanes = 256;

__global__ __launch_bounds__(kCopyLanes) void png_compact_kernel(const tt_png_enc_image* __restrict__ images, int num_images,
                                                                 const uint8_t* __restrict__ ws, const int32_t* __restrict__ sizes,
                                                                 const long long* __restrict__ seg_at, uint8_t* __restrict__ files) {
    const EncWhere w = enc_find(images, num_images, kBySegment, blockIdx.x);
    if (w.image < 0) return;
    const tt_png_enc_image im = images[w.image];
    const EncRegion r = enc_region(im);
    const long long cap = w.local == r.g.nseg - 1 ? r.slot_last : r.slot_full;
    long long n = sizes[blockIdx.x];
    if (n > cap) n = cap;
    const long long at = seg_at[blockIdx.x];
    if (n < 0 || at < 0 || at > im.file_capacity - n) return;                // (not what the layout kernel wrote: nothing is copied)
    const uint8_t* src = ws + w.region_at + r.slots_at + w.local * r.slot_full;
    uint8_t* dst = files + im.file_offset + at;
    for (long long i = threadIdx.x; i < n; i += kCopyLanes) dst[i] = src[i];
}

// The ranges of one call: the Adler-32 of every image's scanlines (ranges 0 .. num_images, over the workspace), then per image
// the CRC-32 of IHDR, ttSG and IDAT, each over its type bytes and body (over files_dev).
struct EncRanges {
    const tt_png_enc_image* images;
    const long long* payload;
    int num_images;
    __host__ __device__ long long bytes(int r) const {
        if (r < num_images) return enc::file_geom(images[r].height, images[r].width, images[r].channels, images[r].rows_per_segment).expect;
        const int img = (r - num_images) / 3, k = (r - num_images) % 3;
        if (k == 0) return 17;
        const enc::FileGeom g = enc::file_geom(images[img].height, images[img].width, images[img].channels, images[img].rows_per_segment);
        if (k == 1) return g.idat_at - 4 - (enc::kTtsgAt + 4);
        long long p = payload[img];
        const long long most = images[img].file_capacity - g.idat_at - 24;
        if (p < 8) p = 8;
        if (p > most) p = most;
        return 4 + p;
    }
    __host__ __device__ long long offset(int r) const {
        if (r < num_images) return enc_find(images, num_images, kByImage, r).region_at;
        const int img = (r - num_images) / 3, k = (r - num_images) % 3;
        const enc::FileGeom g = enc::file_geom(images[img].height, images[img].width, images[img].channels, images[img].rows_per_segment);
        return images[img].file_offset + (k == 0 ? 12 : k == 1 ? enc::kTtsgAt + 4 : g.idat_at + 4);
    }
};

// One lane per range: fold its tiles and write the value, big-endian, where the file holds it: the Adler-32 in the last
// four bytes of the IDAT payload, a CRC-32 behind its chunk's body.
__global__ __launch_bounds__(tt_cksum::kLanes) void png_encode_fold_kernel(EncRanges src, int first_range, int num_ranges,
                                                                           const int* __restrict__ first_tile,
                                                                           const tt_cksum::Partial* __restrict__ parts, long long num_tiles,
                                                                           uint8_t* __restrict__ files, tt_cksum::PowTable pow) {
    const long long r = first_range + (long long)blockIdx.x * tt_cksum::kLanes + threadIdx.x;
    if (r >= num_ranges) return;
    const long long bytes = src.bytes((int)r), first = first_tile[r];
    if (bytes < 0 || first < 0 || first > num_tiles - tt_cksum::tiles_of(bytes)) return;      // not the table the host sized for
    if (r < src.num_images) {
        const tt_png_enc_image im = src.images[r];
        const enc::FileGeom g = enc::file_geom(im.height, im.width, im.channels, im.rows_per_segment);
        const long long p = src.bytes(src.num_images + 3 * (int)r + 2) - 4;                   // the payload, clamped to the slot
        enc::put_be32(files + im.file_offset + g.idat_at + 8 + p - 4, tt_cksum::fold_adler32(parts + first, bytes, 1u));
    } else {
        enc::put_be32(files + src.offset((int)r) + bytes, tt_cksum::fold_crc32(pow, parts + first, bytes, 0u));
    }
}

struct EncLayout {
    long long segments, regions;        // of all images: segments, bytes of the regions
    long long sizes, seg_at, payload, first_tile, tile_table, parts, total;
    long long adler_tiles, tiles, rows;
    int num_ranges;
};

// 0 where the table is refused for its sizes
static long long enc_image_ok(const tt_png_enc_image& im) {
    if ((im.channels != 1 && im.channels != 3) || im.height < 1 || im.width < 1 || im.rows_per_segment < 1) return 0;
    if (im.filter < TT_PNGE_FILTER_NONE || im.filter > TT_PNGE_FILTER_ADAPTIVE) return 0;
    const enc::FileGeom g = enc::file_geom(im.height, im.width, im.channels, im.rows_per_segment);
    if (g.rows * g.stride > INT_MAX - 64) return 0;
    const long long bound = enc::file_bound(g, im.height);
    if (bound - g.idat_at - 24 > 2147483640LL) return 0;                       // the zlib stream: at most 2^31 - 8 bytes
    return bound;
}

static bool enc_layout(const tt_png_enc_image* images, int num_images, EncLayout& L) {
    L = EncLayout{};
    if (!images || num_images < 1 || num_images > TT_PNG_MAX_IMAGES) return false;
    for (int i = 0; i < num_images; ++i) {
        const long long bound = enc_image_ok(images[i]);
        if (!bound) return false;
        const EncRegion r = enc_region(images[i]);
        L.segments += r.g.nseg;
        L.regions += r.bytes;
        L.rows += images[i].height;
        L.adler_tiles += tt_cksum::tiles_of(r.g.expect);
        L.tiles += tt_cksum::tiles_of(17) + tt_cksum::tiles_of(r.g.idat_at - 4 - (enc::kTtsgAt + 4)) + tt_cksum::tiles_of(bound - r.g.idat_at - 20);
    }
    L.tiles += L.adler_tiles;
    if (L.tiles > INT_MAX || L.segments > INT_MAX || L.rows > INT_MAX) return false;
    L.num_ranges = 4 * num_images;
    L.sizes = L.regions;
    L.seg_at = L.sizes + enc_up(4 * L.segments);
    L.payload = L.seg_at + enc_up(8 * L.segments);
    L.first_tile = L.payload + enc_up(8LL * num_images);
    L.tile_table = L.first_tile + enc_up(4LL * L.num_ranges);
    L.parts = L.tile_table + enc_up((long long)sizeof(tt_cksum::Tile) * L.tiles);
    L.total = L.parts + enc_up((long long)sizeof(tt_cksum::Partial) * L.tiles);
    return true;
}

static int png_encode(const uint8_t* pixels_dev, long long pixel_bytes, const tt_png_enc_image* images_host,
                      const tt_png_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes, uint8_t* files_dev,
                      long long files_bytes, long long* file_sizes_dev, int phases, void* stream) {
    TT_REQUIRE(pixels_dev && images_host && images_dev && workspace && files_dev && file_sizes_dev, "tt_png_encode_u8: null pointer");
    TT_REQUIRE(num_images >= 1 && num_images <= TT_PNG_MAX_IMAGES, "tt_png_encode_u8: %d images, 1..%d", num_images, TT_PNG_MAX_IMAGES);
    TT_REQUIRE(((uintptr_t)images_dev & 7) == 0 && ((uintptr_t)files_dev & 3) == 0 && ((uintptr_t)file_sizes_dev & 7) == 0 &&
                   ((uintptr_t)workspace & (kEncAlign - 1)) == 0,
               "tt_png_encode_u8: misaligned table, files, file sizes or workspace (8, 4, 8, 256 bytes)");
    TT_REQUIRE(pixel_bytes >= 0 && files_bytes >= 0, "tt_png_encode_u8: %lld pixel bytes, %lld file bytes", pixel_bytes, files_bytes);
    for (int i = 0; i < num_images; ++i) {
        const tt_png_enc_image& im = images_host[i];
        TT_REQUIRE(im.channels == 1 || im.channels == 3, "tt_png_encode_u8: image %d has %d channels, 1 or 3", i, im.channels);
        TT_REQUIRE(im.height >= 1 && im.width >= 1, "tt_png_encode_u8: image %d is %d x %d pixels", i, im.height, im.width);
        TT_REQUIRE(im.rows_per_segment >= 1, "tt_png_encode_u8: image %d has rows_per_segment %d", i, im.rows_per_segment);
        TT_REQUIRE(im.filter >= TT_PNGE_FILTER_NONE && im.filter <= TT_PNGE_FILTER_ADAPTIVE, "tt_png_encode_u8: image %d: unknown filter mode %d",
                   i, im.filter);
        const long long bound = enc_image_ok(im);
        TT_REQUIRE(bound > 0, "tt_png_encode_u8: image %d: a segment or the zlib stream could pass 2^31 - 8 bytes", i);
        const long long image = (long long)im.height * im.width * im.channels;
        TT_REQUIRE(im.pixel_offset >= 0 && im.pixel_offset <= pixel_bytes && image <= pixel_bytes - im.pixel_offset,
                   "tt_png_encode_u8: image %d: pixels [%lld, +%lld) outside the %lld pixel bytes", i, im.pixel_offset, image, pixel_bytes);
        TT_REQUIRE((im.file_offset & 3) == 0, "tt_png_encode_u8: image %d: file_offset %lld is not a multiple of 4", i, im.file_offset);
        TT_REQUIRE(im.file_capacity >= bound, "tt_png_encode_u8: image %d: a slot of %lld bytes, tt_png_encode_bound is %lld", i,
                   im.file_capacity, bound);
        TT_REQUIRE(im.file_offset >= 0 && im.file_offset <= files_bytes && im.file_capacity <= files_bytes - im.file_offset,
                   "tt_png_encode_u8: image %d: slot [%lld, +%lld) outside the %lld file bytes", i, im.file_offset, im.file_capacity,
                   files_bytes);
        for (int j = 0; j < i; ++j)
            TT_REQUIRE(im.file_offset >= images_host[j].file_offset + images_host[j].file_capacity ||
                           images_host[j].file_offset >= im.file_offset + im.file_capacity,
                       "tt_png_encode_u8: the slots of images %d and %d overlap", j, i);
    }
    EncLayout L;
    TT_REQUIRE(enc_layout(images_host, num_images, L), "tt_png_encode_u8: more than 2^31 - 1 rows, segments or checksum tiles");
    TT_REQUIRE(workspace_bytes >= L.total, "tt_png_encode_u8: need %lld bytes of workspace, got %lld", L.total, workspace_bytes);

    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    int32_t* sizes = (int32_t*)(ws + L.sizes);
    long long* seg_at = (long long*)(ws + L.seg_at);
    long long* payload = (long long*)(ws + L.payload);
    int* first_tile = (int*)(ws + L.first_tile);
    tt_cksum::Tile* tiles = (tt_cksum::Tile*)(ws + L.tile_table);
    tt_cksum::Partial* parts = (tt_cksum::Partial*)(ws + L.parts);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)L.rows), dim3(enc::kLanes), 0, st, pixels_dev, images_dev, num_images, ws);
    if (phases < 2) return check_launch("tt_png_encode_u8");
    hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)L.segments), dim3(enc::kLanes), 0, st, images_dev, num_images, ws, sizes);
    if (phases < 3) return check_launch("tt_png_encode_u8");
    hipLaunchKernelGGL(png_layout_kernel, dim3((unsigned)div_up(num_images, enc::kLanes)), dim3(enc::kLanes), 0, st, images_dev, num_images,
                       sizes, seg_at, payload, files_dev, file_sizes_dev);
    hipLaunchKernelGGL(png_compact_kernel, dim3((unsigned)L.segments), dim3(kCopyLanes), 0, st, images_dev, num_images, ws, sizes, seg_at,
                       files_dev);
    const EncRanges src{images_dev, payload, num_images};
    hipLaunchKernelGGL(checksum_plan_kernel<EncRanges>, dim3(1), dim3(tt_cksum::kLanes), 0, st, src, L.num_ranges, first_tile, tiles, L.tiles);
    checksum_launch_tiles(ws, L.regions, files_dev, files_bytes, num_images, tiles, L.adler_tiles, parts, st);
    hipLaunchKernelGGL(png_encode_fold_kernel, dim3((unsigned)div_up(num_images, tt_cksum::kLanes)), dim3(tt_cksum::kLanes), 0, st, src, 0,
                       num_images, first_tile, parts, L.tiles, files_dev, checksum_pow_table());
    checksum_launch_tiles(ws, L.regions, files_dev, files_bytes, num_images, tiles + L.adler_tiles, L.tiles - L.adler_tiles,
                          parts + L.adler_tiles, st);
    hipLaunchKernelGGL(png_encode_fold_kernel, dim3((unsigned)div_up(3 * num_images, tt_cksum::kLanes)), dim3(tt_cksum::kLanes), 0, st, src,
                       num_images, L.num_ranges, first_tile, parts, L.tiles, files_dev, checksum_pow_table());
    return check_launch("tt_png_encode_u8");
}

}  // namespace tt

using namespace tt;

extern "C" long long tt_png_encode_bound(const tt_png_enc_image* images_host, int num_images) {
    if (!images_host || num_images < 1 || num_images > TT_PNG_MAX_IMAGES) return 0;
    long long total = 0;
    for (int i = 0; i < num_images; ++i) {
        const long long bound = enc_image_ok(images_host[i]);
        if (!bound) return 0;
        total += bound;
    }
    return total;
}

extern "C" long long tt_png_encode_workspace_bytes(const tt_png_enc_image* images_host, int num_images) {
    EncLayout L;
    return enc_layout(images_host, num_images, L) ? L.total : 0;
}

extern "C" int tt_png_encode_u8(const uint8_t* pixels_dev, long long pixel_bytes, const tt_png_enc_image* images_host,
                                const tt_png_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                                uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, void* stream) {
    return png_encode(pixels_dev, pixel_bytes, images_host, images_dev, num_images, workspace, workspace_bytes, files_dev, files_bytes,
                      file_sizes_dev, 3, stream);
}

extern "C" int tt_png_encode_u8_phases(const uint8_t* pixels_dev, long long pixel_bytes, const tt_png_enc_image* images_host,
                                       const tt_png_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                                       uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, int phases, void* stream) {
    return png_encode(pixels_dev, pixel_bytes, images_host, images_dev, num_images, workspace, workspace_bytes, files_dev, files_bytes,
                      file_sizes_dev, phases, stream);
}
