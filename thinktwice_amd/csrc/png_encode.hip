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
// The workspace: file_slots.h's (per image a region [scanlines | one slot per segment], then sizes and seg_at per segment);
// behind it payload (int64 per image), first_tile, the tile table, the partials.
#include "tt_common.h"          // (first: png_deflate.h's barrier and atomics are the HIP runtime's)
#include "png_deflate.h"
#include "file_encode_launch.h"
#include "checksum_launch.h"

namespace tt {

namespace enc = tt_pngenc;
namespace slots = tt_slots;
using PngSlots = enc::SlotFormat;

__global__ __launch_bounds__(enc::kLanes) void png_filter_kernel(const uint8_t* __restrict__ pixels, const tt_png_enc_image* __restrict__ images,
                                                                 int num_images, uint8_t* __restrict__ ws) {
    __shared__ enc::FilterState F;
    const slots::Where w = slots::find<PngSlots>(images, num_images, slots::kByUnit, blockIdx.x);
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
    const slots::Where w = slots::find<PngSlots>(images, num_images, slots::kByPart, blockIdx.x);
    if (w.image < 0) return;
    const tt_png_enc_image im = images[w.image];
    const slots::Region<PngSlots> r = slots::region<PngSlots>(im);
    const bool last = w.local == r.g.nseg - 1;
    const int lane = (int)threadIdx.x;
    enc::Stats stats;
    const long long got = enc::deflate_segment(S, ws + w.region_at + w.local * r.g.n_full, (int)(last ? r.g.n_last : r.g.n_full),
                                               slots::slot_at(ws + w.region_at, r, w.local), slots::slot_cap(r, w.local),
                                               enc::Lanes{lane, lane + 1}, stats);
    if (lane == 0) sizes[blockIdx.x] = (int32_t)got;
}

__global__ __launch_bounds__(enc::kLanes) void png_layout_kernel(const tt_png_enc_image* __restrict__ images, int num_images,
                                                                 const int32_t* __restrict__ sizes, long long* __restrict__ seg_at,
                                                                 long long* __restrict__ payload, uint8_t* __restrict__ files,
                                                                 long long* __restrict__ file_sizes) {
    const int img = (int)(blockIdx.x * enc::kLanes + threadIdx.x);
    if (img >= num_images) return;
    const slots::Where w = slots::find<PngSlots>(images, num_images, slots::kByImage, img);
    const tt_png_enc_image im = images[img];
    const enc::FileGeom g = PngSlots::geom(im);
    const long long bytes = enc::write_container(files + im.file_offset, im.height, im.width, im.channels, im.rows_per_segment, g,
                                                 sizes + w.first_part, seg_at + w.first_part);
    file_sizes[img] = bytes;
    payload[img] = bytes - g.idat_at - 12 - 12;
}

__global__ __launch_bounds__(kCopyLanes) void png_compact_kernel(const tt_png_enc_image* __restrict__ images, int num_images,
                                                                 const uint8_t* __restrict__ ws, const int32_t* __restrict__ sizes,
                                                                 const long long* __restrict__ seg_at, uint8_t* __restrict__ files) {
    compact_block<PngSlots>(images, num_images, ws, sizes, seg_at, files);
}

// The ranges of one call: the Adler-32 of every image's scanlines (ranges 0 .. num_images, over the workspace), then per image
// the CRC-32 of IHDR, ttSG and IDAT, each over its type bytes and body (over files_dev).
struct EncRanges {
    const tt_png_enc_image* images;
    const long long* payload;
    int num_images;
    __host__ __device__ long long bytes(int r) const {
        if (r < num_images) return PngSlots::geom(images[r]).expect;
        const int img = (r - num_images) / 3, k = (r - num_images) % 3;
        if (k == 0) return 17;
        const enc::FileGeom g = PngSlots::geom(images[img]);
        if (k == 1) return g.idat_at - 4 - (enc::kTtsgAt + 4);
        long long p = payload[img];
        const long long most = images[img].file_capacity - g.idat_at - 24;
        if (p < 8) p = 8;
        if (p > most) p = most;
        return 4 + p;
    }
    __host__ __device__ long long offset(int r) const {
        if (r < num_images) return slots::find<PngSlots>(images, num_images, slots::kByImage, r).region_at;
        const int img = (r - num_images) / 3, k = (r - num_images) % 3;
        const enc::FileGeom g = PngSlots::geom(images[img]);
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
        const enc::FileGeom g = PngSlots::geom(im);
        const long long p = src.bytes(src.num_images + 3 * (int)r + 2) - 4;                   // the payload, clamped to the slot
        enc::put_be32(files + im.file_offset + g.idat_at + 8 + p - 4, tt_cksum::fold_adler32(parts + first, bytes, 1u));
    } else {
        enc::put_be32(files + src.offset((int)r) + bytes, tt_cksum::fold_crc32(pow, parts + first, bytes, 0u));
    }
}

// The checksum tables behind file_slots.h's part of the workspace.
struct EncLayout {
    slots::Totals t;
    long long payload, first_tile, tile_table, parts, total;
    long long adler_tiles, tiles;
    int num_ranges;
};

static bool enc_layout(const tt_png_enc_image* images, int num_images, EncLayout& L) {
    L = EncLayout{};
    if (!slots::totals<PngSlots>(images, num_images, L.t)) return false;
    for (int i = 0; i < num_images; ++i) {
        const enc::FileGeom g = PngSlots::geom(images[i]);
        L.adler_tiles += tt_cksum::tiles_of(g.expect);
        L.tiles += tt_cksum::tiles_of(17) + tt_cksum::tiles_of(g.idat_at - 4 - (enc::kTtsgAt + 4)) +
                   tt_cksum::tiles_of(PngSlots::bound(images[i]) - g.idat_at - 20);
    }
    L.tiles += L.adler_tiles;
    if (L.tiles > 2147483647LL) return false;
    L.num_ranges = 4 * num_images;
    L.payload = L.t.end;
    L.first_tile = L.payload + slots::up(8LL * num_images);
    L.tile_table = L.first_tile + slots::up(4LL * L.num_ranges);
    L.parts = L.tile_table + slots::up((long long)sizeof(tt_cksum::Tile) * L.tiles);
    L.total = L.parts + slots::up((long long)sizeof(tt_cksum::Partial) * L.tiles);
    return true;
}

// The format's own refusals of image i.
static int png_image_check(const tt_png_enc_image& im, int i) {
    TT_REQUIRE(im.channels == 1 || im.channels == 3, "tt_png_encode_u8: image %d has %d channels, 1 or 3", i, im.channels);
    TT_REQUIRE(im.height >= 1 && im.width >= 1, "tt_png_encode_u8: image %d is %d x %d pixels", i, im.height, im.width);
    TT_REQUIRE(im.rows_per_segment >= 1, "tt_png_encode_u8: image %d has rows_per_segment %d", i, im.rows_per_segment);
    TT_REQUIRE(im.filter >= TT_PNGE_FILTER_NONE && im.filter <= TT_PNGE_FILTER_ADAPTIVE, "tt_png_encode_u8: image %d: unknown filter mode %d",
               i, im.filter);
    TT_REQUIRE(PngSlots::bound(im) > 0, "tt_png_encode_u8: image %d: a segment or the zlib stream could pass 2^31 - 8 bytes", i);
    return 0;
}

}  // namespace tt

using namespace tt;

extern "C" int tt_png_encode_u8_phases(const uint8_t* pixels_dev, long long pixel_bytes, const tt_png_enc_image* images_host,
                                       const tt_png_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                                       uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, int phases, void* stream) {
    if (check_file_table<PngSlots>("tt_png_encode_u8", "tt_png_encode_bound", pixels_dev, pixel_bytes, images_host, images_dev, num_images,
                                   workspace, files_dev, files_bytes, file_sizes_dev, png_image_check))
        return -1;
    EncLayout L;
    TT_REQUIRE(enc_layout(images_host, num_images, L), "tt_png_encode_u8: more than 2^31 - 1 rows, segments or checksum tiles");
    TT_REQUIRE(workspace_bytes >= L.total, "tt_png_encode_u8: need %lld bytes of workspace, got %lld", L.total, workspace_bytes);

    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    int32_t* sizes = (int32_t*)(ws + L.t.sizes);
    long long* seg_at = (long long*)(ws + L.t.part_at);
    long long* payload = (long long*)(ws + L.payload);
    int* first_tile = (int*)(ws + L.first_tile);
    tt_cksum::Tile* tiles = (tt_cksum::Tile*)(ws + L.tile_table);
    tt_cksum::Partial* parts = (tt_cksum::Partial*)(ws + L.parts);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)L.t.units), dim3(enc::kLanes), 0, st, pixels_dev, images_dev, num_images, ws);
    if (phases < 2) return check_launch("tt_png_encode_u8");
    hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)L.t.parts), dim3(enc::kLanes), 0, st, images_dev, num_images, ws, sizes);
    if (phases < 3) return check_launch("tt_png_encode_u8");
    hipLaunchKernelGGL(png_layout_kernel, dim3((unsigned)div_up(num_images, enc::kLanes)), dim3(enc::kLanes), 0, st, images_dev, num_images,
                       sizes, seg_at, payload, files_dev, file_sizes_dev);
    hipLaunchKernelGGL(png_compact_kernel, dim3((unsigned)L.t.parts), dim3(kCopyLanes), 0, st, images_dev, num_images, ws, sizes, seg_at,
                       files_dev);
    const EncRanges src{images_dev, payload, num_images};
    hipLaunchKernelGGL(checksum_plan_kernel<EncRanges>, dim3(1), dim3(tt_cksum::kLanes), 0, st, src, L.num_ranges, first_tile, tiles, L.tiles);
    checksum_launch_tiles(ws, L.t.regions, files_dev, files_bytes, num_images, tiles, L.adler_tiles, parts, st);
    hipLaunchKernelGGL(png_encode_fold_kernel, dim3((unsigned)div_up(num_images, tt_cksum::kLanes)), dim3(tt_cksum::kLanes), 0, st, src, 0,
                       num_images, first_tile, parts, L.tiles, files_dev, checksum_pow_table());
    checksum_launch_tiles(ws, L.t.regions, files_dev, files_bytes, num_images, tiles + L.adler_tiles, L.tiles - L.adler_tiles,
                          parts + L.adler_tiles, st);
    hipLaunchKernelGGL(png_encode_fold_kernel, dim3((unsigned)div_up(3 * num_images, tt_cksum::kLanes)), dim3(tt_cksum::kLanes), 0, st, src,
                       num_images, L.num_ranges, first_tile, parts, L.tiles, files_dev, checksum_pow_table());
    return check_launch("tt_png_encode_u8");
}

extern "C" long long tt_png_encode_bound(const tt_png_enc_image* images_host, int num_images) {
    return slots::bound_sum<PngSlots>(images_host, num_images);
}

extern "C" long long tt_png_encode_workspace_bytes(const tt_png_enc_image* images_host, int num_images) {
    EncLayout L;
    return enc_layout(images_host, num_images, L) ? L.total : 0;
}

extern "C" int tt_png_encode_u8(const uint8_t* pixels_dev, long long pixel_bytes, const tt_png_enc_image* images_host,
                                const tt_png_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                                uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, void* stream) {
    return tt_png_encode_u8_phases(pixels_dev, pixel_bytes, images_host, images_dev, num_images, workspace, workspace_bytes, files_dev,
                                   files_bytes, file_sizes_dev, 3, stream);
}
