// tt_png_decode_u8 with the streams' Adler-32 and the IDAT chunks' CRC-32 verified on the device (thinktwice_hip.h,
// tt_png_decode_u8_verified).  Launch order: the tile plan (it needs only the tables), the inflate, which also hands out each
// stream's Adler-32 field, the checksum tiles over every image's scanlines and every chunk's body (csrc/checksum.hip), fold +
// compare + status, the unfilter.  The unfilter returns at once for an image whose status is not TT_PNG_OK, which is what
// leaves a failed image's destination untouched.  No workgroup waits for another.
//
// A translation unit of its own: csrc/png.hip's kernels, which tt_png_decode_u8 launches, stay compiled as they were.
#include <limits.h>

#include "tt_common.h"          // (first: png_inflate.h's barrier is the HIP runtime's)
#include "png_inflate.h"
#include "png_launch.h"
#include "checksum_launch.h"

namespace tt {

// png.hip's inflate kernel, and trailer[img] = the stream's Adler-32 field where the status is TT_PNG_OK.
__global__ __launch_bounds__(64) void png_inflate_trailer_kernel(const uint8_t* __restrict__ packed, long long packed_bytes,
                                                                 const tt_png_image* __restrict__ images, uint8_t* __restrict__ ws,
                                                                 int32_t* __restrict__ status, uint32_t* __restrict__ trailer) {
    __shared__ tt_png::State S;
    const int img = (int)blockIdx.x, lane = (int)threadIdx.x;
    const tt_png_image im = images[img];
    const long long off = png_slot_offset(images, img);
    const int skew = (int)(im.stream_offset & 3);                // `packed` is 16-byte aligned: read from the word the stream starts in
    const long long word0 = im.stream_offset - skew;
    const int st = tt_png::inflate_zlib(S, packed + word0, skew, skew + (int)im.stream_bytes, packed_bytes - word0, ws + off,
                                        (int)png_expect(im), lane, kWave, trailer + img);
    if (lane == 0) status[img] = st;
}

// The ranges of one verified call: with TT_PNGV_ADLER32 the scanlines of every image in the workspace (ranges 0 .. num_adler),
// then, with TT_PNGV_CRC32, every IDAT body in `packed`.
struct PngRanges {
    const tt_png_image* images;
    const tt_png_chunk* chunks;
    int num_adler;
    __host__ __device__ long long bytes(int r) const { return r < num_adler ? png_expect(images[r]) : chunks[r - num_adler].bytes; }
    __host__ __device__ long long offset(int r) const {
        if (r >= num_adler) return chunks[r - num_adler].offset;
        long long off = 0;                                       // the slot of image r: the sum of the earlier slots
        for (int j = 0; j < r; ++j) off += png_slot(images[j]);
        return off;
    }
};

// zlib.crc32(b"IDAT"): the running value every IDAT body starts from
static uint32_t png_crc_of_idat() {
    uint32_t c = ~0u;
    for (const char* p = "IDAT"; *p; ++p) c = tt_cksum::crc_table_entry((c ^ (uint8_t)*p) & 255u) ^ (c >> 8);
    return ~c;
}

// One lane per range: fold its tiles, compare with the stream's trailer or the chunk's CRC field, and raise the image's
// status if the inflate left it at TT_PNG_OK.  TT_PNGV_BAD_CRC32 > TT_PNGV_BAD_ADLER32, so the maximum is the precedence.
__global__ __launch_bounds__(tt_cksum::kLanes) void png_verify_fold_kernel(PngRanges src, int num_ranges, int num_images,
                                                                           const int* __restrict__ first_tile,
                                                                           const tt_cksum::Partial* __restrict__ parts,
                                                                           long long num_tiles, const uint32_t* __restrict__ trailer,
                                                                           uint32_t crc_start, int32_t* status, tt_cksum::PowTable pow) {
    const long long r = (long long)blockIdx.x * tt_cksum::kLanes + threadIdx.x;
    if (r >= num_ranges) return;
    const bool adler = r < src.num_adler;
    const int img = adler ? (int)r : src.chunks[r - src.num_adler].image;
    if (img < 0 || img >= num_images) return;
    const int before = __hip_atomic_load(&status[img], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (before != TT_PNG_OK && before != TT_PNGV_BAD_ADLER32 && before != TT_PNGV_BAD_CRC32) return;      // the inflate's own error stays
    const long long bytes = src.bytes((int)r), first = first_tile[r];
    bool ok = bytes >= 0 && first >= 0 && first <= num_tiles - tt_cksum::tiles_of(bytes);
    if (ok) {
        const uint32_t want = adler ? trailer[r] : src.chunks[r - src.num_adler].crc;
        const uint32_t got = adler ? tt_cksum::fold_adler32(parts + first, bytes, 1u) : tt_cksum::fold_crc32(pow, parts + first, bytes, crc_start);
        ok = got == want;
    }
    if (!ok) atomicMax(&status[img], adler ? (int)TT_PNGV_BAD_ADLER32 : (int)TT_PNGV_BAD_CRC32);
}

struct PngVerifyLayout {
    long long scanlines, trailer, first_tile, tile_table, parts, total, tiles;
    int num_adler, num_ranges;
};

// The chunk table's checks and the workspace's layout: 0, or -1 with the error text set.  images_host has passed
// png_sizes_ok and the stream checks of png_check_args.
static int png_verify_layout(const tt_png_image* images_host, int num_images, const tt_png_chunk* chunks_host, int num_chunks,
                             int flags, PngVerifyLayout& L) {
    TT_REQUIRE((flags & ~(TT_PNGV_ADLER32 | TT_PNGV_CRC32)) == 0, "tt_png_decode_u8_verified: unknown bits in verify_flags %d", flags);
    const bool crc = flags & TT_PNGV_CRC32;
    L = PngVerifyLayout{};
    L.scanlines = tt_png_workspace_bytes(images_host, num_images);
    TT_REQUIRE(L.scanlines > 0, "tt_png_decode_u8_verified: an image table that tt_png_decode_u8 refuses");
    L.num_adler = (flags & TT_PNGV_ADLER32) ? num_images : 0;
    for (int i = 0; i < L.num_adler; ++i) L.tiles += tt_cksum::tiles_of(png_expect(images_host[i]));
    if (crc) {
        TT_REQUIRE(chunks_host, "tt_png_decode_u8_verified: TT_PNGV_CRC32 without a chunk table");
        TT_REQUIRE(num_chunks >= 1 && num_chunks <= TT_PNG_MAX_CHUNKS, "tt_png_decode_u8_verified: %d chunks, 1..%d", num_chunks,
                   TT_PNG_MAX_CHUNKS);
        int img = -1;
        long long at = 0;                                        // where the next chunk of image `img` must start
        for (int j = 0; j < num_chunks; ++j) {
            const tt_png_chunk& c = chunks_host[j];
            TT_REQUIRE(c.image >= 0 && c.image < num_images, "tt_png_decode_u8_verified: chunk %d belongs to image %d of %d", j, c.image,
                       num_images);
            TT_REQUIRE(c.image == img || c.image == img + 1, "tt_png_decode_u8_verified: chunk %d of image %d follows image %d's: the "
                       "table lists every image's chunks, image by image", j, c.image, img);
            if (c.image != img) {
                TT_REQUIRE(img < 0 || at == images_host[img].stream_offset + images_host[img].stream_bytes,
                           "tt_png_decode_u8_verified: the chunks of image %d end at byte %lld, its stream at %lld", img, at,
                           img < 0 ? 0LL : images_host[img].stream_offset + images_host[img].stream_bytes);
                img = c.image;
                at = images_host[img].stream_offset;
            }
            TT_REQUIRE(c.bytes >= 0 && c.offset == at && c.bytes <= images_host[img].stream_offset + images_host[img].stream_bytes - at,
                       "tt_png_decode_u8_verified: chunk %d: [%lld, +%lld) does not continue image %d's stream at byte %lld or runs "
                       "past its end", j, c.offset, c.bytes, img, at);
            at += c.bytes;
            L.tiles += tt_cksum::tiles_of(c.bytes);
        }
        TT_REQUIRE(img == num_images - 1 && at == images_host[img].stream_offset + images_host[img].stream_bytes,
                   "tt_png_decode_u8_verified: the chunk table ends inside image %d of %d", img, num_images);
    }
    L.num_ranges = L.num_adler + (crc ? num_chunks : 0);
    TT_REQUIRE(L.tiles <= INT_MAX, "tt_png_decode_u8_verified: more than 2^31 - 1 checksum tiles");
    const auto up = [](long long n) { return (n + kPngSlotAlign - 1) / kPngSlotAlign * kPngSlotAlign; };
    L.trailer = L.scanlines;
    L.first_tile = L.trailer + up(4LL * num_images);
    L.tile_table = L.first_tile + up(4LL * L.num_ranges);
    L.parts = L.tile_table + up((long long)sizeof(tt_cksum::Tile) * L.tiles);
    L.total = flags ? L.parts + up((long long)sizeof(tt_cksum::Partial) * L.tiles) : L.scanlines;
    return 0;
}

}  // namespace tt

using namespace tt;

// what both entries ask of the workspace: the verified layout, then one int32 per segment (png_segments.hip)
long long tt::png_verified_workspace_bytes(const tt_png_image* images_host, int num_images, const tt_png_chunk* chunks_host,
                                           int num_chunks, int verify_flags, int num_segments, long long* segment_status_at) {
    PngVerifyLayout L;
    if (png_verify_layout(images_host, num_images, chunks_host, num_chunks, verify_flags, L)) return 0;
    if (segment_status_at) *segment_status_at = L.total;
    return L.total + (4LL * num_segments + kPngSlotAlign - 1) / kPngSlotAlign * kPngSlotAlign;
}

extern "C" long long tt_png_verify_workspace_bytes(const tt_png_image* images_host, int num_images, const tt_png_chunk* chunks_host,
                                                   int num_chunks, int verify_flags) {
    return png_verified_workspace_bytes(images_host, num_images, chunks_host, num_chunks, verify_flags, 0, nullptr);
}

// tt_png_decode_u8_verified, and with `seg` tt_png_decode_u8_segmented (png_segments.hip, which has checked the table): the
// inflate launch is then the segmented one, everything after it is the same.  phases 1: stop after the inflate.
int tt::png_decode_verified(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                            const tt_png_image* images_dev, int num_images, const tt_png_chunk* chunks_host,
                            const tt_png_chunk* chunks_dev, int num_chunks, int verify_flags, const PngSegments* seg, void* workspace,
                            long long workspace_bytes, uint8_t* out_base, long long out_bytes, int32_t* status_dev, int phases,
                            void* stream) {
    if (png_check_args(packed_dev, packed_bytes, images_host, images_dev, num_images, workspace, out_base, out_bytes, status_dev))
        return -1;
    PngVerifyLayout L;
    if (png_verify_layout(images_host, num_images, chunks_host, num_chunks, verify_flags, L)) return -1;
    const bool crc = verify_flags & TT_PNGV_CRC32;
    TT_REQUIRE(!crc || (chunks_dev && ((uintptr_t)chunks_dev & 7) == 0), "tt_png_decode_u8_verified: TT_PNGV_CRC32 needs the device's "
               "chunk table, 8-byte aligned");
    for (int j = 0; crc && j < num_chunks; ++j)                  // (inside its image's stream, which is inside packed_bytes)
        TT_REQUIRE(chunks_host[j].offset >= 0 && chunks_host[j].offset <= packed_bytes - chunks_host[j].bytes,
                   "tt_png_decode_u8_verified: chunk %d outside the %lld packed bytes", j, packed_bytes);
    const long long total = L.total + (seg ? (4LL * seg->count + kPngSlotAlign - 1) / kPngSlotAlign * kPngSlotAlign : 0);
    TT_REQUIRE(workspace_bytes >= total, "tt_png_decode_u8: need %lld bytes of workspace, got %lld", total, workspace_bytes);

    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    int32_t* segment_status = (int32_t*)(ws + L.total);
    if (verify_flags != 0) {
        uint32_t* trailer = (uint32_t*)(ws + L.trailer);
        int* first_tile = (int*)(ws + L.first_tile);
        tt_cksum::Tile* tiles = (tt_cksum::Tile*)(ws + L.tile_table);
        tt_cksum::Partial* parts = (tt_cksum::Partial*)(ws + L.parts);
        const PngRanges src{images_dev, chunks_dev, L.num_adler};
        static const uint32_t crc_start = png_crc_of_idat();
        hipLaunchKernelGGL(checksum_plan_kernel<PngRanges>, dim3(1), dim3(tt_cksum::kLanes), 0, st, src, L.num_ranges, first_tile, tiles,
                           L.tiles);
        if (seg)
            png_launch_segmented_inflate(packed_dev, packed_bytes, images_dev, num_images, *seg, ws, segment_status, status_dev, trailer, st);
        else
            hipLaunchKernelGGL(png_inflate_trailer_kernel, dim3((unsigned)num_images), dim3(kWave), 0, st, packed_dev, packed_bytes,
                               images_dev, ws, status_dev, trailer);
        if (phases < 2) return check_launch("tt_png_decode_u8");
        checksum_launch_tiles(ws, L.scanlines, packed_dev, packed_bytes, L.num_adler, tiles, L.tiles, parts, st);
        hipLaunchKernelGGL(png_verify_fold_kernel, dim3((unsigned)div_up(L.num_ranges, tt_cksum::kLanes)), dim3(tt_cksum::kLanes), 0, st,
                           src, L.num_ranges, num_images, first_tile, parts, L.tiles, trailer, crc_start, status_dev,
                           checksum_pow_table());
    } else if (seg) {
        png_launch_segmented_inflate(packed_dev, packed_bytes, images_dev, num_images, *seg, ws, segment_status, status_dev, nullptr, st);
        if (phases < 2) return check_launch("tt_png_decode_u8");
    }
    png_launch_unverified(packed_dev, packed_bytes, images_dev, num_images, ws, out_base, status_dev, verify_flags == 0 && !seg, st);
    return check_launch("tt_png_decode_u8");
}

extern "C" int tt_png_decode_u8_verified(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                                         const tt_png_image* images_dev, int num_images, const tt_png_chunk* chunks_host,
                                         const tt_png_chunk* chunks_dev, int num_chunks, int verify_flags, void* workspace,
                                         long long workspace_bytes, uint8_t* out_base, long long out_bytes, int32_t* status_dev,
                                         void* stream) {
    return png_decode_verified(packed_dev, packed_bytes, images_host, images_dev, num_images, chunks_host, chunks_dev, num_chunks,
                               verify_flags, nullptr, workspace, workspace_bytes, out_base, out_bytes, status_dev, 2, stream);
}
