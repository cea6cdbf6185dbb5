// Adler-32 and CRC-32 of byte ranges on the device (thinktwice_hip.h, tt_checksum_ranges_u8): three stream-ordered launches.
//
// plan    one workgroup builds the tile table from the device's copy of the ranges (checksum_launch.h).
// tiles   one 256-lane workgroup per tile of TT_CHECKSUM_TILE bytes.  Lane l reads the contiguous 256 bytes l * 256 .. of the
//         tile and keeps its own partial (png_checksum.h: adler_slice, crc_slice); the partial is moved to the tile's end
//         (adler_shift, crc_shift: what the bytes after the slice make of it) and the 256 of them are summed, or xored, in the
//         wave and across the four waves in LDS.  CRC-32's inner loop is the 256-entry byte table, built in LDS by the
//         workgroup itself (lane b computes entry b).
// fold    one lane per range folds its tiles in order, applies the start value and writes out[range].
// A 4.3 MB range is 66 workgroups, whatever the number of ranges in the call.
#include <limits.h>

#include "checksum_launch.h"

namespace tt {

using namespace tt_cksum;

const PowTable& checksum_pow_table() {
    static const PowTable table = [] {
        PowTable t;
        crc_pow_table(t);
        return t;
    }();
    return table;
}

__global__ __launch_bounds__(kLanes) void checksum_tiles_kernel(const uint8_t* __restrict__ adler_base, long long adler_limit,
                                                                const uint8_t* __restrict__ crc_base, long long crc_limit,
                                                                int num_adler, const Tile* __restrict__ tiles,
                                                                Partial* __restrict__ parts, PowTable pow) {
    __shared__ uint32_t s_table[256];
    __shared__ uint32_t s_lo[kLanes / kWave], s_hi[kLanes / kWave];
    const int lane = (int)threadIdx.x;
    const Tile t = tiles[blockIdx.x];
    const bool adler = t.range < num_adler;
    const uint8_t* base = adler ? adler_base : crc_base;
    const long long limit = adler ? adler_limit : crc_limit;
    if (t.bytes < 1 || t.bytes > kTile || t.offset < 0 || t.offset > limit - t.bytes) {       // (uniform) not a tile of the buffer
        if (lane == 0) parts[blockIdx.x] = Partial{0u, 0u};
        return;
    }
    const int lo = lane * kSlice;
    const int n = t.bytes - lo < 0 ? 0 : (t.bytes - lo < kSlice ? t.bytes - lo : kSlice);
    const long long after = t.bytes - (lo + n);
    uint32_t x = 0, y = 0;
    if (adler) {
        if (n > 0) {
            const Partial p = adler_shift(adler_slice(base + t.offset + lo, n), after);
            x = p.lo;
            y = p.hi;
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            x += __shfl_xor(x, o, kWave);
            y += __shfl_xor(y, o, kWave);
        }
    } else {
        s_table[lane] = crc_table_entry((uint32_t)lane);
        __syncthreads();
        if (n > 0) x = crc_shift(pow, crc_slice(base + t.offset + lo, n, s_table).lo, after);
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) x ^= __shfl_xor(x, o, kWave);
    }
    if ((lane & (kWave - 1)) == 0) {
        s_lo[lane / kWave] = x;
        s_hi[lane / kWave] = y;
    }
    __syncthreads();
    if (lane == 0) {
        Partial r{0u, 0u};
        for (int w = 0; w < kLanes / kWave; ++w) {
            if (adler) {
                r.lo += s_lo[w];                                  // 256 terms below 65521 each: below 2^24
                r.hi += s_hi[w];
            } else {
                r.lo ^= s_lo[w];
            }
        }
        if (adler) {
            r.lo %= kBase;
            r.hi %= kBase;
        }
        parts[blockIdx.x] = r;
    }
}

void checksum_launch_tiles(const uint8_t* adler_base, long long adler_limit, const uint8_t* crc_base, long long crc_limit,
                           int num_adler, const Tile* tiles, long long num_tiles, Partial* parts, hipStream_t stream) {
    if (num_tiles > 0)
        hipLaunchKernelGGL(checksum_tiles_kernel, dim3((unsigned)num_tiles), dim3(kLanes), 0, stream, adler_base, adler_limit, crc_base,
                           crc_limit, num_adler, tiles, parts, checksum_pow_table());
}

__global__ __launch_bounds__(kLanes) void checksum_fold_kernel(const tt_checksum_range* __restrict__ ranges, int num_ranges, int kind,
                                                               const int* __restrict__ first_tile, const Partial* __restrict__ parts,
                                                               long long num_tiles, const uint32_t* __restrict__ start,
                                                               uint32_t* __restrict__ out, PowTable pow) {
    const long long r = (long long)blockIdx.x * kLanes + threadIdx.x;
    if (r >= num_ranges) return;
    const long long bytes = ranges[r].bytes, first = first_tile[r];
    const bool adler = kind == TT_CHECKSUM_ADLER32;
    const uint32_t from = start ? start[r] : (adler ? 1u : 0u);
    if (bytes < 0 || first < 0 || first > num_tiles - tiles_of(bytes)) {         // the device's table is not the one the host sized for
        out[r] = 0u;
        return;
    }
    out[r] = adler ? fold_adler32(parts + first, bytes, from) : fold_crc32(pow, parts + first, bytes, from);
}

constexpr long long kAlign = 256;
static inline long long up(long long n) { return (n + kAlign - 1) / kAlign * kAlign; }

struct Layout {
    long long tiles, first_tile, tile_table, parts, total;
};

// 0 tiles: a table the entry refuses
static Layout checksum_layout(const tt_checksum_range* ranges, int num_ranges) {
    Layout L{};
    if (!ranges || num_ranges < 1 || num_ranges > TT_CHECKSUM_MAX_RANGES) return L;
    long long tiles = 0;
    for (int r = 0; r < num_ranges; ++r) {
        if (ranges[r].bytes < 0) return L;
        tiles += tiles_of(ranges[r].bytes);
        if (tiles > INT_MAX) return L;
    }
    L.tiles = tiles;
    L.first_tile = 0;
    L.tile_table = up(4LL * num_ranges);
    L.parts = L.tile_table + up((long long)sizeof(Tile) * tiles);
    L.total = L.parts + up((long long)sizeof(Partial) * tiles) + kAlign;      // (never 0 for a valid table)
    return L;
}

}  // namespace tt

using namespace tt;

extern "C" long long tt_checksum_workspace_bytes(const tt_checksum_range* ranges_host, int num_ranges) {
    return checksum_layout(ranges_host, num_ranges).total;
}

extern "C" int tt_checksum_ranges_u8(const uint8_t* data_dev, long long data_bytes, const tt_checksum_range* ranges_host,
                                     const tt_checksum_range* ranges_dev, int num_ranges, int kind, const uint32_t* start_dev_or_null,
                                     uint32_t* out_dev, void* workspace, long long workspace_bytes, void* stream) {
    TT_REQUIRE(data_dev && ranges_host && ranges_dev && out_dev && workspace, "tt_checksum_ranges_u8: null pointer");
    TT_REQUIRE(num_ranges >= 1 && num_ranges <= TT_CHECKSUM_MAX_RANGES, "tt_checksum_ranges_u8: %d ranges, 1..%d", num_ranges,
               TT_CHECKSUM_MAX_RANGES);
    TT_REQUIRE(kind == TT_CHECKSUM_ADLER32 || kind == TT_CHECKSUM_CRC32, "tt_checksum_ranges_u8: kind %d, TT_CHECKSUM_ADLER32 or _CRC32",
               kind);
    TT_REQUIRE(data_bytes >= 0, "tt_checksum_ranges_u8: %lld data bytes", data_bytes);
    TT_REQUIRE(((uintptr_t)ranges_dev & 7) == 0 && ((uintptr_t)out_dev & 3) == 0 && ((uintptr_t)start_dev_or_null & 3) == 0 &&
                   ((uintptr_t)workspace & (kAlign - 1)) == 0,
               "tt_checksum_ranges_u8: misaligned table, start, output or workspace (8, 4, 4, 256 bytes)");
    for (int r = 0; r < num_ranges; ++r) {
        const tt_checksum_range& g = ranges_host[r];
        TT_REQUIRE(g.bytes >= 0, "tt_checksum_ranges_u8: range %d has %lld bytes", r, g.bytes);
        TT_REQUIRE(g.offset >= 0 && g.offset <= data_bytes && g.bytes <= data_bytes - g.offset,
                   "tt_checksum_ranges_u8: range %d: [%lld, +%lld) outside the %lld data bytes", r, g.offset, g.bytes, data_bytes);
    }
    const Layout L = checksum_layout(ranges_host, num_ranges);
    TT_REQUIRE(L.total > 0, "tt_checksum_ranges_u8: more than 2^31 - 1 tiles of %d bytes", TT_CHECKSUM_TILE);
    TT_REQUIRE(workspace_bytes >= L.total, "tt_checksum_ranges_u8: need %lld bytes of workspace, got %lld", L.total, workspace_bytes);

    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    int* first_tile = (int*)(ws + L.first_tile);
    Tile* tiles = (Tile*)(ws + L.tile_table);
    Partial* parts = (Partial*)(ws + L.parts);
    hipLaunchKernelGGL(checksum_plan_kernel<RangeTable>, dim3(1), dim3(kLanes), 0, st, RangeTable{ranges_dev}, num_ranges, first_tile,
                       tiles, L.tiles);
    const int num_adler = kind == TT_CHECKSUM_ADLER32 ? num_ranges : 0;
    checksum_launch_tiles(data_dev, data_bytes, data_dev, data_bytes, num_adler, tiles, L.tiles, parts, st);
    hipLaunchKernelGGL(checksum_fold_kernel, dim3((unsigned)div_up(num_ranges, kLanes)), dim3(kLanes), 0, st, ranges_dev, num_ranges, kind,
                       first_tile, parts, L.tiles, start_dev_or_null, out_dev, checksum_pow_table());
    return check_launch("tt_checksum_ranges_u8");
}
