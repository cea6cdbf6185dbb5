// The launches of png_checksum.h's functions that csrc/checksum.hip (tt_checksum_ranges_u8) and csrc/png.hip
// (tt_png_decode_u8_verified) share: the plan kernel, which builds the tile table on the device from whatever table of ranges
// the caller holds there, and the tile kernel.  No workgroup waits for another; every loop is bounded by a count or a length
// from a table the entry has validated on the host.
#pragma once
#include "tt_common.h"
#include "png_checksum.h"

namespace tt {

// One workgroup: lane l plans the l-th run of ranges.  The host has sized `tiles` from its own copy of the same table
// (capacity = its plan_ranges count); nothing is written beyond it if the device's copy disagrees.
template <typename Source>
__global__ __launch_bounds__(tt_cksum::kLanes) void checksum_plan_kernel(Source src, int num_ranges, int* __restrict__ first_tile,
                                                                         tt_cksum::Tile* __restrict__ tiles, long long capacity) {
    __shared__ long long s_first[tt_cksum::kLanes];
    const int lane = (int)threadIdx.x;
    s_first[lane] = tt_cksum::plan_count(src, num_ranges, lane, tt_cksum::kLanes);
    __syncthreads();
    if (lane == 0) {
        long long run = 0;
        for (int l = 0; l < tt_cksum::kLanes; ++l) {
            const long long c = s_first[l];
            s_first[l] = run;
            run += c;
        }
    }
    __syncthreads();
    tt_cksum::plan_write(src, num_ranges, lane, tt_cksum::kLanes, s_first[lane], first_tile, tiles, capacity);
}

// The powers x^(8 * 2^k), computed once per process by tt_cksum::crc_pow_table.
const tt_cksum::PowTable& checksum_pow_table();

// One workgroup per tile -> parts[tile].  Ranges below num_adler are Adler-32 over adler_base[0, adler_limit), the others
// CRC-32 over crc_base[0, crc_limit); a tile that does not lie inside its buffer gives a zero partial and reads nothing.
void checksum_launch_tiles(const uint8_t* adler_base, long long adler_limit, const uint8_t* crc_base, long long crc_limit,
                           int num_adler, const tt_cksum::Tile* tiles, long long num_tiles, tt_cksum::Partial* parts,
                           hipStream_t stream);

}  // namespace tt
