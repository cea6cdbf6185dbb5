// Adler-32 (RFC 1950) and CRC-32 (reflected polynomial 0xEDB88320, as zlib and PNG use it) over byte ranges, cut into tiles:
// what zlib.adler32(data, value) and zlib.crc32(data, value) return.  Everything but the launch code is here, as plain
// functions over byte spans: csrc/checksum.hip and csrc/png.hip compile them as device code, tools/png_checksum_host_check.cpp
// compiles the same text as host C++, lane by lane, only so that it can run under sanitizers on the CPU.
//
// Work.  A range of n bytes is ceil(n / kTile) tiles (none for n = 0); the tile table (plan_ranges / range_tiles) maps each
// tile to (range, offset, bytes).  One workgroup of kLanes lanes takes one tile; lane l takes the contiguous slice
// [l * kSlice, (l + 1) * kSlice) of it, cut at the tile's end.  A slice gives a partial that is independent of everything
// before it; the lanes' partials are combined into the tile's (tile_combine_*), and fold_* combines a range's tiles in order,
// applies the start value and finishes.  Every loop is bounded by a length from the table.
//
// Adler-32.  With A0, B0 the start value's halves: A = A0 + sum d[i], B = B0 + n * A0 + sum (n - i) * d[i], both mod 65521
// (for the start value 1: A = 1 + sum d, B = n + sum (n - i) d[i]).  A partial is (s1, s2) = (sum d[i], sum (len - i) d[i])
// mod 65521 over its own bytes; a piece of (s1, s2) followed by `after` more bytes adds s2 + after * s1 to the whole's s2.
// Both factors are reduced mod 65521 first: 65520^2 = 4,292,870,400 < 2^32, so the product fits uint32_t.
//
// CRC-32.  A partial is the plain remainder R(M) = M(x) * x^32 mod P of its bytes (register 0 at the start, no final
// inversion), in zlib's reflected form: bit 31 is the coefficient of x^0.  R is linear: R(A || B) = R(A) * x^(8|B|) + R(B).
// zlib's crc32(data, v) over n bytes is ~(R(data) + (~v) * x^(8n)): the start value and the inversion are applied once
// per range, in fold_crc32.  x^(8n) is a product of the powers x^(8 * 2^k), from the table crc_pow_table computes.
#pragma once
#include <stdint.h>

#include "../../include/thinktwice_hip.h"

#include "lanes.h"          // TT_HD

namespace tt_cksum {

constexpr int kTile = TT_CHECKSUM_TILE;
constexpr int kLanes = 256;                 // lanes per tile
// Bytes per lane.  A slice of kSlice bytes 0xFF sums to s1 = 255 * 256 = 65,280 and s2 = 255 * 256 * 257 / 2 = 8,388,480 before
// any reduction: both far below 2^32 (zlib's NMAX, 5552, is the longest such run for uint32_t), so a slice reduces once.
constexpr int kSlice = kTile / kLanes;
static_assert(kSlice * kLanes == kTile && kSlice <= 5552, "a slice must not overflow its uint32_t accumulators");
constexpr uint32_t kBase = 65521u;          // the largest prime below 2^16
constexpr uint32_t kPoly = 0xEDB88320u;
constexpr int kPowers = 64;                 // x^(8 * 2^k), k < 64: any byte count a long long holds

struct Tile {
    long long offset;                       // of the tile's first byte in the data buffer
    int range;
    int bytes;                              // 1 .. kTile
};
struct Partial {
    uint32_t lo, hi;                        // Adler-32: s1, s2.  CRC-32: the remainder, 0.
};
struct PowTable {
    uint32_t p[kPowers];
};

TT_HD inline long long tiles_of(long long bytes) { return bytes <= 0 ? 0 : (bytes + kTile - 1) / kTile; }

// The tiles of one range, in order, at tiles[first ...); nothing is written at or beyond tiles[capacity].
TT_HD inline void range_tiles(Tile* tiles, long long first, long long capacity, int range, long long offset, long long bytes) {
    long long t = first;
    for (long long o = 0; o < bytes && t < capacity; o += kTile, ++t) {
        const long long left = bytes - o;
        Tile e;
        e.offset = offset + o;
        e.range = range;
        e.bytes = (int)(left < kTile ? left : kTile);
        tiles[t] = e;
    }
}

// The table builder, for `nlanes` callers that share the ranges out in contiguous runs.  A Source gives bytes(r) and
// offset(r) of range r.  plan_count: the tiles of this lane's ranges.  plan_write, once every lane's count is known and
// `first` is the sum of the counts of the lanes below: first_tile[r] for the lane's ranges (a zero-length range keeps its
// entry and owns no tile) and their tiles.  The host builds the table with one lane of one (plan_ranges).
struct RangeTable {
    const tt_checksum_range* ranges;
    TT_HD long long bytes(int r) const { return ranges[r].bytes; }
    TT_HD long long offset(int r) const { return ranges[r].offset; }
};

template <typename Source>
TT_HD inline long long plan_count(const Source& src, int num_ranges, int lane, int nlanes) {
    const int per = (num_ranges + nlanes - 1) / nlanes;
    const long long lo = (long long)lane * per, hi = lo + per < num_ranges ? lo + per : num_ranges;
    long long count = 0;
    for (long long r = lo; r < hi; ++r) count += tiles_of(src.bytes((int)r));
    return count;
}

template <typename Source>
TT_HD inline void plan_write(const Source& src, int num_ranges, int lane, int nlanes, long long first, int* first_tile, Tile* tiles,
                             long long capacity) {
    const int per = (num_ranges + nlanes - 1) / nlanes;
    const long long lo = (long long)lane * per, hi = lo + per < num_ranges ? lo + per : num_ranges;
    for (long long r = lo; r < hi; ++r) {
        const long long bytes = src.bytes((int)r);
        first_tile[r] = (int)first;
        range_tiles(tiles, first, capacity, (int)r, src.offset((int)r), bytes);
        first += tiles_of(bytes);
    }
}

// The number of tiles; first_tile and tiles (`capacity` entries, none needed for 0) are written unless first_tile is null.
template <typename Source>
TT_HD inline long long plan_ranges(const Source& src, int num_ranges, int* first_tile, Tile* tiles, long long capacity) {
    if (first_tile) plan_write(src, num_ranges, 0, 1, 0, first_tile, tiles, capacity);
    return plan_count(src, num_ranges, 0, 1);
}

// ---------------------------------------------------------------------------------------------------------------- slices
// Bytes [0, n) of p, n <= kSlice: single bytes up to a 4-byte boundary, whole words, single bytes.
TT_HD inline Partial adler_slice(const uint8_t* p, int n) {
    uint32_t a = 0, b = 0;
    int i = 0;
    for (; i < n && ((uintptr_t)(p + i) & 3u); ++i) {
        a += p[i];
        b += a;
    }
    for (; i + 4 <= n; i += 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p + i);
        a += w & 255u;
        b += a;
        a += (w >> 8) & 255u;
        b += a;
        a += (w >> 16) & 255u;
        b += a;
        a += w >> 24;
        b += a;
    }
    for (; i < n; ++i) {
        a += p[i];
        b += a;
    }
    Partial r;
    r.lo = a % kBase;
    r.hi = b % kBase;
    return r;
}

// Entry b of the byte table: the remainder of the one byte b.
TT_HD inline uint32_t crc_table_entry(uint32_t b) {
    for (int k = 0; k < 8; ++k) b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
    return b;
}

// table: the 256 entries of crc_table_entry (LDS on the device)
TT_HD inline Partial crc_slice(const uint8_t* p, int n, const uint32_t* table) {
    uint32_t c = 0;
    int i = 0;
    for (; i < n && ((uintptr_t)(p + i) & 3u); ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8);
    for (; i + 4 <= n; i += 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p + i);
        c = table[(c ^ w) & 255u] ^ (c >> 8);
        c = table[(c ^ (w >> 8)) & 255u] ^ (c >> 8);
        c = table[(c ^ (w >> 16)) & 255u] ^ (c >> 8);
        c = table[(c ^ (w >> 24)) & 255u] ^ (c >> 8);
    }
    for (; i < n; ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8);
    Partial r;
    r.lo = c;
    r.hi = 0;
    return r;
}

// --------------------------------------------------------------------------------------------------------------- GF(2)[x]/P
// a * b mod P in the reflected form (0x80000000 is x^0): 32 steps.
TT_HD inline uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 31; k >= 0; --k) {
        if ((a >> k) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}

// The one place the powers come from: p[k] = x^(8 * 2^k) mod P.  x^8 is bit 31 - 8.
inline void crc_pow_table(PowTable& t) {
    t.p[0] = 0x00800000u;
    for (int k = 1; k < kPowers; ++k) t.p[k] = crc_mul(t.p[k - 1], t.p[k - 1]);
}

// x^(8 * bytes) mod P, bytes >= 0: at most kPowers - 1 products.
TT_HD inline uint32_t crc_xpow8(const PowTable& t, long long bytes) {
    uint32_t p = 0x80000000u;
    unsigned long long n = (unsigned long long)bytes;
    for (int k = 0; k < kPowers && n; ++k, n >>= 1)
        if (n & 1u) p = crc_mul(t.p[k], p);
    return p;
}

// --------------------------------------------------------------------------------------------------------------- combining
// What the piece `part`, followed by `after` more bytes of the same whole, adds to the whole's partial.  Adler-32: to (s1, s2),
// each term below 65521 (a sum of kLanes of them stays below 2^24).  CRC-32: to the remainder, by xor.
TT_HD inline Partial adler_shift(Partial part, long long after) {
    Partial r;
    r.lo = part.lo;
    r.hi = (part.hi + (uint32_t)(after % kBase) * part.lo) % kBase;       // both factors < 65521: the product fits
    return r;
}

TT_HD inline uint32_t crc_shift(const PowTable& t, uint32_t part, long long after) { return crc_mul(part, crc_xpow8(t, after)); }

// The tile's partial from its lanes' (slices[l] covers bytes [l * kSlice, ...) of a tile of `bytes` bytes): the serial
// statement of what the workgroup's reduction computes.
TT_HD inline Partial tile_combine_adler(const Partial* slices, int bytes) {
    uint32_t s1 = 0, s2 = 0;
    for (int l = 0; l * kSlice < bytes; ++l) {
        const int end = (l + 1) * kSlice < bytes ? (l + 1) * kSlice : bytes;
        const Partial c = adler_shift(slices[l], bytes - end);
        s1 += c.lo;
        s2 += c.hi;
    }
    Partial r;
    r.lo = s1 % kBase;
    r.hi = s2 % kBase;
    return r;
}

TT_HD inline Partial tile_combine_crc(const PowTable& t, const Partial* slices, int bytes) {
    uint32_t c = 0;
    for (int l = 0; l * kSlice < bytes; ++l) {
        const int end = (l + 1) * kSlice < bytes ? (l + 1) * kSlice : bytes;
        c ^= crc_shift(t, slices[l].lo, bytes - end);
    }
    Partial r;
    r.lo = c;
    r.hi = 0;
    return r;
}

// --------------------------------------------------------------------------------------------------------------- the fold
// A range of `bytes` bytes whose tiles' partials are parts[0 .. tiles_of(bytes)), in order; start: zlib's second argument.
TT_HD inline uint32_t fold_adler32(const Partial* parts, long long bytes, uint32_t start) {
    uint32_t s1 = 0, s2 = 0;
    const long long n = tiles_of(bytes);
    for (long long t = 0; t < n; ++t) {
        const long long len = t + 1 < n ? kTile : bytes - t * kTile;
        s2 = (s2 + (uint32_t)(len % kBase) * s1 + parts[t].hi) % kBase;     // s1 < 65521: the product fits, the sum is below 2^32
        s1 = (s1 + parts[t].lo) % kBase;
    }
    const uint32_t a0 = (start & 0xffffu) % kBase, b0 = (start >> 16) % kBase;
    const uint32_t a = (a0 + s1) % kBase;
    const uint32_t b = (uint32_t)(((unsigned long long)b0 + (unsigned long long)(bytes % kBase) * a0 + s2) % kBase);
    return (b << 16) | a;
}

TT_HD inline uint32_t fold_crc32(const PowTable& t, const Partial* parts, long long bytes, uint32_t start) {
    uint32_t c = 0;
    const long long n = tiles_of(bytes);
    for (long long i = 0; i < n; ++i) {
        const long long len = i + 1 < n ? kTile : bytes - i * kTile;
        c = crc_mul(c, crc_xpow8(t, len)) ^ parts[i].lo;
    }
    return ~(c ^ crc_mul(~start, crc_xpow8(t, bytes)));
}

}  // namespace tt_cksum
