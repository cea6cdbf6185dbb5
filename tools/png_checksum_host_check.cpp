// Stand-alone checker of thinktwice_amd/csrc/png_checksum.h on the CPU, and of the trailer png_inflate.h hands out: the same
// source the device kernels run, lane by lane -- the tile table, every lane's slice, the workgroup's combine, the fold -- over
// the case file tests/png_checksum_cases.py::write_case_file writes.  Every range, stream, chunk body and scanline buffer is
// a heap block of its exact size (each range once more behind a few bytes, so that its first byte keeps the alignment it has
// in the case's buffer): a build with -fsanitize=address,undefined sees any access outside them.
//
//   png_checksum_host_check <case file>      exit 0: every checksum equals the expected value, every stream ends in its status
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../thinktwice_amd/csrc/png_inflate.h"
#include "../thinktwice_amd/csrc/png_checksum.h"

using namespace tt_cksum;

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static PowTable g_pow;
static uint32_t g_table[256];

// What the three launches compute for one range whose bytes are p[0, bytes): plan, one "workgroup" per tile with kLanes
// slices, fold.
static uint32_t range_checksum(int kind, const uint8_t* p, long long bytes, uint32_t start) {
    tt_checksum_range range{0, bytes};
    const RangeTable src{&range};
    const long long count = plan_ranges(src, 1, nullptr, nullptr, 0);
    std::vector<Tile> tiles((size_t)count);
    std::vector<Partial> parts((size_t)count);
    int first = -1;
    if (plan_ranges(src, 1, &first, tiles.data(), count) != count || first != 0) return ~0u;
    for (long long t = 0; t < count; ++t) {
        Partial slices[kLanes];
        for (int lane = 0; lane < kLanes; ++lane) {
            const int lo = lane * kSlice;
            const int n = tiles[t].bytes - lo < 0 ? 0 : (tiles[t].bytes - lo < kSlice ? tiles[t].bytes - lo : kSlice);
            slices[lane] = Partial{0u, 0u};
            if (n > 0) slices[lane] = kind == TT_CHECKSUM_ADLER32 ? adler_slice(p + tiles[t].offset + lo, n) : crc_slice(p + tiles[t].offset + lo, n, g_table);
        }
        parts[(size_t)t] = kind == TT_CHECKSUM_ADLER32 ? tile_combine_adler(slices, tiles[t].bytes) : tile_combine_crc(g_pow, slices, tiles[t].bytes);
    }
    return kind == TT_CHECKSUM_ADLER32 ? fold_adler32(parts.data(), bytes, start) : fold_crc32(g_pow, parts.data(), bytes, start);
}

// The range in a block of its exact size, then behind `skew` bytes.
static bool check_range(int kind, const uint8_t* data, long long offset, long long bytes, uint32_t start, uint32_t want) {
    bool ok = true;
    for (int pass = 0; pass < 2; ++pass) {
        const size_t skew = pass ? (size_t)(offset & 15) : 0;
        uint8_t* block = (uint8_t*)malloc(skew + (size_t)bytes);
        if (bytes) memcpy(block + skew, data + offset, (size_t)bytes);
        ok = ok && range_checksum(kind, block + skew, bytes, start) == want;
        free(block);
    }
    return ok;
}

// The tile table of a whole case: every range's tiles in order, each at most kTile bytes, together exactly the range.
static bool check_plan(const std::vector<tt_checksum_range>& ranges) {
    const RangeTable src{ranges.data()};
    const int n = (int)ranges.size();
    const long long count = plan_ranges(src, n, nullptr, nullptr, 0);
    std::vector<Tile> tiles((size_t)count);
    std::vector<int> first((size_t)n, -1);
    plan_ranges(src, n, first.data(), tiles.data(), count);
    long long t = 0;
    for (int r = 0; r < n; ++r) {
        if (first[(size_t)r] != t) return false;
        long long at = ranges[(size_t)r].offset, left = ranges[(size_t)r].bytes;
        while (left > 0) {
            if (t >= count) return false;
            const Tile& e = tiles[(size_t)t++];
            if (e.range != r || e.offset != at || e.bytes < 1 || e.bytes > kTile || e.bytes > left) return false;
            if (e.bytes < kTile && e.bytes != left) return false;
            at += e.bytes;
            left -= e.bytes;
        }
    }
    if (t != count) return false;
    // the same table from kLanes planners, as the device builds it
    std::vector<Tile> tiles2((size_t)count);
    std::vector<int> first2((size_t)n, -1);
    long long run = 0;
    for (int lane = 0; lane < kLanes; ++lane) {
        const long long c = plan_count(src, n, lane, kLanes);
        plan_write(src, n, lane, kLanes, run, first2.data(), tiles2.data(), count);
        run += c;
    }
    if (run != count || first2 != first) return false;
    for (long long k = 0; k < count; ++k)
        if (tiles2[(size_t)k].offset != tiles[(size_t)k].offset || tiles2[(size_t)k].range != tiles[(size_t)k].range ||
            tiles2[(size_t)k].bytes != tiles[(size_t)k].bytes)
            return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <case file>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    char magic[8];
    int32_t count = 0;
    if (!f || !read_exact(f, magic, 8) || memcmp(magic, "TTCKSC01", 8) != 0 || !read_exact(f, &count, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    crc_pow_table(g_pow);
    for (uint32_t b = 0; b < 256; ++b) g_table[b] = crc_table_entry(b);
    uint32_t crc_idat = ~0u;
    for (const char* p = "IDAT"; *p; ++p) crc_idat = g_table[(crc_idat ^ (uint8_t)*p) & 255u] ^ (crc_idat >> 8);
    crc_idat = ~crc_idat;
    tt_png::State* S = new tt_png::State;
    int failed = 0;
    for (int i = 0; i < count; ++i) {
        int32_t name_len = 0, type = 0;
        if (!read_exact(f, &name_len, 4) || name_len < 0 || name_len > 4096) return 2;
        std::string name((size_t)name_len, ' ');
        if (!read_exact(f, &name[0], (size_t)name_len) || !read_exact(f, &type, 4)) return 2;
        bool ok = true;
        if (type == 0) {
            int32_t kind = 0, num = 0;
            int64_t bytes = 0;
            if (!read_exact(f, &kind, 4) || !read_exact(f, &bytes, 8)) return 2;
            uint8_t* data = (uint8_t*)malloc((size_t)bytes);
            if (!read_exact(f, data, (size_t)bytes) || !read_exact(f, &num, 4)) return 2;
            std::vector<tt_checksum_range> ranges;
            int bad = 0;
            for (int r = 0; r < num; ++r) {
                int64_t ob[2];
                uint32_t sw[2];
                if (!read_exact(f, ob, 16) || !read_exact(f, sw, 8)) return 2;
                ranges.push_back(tt_checksum_range{ob[0], ob[1]});
                if (!check_range(kind, data, ob[0], ob[1], sw[0], sw[1])) ++bad;
            }
            ok = bad == 0 && check_plan(ranges);
            printf("%s %s: %d ranges, %d wrong\n", ok ? "ok  " : "FAIL", name.c_str(), num, bad);
            free(data);
        } else {
            int32_t hwcs[4], chunks = 0;
            int64_t stream_len = 0;
            if (!read_exact(f, hwcs, 16) || !read_exact(f, &stream_len, 8)) return 2;
            uint8_t* stream = (uint8_t*)malloc((size_t)stream_len);
            if (!read_exact(f, stream, (size_t)stream_len) || !read_exact(f, &chunks, 4)) return 2;
            const int H = hwcs[0], W = hwcs[1], C = hwcs[2], expected = hwcs[3];
            const long long expect = (long long)H * (1 + (long long)W * C), image = (long long)H * W * C;
            uint8_t* lines = (uint8_t*)malloc((size_t)expect);
            uint8_t* pixels = (uint8_t*)malloc((size_t)image);
            uint32_t trailer = 0x5a5a5a5au;
            int st = tt_png::inflate_zlib(*S, stream, 0, (int)stream_len, stream_len, lines, (int)expect, 0, 1, &trailer);
            bool crc_ok = true;
            long long at = 0;
            for (int k = 0; k < chunks; ++k) {
                int64_t n = 0;
                uint32_t field = 0;
                if (!read_exact(f, &n, 8) || !read_exact(f, &field, 4)) return 2;
                if (at + n > stream_len) return 2;
                crc_ok = check_range(TT_CHECKSUM_CRC32, stream, at, n, crc_idat, field) && crc_ok;
                at += n;
            }
            if (at != stream_len) return 2;
            if (st == TT_PNG_OK && !crc_ok) st = TT_PNGV_BAD_CRC32;
            if (st == TT_PNG_OK && !check_range(TT_CHECKSUM_ADLER32, lines, 0, expect, 1u, trailer)) st = TT_PNGV_BAD_ADLER32;
            if (st == TT_PNG_OK) st = tt_png::unfilter_serial(lines, H, W, C, pixels);
            ok = st == expected;
            printf("%s %s: status %d, expected %d\n", ok ? "ok  " : "FAIL", name.c_str(), st, expected);
            free(stream);
            free(lines);
            free(pixels);
        }
        failed += ok ? 0 : 1;
    }
    fclose(f);
    delete S;
    printf("%d cases, %d failed\n", count, failed);
    return failed ? 1 : 0;
}
