// Stand-alone checker of thinktwice_amd/csrc/jpeg_core.h on the CPU: the same source the device kernels run, with one thread
// playing the 64 lanes, over the case file tests/jpeg_encode_cases.py::write_case_file writes.  Every case is encoded to a
// complete JPEG file (the bytes tt_jpeg_encode_u8 writes) the way the device does it: every block transformed on its own, every
// restart interval coded into its own slot, the header, then the intervals copied behind it.  Every buffer is a heap block of
// the exact size between two runs of guard bytes: a build with -fsanitize=address,undefined sees any access outside the
// pixels, the coefficients, an interval's slot or the file, and the guards are checked for a stray write that stays inside the
// heap block.
//
//   jpeg_encode_host_check <case file> <output directory>
//       writes <output directory>/<case index>.jpg and prints per case "ok   <name>: bytes B intervals N bound M";
//       exit 0 if every case stayed inside its bounds and its guards
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../thinktwice_amd/csrc/jpeg_core.h"

namespace jpg = tt_jpeg;

constexpr int kGuard = 64;
constexpr uint8_t kGuardByte = 0xA5;

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static uint8_t* guarded(long long n) {
    uint8_t* p = (uint8_t*)malloc((size_t)n + 2 * kGuard);
    memset(p, kGuardByte, (size_t)n + 2 * kGuard);
    return p + kGuard;
}
static bool guards_ok(const uint8_t* p, long long n) {
    for (int i = 0; i < kGuard; ++i)
        if (p[-1 - i] != kGuardByte || p[n + i] != kGuardByte) return false;
    return true;
}
static void release(uint8_t* p) { free(p - kGuard); }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <case file> <output directory>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    char magic[8];
    int32_t count = 0;
    if (!f || !read_exact(f, magic, 8) || memcmp(magic, "TTJPGE01", 8) != 0 || !read_exact(f, &count, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    jpg::State* S = new jpg::State;
    const jpg::Lanes L{0, jpg::kLanes};
    int failed = 0;
    for (int i = 0; i < count; ++i) {
        int32_t name_len = 0, p[6];
        if (!read_exact(f, &name_len, 4) || name_len < 0 || name_len > 4096) return 2;
        std::string name((size_t)name_len, ' ');
        if (!read_exact(f, &name[0], (size_t)name_len) || !read_exact(f, p, 24)) return 2;
        const int H = p[0], W = p[1], C = p[2], quality = p[3], sub = p[4], rr = p[5];
        if (H < 1 || W < 1 || H > jpg::kMaxDim || W > jpg::kMaxDim || (C != 1 && C != 3) || quality < 1 || quality > 100 ||
            (sub != TT_JPEG_444 && sub != TT_JPEG_420) || rr < 1)
            return 2;
        const jpg::Geom g = jpg::geom(H, W, C, sub, rr);
        if (g.dri > 65535) return 2;
        const long long image = (long long)H * W * C;
        uint8_t* pixels = guarded(image);
        if (!read_exact(f, pixels, (size_t)image)) return 2;

        uint16_t q[128];
        jpg::fill_quant(q, quality, L);
        uint8_t* coef_bytes = guarded(g.blocks * 128);
        int16_t* coefs = (int16_t*)coef_bytes;
        for (long long b = 0; b < g.blocks; ++b) jpg::transform_block(pixels, H, W, g, b, q, coefs + b * 64);

        std::vector<uint8_t*> slots((size_t)g.nint);
        std::vector<long long> sizes((size_t)g.nint), caps((size_t)g.nint);
        long long total = 0;
        bool ok = true;
        for (int k = 0; k < g.nint; ++k) {
            const long long n = jpg::interval_blocks(g, rr, k), cap = jpg::interval_slot_bytes(n);
            slots[(size_t)k] = guarded(cap);
            caps[(size_t)k] = cap;
            const long long got = jpg::encode_interval(*S, coefs + jpg::interval_first_block(g, rr, k) * 64, n, g.bpm, slots[(size_t)k], cap,
                                                       k == g.nint - 1 ? jpg::kEoi : jpg::kRst0 + (k & 7), L);
            ok = ok && got >= 2 && got <= jpg::interval_bound(n) && guards_ok(slots[(size_t)k], cap);
            sizes[(size_t)k] = got;
            total += got;
        }
        const long long bytes = g.header + total, bound = jpg::file_bound(g);
        ok = ok && bytes <= bound && guards_ok(pixels, image) && guards_ok(coef_bytes, g.blocks * 128);
        uint8_t* file = guarded(bytes);
        ok = ok && jpg::write_header(file, H, W, quality, g) == g.header;
        long long at = g.header;
        for (int k = 0; k < g.nint; ++k) {
            memcpy(file + at, slots[(size_t)k], (size_t)sizes[(size_t)k]);
            at += sizes[(size_t)k];
        }
        ok = ok && guards_ok(file, bytes);
        const std::string path = std::string(argv[2]) + "/" + std::to_string(i) + ".jpg";
        FILE* o = fopen(path.c_str(), "wb");
        if (!o || fwrite(file, 1, (size_t)bytes, o) != (size_t)bytes) return 2;
        fclose(o);
        printf("%s %s: bytes %lld intervals %d bound %lld header %d\n", ok ? "ok  " : "FAIL", name.c_str(), bytes, g.nint, bound, g.header);
        failed += ok ? 0 : 1;
        for (uint8_t* s : slots) release(s);
        release(pixels);
        release(coef_bytes);
        release(file);
    }
    fclose(f);
    delete S;
    printf("%d cases, %d failed\n", count, failed);
    return failed ? 1 : 0;
}
