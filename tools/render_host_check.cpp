// Host checker of the rasteriser: thinktwice_amd/csrc/render_raster.h compiled for the CPU and driven pixel by pixel over the case
// file of tests/render_cases.py (write_case_file states the format).  Build with -ffp-contract=off, and with
// -fsanitize=address,undefined to have every read of a source and every write of the canvas checked: the gaps of a case's blob
// between its live regions are poisoned while the case runs.
//   render_host_check cases.bin out.bin
// out.bin: per case int32 rc, int64 dropped points, then (rc == 0) the Hc * Wc * 3 canvas bytes.  Exit status 0 if every case
// behaved (an error case was refused, the guards and the workspace's planes were left as they must be).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../thinktwice_amd/csrc/render_raster.h"

#if defined(__SANITIZE_ADDRESS__)
#define TT_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define TT_ASAN 1
#endif
#endif
#ifdef TT_ASAN
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#endif

using namespace tt_render;

static const int kGuard = 64;

// the entry's checks and launches, one pixel at a time; -1 where tt_render_u8 returns an error
static int host_render(uint8_t* canvas, int Hc, int Wc, const tt_render_item* items, int n, uint8_t* ws, long long ws_bytes) {
    if (!canvas || !ws || n < 0 || n > TT_RENDER_MAX_ITEMS || (n > 0 && !items)) return -1;
    if (Hc < 1 || Hc > kMaxSide || Wc < 1 || Wc > kMaxSide || ws_bytes < up256(8LL * TT_RENDER_STATUS_WORDS)) return -1;
    long long next = up256(8LL * TT_RENDER_STATUS_WORDS);
    for (int i = 0; i < n; ++i) {
        const char* fault = item_fault(items[i], next, ws_bytes, true);
        if (fault) {
            printf("     refused: ");
            printf(fault, i);
            printf("\n");
            return -1;
        }
    }
    std::vector<PolyFix> poly(n > 0 ? n : 1);
    long long dropped = 0;
    for (int i = 0; i < n; ++i) {
        const tt_render_item& it = items[i];
        if (it.kind == TT_RENDER_POINTS_BEV && it.w > 0 && it.h > 0)
            for (int k = 0; k < it.count; ++k) {
                int word;
                uint32_t val;
                if (splat_target(it, Hc, Wc, k, word, val)) {
                    uint32_t* plane = (uint32_t*)(ws + it.ws_offset);
                    if (plane[word] < val) plane[word] = val;
                }
            }
        if (is_poly(it.kind)) dropped += poly_fix(it, &poly[i]);
    }
    ((long long*)ws)[TT_RENDER_STATUS_DROPPED] += dropped;
    for (int py = 0; py < Hc; ++py)
        for (int px = 0; px < Wc; ++px) {
            uint32_t col = 0;
            for (int i = 0; i < n; ++i) {
                const Box b = item_box(items[i], &poly[i], Hc, Wc);
                if (px < b.x0 || px >= b.x1 || py < b.y0 || py >= b.y1) continue;
                CellCache cc{-1, 0};
                col = shade(items[i], &poly[i], ws, px, py, col, cc);
            }
            uint8_t* out = canvas + ((long long)py * Wc + px) * 3;
            out[0] = (uint8_t)(col & 255u);
            out[1] = (uint8_t)(col >> 8 & 255u);
            out[2] = (uint8_t)(col >> 16 & 255u);
        }
    return 0;
}

template <typename T> static bool get(FILE* f, T& v) { return fread(&v, sizeof(T), 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: render_host_check cases.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    char magic[4];
    int32_t count = 0;
    if (!in || !out || fread(magic, 1, 4, in) != 4 || memcmp(magic, "TTRC", 4) != 0 || !get(in, count)) {
        fprintf(stderr, "cannot read %s or write %s\n", argv[1], argv[2]);
        return 2;
    }
    int failed = 0;
    for (int c = 0; c < count; ++c) {
        int32_t name_len, Hc, Wc, n, expect_error, n_live;
        int64_t ws_bytes, blob_bytes, table_at;
        if (!get(in, name_len)) return 2;
        std::string name(name_len, ' ');
        if (fread(&name[0], 1, name_len, in) != (size_t)name_len) return 2;
        if (!get(in, Hc) || !get(in, Wc) || !get(in, n) || !get(in, expect_error) || !get(in, ws_bytes) || !get(in, blob_bytes) ||
            !get(in, table_at) || !get(in, n_live))
            return 2;
        std::vector<int64_t> live(2 * (size_t)n_live);
        if (n_live && fread(live.data(), 8, live.size(), in) != live.size()) return 2;
        uint8_t* blob = (uint8_t*)aligned_alloc(256, (size_t)up256(blob_bytes));
        if (fread(blob, 1, (size_t)blob_bytes, in) != (size_t)blob_bytes) return 2;
        tt_render_item* items = (tt_render_item*)(blob + table_at);
        for (int i = 0; i < n; ++i) {
            items[i].src = items[i].src ? blob + ((uintptr_t)items[i].src - 1) : nullptr;
            items[i].aux = items[i].aux ? blob + ((uintptr_t)items[i].aux - 1) : nullptr;
        }
        ASAN_POISON_MEMORY_REGION(blob, (size_t)blob_bytes);
        for (int i = 0; i < n_live; ++i) ASAN_UNPOISON_MEMORY_REGION(blob + live[2 * i], (size_t)live[2 * i + 1]);
        const size_t canvas_bytes = (size_t)Hc * Wc * 3;
        std::vector<uint8_t> canvas(canvas_bytes + 2 * kGuard, 0xA5);
        uint8_t* ws = (uint8_t*)aligned_alloc(256, (size_t)up256(ws_bytes + kGuard));
        memset(ws, 0, (size_t)ws_bytes);
        memset(ws + ws_bytes, 0xA5, kGuard);
        const int rc = host_render(canvas.data() + kGuard, Hc, Wc, items, n, ws, ws_bytes);
        ASAN_UNPOISON_MEMORY_REGION(blob, (size_t)blob_bytes);
        bool ok = expect_error ? rc != 0 : rc == 0;
        for (int i = 0; i < kGuard; ++i) ok = ok && canvas[i] == 0xA5 && canvas[kGuard + canvas_bytes + i] == 0xA5 && ws[ws_bytes + i] == 0xA5;
        const int64_t dropped = ((long long*)ws)[TT_RENDER_STATUS_DROPPED];
        for (long long i = 8LL * TT_RENDER_STATUS_WORDS; i < ws_bytes; ++i) ok = ok && ws[i] == 0;    // the planes are zero again
        const int32_t rc32 = rc;
        fwrite(&rc32, 4, 1, out);
        fwrite(&dropped, 8, 1, out);
        if (rc == 0) fwrite(canvas.data() + kGuard, 1, canvas_bytes, out);
        printf("%s %s: rc %d dropped %lld\n", ok ? "ok  " : "FAIL", name.c_str(), rc, (long long)dropped);
        failed += ok ? 0 : 1;
        free(ws);
        free(blob);
    }
    fclose(out);
    fclose(in);
    printf("%d cases, %d failed\n", count, failed);
    return failed ? 1 : 0;
}
