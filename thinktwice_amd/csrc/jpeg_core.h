// The JPEG encoder's core, written once: baseline sequential DCT (ITU-T T.81, SOF0, 8 bit) in a JFIF wrapper, with restart
// intervals so that the entropy stage is independent per interval.  Plain functions over byte spans, no HIP type in any
// signature.  csrc/jpeg_encode.hip compiles them as device code (one lane per 8 x 8 block in the transform, one 64-lane
// workgroup per restart interval in the entropy pass); tools/jpeg_encode_host_check.cpp compiles the same text as host C++.
//
// Execution model: lanes.h's.  The entropy pass is written for 64 lanes (`Lanes`, TT_ENC_LANES, PerLane, TT_PNG_SYNC);
// the host plays all 64, so its bytes are the device's.  The transform of a block is a function of the pixels and the block's
// index alone and touches no shared state.
//
// Determinism.  The bytes are a function of the pixels and the parameters.  The one shared update is an integer OR into the
// interval's bit buffer (disjoint bits, commutative); both prefix sums are exact integer functions of the 64 lanes' values.
//
// Arithmetic (integer only; this project's own, so the files are not byte-equal to another encoder's):
//   colour     Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//              Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16        16 fractional bits, one rounding;
//              Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16        every result lies in 0..255
//   padding    a sample outside the picture is the sample of the nearest pixel inside (last column, last row repeated)
//   4:2:0      a chroma sample is (a + b + c + d + 2) >> 2 over the 2 x 2 pixels' 8-bit Cb (Cr) values
//   level      s = sample - 128
//   DCT        separable, T[u][x] = +-K[k], K[k] = round(2^14 * cos(k pi / 16) / 2), k = 1..7 (K[4] serves u = 0): 14
//              fractional bits.  Rows first: P[y][u] = sum_x T[u][x] s[y][x], exact; R[y][u] = (P + 1024) >> 11 (3
//              fractional bits, so that the second pass stays inside 32 bits: |R| <= 4018, |F| <= 8 * 8035 * 4018 < 2^28.3);
//              F[v][u] = sum_y T[v][y] R[y][u], exact, 17 fractional bits.
//   quantise   to nearest, ties away from zero: q = sign(F) * ((|F| + (Q << 16)) / (Q << 17)); an AC value is then clamped to
//              +-1023 (its largest category in the standard tables is 10; exact arithmetic cannot pass it, rounding might).
// The DC value lies in -1024..1016, so a DC difference has category 0..11.
//
// Entropy coding.  Per block: the DC difference to the previous block of the same component in the interval (0 for the first:
// a parallel step, the neighbour's DC is read from the coefficients), then run/size pairs with ZRL (F0) and EOB (00).  A step
// takes 64 consecutive blocks, one per lane: every lane sizes its block, an exclusive prefix sum places it, every lane ORs its
// codes into the LDS bit buffer (most significant bit first), the whole bytes are flushed: the lanes take consecutive runs of
// bytes, count their FF bytes, a second prefix sum places the runs, and every FF is followed by 00.  At the end the last byte
// is padded with 1 bits and the interval's marker follows: RSTm, m = interval mod 8, or EOI after the last.
//
// Sizes.  A block is at most 64 * (16 + 11) bits = 216 bytes, 432 when every byte is stuffed; an interval adds its marker.
#pragma once
#include <stdint.h>

#include "../../include/thinktwice_hip.h"
#include "lanes.h"              // the lane convention: Lanes, PerLane, TT_ENC_LANES, exclusive_scan, TT_ENC_OR, TT_PNG_SYNC

namespace tt_jpeg {

using tt_pngenc::kLanes;
using tt_pngenc::Lanes;
using tt_pngenc::PerLane;

constexpr int kBlockBytes = 216;                          // 64 coefficients of at most 27 bits
constexpr int kBufWords = kLanes * kBlockBytes / 4 + 4;   // a step's bits and the byte carried over
constexpr int kMaxDim = 65535;
constexpr int kEoi = 0xD9, kRst0 = 0xD0;

// natural (row-major) index of zig-zag position i
TT_HD inline int zigzag(int i) {
    static constexpr uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[i];
}

// T.81 Annex K.1 / K.2, natural order
TT_HD inline int base_quant(int table, int i) {
    static constexpr uint8_t t[2][64] = {
        {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    return t[table][i];
}

TT_HD inline int quant_entry(int table, int i, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (base_quant(table, i) * s + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}

// T.81 Annex K.3: table 0 DC luminance, 1 DC chrominance, 2 AC luminance, 3 AC chrominance
TT_HD inline int huff_bits(int table, int i) {
    static constexpr uint8_t t[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                         {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                         {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                         {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
    return t[table][i];
}
TT_HD inline int huff_count(int table) { return table < 2 ? 12 : 162; }
TT_HD inline int huff_val(int table, int i) {
    static constexpr uint8_t ac[2][162] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
         0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
         0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
         0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
         0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
         0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
         0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
         0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
         0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
         0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
         0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
         0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
         0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
         0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
         0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
    return table < 2 ? i : ac[table - 2][i];
}

// ---------------------------------------------------------------------------------------------------------------- geometry
struct Geom {
    int nc;                 // components: 1 or 3
    int mw, mh;             // an MCU in pixels: 8 x 8, or 16 x 16 at 4:2:0
    int bpm;                // blocks per MCU: 1 (grey), 3 (4:4:4: Y Cb Cr), 6 (4:2:0: Y00 Y01 Y10 Y11 Cb Cr)
    int mx, my;             // MCUs per row, MCU rows
    int nint;               // restart intervals
    long long dri;          // MCUs per interval: restart_rows * mx (the entry refuses one above 65535)
    long long blocks;       // of the image
    int header;             // bytes before the scan
};

// H, W in 1..65535, C 1 or 3, sub a tt_jpeg_subsampling, restart_rows >= 1
TT_HD inline Geom geom(int H, int W, int C, int sub, int restart_rows) {
    Geom g;
    g.nc = C;
    const bool s420 = C == 3 && sub == TT_JPEG_420;
    g.mw = g.mh = s420 ? 16 : 8;
    g.bpm = C == 1 ? 1 : s420 ? 6 : 3;
    g.mx = (W + g.mw - 1) / g.mw;
    g.my = (H + g.mh - 1) / g.mh;
    g.dri = (long long)restart_rows * g.mx;
    g.nint = (int)((g.my + (long long)restart_rows - 1) / restart_rows);
    g.blocks = (long long)g.mx * g.my * g.bpm;
    // SOI 2, APP0 18, DQT 4 + 65 per table, SOF0 10 + 3 per component, DHT 4 + (29 + 179) per pair, DRI 6, SOS 8 + 2 per component
    g.header = C == 1 ? 2 + 18 + 69 + 13 + 212 + 6 + 10 : 2 + 18 + 134 + 19 + 420 + 6 + 14;
    return g;
}

// MCU rows of interval k
TT_HD inline int interval_rows(const Geom& g, int restart_rows, int k) {
    const long long left = g.my - (long long)k * restart_rows;
    return (int)(left < restart_rows ? left : restart_rows);
}
TT_HD inline long long interval_blocks(const Geom& g, int restart_rows, int k) { return (long long)interval_rows(g, restart_rows, k) * g.mx * g.bpm; }
TT_HD inline long long interval_first_block(const Geom& g, int restart_rows, int k) { return (long long)k * restart_rows * g.mx * g.bpm; }
// the most an interval of n blocks can become, its marker included; the slot the entropy pass writes it to
TT_HD inline long long interval_bound(long long n) { return 2 * kBlockBytes * n + 2; }
TT_HD inline long long interval_slot_bytes(long long n) { return (interval_bound(n) + 15) / 16 * 16; }
TT_HD inline long long file_bound(const Geom& g) { return g.header + 2 * kBlockBytes * g.blocks + 2LL * g.nint; }

// ---------------------------------------------------------------------------------------------------------------- transform
// 8 values -> their DCT times 2^14 (see the head of the file): exact integer sums
TT_HD inline void dct8(const int* x, int* X) {
    constexpr int K1 = 8035, K2 = 7568, K3 = 6811, K4 = 5793, K5 = 4551, K6 = 3135, K7 = 1598;
    const int s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const int d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    X[0] = K4 * (s0 + s1 + s2 + s3);
    X[4] = K4 * (s0 - s1 - s2 + s3);
    X[2] = K2 * (s0 - s3) + K6 * (s1 - s2);
    X[6] = K6 * (s0 - s3) - K2 * (s1 - s2);
    X[1] = K1 * d0 + K3 * d1 + K5 * d2 + K7 * d3;
    X[3] = K3 * d0 - K7 * d1 - K1 * d2 - K5 * d3;
    X[5] = K5 * d0 - K1 * d1 + K7 * d2 + K3 * d3;
    X[7] = K7 * d0 - K5 * d1 + K3 * d2 - K1 * d3;
}

// component `comp` (0 Y, 1 Cb, 2 Cr) of an RGB pixel
TT_HD inline int ycc(const uint8_t* p, int comp) {
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// Block b of the image in scan order (MCU by MCU, within one the order of Geom::bpm) -> 64 quantised coefficients in zig-zag
// order.  q: the quantisation tables in natural order, [2][64].
TT_HD inline void transform_block(const uint8_t* px, int H, int W, const Geom& g, long long b, const uint16_t* q, int16_t* out) {
    const long long m = b / g.bpm;
    const int r = (int)(b % g.bpm), my = (int)(m / g.mx), mx = (int)(m % g.mx);
    const int comp = g.bpm == 1 ? 0 : g.bpm == 3 ? r : r < 4 ? 0 : r - 3;
    const bool half = g.bpm == 6 && comp > 0;                   // a 4:2:0 chroma block: 16 x 16 pixels
    const int x0 = mx * g.mw + ((g.bpm == 6 && comp == 0) ? (r & 1) * 8 : 0);
    const int y0 = my * g.mh + ((g.bpm == 6 && comp == 0) ? (r >> 1) * 8 : 0);
    const uint16_t* qt = q + (comp ? 64 : 0);
    int R[64];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int s[8], P[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int v;
            if (half) {
                v = 2;
                for (int dy = 0; dy < 2; ++dy)
                    for (int dx = 0; dx < 2; ++dx) {
                        int y = y0 + 2 * j + dy, x = x0 + 2 * i + dx;
                        y = y < H ? y : H - 1;
                        x = x < W ? x : W - 1;
                        v += ycc(px + ((long long)y * W + x) * 3, comp);
                    }
                v >>= 2;
            } else {
                int y = y0 + j, x = x0 + i;
                y = y < H ? y : H - 1;
                x = x < W ? x : W - 1;
                v = g.nc == 1 ? px[(long long)y * W + x] : ycc(px + ((long long)y * W + x) * 3, comp);
            }
            s[i] = v - 128;
        }
        dct8(s, P);
#pragma unroll
        for (int u = 0; u < 8; ++u) R[j * 8 + u] = (P[u] + 1024) >> 11;
    }
    int F[64];                                                  // natural order: F[v * 8 + u]
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int c[8], X[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = R[j * 8 + u];
        dct8(c, X);
#pragma unroll
        for (int v = 0; v < 8; ++v) F[v * 8 + u] = X[v];
    }
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int n = zigzag(i), f = F[n];
        const uint32_t a = (uint32_t)(f < 0 ? -f : f), Q = qt[n];
        int v = (int)((a + (Q << 16)) / (Q << 17));
        if (i > 0 && v > 1023) v = 1023;
        out[i] = (int16_t)(f < 0 ? -v : v);
    }
}

// the tables of one quality, natural order, q[2][64]: every lane its entries
TT_HD inline void fill_quant(uint16_t* q, int quality, Lanes L) {
    TT_ENC_LANES(l) {
        q[l] = (uint16_t)quant_entry(0, l, quality);
        q[64 + l] = (uint16_t)quant_entry(1, l, quality);
    }
}

// ---------------------------------------------------------------------------------------------------------------- entropy
struct State {
    uint32_t buf[kBufWords];            // the interval's bits not yet in memory, most significant bit of word 0 first
    uint32_t dc[2][12];                 // (code << 5) | length, by category
    uint32_t ac[2][256];                // the same, by run/size symbol
};

// symbol k (in the order of the table's values) of table t: its canonical code and length, packed
TT_HD inline uint32_t canonical(int t, int k) {
    int code = 0, cum = 0;
    for (int len = 1; len <= 16; ++len) {
        const int n = huff_bits(t, len - 1);
        if (k < cum + n) return ((uint32_t)(code + (k - cum)) << 5) | (uint32_t)len;
        cum += n;
        code = (code + n) << 1;
    }
    return 0;
}

TT_HD inline void build_tables(State& S, Lanes L) {
    TT_ENC_LANES(l) {
        for (int i = l; i < 512; i += kLanes) S.ac[i >> 8][i & 255] = 0;
    }
    TT_PNG_SYNC();
    TT_ENC_LANES(l) {
        if (l < 12) {
            S.dc[0][l] = canonical(0, l);
            S.dc[1][l] = canonical(1, l);
        }
        for (int k = l; k < 162; k += kLanes) {
            S.ac[0][huff_val(2, k)] = canonical(2, k);
            S.ac[1][huff_val(3, k)] = canonical(3, k);
        }
    }
    TT_PNG_SYNC();
}

TT_HD inline int bit_size(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }      // a >= 0

// n <= 27 bits of v at bit `at` of the buffer
TT_HD inline void or_bits(State& S, int at, uint32_t v, int n) {
    const int w = at >> 5, sh = at & 31;
    const uint64_t x = (uint64_t)v << (64 - n - sh);
    const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
    if (hi) TT_ENC_OR(&S.buf[w], hi);
    if (lo) TT_ENC_OR(&S.buf[w + 1], lo);
}

struct CountBits {
    uint32_t n;
    TT_HD void operator()(State&, uint32_t, int len) { n += (uint32_t)len; }
};
struct WriteBits {
    int at;
    TT_HD void operator()(State& S, uint32_t v, int len) {
        or_bits(S, at, v, len);
        at += len;
    }
};

// One block's codes, in order, to `emit`: blk its 64 coefficients, pred the DC it predicts from, tab 0 luminance, 1 chrominance.
template <typename Emit>
TT_HD inline void code_block(State& S, const int16_t* blk, int pred, int tab, Emit& emit) {
    const int diff = blk[0] - pred;
    int size = bit_size(diff < 0 ? -diff : diff);
    uint32_t e = S.dc[tab][size];
    emit(S, ((e >> 5) << size) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1)), (int)(e & 31) + size);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[k];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16) {
            e = S.ac[tab][0xF0];
            emit(S, e >> 5, (int)(e & 31));
        }
        size = bit_size(v < 0 ? -v : v);
        e = S.ac[tab][(run << 4) | size];
        emit(S, ((e >> 5) << size) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1)), (int)(e & 31) + size);
        run = 0;
    }
    if (run) {
        e = S.ac[tab][0];
        emit(S, e >> 5, (int)(e & 31));
    }
}

// block b of an interval: the block of the same component before it, or -1; its table
TT_HD inline long long previous_block(int bpm, long long b) {
    if (bpm == 1) return b - 1;
    if (bpm == 3) return b - 3;
    const int r = (int)(b % 6);
    return r == 0 ? b - 3 : r < 4 ? b - 1 : b - 6;
}
TT_HD inline int block_table(int bpm, long long b) { return bpm == 1 ? 0 : bpm == 3 ? (b % 3 > 0) : (b % 6 >= 4); }

struct Writer {
    uint8_t* out;
    long long cap, base;                // `base` bytes of the interval are in memory (only those below cap are stored)
    int nbits;                          // more in S.buf
};

TT_HD inline uint32_t buf_byte(const State& S, int i) { return (S.buf[i >> 2] >> (24 - 8 * (i & 3))) & 255u; }

// The buffer's whole bytes go to memory, every FF followed by 00; the bits left over move to the buffer's start.
TT_HD inline void flush(State& S, Writer& W, Lanes L) {
    TT_PNG_SYNC();
    const int nbytes = W.nbits >> 3, rem = W.nbits & 7, chunk = (nbytes + kLanes - 1) / kLanes;
    PerLane<uint32_t> ff;
    TT_ENC_LANES(l) {
        const int lo = l * chunk, hi = lo + chunk < nbytes ? lo + chunk : nbytes;
        uint32_t n = 0;
        for (int i = lo; i < hi; ++i) n += buf_byte(S, i) == 255u;
        ff[l] = n;
    }
    const uint32_t stuffed = tt_pngenc::exclusive_scan(ff, L);
    TT_ENC_LANES(l) {
        const int lo = l * chunk, hi = lo + chunk < nbytes ? lo + chunk : nbytes;
        long long p = W.base + lo + ff[l];
        for (int i = lo; i < hi; ++i) {
            const uint32_t v = buf_byte(S, i);
            if (p < W.cap) W.out[p] = (uint8_t)v;
            ++p;
            if (v == 255u) {
                if (p < W.cap) W.out[p] = 0;
                ++p;
            }
        }
    }
    const uint32_t carry = rem ? (TT_PNG_UNIFORM(buf_byte(S, nbytes)) & (0xFF00u >> rem) & 255u) : 0u;
    const int used = ((W.nbits + 31) >> 5) + 1;
    TT_PNG_SYNC();
    TT_ENC_LANES(l)
        for (int w = l; w < used && w < kBufWords; w += kLanes) S.buf[w] = w == 0 ? carry << 24 : 0u;
    TT_PNG_SYNC();
    W.base += nbytes + stuffed;
    W.nbits = rem;
}

// One restart interval: coefs its n blocks (64 int16 each, zig-zag order, scan order), bpm the MCU's blocks -> out[0, cap),
// cap >= interval_bound(n); marker the byte after FF that ends it.  Returns the bytes written (the same in every lane).
TT_HD inline long long encode_interval(State& S, const int16_t* coefs, long long n, int bpm, uint8_t* out, long long cap, int marker, Lanes L) {
    build_tables(S, L);
    TT_ENC_LANES(l)
        for (int w = l; w < kBufWords; w += kLanes) S.buf[w] = 0;
    TT_PNG_SYNC();
    Writer W{out, cap, 0, 0};
    for (long long b0 = 0; b0 < n; b0 += kLanes) {
        PerLane<uint32_t> at;
        TT_ENC_LANES(l) {
            const long long b = b0 + l;
            CountBits c{0};
            if (b < n) {
                const long long p = previous_block(bpm, b);
                code_block(S, coefs + b * 64, p >= 0 ? coefs[p * 64] : 0, block_table(bpm, b), c);
            }
            at[l] = c.n;
        }
        const uint32_t total = tt_pngenc::exclusive_scan(at, L);
        TT_ENC_LANES(l) {
            const long long b = b0 + l;
            if (b < n) {
                const long long p = previous_block(bpm, b);
                WriteBits w{W.nbits + (int)at[l]};
                code_block(S, coefs + b * 64, p >= 0 ? coefs[p * 64] : 0, block_table(bpm, b), w);
            }
        }
        W.nbits += (int)total;
        flush(S, W, L);
    }
    if (W.nbits) {                                              // pad the last byte with 1 bits
        TT_ENC_LANES(l) if (l == 0) or_bits(S, W.nbits, (1u << (8 - W.nbits)) - 1, 8 - W.nbits);
        W.nbits = 8;
        flush(S, W, L);
    }
    TT_ENC_LANES(l) if (l == 0) {
        if (W.base < cap) out[W.base] = 0xFF;
        if (W.base + 1 < cap) out[W.base + 1] = (uint8_t)marker;
    }
    return W.base + 2;
}

// ---------------------------------------------------------------------------------------------------------------- the file
TT_HD inline uint8_t* put16(uint8_t* p, int v) {
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
    return p + 2;
}

// Everything before the scan, g.header bytes: SOI, APP0, DQT, SOF0, DHT, DRI, SOS.  One lane.
TT_HD inline int write_header(uint8_t* f, int H, int W, int quality, const Geom& g) {
    uint8_t* p = f;
    p = put16(p, 0xFFD8);
    p = put16(p, 0xFFE0);
    p = put16(p, 16);
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};     // 1.01, no units, density 1:1, no thumbnail
    for (int i = 0; i < 14; ++i) *p++ = jfif[i];
    const int tables = g.nc == 1 ? 1 : 2;
    p = put16(p, 0xFFDB);
    p = put16(p, 2 + 65 * tables);
    for (int t = 0; t < tables; ++t) {
        *p++ = (uint8_t)t;                                      // 8-bit entries, table t
        for (int i = 0; i < 64; ++i) *p++ = (uint8_t)quant_entry(t, zigzag(i), quality);
    }
    p = put16(p, 0xFFC0);
    p = put16(p, 8 + 3 * g.nc);
    *p++ = 8;
    p = put16(p, H);
    p = put16(p, W);
    *p++ = (uint8_t)g.nc;
    for (int c = 0; c < g.nc; ++c) {
        *p++ = (uint8_t)(c + 1);
        *p++ = (uint8_t)((c == 0 && g.bpm == 6) ? 0x22 : 0x11);
        *p++ = (uint8_t)(c ? 1 : 0);
    }
    p = put16(p, 0xFFC4);
    p = put16(p, 2 + 208 * tables);
    for (int t = 0; t < tables; ++t)
        for (int ac = 0; ac < 2; ++ac) {
            const int h = 2 * ac + t;
            *p++ = (uint8_t)((ac << 4) | t);
            for (int i = 0; i < 16; ++i) *p++ = (uint8_t)huff_bits(h, i);
            for (int i = 0; i < huff_count(h); ++i) *p++ = (uint8_t)huff_val(h, i);
        }
    p = put16(p, 0xFFDD);
    p = put16(p, 4);
    p = put16(p, (int)g.dri);
    p = put16(p, 0xFFDA);
    p = put16(p, 6 + 2 * g.nc);
    *p++ = (uint8_t)g.nc;
    for (int c = 0; c < g.nc; ++c) {
        *p++ = (uint8_t)(c + 1);
        *p++ = (uint8_t)(c ? 0x11 : 0x00);
    }
    *p++ = 0;
    *p++ = 63;
    *p++ = 0;
    return (int)(p - f);
}

// ------------------------------------------------------------------------------------------------- the slot table's format
// What file_slots.h asks of a format: a unit is a workgroup of the transform (64 blocks of 128 bytes), a part a restart interval.
struct SlotFormat {
    typedef tt_jpeg_enc_image Image;
    typedef tt_jpeg::Geom Geom;
    TT_HD static Geom geom(const Image& im) { return tt_jpeg::geom(im.height, im.width, im.channels, im.subsampling, im.restart_rows); }
    TT_HD static long long units(const Image&, const Geom& g) { return (g.blocks + kLanes - 1) / kLanes; }
    TT_HD static int parts(const Geom& g) { return g.nint; }
    TT_HD static long long first_bytes(const Geom& g) { return g.blocks * 128; }
    TT_HD static long long slot_bytes(const Image& im, const Geom& g, bool last) {
        return interval_slot_bytes(interval_blocks(g, im.restart_rows, last ? g.nint - 1 : 0));
    }
    // 0 where the table is refused for its sizes or parameters
    static long long bound(const Image& im) {
        if ((im.channels != 1 && im.channels != 3) || im.height < 1 || im.width < 1 || im.height > kMaxDim || im.width > kMaxDim) return 0;
        if (im.quality < 1 || im.quality > 100 || (im.subsampling != TT_JPEG_444 && im.subsampling != TT_JPEG_420) || im.restart_rows < 1) return 0;
        const Geom g = geom(im);
        if (g.dri > 65535) return 0;
        return file_bound(g);
    }
};

}  // namespace tt_jpeg
