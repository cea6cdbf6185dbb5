// The per-pixel rules of tt_render_u8 (include/thinktwice_hip.h states the contract), as __host__ __device__ functions: the compose
// kernel of render.hip and the host checker tools/render_host_check.cpp compile THIS source, as png_deflate.h serves the encoder.
// Everything is integer arithmetic, or f32 with every operation rounded on its own: the device build spells the roundings out
// (__fmul_rn / __fadd_rn / __fsub_rn), a host build must be compiled with -ffp-contract=off.  tests/render_ref.py restates the
// rules in numpy float32, item by item over the whole canvas, to the same bytes.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/thinktwice_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TT_RHD __host__ __device__ __forceinline__
#else
#define TT_RHD inline
#endif

namespace tt_render {

constexpr int kTileRows = 8;              // rows of one workgroup's tile; one lane owns a column of them
constexpr int kTileCols = 256;            // = lanes of the workgroup
constexpr int kMaxSide = 16384;           // of the canvas and of any rectangle or source
constexpr int kFixLimit = 1 << 20;        // |fixed-point coordinate| of a polyline point, 1/16 px
constexpr int kMaxReach = 1 << 15;        // radius and half_width, 1/16 px

typedef unsigned __int128 u128;

#if defined(__HIP_DEVICE_COMPILE__)
TT_RHD float fmul(float a, float b) { return __fmul_rn(a, b); }
TT_RHD float fadd(float a, float b) { return __fadd_rn(a, b); }
TT_RHD float fsub(float a, float b) { return __fsub_rn(a, b); }
#else
TT_RHD float fmul(float a, float b) { return a * b; }
TT_RHD float fadd(float a, float b) { return a + b; }
TT_RHD float fsub(float a, float b) { return a - b; }
#endif

TT_RHD uint32_t bits_of(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}
TT_RHD bool finite32(float x) { return (bits_of(x) & 0x7f800000u) != 0x7f800000u; }
TT_RHD bool is_nan(float x) { return x != x; }

TT_RHD uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) { return r | g << 8 | b << 16; }
TT_RHD uint32_t rgb_at(const uint8_t* p) { return rgb(p[0], p[1], p[2]); }

// (dst * (256 - a) + src * a + 128) >> 8 per channel, a in 0..256
TT_RHD uint32_t blend(uint32_t dst, uint32_t src, int a) {
    uint32_t out = 0;
    for (int c = 0; c < 24; c += 8) {
        const uint32_t d = (dst >> c) & 255u, s = (src >> c) & 255u;
        out |= ((d * (uint32_t)(256 - a) + s * (uint32_t)a + 128u) >> 8) << c;
    }
    return out;
}

// ------------------------------------------------------------------------------------------------------ polylines and markers
// The points of a POLYLINE_DEV / MARKER item in fixed point (1/16 px of the canvas), which of them survived, and the pixel box
// [bx0, bx1) x [by0, by1) outside which the item covers nothing (already cut to the item's rectangle).
struct PolyFix {
    int n, mode, valid;                   // mode 0: segments (i, i + 1); 1: a closed loop; 2: pairs (0, 1), (2, 3), ...
    int bx0, by0, bx1, by1;
    int pad;
    int x[TT_RENDER_MAX_POINTS], y[TT_RENDER_MAX_POINTS];
};

TT_RHD bool is_poly(int kind) { return kind == TT_RENDER_POLYLINE_DEV || kind == TT_RENDER_MARKER; }

// -> the number of dropped points.  `f` may be null (the counting pass).
TT_RHD int poly_fix(const tt_render_item& it, PolyFix* f) {
    const float* pts = (const float*)it.src;
    int n = 4, mode = 0;
    if (it.kind == TT_RENDER_POLYLINE_DEV) n = it.count;
    else mode = it.count == TT_RENDER_MARKER_BOX ? 1 : 2;
    int dropped = 0, valid = 0;
    int lox = 0, loy = 0, hix = 0, hiy = 0;
    for (int i = 0; i < n; ++i) {
        float x, y;
        if (it.kind == TT_RENDER_POLYLINE_DEV) {
            x = pts[2 * i];
            y = pts[2 * i + 1];
        } else if (mode == 1) {                      // corners: (-, -), (+, -), (+, +), (-, +)
            x = (i == 1 || i == 2) ? fadd(it.p[0], it.p[2]) : fsub(it.p[0], it.p[2]);
            y = (i >= 2) ? fadd(it.p[1], it.p[3]) : fsub(it.p[1], it.p[3]);
        } else {                                     // cross: (cx - hx, cy), (cx + hx, cy), (cx, cy - hy), (cx, cy + hy)
            x = i == 0 ? fsub(it.p[0], it.p[2]) : i == 1 ? fadd(it.p[0], it.p[2]) : it.p[0];
            y = i == 2 ? fsub(it.p[1], it.p[3]) : i == 3 ? fadd(it.p[1], it.p[3]) : it.p[1];
        }
        const float u = fadd(fadd(fmul(it.m[0], x), fmul(it.m[1], y)), it.m[2]);
        const float v = fadd(fadd(fmul(it.m[3], x), fmul(it.m[4], y)), it.m[5]);
        // (a NaN fails both comparisons: nothing that is not a small finite number reaches the conversion)
        const bool ok = finite32(x) && finite32(y) && fabsf(u) <= (float)kFixLimit && fabsf(v) <= (float)kFixLimit;
        if (!ok) {
            ++dropped;
            continue;
        }
        const int ix = (int)rintf(u), iy = (int)rintf(v);
        if (f) {
            f->x[i] = ix;
            f->y[i] = iy;
        }
        if (!valid || ix < lox) lox = ix;
        if (!valid || ix > hix) hix = ix;
        if (!valid || iy < loy) loy = iy;
        if (!valid || iy > hiy) hiy = iy;
        valid |= 1 << i;
    }
    if (f) {
        f->n = n;
        f->mode = mode;
        f->valid = valid;
        f->bx0 = f->by0 = f->bx1 = f->by1 = 0;
        if (valid) {
            const int reach = it.radius > it.half_width ? it.radius : it.half_width;
            // 16 px + 8 within [lo - reach, hi + reach]; >> 4 is the floor
            const int bx0 = (lox - reach - 8) >> 4, bx1 = ((hix + reach - 8) >> 4) + 1;
            const int by0 = (loy - reach - 8) >> 4, by1 = ((hiy + reach - 8) >> 4) + 1;
            f->bx0 = bx0 > it.x0 ? bx0 : it.x0;
            f->by0 = by0 > it.y0 ? by0 : it.y0;
            f->bx1 = bx1 < it.x0 + it.w ? bx1 : it.x0 + it.w;
            f->by1 = by1 < it.y0 + it.h ? by1 : it.y0 + it.h;
        }
    }
    return dropped;
}

// squared distance of P to the segment AB <= hw2, exactly: |coordinates| <= 2^21 + 2^18, so the dot products stay under 2^46
// and only the last comparison needs 128 bits
TT_RHD bool seg_covers(long long ax, long long ay, long long bx, long long by, long long px, long long py, long long hw2) {
    const long long dx = bx - ax, dy = by - ay, qx = px - ax, qy = py - ay;
    const long long len2 = dx * dx + dy * dy, t = qx * dx + qy * dy;
    if (t <= 0) return qx * qx + qy * qy <= hw2;
    if (t >= len2) {
        const long long rx = px - bx, ry = py - by;
        return rx * rx + ry * ry <= hw2;
    }
    long long cross = qx * dy - qy * dx;
    if (cross < 0) cross = -cross;
    return (u128)(unsigned long long)cross * (unsigned long long)cross <= (u128)(unsigned long long)hw2 * (unsigned long long)len2;
}

TT_RHD bool poly_covers(const PolyFix& f, int half_width, int radius, int px, int py) {
    if (px < f.bx0 || px >= f.bx1 || py < f.by0 || py >= f.by1) return false;
    const long long cx = 16LL * px + 8, cy = 16LL * py + 8;
    const long long r2 = (long long)radius * radius, hw2 = (long long)half_width * half_width;
    if (radius > 0)
        for (int i = 0; i < f.n; ++i)
            if (f.valid >> i & 1) {
                const long long dx = cx - f.x[i], dy = cy - f.y[i];
                if (dx * dx + dy * dy <= r2) return true;
            }
    const int nseg = f.mode == 0 ? f.n - 1 : f.mode == 1 ? f.n : f.n / 2;
    for (int k = 0; k < nseg; ++k) {
        const int a = f.mode == 2 ? 2 * k : k, b = f.mode == 2 ? 2 * k + 1 : (k + 1 == f.n ? 0 : k + 1);
        if ((f.valid >> a & 1) && (f.valid >> b & 1) && seg_covers(f.x[a], f.y[a], f.x[b], f.y[b], cx, cy, hw2)) return true;
    }
    return false;
}

// ------------------------------------------------------------------------------------------------------------- logits, clouds
// argmax over row[0..C), ties to the lowest index; -1 if one of the C values is a NaN.  vec (device only): the row is read as
// 16-byte pieces (16-byte aligned, pitch a multiple of 4 floats); a piece's channels >= C come with it and take no part.
TT_RHD int argmax_cl(const float* row, int C, bool vec) {
    float bv = 0.f;
    int bc = -1;
    bool nan = false;
#if defined(__HIP_DEVICE_COMPILE__)
    if (vec) {
        for (int c0 = 0; c0 < C; c0 += 4) {
            const float4 q = *reinterpret_cast<const float4*>(row + c0);
            const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + k < C) {
                    nan |= is_nan(e[k]);
                    if (bc < 0 || e[k] > bv) {
                        bv = e[k];
                        bc = c0 + k;
                    }
                }
        }
        return nan ? -1 : bc;
    }
#endif
    (void)vec;
    for (int c = 0; c < C; ++c) {
        const float v = row[c];
        nan |= is_nan(v);
        if (bc < 0 || v > bv) {
            bv = v;
            bc = c;
        }
    }
    return nan ? -1 : bc;
}

TT_RHD bool rows_vec(const tt_render_item& it) { return (it.stride & 3) == 0 && ((uintptr_t)it.src & 15) == 0; }

// Where point `i` of a POINTS_BEV item lands: false if it is not drawn, else the word of the item's plane and the value the
// atomic maximum takes (height index + 1: an untouched word stays 0).
TT_RHD bool splat_target(const tt_render_item& it, int Hc, int Wc, int i, int& word, uint32_t& val) {
    const float* row = (const float*)it.src + (long long)i * it.stride;
    const float x = row[0], y = row[1], z = row[2];
    if (x == 0.f && y == 0.f && z == 0.f) return false;                  // collate padding
    if (!finite32(x) || !finite32(y) || !finite32(z)) return false;
    const float u = floorf(fadd(fadd(fmul(it.m[0], x), fmul(it.m[1], y)), it.m[2]));
    const float v = floorf(fadd(fadd(fmul(it.m[3], x), fmul(it.m[4], y)), it.m[5]));
    if (!(fabsf(u) <= (float)kFixLimit && fabsf(v) <= (float)kFixLimit)) return false;
    const int px = (int)u >> 4, py = (int)v >> 4;
    if (px < it.x0 || px >= it.x0 + it.w || py < it.y0 || py >= it.y0 + it.h) return false;
    if (px < 0 || px >= Wc || py < 0 || py >= Hc) return false;
    float t = floorf(fmul(fsub(z, it.p[0]), it.p[1]));
    t = t > 0.f ? t : 0.f;                                               // (also takes a NaN of inf * 0 to index 0)
    t = t < 255.f ? t : 255.f;
    word = (py - it.y0) * it.w + (px - it.x0);
    val = (uint32_t)(int)t + 1u;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- the compose
// What a thread remembers while it walks down its column through ONE item: the cell row it last took an argmax for.
struct CellCache {
    int row, value;
};

// The colour of canvas pixel (px, py) after item `it`, given the colour `dst` below it.  (px, py) lies inside the canvas and the
// item's rectangle; `poly` is the item's PolyFix (polylines and markers only); `ws` the workspace.
TT_RHD uint32_t shade(const tt_render_item& it, const PolyFix* poly, uint8_t* ws, int px, int py, uint32_t dst, CellCache& cc) {
    const int lx = px - it.x0, ly = py - it.y0;
    const uint8_t* src8 = (const uint8_t*)it.src;
    const float* src32 = (const float*)it.src;
    const uint8_t* aux = (const uint8_t*)it.aux;
    switch (it.kind) {
        case TT_RENDER_FILL: return blend(dst, it.color, it.alpha);
        case TT_RENDER_IMAGE_F32: {
            const long long plane = (long long)it.sh * it.sw, at = (long long)(ly / it.scale) * it.sw + lx / it.scale;
            uint32_t out = 0;
            bool nan = false;
            for (int c = 0; c < 3; ++c) {
                const float v = src32[c * plane + at];
                nan |= is_nan(v);
                float q = rintf(fadd(fmul(v, it.m[c]), it.m[3 + c]));
                q = q > 0.f ? q : 0.f;
                q = q < 255.f ? q : 255.f;
                out |= (uint32_t)(int)q << (8 * c);
            }
            return blend(dst, nan ? it.color : out, it.alpha);
        }
        case TT_RENDER_IMAGE_U8: {
            const int s = it.scale, ch = it.channels;
            uint32_t sum[3] = {0, 0, 0};
            for (int dy = 0; dy < s; ++dy)
                for (int dx = 0; dx < s; ++dx) {
                    const uint8_t* q = src8 + ((long long)(ly * s + dy) * it.sw + (lx * s + dx)) * ch;
                    for (int c = 0; c < ch; ++c) sum[c] += q[c];
                }
            const uint32_t area = (uint32_t)(s * s);
            for (int c = 0; c < ch; ++c) sum[c] = (sum[c] + area / 2) / area;
            return blend(dst, ch == 1 ? rgb(sum[0], sum[0], sum[0]) : rgb(sum[0], sum[1], sum[2]), it.alpha);
        }
        case TT_RENDER_SEG_OVERLAY:
        case TT_RENDER_DEPTH_MAP: {
            const int cy = ly / it.scale, cx = lx / it.scale;
            if (cc.row != cy) {
                cc.row = cy;
                cc.value = argmax_cl(src32 + ((long long)cy * it.sw + cx) * it.stride, it.channels, rows_vec(it));
            }
            if (cc.value < 0) return it.color;
            if (it.kind == TT_RENDER_SEG_OVERLAY) {
                const uint8_t* e = aux + 4 * cc.value;
                return blend(dst, rgb_at(e), e[3] + (e[3] >> 7));
            }
            const int index = it.channels > 1 ? cc.value * 255 / (it.channels - 1) : 0;
            return blend(dst, rgb_at(aux + 3 * index), it.alpha);
        }
        case TT_RENDER_POINTS_BEV: {
            uint32_t* word = (uint32_t*)(ws + it.ws_offset) + ((long long)ly * it.w + lx);
            const uint32_t v = *word;
            if (!v) return dst;
            *word = 0u;                                                  // this pixel is the word's only reader
            return blend(dst, rgb_at(aux + 3 * (v - 1u)), it.alpha);
        }
        case TT_RENDER_POLYLINE_DEV:
        case TT_RENDER_MARKER: return poly_covers(*poly, it.half_width, it.radius, px, py) ? blend(dst, it.color, it.alpha) : dst;
        case TT_RENDER_TEXT: {
            const int gx = lx / it.scale, gy = ly / it.scale, cell = gx / 6, col = gx % 6;
            if (col >= 5 || gy >= 7) return dst;
            int glyph = aux[src8[cell]];
            glyph = glyph < it.channels ? glyph : it.channels - 1;
            return (aux[256 + 8 * glyph + gy] >> (4 - col) & 1) ? blend(dst, it.color, it.alpha) : dst;
        }
        default: return dst;
    }
}

// The part of the canvas an item can touch, [x0, x1) x [y0, y1): its rectangle (its PolyFix box for polylines) cut to the canvas.
struct Box {
    int x0, y0, x1, y1;
};
TT_RHD Box item_box(const tt_render_item& it, const PolyFix* poly, int Hc, int Wc) {
    Box b;
    if (is_poly(it.kind)) b = Box{poly->bx0, poly->by0, poly->bx1, poly->by1};
    else b = Box{it.x0, it.y0, it.x0 + it.w, it.y0 + it.h};
    b.x0 = b.x0 > 0 ? b.x0 : 0;
    b.y0 = b.y0 > 0 ? b.y0 : 0;
    b.x1 = b.x1 < Wc ? b.x1 : Wc;
    b.y1 = b.y1 < Hc ? b.y1 : Hc;
    return b;
}

// ------------------------------------------------------------------------------------------------------- host-side validation
inline long long up256(long long n) { return (n + 255) / 256 * 256; }

// null if the item is acceptable, else what is wrong with it (a format for one int: the item's index)
inline const char* item_fault(const tt_render_item& it, long long& next_plane, long long workspace_bytes, bool check_pointers) {
    if (it.kind < 0 || it.kind >= TT_RENDER_NUM_KINDS) return "item %d: unknown kind";
    if (it.w < 0 || it.h < 0 || it.w > kMaxSide || it.h > kMaxSide) return "item %d: a rectangle side outside 0..16384";
    if (it.x0 < -(1 << 24) || it.x0 > (1 << 24) || it.y0 < -(1 << 24) || it.y0 > (1 << 24)) return "item %d: a corner beyond +-2^24";
    if (it.alpha < 0 || it.alpha > 256) return "item %d: alpha outside 0..256";
    for (int i = 0; i < 6; ++i)
        if (!finite32(it.m[i])) return "item %d: a non-finite m";
    for (int i = 0; i < 4; ++i)
        if (!finite32(it.p[i])) return "item %d: a non-finite p";
    const bool sourced = it.kind != TT_RENDER_FILL && it.kind != TT_RENDER_MARKER;
    const bool tabled = it.kind == TT_RENDER_SEG_OVERLAY || it.kind == TT_RENDER_DEPTH_MAP || it.kind == TT_RENDER_POINTS_BEV ||
                        it.kind == TT_RENDER_TEXT;
    const bool counted = it.kind == TT_RENDER_POINTS_BEV || it.kind == TT_RENDER_POLYLINE_DEV || it.kind == TT_RENDER_TEXT;
    if (counted && it.count < 0) return "item %d: a negative count";
    if (check_pointers && sourced && !it.src && !(counted && it.count == 0)) return "item %d: null src";
    if (check_pointers && tabled && !it.aux) return "item %d: null aux";
    switch (it.kind) {
        case TT_RENDER_IMAGE_F32:
        case TT_RENDER_IMAGE_U8:
        case TT_RENDER_SEG_OVERLAY:
        case TT_RENDER_DEPTH_MAP: {
            if (it.scale < 1 || it.scale > kMaxSide) return "item %d: scale outside 1..16384";
            if (it.sw < 0 || it.sh < 0 || it.sw > kMaxSide || it.sh > kMaxSide) return "item %d: a source side outside 0..16384";
            const bool reduce = it.kind == TT_RENDER_IMAGE_U8;
            const long long gw = reduce ? it.sw / it.scale : (long long)it.sw * it.scale;
            const long long gh = reduce ? it.sh / it.scale : (long long)it.sh * it.scale;
            if (it.w > gw || it.h > gh) return "item %d: the rectangle is larger than its source gives";
            if (reduce && it.scale > 256) return "item %d: a box factor above 256";
            if (reduce && it.channels != 1 && it.channels != 3) return "item %d: channels not 1 or 3";
            if (it.kind == TT_RENDER_SEG_OVERLAY && (it.channels < 1 || it.channels > 32)) return "item %d: classes outside 1..32";
            if (it.kind == TT_RENDER_DEPTH_MAP && (it.channels < 1 || it.channels > 256)) return "item %d: bins outside 1..256";
            if ((it.kind == TT_RENDER_SEG_OVERLAY || it.kind == TT_RENDER_DEPTH_MAP) && (it.stride < it.channels || it.stride > 4096))
                return "item %d: stride below the channels or above 4096";
            if (check_pointers && (it.kind != TT_RENDER_IMAGE_U8) && ((uintptr_t)it.src & 3)) return "item %d: misaligned f32 source";
            break;
        }
        case TT_RENDER_POINTS_BEV: {
            if (it.stride < 3 || it.stride > 4096) return "item %d: a point stride outside 3..4096";
            if (check_pointers && ((uintptr_t)it.src & 3)) return "item %d: misaligned f32 source";
            const long long bytes = up256(4LL * it.w * it.h);
            if (it.ws_offset != next_plane) return "item %d: ws_offset is not where its plane belongs";
            if (workspace_bytes >= 0 && it.ws_offset + bytes > workspace_bytes) return "item %d: its plane passes the end of the workspace";
            next_plane += bytes;
            break;
        }
        case TT_RENDER_POLYLINE_DEV:
        case TT_RENDER_MARKER:
            if (it.kind == TT_RENDER_POLYLINE_DEV && it.count > TT_RENDER_MAX_POINTS) return "item %d: more than TT_RENDER_MAX_POINTS points";
            if (it.kind == TT_RENDER_MARKER && it.count != TT_RENDER_MARKER_CROSS && it.count != TT_RENDER_MARKER_BOX)
                return "item %d: unknown marker shape";
            if (it.radius < 0 || it.radius > kMaxReach || it.half_width < 0 || it.half_width > kMaxReach)
                return "item %d: radius or half_width outside 0..2^15";
            if (check_pointers && it.kind == TT_RENDER_POLYLINE_DEV && ((uintptr_t)it.src & 3)) return "item %d: misaligned f32 source";
            break;
        case TT_RENDER_TEXT:
            if (it.scale < 1 || it.scale > 256) return "item %d: text scale outside 1..256";
            if (it.channels < 1 || it.channels > 256) return "item %d: glyph count outside 1..256";
            if (it.count > kMaxSide) return "item %d: more than 16384 characters";
            if (it.w > 6LL * it.count * it.scale || it.h > 8 * it.scale) return "item %d: the rectangle is larger than its text";
            break;
        default: break;
    }
    return nullptr;
}

}  // namespace tt_render
