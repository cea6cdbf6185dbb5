// tt_render_u8: a display list drawn into a uint8 canvas on the device (include/thinktwice_hip.h states the contract; the per-pixel
// rules are csrc/render_raster.h, shared with the host checker).  Three kinds of launch:
//   render_splat_kernel   one per POINTS_BEV item: every point's height index, an integer atomicMax on the item's scratch plane
//   render_count_kernel   the dropped points of the list's polylines and markers, added to the status word
//   render_compose_kernel the gather: one 256-lane workgroup per tile of 8 rows x 256 columns, a lane owns one column of it and
//                         keeps its 8 colours in registers while the workgroup walks the list through LDS, TT_RENDER_CHUNK items at
//                         a time (16-byte copies; lane j of a stage brings item j's polyline to fixed point and decides whether
//                         the item can touch the tile at all).  Only the lanes' own pixels are written, each once, at the end.
#include "render_raster.h"
#include "tt_common.h"

namespace tt {

using namespace tt_render;

static_assert(sizeof(tt_render_item) == 128, "tt_render_item is staged as eight 16-byte pieces");
constexpr int kItemPieces = sizeof(tt_render_item) / 16;

__global__ __launch_bounds__(256) void render_splat_kernel(const tt_render_item* __restrict__ items, int index, int Hc, int Wc,
                                                           uint8_t* __restrict__ ws) {
    const tt_render_item it = items[index];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= it.count) return;
    int word;
    uint32_t val;
    if (splat_target(it, Hc, Wc, (int)i, word, val)) atomicMax((uint32_t*)(ws + it.ws_offset) + word, val);
}

__global__ __launch_bounds__(256) void render_count_kernel(const tt_render_item* __restrict__ items, int num_items,
                                                           uint8_t* __restrict__ ws) {
    for (int j = threadIdx.x; j < num_items; j += blockDim.x) {
        if (!is_poly(items[j].kind)) continue;
        const tt_render_item it = items[j];
        const int dropped = poly_fix(it, nullptr);
        if (dropped) atomicAdd((unsigned long long*)ws + TT_RENDER_STATUS_DROPPED, (unsigned long long)dropped);
    }
}

__global__ __launch_bounds__(kTileCols) void render_compose_kernel(uint8_t* __restrict__ canvas, int Hc, int Wc,
                                                                   const tt_render_item* __restrict__ items, int num_items,
                                                                   uint8_t* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) tt_render_item s_item[TT_RENDER_CHUNK];
    __shared__ PolyFix s_poly[TT_RENDER_CHUNK];
    __shared__ Box s_box[TT_RENDER_CHUNK];                 // the item's reach inside this tile; empty = skipped by the workgroup
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * kTileCols, ty0 = blockIdx.y * kTileRows;
    const int tx1 = min(tx0 + kTileCols, Wc), ty1 = min(ty0 + kTileRows, Hc);
    const int px = tx0 + tid;
    uint32_t col[kTileRows];
#pragma unroll
    for (int r = 0; r < kTileRows; ++r) col[r] = 0u;

    for (int base = 0; base < num_items; base += TT_RENDER_CHUNK) {
        const int cnt = min(TT_RENDER_CHUNK, num_items - base);
        const uint4* from = reinterpret_cast<const uint4*>(items + base);
        uint4* to = reinterpret_cast<uint4*>(s_item);
        for (int i = tid; i < cnt * kItemPieces; i += kTileCols) to[i] = from[i];
        __syncthreads();
        if (tid < cnt) {
            const tt_render_item& it = s_item[tid];
            if (is_poly(it.kind)) poly_fix(it, &s_poly[tid]);
            Box b = item_box(it, &s_poly[tid], Hc, Wc);
            b.x0 = max(b.x0, tx0);
            b.y0 = max(b.y0, ty0);
            b.x1 = min(b.x1, tx1);
            b.y1 = min(b.y1, ty1);
            s_box[tid] = b;
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const Box b = s_box[j];
            if (b.x0 >= b.x1 || b.y0 >= b.y1) continue;    // (uniform: the whole workgroup skips the item)
            if (px < b.x0 || px >= b.x1) continue;
            const tt_render_item& it = s_item[j];
            CellCache cc{-1, 0};
#pragma unroll
            for (int r = 0; r < kTileRows; ++r) {
                const int py = ty0 + r;
                if (py >= b.y0 && py < b.y1) col[r] = shade(it, &s_poly[j], ws, px, py, col[r], cc);
            }
        }
        __syncthreads();                                   // the next stage overwrites what the lanes were reading
    }
    if (px < Wc) {
#pragma unroll
        for (int r = 0; r < kTileRows; ++r) {
            const int py = ty0 + r;
            if (py < Hc) {
                uint8_t* out = canvas + ((long long)py * Wc + px) * 3;
                out[0] = (uint8_t)(col[r] & 255u);
                out[1] = (uint8_t)(col[r] >> 8 & 255u);
                out[2] = (uint8_t)(col[r] >> 16 & 255u);
            }
        }
    }
}

// 0 where the table is refused; else the workspace's size
static long long render_layout(const tt_render_item* items, int num_items, long long workspace_bytes, bool check_pointers, int* bad,
                               const char** why) {
    long long next = up256(8LL * TT_RENDER_STATUS_WORDS);
    for (int i = 0; i < num_items; ++i) {
        const char* fault = item_fault(items[i], next, workspace_bytes, check_pointers);
        if (fault) {
            if (bad) *bad = i;
            if (why) *why = fault;
            return 0;
        }
    }
    return next;
}

}  // namespace tt

using namespace tt;

extern "C" long long tt_render_workspace_bytes(const tt_render_item* items_host, int num_items) {
    if (num_items < 0 || num_items > TT_RENDER_MAX_ITEMS || (num_items > 0 && !items_host)) return 0;
    return render_layout(items_host, num_items, -1, false, nullptr, nullptr);
}

extern "C" int tt_render_u8(uint8_t* canvas_dev, int Hc, int Wc, const tt_render_item* items_host, const tt_render_item* items_dev,
                            int num_items, void* workspace, long long workspace_bytes, void* stream) {
    TT_REQUIRE(canvas_dev && workspace, "tt_render_u8: null canvas or workspace");
    TT_REQUIRE(num_items >= 0 && num_items <= TT_RENDER_MAX_ITEMS, "tt_render_u8: %d items, 0..%d", num_items, TT_RENDER_MAX_ITEMS);
    TT_REQUIRE(num_items == 0 || (items_host && items_dev), "tt_render_u8: null item table");
    TT_REQUIRE(((uintptr_t)items_dev & 15) == 0 && ((uintptr_t)workspace & 255) == 0,
               "tt_render_u8: misaligned device table or workspace (16, 256 bytes)");
    TT_REQUIRE(Hc >= 1 && Hc <= kMaxSide && Wc >= 1 && Wc <= kMaxSide, "tt_render_u8: a canvas of %d x %d pixels, sides 1..%d", Hc, Wc,
               kMaxSide);
    TT_REQUIRE(workspace_bytes >= up256(8LL * TT_RENDER_STATUS_WORDS), "tt_render_u8: %lld bytes of workspace cannot hold the status words",
               workspace_bytes);
    int bad = -1;
    const char* why = nullptr;
    if (!render_layout(items_host, num_items, workspace_bytes, true, &bad, &why)) {
        char text[160];
        snprintf(text, sizeof(text), why, bad);
        TT_REQUIRE(false, "tt_render_u8: %s", text);
    }
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    bool polys = false;
    for (int i = 0; i < num_items; ++i) {
        const tt_render_item& it = items_host[i];
        polys |= is_poly(it.kind);
        if (it.kind == TT_RENDER_POINTS_BEV && it.count > 0 && it.w > 0 && it.h > 0)
            hipLaunchKernelGGL(render_splat_kernel, dim3((unsigned)div_up(it.count, 256)), dim3(256), 0, st, items_dev, i, Hc, Wc, ws);
    }
    if (polys) hipLaunchKernelGGL(render_count_kernel, dim3(1), dim3(256), 0, st, items_dev, num_items, ws);
    hipLaunchKernelGGL(render_compose_kernel, dim3((unsigned)div_up(Wc, kTileCols), (unsigned)div_up(Hc, kTileRows)), dim3(kTileCols), 0, st,
                       canvas_dev, Hc, Wc, items_dev, num_items, ws);
    return check_launch("tt_render_u8");
}
