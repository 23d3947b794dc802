// temporal_device.h — what the kernels of the passes that keep a history across frames share (history_pass.hip,
// taa_pass.hip, upscale_pass.hip): a row of the frame's reprojection table, its wave-uniform lookup, the accumulated
// history as the per-pixel rules index it, and the 64 x 4 tile of the two resolve kernels. Device helpers only; the
// kernels stay in their units' anonymous namespaces, and the per-pixel rules in history_math.h, taa_math.h and
// upscale_math.h.
#pragma once

#ifndef TRI_KERNEL_TU
#error "temporal_device.h: define TRI_KERNEL_TU before the first include (raster_launch.h's address-space qualifier)"
#endif
#include "raster_launch.h"

#include "taa_math.h"

namespace temporal {

// One draw's row of the reprojection table (tri_motion.hip stages it): 16 floats.
struct Rows {
    float r[16];
};

__device__ __forceinline__ Rows load_rows(TRI_G const float* table, uint32_t k) {
    TRI_G const float4* t = reinterpret_cast<TRI_G const float4*>(table) + (size_t)k * 4;  // 64-B rows: 16-B aligned
    const float4 a = t[0], b = t[1], c = t[2], d = t[3];
    return Rows{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w}};
}

// Whether the wave's lanes share one id (clamped to the table by the caller) — one draw, or the background, under the
// whole wave — and that id, wave-uniform: the caller then takes the row through it, one lookup broadcast, and
// otherwise per lane from global memory:
//     const temporal::WaveId w = temporal::wave_id(id);
//     const temporal::Rows R = w.shared ? temporal::load_rows(table, w.first) : temporal::load_rows(table, id);
// (The choice stays in the kernel: as a function returning Rows it compiles to other code.)
struct WaveId {
    uint32_t first;
    bool shared;
};

__device__ __forceinline__ WaveId wave_id(uint32_t id) {
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)id);
    return WaveId{first, __all(id == first) != 0};
}

// The accumulated history as taa::resolve_pixel and upscale::resolve_pixel index it: one 8-B load per texel.
struct AccAt {
    TRI_G const uint2* p;
    __device__ __forceinline__ taa::Texel operator[](uint32_t i) const {
        const uint2 v = p[i];
        return taa::Texel{v.x, v.y};
    }
};

// The resolve kernels' tile: one pixel per lane, 64 x 4 pixels per 256-thread workgroup, so a wave is 64 horizontally
// consecutive pixels of one row.
constexpr uint32_t kTileW = 64, kTileH = TRI_BLOCK / kTileW;
static_assert(kTileW * kTileH == TRI_BLOCK, "a workgroup is one tile");

struct TilePixel {
    uint32_t x, y;
};

// The lane's pixel in a frame `width` wide (it may lie beyond the frame's right or bottom edge: the caller returns).
__device__ __forceinline__ TilePixel tile_pixel(uint32_t width) {
    const uint32_t tiles_x = (width + kTileW - 1u) / kTileW;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    return TilePixel{tx * kTileW + (threadIdx.x & (kTileW - 1u)), ty * kTileH + threadIdx.x / kTileW};
}

// The launchers' grid: at most 2^31 pixels (history::check_extent), so fewer than 2^31 tiles whatever the frame's
// shape; 0 where the extent gives no launchable grid.
inline uint32_t tile_count(uint32_t width, uint32_t height) {
    const uint64_t tiles = (uint64_t)((width + kTileW - 1u) / kTileW) * (uint64_t)((height + kTileH - 1u) / kTileH);
    return tiles > 0x7FFFFFFFull ? 0u : (uint32_t)tiles;
}

}  // namespace temporal
