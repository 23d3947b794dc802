// taa_pass.hip — the temporal anti-aliasing pass (include/tri_raster.h "temporal anti-aliasing"): the accumulated
// history fetched where each pixel's surface lay, clamped to the current frame's 3 x 3 colour range, mixed with the
// current colour and stored as the next history (16-bit) and as the resolved image (8-bit), with a mask byte.
//
//   k_taa_resolve  one pixel per lane, a 64 x 4 tile per 256-thread workgroup: a wave is 64 horizontally consecutive
//                  pixels of one row, so the current planes' loads, the 3 x 3 window's nine loads (three rows, each
//                  lane's neighbours are its neighbour lanes' centres: the same cache lines) and every store are
//                  contiguous across the wave, and the four 8-B history taps of neighbouring lanes are 8 B apart
//                  (k_reproject<4>'s were 16 B apart across lanes, which limited it). Every access to the context's
//                  planes is a 4-B one, so a caller's tri_bind_output targets may start anywhere and no second variant
//                  is needed; the object's own planes take 8-B, 4-B and 1-B stores. The table row comes through a
//                  wave-uniform index when the wave's pixels share one id, otherwise per pixel from global memory, as in
//                  k_reproject. Nothing of the previous planes is read before `inside` holds; every window coordinate is
//                  clamped to the frame. No LDS, no atomics, plain vector stores.
//
// The per-pixel rule is taa::resolve_pixel (taa_math.h), the function host/tools/taa_check.cpp runs under the
// sanitizers; the unit is built with -ffp-contract=off like the rest of the library, so a float32 restatement gives the
// same bytes.
#define TRI_KERNEL_TU 1
#include "raster_launch.h"

#include "taa_math.h"

namespace {

constexpr uint32_t kTileW = 64, kTileH = TRI_BLOCK / kTileW;
static_assert(kTileW * kTileH == TRI_BLOCK, "a workgroup is one tile");

struct Rows {
    float r[16];
};

__device__ __forceinline__ Rows load_rows(TRI_G const float* table, uint32_t k) {
    TRI_G const float4* t = reinterpret_cast<TRI_G const float4*>(table) + (size_t)k * 4;  // 64-B rows: 16-B aligned
    const float4 a = t[0], b = t[1], c = t[2], d = t[3];
    return Rows{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w}};
}

// The accumulated history as taa::resolve_pixel indexes it: one 8-B load per texel.
struct AccAt {
    TRI_G const uint2* p;
    __device__ __forceinline__ taa::Texel operator[](uint32_t i) const {
        const uint2 v = p[i];
        return taa::Texel{v.x, v.y};
    }
};

__global__ __launch_bounds__(TRI_BLOCK) void k_taa_resolve(TriTaaArgs a) {
    const uint32_t tiles_x = (a.W + kTileW - 1u) / kTileW;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t x = tx * kTileW + (threadIdx.x & (kTileW - 1u)), y = ty * kTileH + threadIdx.x / kTileW;
    if (x >= a.W || y >= a.H) return;  // every index below lies inside the frame
    const uint32_t p = y * a.W + x;
    const uint32_t rid = a.ids[p];  // the rule compares and stores the id as it is
    taa::Pixel o;
    if (!a.has_prev) {  // (frame-uniform)
        o = taa::restart(a.colour[p], taa::kNoHistory);
    } else {
        const float depth = a.depth[p];
        const uint32_t id = min(rid, a.ndraws);  // an id beyond the table cannot come out of the id pass; clamped all the same
        const history::Frame f{a.W, a.H, a.sx, a.sy, a.hw, a.hh, 0.0f};
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)id);
        // one draw (or the background) under the whole wave: one lookup, broadcast
        const Rows R = __all(id == first) ? load_rows(a.table, first) : load_rows(a.table, id);
        o = taa::resolve_pixel(R.r, x, y, rid, depth, a.colour, f, true, a.reject_id != 0u, a.alpha, a.prev_ids, AccAt{a.prev_acc});
    }
    a.next_acc[p] = make_uint2(o.acc.bg, o.acc.ra);
    a.next_ids[p] = rid;
    a.resolved[p] = o.resolved;
    a.mask[p] = (uint8_t)o.mask;
}

}  // namespace

hipError_t tri_launch_taa_resolve(const TriTaaArgs& args, hipStream_t stream) {
    // at most 2^31 pixels (history::check_extent): fewer than 2^31 tiles whatever the frame's shape
    const uint64_t tiles = (uint64_t)((args.W + kTileW - 1u) / kTileW) * (uint64_t)((args.H + kTileH - 1u) / kTileH);
    if (tiles == 0 || tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    k_taa_resolve<<<dim3((uint32_t)tiles), dim3(TRI_BLOCK), 0, stream>>>(args);
    return hipGetLastError();
}
