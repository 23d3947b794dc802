// upscale_pass.hip — the temporal upscaling pass (include/tri_raster.h "temporal upscaling"): a jittered frame of
// Wr x Hr resolved over an accumulated history of Wo x Ho. Each output pixel takes the render pixel whose jittered sample
// lies nearest, weighs it by the sample's distance from its own centre, fetches the history where its surface lay, clamps
// it to the render frame's 3 x 3 colour range and stores the next history (16-bit), the resolved image (8-bit) and a mask
// byte, all at the output extent.
//
//   k_upscale_resolve  one OUTPUT pixel per lane, a 64 x 4 output tile per 256-thread workgroup, k_taa_resolve's shape: a
//                      wave is 64 horizontally consecutive output pixels of one row, so the stores (8-B, 4-B, 1-B) and,
//                      under small motion, the four 8-B history taps are contiguous across the wave. The render frame is
//                      read through the caches, without an LDS tile: at 2 x a wave's 64 lanes name 32 (or 33) consecutive
//                      render pixels of one row, neighbouring lanes ask for the same address or the next, and the three
//                      window rows are three runs of at most 35 words — the same lines the centre loads brought in. Every
//                      access to the context's planes is a 4-B one, so a caller's tri_bind_output targets may start
//                      anywhere. The table row comes through a wave-uniform index when the wave's pixels share one id,
//                      otherwise per pixel from global memory. Nothing of the previous planes is read before `inside`
//                      holds; every window coordinate is clamped to the render frame. No LDS, no atomics, plain vector
//                      stores. The frame's ids reach the written set through tri_upscale_resolve's copy on the same stream.
//
// The per-pixel rule is upscale::sample and upscale::resolve_pixel (upscale_math.h), the functions
// host/tools/upscale_check.cpp runs under the sanitizers; the unit is built with -ffp-contract=off like the rest of the
// library, so a float32 restatement gives the same bytes.
#define TRI_KERNEL_TU 1
#include "raster_launch.h"

#include "upscale_math.h"

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

// The accumulated history as upscale::resolve_pixel indexes it: one 8-B load per texel.
struct AccAt {
    TRI_G const uint2* p;
    __device__ __forceinline__ taa::Texel operator[](uint32_t i) const {
        const uint2 v = p[i];
        return taa::Texel{v.x, v.y};
    }
};

__global__ __launch_bounds__(TRI_BLOCK) void k_upscale_resolve(TriUpscaleArgs a) {
    const uint32_t tiles_x = (a.Wo + kTileW - 1u) / kTileW;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t X = tx * kTileW + (threadIdx.x & (kTileW - 1u)), Y = ty * kTileH + threadIdx.x / kTileW;
    if (X >= a.Wo || Y >= a.Ho) return;  // every output index below lies inside the output frame
    const upscale::Scale s{a.Wr, a.Hr, a.Wo, a.Ho, a.rx, a.ry, a.ox, a.oy};
    const upscale::Sample sm = upscale::sample(X, Y, s, a.jx, a.jy);  // xr < Wr, yr < Hr: clamped by the rule
    const uint32_t q = sm.yr * a.Wr + sm.xr;
    taa::Pixel o;
    if (!a.has_prev) {  // (frame-uniform)
        o = taa::restart(a.colour[q], upscale::kNoHistory);
    } else {
        const uint32_t rid = a.ids[q];  // the rule compares the id as it is
        const float depth = a.depth[q];
        const uint32_t id = min(rid, a.ndraws);  // an id beyond the table cannot come out of the id pass; clamped all the same
        const history::Frame f{a.Wo, a.Ho, a.sx, a.sy, a.hw, a.hh, 0.0f};
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)id);
        // one draw (or the background) under the whole wave: one lookup, broadcast
        const Rows R = __all(id == first) ? load_rows(a.table, first) : load_rows(a.table, id);
        o = upscale::resolve_pixel(R.r, X, Y, sm, rid, depth, a.colour, s, f, true, a.reject_id != 0u, a.alpha, a.prev_ids,
                                   AccAt{a.prev_acc});
    }
    const uint32_t p = Y * a.Wo + X;
    a.next_acc[p] = make_uint2(o.acc.bg, o.acc.ra);
    a.resolved[p] = o.resolved;
    a.mask[p] = (uint8_t)o.mask;
}

}  // namespace

hipError_t tri_launch_upscale_resolve(const TriUpscaleArgs& args, hipStream_t stream) {
    // at most 2^31 output pixels (history::check_extent): fewer than 2^31 tiles whatever the frame's shape
    const uint64_t tiles = (uint64_t)((args.Wo + kTileW - 1u) / kTileW) * (uint64_t)((args.Ho + kTileH - 1u) / kTileH);
    if (tiles == 0 || tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    k_upscale_resolve<<<dim3((uint32_t)tiles), dim3(TRI_BLOCK), 0, stream>>>(args);
    return hipGetLastError();
}
