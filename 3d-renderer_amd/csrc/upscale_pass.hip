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
#include "temporal_device.h"

#include "upscale_math.h"

namespace {

__global__ __launch_bounds__(TRI_BLOCK) void k_upscale_resolve(TriUpscaleArgs a) {
    const auto [X, Y] = temporal::tile_pixel(a.Wo);
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
        const temporal::WaveId w = temporal::wave_id(id);
        const temporal::Rows R = w.shared ? temporal::load_rows(a.table, w.first) : temporal::load_rows(a.table, id);
        o = upscale::resolve_pixel(R.r, X, Y, sm, rid, depth, a.colour, s, f, true, a.reject_id != 0u, a.alpha, a.prev_ids,
                                   temporal::AccAt{a.prev_acc});
    }
    const uint32_t p = Y * a.Wo + X;
    a.next_acc[p] = make_uint2(o.acc.bg, o.acc.ra);
    a.resolved[p] = o.resolved;
    a.mask[p] = (uint8_t)o.mask;
}

}  // namespace

hipError_t tri_launch_upscale_resolve(const TriUpscaleArgs& args, hipStream_t stream) {
    const uint32_t tiles = temporal::tile_count(args.Wo, args.Ho);
    if (tiles == 0) return hipErrorInvalidValue;
    k_upscale_resolve<<<dim3(tiles), dim3(TRI_BLOCK), 0, stream>>>(args);
    return hipGetLastError();
}
