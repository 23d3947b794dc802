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
#include "temporal_device.h"

#include "taa_math.h"

namespace {

__global__ __launch_bounds__(TRI_BLOCK) void k_taa_resolve(TriTaaArgs a) {
    const auto [x, y] = temporal::tile_pixel(a.W);
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
        const temporal::WaveId w = temporal::wave_id(id);
        const temporal::Rows R = w.shared ? temporal::load_rows(a.table, w.first) : temporal::load_rows(a.table, id);
        o = taa::resolve_pixel(R.r, x, y, rid, depth, a.colour, f, true, a.reject_id != 0u, a.alpha, a.prev_ids, temporal::AccAt{a.prev_acc});
    }
    a.next_acc[p] = make_uint2(o.acc.bg, o.acc.ra);
    a.next_ids[p] = rid;
    a.resolved[p] = o.resolved;
    a.mask[p] = (uint8_t)o.mask;
}

}  // namespace

hipError_t tri_launch_taa_resolve(const TriTaaArgs& args, hipStream_t stream) {
    const uint32_t tiles = temporal::tile_count(args.W, args.H);
    if (tiles == 0) return hipErrorInvalidValue;
    k_taa_resolve<<<dim3(tiles), dim3(TRI_BLOCK), 0, stream>>>(args);
    return hipGetLastError();
}
