// history_pass.hip — the history reprojection pass (include/tri_raster.h "history reprojection"): the previous frame's
// colour fetched where each pixel's motion vector points, a mask byte that says where that fetch is not valid, and the
// frame just rendered stored as the next call's previous frame.
//
//   k_reproject<VEC>  a stream over the frame's W x H pixels as one flat array, like k_motion. Per pixel it reads 12 B of
//                     the current frame (colour, id, depth), writes them to the other history set, and writes 4 B of
//                     warped colour and 1 B of mask. VEC = 4: a lane takes four consecutive pixels — one 16-B load of
//                     each current plane, 16-B stores of the three history planes and of the warped colour, one 4-B
//                     store of four mask bytes — and the flat index keeps every access aligned whatever W is (x and y
//                     are carried per pixel); the npix % 4 pixels left over are taken one per lane by the lanes behind
//                     the last vector. VEC = 1: one pixel per lane, for images that do not start on a 16-B boundary (a
//                     caller's tri_bind_output targets). The table row comes through a wave-uniform index when the
//                     wave's pixels share one id, otherwise per pixel from global memory. The gathers — the previous id
//                     and depth at the nearest pixel, four colour taps — go through the caches (a wave's taps fall in a
//                     few neighbouring rows). A lane first locates its four pixels, then issues the fetches of all four,
//                     then resolves them: up to 24 gathers in flight instead of one pixel's dependent chain after
//                     another's. A lane issues no gather for a pixel that has no projection or lies outside (nothing
//                     is read before `inside` holds); the taps of a pixel that ends with the ID or DEPTH bit have
//                     been fetched, every index inside the frame. No LDS, no atomics, plain vector stores.
//
// The per-pixel rule is history::reproject_pixel (history_math.h), the function host/tools/history_check.cpp runs under
// the sanitizers; the unit is built with -ffp-contract=off like the rest of the library, so a float32 restatement gives
// the same bytes.
#define TRI_KERNEL_TU 1
#include "temporal_device.h"

#include "history_math.h"

namespace {

constexpr uint32_t kReprojectMaxBlocks = 2048;  // a grid-stride loop over the rest: 8 workgroups on each of 256 CUs

using temporal::Rows;
using temporal::load_rows;

__device__ __forceinline__ history::Pixel pixel(const Rows& R, uint32_t x, uint32_t y, uint32_t id, float depth, uint32_t colour,
                                                const history::Frame& f, const TriReprojectArgs& a) {
    return history::reproject_pixel(R.r, x, y, id, depth, colour, f, true, a.prev_ids, a.prev_depth, a.prev_colour);
}

template <int VEC>
__global__ __launch_bounds__(TRI_BLOCK) void k_reproject(TriReprojectArgs a) {
    static_assert(VEC == 1 || VEC == 4, "one pixel per lane, or four");
    // work items: nvec vectors of VEC pixels, then the tail pixels one by one; every index below stays < a.npix
    const uint32_t nvec = a.npix / VEC, tail = a.npix - nvec * VEC, items = nvec + tail;
    const uint32_t stride = gridDim.x * TRI_BLOCK;
    const uint32_t last = a.ndraws;  // an id beyond the table cannot come out of the id pass; clamped all the same
    const history::Frame f{a.W, a.H, a.sx, a.sy, a.hw, a.hh, a.tolerance};
    for (uint32_t base = blockIdx.x * TRI_BLOCK; base < items; base += stride) {  // (wave-uniform bound)
        const uint32_t t = base + threadIdx.x;
        if (t >= items) continue;
        if (VEC == 4 && t < nvec) {
            const uint32_t p = t * 4u;
            const uint4 c4 = reinterpret_cast<TRI_G const uint4*>(a.colour)[t];
            const uint4 id4 = reinterpret_cast<TRI_G const uint4*>(a.ids)[t];
            const float4 d4 = reinterpret_cast<TRI_G const float4*>(a.depth)[t];
            reinterpret_cast<TRI_G uint4*>(a.next_colour)[t] = c4;
            reinterpret_cast<TRI_G uint4*>(a.next_ids)[t] = id4;
            reinterpret_cast<TRI_G float4*>(a.next_depth)[t] = d4;
            const uint32_t col[4] = {c4.x, c4.y, c4.z, c4.w};
            history::Pixel o[4];
            if (!a.has_prev) {  // (frame-uniform)
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = history::Pixel{col[k], history::kNoHistory};
            } else {
                const uint32_t rid[4] = {id4.x, id4.y, id4.z, id4.w};  // the rule compares the id as stored
                const uint32_t id[4] = {min(id4.x, last), min(id4.y, last), min(id4.z, last), min(id4.w, last)};
                const float dep[4] = {d4.x, d4.y, d4.z, d4.w};
                uint32_t y = p / a.W, x = p - y * a.W;
                const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)id[0]);
                const bool same = id[0] == first && id[1] == first && id[2] == first && id[3] == first;
                history::Where w[4];
                if (__all(same)) {  // one draw (or the background) under the whole wave: one lookup, broadcast
                    const Rows R = load_rows(a.table, first);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        w[k] = history::locate(R.r, x, y, rid[k], dep[k], f);
                        if (++x == a.W) { x = 0; ++y; }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        w[k] = history::locate(load_rows(a.table, id[k]).r, x, y, rid[k], dep[k], f);
                        if (++x == a.W) { x = 0; ++y; }
                    }
                }
                // every fetch of the lane's four pixels before the first use of any: up to 24 gathers in flight
                history::Fetched g[4] = {};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (!w[k].mask) g[k] = history::fetch(w[k], f, a.prev_ids, a.prev_depth, a.prev_colour);
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = history::resolve(w[k], g[k], rid[k], col[k], f);
            }
            reinterpret_cast<TRI_G uint4*>(a.warped)[t] = make_uint4(o[0].colour, o[1].colour, o[2].colour, o[3].colour);
            reinterpret_cast<TRI_G uint32_t*>(a.mask)[t] = o[0].mask | (o[1].mask << 8) | (o[2].mask << 16) | (o[3].mask << 24);
        } else {
            const uint32_t p = nvec * VEC + (t - nvec);  // VEC == 1: p == t
            const uint32_t colour = a.colour[p], rid = a.ids[p];
            const float depth = a.depth[p];
            a.next_colour[p] = colour;
            a.next_ids[p] = rid;
            a.next_depth[p] = depth;
            history::Pixel o{colour, history::kNoHistory};
            if (a.has_prev) {
                const uint32_t id = min(rid, last);
                const uint32_t y = p / a.W, x = p - y * a.W;
                o = pixel(load_rows(a.table, id), x, y, rid, depth, colour, f, a);
            }
            a.warped[p] = o.colour;
            a.mask[p] = (uint8_t)o.mask;
        }
    }
}

}  // namespace

hipError_t tri_launch_reproject(const TriReprojectArgs& args, bool vec4, hipStream_t stream) {
    const uint32_t items = vec4 ? args.npix / 4u + args.npix % 4u : args.npix;
    const uint32_t blocks = (items + TRI_BLOCK - 1) / TRI_BLOCK;
    const dim3 grid(blocks < 1u ? 1u : (blocks > kReprojectMaxBlocks ? kReprojectMaxBlocks : blocks));
    if (vec4) k_reproject<4><<<grid, dim3(TRI_BLOCK), 0, stream>>>(args);
    else k_reproject<1><<<grid, dim3(TRI_BLOCK), 0, stream>>>(args);
    return hipGetLastError();
}
