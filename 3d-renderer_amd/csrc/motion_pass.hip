// motion_pass.hip — the motion-vector pass (include/tri_raster.h "motion vectors"): where the surface under each pixel
// lay one frame ago, from the pixel's id, its depth and one 4 x 4 reprojection matrix per draw (motion_math.h).
//
//   k_motion<VEC>  a stream over the context's W x rows pixels as one flat array, behind the frame's raster kernel. Per
//                  pixel it reads 4 B of id and 4 B of depth and writes 8 B of motion. VEC = 4: a lane takes four
//                  consecutive pixels — one 16-B load of each input, two 16-B stores — and the flat index keeps every
//                  access 16-B aligned whatever W is (a lane's pixels may straddle a row end: x and y are carried per
//                  pixel); the npix % 4 pixels left over are taken one per lane by the lanes behind the last vector.
//                  VEC = 1: one pixel per lane, for images that do not start on a 16-B boundary (a caller's depth
//                  target). The table row is the only gather. A wave whose pixels all carry one id — the common
//                  case — reads its three rows once through a wave-uniform index (scalar loads, broadcast); a mixed
//                  wave gathers per pixel from global memory, which any draw count fits. No LDS, no atomics.
//
// The arithmetic is motion::pixel_motion's, operation for operation; the unit is built with -ffp-contract=off like the
// rest of the library, so a float32 restatement gives the same bits.
#define TRI_KERNEL_TU 1
#include "raster_launch.h"

namespace {

constexpr uint32_t kMotionMaxBlocks = 2048;  // a grid-stride loop over the rest: 8 workgroups on each of 256 CUs

// Rows 0, 1 and 3 of R_k: all that x, y and w need.
struct MotionRows {
    float4 r0, r1, r3;
};

__device__ __forceinline__ MotionRows load_rows(TRI_G const float* table, uint32_t k) {
    TRI_G const float4* t = reinterpret_cast<TRI_G const float4*>(table) + (size_t)k * 4;  // 64-B rows: 16-B aligned
    return MotionRows{t[0], t[1], t[3]};
}

__device__ __forceinline__ float2 pixel_motion(const MotionRows& R, uint32_t x, uint32_t y, uint32_t id, float depth,
                                               const TriMotionArgs& a) {
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    const float xn = fx * a.sx - 1.0f, yn = fy * a.sy - 1.0f;
    const float z = id ? depth : 1.0f;
    const float q0 = ((R.r0.x * xn + R.r0.y * yn) + R.r0.z * z) + R.r0.w;
    const float q1 = ((R.r1.x * xn + R.r1.y * yn) + R.r1.z * z) + R.r1.w;
    const float q3 = ((R.r3.x * xn + R.r3.y * yn) + R.r3.z * z) + R.r3.w;
    float2 m = make_float2(0.0f, 0.0f);
    if (q3 > 0.0f) {  // (false for NaN)
        const float iw = 1.0f / q3;
        const float mx = (q0 * iw - xn) * a.hw, my = (q1 * iw - yn) * a.hh;
        if (isfinite(mx) && isfinite(my)) m = make_float2(mx, my);
    }
    return m;
}

template <int VEC>
__global__ __launch_bounds__(TRI_BLOCK) void k_motion(TriMotionArgs a) {
    static_assert(VEC == 1 || VEC == 4, "one pixel per lane, or four");
    // work items: nvec vectors of VEC pixels, then the tail pixels one by one; every index below stays < a.npix
    const uint32_t nvec = a.npix / VEC, tail = a.npix - nvec * VEC, items = nvec + tail;
    const uint32_t stride = gridDim.x * TRI_BLOCK;
    const uint32_t last = a.ndraws;  // an id beyond the table cannot come out of the id pass; clamped all the same
    for (uint32_t base = blockIdx.x * TRI_BLOCK; base < items; base += stride) {  // (wave-uniform bound)
        const uint32_t t = base + threadIdx.x;
        if (t >= items) continue;
        if (VEC == 4 && t < nvec) {
            const uint32_t p = t * 4u;
            const uint4 id4 = reinterpret_cast<TRI_G const uint4*>(a.ids)[t];
            const float4 d4 = reinterpret_cast<TRI_G const float4*>(a.depth)[t];
            const uint32_t id[4] = {min(id4.x, last), min(id4.y, last), min(id4.z, last), min(id4.w, last)};
            const float dep[4] = {d4.x, d4.y, d4.z, d4.w};
            uint32_t y = p / a.W, x = p - y * a.W;
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)id[0]);
            const bool same = id[0] == first && id[1] == first && id[2] == first && id[3] == first;
            float2 m[4];
            if (__all(same)) {  // one draw (or the background) under the whole wave: one lookup, broadcast
                const MotionRows R = load_rows(a.table, first);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    m[k] = pixel_motion(R, x, a.y0 + y, id[k], dep[k], a);
                    if (++x == a.W) { x = 0; ++y; }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    m[k] = pixel_motion(load_rows(a.table, id[k]), x, a.y0 + y, id[k], dep[k], a);
                    if (++x == a.W) { x = 0; ++y; }
                }
            }
            TRI_G float4* out = reinterpret_cast<TRI_G float4*>(a.motion) + (size_t)t * 2;
            out[0] = make_float4(m[0].x, m[0].y, m[1].x, m[1].y);
            out[1] = make_float4(m[2].x, m[2].y, m[3].x, m[3].y);
        } else {
            const uint32_t p = nvec * VEC + (t - nvec);  // VEC == 1: p == t
            const uint32_t id = min(a.ids[p], last);
            const uint32_t y = p / a.W, x = p - y * a.W;
            const float2 m = pixel_motion(load_rows(a.table, id), x, a.y0 + y, id, a.depth[p], a);
            reinterpret_cast<TRI_G float2*>(a.motion)[p] = m;
        }
    }
}

}  // namespace

const void* tri_motion_kernel(bool vec4) {
    return vec4 ? reinterpret_cast<const void*>(k_motion<4>) : reinterpret_cast<const void*>(k_motion<1>);
}

dim3 tri_motion_grid(uint32_t npix, bool vec4) {
    const uint32_t items = vec4 ? npix / 4u + npix % 4u : npix;
    const uint32_t blocks = (items + TRI_BLOCK - 1) / TRI_BLOCK;
    return dim3(blocks < 1u ? 1u : (blocks > kMotionMaxBlocks ? kMotionMaxBlocks : blocks));
}
