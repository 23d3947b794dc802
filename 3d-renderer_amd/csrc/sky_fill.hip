// sky_fill.hip — k_sky_fill: the skybox pass for the cubemaps k_raster's own sky pass does not read (R8G8B8A8_UNORM,
// R16G16B16A16_SFLOAT, mip chains; one-level sRGB too when TRI_SKYBOX_PREFILL asks for it). A full-target pass, one
// lane per pixel, on the context's stream in front of the frame's raster kernel: it writes every pixel's sky colour
// (Skybox.vert:30-41, Skybox.frag:28-35), or the clear colour where the sky does not cover the pixel, and the raster
// kernel then runs with TRI_SKY_PREFILLED and stores the mesh pixels alone. A store-bound pass: IEEE division
// throughout, plain vector stores, no kernel of the raster family grows a register for the new formats.
//
// Direction: sky_ray / sky_persp_dir (raster_bin.h), the functions k_raster's sky pass calls. Face selection,
// LINEAR filtering and the taps across edges and corners are SkyTex's rules (raster_bin.h) applied per level; the
// level of detail follows Vulkan's rules with the choices written at lod() below.
#define TRI_KERNEL_TU 1
#define TRI_PK_SHADE 0
#include "raster_bin.h"

namespace {

// exact binary16 -> binary32 (subnormals, infinities and NaNs included), in integer arithmetic: independent of the
// wave's denormal mode
__device__ __forceinline__ float half_bits_to_float(uint32_t h) {
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 0u) return __uint_as_float(s | __float_as_uint((float)m * 5.9604644775390625e-8f));  // m * 2^-24, exact
    if (e == 31u) return __uint_as_float(s | 0x7F800000u | (m << 13));
    return __uint_as_float(s | ((e + 112u) << 23) | (m << 13));
}

// One level of the cubemap: 6 faces of n x n texels, rows top to bottom.
template <uint32_t FMT>
struct SkyLevel {
    TRI_G const uint32_t* t;  // the level's first texel (4 B per texel; 8 B with TRI_SKY_FMT_RGBA16F)
    int32_t n;
    const float* lut;  // sRGB decode (LDS); unused by the other formats
    __device__ __forceinline__ f3 texel(int face, int32_t i, int32_t j) const {
        const size_t idx = ((size_t)face * (size_t)n + (size_t)j) * (size_t)n + (size_t)i;
        if constexpr (FMT == TRI_SKY_FMT_RGBA16F) {
            const uint2 p = *reinterpret_cast<TRI_G const uint2*>(t + 2 * idx);
            return mk(half_bits_to_float(p.x & 0xFFFFu), half_bits_to_float(p.x >> 16), half_bits_to_float(p.y & 0xFFFFu));
        } else {
            const uint32_t p = t[idx];
            if constexpr (FMT == TRI_SKY_FMT_RGBA8_SRGB) return mk(lut[p & 0xFFu], lut[(p >> 8) & 0xFFu], lut[(p >> 16) & 0xFFu]);
            else return mk((float)(p & 0xFFu) / 255.0f, (float)((p >> 8) & 0xFFu) / 255.0f, (float)((p >> 16) & 0xFFu) / 255.0f);
        }
    }
    // a tap one texel outside the face: the texel of the adjacent face its centre's direction selects
    __device__ __forceinline__ f3 across(int face, int32_t i, int32_t j) const {
        const float sc = 2.0f * (((float)i + 0.5f) / (float)n) - 1.0f;
        const float tc = 2.0f * (((float)j + 0.5f) / (float)n) - 1.0f;
        float s, tt;
        const int f2 = cube_face(face_dir(face, sc, tc), s, tt);
        const int32_t i2 = min(max((int32_t)floorf(s * (float)n), 0), n - 1);
        const int32_t j2 = min(max((int32_t)floorf(tt * (float)n), 0), n - 1);
        return texel(f2, i2, j2);
    }
    __device__ __forceinline__ f3 fetch(int face, int32_t i, int32_t j) const {
        const bool in_i = i >= 0 && i < n, in_j = j >= 0 && j < n;
        if (in_i && in_j) return texel(face, i, j);
        if (in_i || in_j) return across(face, i, j);
        // a corner: the mean of the three texels that meet there
        const int32_t ci = min(max(i, 0), n - 1), cj = min(max(j, 0), n - 1);
        const f3 a = texel(face, ci, cj), b = across(face, i, cj), c = across(face, ci, j);
        return mk(((a.x + b.x) + c.x) / 3.0f, ((a.y + b.y) + c.y) / 3.0f, ((a.z + b.z) + c.z) / 3.0f);
    }
    __device__ __forceinline__ f3 sample(f3 d) const {
        float s, tt;
        const int face = cube_face(d, s, tt);
        const float u = s * (float)n - 0.5f, v = tt * (float)n - 0.5f;
        const float fu = floorf(u), fv = floorf(v);
        const float a = u - fu, bb = v - fv;
        // (s, t in [0, 1], so the taps lie in [-1, n]: fetch() reads no texel outside the level)
        const int32_t i0 = min(max((int32_t)fu, -1), n - 1), j0 = min(max((int32_t)fv, -1), n - 1);
        f3 t00, t10, t01, t11;
        if (i0 >= 0 && i0 + 1 < n && j0 >= 0 && j0 + 1 < n) {  // inside the face (nearly every pixel): four plain loads
            t00 = texel(face, i0, j0); t10 = texel(face, i0 + 1, j0);
            t01 = texel(face, i0, j0 + 1); t11 = texel(face, i0 + 1, j0 + 1);
        } else {  // a tap across an edge or corner of the face
            t00 = fetch(face, i0, j0); t10 = fetch(face, i0 + 1, j0);
            t01 = fetch(face, i0, j0 + 1); t11 = fetch(face, i0 + 1, j0 + 1);
        }
        auto lp = [](float x, float y, float w) { return x + w * (y - x); };
        return mk(lp(lp(t00.x, t10.x, a), lp(t01.x, t11.x, a), bb), lp(lp(t00.y, t10.y, a), lp(t01.y, t11.y, a), bb),
                  lp(lp(t00.z, t10.z, a), lp(t01.z, t11.z, a), bb));
    }
};

// The sampling direction of pixel (px, py) — any pixel of the frame's plane, inside the target or not — or false
// where the sky does not cover it.
__device__ __forceinline__ bool sky_dir(const TriSkyFillArgs& a, int32_t px, int32_t py, f3& d) {
    if (a.mode == TRI_SKY_PERSP) {
        d = sky_persp_dir(a.W, a.H, a.far, px, py);
        return true;
    }
    return sky_ray(
        a.W, a.H, a.ip, a.R, a.pw, px, py, []() { return false; },
        [&](f3 h) {
            d = norm3(h);
            return true;
        });
}

// (s_c, t_c, r_c) of a vector on `face` (Vulkan's cube map face selection table): linear in v, so the same map
// carries the direction's derivatives
__device__ __forceinline__ f3 face_coords(int face, f3 v) {
    switch (face) {
        case 0: return mk(-v.z, -v.y, v.x);
        case 1: return mk(v.z, -v.y, v.x);
        case 2: return mk(v.x, v.z, v.y);
        case 3: return mk(v.x, -v.z, v.y);
        case 4: return mk(v.x, -v.y, v.z);
        default: return mk(-v.x, -v.y, v.z);
    }
}

// The level of detail d = min(clamp(log2 rho_max, 0, mips), mips - 1) of pixel (x, y) with normalised direction P.
// Derivatives: fine quad differences of the normalised direction, quads aligned to even absolute frame coordinates —
// dP/dx = P(right) - P(left) in the pixel's own row, dP/dy likewise down its own column — with the neighbour computed
// from its coordinates (sky or not, inside the viewport and the band or not); a neighbour without a sky direction
// gives a zero derivative. The cube map derivative transformation is applied on the pixel's own face.
__device__ __forceinline__ float lod(const TriSkyFillArgs& a, int32_t x, int32_t y, f3 P) {
    float s, t;
    const int face = cube_face(P, s, t);
    const f3 c = face_coords(face, P);
    const float ma = fabsf(c.z), sgn = c.z >= 0.0f ? 1.0f : -1.0f, r2 = c.z * c.z;
    auto rho = [&](int32_t nx, int32_t ny, bool own_is_second) {
        f3 q;
        if (!sky_dir(a, nx, ny, q)) return 0.0f;
        q = norm3(q);
        const f3 dP = own_is_second ? sub3(P, q) : sub3(q, P);
        const f3 dc = face_coords(face, dP);
        const float dma = sgn * dc.z;
        const float ds = 0.5f * ((ma * dc.x - c.x * dma) / r2);
        const float dt = 0.5f * ((ma * dc.y - c.y * dma) / r2);
        return (float)a.size * sqrtf(ds * ds + dt * dt);
    };
    const float rmax = fmaxf(rho(x ^ 1, y, (x & 1) != 0), rho(x, y ^ 1, (y & 1) != 0));
    if (!(rmax > 0.0f)) return 0.0f;
    const float lambda = fminf(fmaxf(log2f(rmax), 0.0f), (float)a.mips);
    return fminf(lambda, (float)(a.mips - 1u));
}

// One lane per pixel: a wave covers 64 pixels of a row (256-B stores), a workgroup 4 rows.
template <uint32_t FMT, bool MIPPED>
__global__ __launch_bounds__(TRI_BLOCK) void k_sky_fill(const TriSkyFillArgs a) {
    __shared__ float lut[FMT == TRI_SKY_FMT_RGBA8_SRGB ? 256 : 1];
    if constexpr (FMT == TRI_SKY_FMT_RGBA8_SRGB) {
        for (int i = (int)threadIdx.x; i < 256; i += TRI_BLOCK) lut[i] = a.lut[i];
        __syncthreads();
    }
    const int32_t x = (int32_t)(blockIdx.x * 64 + (threadIdx.x & 63));
    const int32_t y = a.y0 + (int32_t)(blockIdx.y * (TRI_BLOCK / 64) + (threadIdx.x >> 6));
    if (x >= a.W || y >= a.y1) return;
    uint32_t out = a.clear_bgra;
    f3 d;
    if (sky_dir(a, x, y, d)) {
        TRI_G const uint32_t* base = (TRI_G const uint32_t*)a.texels;
        constexpr size_t kWords = FMT == TRI_SKY_FMT_RGBA16F ? 2 : 1;  // 4-B words per texel
        f3 c;
        if constexpr (!MIPPED) {
            c = SkyLevel<FMT>{base, (int32_t)a.size, lut}.sample(d);
        } else {
            d = norm3(d);
            const float lv = lod(a, x, y, d);
            const float fl = floorf(lv), delta = lv - fl;
            const uint32_t l0 = (uint32_t)fl, l1 = min(l0 + 1u, a.mips - 1u);
            auto level = [&](uint32_t l) {
                return SkyLevel<FMT>{base + kWords * (size_t)a.level_texel[l], (int32_t)max(1u, a.size >> l), lut};
            };
            c = level(l0).sample(d);
            if (delta > 0.0f) {
                const f3 c1 = level(l1).sample(d);
                c = mk((1.0f - delta) * c.x + delta * c1.x, (1.0f - delta) * c.y + delta * c1.y,
                       (1.0f - delta) * c.z + delta * c1.z);
            }
        }
        out = unorm8(c.z) | (unorm8(c.y) << 8) | (unorm8(c.x) << 16) | (255u << 24);
    }
    a.color[(size_t)(y - a.y0) * (size_t)a.W + (size_t)x] = out;
}

template <uint32_t FMT>
const void* fill_kernel(bool mipped) {
    return mipped ? reinterpret_cast<const void*>(k_sky_fill<FMT, true>) : reinterpret_cast<const void*>(k_sky_fill<FMT, false>);
}

}  // namespace

hipError_t tri_launch_sky_fill(const TriSkyFillArgs& args, hipStream_t stream) {
    if (args.W <= 0 || args.y1 <= args.y0) return hipSuccess;
    const void* k = args.format == TRI_SKY_FMT_RGBA16F      ? fill_kernel<TRI_SKY_FMT_RGBA16F>(args.mips > 1)
                    : args.format == TRI_SKY_FMT_RGBA8_UNORM ? fill_kernel<TRI_SKY_FMT_RGBA8_UNORM>(args.mips > 1)
                                                             : fill_kernel<TRI_SKY_FMT_RGBA8_SRGB>(args.mips > 1);
    const dim3 g((uint32_t)((args.W + 63) / 64), (uint32_t)((args.y1 - args.y0 + TRI_BLOCK / 64 - 1) / (TRI_BLOCK / 64)));
    void* params[] = {const_cast<TriSkyFillArgs*>(&args)};
    return hipLaunchKernel(k, g, dim3(TRI_BLOCK), params, 0, stream);
}
