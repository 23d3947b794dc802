// upscale_math.h — the plain-C++ part of temporal upscaling (include/tri_raster.h "temporal upscaling"): the argument
// rules of tri_upscale's entry points, the jitter period, and the per-pixel resolve rule as inline functions.
// k_upscale_resolve (upscale_pass.hip) and host/tools/upscale_check.cpp both compile upscale::resolve_pixel below: the
// device runs what the sanitizers checked on the CPU. No HIP header is needed; under hipcc the functions are marked for
// both sides. taa_math.h and history_math.h are used as they are: history::locate (at the OUTPUT extent),
// taa::neighbourhood and taa::id_nearby (at the RENDER extent), taa::restart, taa::accumulate, taa::Texel, history::Sets.
//
// Wr x Hr is the render extent (the context's), Wo x Ho the output extent (the object's). The host computes, each as one
// float32 division, rx = (float)Wr / (float)Wo, ry = (float)Hr / (float)Ho, ox = (float)Wo / (float)Wr,
// oy = (float)Ho / (float)Hr. (jx, jy) is the frame's jitter in render pixels, alpha lies in (0, 1].
//
// The rule, in integers and in float32 with no contraction, in exactly this order, for output pixel (X, Y):
//     px = ((float)X + 0.5f) * rx                      py likewise with Y, ry
//     xr = clampi((int)floorf(px + jx), Wr - 1)        yr likewise — the render pixel whose jittered sample lies nearest
//     c, i, d = colour, id, depth of render pixel (xr, yr);  R = the staged motion table's row for i
//     dx = (((float)xr + 0.5f) - jx) * ox - ((float)X + 0.5f)      dy likewise — the sample minus the output centre, output px
//     k  = fmaxf(0.0f, 1.0f - fabsf(dx)) * fmaxf(0.0f, 1.0f - fabsf(dy))       a = alpha * k
//     NO_HISTORY (1): the object holds no previous frame; the mask is then exactly 1 everywhere
//     w = history::locate(R, X, Y, i, d, make_frame(Wo, Ho, 0))    bits 2 NO_PROJ / 4 OUTSIDE; taps, fu, fv, at: OUTPUT extent
//     with TRI_UPSCALE_REJECT_ID, only when inside:
//         xi = at % Wo, yi = at / Wo;   xq = min((int)(((float)xi + 0.5f) * rx), Wr - 1),   yq likewise
//         ID (8) iff !taa::id_nearby(I', yq * Wr + xq, i, Wr, Hr)    — I': the previous ids, RENDER extent, 3 x 3 clamped
//     n = taa::neighbourhood(colour, xr, yr, Wr, Hr)               — the 3 x 3 range of the render frame, as bytes
//     valid (mask & 15 == 0):  taa::accumulate(c, n, the four taps of A' (output extent), fu, fv, a) — its bit 32 CLAMPED
//                              NO_SAMPLE (64) in addition iff k == 0.0f (the frame added nothing to this pixel)
//     invalid:                 taa::restart(c, mask)               — the nearest sample, whatever k is
//     stored: A[Y][X] (4 x uint16), resolved[Y][X] (B8G8R8A8), mask[Y][X] at the output extent;
//             I[y][x] = ids[y][x] for every render pixel
// No index is formed from the previous position before `inside` holds; every window coordinate is clamped.
//
// At a scale of 1 (Wo == Wr, Ho == Hr) this is NOT tri_taa's rule: xr = X and dx = -jx, so the current frame's weight is
// a = alpha * (1 - |jx|)(1 - |jy|) instead of alpha — a sample far from the pixel's centre counts for less.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "taa_math.h"

namespace upscale {

using history::Msg;

constexpr uint32_t kNoHistory = TRI_UPSCALE_NO_HISTORY, kNoProj = TRI_UPSCALE_NO_PROJ, kOutside = TRI_UPSCALE_OUTSIDE,
                   kId = TRI_UPSCALE_ID, kClamped = TRI_UPSCALE_CLAMPED, kNoSample = TRI_UPSCALE_NO_SAMPLE;
static_assert(kNoProj == history::kNoProj && kOutside == history::kOutside && kNoHistory == taa::kNoHistory &&
                  kId == taa::kId && kClamped == taa::kClamped,
              "the bits history::locate and taa::accumulate set are the mask's");
constexpr uint32_t kMaxScale = 3, kMaxSide = 0x40000000u;

// ---- the argument rules (host only) -----------------------------------------------------------------------------------
// tri_upscale_create: both extents are history extents, and the output is 1 to 3 times the render extent per axis.
// No side above 2^30: the rule turns pixel coordinates into float32 and back into int, and the windows it shares with
// taa_math.h index with int; up to 2^30 every such cast is in range (2^31 - 1 already rounds to 2^31 as a float).
inline int check_extents(uint32_t rw, uint32_t rh, uint32_t ow, uint32_t oh, Msg& m) {
    if (const int rc = history::check_extent(rw, rh, m)) return rc;
    if (const int rc = history::check_extent(ow, oh, m)) return rc;
    if (rw > kMaxSide || rh > kMaxSide || ow > kMaxSide || oh > kMaxSide) {
        std::snprintf(m.text, sizeof m.text, "a side above 2^30 pixels");
        return TRI_E_INVALID;
    }
    if (ow < rw || oh < rh || (uint64_t)ow > (uint64_t)kMaxScale * rw || (uint64_t)oh > (uint64_t)kMaxScale * rh) {
        std::snprintf(m.text, sizeof m.text, "an output of %u x %u from a render of %u x %u (1 to %u times per axis)", ow, oh, rw,
                      rh, kMaxScale);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}

// tri_upscale_resolve's parameters.
inline int check_params(const tri_upscale_params* p, Msg& m) {
    if (!p) {
        std::snprintf(m.text, sizeof m.text, "null parameters");
        return TRI_E_INVALID;
    }
    if (!(p->alpha > 0.0f && p->alpha <= 1.0f)) {  // (NaN fails the first test)
        std::snprintf(m.text, sizeof m.text, "an alpha of %g (0 < alpha <= 1)", (double)p->alpha);
        return TRI_E_INVALID;
    }
    for (int k = 0; k < 2; ++k)
        if (!(__builtin_fabsf(p->jitter[k]) <= 0.5f)) {  // (NaN and the infinities fail it)
            std::snprintf(m.text, sizeof m.text, "a jitter of %g (at most half a render pixel)", (double)p->jitter[k]);
            return TRI_E_INVALID;
        }
    const uint32_t known = TRI_UPSCALE_REDO | TRI_UPSCALE_REJECT_ID;
    if (p->flags & ~known) {
        std::snprintf(m.text, sizeof m.text, "unknown flag bits 0x%x", p->flags & ~known);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}

// tri_upscale_jitter_period: eight samples per output pixel's area, min(64, ceil(8 (Wo / Wr) (Ho / Hr))) in double.
inline int jitter_period(uint32_t rw, uint32_t rh, uint32_t ow, uint32_t oh, uint32_t* period, Msg& m) {
    if (!period) {
        std::snprintf(m.text, sizeof m.text, "null argument");
        return TRI_E_INVALID;
    }
    *period = 0;
    if (const int rc = check_extents(rw, rh, ow, oh, m)) return rc;
    const double n = std::ceil(8.0 * ((double)ow / (double)rw) * ((double)oh / (double)rh));
    *period = n > (double)taa::kMaxPeriod ? taa::kMaxPeriod : (uint32_t)n;
    return TRI_OK;
}

// ---- the per-pixel rule -----------------------------------------------------------------------------------------------
// Both extents and the four ratios, float32 from the host.
struct Scale {
    uint32_t Wr, Hr, Wo, Ho;
    float rx, ry, ox, oy;  // Wr / Wo, Hr / Ho, Wo / Wr, Ho / Hr
};
inline Scale make_scale(uint32_t Wr, uint32_t Hr, uint32_t Wo, uint32_t Ho) {
    return Scale{Wr, Hr, Wo, Ho, (float)Wr / (float)Wo, (float)Hr / (float)Ho, (float)Wo / (float)Wr, (float)Ho / (float)Hr};
}

// The render pixel an output pixel takes its sample from, and the sample's weight: arithmetic alone. A caller reads the
// id at (xr, yr) next, which names the table row resolve_pixel needs.
struct Sample {
    uint32_t xr, yr;
    float k;
};
TRI_HIST_FN Sample sample(uint32_t X, uint32_t Y, const Scale& s, float jx, float jy) {
    const float cx = (float)X + 0.5f, cy = (float)Y + 0.5f;
    const float px = cx * s.rx, py = cy * s.ry;
    const int xr = history::clampi((int)__builtin_floorf(px + jx), (int)s.Wr - 1);
    const int yr = history::clampi((int)__builtin_floorf(py + jy), (int)s.Hr - 1);
    const float dx = (((float)xr + 0.5f) - jx) * s.ox - cx;
    const float dy = (((float)yr + 0.5f) - jy) * s.oy - cy;
    const float k = __builtin_fmaxf(0.0f, 1.0f - __builtin_fabsf(dx)) * __builtin_fmaxf(0.0f, 1.0f - __builtin_fabsf(dy));
    return Sample{(uint32_t)xr, (uint32_t)yr, k};
}

// The nearest previous output pixel `at` (inside the output frame) as an index into the render-extent planes.
TRI_HIST_FN uint32_t render_index(uint32_t at, const Scale& s) {
    const uint32_t yi = at / s.Wo, xi = at - yi * s.Wo;
    const int xq = (int)(((float)xi + 0.5f) * s.rx), yq = (int)(((float)yi + 0.5f) * s.ry);  // >= 0
    const int xmax = (int)s.Wr - 1, ymax = (int)s.Hr - 1;
    return (uint32_t)(yq > ymax ? ymax : yq) * s.Wr + (uint32_t)(xq > xmax ? xmax : xq);
}

// The rule for output pixel (X, Y) once its sample is known. R: the table row of id; colour: the current frame's Wr x Hr
// plane (the centre and the 3 x 3 window are read from it); prev_ids: the previous Wr x Hr ids, prev_acc: the previous
// Wo x Ho accumulated colour, both read only where the pixel is inside (never when has_prev is false). The pointer types
// are the caller's (the kernel passes global-address-space pointers).
template <typename ColourPtr, typename IdPtr, typename AccPtr>
TRI_HIST_FN taa::Pixel resolve_pixel(const float* R, uint32_t X, uint32_t Y, const Sample& sm, uint32_t id, float depth,
                                     ColourPtr colour, const Scale& s, const history::Frame& out, bool has_prev, bool reject_id,
                                     float alpha, IdPtr prev_ids, AccPtr prev_acc) {
    const uint32_t c = colour[sm.yr * s.Wr + sm.xr];
    if (!has_prev) return taa::restart(c, kNoHistory);
    // the reads in k_taa_resolve's order: the window ahead of the branches, the taps and the nine ids together
    const taa::Range n = taa::neighbourhood(colour, sm.xr, sm.yr, s.Wr, s.Hr);
    const history::Where w = history::locate(R, X, Y, id, depth, out);
    if (w.mask) return taa::restart(c, w.mask);
    taa::Texel t[4];
    for (int k = 0; k < 4; ++k) t[k] = prev_acc[w.tap[k]];
    const bool rejected = reject_id && !taa::id_nearby(prev_ids, render_index(w.at, s), id, s.Wr, s.Hr);
    if (rejected) return taa::restart(c, kId);
    taa::Pixel o = taa::accumulate(c, n, t, w.fu, w.fv, alpha * sm.k);
    if (sm.k == 0.0f) o.mask |= kNoSample;
    return o;
}

}  // namespace upscale
