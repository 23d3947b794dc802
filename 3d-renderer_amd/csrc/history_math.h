// history_math.h — the plain-C++ part of the history reprojection pass (include/tri_raster.h "history reprojection"):
// the argument rules of its entry points and the per-pixel rule as ONE inline function. k_reproject
// (history_pass.hip) and host/tools/history_check.cpp both compile reproject_pixel below: the device runs what the
// sanitizers checked on the CPU. No HIP header is needed; under hipcc the functions are marked for both sides.
//
// The rule, in float32 with no contraction and in exactly this order (R: the pixel's row of the frame's motion table,
// i / d / c its current id, depth and colour; I', D', C' the stored previous frame; W x H the frame):
//     fx, fy, xn, yn, z, q_0, q_1, q_3, iw, m      as motion::pixel_motion (m is what k_motion stores, zeros included)
//     q_2  = ((R[2][0] * xn + R[2][1] * yn) + R[2][2] * z) + R[2][3]
//     proj = q_3 > 0.0f and m.x, m.y finite before the zeroing
//     u = fx + m.x     v = fy + m.y                 (the previous position, pixel centres at + 0.5)
//     inside = proj && u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H
//     xi = (int)floorf(u)   yi = (int)floorf(v)     only when inside
//     i' = I'[yi][xi]       d' = i' ? D'[yi][xi] : 1.0f        zp = q_2 * iw
// Mask bits: 1 NO_HISTORY (no previous frame: the mask is exactly 1), 2 NO_PROJ (!proj), 4 OUTSIDE (proj && !inside),
// 8 ID (inside && i' != i), 16 DEPTH (inside && i' == i && i != 0 && tolerance > 0 && !(fabsf(zp - d') <= tolerance)).
// Where the mask is 0 the colour is the bilinear fetch of C' at (u - 0.5, v - 0.5), taps clamped to the frame, per
// channel  t = c00 * (1 - fu) + c10 * fu,  b = c01 * (1 - fu) + c11 * fu,  r = t * (1 - fv) + b * fv,
// out = min((int)(r + 0.5f), 255); elsewhere it is the current colour, unchanged. No index is formed from u, v or what
// follows from them before `inside` has been tested: they may be NaN or huge.
#pragma once

#include <cstdint>
#include <cstdio>

#include "../../include/tri_raster.h"

#if defined(__HIPCC__)
#define TRI_HIST_FN __host__ __device__ inline
#else
#define TRI_HIST_FN inline
#endif

namespace history {

constexpr uint32_t kNoHistory = TRI_REPROJECT_NO_HISTORY, kNoProj = TRI_REPROJECT_NO_PROJ, kOutside = TRI_REPROJECT_OUTSIDE,
                   kId = TRI_REPROJECT_ID, kDepth = TRI_REPROJECT_DEPTH;

struct Msg {
    char text[160] = {0};
};

// tri_history_create: W x H >= 1 each (and within the renderer's limit), at most 2^31 pixels.
inline int check_extent(uint32_t width, uint32_t height, Msg& m) {
    if (width == 0 || height == 0) {
        std::snprintf(m.text, sizeof m.text, "an extent of %u x %u", width, height);
        return TRI_E_INVALID;
    }
    if ((uint64_t)width * (uint64_t)height > 0x80000000ull) {
        std::snprintf(m.text, sizeof m.text, "%u x %u is more than 2^31 pixels", width, height);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}

// tri_history_reproject's parameters.
inline int check_params(const tri_reproject_params* p, Msg& m) {
    if (!p) {
        std::snprintf(m.text, sizeof m.text, "null parameters");
        return TRI_E_INVALID;
    }
    if (!(p->depth_tolerance >= 0.0f) || !__builtin_isfinite(p->depth_tolerance)) {  // (NaN fails the first test)
        std::snprintf(m.text, sizeof m.text, "a depth tolerance of %g", (double)p->depth_tolerance);
        return TRI_E_INVALID;
    }
    if (p->flags & ~(uint32_t)TRI_HISTORY_REDO) {
        std::snprintf(m.text, sizeof m.text, "unknown flag bits 0x%x", p->flags & ~(uint32_t)TRI_HISTORY_REDO);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}

// The object against the context it is asked to read.
inline int check_context(int device, uint32_t width, uint32_t height, int ctx_device, uint32_t ctx_width, uint32_t ctx_height,
                         Msg& m) {
    if (device != ctx_device) {
        std::snprintf(m.text, sizeof m.text, "the context is on device %d, the history on %d", ctx_device, device);
        return TRI_E_INVALID;
    }
    if (width != ctx_width || height != ctx_height) {
        std::snprintf(m.text, sizeof m.text, "the context is %u x %u, the history %u x %u", ctx_width, ctx_height, width, height);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}

// Which set a call reads and which it stores into. The sets swap at the start of a call, unless it is a redo (or the
// first call since create / reset, which has nothing to swap): a redo reads the set the last call read and overwrites
// what that call stored.
struct Sets {
    bool ran = false;         // a call has stored a frame since create / reset
    uint32_t read = 0;        // the set the last call read; it stored into read ^ 1
    bool read_valid = false;  // ... and whether that set held a frame
    void reset() { ran = false; read_valid = false; }
    // Start a call: returns the set to read (valid: whether it holds a frame); the call stores into the other one.
    uint32_t begin(bool redo, bool* valid) {
        if (!ran) read_valid = false;
        else if (!redo) { read ^= 1u; read_valid = true; }
        ran = true;
        *valid = read_valid;
        return read;
    }
};

// The frame's constants, float32 from the host as k_motion's.
struct Frame {
    uint32_t W, H;
    float sx, sy, hw, hh;  // 2 / W, 2 / H, W / 2, H / 2
    float tolerance;
};
inline Frame make_frame(uint32_t W, uint32_t H, float tolerance) {
    return Frame{W, H, 2.0f / (float)W, 2.0f / (float)H, 0.5f * (float)W, 0.5f * (float)H, tolerance};
}

struct Pixel {
    uint32_t colour;  // B G R A in memory order
    uint32_t mask;
};

TRI_HIST_FN int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One channel of the bilinear fetch (sh: the channel's bit position).
TRI_HIST_FN uint32_t blend(uint32_t c00, uint32_t c10, uint32_t c01, uint32_t c11, int sh, float fu, float fv) {
    const float a = (float)((c00 >> sh) & 0xFFu), b = (float)((c10 >> sh) & 0xFFu);
    const float c = (float)((c01 >> sh) & 0xFFu), d = (float)((c11 >> sh) & 0xFFu);
    const float t = a * (1.0f - fu) + b * fu;
    const float bt = c * (1.0f - fu) + d * fu;
    const float r = t * (1.0f - fv) + bt * fv;
    const int o = (int)(r + 0.5f);
    return (uint32_t)(o > 255 ? 255 : o) << sh;
}

// The rule in three steps, so that a caller with several pixels in hand (the kernel: four per lane) can take the first
// step for all of them, then issue every fetch, then finish — the fetches of all pixels are in flight together instead of
// one pixel's chain after another's. reproject_pixel below is the three in a row.

// Step 1, arithmetic alone: where the pixel lay, and which elements of the previous planes the rule reads.
struct Where {
    uint32_t mask;    // kNoProj, kOutside, or 0: inside — only then are the fields below set and may anything be fetched
    uint32_t at;      // the nearest previous pixel: I' and D' (indices fit: at most 2^31 pixels)
    uint32_t tap[4];  // the taps (x0, y0) (x0+1, y0) (x0, y0+1) (x0+1, y0+1), clamped to the frame
    float fu, fv, zp;
};

// R: the 16 floats of the pixel's table row, row-major.
TRI_HIST_FN Where locate(const float* R, uint32_t x, uint32_t y, uint32_t id, float depth, const Frame& f) {
    Where w{};
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    const float xn = fx * f.sx - 1.0f, yn = fy * f.sy - 1.0f;
    const float z = id ? depth : 1.0f;
    const float q0 = ((R[0] * xn + R[1] * yn) + R[2] * z) + R[3];
    const float q1 = ((R[4] * xn + R[5] * yn) + R[6] * z) + R[7];
    const float q2 = ((R[8] * xn + R[9] * yn) + R[10] * z) + R[11];
    const float q3 = ((R[12] * xn + R[13] * yn) + R[14] * z) + R[15];
    w.mask = kNoProj;
    if (!(q3 > 0.0f)) return w;  // (NaN too)
    const float iw = 1.0f / q3;
    const float mx = (q0 * iw - xn) * f.hw, my = (q1 * iw - yn) * f.hh;
    if (!__builtin_isfinite(mx) || !__builtin_isfinite(my)) return w;
    const float u = fx + mx, v = fy + my;
    const bool inside = u >= 0.0f && u < (float)f.W && v >= 0.0f && v < (float)f.H;
    w.mask = kOutside;
    if (!inside) return w;
    // 0 <= u < W and 0 <= v < H from here on: every index below lies inside the frame
    w.mask = 0u;
    const int xi = (int)__builtin_floorf(u), yi = (int)__builtin_floorf(v);
    w.at = (uint32_t)yi * f.W + (uint32_t)xi;
    w.zp = q2 * iw;
    const float su = u - 0.5f, sv = v - 0.5f;
    const float x0 = __builtin_floorf(su), y0 = __builtin_floorf(sv);  // -1 .. W - 1, -1 .. H - 1
    w.fu = su - x0;
    w.fv = sv - y0;
    const int xmax = (int)f.W - 1, ymax = (int)f.H - 1;
    const uint32_t xa = (uint32_t)clampi((int)x0, xmax), xb = (uint32_t)clampi((int)x0 + 1, xmax);
    const uint32_t ra = (uint32_t)clampi((int)y0, ymax) * f.W, rb = (uint32_t)clampi((int)y0 + 1, ymax) * f.W;
    w.tap[0] = ra + xa;
    w.tap[1] = ra + xb;
    w.tap[2] = rb + xa;
    w.tap[3] = rb + xb;
    return w;
}

// Step 2: what was fetched for a pixel that is inside. The depth is fetched only under a tolerance > 0 (it decides
// nothing otherwise); every element lies inside the frame whatever id the previous pixel has.
struct Fetched {
    uint32_t id;
    float depth;
    uint32_t c[4];
};
template <typename IdPtr, typename DepthPtr, typename ColourPtr>
TRI_HIST_FN Fetched fetch(const Where& w, const Frame& f, IdPtr prev_ids, DepthPtr prev_depth, ColourPtr prev_colour) {
    Fetched g{};
    g.id = prev_ids[w.at];
    if (f.tolerance > 0.0f) g.depth = prev_depth[w.at];
    for (int k = 0; k < 4; ++k) g.c[k] = prev_colour[w.tap[k]];
    return g;
}

// Step 3: the bits that need the previous frame, and the colour. (g.id == id != 0 at the depth test: the stored depth,
// not the background's 1.)
TRI_HIST_FN Pixel resolve(const Where& w, const Fetched& g, uint32_t id, uint32_t colour, const Frame& f) {
    if (w.mask) return Pixel{colour, w.mask};
    if (g.id != id) return Pixel{colour, kId};
    if (id != 0 && f.tolerance > 0.0f && !(__builtin_fabsf(w.zp - g.depth) <= f.tolerance)) return Pixel{colour, kDepth};
    uint32_t out = 0;
    for (int sh = 0; sh < 32; sh += 8) out |= blend(g.c[0], g.c[1], g.c[2], g.c[3], sh, w.fu, w.fv);
    return Pixel{out, 0u};
}

// The rule for pixel (x, y). prev_*: the previous frame's W x H planes, read only where the pixel is inside (never when
// has_prev is false). The pointer types are the caller's (the kernel passes global-address-space pointers).
template <typename IdPtr, typename DepthPtr, typename ColourPtr>
TRI_HIST_FN Pixel reproject_pixel(const float* R, uint32_t x, uint32_t y, uint32_t id, float depth, uint32_t colour,
                                  const Frame& f, bool has_prev, IdPtr prev_ids, DepthPtr prev_depth, ColourPtr prev_colour) {
    if (!has_prev) return Pixel{colour, kNoHistory};
    const Where w = locate(R, x, y, id, depth, f);
    Fetched g{};
    if (!w.mask) g = fetch(w, f, prev_ids, prev_depth, prev_colour);
    return resolve(w, g, id, colour, f);
}

}  // namespace history
