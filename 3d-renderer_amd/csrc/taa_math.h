// taa_math.h — the plain-C++ part of temporal anti-aliasing (include/tri_raster.h "temporal anti-aliasing"): the
// sub-pixel jitter, the argument rules of tri_taa's entry points, and the per-pixel resolve rule as inline functions.
// k_taa_resolve (taa_pass.hip) and host/tools/taa_check.cpp both compile taa::resolve_pixel below: the device runs what
// the sanitizers checked on the CPU. No HIP header is needed; under hipcc the functions are marked for both sides.
// history_math.h is used as it is: history::locate says where a pixel lay one frame ago (mask bits 2 and 4, the four
// taps, fu, fv), history::Sets swaps the two history sets, check_extent and check_context are the object's rules.
//
// The rule, in integers and in float32 with no contraction, in exactly this order (c the pixel's current colour, 4 bytes
// B G R A; i, d its id and depth; R the row of the frame's motion table for i; A' the previous accumulated colour, four
// uint16 per pixel B G R A; I' the previous ids; W x H the frame):
//     w = history::locate(R, x, y, i, d, frame)       mask bits 2 NO_PROJ / 4 OUTSIDE, xi yi, the taps, fu fv
//     NO_HISTORY (1): the object holds no previous frame; the mask is then exactly 1 on every pixel
//     with TRI_TAA_REJECT_ID, only when inside:
//         ID (8) iff none of I'[clamp(yi+dy, 0, H-1)][clamp(xi+dx, 0, W-1)], dx, dy in {-1, 0, 1}, equals i
//     neighbourhood, per channel, as bytes:
//         lo, hi = min, max of c over (clamp(x+dx, 0, W-1), clamp(y+dy, 0, H-1)), dx, dy in {-1, 0, 1}
//     cur16 = (float)(c_ch * 257)     lo16 = (float)(lo * 257)     hi16 = (float)(hi * 257)
//     valid = (mask & 15) == 0
//     valid:   t = c00 * (1.0f - fu) + c10 * fu,  b = c01 * (1.0f - fu) + c11 * fu,  h = t * (1.0f - fv) + b * fv
//              (the taps of A' as float, h not rounded)
//              hc = fminf(fmaxf(h, lo16), hi16)          CLAMPED (32) iff hc != h in any channel
//              r  = hc * (1.0f - alpha) + cur16 * alpha
//              s  = min((int)(r + 0.5f), 65535)
//              out8 = min((int)((float)s * (1.0f / 257.0f) + 0.5f), 255)
//     invalid: s = c_ch * 257         out8 = c_ch        (history restarts from the current frame)
//     stored:  A[p] = s (4 x uint16), I[p] = i, resolved[p] = out8 (B8G8R8A8), mask[p]
// No index is formed from the previous position before `inside` holds, as in history_math.h; the two 3 x 3 windows clamp
// every coordinate to the frame.
#pragma once

#include <cstdint>
#include <cstdio>

#include "history_math.h"

namespace taa {

using history::Msg;

constexpr uint32_t kNoHistory = TRI_TAA_NO_HISTORY, kNoProj = TRI_TAA_NO_PROJ, kOutside = TRI_TAA_OUTSIDE, kId = TRI_TAA_ID,
                   kClamped = TRI_TAA_CLAMPED;
static_assert(kNoProj == history::kNoProj && kOutside == history::kOutside && kNoHistory == history::kNoHistory &&
                  kId == history::kId,
              "the bits history::locate sets are the mask's");
constexpr uint32_t kMaxPeriod = 64;

// ---- the jitter (host only) -------------------------------------------------------------------------------------------
// The radical inverse of k in `base` as one correctly rounded double division of two integers.
inline double radical_inverse(uint32_t k, uint32_t base) {
    uint64_t num = 0, den = 1;
    for (; k; k /= base) {
        num = num * base + k % base;
        den *= base;
    }
    return (double)num / (double)den;
}

// tri_taa_jitter: the Halton (2, 3) point of index % period + 1, centred on the pixel: both components in [-0.5, 0.5).
inline int jitter(uint32_t index, uint32_t period, float* xy, Msg& m) {
    if (!xy) {
        std::snprintf(m.text, sizeof m.text, "null argument");
        return TRI_E_INVALID;
    }
    if (period > kMaxPeriod) {
        std::snprintf(m.text, sizeof m.text, "a period of %u (at most %u)", period, kMaxPeriod);
        return TRI_E_INVALID;
    }
    xy[0] = xy[1] = 0.0f;
    if (period == 0) return TRI_OK;
    const uint32_t k = index % period + 1u;
    xy[0] = (float)(radical_inverse(k, 2) - 0.5);
    xy[1] = (float)(radical_inverse(k, 3) - 0.5);
    return TRI_OK;
}

// tri_taa_jitter_projection: row 0 += (2 jx / W) row 3, row 1 += (2 jy / H) row 3 of a column-major projection — after
// the divide every point's NDC moves by (2 jx / W, 2 jy / H), (jx, jy) pixels; rows 2 and 3 (depth, w) are copied.
inline int jitter_projection(const float* proj, float jx, float jy, uint32_t W, uint32_t H, float* out, Msg& m) {
    if (!proj || !out) {
        std::snprintf(m.text, sizeof m.text, "null argument");
        return TRI_E_INVALID;
    }
    if (W == 0 || H == 0) {
        std::snprintf(m.text, sizeof m.text, "an extent of %u x %u", W, H);
        return TRI_E_INVALID;
    }
    const double dx = 2.0 * (double)jx / (double)W, dy = 2.0 * (double)jy / (double)H;
    float r[16];
    for (int c = 0; c < 4; ++c) {
        r[4 * c + 0] = (float)((double)proj[4 * c + 0] + dx * (double)proj[4 * c + 3]);
        r[4 * c + 1] = (float)((double)proj[4 * c + 1] + dy * (double)proj[4 * c + 3]);
        r[4 * c + 2] = proj[4 * c + 2];
        r[4 * c + 3] = proj[4 * c + 3];
    }
    for (int i = 0; i < 16; ++i) out[i] = r[i];  // (out may be proj)
    return TRI_OK;
}

// ---- the argument rules ---------------------------------------------------------------------------------------------
// tri_taa_resolve's parameters.
inline int check_params(const tri_taa_params* p, Msg& m) {
    if (!p) {
        std::snprintf(m.text, sizeof m.text, "null parameters");
        return TRI_E_INVALID;
    }
    if (!(p->alpha > 0.0f && p->alpha <= 1.0f)) {  // (NaN fails the first test)
        std::snprintf(m.text, sizeof m.text, "an alpha of %g (0 < alpha <= 1)", (double)p->alpha);
        return TRI_E_INVALID;
    }
    const uint32_t known = TRI_TAA_REDO | TRI_TAA_REJECT_ID;
    if (p->flags & ~known) {
        std::snprintf(m.text, sizeof m.text, "unknown flag bits 0x%x", p->flags & ~known);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}

// ---- the per-pixel rule ---------------------------------------------------------------------------------------------
// One pixel of the accumulated history as it lies in memory: four uint16, B G R A (R16G16B16A16_UNORM), in two words.
struct alignas(8) Texel {
    uint32_t bg, ra;
};
TRI_HIST_FN uint32_t channel16(const Texel& t, int k) { return ((k & 2) ? t.ra : t.bg) >> ((k & 1) * 16) & 0xFFFFu; }

struct Pixel {
    Texel acc;          // s
    uint32_t resolved;  // out8, B G R A in memory order
    uint32_t mask;
};

// lo, hi per channel over a 3 x 3 window, packed like a colour.
struct Range {
    uint32_t lo, hi;
};
TRI_HIST_FN void widen(Range& r, uint32_t c) {
    uint32_t lo = 0, hi = 0;
    for (int sh = 0; sh < 32; sh += 8) {
        const uint32_t v = (c >> sh) & 0xFFu, a = (r.lo >> sh) & 0xFFu, b = (r.hi >> sh) & 0xFFu;
        lo |= (v < a ? v : a) << sh;
        hi |= (v > b ? v : b) << sh;
    }
    r.lo = lo;
    r.hi = hi;
}

// The current colour's range round (x, y), every coordinate clamped to the frame.
template <typename ColourPtr>
TRI_HIST_FN Range neighbourhood(ColourPtr colour, uint32_t x, uint32_t y, uint32_t W, uint32_t H) {
    const int xmax = (int)W - 1, ymax = (int)H - 1;
    Range r{0xFFFFFFFFu, 0u};
    for (int dy = -1; dy <= 1; ++dy) {
        const uint32_t row = (uint32_t)history::clampi((int)y + dy, ymax) * W;
        for (int dx = -1; dx <= 1; ++dx) widen(r, colour[row + (uint32_t)history::clampi((int)x + dx, xmax)]);
    }
    return r;
}

// Whether any of the nine previous ids round the nearest previous pixel `at` (= yi * W + xi, inside the frame) is id.
template <typename IdPtr>
TRI_HIST_FN bool id_nearby(IdPtr prev_ids, uint32_t at, uint32_t id, uint32_t W, uint32_t H) {
    const int yi = (int)(at / W), xi = (int)(at - (uint32_t)yi * W);
    const int xmax = (int)W - 1, ymax = (int)H - 1;
    bool found = false;
    for (int dy = -1; dy <= 1; ++dy) {
        const uint32_t row = (uint32_t)history::clampi(yi + dy, ymax) * W;
        for (int dx = -1; dx <= 1; ++dx) found |= prev_ids[row + (uint32_t)history::clampi(xi + dx, xmax)] == id;
    }
    return found;
}

// invalid: the history restarts from the current frame.
TRI_HIST_FN Pixel restart(uint32_t c, uint32_t mask) {
    const uint32_t b = c & 0xFFu, g = (c >> 8) & 0xFFu, r = (c >> 16) & 0xFFu, a = c >> 24;
    return Pixel{Texel{b * 257u | (g * 257u) << 16, r * 257u | (a * 257u) << 16}, c, mask};
}

// valid: the four taps blended, clamped to the neighbourhood, and the current frame mixed in.
TRI_HIST_FN Pixel accumulate(uint32_t c, const Range& n, const Texel* t, float fu, float fv, float alpha) {
    uint32_t s16[4], out = 0, mask = 0;
    for (int k = 0; k < 4; ++k) {
        const int sh = 8 * k;
        const float cur16 = (float)(((c >> sh) & 0xFFu) * 257u);
        const float lo16 = (float)(((n.lo >> sh) & 0xFFu) * 257u), hi16 = (float)(((n.hi >> sh) & 0xFFu) * 257u);
        const float c00 = (float)channel16(t[0], k), c10 = (float)channel16(t[1], k);
        const float c01 = (float)channel16(t[2], k), c11 = (float)channel16(t[3], k);
        const float tp = c00 * (1.0f - fu) + c10 * fu;
        const float bt = c01 * (1.0f - fu) + c11 * fu;
        const float h = tp * (1.0f - fv) + bt * fv;
        const float hc = __builtin_fminf(__builtin_fmaxf(h, lo16), hi16);
        if (hc != h) mask = kClamped;
        const float r = hc * (1.0f - alpha) + cur16 * alpha;
        const int si = (int)(r + 0.5f);
        const uint32_t s = (uint32_t)(si > 65535 ? 65535 : si);
        const int o = (int)((float)s * (1.0f / 257.0f) + 0.5f);
        s16[k] = s;
        out |= (uint32_t)(o > 255 ? 255 : o) << sh;
    }
    return Pixel{Texel{s16[0] | s16[1] << 16, s16[2] | s16[3] << 16}, out, mask};
}

// The rule for pixel (x, y). colour: the current frame's W x H plane (the 3 x 3 window is read from it); prev_ids,
// prev_acc: the previous W x H planes, read only where the pixel is inside (never when has_prev is false). The pointer
// types are the caller's (the kernel passes global-address-space pointers).
template <typename ColourPtr, typename IdPtr, typename AccPtr>
TRI_HIST_FN Pixel resolve_pixel(const float* R, uint32_t x, uint32_t y, uint32_t id, float depth, ColourPtr colour,
                                const history::Frame& f, bool has_prev, bool reject_id, float alpha, IdPtr prev_ids,
                                AccPtr prev_acc) {
    const uint32_t c = colour[y * f.W + x];
    if (!has_prev) return restart(c, kNoHistory);
    // The order of the reads is the kernel's latency: the window needs nothing but (x, y), so it is read ahead of the
    // branches, with the centre; the taps and the nine previous ids are read together once the pixel is inside, before
    // the id test decides — a pixel that ends with the ID bit has had its taps read (every index inside the frame), as
    // in k_reproject. Three dependent round trips instead of six.
    const Range n = neighbourhood(colour, x, y, f.W, f.H);
    const history::Where w = history::locate(R, x, y, id, depth, f);
    if (w.mask) return restart(c, w.mask);
    Texel t[4];
    for (int k = 0; k < 4; ++k) t[k] = prev_acc[w.tap[k]];
    const bool rejected = reject_id && !id_nearby(prev_ids, w.at, id, f.W, f.H);
    if (rejected) return restart(c, kId);
    return accumulate(c, n, t, w.fu, w.fv, alpha);
}

}  // namespace taa
