// id_select.h — the plain-C++ rules of the entity-id pass (include/tri_raster.h "entity ids"): the argument checks of
// its entry points, the primitive -> draw lookup the id kernel takes from the raster (restated over the host tables),
// and the outline rule as a host function. No HIP: host/tools/id_check.cpp runs all of it under the sanitizers, and the
// C-ABI (tri_ids.hip) calls the same checks.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/tri_raster.h"

namespace idsel {

constexpr uint32_t kMaxOutlineWidth = 8;  // k_id_outline's halo (id_pass.hip)

struct Msg {
    char text[160] = {0};
};

// The id of a pixel won by a primitive of resolved draw d. fsel::resolve_draws keeps one record per caller draw — a
// skipped draw (bad mesh index, an empty or out-of-range index run) stays in the tables with no slots and no
// primitives — so the resolved index IS the caller's index and no translation table travels to the device.
inline uint32_t id_of_draw(uint32_t d) { return d + 1u; }

// The draw of primitive p from the ndraws + 1 primitive bases: the last draw whose base is <= p. This is what both
// device routes compute (prim_slots' scalar search over TriFrameParams::pbase, k_setup's find_range for prim_vs);
// draws without primitives (pb[d + 1] == pb[d]) are passed over by construction.
inline uint32_t draw_of_prim(const uint32_t* pb, uint32_t ndraws, uint32_t p) {
    uint32_t d = 0;
    while (d + 1 < ndraws && p >= pb[d + 1]) ++d;
    return d;
}

// Words of a per-draw bitmap.
inline uint32_t bitmap_words(uint32_t ndraws) { return (ndraws + 31u) / 32u; }

// tri_pick: (x, y) in full-frame coordinates inside a context that renders rows [y0, y1) of a frame W wide.
inline int check_pick(int32_t W, int32_t y0, int32_t y1, int32_t x, int32_t y, Msg& m) {
    if (x < 0 || x >= W || y < y0 || y >= y1) {
        std::snprintf(m.text, sizeof m.text, "pixel (%d, %d) outside columns [0, %d) x rows [%d, %d)", x, y, W, y0, y1);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}

// tri_pick_rect: the inclusive rectangle clamped to the context's pixels; *empty when nothing is left of it.
struct Rect {
    int32_t x0, y0, x1, y1;
};
inline int check_rect(int32_t W, int32_t y0, int32_t y1, Rect& r, uint32_t ndraws, uint32_t word_count, bool have_bits,
                      bool* empty, Msg& m) {
    if (r.x1 < r.x0 || r.y1 < r.y0) {
        std::snprintf(m.text, sizeof m.text, "rectangle (%d, %d)-(%d, %d) has its corners reversed", r.x0, r.y0, r.x1, r.y1);
        return TRI_E_INVALID;
    }
    const uint32_t need = bitmap_words(ndraws);
    if (word_count < need || (need && !have_bits)) {
        std::snprintf(m.text, sizeof m.text, "%u draws need %u bitmap words, %u given", ndraws, need, have_bits ? word_count : 0u);
        return TRI_E_INVALID;
    }
    r.x0 = r.x0 < 0 ? 0 : r.x0;
    r.y0 = r.y0 < y0 ? y0 : r.y0;
    r.x1 = r.x1 > W - 1 ? W - 1 : r.x1;
    r.y1 = r.y1 > y1 - 1 ? y1 - 1 : r.y1;
    *empty = r.x1 < r.x0 || r.y1 < r.y0;
    return TRI_OK;
}

// tri_set_outline's descriptor against the context's current draw count.
inline int check_outline(const tri_outline& o, uint32_t ndraws, Msg& m) {
    if (o.width_px < 1 || o.width_px > kMaxOutlineWidth) {
        std::snprintf(m.text, sizeof m.text, "outline width %u outside 1..%u", o.width_px, kMaxOutlineWidth);
        return TRI_E_INVALID;
    }
    if (o.draw_count && !o.draws) {
        std::snprintf(m.text, sizeof m.text, "null draw list with %u entries", o.draw_count);
        return TRI_E_INVALID;
    }
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(o.rgba[k])) {
            std::snprintf(m.text, sizeof m.text, "non-finite outline colour");
            return TRI_E_INVALID;
        }
    for (uint32_t i = 0; i < o.draw_count; ++i)
        if (o.draws[i] >= ndraws) {
            std::snprintf(m.text, sizeof m.text, "outline draw %u of a list of %u", o.draws[i], ndraws);
            return TRI_E_INVALID;
        }
    return TRI_OK;
}

// The per-draw selection flags k_id_outline reads: ndraws words (at least one), 1 for a selected draw. Indices beyond
// ndraws (a draw list that shrank after tri_set_outline) select nothing.
inline void selection_flags(const uint32_t* draws, uint32_t count, uint32_t ndraws, std::vector<uint32_t>& flags) {
    flags.assign(ndraws ? ndraws : 1u, 0u);
    for (uint32_t i = 0; i < count; ++i)
        if (draws[i] < ndraws) flags[draws[i]] = 1u;
}

// The outline rule over `rows` rows of W ids: S(p) = id(p) >= 1 and draw id(p) - 1 selected; p is an outline pixel
// iff S(p) == 0 and some q inside the rows with max(|dx|, |dy|) <= r has S(q) == 1.
inline void outline_mask(const uint32_t* ids, int32_t W, int32_t rows, const uint32_t* flags, uint32_t ndraws, int32_t r,
                         std::vector<uint8_t>& mask) {
    const auto S = [&](int32_t x, int32_t y) {
        const uint32_t id = ids[(size_t)y * W + x];
        return id >= 1u && id - 1u < ndraws && flags[id - 1u] != 0u;
    };
    mask.assign((size_t)W * rows, 0);
    for (int32_t y = 0; y < rows; ++y)
        for (int32_t x = 0; x < W; ++x) {
            if (S(x, y)) continue;
            bool near = false;
            for (int32_t qy = y - r < 0 ? 0 : y - r; qy <= y + r && qy < rows && !near; ++qy)
                for (int32_t qx = x - r < 0 ? 0 : x - r; qx <= x + r && qx < W && !near; ++qx) near = S(qx, qy);
            mask[(size_t)y * W + x] = near ? 1 : 0;
        }
}

}  // namespace idsel
