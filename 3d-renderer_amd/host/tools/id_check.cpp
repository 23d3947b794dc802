// id_check — host-only check of the entity-id pass's plain-C++ rules (csrc/id_select.h over csrc/frame_select.h's draw
// resolution), built under the address and undefined-behaviour sanitizers (make id-check). No device. Three groups:
//   1. draw lists with skipped draws: the resolved tables keep one record per caller draw, so the primitive -> draw
//      lookup of both device routes (the primitive bases of the index route; k_setup's search for prim_vs) yields the
//      caller's index, and the id is that index + 1;
//   2. the outline rule over small id arrays, written out by hand, and the selection flags;
//   3. the argument checks of tri_pick, tri_pick_rect and tri_set_outline.
#include "../../csrc/frame_select.h"
#include "../../csrc/id_select.h"

#include <cstdlib>
#include <string>

namespace {

int g_failures = 0;

#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++g_failures;                                                         \
        }                                                                         \
    } while (0)

tri_draw draw(uint32_t mesh) {
    tri_draw d{};
    d.mesh_index = mesh;
    for (int i = 0; i < 4; ++i) d.pc.model[5 * i] = 1.0f;
    for (float& t : d.pc.tint) t = 1.0f;
    d.pc.texture_scale[0] = d.pc.texture_scale[1] = 1.0f;
    d.pc.tiling_factor = 1.0f;
    return d;
}

// 10 vertices; mesh 0: two triangles, mesh 1: three (base_vertex 4), mesh 2: an index run past the buffer, mesh 3: empty
struct Fixture {
    std::vector<tri_vertex> v;
    std::vector<uint32_t> idx{0, 1, 2, 0, 2, 3, 1, 2, 3, 2, 3, 4, 3, 4, 5};
    std::vector<tri_mesh_range> meshes{{0, 6, 0, 0}, {6, 9, 4, 0}, {12, 9, 0, 0}, {0, 0, 0, 0}};
    fsel::GeomAnalysis a;
    Fixture() {
        for (int i = 0; i < 10; ++i) {
            tri_vertex t{};
            t.position[0] = (float)i; t.position[1] = (float)(i % 3); t.position[2] = -(float)(i % 2);
            t.normal[2] = 1.0f;
            t.color[0] = 0.1f * (float)i; t.color[1] = 0.5f; t.color[2] = 1.0f;
            v.push_back(t);
        }
    }
};

void skipped_draws() {
    Fixture f;
    fsel::Msg m;
    EXPECT(fsel::analyse_geometry(f.v.data(), f.v.size(), f.idx.data(), f.idx.size(), f.meshes.data(),
                                  (uint32_t)f.meshes.size(), f.a, m) == TRI_OK);
    const std::vector<TriTexDesc> tex(TRI_MAX_TEXTURE_SLOTS, TriTexDesc{nullptr, 1, 1, {1.0f, 1.0f, 1.0f, 1.0f}});
    // caller's list: valid, bad mesh index, valid, an index run past the buffer, an empty mesh, valid, bad (trailing)
    const std::vector<tri_draw> draws{draw(0), draw(99), draw(1), draw(2), draw(3), draw(0), draw(7)};
    const uint32_t prims[7] = {2, 0, 3, 0, 0, 2, 0};
    fsel::DrawResolution r;
    EXPECT(fsel::resolve_draws(draws.data(), (uint32_t)draws.size(), tex.data(), f.a.info, r, m) == TRI_OK);
    EXPECT(r.ndraws == draws.size());  // one record per caller draw: resolved index == caller index
    EXPECT(r.nprims == 7u);
    uint32_t p = 0;
    for (uint32_t d = 0; d < r.ndraws; ++d) {
        EXPECT(r.pb[d + 1] - r.pb[d] == prims[d]);
        for (uint32_t k = 0; k < prims[d]; ++k, ++p) {
            EXPECT(idsel::draw_of_prim(r.pb.data(), r.ndraws, p) == d);  // the index route's scalar search
            // k_setup's binary search over the same bases (the draw it writes into prim_vs)
            int lo = 0, hi = (int)r.ndraws - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (r.pb[mid] <= p) lo = mid; else hi = mid - 1;
            }
            // (empty draws in front of d share its base and sort before it; those behind it start past p)
            EXPECT(lo == (int)d);
            EXPECT(idsel::id_of_draw(d) == d + 1u);
        }
    }
    EXPECT(p == r.nprims);
    if (r.idx_route)  // the frame's own copy of the bases
        for (uint32_t d = 0; d < r.ndraws; ++d) EXPECT(r.pbase[d] == r.pb[d]);
    // a list that is all skips
    const std::vector<tri_draw> none{draw(99), draw(3)};
    EXPECT(fsel::resolve_draws(none.data(), 2, tex.data(), f.a.info, r, m) == TRI_OK);
    EXPECT(r.ndraws == 2 && r.nprims == 0);
    // one valid draw behind a skip: not a single-draw frame, its id stays 2
    const std::vector<tri_draw> two{draw(99), draw(1)};
    EXPECT(fsel::resolve_draws(two.data(), 2, tex.data(), f.a.info, r, m) == TRI_OK);
    EXPECT(r.ndraws == 2 && r.nprims == 3);
    for (uint32_t q = 0; q < 3; ++q) EXPECT(idsel::id_of_draw(idsel::draw_of_prim(r.pb.data(), 2, q)) == 2u);
}

void outline_rule() {
    // 7 x 5 ids; draw 0 (id 1) is a single pixel at (3, 2), draw 1 (id 2) fills the first column
    const int32_t W = 7, H = 5;
    std::vector<uint32_t> ids((size_t)W * H, 0u);
    ids[2 * W + 3] = 1u;
    for (int y = 0; y < H; ++y) ids[(size_t)y * W] = 2u;
    std::vector<uint32_t> flags;
    std::vector<uint8_t> mask;
    const uint32_t sel0[] = {0};
    idsel::selection_flags(sel0, 1, 2, flags);
    EXPECT(flags.size() == 2 && flags[0] == 1u && flags[1] == 0u);
    idsel::outline_mask(ids.data(), W, H, flags.data(), 2, 1, mask);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const bool ring = std::abs(x - 3) <= 1 && std::abs(y - 2) <= 1 && !(x == 3 && y == 2);
            EXPECT(mask[(size_t)y * W + x] == (ring ? 1 : 0));
        }
    idsel::outline_mask(ids.data(), W, H, flags.data(), 2, 2, mask);  // reaches rows 0 and 4, clipped at neither side
    int n = 0;
    for (uint8_t b : mask) n += b;
    EXPECT(n == 5 * 5 - 1);
    EXPECT(mask[2 * W + 0] == 0 && mask[0 * W + 1] == 1);  // column 0 is out of reach (dx = 3); draw 1's pixels count
                                                            // as unselected pixels in reach when they are
    idsel::outline_mask(ids.data(), W, H, flags.data(), 2, 8, mask);  // wider than the array: everything but the pixel
    n = 0;
    for (uint8_t b : mask) n += b;
    EXPECT(n == W * H - 1 && mask[2 * W + 3] == 0);
    // the first column selected: an outline along column 1 only, cut at the array's edges
    const uint32_t sel1[] = {1, 1};
    idsel::selection_flags(sel1, 2, 2, flags);
    EXPECT(flags[0] == 0u && flags[1] == 1u);
    idsel::outline_mask(ids.data(), W, H, flags.data(), 2, 1, mask);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) EXPECT(mask[(size_t)y * W + x] == (x == 1 ? 1 : 0));
    // nothing selected; indices past the draw count select nothing; ids past the draw count are ignored
    const uint32_t sel9[] = {9};
    idsel::selection_flags(sel9, 1, 2, flags);
    idsel::outline_mask(ids.data(), W, H, flags.data(), 2, 3, mask);
    for (uint8_t b : mask) EXPECT(b == 0);
    idsel::selection_flags(nullptr, 0, 0, flags);
    EXPECT(flags.size() == 1 && flags[0] == 0u);
    ids[0] = 77u;
    idsel::outline_mask(ids.data(), W, H, flags.data(), 0, 1, mask);
    for (uint8_t b : mask) EXPECT(b == 0);
}

void argument_checks() {
    idsel::Msg m;
    // a band of rows [10, 30) of a frame 64 wide
    EXPECT(idsel::check_pick(64, 10, 30, 0, 10, m) == TRI_OK);
    EXPECT(idsel::check_pick(64, 10, 30, 63, 29, m) == TRI_OK);
    EXPECT(idsel::check_pick(64, 10, 30, 64, 10, m) == TRI_E_INVALID);
    EXPECT(idsel::check_pick(64, 10, 30, -1, 10, m) == TRI_E_INVALID);
    EXPECT(idsel::check_pick(64, 10, 30, 0, 9, m) == TRI_E_INVALID);
    EXPECT(idsel::check_pick(64, 10, 30, 0, 30, m) == TRI_E_INVALID && std::string(m.text).find("rows [10, 30)") != std::string::npos);
    EXPECT(idsel::bitmap_words(0) == 0 && idsel::bitmap_words(1) == 1 && idsel::bitmap_words(32) == 1 && idsel::bitmap_words(33) == 2);
    bool empty = true;
    idsel::Rect r{-5, 0, 100, 100};
    EXPECT(idsel::check_rect(64, 10, 30, r, 33, 2, true, &empty, m) == TRI_OK && !empty);
    EXPECT(r.x0 == 0 && r.y0 == 10 && r.x1 == 63 && r.y1 == 29);
    r = idsel::Rect{5, 12, 5, 12};
    EXPECT(idsel::check_rect(64, 10, 30, r, 33, 2, true, &empty, m) == TRI_OK && !empty && r.x0 == 5 && r.y1 == 12);
    r = idsel::Rect{0, 0, 63, 9};  // above the band
    EXPECT(idsel::check_rect(64, 10, 30, r, 33, 2, true, &empty, m) == TRI_OK && empty);
    r = idsel::Rect{0, 0, 63, 63};
    EXPECT(idsel::check_rect(64, 10, 30, r, 33, 1, true, &empty, m) == TRI_E_INVALID);   // a word short
    EXPECT(idsel::check_rect(64, 10, 30, r, 33, 2, false, &empty, m) == TRI_E_INVALID);  // no bitmap
    EXPECT(idsel::check_rect(64, 10, 30, r, 0, 0, false, &empty, m) == TRI_OK);          // no draws: nothing to return
    r = idsel::Rect{9, 0, 8, 63};
    EXPECT(idsel::check_rect(64, 10, 30, r, 1, 1, true, &empty, m) == TRI_E_INVALID);    // reversed
    const uint32_t d[] = {0, 2};
    tri_outline o{d, 2, {1.0f, 0.6f, 0.0f, 1.0f}, 2, 0};
    EXPECT(idsel::check_outline(o, 3, m) == TRI_OK);
    EXPECT(idsel::check_outline(o, 2, m) == TRI_E_INVALID);  // draw 2 of a list of 2
    o.width_px = 0;
    EXPECT(idsel::check_outline(o, 3, m) == TRI_E_INVALID);
    o.width_px = 9;
    EXPECT(idsel::check_outline(o, 3, m) == TRI_E_INVALID);
    o.width_px = 8;
    EXPECT(idsel::check_outline(o, 3, m) == TRI_OK);
    o.rgba[3] = NAN;
    EXPECT(idsel::check_outline(o, 3, m) == TRI_E_INVALID);
    o.rgba[3] = 0.5f;
    o.draws = nullptr;
    EXPECT(idsel::check_outline(o, 3, m) == TRI_E_INVALID);
    o.draw_count = 0;
    EXPECT(idsel::check_outline(o, 0, m) == TRI_OK);  // an empty selection is valid on any draw list
}

}  // namespace

int main() {
    skipped_draws();
    outline_rule();
    argument_checks();
    if (g_failures) {
        std::fprintf(stderr, "id_check: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("id_check ok\n");
    return 0;
}
