// frame_select_check — host-only check of the frame selection rules (csrc/frame_select.h: the geometry analysis, the
// draw-list resolution, the bin grid, the queue capacities and the frame-parameter derivation), built under the address
// and undefined-behaviour sanitizers (make frame-select-check). No device: the rules are plain C++. Every expected
// value below is written out from the rule as its comment in frame_select.h and DESIGN.md state it, at the smallest
// sizes that reach each branch.
#include "../../csrc/frame_select.h"

#include <cstdlib>
#include <numeric>
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

tri_vertex vert(float x, float y, float z, float u, float v, float r, float g, float b) {
    tri_vertex t{};
    t.position[0] = x; t.position[1] = y; t.position[2] = z;
    t.normal[2] = 1.0f;
    t.color[0] = r; t.color[1] = g; t.color[2] = b;
    t.texcoord[0] = u; t.texcoord[1] = v;
    return t;
}

// The fixture: 10 vertices with unit normals, texture coordinates within [0, 1] and different colours; mesh 0 is two
// triangles over vertices 0..3, mesh 1 three triangles whose mesh-local indices 1..5 land on vertices 5..9
// (base_vertex 4), its index rows right behind mesh 0's. A case may append further mesh ranges before analyse().
struct Fixture {
    std::vector<tri_vertex> v;
    std::vector<uint32_t> idx{0, 1, 2, 0, 2, 3, 1, 2, 3, 2, 3, 4, 3, 4, 5};
    std::vector<tri_mesh_range> meshes{{0, 6, 0, 0}, {6, 9, 4, 0}};
    fsel::GeomAnalysis a;
    Fixture() {
        for (int i = 0; i < 10; ++i)
            v.push_back(vert((float)i, (float)(i % 3), -(float)(i % 2), 0.1f * (float)i, 1.0f - 0.1f * (float)i, 0.1f * (float)i, 0.5f, 1.0f));
    }
    int analyse(fsel::Msg* why = nullptr) {
        fsel::Msg m;
        return fsel::analyse_geometry(v.data(), v.size(), idx.data(), idx.size(), meshes.data(), (uint32_t)meshes.size(), a,
                                      why ? *why : m);
    }
};

// slot 0: the default 1x1 white texel (and every unused slot's alias); slot 1: a 4 x 4 texture
std::vector<TriTexDesc> slots() {
    std::vector<TriTexDesc> t(TRI_MAX_TEXTURE_SLOTS, TriTexDesc{nullptr, 1, 1, {1.0f, 1.0f, 1.0f, 1.0f}});
    t[1].w = t[1].h = 4;
    return t;
}
std::vector<TriTexDesc> solid_slots() { return std::vector<TriTexDesc>(TRI_MAX_TEXTURE_SLOTS, TriTexDesc{nullptr, 1, 1, {1.0f, 1.0f, 1.0f, 1.0f}}); }

tri_draw draw(uint32_t mesh) {
    tri_draw d{};
    d.mesh_index = mesh;
    for (int i = 0; i < 4; ++i) d.pc.model[5 * i] = 1.0f;
    for (float& t : d.pc.tint) t = 1.0f;
    d.pc.texture_scale[0] = d.pc.texture_scale[1] = 1.0f;
    d.pc.tiling_factor = 1.0f;
    return d;
}

int resolve(const std::vector<tri_draw>& draws, const fsel::GeomInfo& g, fsel::DrawResolution& r,
            const std::vector<TriTexDesc>& tex = solid_slots(), fsel::Msg* why = nullptr) {
    fsel::Msg m;
    return fsel::resolve_draws(draws.data(), (uint32_t)draws.size(), tex.data(), g, r, why ? *why : m);
}

// A 64 x 64 whole-frame context on a 256-CU device whose set-up kernel holds 6 workgroups per CU, identity view and
// projection, default material, no shadow map, sky or AI frame.
struct Ctx {
    tri_global_ubo ubo{};
    tri_material_record mat0{{1, 1, 1, 1}, {1, 1, 1, 0}};
    tri_shadow_config shadow{};
    float pv[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<TriTexDesc> tex = solid_slots();
    fsel::FrameState s{};
    TriFrameParams fp;
    uint32_t path = 0, stat_slots = 0;
    const char* why = nullptr;
    Ctx() {
        for (int i = 0; i < 4; ++i) ubo.view[5 * i] = ubo.projection[5 * i] = 1.0f;
        ubo.directional_light_direction[1] = -1.0f;
        s.W = s.H = 64; s.y0 = 0; s.y1 = 64; s.bin_log2 = 5; s.nbx = s.nby = 2; s.nbins = 4;
        s.cu_count = 256;
        s.setup_wgs_resident = 6;
        s.ovf_rec_cap = 1u << 16; s.ovf_vert_cap = 1u << 17; s.bin_cap = 256;
    }
    int derive(const fsel::DrawResolution& r, const fsel::GeomInfo& g) {
        s.res = &r; s.ucol = g.ucol; s.need_lut = fsel::slots_need_lut(tex.data()); s.ubo = &ubo; s.pv = pv; s.mat0 = &mat0; s.shadow = &shadow;
        why = nullptr;
        return fsel::derive_frame(s, fp, &path, &stat_slots, &why);
    }
    void with_shadow() {
        shadow.size = 64;
        for (int i = 0; i < 4; ++i) shadow.light_view_proj[5 * i] = 1.0f;
        s.s_nbx = 2; s.s_nbins = 4; s.s_bin_cap = 256;
    }
};

void single_draw_cases() {  // 1-6
    Fixture f;
    EXPECT(f.analyse() == TRI_OK);
    EXPECT(f.a.info.obj_ok && !f.a.info.uni_col);
    fsel::DrawResolution r;
    {  // 1: the single-draw solid instantiation with object-space varyings, nothing to carry or fold
        Ctx c;
        EXPECT(resolve({draw(1)}, f.a.info, r) == TRI_OK);
        EXPECT(r.ndraws == 1 && r.nprims == 3 && r.nslots == 5 && r.dd[0].clip_from_world == 1u);
        EXPECT(c.derive(r, f.a.info) == TRI_OK);
        EXPECT(c.fp.one_draw && c.fp.shade_solid && c.fp.vary36 && c.fp.vary_obj && !c.fp.obj_xform && !c.fp.obj_ucol);
        EXPECT(!c.fp.obj48 && !c.fp.idx_route && !c.fp.exact_shading && !c.fp.shadow_on && !c.fp.need_lut);
        EXPECT(c.fp.vin_base == 5u);  // base_vertex 4 + the mesh's lowest index 1
        EXPECT(c.path == (TRI_PATH_ONE_DRAW | TRI_PATH_VARY_OBJ));
    }
    {  // 2: a translated model is carried per pixel
        Ctx c;
        tri_draw d = draw(1);
        d.pc.model[12] = 2.0f;
        EXPECT(resolve({d}, f.a.info, r) == TRI_OK);
        EXPECT(c.derive(r, f.a.info) == TRI_OK);
        EXPECT(c.fp.vary_obj && c.fp.obj_xform && !c.fp.obj_ucol);
        EXPECT(c.path == (TRI_PATH_ONE_DRAW | TRI_PATH_VARY_OBJ | TRI_PATH_OBJ_XFORM));
    }
    {  // 3: one colour on every vertex
        Fixture u;
        for (tri_vertex& t : u.v) { t.color[0] = 0.25f; t.color[1] = 0.5f; t.color[2] = 0.75f; }
        EXPECT(u.analyse() == TRI_OK);
        EXPECT(u.a.info.uni_col);
        Ctx c;
        EXPECT(resolve({draw(1)}, u.a.info, r) == TRI_OK);
        EXPECT(c.derive(r, u.a.info) == TRI_OK);
        EXPECT(c.fp.vary_obj && !c.fp.obj_xform && c.fp.obj_ucol);
        EXPECT(c.fp.ucol[0] == 0.25f && c.fp.ucol[1] == 0.5f && c.fp.ucol[2] == 0.75f);
        EXPECT(c.path == (TRI_PATH_ONE_DRAW | TRI_PATH_VARY_OBJ | TRI_PATH_OBJ_UCOL));
    }
    {  // 4: one normal of squared length 1 + 2e-5 (the bound is 1e-5): world-space varyings
        Fixture n;
        n.v[7].normal[2] = std::sqrt(1.0f + 2e-5f);
        EXPECT(n.analyse() == TRI_OK);
        EXPECT(!n.a.info.obj_ok);
        Ctx c;
        EXPECT(resolve({draw(1)}, n.a.info, r) == TRI_OK);
        EXPECT(c.derive(r, n.a.info) == TRI_OK);
        EXPECT(c.fp.shade_solid && c.fp.vary36 && !c.fp.vary_obj && !c.fp.obj_xform && !c.fp.obj_ucol && c.fp.vin_base == 0u);
        EXPECT(c.path == TRI_PATH_ONE_DRAW);
    }
    {  // 5: the shadow pre-pass leaves the ONE records: obj48 instead
        Ctx c;
        c.with_shadow();
        EXPECT(resolve({draw(1)}, f.a.info, r) == TRI_OK);
        EXPECT(c.derive(r, f.a.info) == TRI_OK);
        EXPECT(c.fp.shade_solid && !c.fp.vary36 && !c.fp.vary_obj && c.fp.obj48 && !c.fp.obj48_xform && c.fp.shadow_on);
        EXPECT(c.fp.vdelta[0] == 5u);
        EXPECT(c.path == (TRI_PATH_ONE_DRAW | TRI_PATH_OBJ48 | TRI_PATH_SHADOW));
    }
    {  // 6: ... but not over a transformed draw
        Ctx c;
        c.with_shadow();
        tri_draw d = draw(1);
        d.pc.model[12] = 2.0f;
        EXPECT(resolve({d}, f.a.info, r) == TRI_OK);
        EXPECT(r.obj48 && r.obj48_xform);
        EXPECT(c.derive(r, f.a.info) == TRI_OK);
        EXPECT(!c.fp.vary36 && !c.fp.obj48 && !c.fp.obj48_xform && c.fp.vdelta[0] == 0u);
        EXPECT(c.path == (TRI_PATH_ONE_DRAW | TRI_PATH_SHADOW));
    }
}

void draw_list_cases() {  // 7-15
    Fixture f;
    f.meshes.push_back({9, 6, 4, 0});  // mesh 2: the last two triangles of mesh 1's rows
    EXPECT(f.analyse() == TRI_OK);
    const fsel::GeomInfo& g = f.a.info;
    fsel::DrawResolution r;
    {  // 7: meshes concatenated in draw order: first_index = 0 + 3 * first primitive for both
        Ctx c;
        EXPECT(resolve({draw(0), draw(1)}, g, r) == TRI_OK);
        EXPECT(r.nprims == 5 && r.nslots == 9 && r.vb[1] == 4 && r.vb[2] == 9 && r.pb[1] == 2 && r.pb[2] == 5);
        EXPECT(r.idx_route && r.idx_k == 0u && r.pbase[0] == 0u && r.pbase[1] == 2u);
        EXPECT(r.vbd[0] == 0u && r.vbd[1] == 3u);        // first slot 4 - the mesh's lowest index 1
        EXPECT(r.obj48 && !r.obj48_xform && r.vdelta[0] == 0u && r.vdelta[1] == 1u);  // 4 + 1 - first slot 4
        EXPECT(c.derive(r, g) == TRI_OK);
        EXPECT(!c.fp.one_draw && !c.fp.shade_solid && !c.fp.vary36 && c.fp.obj48 && c.fp.idx_route);
        EXPECT(c.fp.idx_k == 0u && c.fp.pbase[1] == 2u && c.fp.vbd[1] == 3u && c.fp.vdelta[1] == 1u);
        EXPECT(c.path == (TRI_PATH_OBJ48 | TRI_PATH_IDX_ROUTE));
        // 10: the shadow kernels carry no draw search
        c.with_shadow();
        EXPECT(c.derive(r, g) == TRI_OK);
        EXPECT(!c.fp.idx_route && c.fp.idx_k == 0u && c.fp.pbase[1] == 0u && c.fp.vbd[1] == 0u && c.fp.obj48);
        EXPECT(c.path == (TRI_PATH_OBJ48 | TRI_PATH_SHADOW));
    }
    // 8: K = 6 for mesh 1 first, K = 9 - 3 * 3 = 0 for mesh 2 behind it
    EXPECT(resolve({draw(1), draw(2)}, g, r) == TRI_OK);
    EXPECT(!r.idx_route && r.obj48);
    // 9: the second draw of mesh 0 has K = 0 - 3 * 2 < 0
    EXPECT(resolve({draw(0), draw(0)}, g, r) == TRI_OK);
    EXPECT(!r.idx_route && r.obj48);
    {  // 15: an out-of-range mesh index is an inactive draw between the two: no slots, no primitives, same flags
        Ctx c;
        EXPECT(resolve({draw(0), draw(99), draw(1)}, g, r) == TRI_OK);
        EXPECT(r.ndraws == 3 && r.nprims == 5 && r.nslots == 9 && r.dd[1].vert_count == 0u && r.dd[1].ncl == 0u);
        EXPECT(r.vb[1] == 4 && r.vb[2] == 4 && r.pb[1] == 2 && r.pb[2] == 2);
        EXPECT(r.idx_route && r.idx_k == 0u && r.obj48 && !r.obj48_xform && !r.any_skin);
        EXPECT(c.derive(r, g) == TRI_OK);
        EXPECT(c.path == (TRI_PATH_OBJ48 | TRI_PATH_IDX_ROUTE));
    }
    {  // 13, 14: what takes a draw list off obj48, and a draw off clip_from_world
        tri_draw uv = draw(1), skinned = draw(1), proj = draw(1);
        uv.pc.tiling_factor = 2.0f;
        skinned.pc.bone_count = 1;
        proj.pc.model[3] = 0.5f;
        EXPECT(resolve({draw(0), uv}, g, r) == TRI_OK);
        EXPECT(!r.obj48 && r.dd[1].clip_from_world == 1u && r.idx_route);
        EXPECT(resolve({draw(0), skinned}, g, r) == TRI_OK);
        EXPECT(!r.obj48 && r.any_skin && r.dd[0].clip_from_world == 1u && r.dd[1].clip_from_world == 0u);
        EXPECT(resolve({draw(0), proj}, g, r) == TRI_OK);
        EXPECT(!r.obj48 && !r.any_skin && r.dd[0].clip_from_world == 1u && r.dd[1].clip_from_world == 0u);
    }
    {  // 11, 12: TRI_OBJ48_DRAWS single-triangle meshes in a row, then one more
        Fixture many;
        many.idx.clear();
        many.meshes.clear();
        for (uint32_t m = 0; m <= TRI_OBJ48_DRAWS; ++m) {
            many.idx.insert(many.idx.end(), {0, 1, 2});
            many.meshes.push_back({3 * m, 3, 0, 0});
        }
        EXPECT(many.analyse() == TRI_OK);
        std::vector<tri_draw> d;
        for (uint32_t m = 0; m < TRI_OBJ48_DRAWS; ++m) d.push_back(draw(m));
        Ctx c;
        EXPECT(resolve(d, many.a.info, r) == TRI_OK);
        EXPECT(r.obj48 && r.idx_route && r.idx_k == 0u && r.pbase[TRI_OBJ48_DRAWS - 1] == TRI_OBJ48_DRAWS - 1);
        EXPECT(r.vbd[TRI_OBJ48_DRAWS - 1] == 3u * (TRI_OBJ48_DRAWS - 1));
        EXPECT(c.derive(r, many.a.info) == TRI_OK);
        EXPECT(c.fp.obj48 && c.fp.idx_route);
        d.push_back(draw(TRI_OBJ48_DRAWS));
        EXPECT(resolve(d, many.a.info, r) == TRI_OK);
        EXPECT(r.ndraws == TRI_OBJ48_DRAWS + 1 && !r.obj48 && !r.idx_route);
        EXPECT(c.derive(r, many.a.info) == TRI_OK);
        EXPECT(!c.fp.obj48 && !c.fp.idx_route && c.path == 0u);
    }
}

void uv_reach_cases() {  // 16, 17: |uv| <= 1 over a 4 x 4 texture reaches (1 + offset) * 4 texels
    Fixture f;
    EXPECT(f.analyse() == TRI_OK);
    EXPECT(f.a.info.uv_abs[0] == 0.1f * 9.0f && f.a.info.uv_abs[1] == 1.0f);
    const std::vector<TriTexDesc> tex = slots();
    fsel::DrawResolution r;
    auto exact_at = [&](float offset, const fsel::GeomInfo& g) {
        tri_draw d = draw(1);
        d.pc.texture_slot = 1;
        d.pc.texture_offset[1] = offset;
        EXPECT(resolve({d}, g, r, tex) == TRI_OK);
        Ctx c;
        c.tex = tex;
        EXPECT(c.derive(r, g) == TRI_OK);
        EXPECT(c.fp.need_lut && !c.fp.shade_solid && !c.fp.vary36);
        EXPECT((c.fp.exact_shading != 0) == ((c.path & TRI_PATH_EXACT) != 0));
        return c.fp.exact_shading != 0;
    };
    EXPECT(!exact_at(0.0f, f.a.info) && r.uv_texels == 4.0f);
    EXPECT(!exact_at(2046.99f, f.a.info) && r.uv_texels < fsel::kUvFastTexels && r.uv_texels > 8191.9f);
    EXPECT(!exact_at(2047.0f, f.a.info) && r.uv_texels == fsel::kUvFastTexels);  // "beyond": the bound itself is fast
    EXPECT(exact_at(2047.01f, f.a.info) && r.uv_texels > fsel::kUvFastTexels && r.uv_texels < 8192.1f);
    Fixture nan;
    nan.v[2].texcoord[0] = NAN;  // a vertex no draw of mesh 1 reaches: the bound is per geometry
    EXPECT(nan.analyse() == TRI_OK);
    EXPECT(std::isinf(nan.a.info.uv_abs[0]));
    EXPECT(exact_at(0.0f, nan.a.info) && std::isinf(r.uv_texels));
    {  // the flag alone, and a solid slot ignores the reach
        Ctx c;
        EXPECT(resolve({draw(1)}, nan.a.info, r) == TRI_OK);
        EXPECT(r.uv_texels == 0.0f);
        EXPECT(c.derive(r, nan.a.info) == TRI_OK);
        EXPECT(!c.fp.exact_shading);
        c.s.flags = TRI_FLAG_EXACT_SHADING;
        EXPECT(c.derive(r, nan.a.info) == TRI_OK);
        EXPECT(c.fp.exact_shading && (c.path & TRI_PATH_EXACT));
    }
}

void setup_grid_cases() {  // 18-21: 256 CUs x 3 workgroups x 256 lanes = 196608 primitives at one per lane
    Fixture f;
    EXPECT(f.analyse() == TRI_OK);
    fsel::DrawResolution r;
    EXPECT(resolve({draw(0), draw(1)}, f.a.info, r) == TRI_OK);
    Ctx c;
    auto ppt = [&](uint32_t nprims) {
        r.nprims = nprims;
        EXPECT(c.derive(r, f.a.info) == TRI_OK);
        EXPECT(c.fp.nchunks == (nprims + (uint32_t)c.fp.ppt * 256u - 1) / ((uint32_t)c.fp.ppt * 256u));
        EXPECT(c.stat_slots == c.fp.nchunks && !c.fp.cull_on && !c.fp.setup_multi);
        return c.fp.ppt;
    };
    EXPECT(ppt(5) == 1 && c.fp.nchunks == 1u && c.fp.chunk_stride == 1u);
    EXPECT(ppt(196608) == 1 && c.fp.nchunks == 768u);
    EXPECT(ppt(196609) == 2 && c.fp.nchunks == 385u);
    EXPECT(ppt(2 * 196608 + 1) == 4);       // 3 per lane, rounded up to pairs
    EXPECT(ppt(4 * 196608 + 1) == 6);       // 5
    EXPECT(ppt(40 * 196608) == TRI_MAX_PPT);  // 19: 40 per lane, clamped
    EXPECT(c.fp.nchunks == 40u * 768u / TRI_MAX_PPT);
    c.with_shadow();  // one resident round: 256 x 6 x 256 = 393216 at one per lane
    EXPECT(ppt(393216) == 1 && ppt(393217) == 2);
    {  // 20: rows [0, 32) of 64 with clusters cull: 4096 chunks whatever the device, and never one per lane
        Ctx b;
        b.s.y1 = 32;
        r.nprims = 2 * 4096 * 256 + 1;  // 3 per lane of 4096 chunks (11 per lane of the 768 of a whole frame)
        EXPECT(b.derive(r, f.a.info) == TRI_OK);
        EXPECT(b.fp.cull_on && b.fp.cull_vertex && b.fp.ppt == 4 && b.fp.nchunks == 2049u && b.fp.ncl_total == 2u);
        EXPECT(!b.fp.setup_multi && b.stat_slots == 2049u);  // two draws
        r.nprims = 5;
        EXPECT(b.derive(r, f.a.info) == TRI_OK);
        EXPECT(b.fp.ppt == 2 && b.fp.nchunks == 1u);
        Ctx w;  // the same count on the whole frame
        r.nprims = 2 * 4096 * 256 + 1;
        EXPECT(w.derive(r, f.a.info) == TRI_OK);
        EXPECT(!w.fp.cull_on && w.fp.ppt == 12);
        w.s.flags = TRI_FLAG_CLUSTER_CULL;  // ... which culls on request
        EXPECT(w.derive(r, f.a.info) == TRI_OK);
        EXPECT(w.fp.cull_on && w.fp.ppt == 4);
        r.ncl_total = 0;  // no clusters, nothing to cull by
        EXPECT(b.derive(r, f.a.info) == TRI_OK);
        EXPECT(!b.fp.cull_on && b.fp.ppt == 12);
    }
    {  // 21: a single-draw band without the pre-pass runs a quarter of the workgroups, four chunks each
        Ctx b;
        b.s.y1 = 32;
        EXPECT(resolve({draw(1)}, f.a.info, r) == TRI_OK);
        r.nprims = 2 * 4096 * 256 + 1;
        EXPECT(b.derive(r, f.a.info) == TRI_OK);
        EXPECT(b.fp.setup_multi && b.fp.nchunks == 2049u && b.stat_slots == 513u);
        b.with_shadow();
        EXPECT(b.derive(r, f.a.info) == TRI_OK);
        EXPECT(b.fp.cull_on && !b.fp.cull_vertex && !b.fp.setup_multi && b.stat_slots == 2049u);
    }
}

void ai_blend_cases() {  // 22, 23
    Fixture f;
    EXPECT(f.analyse() == TRI_OK);
    fsel::DrawResolution r;
    EXPECT(resolve({draw(1)}, f.a.info, r) == TRI_OK);
    Ctx c;
    c.ubo.ai_blend_config[0] = 2.0f;  // clamped to 1
    c.ubo.ai_blend_config[1] = 0.5f;
    c.ubo.ai_blend_config[2] = 0.25f;
    EXPECT(c.derive(r, f.a.info) == TRI_OK);  // AiBlendConfig.w == 0: off
    EXPECT(!c.fp.ai_on && c.fp.vary36);
    c.ubo.ai_blend_config[3] = 1.0f;
    EXPECT(c.derive(r, f.a.info) == TRI_E_STATE);
    EXPECT(c.why && std::string(c.why) == "tri_render: AiBlendConfig.w > 0 but no AI frame uploaded (tri_upload_ai_frame)");
    c.s.ai_w = 8;
    c.s.ai_h = 4;
    EXPECT(c.derive(r, f.a.info) == TRI_OK);
    EXPECT(c.fp.ai_on && c.fp.ai_wgt == 1.0f && c.fp.ai_sx == 0.5f && c.fp.ai_sy == 0.25f && c.fp.ai_tw == 8u && c.fp.ai_th == 4u);
    EXPECT(c.fp.shade_solid && !c.fp.vary36 && !c.fp.vary_obj && c.fp.obj48);  // never the ONE 36-B records
    c.with_shadow();
    EXPECT(c.derive(r, f.a.info) == TRI_E_UNSUPPORTED);
    EXPECT(c.why && std::string(c.why) ==
                        "tri_render: the AI frame blend with the shadow pre-pass (the reference has no shadow pass)");
    c.ubo.ai_blend_config[0] = 0.0f;  // a zero weight is no blend
    EXPECT(c.derive(r, f.a.info) == TRI_OK);
    EXPECT(!c.fp.ai_on);
}

void chunk_stride_case() {  // 24
    int bad = 0;
    for (uint32_t n = 1; n <= 4096; ++n) {
        const uint32_t s = fsel::chunk_stride(n);
        if (n <= 2 ? s != 1u : !(s >= 1u && s < n && std::gcd(s, n) == 1u)) ++bad;
    }
    EXPECT(bad == 0);
    EXPECT(fsel::chunk_stride(768) == 475u);  // 768 x 0.618... = 474.6 -> 474 | 1 = 475 = 5^2 x 19, coprime to 2^8 x 3
}

void bin_grid_cases() {  // 25: the cases of test_grid_selection_by_frame_size and _by_density
    if (TRI_FORCE_BIN_LOG2) return;
    EXPECT(fsel::choose_bin_log2(2048, 2016, 0, 2016, 0) == 4);     // 64 x 63 = 4032 bins of 32 px: small and sparse
    EXPECT(fsel::choose_bin_log2(2048, 2048, 0, 2048, 0) == 5);     // 4096: not small
    EXPECT(fsel::choose_bin_log2(4096, 4096, 0, 4096, 0) == 5);     // 16384 keep 32 px
    EXPECT(fsel::choose_bin_log2(4097, 4096, 0, 4096, 0) == 6);     // 129 x 128
    EXPECT(fsel::choose_bin_log2(4100, 4100, 0, 2050, 0) == 5);     // a band counts its own rows: 129 x 65
    EXPECT(fsel::choose_bin_log2(320, 240, 0, 240, 3840) == 5);     // exactly 0.05 triangles per pixel
    EXPECT(fsel::choose_bin_log2(320, 240, 0, 240, 3839) == 4);
    // queue capacities: 8 x the mean of 1.3 entries per triangle, in 64s, at least 256, never shrinking
    EXPECT(fsel::bin_queue_cap(0, 0, 4) == 256u);
    EXPECT(fsel::bin_queue_cap(0, 1000000, 100) == 104064u);  // mean 13000: (8 x 13000 + 127) / 64 = 1626 x 64
    EXPECT(fsel::bin_queue_cap(200000, 1000000, 100) == 200000u);
    EXPECT(fsel::bin_queue_cap(0, 100, 0) == 1152u);  // no bins count as one: mean 130, (8 x 130 + 127) / 64 = 18 x 64
    EXPECT(fsel::bin_queue_cap(0, TRI_PRIM_MAX, 1) == (1u << 30));  // 8 x 697932184 is beyond the ceiling
}

void geometry_case() {  // 26
    Fixture f;
    f.meshes.push_back({12, 6, 0, 0});  // rows 12..17 of 15: past the end
    EXPECT(f.analyse() == TRI_OK);
    const fsel::GeomInfo& g = f.a.info;
    EXPECT(g.nverts == 10 && g.nidx == 15 && g.meshes.size() == 3);
    EXPECT(g.mesh_min[0] == 0u && g.mesh_max[0] == 3u && g.mesh_min[1] == 1u && g.mesh_max[1] == 5u);
    EXPECT(g.mesh_min[2] == 0u && g.mesh_max[2] == 0u && g.mesh_ncl[2] == 0u);
    EXPECT(f.a.clusters.size() == 2 && g.mesh_cl_first[0] == 0u && g.mesh_cl_first[1] == 1u && g.mesh_ncl[0] == 1u && g.mesh_ncl[1] == 1u);
    EXPECT(f.a.vblk.size() == 2 && g.mesh_vblk_first[0] == 0u && g.mesh_vblk_first[1] == 1u);
    EXPECT(f.a.vblk[0].x == 0u && f.a.vblk[0].y == 0u && f.a.vblk[1].x == 0u && f.a.vblk[1].y == 0u);
    // mesh 1 references vertices 5..9: x 5..9, y = i % 3 in 0..2, z = -(i % 2) in -1..0
    const TriCluster& c1 = f.a.clusters[1];
    EXPECT(c1.vmin == 1u && c1.vmax == 5u && c1.lo[0] == 5.0f && c1.hi[0] == 9.0f && c1.lo[1] == 0.0f && c1.hi[1] == 2.0f &&
           c1.lo[2] == -1.0f && c1.hi[2] == 0.0f);
    EXPECT(f.a.vbox.size() == 2 && f.a.vbox[1].lo[0] == 5.0f && f.a.vbox[1].hi[0] == 9.0f && f.a.vbox[0].lo[0] == 0.0f &&
           f.a.vbox[0].hi[0] == 3.0f);
    EXPECT(f.a.vin.size() == 10 && f.a.vin[9].px == 9.0f && f.a.vin[9].nz == 1.0f && f.a.vin[9].u == 0.1f * 9.0f && f.a.vin[9].cg == 0.5f);
    EXPECT(f.a.pos.size() == 30 && f.a.attr.size() == 90 && f.a.pos[27] == 9.0f && f.a.attr[81] == 9.0f && f.a.attr[89] == 1.0f);
    EXPECT(!f.a.has_skin && f.a.skin.empty());
    fsel::DrawResolution r;  // a draw of the skipped mesh is inactive
    EXPECT(resolve({draw(2)}, g, r) == TRI_OK);
    EXPECT(r.nprims == 0 && r.nslots == 0 && !r.draw0_obj);
    {  // a mesh spanning more than one 256-slot vertex block and more than one 512-triangle cluster
        Fixture big;
        big.v.clear();
        for (int i = 0; i < 600; ++i) big.v.push_back(vert((float)i, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f));
        big.idx.clear();
        for (uint32_t t = 0; t < 598; ++t) big.idx.insert(big.idx.end(), {t, t + 1, t + 2});
        big.meshes = {{0, 3 * 598, 0, 0}};
        EXPECT(big.analyse() == TRI_OK);
        EXPECT(big.a.clusters.size() == 2 && big.a.vblk.size() == 3);  // triangles 0..511 | 512..597; slots 0..255 | ..511 | ..599
        EXPECT(big.a.clusters[0].vmin == 0u && big.a.clusters[0].vmax == 513u && big.a.clusters[1].vmin == 512u && big.a.clusters[1].vmax == 599u);
        EXPECT(big.a.vblk[0].x == 0u && big.a.vblk[0].y == 0u && big.a.vblk[1].x == 0u && big.a.vblk[1].y == 0u);
        EXPECT(big.a.vblk[2].x == 0u && big.a.vblk[2].y == 1u);
        EXPECT(big.a.vbox[1].lo[0] == 0.0f && big.a.vbox[1].hi[0] == 513.0f && big.a.vbox[2].hi[0] == 599.0f);
    }
    {  // the index range error
        Fixture wide;
        wide.idx[7] = 0x80000000u;
        fsel::Msg why;
        EXPECT(wide.analyse(&why) == TRI_E_INVALID);
        EXPECT(std::string(why.text) == "mesh 1: index range too large");
    }
    {  // a weight anywhere brings the skin records
        Fixture sk;
        sk.v[3].bone_weights[1] = 0.5f;
        sk.v[3].bone_indices[1] = 7;
        EXPECT(sk.analyse() == TRI_OK);
        EXPECT(sk.a.has_skin && sk.a.skin.size() == 10 && sk.a.skin[3].idx[1] == 7 && sk.a.skin[3].w[1] == 0.5f && sk.a.skin[4].w[1] == 0.0f);
    }
}

void limit_case() {  // the two size limits of a draw list, through their messages
    fsel::GeomInfo g;  // one mesh claiming 2^32 - 1 indices (tables only: nothing reads an index here)
    g.nidx = 1ull << 32;
    g.nverts = 3;
    g.meshes = {{0, 0xFFFFFFFFu, 0, 0}};
    g.mesh_min = {0};
    g.mesh_max = {2};
    g.mesh_cl_first = g.mesh_ncl = g.mesh_vblk_first = {0};
    fsel::DrawResolution r;
    fsel::Msg why;
    EXPECT(resolve({draw(0)}, g, r, solid_slots(), &why) == TRI_E_INVALID);
    EXPECT(std::string(why.text) == "too many primitives (1431655765 > 536870911)");
    g.meshes = {{0, 3, 0, 0}};
    g.mesh_max = {0xFFFFFFF0u};
    EXPECT(resolve({draw(0)}, g, r, solid_slots(), &why) == TRI_E_INVALID);
    EXPECT(std::string(why.text) == "too many vertex-shader invocations (4294967281)");
}

}  // namespace

int main() {
    single_draw_cases();
    draw_list_cases();
    uv_reach_cases();
    setup_grid_cases();
    ai_blend_cases();
    chunk_stride_case();
    bin_grid_cases();
    geometry_case();
    limit_case();
    if (g_failures) {
        std::fprintf(stderr, "frame_select_check: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("frame_select_check: ok\n");
    return 0;
}
