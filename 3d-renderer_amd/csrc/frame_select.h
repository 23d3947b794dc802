// frame_select.h — every host-side decision about which kernels a frame runs and with what constants, as pure
// functions over plain structs: the geometry analysis of an upload, the draw-list resolution, the bin grid and its
// queue capacities, and the derivation of a frame's TriFrameParams. Plain C++17, no HIP: the C-ABI units include it
// (tri_raster_capi.hip, tri_geometry.hip, tri_resources.hip), and so does the stand-alone check
// (host/tools/frame_select_check.cpp), which is how a rule here is tested without a device.
//
// A function that can refuse returns a TRI_E_* code and leaves the text for tri_last_error in its Msg.
#pragma once

#include "raster_common.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

// k_setup workgroups per CU for frames without the shadow pre-pass. With frames in flight, one frame's set-up runs
// beside another frame's k_raster, and every resident set-up workgroup holds wave slots and LDS that the raster's
// bins cannot use while it waits on its fetch -> atomic -> store chain. Fewer, longer workgroups (more primitives
// per lane) make the set-up slower alone (C3 27.9 -> 37 us) but the frame rate higher (C3 10.39-10.43k -> 10.55k,
// C3 under a TRS draw +1 %, C2 unchanged: its set-up is one primitive per lane either way). The shadow set-up bins
// every primitive twice and keeps the resident round (C5 4.90k -> 4.75k with 2). Round 6: with the single-draw set-up
// within 64 VGPRs and the raster's C3 instantiation within 56 (raster_kernels.hip: TRI_SETUP_WAVES_ONE,
// raster_plain.hip: TRI_RASTER_ONE_VGPRS) a set-up wave displaces at most one raster wave, and 3 per CU beat 2 (same-box A/B).
#ifndef TRI_SETUP_WGS_PER_CU_OVERLAP
#define TRI_SETUP_WGS_PER_CU_OVERLAP 3
#endif
// k_setup's chunk target for bands (cluster culling): most chunks are culled and exit at once
#ifndef TRI_SETUP_BAND_CHUNKS
#define TRI_SETUP_BAND_CHUNKS 4096
#endif
// -DTRI_FORCE_BIN_LOG2=4..6 forces a bin size (diagnostics builds only, tools/build_variant.sh).
#ifndef TRI_FORCE_BIN_LOG2
#define TRI_FORCE_BIN_LOG2 0
#endif

namespace fsel {

struct Msg {
    char text[192];
};

inline uint32_t unorm8_host(float c) {
    const float cc = std::fmin(std::fmax(c, 0.0f), 1.0f);
    return (uint32_t)(int)(cc * 255.0f + 0.5f);
}

// R8G8B8A8_SRGB decode of one channel byte (sRGB EOTF in double, rounded): the kernels' LUT.
inline float srgb_decode(int i) {
    const double v = i / 255.0;
    return (float)(v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4));
}

inline float clamp01(float x) { return std::fmin(std::fmax(x, 0.0f), 1.0f); }

// transpose(inverse(mat3(M))) exactly as Default.vert:95 evaluates it per vertex (glm cofactor
// form, same float operation order as the oracle); out[c*3+r] = NM[c][r] = inverse[r][c].
inline void normal_matrix(const float* M, float* out) {
    auto m = [M](int c, int r) { return M[c * 4 + r]; };
    const float det = (m(0, 0) * (m(1, 1) * m(2, 2) - m(2, 1) * m(1, 2)) -
                       m(1, 0) * (m(0, 1) * m(2, 2) - m(2, 1) * m(0, 2))) +
                      m(2, 0) * (m(0, 1) * m(1, 2) - m(1, 1) * m(0, 2));
    const float od = 1.0f / det;
    float inv[3][3];
    inv[0][0] = +(m(1, 1) * m(2, 2) - m(2, 1) * m(1, 2)) * od;
    inv[1][0] = -(m(1, 0) * m(2, 2) - m(2, 0) * m(1, 2)) * od;
    inv[2][0] = +(m(1, 0) * m(2, 1) - m(2, 0) * m(1, 1)) * od;
    inv[0][1] = -(m(0, 1) * m(2, 2) - m(2, 1) * m(0, 2)) * od;
    inv[1][1] = +(m(0, 0) * m(2, 2) - m(2, 0) * m(0, 2)) * od;
    inv[2][1] = -(m(0, 0) * m(2, 1) - m(2, 0) * m(0, 1)) * od;
    inv[0][2] = +(m(0, 1) * m(1, 2) - m(1, 1) * m(0, 2)) * od;
    inv[1][2] = -(m(0, 0) * m(1, 2) - m(1, 0) * m(0, 2)) * od;
    inv[2][2] = +(m(0, 0) * m(1, 1) - m(1, 0) * m(0, 1)) * od;
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) out[c * 3 + r] = inv[r][c];
}

inline bool identity_model(const float* m) {
    for (int i = 0; i < 16; ++i)
        if (m[i] != ((i % 5 == 0) ? 1.0f : 0.0f)) return false;
    return true;
}

// glm mat4 * mat4 (column j = ((A0*B[j][0] + A1*B[j][1]) + A2*B[j][2]) + A3*B[j][3])
inline void mat4_mul(const float* a, const float* b, float* r) {
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) {
            float s = a[0 * 4 + i] * b[j * 4 + 0];
            s = s + a[1 * 4 + i] * b[j * 4 + 1];
            s = s + a[2 * 4 + i] * b[j * 4 + 2];
            s = s + a[3 * 4 + i] * b[j * 4 + 3];
            r[j * 4 + i] = s;
        }
}

// ---- geometry analysis (UploadMeshFromCache, Renderer.cpp:1965-2116) -------------------------------------------

// What the draw resolution reads of an uploaded geometry.
struct GeomInfo {
    // every vertex has a finite position and a unit normal (|n|^2 within 1e-5 of 1): a draw over it may keep
    // its varyings in object space (TriFrameParams::vary_obj)
    bool obj_ok = false;
    bool uni_col = false;  // every vertex has the colour ucol (TriFrameParams::obj_ucol)
    float ucol[3] = {0.0f, 0.0f, 0.0f};
    float uv_abs[2] = {0.0f, 0.0f};  // max |u|, |v| over the vertices (infinite if any is not finite)
    uint64_t nverts = 0;
    uint64_t nidx = 0;
    std::vector<tri_mesh_range> meshes;
    std::vector<uint32_t> mesh_min, mesh_max;
    std::vector<uint32_t> mesh_cl_first, mesh_ncl, mesh_vblk_first;  // cluster culling tables per mesh
};

// The inclusive interval of a mesh's clusters whose index range meets one 256-slot vertex block (x > y: none).
struct VblkInterval {
    uint32_t x, y;
};

// An upload as the device takes it: the converted vertex streams and the cluster tables, with the GeomInfo beside.
struct GeomAnalysis {
    GeomInfo info;
    std::vector<TriVsIn> vin;     // AoS 100-byte Vertex -> 48-byte shading records
    std::vector<TriVsSkin> skin;  // 32-byte skin records, only when weights exist (has_skin)
    bool has_skin = false;
    // the object-space streams of vary_obj frames: positions (k_vertex) and 36-B attribute records (k_raster)
    std::vector<float> pos, attr;
    // cluster tables (row-band culling): runs of TRI_CLUSTER_PRIMS primitives with their object-space
    // boxes and index ranges; per 256-slot vertex block the interval of clusters whose range meets it
    std::vector<TriCluster> clusters;
    std::vector<VblkInterval> vblk;
    std::vector<TriCluster> vbox;  // parallel to vblk
};

inline int analyse_geometry(const tri_vertex* v, uint64_t nv, const uint32_t* idx, uint64_t ni, const tri_mesh_range* meshes,
                            uint32_t nm, GeomAnalysis& out, Msg& msg) {
    GeomInfo& g = out.info;
    std::vector<TriVsIn>& vin = out.vin;
    vin.assign(nv, TriVsIn{});
    out.skin.clear();
    bool has_skin = false, obj_ok = true;
    float uv_abs[2] = {0.0f, 0.0f};
    for (uint64_t i = 0; i < nv; ++i) {
        for (int k = 0; k < 2; ++k) {
            const float t = std::fabs(v[i].texcoord[k]);
            uv_abs[k] = t <= uv_abs[k] ? uv_abs[k] : (std::isfinite(t) ? t : INFINITY);
        }
        const tri_vertex& s = v[i];
        TriVsIn& o = vin[i];
        o.px = s.position[0]; o.py = s.position[1]; o.pz = s.position[2];
        o.nx = s.normal[0]; o.ny = s.normal[1]; o.nz = s.normal[2];
        const double n2 = (double)o.nx * o.nx + (double)o.ny * o.ny + (double)o.nz * o.nz;
        obj_ok = obj_ok && std::fabs(n2 - 1.0) <= 1e-5 && std::isfinite(o.px) && std::isfinite(o.py) &&
                 std::isfinite(o.pz);
        o.cr = s.color[0]; o.cg = s.color[1]; o.cb = s.color[2];
        o.u = s.texcoord[0]; o.v = s.texcoord[1]; o.pad = 0.0f;
        has_skin = has_skin || s.bone_weights[0] > 0.f || s.bone_weights[1] > 0.f || s.bone_weights[2] > 0.f ||
                   s.bone_weights[3] > 0.f;
    }
    if (has_skin) {
        out.skin.resize(nv);
        for (uint64_t i = 0; i < nv; ++i) {
            std::memcpy(out.skin[i].idx, v[i].bone_indices, 16);
            std::memcpy(out.skin[i].w, v[i].bone_weights, 16);
        }
    }
    out.has_skin = has_skin;
    g.obj_ok = obj_ok;
    g.uv_abs[0] = uv_abs[0]; g.uv_abs[1] = uv_abs[1];
    g.uni_col = nv > 0;
    for (uint64_t i = 0; i < nv && g.uni_col; ++i)
        g.uni_col = vin[i].cr == vin[0].cr && vin[i].cg == vin[0].cg && vin[i].cb == vin[0].cb;
    if (g.uni_col) { g.ucol[0] = vin[0].cr; g.ucol[1] = vin[0].cg; g.ucol[2] = vin[0].cb; }
    out.pos.resize(3 * nv);
    out.attr.resize(9 * nv);
    for (uint64_t i = 0; i < nv; ++i) {
        const TriVsIn& o = vin[i];
        out.pos[3 * i] = o.px; out.pos[3 * i + 1] = o.py; out.pos[3 * i + 2] = o.pz;
        const float a[9] = {o.px, o.py, o.pz, o.nx, o.ny, o.nz, o.cr, o.cg, o.cb};
        std::memcpy(&out.attr[9 * i], a, sizeof a);
    }
    g.nverts = nv;
    g.nidx = ni;
    g.meshes.assign(meshes, meshes + nm);
    g.mesh_min.assign(nm, 0);
    g.mesh_max.assign(nm, 0);
    for (uint32_t m = 0; m < nm; ++m) {  // referenced vertex range per mesh (VS invocation range)
        const tri_mesh_range& mr = meshes[m];
        if (mr.index_count < 3 || (uint64_t)mr.first_index + mr.index_count > ni) continue;
        const uint32_t cnt = (mr.index_count / 3) * 3;
        uint32_t mn = 0xFFFFFFFFu, mx = 0;
        for (uint32_t i = 0; i < cnt; ++i) {
            mn = std::min(mn, idx[mr.first_index + i]);
            mx = std::max(mx, idx[mr.first_index + i]);
        }
        if (mx - mn >= 0x7FFFFFFFu) {
            std::snprintf(msg.text, sizeof msg.text, "mesh %u: index range too large", m);
            return TRI_E_INVALID;
        }
        g.mesh_min[m] = mn;
        g.mesh_max[m] = mx;
    }
    std::vector<TriCluster>& cl = out.clusters;
    std::vector<VblkInterval>& vblk = out.vblk;
    std::vector<TriCluster>& vbox = out.vbox;
    cl.clear();
    vblk.clear();
    vbox.clear();
    g.mesh_cl_first.assign(nm, 0);
    g.mesh_ncl.assign(nm, 0);
    g.mesh_vblk_first.assign(nm, 0);
    for (uint32_t m = 0; m < nm; ++m) {
        const tri_mesh_range& mr = meshes[m];
        if (mr.index_count < 3 || (uint64_t)mr.first_index + mr.index_count > ni) continue;
        const uint32_t ntri = mr.index_count / 3;
        const uint32_t ncl = (ntri + TRI_CLUSTER_PRIMS - 1) / TRI_CLUSTER_PRIMS;
        const uint32_t mn = g.mesh_min[m];
        const uint32_t nblk = (g.mesh_max[m] - mn) / TRI_VBLOCK + 1;
        g.mesh_cl_first[m] = (uint32_t)cl.size();
        g.mesh_ncl[m] = ncl;
        g.mesh_vblk_first[m] = (uint32_t)vblk.size();
        vblk.resize(vblk.size() + nblk, VblkInterval{0xFFFFFFFFu, 0u});
        VblkInterval* iv = vblk.data() + g.mesh_vblk_first[m];
        for (uint32_t k = 0; k < ncl; ++k) {
            TriCluster t;
            for (int a = 0; a < 3; ++a) { t.lo[a] = INFINITY; t.hi[a] = -INFINITY; }
            t.vmin = 0xFFFFFFFFu;
            t.vmax = 0;
            const uint32_t i0 = mr.first_index + 3 * k * TRI_CLUSTER_PRIMS;
            const uint32_t i1 = mr.first_index + 3 * std::min(ntri, (k + 1) * TRI_CLUSTER_PRIMS);
            for (uint32_t i = i0; i < i1; ++i) {
                const uint32_t x = idx[i];
                t.vmin = std::min(t.vmin, x);
                t.vmax = std::max(t.vmax, x);
                const int64_t gi = (int64_t)mr.base_vertex + x;
                if (gi < 0 || (uint64_t)gi >= nv) continue;
                for (int a = 0; a < 3; ++a) {
                    t.lo[a] = std::fmin(t.lo[a], v[gi].position[a]);
                    t.hi[a] = std::fmax(t.hi[a], v[gi].position[a]);
                }
            }
            for (uint32_t bk = (t.vmin - mn) / TRI_VBLOCK; bk <= (t.vmax - mn) / TRI_VBLOCK; ++bk) {
                iv[bk].x = std::min(iv[bk].x, k);
                iv[bk].y = std::max(iv[bk].y, k);
            }
            cl.push_back(t);
        }
        // per vertex block: the union of the boxes of every cluster whose index range meets it (empty when
        // none does): k_vertex keeps the block iff that box can reach the rows, one load and one test per wave
        for (uint32_t bk = 0; bk < nblk; ++bk) {
            TriCluster u;
            for (int a = 0; a < 3; ++a) { u.lo[a] = INFINITY; u.hi[a] = -INFINITY; }
            u.vmin = u.vmax = 0;
            for (uint32_t k = iv[bk].x; iv[bk].x <= iv[bk].y && k <= iv[bk].y; ++k) {
                const TriCluster& t = cl[g.mesh_cl_first[m] + k];
                for (int a = 0; a < 3; ++a) { u.lo[a] = std::fmin(u.lo[a], t.lo[a]); u.hi[a] = std::fmax(u.hi[a], t.hi[a]); }
            }
            vbox.push_back(u);
        }
    }
    return TRI_OK;
}

// ---- draw-list resolution --------------------------------------------------------------------------------------

// Object-space varyings (TriFrameParams::vary_obj) are the world-space ones up to rounding when the draw is
// affine and unskinned (clip_from_world: world = A p + t, a linear map of the interpolated position), its normal
// matrix is conformal (orthogonal columns of one length s, so normalize(NM n) = NM n / s for every unit n and the
// fragment's normalize sees the same direction) and every object normal is unit, with all its vertex records
// in the vertex buffer.
inline bool draw_obj_ok(const GeomInfo& g, const TriDrawDev& d) {
    if (!g.obj_ok || !d.clip_from_world || d.vert_count == 0) return false;
    const int64_t first = (int64_t)d.base_vertex + (int64_t)d.min_index;
    if (first < 0 || (uint64_t)first + d.vert_count > g.nverts) return false;
    double c[3][3];
    for (int k = 0; k < 3; ++k)
        for (int r = 0; r < 3; ++r) c[k][r] = d.nm[k * 3 + r];
    auto dot = [&](int a, int b) { return c[a][0] * c[b][0] + c[a][1] * c[b][1] + c[a][2] * c[b][2]; };
    const double s2 = (dot(0, 0) + dot(1, 1) + dot(2, 2)) / 3.0;
    if (!(s2 > 0.0) || !std::isfinite(s2)) return false;
    const double tol = 1e-5 * s2;
    return std::fabs(dot(0, 0) - s2) <= tol && std::fabs(dot(1, 1) - s2) <= tol && std::fabs(dot(2, 2) - s2) <= tol &&
           std::fabs(dot(0, 1)) <= tol && std::fabs(dot(0, 2)) <= tol && std::fabs(dot(1, 2)) <= tol;
}

// The fast build interpolates a fragment's varyings with weights that carry an absolute error of a few 2^-24 each
// (fast_weights) in a contracted sum, the oracle with exactly rounded ones in its own order. On texture coordinates
// of magnitude M texels the two forms place the bilinear taps about M * 2^-21 texels apart (three weights, the
// reciprocal of their sum, the sum's order): nothing at the M of ordinary content, 2^-8 texel at M = 2^13, one
// byte-level of a full-contrast texel pair, and from there on past the 1-LSB bar (an offset of 4096 over a 6 x 10
// texture: 6 LSB). Float32 coordinates of that size resolve the texture no finer than that themselves, so only the
// oracle's own operation order defines the frame: beyond this many texels a frame takes the exact instantiation
// (interp_exact over exact_weights), whatever the context's flags. 4 x a 2048^2 texture (C5) is still within.
constexpr float kUvFastTexels = 8192.0f;

// A draw list resolved against the uploaded meshes (GatherMeshDraws + the draw loop's skips): the device records
// and base tables (dd, ds of ndraws entries; vb, pb, cb of ndraws + 1), and what the frame derivation reads.
struct DrawResolution {
    std::vector<TriDrawDev> dd;
    std::vector<TriDrawShade> ds;
    std::vector<uint32_t> vb, pb, cb;
    uint32_t ndraws = 0, nslots = 0, nprims = 0, ncl_total = 0;
    bool any_skin = false;
    TriDrawDev draw0{};      // the resolved draw when there is exactly one (passed by value to the kernels)
    TriDrawShade shade0{};   // the shade record of a single-draw frame
    float uv_texels = 0.0f;    // the active textured draws' largest |uv| in texels (see kUvFastTexels)
    bool draw0_obj = false;    // draw0 may keep object-space varyings (draw_obj_ok)
    bool draw0_xform = false;  // ... and its model matrix is not the identity
    bool draw0_ucol = false;   // ... and every vertex of its geometry has one colour
    bool obj48 = false;        // every active draw may keep object-space varyings (TriFrameParams::obj48)
    bool obj48_xform = false;  // ... and some draw's model matrix is not the identity
    uint32_t vdelta[TRI_OBJ48_DRAWS] = {};  // per draw: base_vertex + min_index - first slot
    bool idx_route = false;                   // TriFrameParams::idx_route and its tables
    uint32_t idx_k = 0, pbase[TRI_OBJ48_DRAWS] = {}, vbd[TRI_OBJ48_DRAWS] = {};
};

// texdesc: the TRI_MAX_TEXTURE_SLOTS slot descriptors, aliases resolved. On a refusal only r's tables and uv_texels
// have changed.
inline int resolve_draws(const tri_draw* draws, uint32_t n, const TriTexDesc* texdesc, const GeomInfo& g, DrawResolution& r,
                         Msg& msg) {
    std::vector<TriDrawDev>& dd = r.dd;
    std::vector<TriDrawShade>& ds = r.ds;
    std::vector<uint32_t>&vb = r.vb, &pb = r.pb, &cbase = r.cb;
    dd.resize(n);
    ds.resize(n);
    vb.resize(n + 1);
    pb.resize(n + 1);
    cbase.resize(n + 1);
    uint64_t vslots = 0, prims = 0, ncl = 0;
    bool skin = false;
    float uv_texels = 0.0f;
    for (uint32_t d = 0; d < n; ++d) {
        const tri_draw& src = draws[d];
        TriDrawDev& o = dd[d];
        std::memset(&o, 0, sizeof o);
        std::memcpy(o.model, src.pc.model, 64);
        normal_matrix(src.pc.model, o.nm);
        TriDrawShade& sh = ds[d];
        std::memset(&sh, 0, sizeof sh);
        std::memcpy(sh.tint, src.pc.tint, 16);
        const int32_t slot = src.pc.texture_slot;
        sh.tex = texdesc[(slot >= 0 && slot < TRI_MAX_TEXTURE_SLOTS) ? slot : 0];
        o.tex_scale[0] = src.pc.texture_scale[0];
        o.tex_scale[1] = src.pc.texture_scale[1];
        o.tex_offset[0] = src.pc.texture_offset[0];
        o.tex_offset[1] = src.pc.texture_offset[1];
        o.tiling = src.pc.tiling_factor;
        o.bone_offset = src.pc.bone_offset;
        o.bone_count = src.pc.bone_count;
        o.clip_from_world = (o.bone_count <= 0 && o.model[3] == 0.0f && o.model[7] == 0.0f && o.model[11] == 0.0f &&
                             o.model[15] == 1.0f) ? 1u : 0u;
        vb[d] = (uint32_t)vslots;
        pb[d] = (uint32_t)prims;
        cbase[d] = (uint32_t)ncl;
        if (src.mesh_index >= g.meshes.size()) continue;  // Renderer.cpp:5118-5127 skip
        const tri_mesh_range& mr = g.meshes[src.mesh_index];
        if (mr.index_count < 3 || (uint64_t)mr.first_index + mr.index_count > g.nidx) continue;
        o.first_index = (int32_t)mr.first_index;
        o.base_vertex = mr.base_vertex;
        o.min_index = g.mesh_min[src.mesh_index];
        o.vert_count = g.mesh_max[src.mesh_index] - o.min_index + 1;
        o.cl_first = g.mesh_cl_first[src.mesh_index];
        o.vblk_first = g.mesh_vblk_first[src.mesh_index];
        o.ncl = g.mesh_ncl[src.mesh_index];
        vslots += o.vert_count;
        prims += mr.index_count / 3;
        ncl += o.ncl;
        skin = skin || (o.bone_count > 0);
        if (sh.tex.w != 1 || sh.tex.h != 1) {  // a filtered texture: how far from the origin its taps can lie
            const float ext[2] = {(float)sh.tex.w, (float)sh.tex.h};
            for (int k = 0; k < 2; ++k) {
                const float t = (g.uv_abs[k] * std::fabs(o.tex_scale[k] * o.tiling) + std::fabs(o.tex_offset[k])) * ext[k];
                uv_texels = t <= uv_texels ? uv_texels : (std::isfinite(t) ? t : INFINITY);
            }
        }
    }
    r.uv_texels = uv_texels;
    vb[n] = (uint32_t)vslots;
    pb[n] = (uint32_t)prims;
    cbase[n] = (uint32_t)ncl;
    if (vslots > 0xFFFFFFF0ull) {
        std::snprintf(msg.text, sizeof msg.text, "too many vertex-shader invocations (%llu)", (unsigned long long)vslots);
        return TRI_E_INVALID;
    }
    if (prims > TRI_PRIM_MAX) {
        std::snprintf(msg.text, sizeof msg.text, "too many primitives (%llu > %u)", (unsigned long long)prims, TRI_PRIM_MAX);
        return TRI_E_INVALID;
    }
    r.ndraws = n;
    if (n == 1) {
        r.draw0 = dd[0];
        r.shade0 = ds[0];
    }
    r.draw0_obj = n == 1 && draw_obj_ok(g, dd[0]);
    r.draw0_xform = r.draw0_obj && !identity_model(dd[0].model);
    r.draw0_ucol = r.draw0_obj && g.uni_col;
    // object-space varyings for any draw list (obj48): every active draw affine, unskinned, conformal, with an
    // identity texture transform (uv * scale * tiling + offset == uv bit for bit), at most TRI_OBJ48_DRAWS of them
    r.obj48 = n >= 1 && n <= TRI_OBJ48_DRAWS && !skin;
    r.obj48_xform = false;
    for (uint32_t d = 0; d < n && r.obj48; ++d) {
        const TriDrawDev& o = dd[d];
        r.vdelta[d] = (uint32_t)((int64_t)o.base_vertex + (int64_t)o.min_index - (int64_t)vb[d]);
        if (o.vert_count == 0) continue;  // inactive: no slots, no primitives
        const bool uv_id = o.tex_scale[0] == 1.0f && o.tex_scale[1] == 1.0f && o.tiling == 1.0f &&
                           o.tex_offset[0] == 0.0f && o.tex_offset[1] == 0.0f;
        r.obj48 = uv_id && draw_obj_ok(g, o);
        r.obj48_xform = r.obj48_xform || !identity_model(o.model);
    }
    // the index route (TriFrameParams::idx_route): every active draw's index rows start at idx_k + 3 * its first
    // primitive (one K for all)
    r.idx_route = n >= 2 && n <= TRI_OBJ48_DRAWS;
    bool have_k = false;
    for (uint32_t d = 0; d < n && r.idx_route; ++d) {
        const TriDrawDev& o = dd[d];
        r.vbd[d] = (uint32_t)((int64_t)vb[d] - (int64_t)o.min_index);
        r.pbase[d] = pb[d];
        if (pb[d + 1] == pb[d]) continue;  // no primitives (inactive or skipped)
        const int64_t k = (int64_t)o.first_index - 3 * (int64_t)pb[d];
        if (k < 0 || (have_k && (uint32_t)k != r.idx_k)) r.idx_route = false;
        r.idx_k = (uint32_t)k;
        have_k = true;
    }
    r.nslots = (uint32_t)vslots;
    r.nprims = (uint32_t)prims;
    r.ncl_total = (uint32_t)ncl;
    r.any_skin = skin;
    return TRI_OK;
}

// ---- bin grid and queue capacities -----------------------------------------------------------------------------

// Bin grid: 32x32-pixel bins while the grid stays under 16384 bins (else 64x64). Sparse frames
// (fewer than 0.05 triangles per pixel, e.g. C2's 50k-triangle sphere at 1080p) on small grids use
// 16x16 bins: more workgroups to balance, and few triangles span several bins. Dense bands keep 32x32
// (16x16 measured 10-25 % slower there: more bin entries, each paying its edge set-up).
// A W x H frame, of which the context renders rows [y0, y1); returns log2 of the bin edge.
inline int choose_bin_log2(int32_t W, int32_t H, int32_t y0, int32_t y1, uint32_t nprims) {
    constexpr int forced = TRI_FORCE_BIN_LOG2;
    static_assert(forced == 0 || (forced >= 4 && forced <= 6), "TRI_FORCE_BIN_LOG2: 4, 5 or 6");
    auto bins = [=](int bl) {
        const int32_t bs = 1 << bl;
        return ((W + bs - 1) / bs) * ((y1 - y0 + bs - 1) / bs);
    };
    int bl = forced;
    if (!bl) {
        const double density = (double)nprims / ((double)W * (double)H);
        const int32_t n32 = bins(5);
        bl = n32 > 16384 ? 6 : ((n32 < 4096 && density < 0.05) ? 4 : 5);
    }
    return bl;
}

// per-bin queue capacity (the frame's bins and the shadow map's alike): ~8x the mean entries per bin (1.3 bins per
// triangle), >= 256, never below `cap`: what an overflow grew it to from the observed maximum
inline uint32_t bin_queue_cap(uint32_t cap, uint32_t nprims, uint32_t nbins) {
    const uint64_t mean = ((uint64_t)nprims * 13 / 10) / (uint64_t)std::max<uint32_t>(nbins, 1);
    cap = std::max<uint32_t>(cap, (uint32_t)std::min<uint64_t>(((8 * mean + 64 + 63) / 64) * 64, 1u << 30));
    return std::max<uint32_t>(cap, 256u);
}

// A stride near nchunks / golden ratio, coprime to nchunks.
inline uint32_t chunk_stride(uint32_t n) {
    if (n <= 2) return 1;
    uint32_t s = (uint32_t)((double)n * 0.6180339887) | 1u;
    auto gcd = [](uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; };
    while (gcd(s, n) != 1) ++s;
    return s % n ? s % n : 1u;
}

// ---- frame constants -------------------------------------------------------------------------------------------

// Default.frag frame constants hoisted for the fast shading build (Default.frag:131-174).
inline void shade_constants(const tri_global_ubo& g, const tri_material_record& m, TriShadeConst& sc) {
    std::memset(&sc, 0, sizeof sc);
    std::memcpy(sc.cam, g.camera_position, 16);
    std::memcpy(sc.base, m.base_color_factor, 16);
    sc.metallic = clamp01(m.material_factors[0]);
    sc.roughness = std::fmin(std::fmax(m.material_factors[1], 0.045f), 1.0f);
    sc.amb_strength = clamp01(m.material_factors[2]);
    const float a = sc.roughness * sc.roughness, a2 = a * a, rr = sc.roughness + 1.0f;
    sc.a2m1 = a2 - 1.0f;
    sc.a2pi = a2 / 3.14159265359f;
    sc.kg = rr * rr * 0.125f;
    sc.omkg = 1.0f - sc.kg;
    sc.kgo = sc.kg / sc.omkg;     // omkg >= 0.5 (k <= 0.5 for roughness <= 1)
    sc.a2pio = sc.a2pi / sc.omkg;
    sc.spAk = 0.25f * sc.a2pio;
    sc.spBk = 1e4f * sc.a2pio;
    sc.om = 0.04f * (1.0f - sc.metallic);
    sc.kd = (1.0f - sc.metallic) * (1.0f / 3.14159265359f);
    for (int i = 0; i < 3; ++i) sc.amb[i] = g.ambient_color_intensity[i] * g.ambient_color_intensity[3];
    sc.has_sun = g.light_counts[0] > 0u ? 1u : 0u;
    const float lx = -g.directional_light_direction[0], ly = -g.directional_light_direction[1],
                lz = -g.directional_light_direction[2];
    const float il = 1.0f / std::sqrt((lx * lx + ly * ly) + lz * lz);
    sc.sun_l[0] = lx * il; sc.sun_l[1] = ly * il; sc.sun_l[2] = lz * il;
    for (int i = 0; i < 3; ++i) sc.sun_rad[i] = g.directional_light_color[i] * g.directional_light_color[3];
    sc.npt = std::min<uint32_t>(g.light_counts[1], TRI_MAX_POINT_LIGHTS);
    for (uint32_t i = 0; i < sc.npt; ++i) {
        const tri_point_light& pl = g.point_lights[i];
        for (int k = 0; k < 3; ++k) {
            sc.pl[i].pos[k] = pl.position_range[k];
            sc.pl[i].rad[k] = pl.color_intensity[k] * pl.color_intensity[3];
        }
        sc.pl[i].pos[3] = 1.0f / std::fmax(pl.position_range[3], 1e-4f);
    }
}

// Skybox constants: inverse(Projection) by cofactors in double (rounded to float), mat3(View) and
// the projection's w row (same arithmetic as the oracle's sky_constants()).
inline void sky_constants(const tri_global_ubo& g, float* ip, float* R, float* pw) {
    double a[16], inv[16];
    for (int i = 0; i < 16; ++i) a[i] = g.projection[i];
    inv[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] + a[13] * a[6] * a[11] - a[13] * a[7] * a[10];
    inv[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] - a[12] * a[6] * a[11] + a[12] * a[7] * a[10];
    inv[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] + a[12] * a[5] * a[11] - a[12] * a[7] * a[9];
    inv[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] - a[12] * a[5] * a[10] + a[12] * a[6] * a[9];
    inv[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] - a[13] * a[2] * a[11] + a[13] * a[3] * a[10];
    inv[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] + a[12] * a[2] * a[11] - a[12] * a[3] * a[10];
    inv[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] - a[12] * a[1] * a[11] + a[12] * a[3] * a[9];
    inv[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] + a[12] * a[1] * a[10] - a[12] * a[2] * a[9];
    inv[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] + a[13] * a[2] * a[7] - a[13] * a[3] * a[6];
    inv[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] - a[12] * a[2] * a[7] + a[12] * a[3] * a[6];
    inv[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] + a[12] * a[1] * a[7] - a[12] * a[3] * a[5];
    inv[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] - a[12] * a[1] * a[6] + a[12] * a[2] * a[5];
    inv[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] - a[9] * a[2] * a[7] + a[9] * a[3] * a[6];
    inv[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] + a[8] * a[2] * a[7] - a[8] * a[3] * a[6];
    inv[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] - a[8] * a[1] * a[7] + a[8] * a[3] * a[5];
    inv[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] + a[8] * a[1] * a[6] - a[8] * a[2] * a[5];
    const double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
    const double id = det != 0.0 ? 1.0 / det : 0.0;
    for (int i = 0; i < 16; ++i) ip[i] = (float)(inv[i] * id);
    for (int col = 0; col < 3; ++col)
        for (int r = 0; r < 3; ++r) R[col * 3 + r] = g.view[col * 4 + r];
    for (int col = 0; col < 4; ++col) pw[col] = g.projection[col * 4 + 3];
}

// Each level's first texel and the chain's texel count (level l: 6 faces of max(1, n >> l) squared)
inline uint64_t sky_chain_texels(uint32_t n, uint32_t mips, uint32_t* level_texel) {
    uint64_t at = 0;
    for (uint32_t l = 0; l < mips; ++l) {
        const uint64_t e = std::max(1u, n >> l);
        if (level_texel) level_texel[l] = (uint32_t)at;
        at += 6ull * e * e;
    }
    return at;
}

// ---- tri_shadow_fit_ortho: glm::lookAtRH + glm::orthoRH_ZO (same operation order as the oracle's
// restatement, oracle_shadow_fit_ortho; CPU test compares them bit for bit) ----------------------
struct V3 { float x, y, z; };
inline V3 v3sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 v3mul(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float v3dot(V3 a, V3 b) {  // glm compute_dot: (x + y) + z
    const float tx = a.x * b.x, ty = a.y * b.y, tz = a.z * b.z;
    return (tx + ty) + tz;
}
inline V3 v3cross(V3 x, V3 y) { return {x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y}; }
inline V3 v3norm(V3 v) { return v3mul(v, 1.0f / std::sqrt(v3dot(v, v))); }

inline void shadow_fit_ortho(const float dir[3], const float mn[3], const float mx[3], float out[16]) {
    V3 d{dir[0], dir[1], dir[2]};
    if (!(v3dot(d, d) > 1e-12f)) d = {-0.5f, -1.0f, -0.3f};
    d = v3norm(d);
    const V3 lo{mn[0], mn[1], mn[2]}, hi{mx[0], mx[1], mx[2]};
    const V3 c{(lo.x + hi.x) * 0.5f, (lo.y + hi.y) * 0.5f, (lo.z + hi.z) * 0.5f};
    const float r = std::max(std::sqrt(v3dot(v3sub(hi, lo), v3sub(hi, lo))) * 0.5f, 1e-3f);
    const V3 eye = v3sub(c, v3mul(d, 2.0f * r));
    const V3 up = std::fabs(d.y) > 0.99f ? V3{0.0f, 0.0f, 1.0f} : V3{0.0f, 1.0f, 0.0f};
    // glm::lookAtRH(eye, c, up), column-major V[col*4 + row]
    const V3 f = v3norm(v3sub(c, eye));
    const V3 sv = v3norm(v3cross(f, up));
    const V3 u = v3cross(sv, f);
    float V[16] = {sv.x, u.x, -f.x, 0.0f, sv.y, u.y, -f.y, 0.0f, sv.z, u.z, -f.z, 0.0f,
                   -v3dot(sv, eye), -v3dot(u, eye), v3dot(f, eye), 1.0f};
    float b0[3] = {INFINITY, INFINITY, INFINITY}, b1[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < 8; ++k) {
        const float p[4] = {(k & 1) ? hi.x : lo.x, (k & 2) ? hi.y : lo.y, (k & 4) ? hi.z : lo.z, 1.0f};
        for (int a = 0; a < 3; ++a) {  // glm mat4 * vec4: (m0 v0 + m1 v1) + (m2 v2 + m3 v3)
            const float add0 = V[0 * 4 + a] * p[0] + V[1 * 4 + a] * p[1];
            const float add1 = V[2 * 4 + a] * p[2] + V[3 * 4 + a] * p[3];
            const float q = add0 + add1;
            b0[a] = std::min(b0[a], q);
            b1[a] = std::max(b1[a], q);
        }
    }
    float m[3];
    for (int a = 0; a < 3; ++a) m[a] = (b1[a] - b0[a]) * 0.01f + 1e-4f;
    // glm::orthoRH_ZO(l, r, b, t, n, f); view space looks down -z
    const float l = b0[0] - m[0], rr = b1[0] + m[0], bt = b0[1] - m[1], tp = b1[1] + m[1];
    const float n = -b1[2] - m[2], fr = -b0[2] + m[2];
    float P[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    P[0] = 2.0f / (rr - l);
    P[5] = 2.0f / (tp - bt);
    P[10] = -1.0f / (fr - n);
    P[12] = -(rr + l) / (rr - l);
    P[13] = -(tp + bt) / (tp - bt);
    P[14] = -n / (fr - n);
    mat4_mul(P, V, out);
}

// Some texture larger than 1x1 among the slot descriptors (aliases resolved): every k_raster workgroup stages the
// sRGB LUT.
inline bool slots_need_lut(const TriTexDesc* texdesc) {
    for (int t = 0; t < TRI_MAX_TEXTURE_SLOTS; ++t)
        if (texdesc[t].w != 1 || texdesc[t].h != 1) return true;
    return false;
}

// ---- the frame's parameters ------------------------------------------------------------------------------------

// What derive_frame reads of a context: scalars by value, the large records by pointer (none is copied here).
struct FrameState {
    int32_t W, H, y0, y1, nbx, nby, nbins, bin_log2;
    uint32_t flags;  // tri_config::flags
    int cu_count;
    uint32_t setup_wgs_resident;  // k_setup workgroups per CU in one resident round (its occupancy: TRI_SETUP_WGS_PER_CU)
    const DrawResolution* res;
    const float* ucol;  // the geometry's uniform colour (read when res->draw0_ucol)
    bool need_lut;  // some texture slot holds more than 1x1 texels (slots_need_lut)
    const tri_global_ubo* ubo;
    const float* pv;
    const tri_material_record* mat0;
    const tri_shadow_config* shadow;
    uint32_t s_nbx, s_nbins, s_bin_cap;
    uint32_t ai_w, ai_h;
    uint32_t sky_size, sky_uniform_bgra;
    bool sky_uniform, sky_prefill;
    uint32_t ovf_rec_cap, ovf_vert_cap, bin_cap, nbones, clear_bgra;
};

// Fills fp (every field) from s; *path gets the frame's TRI_PATH_* bits but the kind, *stat_slots the set-up
// launch's statistics slots. A refusal names its message in *msg.
inline int derive_frame(const FrameState& s, TriFrameParams& fp, uint32_t* path, uint32_t* stat_slots, const char** msg) {
    const DrawResolution& r = *s.res;
    const tri_global_ubo& ubo = *s.ubo;
    const uint32_t shadow_size = s.shadow->size;
    std::memset(&fp, 0, sizeof fp);
    fp.W = s.W; fp.H = s.H; fp.y0 = s.y0; fp.y1 = s.y1;
    fp.nbx = s.nbx; fp.nby = s.nby; fp.nbins = s.nbins;
    fp.bin_log2 = s.bin_log2;
    // k_setup grid: a shadow frame takes at most one resident round of workgroups (6 per CU at its
    // occupancy): a workgroup's fetch -> set-up -> reservation -> store chain is latency, and a partial
    // second round doubles the kernel (C3: 1953 chunks of 512 -> 977 of 1024, set-up 33 -> 30 us). Other
    // frames take TRI_SETUP_WGS_PER_CU_OVERLAP per CU with more primitives each, leaving wave slots to the raster of
    // the frame in flight beside them. A band (cluster culling) keeps 512-primitive chunks: most of them exit at
    // once, and the visible ones keep one chain each.
    const bool culling = (s.y0 != 0 || s.y1 != s.H || (s.flags & TRI_FLAG_CLUSTER_CULL)) && r.ncl_total > 0;
    const uint32_t target_chunks = culling ? (uint32_t)TRI_SETUP_BAND_CHUNKS
                                           : (uint32_t)s.cu_count * (shadow_size ? s.setup_wgs_resident
                                                                                 : TRI_SETUP_WGS_PER_CU_OVERLAP);
    uint32_t ppt = (r.nprims + target_chunks * TRI_BLOCK - 1) / (target_chunks * TRI_BLOCK);
    // k_setup sets up and bins pairs: an odd count leaves half of its last round idle, which costs more
    // than the extra chunks save (C3: 3 per lane 29.2 us, 4 per lane 28.3 us), except on a frame whose
    // primitives fit one primitive per lane in one round (C2: 14.2 -> 12.9 us)
    ppt = ppt <= 1 && !culling ? 1u : std::min<uint32_t>(std::max<uint32_t>((ppt + 1) & ~1u, 2), TRI_MAX_PPT);
    fp.ppt = (int32_t)ppt;
    fp.nchunks = (r.nprims + ppt * TRI_BLOCK - 1) / (ppt * TRI_BLOCK);
    fp.chunk_stride = chunk_stride(fp.nchunks);
    *stat_slots = fp.nchunks;
    fp.hw = (float)s.W * 0.5f;
    fp.hh = (float)s.H * 0.5f;
    fp.gx = (2.0f * TRI_GUARD_BAND_PX) / (float)s.W - 1.0f;
    fp.gy = (2.0f * TRI_GUARD_BAND_PX) / (float)s.H - 1.0f;
    fp.nprims = r.nprims;
    fp.nslots = r.nslots;
    fp.ndraws = r.ndraws;
    fp.one_draw = r.ndraws == 1 ? 1u : 0u;
    if (fp.one_draw) fp.draw0 = r.draw0;
    fp.shade_solid = (fp.one_draw && r.shade0.tex.w == 1 && r.shade0.tex.h == 1) ? 1u : 0u;
    // the frames k_raster_plain<.., ONE> shades keep 36-B varyings (no texture coordinates)
    // Default.frag's AI frame blend (:182-191): on when AiBlendConfig.w > 0 and its clamped weight is positive; its
    // frames take k_raster_ai (the general instantiation: world-space or obj48 varyings, never the ONE 36-B records)
    const float ai_wgt = std::fmin(std::fmax(ubo.ai_blend_config[0], 0.0f), 1.0f);
    fp.ai_on = (ubo.ai_blend_config[3] > 0.0f && ai_wgt > 0.0f) ? 1u : 0u;
    if (fp.ai_on) {
        if (!s.ai_w) {
            *msg = "tri_render: AiBlendConfig.w > 0 but no AI frame uploaded (tri_upload_ai_frame)";
            return TRI_E_STATE;
        }
        if (shadow_size) {
            *msg = "tri_render: the AI frame blend with the shadow pre-pass (the reference has no shadow pass)";
            return TRI_E_UNSUPPORTED;
        }
        fp.ai_wgt = ai_wgt;
        fp.ai_sx = ubo.ai_blend_config[1];
        fp.ai_sy = ubo.ai_blend_config[2];
        fp.ai_tw = s.ai_w;
        fp.ai_th = s.ai_h;
    }
    fp.vary36 = (fp.shade_solid && !shadow_size && !fp.ai_on) ? 1u : 0u;
    fp.vary_obj = fp.vary36 && r.draw0_obj ? 1u : 0u;
    fp.obj_xform = fp.vary_obj && r.draw0_xform ? 1u : 0u;
    fp.vin_base = fp.vary_obj ? (uint32_t)((int64_t)r.draw0.base_vertex + (int64_t)r.draw0.min_index) : 0u;
    fp.obj_ucol = fp.vary_obj && r.draw0_ucol ? 1u : 0u;
    if (fp.obj_ucol) std::memcpy(fp.ucol, s.ucol, sizeof fp.ucol);
    // object-space varyings for the other instantiations (the ONE frames keep vary_obj's 36-B records)
    // (not with the pre-pass over a transformed draw: the shadow instantiation carries no per-draw transform)
    fp.obj48 = (!fp.vary36 && r.obj48 && !(shadow_size && r.obj48_xform)) ? 1u : 0u;
    fp.obj48_xform = fp.obj48 && r.obj48_xform ? 1u : 0u;
    // (not with the pre-pass: the shadow kernels carry no draw search)
    fp.idx_route = (r.idx_route && !shadow_size) ? 1u : 0u;
    if (fp.idx_route) {
        fp.idx_k = r.idx_k;
        std::memcpy(fp.pbase, r.pbase, sizeof fp.pbase);
        std::memcpy(fp.vbd, r.vbd, sizeof fp.vbd);
    }
    if (fp.obj48) std::memcpy(fp.vdelta, r.vdelta, sizeof fp.vdelta);  // (zero otherwise: world-space records
                                                                         // at the slots themselves)
    *path = (fp.obj48 ? TRI_PATH_OBJ48 : 0u) | (fp.shade_solid ? TRI_PATH_ONE_DRAW : 0u) | (fp.vary_obj ? TRI_PATH_VARY_OBJ : 0u) |
            (fp.obj_xform ? TRI_PATH_OBJ_XFORM : 0u) | (fp.obj_ucol ? TRI_PATH_OBJ_UCOL : 0u) |
            (shadow_size ? TRI_PATH_SHADOW : 0u) | (fp.idx_route ? TRI_PATH_IDX_ROUTE : 0u);
    fp.ovf_rec_cap = s.ovf_rec_cap;
    fp.ovf_vert_cap = s.ovf_vert_cap;
    fp.bin_cap = s.bin_cap;
    fp.bone_count = s.nbones;
    fp.clear_bgra = s.clear_bgra;
    fp.write_depth = (s.flags & TRI_FLAG_NO_DEPTH_OUTPUT) ? 0u : 1u;
    // ... and frames whose texture coordinates reach beyond kUvFastTexels texels, in either build
    fp.exact_shading = ((s.flags & TRI_FLAG_EXACT_SHADING) || !(r.uv_texels <= kUvFastTexels)) ? 1u : 0u;
    if (fp.exact_shading) *path |= TRI_PATH_EXACT;
    fp.sky_size = s.sky_size;
    if (s.sky_size) {
        sky_constants(ubo, fp.sky_ip, fp.sky_R, fp.sky_pw);
        // the projection's centre is the view origin when its w row has no constant term
        const bool persp = fp.sky_pw[3] == 0.0f;
        fp.sky_mode = !persp ? TRI_SKY_RAY : (s.sky_uniform ? TRI_SKY_UNIFORM : TRI_SKY_PERSP);
        fp.sky_bgra = s.sky_uniform_bgra;
        fp.sky_lut = fp.sky_mode != TRI_SKY_UNIFORM || fp.exact_shading ? 1u : 0u;
        if (s.sky_prefill) {  // k_sky_fill draws the sky: the raster kernel stores no background colour
            fp.sky_mode = TRI_SKY_PREFILLED;
            fp.sky_lut = 0u;
        }
        for (int k = 0; k < 4; ++k) {  // inverse(P) * (xn, yn, 1, 1), row k
            fp.sky_far[4 * k + 0] = fp.sky_ip[0 * 4 + k];
            fp.sky_far[4 * k + 1] = fp.sky_ip[1 * 4 + k];
            fp.sky_far[4 * k + 2] = fp.sky_ip[2 * 4 + k] + fp.sky_ip[3 * 4 + k];
        }
    }
    fp.need_lut = s.need_lut ? 1u : 0u;
    fp.cull_on = culling ? 1u : 0u;
    fp.cull_vertex = fp.cull_on && !shadow_size ? 1u : 0u;  // the pre-pass needs every caster
    fp.ncl_total = r.ncl_total;
    fp.setup_multi = fp.cull_on && fp.one_draw && !shadow_size ? 1u : 0u;
    if (fp.setup_multi) *stat_slots = (fp.nchunks + 3u) / 4u;  // the launch's statistics slots
    if (shadow_size) {
        fp.shadow_on = 1u;
        fp.s_size = shadow_size;
        fp.s_nbx = s.s_nbx;
        fp.s_nbins = s.s_nbins;
        fp.s_bin_cap = s.s_bin_cap;
        fp.s_hw = (float)shadow_size * 0.5f;
        fp.s_g = (2.0f * TRI_GUARD_BAND_PX) / (float)shadow_size - 1.0f;
        fp.s_bias = s.shadow->depth_bias;
        fp.s_slope = s.shadow->slope_bias;
        std::memcpy(fp.lvp, s.shadow->light_view_proj, 64);
    }
    std::memcpy(fp.pv, s.pv, 64);
    fp.ubo = ubo;
    fp.mat0 = *s.mat0;
    shade_constants(ubo, *s.mat0, fp.sc);
    if (fp.shade_solid) {  // (after shade_constants, which clears fp.sc)
        std::memcpy(fp.sc.solid, r.shade0.tex.solid, 16);
        std::memcpy(fp.sc.tint, r.shade0.tint, 16);
        for (int i = 0; i < 3; ++i) fp.sc.sbt[i] = (fp.sc.solid[i] * fp.sc.base[i]) * fp.sc.tint[i];
        fp.sc.sbt[3] = (fp.sc.base[3] * fp.sc.tint[3]) * fp.sc.solid[3];
        fp.sc.a8 = (uint32_t)(int)(std::fmin(std::fmax(fp.sc.sbt[3], 0.0f), 1.0f) * 255.0f + 0.5f);  // unorm8
        const float kd = fp.sc.kd;
        for (int i = 0; i < 3; ++i) {
            fp.sc.sbtm[i] = fp.sc.sbt[i] * fp.sc.metallic;
            fp.sc.sbtkd[i] = fp.sc.sbt[i] * kd;
            fp.sc.sbtamb[i] = (fp.sc.amb[i] * fp.sc.sbt[i]) * fp.sc.amb_strength;
        }
    }
    return TRI_OK;
}

}  // namespace fsel
