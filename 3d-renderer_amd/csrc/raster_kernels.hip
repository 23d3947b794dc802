// raster_kernels.hip — the frame's middle kernels, the shadow pre-pass's raster kernels, the presentation blit, and
// the frame plan that launches every kernel of a frame (the first ones live in vertex_stage.hip, the raster kernels
// of frames without the pre-pass in raster_plain.hip).
//
//   k_setup          tri_setup_bin  primitive assembly + trivial reject + cull + bbox on the per-vertex
//                                   snapped coordinates (Pipeline.cpp:611-643), binned into per-bin queues
//                                   (workgroup- or wave-aggregated atomics); nothing else is stored per
//                                   triangle. Triangles that need homogeneous clipping (rare) are clipped by
//                                   their wave in place: Sutherland-Hodgman against w>=WMIN, z>=0 and the
//                                   guard band + fan, one primitive per wave at a time
//   k_shadow_raster  the shadow map's depth raster, one or more workgroups per 32x32 bin of the map
//   k_raster<.., true>  tile_raster_shade (raster_bin.h) for frames with the pre-pass: one workgroup per bin
//   k_blit           the presentation blit
#define TRI_KERNEL_TU 1  // device pointers in TriDeviceBuffers carry the global address space (raster_launch.h)
#define TRI_PK_SHADE 1   // packed colour pairs (raster_bin.h)
#include "raster_bin.h"

// Tunables (numeric; -D overrides them for A/B builds). k_setup's occupancy and workgroups per CU: raster_launch.h.
#ifndef TRI_RASTER_WAVES
#define TRI_RASTER_WAVES 6  // k_raster occupancy target at 32x32 bins (waves per SIMD)
#endif
#ifndef TRI_RASTER_WAVES_SHADOW
#define TRI_RASTER_WAVES_SHADOW 6  // the fast build's shadow instantiation (80 VGPRs, 6 spilled: C5 raster 158.7 us
                                   // against 166.5 at 5 waves; the exact build keeps 5)
#endif
// TRI_SETUP_WAVES_ONE: the single-draw instantiation without the pre-pass (C2, C3) within 64 VGPRs, so that each of its
// waves takes exactly one raster wave's registers from a concurrent frame's k_raster (8 waves x 64 fill a SIMD's
// register file) instead of 72 — with 3 of its workgroups per CU (TRI_SETUP_WGS_PER_CU_OVERLAP) C3 +0.6 % (round 6 A/B)
#ifndef TRI_SETUP_WAVES_ONE
#define TRI_SETUP_WAVES_ONE 8
#endif
// Binning rounds whose queue reservations k_setup keeps in flight together.
#ifndef TRI_RES_BATCH
#define TRI_RES_BATCH 4
#endif
// Cells of the workgroup-aggregated binning's LDS grid (bin_pair_box)
#ifndef TRI_BIN_GRID
#define TRI_BIN_GRID 1024
#endif
// Primitives per lane that k_setup sets up, then bins, together (2 or 4)
#ifndef TRI_SETUP_GROUP
#define TRI_SETUP_GROUP 2
#endif
// Workgroups per bin of the shadow map (k_shadow_raster)
#ifndef TRI_SHADOW_PARTS
#define TRI_SHADOW_PARTS 4
#endif
// lanes per triangle in the shadow pre-pass's per-lane walk (two paid with the per-texel walk; with the span
// walk one: C5 k_shadow_raster 44.5 -> 43.9 us)
#ifndef TRI_SHADOW_SHARE
#define TRI_SHADOW_SHARE 1
#endif

namespace {

// ------------------------------------------------------------------------------------------
// tri_setup_bin
// ------------------------------------------------------------------------------------------
constexpr int kLdsDraws = 64;  // k_setup stages up to this many draws' lookup data in LDS

// Attribute j (0 position, 1 normal, 2 colour) of geometry vertex gv's 36-B object record
__device__ __forceinline__ F3 vattr_at(const TriDeviceBuffers& b, uint32_t gv, int j) {
    TRI_G const float* q = b.vattr + 9u * gv + 3 * j;
    return F3{q[0], q[1], q[2]};
}
// ... of vertex record vin_base + slot, object space (vary_obj)
__device__ __forceinline__ F3 vin_attr(const TriFrameParams& fp, const TriDeviceBuffers& b, uint32_t slot, int j) {
    return vattr_at(b, fp.vin_base + slot, j);
}

// k_setup's gathers of a primitive's indices, snapped vertices and outcodes as buffer loads from wave-uniform
// descriptors: a record index per lane, no 64-bit address arithmetic, one 12-B index load.
struct SetupBufs {
    RecBuf snap;
    Rsrc oc;
};
__device__ __forceinline__ TriSnap setup_snap(const SetupBufs& sb, uint32_t slot) {
    const uint4 q = rec128<16>(sb.snap, slot, 0u);
    return TriSnap{(int32_t)q.x, (int32_t)q.y, __uint_as_float(q.z), __uint_as_float(q.w)};
}
__device__ __forceinline__ uint32_t setup_oc(const SetupBufs& sb, uint32_t slot) {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(sb.oc, slot, 0, 0);
}

// Setup of a triangle from snapped vertices (all inside w>=WMIN, z>=0 and the guard band).
// Mirrors oracle setup_triangle(). Returns false when culled or when its bbox is empty.
__device__ __forceinline__ bool setup_snapped(const TriFrameParams& fp, const int32_t X[3], const int32_t Y[3],
                                              const float z[3], const float iw[3], uint32_t s0, uint32_t s1,
                                              uint32_t s2, uint32_t prim_sub, TriRec& r, uint2& br) {
    const int64_t S = (int64_t)(X[1] - X[0]) * (int64_t)(Y[2] - Y[0]) -
                      (int64_t)(Y[1] - Y[0]) * (int64_t)(X[2] - X[0]);
    if (S >= 0) return false;  // zero area or back-facing (cull BACK, front CCW)
    const int32_t xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
    const int32_t ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
    int32_t px0 = -floor_shift8(128 - xmin), px1 = floor_shift8(xmax - 128);
    int32_t py0 = -floor_shift8(128 - ymin), py1 = floor_shift8(ymax - 128);
    px0 = max(px0, 0);
    px1 = min(px1, fp.W - 1);
    py0 = max(py0, fp.y0);
    py1 = min(py1, fp.y1 - 1);
    if (px0 > px1 || py0 > py1) return false;
    // swap v1 <-> v2 so the edge functions see S' = -S > 0
    r.X[0] = X[0]; r.X[1] = X[2]; r.X[2] = X[1];
    r.Y[0] = Y[0]; r.Y[1] = Y[2]; r.Y[2] = Y[1];
    r.z[0] = z[0]; r.z[1] = z[2]; r.z[2] = z[1];
    r.iw[0] = iw[0]; r.iw[1] = iw[2]; r.iw[2] = iw[1];
    r.v[0] = s0; r.v[1] = s2; r.v[2] = s1;
    r.prim_sub = prim_sub;
    const uint32_t bl = (uint32_t)fp.bin_log2;
    const uint32_t bx0 = (uint32_t)px0 >> bl, bx1 = (uint32_t)px1 >> bl;
    const uint32_t by0 = (uint32_t)(py0 - fp.y0) >> bl, by1 = (uint32_t)(py1 - fp.y0) >> bl;
    br = make_uint2(bx0 | (by0 << 16), bx1 | (by1 << 16));
    return true;
}

__device__ __forceinline__ bool setup_from_clip(const TriFrameParams& fp, float4 c0, float4 c1, float4 c2,
                                                uint32_t s0, uint32_t s1, uint32_t s2, uint32_t prim_sub, TriRec& r,
                                                uint2& br) {
    int32_t X[3], Y[3];
    float z[3], iw[3];
    snap_compute(fp, c0, X[0], Y[0], z[0], iw[0]);
    snap_compute(fp, c1, X[1], Y[1], z[1], iw[1]);
    snap_compute(fp, c2, X[2], Y[2], z[2], iw[2]);
    return setup_snapped(fp, X, Y, z, iw, s0, s1, s2, prim_sub, r, br);
}

template <typename F>
__device__ __forceinline__ void for_bins(uint2 br, int nbx, F&& f) {
    const uint32_t bx0 = br.x & 0xFFFFu, by0 = br.x >> 16, bx1 = br.y & 0xFFFFu, by1 = br.y >> 16;
    for (uint32_t by = by0; by <= by1; ++by)
        for (uint32_t bx = bx0; bx <= bx1; ++bx) f(by * (uint32_t)nbx + bx);
}

// Wave-aggregated queue reservation: every lane with `want` gets one slot in bin `bin`. Lanes of the
// wave that target the same bin form a group; each group's leader issues ONE atomicAdd for the whole
// group (all leaders at once, one round trip), and members take consecutive slots after it. Must be
// reached by the whole wave (uniform control flow).

// Reservation plan (ALU and ballots only): each wanting lane learns its group's leader lane and its
// rank in the group; a leader learns its group's size.
__device__ __forceinline__ void wave_reserve_plan(uint32_t bin, bool want, uint32_t& leader, uint32_t& rank,
                                                  uint32_t& cnt) {
    uint64_t pending = __ballot(want);
    const uint32_t lane = lanes_below(~0ull);
    leader = lane; rank = 0; cnt = 0;
    while (pending) {
        const uint32_t l = (uint32_t)__builtin_ctzll(pending);
        const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)bin, (int)l);
        const uint64_t grp = __ballot(want && bin == lb) & pending;
        if (want && bin == lb) {
            leader = l;
            rank = lanes_below(grp);
        }
        if (lane == l) cnt = (uint32_t)__builtin_popcountll(grp);
        pending &= ~grp;
    }
}

constexpr int kResBatch = TRI_RES_BATCH;  // binning rounds whose queue reservations k_setup keeps in flight together

// ------------------------------------------------------------------------------------------
// Homogeneous clipping (oracle clip_polygon: Sutherland-Hodgman against w >= WMIN, z >= 0 and the
// guard band, then a fan), done by the whole wave for one primitive at a time inside k_setup: lane i
// holds polygon vertex i, the output order of the sequential algorithm is rebuilt with ballots, and
// the two polygon buffers live in a per-wave LDS slice. No separate launch, no per-lane arrays.
// ------------------------------------------------------------------------------------------
struct ClipVert {
    float4 c;
    float b0, b1, b2;  // barycentric weights on the source triangle (for the varyings)
};
constexpr int kClipStride = 8;  // floats per LDS polygon vertex
constexpr int kWavesPerBlock = TRI_BLOCK / 64;

__device__ __forceinline__ ClipVert lerp_cv(const ClipVert& a, const ClipVert& b, float t) {
    ClipVert o;
#define L(f) o.f = a.f + t * (b.f - a.f)
    L(c.x); L(c.y); L(c.z); L(c.w); L(b0); L(b1); L(b2);
#undef L
    return o;
}

__device__ __forceinline__ float plane_dist(const TriFrameParams& fp, int plane, float4 c) {
    switch (plane) {
        case 0: return c.w - TRI_WMIN;
        case 1: return c.z;
        case 2: return c.x + fp.gx * c.w;
        case 3: return fp.gx * c.w - c.x;
        case 4: return c.y + fp.gy * c.w;
        default: return fp.gy * c.w - c.y;
    }
}

// The polygons live in LDS: the pointers say so (a generic pointer would make every access a flat instruction)
#if defined(__HIP_DEVICE_COMPILE__)
#define TRI_LDS __attribute__((address_space(3)))
#else
#define TRI_LDS
#endif
__device__ __forceinline__ void cv_store(TRI_LDS float* p, const ClipVert& v) {
    p[0] = v.c.x; p[1] = v.c.y; p[2] = v.c.z; p[3] = v.c.w; p[4] = v.b0; p[5] = v.b1; p[6] = v.b2;
}
__device__ __forceinline__ ClipVert cv_load(TRI_LDS const float* p) {
    ClipVert v;
    v.c = make_float4(p[0], p[1], p[2], p[3]);
    v.b0 = p[4]; v.b1 = p[5]; v.b2 = p[6];
    return v;
}

// LDS traffic between lanes of one wave: DS instructions of a wave execute in order, so a
// compiler barrier is all that is needed between a lane's store and another lane's load.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Clip primitive `prim` (vertex slots sl[3]) with the whole wave; lanes that set up a fan
// sub-triangle bin it. Must be reached by the whole wave.
// `draw`: the primitive's draw (wave-uniform), for obj48 frames' object records and model matrix.
template <bool LPOS, bool ONE>
__device__ __forceinline__ void clip_prim_wave(const TriFrameParams& fp, const TriDeviceBuffers& b, TRI_LDS float* poly,
                                               uint32_t prim, uint32_t sl0, uint32_t sl1, uint32_t sl2, bool cfw,
                                               uint32_t draw, uint32_t& nsetup, uint32_t& nentries) {
    const uint32_t lane = lanes_below(~0ull);
    const uint64_t below = (lane == 63) ? 0x7FFFFFFFFFFFFFFFull : ((1ull << lane) - 1ull);
    TRI_LDS float* buf[2] = {poly, poly + TRI_MAX_CLIP_VERTS * kClipStride};
    // object-space records: the ONE frames' (vary_obj: 36-B records at vin_base + slot, never with the pre-pass),
    // or obj48's (the 48-B input records at slot + vdelta[draw]). ONE here is k_setup's single-draw instantiation, not
    // the raster's: a single draw may be an obj48 frame too (a textured draw, the pre-pass, the AI blend), and then
    // k_vertex wrote no varyings for the clipper to read (draw is 0 and fp.draw0 is that draw)
    const bool obj1 = !LPOS && obj_mode(fp), o48 = obj48_mode(fp);
    const bool one_draw = ONE || fp.one_draw;
    const uint32_t dl = o48 ? fp.vdelta[min(draw, (uint32_t)TRI_OBJ48_DRAWS - 1u)] : fp.vin_base;
    if (lane < 3) {
        ClipVert v;
        const uint32_t sl = lane == 0 ? sl0 : (lane == 1 ? sl1 : sl2);
        if (cfw && b.oc[sl] == 0u) {  // not stored by k_vertex: world.w == 1
            F3 wv;
            if (obj1 || o48) {  // k_vertex's world position, from the record (same operations)
                const F3 p = vattr_at(b, dl + sl, 0);
                float m[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) m[i] = (o48 && !one_draw) ? b.draws[draw].model[i] : fp.draw0.model[i];
                const float4 w = mat_vec_seq(m, make_float4(p.x, p.y, p.z, 1.0f));
                wv = F3{w.x, w.y, w.z};
            } else {
                wv = vary36_mode(fp) ? ldF3(reinterpret_cast<TRI_G const F3*>(b.vary) + 3u * sl)
                                     : F3{b.vary[3u * sl].x, b.vary[3u * sl].y, b.vary[3u * sl].z};
            }
            v.c = mat_vec_seq(fp.pv, make_float4(wv.x, wv.y, wv.z, 1.0f));
        } else {
            v.c = b.clip[sl];
        }
        v.b0 = lane == 0 ? 1.0f : 0.0f;
        v.b1 = lane == 1 ? 1.0f : 0.0f;
        v.b2 = lane == 2 ? 1.0f : 0.0f;
        cv_store(buf[0] + lane * kClipStride, v);
    }
    int n = 3, cur = 0;
    for (int plane = 0; plane < 6 && n > 0; ++plane) {
        wave_lds_sync();
        const bool act = (int)lane < n;
        ClipVert a{}, nb{};
        float da = 0.0f, db = 0.0f;
        if (act) {
            a = cv_load(buf[cur] + lane * kClipStride);
            nb = cv_load(buf[cur] + ((int)lane + 1 < n ? lane + 1 : 0) * kClipStride);
            da = plane_dist(fp, plane, a.c);
            db = plane_dist(fp, plane, nb.c);
        }
        const bool in = act && da >= 0.0f;
        const bool cross = act && ((da >= 0.0f) != (db >= 0.0f));
        const uint64_t m_in = __ballot(in), m_cr = __ballot(cross);
        const int pos = __builtin_popcountll(m_in & below) + __builtin_popcountll(m_cr & below);
        wave_lds_sync();
        if (in && pos < TRI_MAX_CLIP_VERTS) cv_store(buf[cur ^ 1] + pos * kClipStride, a);
        const int pos2 = pos + (in ? 1 : 0);
        if (cross && pos2 < TRI_MAX_CLIP_VERTS) {
            const float t = da / (da - db);
            cv_store(buf[cur ^ 1] + pos2 * kClipStride, lerp_cv(a, nb, t));
        }
        n = min(__builtin_popcountll(m_in) + __builtin_popcountll(m_cr), TRI_MAX_CLIP_VERTS);
        cur ^= 1;
    }
    wave_lds_sync();
    if (n < 3) return;
    n = min(n, TRI_MAX_CLIP_POLY);
    const uint32_t nsub = (uint32_t)(n - 2);
    uint32_t rbase = 0, vbase = 0;
    if (lane == 0) {
        rbase = atomicAdd(&b.counters->ovf_records, nsub);
        vbase = atomicAdd(&b.counters->ovf_verts, (uint32_t)n);
    }
    rbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)rbase);
    vbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)vbase);
    if (rbase + nsub > fp.ovf_rec_cap || vbase + (uint32_t)n > fp.ovf_vert_cap) {
        if (lane == 0)
            atomicOr(&b.counters->flags, (rbase + nsub > fp.ovf_rec_cap) ? TRI_OVF_CLIP_RECORDS : TRI_OVF_CLIP_VERTS);
        return;
    }
    const uint32_t sbase = fp.nslots + vbase;
    TRI_LDS const float* src = buf[cur];
    if ((int)lane < n) {  // varyings of polygon vertex `lane` from the source triangle's barycentrics
        const ClipVert s = cv_load(src + lane * kClipStride);
        if (vary36_mode(fp)) {  // (object-space attributes from the vertex records with vary_obj)
            TRI_G const F3* v0 = reinterpret_cast<TRI_G const F3*>(b.vary) + 3u * sl0;
            TRI_G const F3* v1 = reinterpret_cast<TRI_G const F3*>(b.vary) + 3u * sl1;
            TRI_G const F3* v2 = reinterpret_cast<TRI_G const F3*>(b.vary) + 3u * sl2;
            TRI_G F3* vo = reinterpret_cast<TRI_G F3*>(b.vary) + 3u * (sbase + lane);
            const bool obj = !LPOS && obj_mode(fp);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const F3 x = obj ? vin_attr(fp, b, sl0, j) : ldF3(v0 + j), y = obj ? vin_attr(fp, b, sl1, j) : ldF3(v1 + j),
                         z = obj ? vin_attr(fp, b, sl2, j) : ldF3(v2 + j);
                vo[j] = F3{(s.b0 * x.x + s.b1 * y.x) + s.b2 * z.x, (s.b0 * x.y + s.b1 * y.y) + s.b2 * z.y,
                           (s.b0 * x.z + s.b1 * y.z) + s.b2 * z.z};
            }
        } else {  // 48-B records: the world-space varyings, or (obj48) the input records' own layout
            const float4* v0 = o48 ? reinterpret_cast<TRI_G const float4*>(b.vin + (dl + sl0)) : b.vary + 3u * sl0;
            const float4* v1 = o48 ? reinterpret_cast<TRI_G const float4*>(b.vin + (dl + sl1)) : b.vary + 3u * sl1;
            const float4* v2 = o48 ? reinterpret_cast<TRI_G const float4*>(b.vin + (dl + sl2)) : b.vary + 3u * sl2;
            float4* vo = b.vary + 3u * (sbase + lane);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float4 x = v0[j], y = v1[j], z = v2[j];
                vo[j] = make_float4((s.b0 * x.x + s.b1 * y.x) + s.b2 * z.x, (s.b0 * x.y + s.b1 * y.y) + s.b2 * z.y,
                                    (s.b0 * x.z + s.b1 * y.z) + s.b2 * z.z, (s.b0 * x.w + s.b1 * y.w) + s.b2 * z.w);
            }
        }
        if constexpr (LPOS) {  // shadow pre-pass on: the polygon vertex's light-space position, same weights
            const float4 x = b.lpos[sl0], y = b.lpos[sl1], z = b.lpos[sl2];
            b.lpos[sbase + lane] = make_float4((s.b0 * x.x + s.b1 * y.x) + s.b2 * z.x,
                                               (s.b0 * x.y + s.b1 * y.y) + s.b2 * z.y,
                                               (s.b0 * x.z + s.b1 * y.z) + s.b2 * z.z, 0.0f);
        }
    }
    if (lane == 0) b.clip_slot[prim] = rbase;  // k_raster's fragment fetch finds sub-triangle `sub` at + sub - 1
    if (lane < nsub) {  // fan sub-triangle k = lane + 1: (v0, vk, vk+1)
        const uint32_t k = lane + 1;
        TriRec r;
        uint2 br;
        const uint32_t ps = (prim << 3) | k;  // sub = k >= 1 marks a clipped primitive's sub-triangle
        const uint32_t rid = rbase + k - 1;
        const float4 c0 = cv_load(src).c, ck = cv_load(src + k * kClipStride).c,
                     ck1 = cv_load(src + (k + 1) * kClipStride).c;
        if (setup_from_clip(fp, c0, ck, ck1, sbase, sbase + k, sbase + k + 1, ps, r, br)) {
            ++nsetup;
            b.recs[rid] = r;
            for_bins(br, fp.nbx, [&](uint32_t bi) {  // rare path: one global atomic per entry
                const uint32_t pos = atomicAdd(&b.bin_count[bi], 1u);
                if (pos < fp.bin_cap) b.bin_list[(size_t)bi * fp.bin_cap + pos] = TRI_ENTRY_CLIPPED | rid;
                else note_bin_overflow(b, pos + 1);
                ++nentries;
            });
        }
    }
}

// Shadow pre-pass set-up of a triangle from its map snaps (oracle shadow_raster_triangle): no culling,
// only zero-area triangles drop; the bbox of texel centres inside the map, as 32x32 bin ranges.
__device__ __forceinline__ bool shadow_bins(const TriFrameParams& fp, const int32_t X[3], const int32_t Y[3], uint2& br) {
    const int64_t S = (int64_t)(X[1] - X[0]) * (int64_t)(Y[2] - Y[0]) -
                      (int64_t)(Y[1] - Y[0]) * (int64_t)(X[2] - X[0]);
    if (S == 0) return false;
    const int32_t xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
    const int32_t ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
    const int32_t n1 = (int32_t)fp.s_size - 1;
    const int32_t px0 = max(-floor_shift8(128 - xmin), 0), px1 = min(floor_shift8(xmax - 128), n1);
    const int32_t py0 = max(-floor_shift8(128 - ymin), 0), py1 = min(floor_shift8(ymax - 128), n1);
    if (px0 > px1 || py0 > py1) return false;
    br = make_uint2((uint32_t)(px0 >> 5) | ((uint32_t)(py0 >> 5) << 16), (uint32_t)(px1 >> 5) | ((uint32_t)(py1 >> 5) << 16));
    return true;
}

__device__ __forceinline__ void note_shadow_bin_overflow(const TriDeviceBuffers& b, uint32_t needed) {
    atomicOr(&b.counters->flags, TRI_OVF_SHADOW_BIN_LIST);
    atomicMax(&b.counters->sbin_max, needed);
}

// One lane per primitive (ppt primitives per lane): assembly from the snapped vertices, trivial
// reject, cull, bbox, then one bin-queue entry per touched bin (batched wave reservations). Nothing else is
// written for a visible triangle: k_raster rebuilds it from `snap`. Triangles needing homogeneous
// clipping are clipped right here by their wave (clip_prim_wave). Entry order inside a bin is free:
// k_raster resolves visibility with (depth, primitive order) keys.

// Per-wave binning (the shadow and frame rounds whose workgroup bin box is too large for bin_pair_box's
// LDS grid): the lane's bin-queue entries, one per round: triangle 0's bbox bins, then triangle 1's. A batch of
// kResBatch rounds is planned with ballots and its reservations (one returning atomic per (wave, bin))
// are all issued before any result is used, so a wave waits for one atomic round trip per batch instead
// of one per round. Must be reached by the whole wave. Diagnostics: TRI_ABLATE=8 waits per round.
// Component-wise selects (a plain `c ? a : b` on uint4 became a dynamically indexed stack array).
__device__ __forceinline__ uint32_t pick(bool c, uint32_t a, uint32_t b) { return c ? a : b; }
__device__ __forceinline__ uint4 pick(bool c, uint4 a, uint4 b) {
    return make_uint4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

template <bool SHADOW_QUEUES, typename Q>
__device__ __forceinline__ void bin_pair(const TriDeviceBuffers& b, bool ok0, bool ok1, uint2 br0, uint2 br1, Q p0, Q p1,
                                         uint32_t nbx, uint32_t* bin_count, Q* bin_list, uint32_t cap, uint32_t lane,
                                         uint32_t& nentries) {
    bool has = (ok0 || ok1) && !(kAblate & 4);  // diagnostics: 4 = setup without binning
    bool second = !ok0;
    uint2 cur = second ? br1 : br0;
    uint32_t bx = cur.x & 0xFFFFu, by = cur.x >> 16;
    uint32_t bx0 = bx, bx1 = cur.y & 0xFFFFu, by1 = cur.y >> 16;
    const int batch = (kAblate & 8) ? 1 : kResBatch;
    while (__ballot(has)) {
        uint32_t rbin[kResBatch], rlr[kResBatch], rbase[kResBatch];  // rlr: group leader lane | rank << 8
        bool rwant[kResBatch], rsec[kResBatch];
#pragma unroll
        for (int r = 0; r < kResBatch; ++r) {
            rwant[r] = has && r < batch;
            rbin[r] = by * nbx + bx;
            rsec[r] = second;
            if (rwant[r]) {
                if (bx < bx1) {
                    ++bx;
                } else if (by < by1) {
                    bx = bx0;
                    ++by;
                } else if (!second && ok1) {
                    second = true;
                    bx = bx0 = br1.x & 0xFFFFu; by = br1.x >> 16;
                    bx1 = br1.y & 0xFFFFu; by1 = br1.y >> 16;
                } else {
                    has = false;
                }
            }
            uint32_t cnt, lead, rank;
            wave_reserve_plan(rbin[r], rwant[r], lead, rank, cnt);
            rlr[r] = lead | (rank << 8);
            rbase[r] = 0;
            if (rwant[r] && lane == lead && !(kAblate & 16))  // diagnostics: 16 = no atomics
                rbase[r] = atomicAdd(&bin_count[rbin[r]], cnt);
        }
#pragma unroll
        for (int r = 0; r < kResBatch; ++r) {
            const uint32_t pos = (uint32_t)__shfl((int)rbase[r], (int)(rlr[r] & 0xFFu)) + (rlr[r] >> 8);
            if (rwant[r]) {
                if (kAblate & 32) continue;  // diagnostics: 32 = no queue stores
                if (pos < cap) bin_list[(size_t)rbin[r] * cap + pos] = pick(rsec[r], p1, p0);
                else if (SHADOW_QUEUES) note_shadow_bin_overflow(b, pos + 1);
                else note_bin_overflow(b, pos + 1);
                ++nentries;
            }
        }
    }
}

// Workgroup-aggregated binning: a round's entries (two primitives per lane) are counted per bin in an
// LDS grid over the workgroup's union bin box (a wave min-reduction + one LDS atomicMin per wave and
// corner), one returning global atomic per (workgroup, bin) reserves the bin's run, and each entry takes
// its position in the run from a returning LDS atomic. The counts return to zero as positions are handed
// out, so the grid is never cleared. A round whose box exceeds kBinGrid cells bins with the per-wave
// reservations above (a uniform choice: every wave reads the same box). Must be reached by the whole
// workgroup. Rejected alternative: an LDS hash table keyed by bin (CAS probing): C3 set-up +2 us.
constexpr uint32_t kBinGrid = TRI_BIN_GRID;
struct BinBox {
    uint32_t cnt[kBinGrid];
    uint32_t base[kBinGrid];
    uint32_t box[2][2][4];  // per queue set and round parity: min bx, min by, ~max bx, ~max by (LDS atomicMin)
};

// The wave's minimum (uniform), as a DPP scan: row_shr 1/2/4/8 inside each row of 16, then row_bcast:15 / :31
// across rows; lane 63 ends with the minimum of all lanes. Lanes whose DPP source is out of range keep ~0 (the
// identity), so each step is one v_min with a DPP operand instead of a ds_bpermute round trip per step.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_max_id(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)~0u, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    v = min(v, dpp_max_id<0x111>(v));
    v = min(v, dpp_max_id<0x112>(v));
    v = min(v, dpp_max_id<0x114>(v));
    v = min(v, dpp_max_id<0x118>(v));
    v = min(v, dpp_max_id<0x142, 0xa>(v));
    v = min(v, dpp_max_id<0x143, 0xc>(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

constexpr int kSetupGroup = TRI_SETUP_GROUP;  // primitives per lane set up, then binned, together
static_assert(kSetupGroup == 2 || kSetupGroup == 4, "k_setup groups are one or two primitive pairs");

template <bool SHADOW_QUEUES>
__device__ __forceinline__ void bin_pair_box(const TriDeviceBuffers& b, BinBox& g, uint32_t round,
                                             const bool (&ok)[kSetupGroup], const uint2 (&br)[kSetupGroup],
                                             const uint32_t (&p)[kSetupGroup], uint32_t nbx, uint32_t* bin_count,
                                             uint32_t* bin_list, uint32_t cap, uint32_t lane, uint32_t& nentries) {
    if (kAblate & 4) return;  // diagnostics: 4 = setup without binning
    const uint32_t q = round & 1u;
    uint32_t (&box)[2][4] = g.box[SHADOW_QUEUES ? 1 : 0];
    uint32_t m[4] = {~0u, ~0u, ~0u, ~0u};
#pragma unroll
    for (int t = 0; t < kSetupGroup; ++t)
        if (ok[t]) {
            m[0] = min(m[0], br[t].x & 0xFFFFu); m[1] = min(m[1], br[t].x >> 16);
            m[2] = min(m[2], ~(br[t].y & 0xFFFFu)); m[3] = min(m[3], ~(br[t].y >> 16));
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m[i] = wave_min(m[i]);
        if (lane == 0 && m[i] != ~0u) atomicMin(&box[q][i], m[i]);
    }
    __syncthreads();
    const uint32_t ox = box[q][0], oy = box[q][1], ex = ~box[q][2], ey = ~box[q][3];
    // the other parity's box was last read before this barrier; the next round accumulates into it only
    // after one more barrier (below, or on the early paths)
    if (threadIdx.x < 4) box[q ^ 1u][threadIdx.x] = ~0u;
    if (ox == ~0u) {  // no entry in the workgroup this round
        __syncthreads();
        return;
    }
    const uint32_t w = ex - ox + 1u, cells = w * (ey - oy + 1u);
    if (cells > kBinGrid) {
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kSetupGroup; t += 2)
            bin_pair<SHADOW_QUEUES>(b, ok[t], ok[t + 1], br[t], br[t + 1], p[t], p[t + 1], nbx, bin_count, bin_list,
                                    cap, lane, nentries);
        return;
    }
#pragma unroll
    for (int t = 0; t < kSetupGroup; ++t)
        if (ok[t])
            for (uint32_t by = br[t].x >> 16; by <= (br[t].y >> 16); ++by)
                for (uint32_t bx = br[t].x & 0xFFFFu; bx <= (br[t].y & 0xFFFFu); ++bx)
                    atomicAdd(&g.cnt[(by - oy) * w + bx - ox], 1u);
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < cells; c += TRI_BLOCK) {
        const uint32_t n = g.cnt[c];
        if (n) {
            const uint32_t cy = c / w;
            const uint32_t base = atomicAdd(&bin_count[(oy + cy) * nbx + ox + (c - cy * w)], n);
            g.base[c] = base;
            if (base + n > cap) {
                if (SHADOW_QUEUES) note_shadow_bin_overflow(b, base + n);
                else note_bin_overflow(b, base + n);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kSetupGroup; ++t)
        if (ok[t])
            for (uint32_t by = br[t].x >> 16; by <= (br[t].y >> 16); ++by)
                for (uint32_t bx = br[t].x & 0xFFFFu; bx <= (br[t].y & 0xFFFFu); ++bx) {
                    const uint32_t c = (by - oy) * w + bx - ox;
                    const uint32_t pos = g.base[c] + atomicSub(&g.cnt[c], 1u) - 1u;
                    if (pos < cap) bin_list[(size_t)(by * nbx + bx) * cap + pos] = p[t];
                    ++nentries;
                }
}

// WITH_SHADOW (frames with the shadow pre-pass): the same index fetch also sets up every primitive
// for the map (oracle shadow_raster_triangle: light-NDC snaps, no culling, no clipping, guard-band
// violators dropped) and bins it into the map's own queues; clipped polygon vertices get light-space
// positions. A separate instantiation keeps that code, and its registers, out of other frames.
// ONE: a single-draw frame (fp.one_draw known set: the draw search, LDS staging and prim_vs records compile
// away)
// One set-up workgroup: chunk workgroup `bid` of `nblk`.
template <bool WITH_SHADOW, bool ONE>
__device__ __forceinline__ void setup_body(const TriFrameParams& fp, const TriDeviceBuffers& b, uint32_t bid,
                                           uint32_t nblk) {
    if constexpr (WITH_SHADOW) {  // the map to 1.0 before k_shadow_raster's parts merge into it (coalesced stores)
        const uint32_t nt = fp.s_size * fp.s_size;
        for (uint32_t i = bid * TRI_BLOCK + threadIdx.x; i < nt; i += nblk * TRI_BLOCK) b.shadow_map[i] = 0x3F800000u;
    }
    __shared__ uint32_t red[2];
    __shared__ float clip_poly[kWavesPerBlock][2 * TRI_MAX_CLIP_VERTS * kClipStride];
    // Frames with a few draws: each draw's primitive base, first index, slot offset and cluster base
    // staged in LDS once per workgroup, so a primitive finds its draw and index row without the global
    // binary search -> draw record chain in front of its index fetch.
    __shared__ uint32_t dpb[kLdsDraws + 1], dfi[kLdsDraws], dvb[kLdsDraws], dcb[kLdsDraws];
    const bool lds_draws = !ONE && !fp.one_draw && fp.ndraws <= (uint32_t)kLdsDraws;
    __shared__ BinBox bin_box;
    // Row bands of single-draw frames (fp.setup_multi): a quarter of the chunks' workgroups, each owning the
    // four chunks bid + i * nblk. Wave i reads chunk i's cluster flags, and the workgroup sets up
    // and bins the visible ones in turn (a band's visible chunks are contiguous, so the stride gives each
    // workgroup at most one at N = 8, and 3/4 of the launch's mostly empty dispatches are gone).
    __shared__ uint32_t chunk_vis[TRI_BLOCK / 64];
    const bool multi = ONE && !WITH_SHADOW && fp.cull_on && fp.setup_multi;
    const auto chunk_visible = [&](uint32_t ck) {
        const uint32_t p0 = ck * (uint32_t)(TRI_BLOCK * fp.ppt);
        const uint32_t p1 = min(p0 + (uint32_t)(TRI_BLOCK * fp.ppt), fp.nprims);
        bool any = false;
        for (uint32_t c = p0 / TRI_CLUSTER_PRIMS; c <= (p1 - 1) / TRI_CLUSTER_PRIMS && !any; ++c) any = b.cvis[c] != 0u;
        return any;
    };
    if constexpr (ONE && !WITH_SHADOW) {
        if (multi) {
            const uint32_t w = threadIdx.x / 64u, ck = bid + w * nblk;
            const bool vis = ck < fp.nchunks && chunk_visible(ck);
            if ((threadIdx.x & 63u) == 0) chunk_vis[w] = vis ? 1u : 0u;
            __syncthreads();
            bool any = false;
#pragma unroll
            for (int i = 0; i < TRI_BLOCK / 64; ++i) any = any || chunk_vis[i] != 0u;
            if (!any) {
                if (threadIdx.x == 0) b.setup_stats[bid] = make_uint2(0u, 0u);
                return;
            }
        } else if (fp.cull_on) {
            // A row band's chunk whose clusters k_vertex culled (most chunks at N = 8): the whole workgroup
            // leaves before the LDS set-up and the binning barriers (its cluster flags: a few scalar loads)
            if (!chunk_visible((uint32_t)(((uint64_t)bid * fp.chunk_stride) % fp.nchunks))) {
                if (threadIdx.x == 0) b.setup_stats[bid] = make_uint2(0u, 0u);
                return;
            }
        }
    }
    for (uint32_t s = threadIdx.x; s < kBinGrid; s += TRI_BLOCK) bin_box.cnt[s] = 0;
    if (threadIdx.x < 16) bin_box.box[threadIdx.x >> 3][(threadIdx.x >> 2) & 1][threadIdx.x & 3] = ~0u;
    TRI_SSTAMP(0);
    if (threadIdx.x < 2) red[threadIdx.x] = 0;
    if (lds_draws) {
        for (uint32_t i = threadIdx.x; i <= fp.ndraws; i += TRI_BLOCK) dpb[i] = b.draw_pbase[i];
        for (uint32_t i = threadIdx.x; i < fp.ndraws; i += TRI_BLOCK) {
            dfi[i] = (uint32_t)b.draws[i].first_index;
            dvb[i] = b.draw_vbase[i] - b.draws[i].min_index;
            dcb[i] = fp.cull_on ? b.draw_cbase[i] : 0u;
        }
    }
    __syncthreads();
    uint32_t nsetup = 0, nentries = 0, sentries = 0;
    const uint32_t lane = lanes_below(~0ull);
    const SetupBufs sbuf{rec_buf(b.snap, 16u, fp.nslots), make_rsrc(b.oc, fp.nslots)};
    const RecBuf ibuf = rec_buf(b.indices + fp.draw0.first_index, 12u, fp.nprims);  // single-draw frames
    uint32_t round_base = 0;  // binning rounds so far (the bin box alternates its two halves per round)
    for (uint32_t ci = 0; ci < (multi ? (uint32_t)(TRI_BLOCK / 64) : 1u); ++ci) {
    if (multi && !chunk_vis[ci]) continue;  // uniform
    // Spread concurrently running workgroups over the primitive stream: meshes are usually
    // index-ordered in screen space, and neighbouring chunks hammering the same bin counters
    // serialise their atomics. The stride is coprime to nchunks, so the remap is a bijection.
    const uint32_t chunk = multi ? bid + ci * nblk : (uint32_t)(((uint64_t)bid * fp.chunk_stride) % fp.nchunks);
    const uint32_t chunk0 = chunk * (uint32_t)(TRI_BLOCK * fp.ppt);
    // Two primitives per lane, set up and binned together: both index/vertex fetch chains are in
    // flight at once, and the queue reservations of both are batched (one atomic round trip per
    // batch), so a wave's dependent latencies are paid once for two primitives.
    for (int k = 0; k < fp.ppt; k += kSetupGroup) {  // uniform trip count: binning needs the whole workgroup
        uint32_t p[kSetupGroup], sl0[kSetupGroup], sl1[kSetupGroup], sl2[kSetupGroup];
        bool ok[kSetupGroup], needs_clip[kSetupGroup], sok[kSetupGroup];
        int pd[kSetupGroup];  // the primitive's draw
        uint2 br[kSetupGroup], sbr[kSetupGroup];
#pragma unroll
        for (int t = 0; t < kSetupGroup; ++t) {
            const bool in_chunk = k + t < fp.ppt;  // ppt need not be a multiple of the group
            p[t] = in_chunk ? chunk0 + (k + t) * TRI_BLOCK + threadIdx.x : ~0u;
            ok[t] = false; needs_clip[t] = false; sok[t] = false;
            sl0[t] = sl1[t] = sl2[t] = 0;
            br[t] = make_uint2(0u, 0u);
            sbr[t] = make_uint2(0u, 0u);
            bool culled = false;
            int& d = pd[t];
            d = 0;
            uint32_t vb = 0, i0 = 0, i1 = 0, i2 = 0;
            if (p[t] < fp.nprims) {
                // the indices are fetched together with the cluster flag, not after it: a band's
                // visible primitives skip one dependent load (a culled one wastes 12 bytes)
                const uint32_t* ip;
                if (ONE || fp.one_draw) {  // kernel-argument constants: the index fetch starts at once
                    vb = 0u - fp.draw0.min_index;
                    const u32x3v q = rec96<12>(ibuf, p[t], 0u);
                    i0 = q[0]; i1 = q[1]; i2 = q[2];
                    if (fp.cull_on) culled = !b.cvis[p[t] / TRI_CLUSTER_PRIMS];
                } else if (lds_draws) {
                    d = find_range_lds(dpb, (int)fp.ndraws, p[t]);
                    const uint32_t lp = p[t] - dpb[d];
                    ip = b.indices + dfi[d] + 3u * lp;
                    vb = dvb[d];
                    i0 = ip[0]; i1 = ip[1]; i2 = ip[2];
                    if (fp.cull_on) culled = !b.cvis[dcb[d] + lp / TRI_CLUSTER_PRIMS];
                } else {
                    d = find_range(b.draw_pbase, (int)fp.ndraws, p[t]);
                    const TriDrawDev& dr = b.draws[d];
                    const uint32_t lp = p[t] - b.draw_pbase[d];
                    ip = b.indices + dr.first_index + 3u * lp;
                    vb = b.draw_vbase[d] - dr.min_index;
                    i0 = ip[0]; i1 = ip[1]; i2 = ip[2];
                    if (fp.cull_on) culled = !b.cvis[b.draw_cbase[d] + lp / TRI_CLUSTER_PRIMS];
                }
            }
            // a primitive culled for the context's rows may still cast a shadow into the map
            if (p[t] < fp.nprims && (!culled || WITH_SHADOW)) {
                sl0[t] = vb + i0; sl1[t] = vb + i1; sl2[t] = vb + i2;
                if (!culled) {
                    const TriSnap a0 = setup_snap(sbuf, sl0[t]), a1 = setup_snap(sbuf, sl1[t]), a2 = setup_snap(sbuf, sl2[t]);
                    const uint32_t oc0 = setup_oc(sbuf, sl0[t]), oc1 = setup_oc(sbuf, sl1[t]), oc2 = setup_oc(sbuf, sl2[t]);
                    // invalid vertex, or trivial reject: all three vertices outside one clip half-space
                    if (!((oc0 | oc1 | oc2) & TRI_OC_BAD) && !(oc0 & oc1 & oc2 & TRI_OC_REJECT)) {
                        if ((oc0 | oc1 | oc2) & TRI_OC_CLIP) {
                            needs_clip[t] = true;
                        } else {
                            const int32_t X[3] = {snap_X(a0), snap_X(a1), snap_X(a2)};
                            const int32_t Y[3] = {snap_Y(a0), snap_Y(a1), snap_Y(a2)};
                            const float z[3] = {a0.z, a1.z, a2.z};
                            const float iw[3] = {a0.iw, a1.iw, a2.iw};
                            TriRec r;
                            ok[t] = setup_snapped(fp, X, Y, z, iw, sl0[t], sl1[t], sl2[t], p[t] << 3, r, br[t]);
                        }
                    }
                }
                if constexpr (WITH_SHADOW) {
                    const TriSnap l0 = b.lsnap[sl0[t]], l1 = b.lsnap[sl1[t]], l2 = b.lsnap[sl2[t]];
                    const uint32_t oc0 = (uint32_t)l0.xo >> 24, oc1 = (uint32_t)l1.xo >> 24, oc2 = (uint32_t)l2.xo >> 24;
                    if (!((oc0 | oc1 | oc2) & (TRI_OC_BAD | TRI_OC_CLIP)) && !(oc0 & oc1 & oc2 & TRI_OC_REJECT)) {
                        const int32_t X[3] = {(l0.xo << 8) >> 8, (l1.xo << 8) >> 8, (l2.xo << 8) >> 8};
                        const int32_t Y[3] = {l0.y, l1.y, l2.y};
                        sok[t] = shadow_bins(fp, X, Y, sbr[t]);
                    }
                }
                // k_raster's (and k_shadow_raster's) route from the primitive to its vertex slots and draw; a
                // single-draw frame finds the slots in the index buffer instead (prim_slots)
                if (!ONE && !fp.one_draw && !fp.idx_route && (ok[t] || needs_clip[t] || sok[t]))
                    b.prim_vs[p[t]] = make_uint4(sl0[t], sl1[t], sl2[t], (uint32_t)d | (needs_clip[t] ? TRI_PRIM_CLIPPED : 0u));
            }
            nsetup += ok[t] ? 1u : 0u;
        }
        if (k == 0) TRI_SSTAMP(1);
#pragma unroll
        for (int t = 0; t < kSetupGroup; ++t) {
            uint64_t cm = __ballot(needs_clip[t]);  // rare: the wave clips its primitives one at a time
            if (cm) {
                if (lane == 0) atomicAdd(&b.counters->tris_clipped, (uint32_t)__builtin_popcountll(cm));
                TRI_LDS float* poly = (TRI_LDS float*)clip_poly[threadIdx.x >> 6];
                while (cm) {
                    const int src = __builtin_ctzll(cm);
                    cm &= cm - 1;
                    clip_prim_wave<WITH_SHADOW, ONE>(fp, b, poly, (uint32_t)__builtin_amdgcn_readlane((int)p[t], src),
                                                (uint32_t)__builtin_amdgcn_readlane((int)sl0[t], src),
                                                (uint32_t)__builtin_amdgcn_readlane((int)sl1[t], src),
                                                (uint32_t)__builtin_amdgcn_readlane((int)sl2[t], src),
                                                (ONE || fp.one_draw) ? fp.draw0.clip_from_world != 0u
                                                            : b.draws[__builtin_amdgcn_readlane(pd[t], src)].clip_from_world != 0u,
                                                (ONE || fp.one_draw) ? 0u : (uint32_t)__builtin_amdgcn_readlane(pd[t], src),
                                                nsetup, nentries);
                }
            }
        }
        bin_pair_box<false>(b, bin_box, round_base + (uint32_t)(k / kSetupGroup), ok, br, p, (uint32_t)fp.nbx,
                            b.bin_count, b.bin_list, fp.bin_cap, lane, nentries);
        if constexpr (WITH_SHADOW)
            bin_pair_box<true>(b, bin_box, round_base + (uint32_t)(k / kSetupGroup), sok, sbr, p, fp.s_nbx,
                               b.sbin_count, b.sbin_list, fp.s_bin_cap, lane, sentries);
        if (k == 0) TRI_SSTAMP(2);
    }
    round_base += (uint32_t)((fp.ppt + kSetupGroup - 1) / kSetupGroup);
    }
    if (nsetup) atomicAdd(&red[0], nsetup);
    if (nentries) atomicAdd(&red[1], nentries);
    __syncthreads();
    // Statistics go to a per-workgroup slot with a plain store: same-address global atomics from
    // every workgroup serialise across the XCDs (measured: +34 us per frame at 4K/1M).
    if (threadIdx.x == 0) b.setup_stats[bid] = make_uint2(red[0], red[1]);
    TRI_SSTAMP(3);
}

template <bool WITH_SHADOW, bool ONE>
__global__ __launch_bounds__(TRI_BLOCK) __attribute__((amdgpu_waves_per_eu((ONE && !WITH_SHADOW) ? TRI_SETUP_WAVES_ONE : TRI_SETUP_WAVES))) void k_setup(TRI_KARGS) {
    TRI_BIND_ARGS;
    setup_body<WITH_SHADOW, ONE>(fp, b, blockIdx.x, gridDim.x);
}

// 6 waves/SIMD at 32x32 bins: the fast build fits 80 VGPRs without spilling (the exact build spills
// a little); 64x64 bins are LDS-limited to 3. One workgroup per bin: a persistent grid (one resident
// round of workgroups, each walking bins blockIdx + k * gridDim on its XCD) measured 121.5 -> 154 us at C3
// (13 VGPRs spilled by values hoisted out of the bin loop, and a static bin order that balances worse
// than the dispatcher's).
template <bool EXACT, int BL, bool SHADOW>
__global__ __launch_bounds__(TRI_BLOCK) __attribute__((amdgpu_waves_per_eu(BL <= 5 ? (SHADOW ? (EXACT ? 5 : TRI_RASTER_WAVES_SHADOW) : TRI_RASTER_WAVES) : 3))) void k_raster(TRI_KARGS) {
    TRI_BIND_ARGS;
    if constexpr (SHADOW)  // the map bins' counts for the next frame (k_shadow_raster's parts only read them)
        for (uint32_t i = blockIdx.x * TRI_BLOCK + threadIdx.x; i < fp.s_nbins; i += gridDim.x * TRI_BLOCK)
            b.sbin_count[i] = 0u;
    raster_bin<EXACT, BL, SHADOW>(fp, b, xcd_bin(blockIdx.x, fp.nbins));
}

// ------------------------------------------------------------------------------------------
// shadow pre-pass raster (oracle shadow_raster_triangle): one workgroup per 32x32 bin of the s_size^2
// map, the bin's depth tile in LDS (min over covering fragments of the [0, 1]-clamped plane depth, as
// uint32 bits: order-free), then one coalesced store of the tile. The triangle of a queue entry is
// rebuilt from its three map snaps (prim_slots -> lsnap), oriented like the set-up (v1 <-> v2 swapped when
// S < 0, kept when S > 0: no culling).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ TriRec load_shadow_entry(const TriFrameParams& fp, const TriDeviceBuffers& b, uint32_t e) {
    const Rsrc snr = make_rsrc(b.lsnap, 16ull * fp.nslots);
    uint32_t sl[3], d;
    prim_slots<false, false>(fp, b, e, sl, d);  // (no index route on shadow frames)
    const uint4 q0 = ld128(snr, sl[0] * 16u), q1 = ld128(snr, sl[1] * 16u), q2 = ld128(snr, sl[2] * 16u);
    const int32_t X0 = ((int32_t)q0.x << 8) >> 8, X1 = ((int32_t)q1.x << 8) >> 8, X2 = ((int32_t)q2.x << 8) >> 8;
    const int32_t Y0 = (int32_t)q0.y, Y1 = (int32_t)q1.y, Y2 = (int32_t)q2.y;
    const int64_t S = (int64_t)(X1 - X0) * (int64_t)(Y2 - Y0) - (int64_t)(Y1 - Y0) * (int64_t)(X2 - X0);
    const bool sw = S < 0;
    TriRec r;
    r.X[0] = X0; r.Y[0] = Y0; r.z[0] = __uint_as_float(q0.w);
    r.X[1] = sw ? X2 : X1; r.Y[1] = sw ? Y2 : Y1; r.z[1] = __uint_as_float(sw ? q2.w : q1.w);
    r.X[2] = sw ? X1 : X2; r.Y[2] = sw ? Y1 : Y2; r.z[2] = __uint_as_float(sw ? q1.w : q2.w);
    r.iw[0] = r.iw[1] = r.iw[2] = 1.0f;
    r.prim_sub = e << 3;
    r.v[0] = r.v[1] = r.v[2] = 0;
    return r;
}

// Depth clamp to [0, 1] on the float bits (finite depth: the plane of snapped vertices with S != 0):
// negative (sign set, -0 included) -> +0, above 1 -> 1.
__device__ __forceinline__ uint32_t clamp_depth_bits(float z) {
    return (uint32_t)min(max(__float_as_int(z), 0), 0x3F800000);
}

// Slope-scaled depth bias of a caster (depthBiasSlopeFactor): slope * its largest depth change per texel.
__device__ __forceinline__ float slope_offset(const TriFrameParams& fp, const EdgeSetup& e) {
    return fp.s_slope * (fmaxf(fabsf(e.dzdX), fabsf(e.dzdY)) * 256.0f);
}

__device__ __forceinline__ void shadow_serial(const TriFrameParams& fp, const TriRec& r, int32_t cx0, int32_t cx1,
                                              int32_t cy0, int32_t cy1, int32_t ox, int32_t oy, uint32_t* dep,
                                              int32_t sub, int32_t step) {
    EdgeSetup e;
    edge_setup(r, e);
    const float off = slope_offset(fp, e);
    bool rej = false;
    int32_t F[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) F[k] = clamp_edge((int64_t)e.A[k] * cx0 + (int64_t)e.B[k] * cy0 + e.D[k], rej);
    if (rej) return;
    const float fdx0 = (float)(256 * cx0 + 128 - r.X[0]);
    float fdy = (float)(256 * (cy0 + sub) + 128 - r.Y[0]);
    uint32_t row = (uint32_t)(((cy0 + sub - oy) << 5) + (cx0 - ox));
#pragma unroll
    for (int k = 0; k < 3; ++k) F[k] += e.B[k] * sub;
    for (int32_t py = cy0 + sub; py <= cy1; py += step) {
        const float t2 = e.dzdY * fdy;
        int32_t f0 = F[0], f1 = F[1], f2 = F[2];
        float fdx = fdx0;
        const uint32_t rend = row + (uint32_t)(cx1 - cx0);
        for (uint32_t a = row; a <= rend; ++a) {
            if ((f0 | f1 | f2) >= 0) atomicMin(&dep[a], clamp_depth_bits(((r.z[0] + e.dzdX * fdx) + t2) + off));
            f0 += e.A[0]; f1 += e.A[1]; f2 += e.A[2];
            fdx += 256.0f;
        }
        F[0] += e.B[0] * step; F[1] += e.B[1] * step; F[2] += e.B[2] * step;
        fdy += 256.0f * (float)step;
        row += (uint32_t)step << 5;
    }
}

// The span walk of raster_span for the map (triangles under 64 px on a side; the rest keep shadow_serial):
// each map row's covered texels from the three edge crossings, exact by the same argument, the same depth
// (plane + slope bias, clamped) as shadow_serial.
__device__ __forceinline__ void shadow_span(const TriFrameParams& fp, const TriRec& r, int32_t cx0, int32_t cx1,
                                            int32_t cy0, int32_t cy1, int32_t ox, int32_t oy, uint32_t* dep,
                                            int32_t sub, int32_t step) {
    const int32_t xmin = min(r.X[0], min(r.X[1], r.X[2])), xmax = max(r.X[0], max(r.X[1], r.X[2]));
    const int32_t ymin = min(r.Y[0], min(r.Y[1], r.Y[2])), ymax = max(r.Y[0], max(r.Y[1], r.Y[2]));
    if (!(xmax - xmin < 16384 && ymax - ymin < 16384)) {
        shadow_serial(fp, r, cx0, cx1, cy0, cy1, ox, oy, dep, sub, step);
        return;
    }
    int32_t A[3], B[3], F[3];
    EdgeSetup e;
    edge_start(r, cx0, cy0, A, B, F, e.dzdX, e.dzdY);  // the 32-bit form (same integers and depth plane)
    const float off = slope_offset(fp, e);
    constexpr float kDelta = 0x1p-15f;
    float nrl[3], dl[3], nrr[3], dr[3], Ff[3], Bs[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float rc = -__builtin_amdgcn_rcpf((float)A[k]);
        nrl[k] = A[k] > 0 ? rc : (A[k] == 0 ? -0x1p100f : 0.0f);
        dl[k] = A[k] >= 0 ? -kDelta : -INFINITY;
        nrr[k] = A[k] < 0 ? rc : 0.0f;
        dr[k] = A[k] < 0 ? kDelta : INFINITY;
        Ff[k] = (float)(F[k] + B[k] * sub);
        Bs[k] = (float)(B[k] * step);
    }
    const float wmax = (float)(cx1 - cx0);
    const int32_t fx0 = 256 * cx0 + 128 - r.X[0];
    float fdy = (float)(256 * (cy0 + sub) + 128 - r.Y[0]);
    uint32_t row = (uint32_t)(((cy0 + sub - oy) << 5) + (cx0 - ox));
    for (int32_t py = cy0 + sub; py <= cy1; py += step) {
        const float tl = fmaxf(fmaxf(__builtin_fmaf(Ff[0], nrl[0], dl[0]), __builtin_fmaf(Ff[1], nrl[1], dl[1])),
                               __builtin_fmaf(Ff[2], nrl[2], dl[2]));
        const float tr = fminf(fminf(__builtin_fmaf(Ff[0], nrr[0], dr[0]), __builtin_fmaf(Ff[1], nrr[1], dr[1])),
                               __builtin_fmaf(Ff[2], nrr[2], dr[2]));
        const float Lf = fmaxf(ceilf(tl), 0.0f), Rf = fminf(floorf(tr), wmax);
        if (Lf <= Rf) {
            const int32_t L = (int32_t)Lf, R = (int32_t)Rf;
            const float t2 = e.dzdY * fdy;
            float fdx = (float)(fx0 + 256 * L);
            const uint32_t rend = row + (uint32_t)R;
            for (uint32_t a = row + (uint32_t)L; a <= rend; ++a) {
                atomicMin(&dep[a], clamp_depth_bits(((r.z[0] + e.dzdX * fdx) + t2) + off));
                fdx += 256.0f;
            }
        }
        Ff[0] += Bs[0]; Ff[1] += Bs[1]; Ff[2] += Bs[2];
        fdy += 256.0f * (float)step;
        row += (uint32_t)step << 5;
    }
}

// The map's bins are very uneven (C5: 1294 of 4096 hold casters, 773 on average, 4042 at most — the light sees
// the grid at a grazing angle), and one workgroup per bin made the heaviest bins the whole kernel. Each bin now
// has TRI_SHADOW_PARTS workgroups: part p takes the bin's entries in blocks of 256, every TRI_SHADOW_PARTS-th block,
// into its own LDS tile. A bin with one block keeps one workgroup and stores its tile; with more, every part
// atomicMin's the texels it covered into the map, which k_setup<true> cleared to 1.0 (k_raster zeroes the bins'
// counts for the next frame: the parts of a bin cannot tell which of them reads its count last).
__global__ __launch_bounds__(TRI_BLOCK) void k_shadow_raster(TRI_KARGS) {
    TRI_BIND_ARGS;
    constexpr int BIN = 32;
    constexpr uint32_t kParts = TRI_SHADOW_PARTS;
    __shared__ uint32_t dep[BIN * BIN];
    __shared__ uint32_t bigq[kBigQueue];
    __shared__ uint32_t nbig, nentries;
    const int tid = threadIdx.x;
    // parts of one bin lie s_nbins workgroups apart: the same XCD (s_nbins is a multiple of 8) and its L2
    const uint32_t part = blockIdx.x / fp.s_nbins;
    const int bin = xcd_bin((int)(blockIdx.x - part * fp.s_nbins), (int)fp.s_nbins);
    const int32_t S = (int32_t)fp.s_size;
    const int32_t ox = (bin % (int)fp.s_nbx) * BIN, oy = (bin / (int)fp.s_nbx) * BIN;
    const int32_t bw = min(BIN, S - ox), bh = min(BIN, S - oy);
    if (tid == 0) {
        nbig = 0;
        const uint32_t cnt = b.sbin_count[bin];
        if (cnt > fp.s_bin_cap && part == 0) note_shadow_bin_overflow(b, cnt);
        nentries = min(cnt, fp.s_bin_cap);
    }
    __syncthreads();
    const uint32_t n = nentries;
    // nothing for this part (the map is already 1.0 there: k_setup<true> cleared it — unless the frame had no
    // primitives, no k_setup, and part 0 writes the empty tile itself)
    const bool store_empty = part == 0 && fp.nchunks == 0;
    if (n <= part * (uint32_t)TRI_BLOCK && !store_empty) return;
    for (int i = tid; i < BIN * BIN; i += TRI_BLOCK) dep[i] = 0x3F800000u;  // clear 1.0
    __syncthreads();
    const uint32_t* queue = b.sbin_list + (size_t)bin * fp.s_bin_cap;
    const int share = n <= (uint32_t)(TRI_BLOCK / TRI_SHADOW_SHARE) ? TRI_SHADOW_SHARE : 1;
    const int sub = tid % share;
    const uint32_t step = share > 1 ? (uint32_t)(TRI_BLOCK / share) : (uint32_t)TRI_BLOCK * kParts;
    for (uint32_t i = tid / share + part * (uint32_t)TRI_BLOCK; i < n; i += step) {
        const uint32_t ri = queue[i];
        const TriRec r = load_shadow_entry(fp, b, ri);
        int32_t cx0, cx1, cy0, cy1;
        rec_bbox(r, ox, oy, bw, bh, cx0, cx1, cy0, cy1);
        if (cx0 > cx1 || cy0 > cy1) continue;
        if ((cx1 - cx0 + 1) * (cy1 - cy0 + 1) > big_area<5>()) {
            if (sub != 0) continue;
            const uint32_t q = atomicAdd(&nbig, 1u);
            if (q < kBigQueue) { bigq[q] = ri; continue; }
            shadow_serial(fp, r, cx0, cx1, cy0, cy1, ox, oy, dep, 0, 1);
            continue;
        }
        shadow_span(fp, r, cx0, cx1, cy0, cy1, ox, oy, dep, sub, share);
    }
    __syncthreads();
    const uint32_t nb = min(nbig, (uint32_t)kBigQueue);
    for (uint32_t q = 0; q < nb; ++q) {  // large triangles: all lanes share the texels
        const TriRec r = load_shadow_entry(fp, b, bigq[q]);
        int32_t cx0, cx1, cy0, cy1;
        rec_bbox(r, ox, oy, bw, bh, cx0, cx1, cy0, cy1);
        EdgeSetup e;
        edge_setup(r, e);
        bool rej = false;
        int32_t F[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) F[k] = clamp_edge((int64_t)e.A[k] * cx0 + (int64_t)e.B[k] * cy0 + e.D[k], rej);
        if (rej) continue;  // uniform across the workgroup
        const float off = slope_offset(fp, e);
        const int32_t rw = cx1 - cx0 + 1, rh = cy1 - cy0 + 1;
        for (int j = tid; j < rw * rh; j += TRI_BLOCK) {
            const int32_t dy = j / rw, dx = j - dy * rw;
            if ((F[0] + e.A[0] * dx + e.B[0] * dy | F[1] + e.A[1] * dx + e.B[1] * dy | F[2] + e.A[2] * dx + e.B[2] * dy) >= 0) {
                const int32_t px = cx0 + dx, py = cy0 + dy;
                atomicMin(&dep[((py - oy) << 5) + (px - ox)], clamp_depth_bits(frag_depth(r, e, px, py) + off));
            }
        }
    }
    __syncthreads();
    const bool alone = n <= (uint32_t)TRI_BLOCK || kParts == 1 || store_empty;  // one part: its tile is the bin's
    for (int i = tid; i < BIN * BIN; i += TRI_BLOCK) {
        const int32_t ly = i >> 5, lx = i & 31;
        if (lx < bw && ly < bh) {
            const size_t o = (size_t)(oy + ly) * S + ox + lx;
            if (alone) b.shadow_map[o] = dep[i];
            else if (dep[i] != 0x3F800000u) atomicMin(&b.shadow_map[o], dep[i]);  // depth bits order as integers
        }
    }
}

// ------------------------------------------------------------------------------------------
// presentation blit (Renderer.cpp:5346-5361, vkCmdBlitImage with VK_FILTER_LINEAR): one lane per
// destination texel; the source coordinate of its centre is (x + 0.5) * (W / dw), filtered
// bilinearly over clamp-to-edge taps on UNORM values (b / 255), rounded to UNORM8. Same float
// operation order as the oracle's blit_linear (bit-exact). Rows are coalesced per wave. The 256-entry
// UNORM table is staged in LDS: read from global memory it was 16 wave-level gathers per texel on the texture
// path, which held a 4K blit at ≈ 70 µs beside the next frame's raster (tri_launch_blit copies an equal-size
// blit instead: its weights are 0 and every channel rounds back to its byte).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRI_BLOCK) void k_blit(const uint32_t* __restrict__ src, int32_t w, int32_t h,
                                                    uint32_t* __restrict__ dst, int32_t dw, int32_t dh, float sx,
                                                    float sy, const float* __restrict__ lut) {
    __shared__ float tab[256];
    for (int i = (int)threadIdx.x; i < 256; i += TRI_BLOCK) tab[i] = lut[i];
    __syncthreads();
    const int32_t x = (int32_t)(blockIdx.x * 64 + (threadIdx.x & 63));
    const int32_t y = (int32_t)(blockIdx.y * (TRI_BLOCK / 64) + (threadIdx.x >> 6));
    if (x >= dw || y >= dh) return;
    const float u = ((float)x + 0.5f) * sx - 0.5f;
    const float v = ((float)y + 0.5f) * sy - 0.5f;
    const float fu = floorf(u), fv = floorf(v);
    const float a = u - fu, bb = v - fv;
    const int32_t i0 = (int32_t)fu, j0 = (int32_t)fv;
    const int32_t xa = min(max(i0, 0), w - 1), xb = min(max(i0 + 1, 0), w - 1);
    const int32_t ya = min(max(j0, 0), h - 1), yb = min(max(j0 + 1, 0), h - 1);
    const uint32_t p00 = src[(size_t)ya * w + xa], p10 = src[(size_t)ya * w + xb];
    const uint32_t p01 = src[(size_t)yb * w + xa], p11 = src[(size_t)yb * w + xb];
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float t00 = tab[(p00 >> (8 * c)) & 0xFFu], t10 = tab[(p10 >> (8 * c)) & 0xFFu];
        const float t01 = tab[(p01 >> (8 * c)) & 0xFFu], t11 = tab[(p11 >> (8 * c)) & 0xFFu];
        const float l0 = t00 + a * (t10 - t00);
        const float l1 = t01 + a * (t11 - t01);
        out |= unorm8(l0 + bb * (l1 - l0)) << (8 * c);
    }
    dst[(size_t)y * dw + x] = out;
}

}  // namespace

// The frame's raster kernel: k_raster<.., true> at its bin size with the shadow pre-pass, else raster_plain.hip's
template <int BL>
static const void* shadow_raster_kernel(bool exact) {
    return exact ? reinterpret_cast<const void*>(k_raster<true, BL, true>)
                 : reinterpret_cast<const void*>(k_raster<false, BL, true>);
}
static const void* raster_kernel(const TriFrameParams& fp) {
    if (!fp.shadow_on) return tri_raster_plain_kernel(fp);
    const bool exact = fp.exact_shading != 0;
    return fp.bin_log2 == 5   ? shadow_raster_kernel<5>(exact)
           : fp.bin_log2 == 4 ? shadow_raster_kernel<4>(exact)
                              : shadow_raster_kernel<6>(exact);
}

void tri_plan_frame(const TriFrameParams& fp, TriFramePlan& plan, bool id_pass, TriMotionPass motion) {
    plan.n = 0;
    auto add = [&](const void* f, dim3 g, dim3 t, int stage) { plan.k[plan.n++] = TriKernelLaunch{f, g, t, stage}; };
    auto F = [](auto kernel) { return reinterpret_cast<const void*>(kernel); };
    const dim3 t(TRI_BLOCK);
    if (fp.nslots > 0 && fp.cull_vertex && fp.one_draw)
        // one workgroup per four vertex blocks (TRI_VBLOCK == TRI_BLOCK slots each)
        add(tri_vertex_stage_kernel(kFrontBand), dim3((fp.nslots + 4u * TRI_VBLOCK - 1) / (4u * TRI_VBLOCK)), t, kStageVertex);
    else if (fp.nslots > 0)
        // with cluster culling every (draw, cluster) flag needs a lane, even when a mesh has fewer vertices
        add(tri_vertex_stage_kernel(kFrontVertex), dim3(((fp.cull_on && fp.ncl_total > fp.nslots ? fp.ncl_total : fp.nslots) + TRI_BLOCK - 1) / TRI_BLOCK),
            t, kStageVertex);
    else
        add(tri_vertex_stage_kernel(kFrontReset), dim3(1), dim3(TRI_BLOCK), kStageVertex);
    if (fp.nchunks > 0) {  // with the pre-pass, one set-up pass bins each primitive for the frame and the map
        const dim3 g(fp.setup_multi ? (fp.nchunks + 3u) / 4u : fp.nchunks);
        const void* k = fp.shadow_on ? (fp.one_draw ? F(k_setup<true, true>) : F(k_setup<true, false>))
                                     : (fp.one_draw ? F(k_setup<false, true>) : F(k_setup<false, false>));
        add(k, g, t, kStageSetup);
    }
    if (fp.shadow_on)  // the map's depth raster, before the frame's raster samples it
        add(F(k_shadow_raster), dim3(fp.s_nbins * TRI_SHADOW_PARTS), t, kStageShadow);
    // the id pass reads the bin counts and queues the raster kernel consumes (a frame without primitives has no
    // queues: its ids are cleared by the caller)
    if (id_pass && fp.nchunks > 0) add(tri_id_raster_kernel(fp), dim3(fp.nbins), t, kStageId);
    add(raster_kernel(fp), dim3(fp.nbins), t, kStageRaster);
    if (motion != kMotionOff) {  // reads the depth the raster kernel wrote
        const bool vec4 = motion == kMotionVec4;
        add(tri_motion_kernel(vec4), tri_motion_grid((uint32_t)fp.W * (uint32_t)(fp.y1 - fp.y0), vec4), t, kStageMotion);
    }
}

#ifdef TRI_DIAG_FRONT
// Diagnostics build: what the front end costs a frame beside its raster (tri_render): 1 = after a context's first
// frame only k_raster runs (over that frame's queues, which it keeps), 2 = the same with two empty launches in place
// of k_vertex and k_setup (the launches and their stream order, without their work), 3 = k_vertex and k_raster
__global__ void k_diag_empty(const TriLaunchArgs*) {}
void tri_diag_front_plan(TriFramePlan& plan) {
    TriFramePlan q;
    q.n = 0;
    for (uint32_t i = 0; i < plan.n; ++i) {
        if (plan.k[i].stage == kStageRaster || (TRI_DIAG_FRONT == 3 && plan.k[i].stage == kStageVertex)) q.k[q.n++] = plan.k[i];
        else if (TRI_DIAG_FRONT == 2) q.k[q.n++] = TriKernelLaunch{reinterpret_cast<const void*>(k_diag_empty), dim3(1), dim3(64), kStageSetup};
    }
    plan = q;
}
#endif

hipError_t tri_run_plan(const TriFramePlan& plan, const TriLaunchArgs& args, TriLaunchArgs* d_args,
                        hipStream_t stream, hipEvent_t* ev, const TriIdArgs* id, hipEvent_t* id_ev,
                        const TriMotionArgs* motion, hipEvent_t* motion_ev) {
    hipError_t e = hipSuccess;
    bool setup_stamped = false;
    if (ev && (plan.n == 0 || plan.k[0].stage != kStageVertex)) (void)hipEventRecord(ev[kStageVertex], stream);
    for (uint32_t i = 0; i < plan.n; ++i) {
        const TriKernelLaunch& k = plan.k[i];
        if (ev && k.stage >= 0) {
            // stamps in the order the stages run; a frame without set-up still stamps it (zero length)
            if ((k.stage == kStageRaster || k.stage == kStageShadow) && !setup_stamped) {
                (void)hipEventRecord(ev[kStageSetup], stream);
                setup_stamped = true;
            }
            if (k.stage == kStageSetup) setup_stamped = true;
            (void)hipEventRecord(ev[k.stage], stream);
        }
        void* first[] = {const_cast<TriLaunchArgs*>(&args), &d_args};
        void* later[] = {&d_args};
        void* idp[] = {&d_args, const_cast<TriIdArgs*>(id)};  // the id pass: the published arguments, then its own
        if (k.stage == kStageId && !id) return hipErrorInvalidValue;
        if (k.stage == kStageId && id_ev) (void)hipEventRecord(id_ev[0], stream);
        void* mop[] = {const_cast<TriMotionArgs*>(motion)};  // the motion pass: its own arguments alone
        if (k.stage == kStageMotion && !motion) return hipErrorInvalidValue;
        if (k.stage == kStageMotion && motion_ev) (void)hipEventRecord(motion_ev[0], stream);
        // the frame's first kernel (k_vertex's stage) takes the arguments by value and publishes them
        void** kargs = k.stage == kStageVertex ? first : k.stage == kStageId ? idp : k.stage == kStageMotion ? mop : later;
        e = hipLaunchKernel(k.func, k.grid, k.block, kargs, 0, stream);
        if (e != hipSuccess) return e;
        if (k.stage == kStageId && id_ev) (void)hipEventRecord(id_ev[1], stream);
        if (k.stage == kStageMotion && motion_ev) (void)hipEventRecord(motion_ev[1], stream);
    }
    if (ev) (void)hipEventRecord(ev[kStageCount], stream);
    return hipGetLastError();
}

hipError_t tri_launch_blit(const uint32_t* src, int32_t w, int32_t h, uint32_t* dst, int32_t dw, int32_t dh,
                           const float* unorm_lut, hipStream_t stream) {
    if (w == dw && h == dh)  // u = x, v = y: both weights 0, and unorm8(b / 255) == b for every byte
        return hipMemcpyAsync(dst, src, (size_t)w * h * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
    const float sx = (float)w / (float)dw, sy = (float)h / (float)dh;
    const dim3 g((uint32_t)((dw + 63) / 64), (uint32_t)((dh + TRI_BLOCK / 64 - 1) / (TRI_BLOCK / 64)));
    hipLaunchKernelGGL(k_blit, g, dim3(TRI_BLOCK), 0, stream, src, w, h, dst, dw, dh, sx, sy, unorm_lut);
    return hipGetLastError();
}

#ifdef TRI_PHASE_TIMING
extern "C" int tri_debug_setup_times(unsigned long long* out, int nslots) {
    const size_t n = (size_t)(nslots < kPhaseSlots ? nslots : kPhaseSlots) * 4 * sizeof(unsigned long long);
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tri_setup_phase), n, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
