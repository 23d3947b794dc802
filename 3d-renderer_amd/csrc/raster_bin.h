// raster_bin.h — one bin of a k_raster* kernel (tile_raster_shade): coverage + early-Z in LDS with 64-bit (depth,
// primitive-order) keys (== in-order LESS_OR_EQUAL, Pipeline.cpp:655-658), then Default.frag:123-192 once per
// visible pixel, the skybox pass over the background, coalesced B8G8R8A8 + D32 stores. Included by the two units
// that define raster kernels: raster_kernels.hip (k_raster<.., true>, the shadow pre-pass's frames; the map raster
// shares the coverage helpers) and raster_plain.hip (every other frame).
//
// The fragment stage has two builds: EXACT (IEEE div/sqrt/powf, the oracle's operation order) and the default fast
// build (v_rcp/v_rsq/v_exp/v_log, hoisted frame constants), both within 1 LSB of the oracle's UNORM8 output.
//
// Parameter, defined by the includer: TRI_PK_SHADE — 1: the fast build's colour channels x, y as one packed-FP32
// pair (raster_kernels.hip: C5 k_raster 197.4 -> 195.8 us), 0: scalar channels with host-folded single-draw factors
// (raster_plain.hip, built without SLP vectorisation: C3 103.9 vs 105.7 us).
#pragma once
#include "raster_device.h"

#ifndef TRI_PK_SHADE
#error "raster_bin.h: define TRI_PK_SHADE (0 or 1) before the include"
#endif

// Tunables (numeric; -D overrides them for A/B builds).
// bbox∩bin pixels above which a triangle is rasterized by the whole workgroup (cooperatively):
// 32x32 bins 96 (64: C3 raster 119 -> 143 us; 160: unchanged), 16x16 bins 160 (96 -> 160: C2 raster
// 41.8 -> 35.7 us, C2 28.4k -> 33.3k fps)
#ifndef TRI_BIG_AREA
#define TRI_BIG_AREA 96
#endif
#ifndef TRI_BIG_AREA16
#define TRI_BIG_AREA16 160
#endif
// Wave priority of a 32x32 bin past its coverage (shading, stores); the start of the bin to the end of its coverage
// runs one above it (raster_bin). Above 0: above a concurrent frame's front end.
#ifndef TRI_RASTER_PRIO
#define TRI_RASTER_PRIO 0
#endif
// Large-triangle queue entries of the single-draw instantiation's 32x32 bins: the queue-position table's 3 KB come
// from this queue, so that 8 workgroups still fit the LDS; 192 entries rather than 384: a bin with more large
// triangles walks the rest per lane, C3 +0.3 %, same box
#ifndef TRI_QTAB_BIGN
#define TRI_QTAB_BIGN 192
#endif

namespace {

constexpr uint64_t kBgKey = 0x3F800001ull << 32;  // above every fragment key (depth bits <= 1.0 after the clamp)
constexpr float kPi = 3.14159265359f;                                  // Default.frag:65

// IEEE a / b for several numerators over one denominator. This is the compiler's own f32 division
// sequence (v_rcp, one Newton step on the reciprocal, two FMA corrections of the quotient: LLVM's
// LowerFDIV32) without its v_div_scale / v_div_fixup range handling, which changes nothing for finite
// normal operands whose exponents are far from the format's limits -- exact integers below 2^48, their
// ratios, depth differences and perspective weights. The refined reciprocal is computed once per
// denominator, so each further quotient costs a multiply and four FMAs instead of a full division, with
// the same bits.
struct RcpRef {
    float b, y;
};
__device__ __forceinline__ RcpRef rcp_ref(float b) {
    const float y0 = __builtin_amdgcn_rcpf(b);
    return RcpRef{b, __builtin_fmaf(__builtin_fmaf(-b, y0, 1.0f), y0, y0)};
}
__device__ __forceinline__ float div_rn(float a, const RcpRef& r) {
    const float q0 = a * r.y;
    const float q1 = __builtin_fmaf(__builtin_fmaf(-r.b, q0, a), r.y, q0);
    return __builtin_fmaf(__builtin_fmaf(-r.b, q1, a), r.y, q1);
}

// Workgroup barrier ordering LDS only (s_waitcnt lgkmcnt(0) + s_barrier): global loads issued before it stay
// in flight (__syncthreads' fence would wait for them too).
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_zero_id(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
// Inclusive prefix sum over the wave's lanes as a DPP scan: row_shr 1/2/4/8 inside each row of 16, then
// row_bcast:15 / :31 across rows (out-of-range sources add 0)
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) {
    v += dpp_zero_id<0x111>(v);
    v += dpp_zero_id<0x112>(v);
    v += dpp_zero_id<0x114>(v);
    v += dpp_zero_id<0x118>(v);
    v += dpp_zero_id<0x142, 0xa>(v);
    v += dpp_zero_id<0x143, 0xc>(v);
    return v;
}

// k_raster's gather sources: 16-B snaps, varyings, 48-B shade records. `src` holds an unclipped primitive's
// vertex attributes: the varyings, or with vary_obj the draw's own 36-B object-space records (vattr).
struct FetchBufs {
    RecBuf snap, vary, src, shade;
    const void* shade_base;  // the shade records for scalar loads (load_shade)
    uint32_t shade_bytes;
};
// obj48: the offset from draw d's vertex slots to its geometry vertices; a wave whose lanes share the draw (the
// common case) reads it with one scalar load
__device__ __forceinline__ uint32_t obj_delta(const TriFrameParams& fp, uint32_t d) {
    d = min(d, (uint32_t)TRI_OBJ48_DRAWS - 1u);
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
    if (__ballot(d != d0) == 0ull) return fp.vdelta[d0];
    return fp.vdelta[d];
}
// Frame kinds (k_raster_kind, include/tri_raster.h TRI_KIND_*): the fast single-draw instantiation with the
// frame-uniform switches its pixel loop would test as compile-time constants. KIND < 0 is the generic instantiation,
// which reads them from the frame's arguments; a kind's frames always carry object-space varyings (vary_obj).
constexpr int kKindGeneric = -1;
template <int KIND>
__device__ __forceinline__ bool kind_flag(uint32_t bit, bool runtime) {
    if constexpr (KIND >= 0) return ((uint32_t)KIND & bit) != 0u;
    else return runtime;
}
template <int KIND>
__device__ __forceinline__ bool kind_obj(const TriFrameParams& fp) {
    if constexpr (KIND >= 0) return true;
    else return obj_mode(fp);
}
template <bool ONE = false, int KIND = kKindGeneric>
__device__ __forceinline__ FetchBufs fetch_bufs(const TriFrameParams& fp, const TriDeviceBuffers& b) {
    FetchBufs f;
    f.snap = rec_buf(b.snap, 16u, fp.nslots);
    f.vary = rec_buf(b.vary, ONE ? 36u : 48u, (uint64_t)fp.nslots + fp.ovf_vert_cap);
    f.src = f.vary;
    if (ONE && kind_obj<KIND>(fp)) f.src = rec_buf(b.vattr + 9u * fp.vin_base, 36u, fp.nslots);
    // obj48: an unclipped primitive's vertices are its geometry's own 48-B input records (index slot + vdelta)
    if (!ONE && obj48_mode(fp)) f.src = rec_buf(b.vin, 48u, b.vertex_count);
    f.shade = rec_buf(b.draw_shade, (uint32_t)sizeof(TriDrawShade), fp.ndraws);
    f.shade_base = (const void*)b.draw_shade;
    f.shade_bytes = (uint32_t)sizeof(TriDrawShade) * fp.ndraws;
    return f;
}
__device__ __forceinline__ TriSnap ld_snap(const FetchBufs& fb, uint32_t slot) {
    const uint4 q = rec128<16>(fb.snap, slot, 0u);
    return TriSnap{(int32_t)q.x, (int32_t)q.y, __uint_as_float(q.z), __uint_as_float(q.w)};
}
// The fragment stage's view of a snapped vertex: X, Y and 1/w (12 bytes, one load; z is not needed).
__device__ __forceinline__ TriSnap ld_snap_xyw(const FetchBufs& fb, uint32_t slot) {
    const u32x3v q = rec96<16>(fb.snap, slot, 0u);
    return TriSnap{(int32_t)q[0], (int32_t)q[1], __uint_as_float(q[2]), 0.0f};
}

// ------------------------------------------------------------------------------------------
// tile_raster_shade: coverage
// ------------------------------------------------------------------------------------------
struct EdgeSetup {
    int32_t A[3], B[3];
    int64_t D[3];
    float dzdX, dzdY;
};

// Mirrors oracle setup_triangle()'s edge / depth-plane derivation.
__device__ __forceinline__ void edge_setup(const TriRec& r, EdgeSetup& e) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = k, j = (k + 1) % 3;
        const int32_t a = r.Y[i] - r.Y[j];
        const int32_t bb = r.X[j] - r.X[i];
        const int64_t c = -((int64_t)a * r.X[i] + (int64_t)bb * r.Y[i]);
        const bool tl = (a > 0) || (a == 0 && bb > 0);
        const int64_t cp = c + 128 * (int64_t)a + 128 * (int64_t)bb - (tl ? 0 : 1);
        e.A[k] = a;
        e.B[k] = bb;
        e.D[k] = cp >> 8;
    }
    const int64_t S = (int64_t)(r.X[1] - r.X[0]) * (int64_t)(r.Y[2] - r.Y[0]) -
                      (int64_t)(r.Y[1] - r.Y[0]) * (int64_t)(r.X[2] - r.X[0]);
    const float fX1 = (float)(r.X[1] - r.X[0]), fY1 = (float)(r.Y[1] - r.Y[0]);
    const float fX2 = (float)(r.X[2] - r.X[0]), fY2 = (float)(r.Y[2] - r.Y[0]);
    const float fS = (float)S;
    const float dz1 = r.z[1] - r.z[0], dz2 = r.z[2] - r.z[0];
    const RcpRef rS = rcp_ref(fS);
    e.dzdX = div_rn(dz1 * fY2 - dz2 * fY1, rS);
    e.dzdY = div_rn(dz2 * fX1 - dz1 * fX2, rS);
}

__device__ __forceinline__ int32_t clamp_edge(int64_t f, bool& reject) {
    constexpr int64_t kLim = (1ll << 30) - 1;
    if (f < -kLim) { reject = true; return -1; }
    return (int32_t)(f > kLim ? kLim : f);
}

__device__ __forceinline__ TriRec load_rec(const TriRec* recs, uint32_t i) {
    const uint4* p = reinterpret_cast<const uint4*>(recs + i);
    const uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];  // field by field: stays in registers
    TriRec r;
    r.X[0] = (int32_t)q0.x; r.X[1] = (int32_t)q0.y; r.X[2] = (int32_t)q0.z;
    r.Y[0] = (int32_t)q0.w; r.Y[1] = (int32_t)q1.x; r.Y[2] = (int32_t)q1.y;
    r.z[0] = __uint_as_float(q1.z); r.z[1] = __uint_as_float(q1.w); r.z[2] = __uint_as_float(q2.x);
    r.iw[0] = __uint_as_float(q2.y); r.iw[1] = __uint_as_float(q2.z); r.iw[2] = __uint_as_float(q2.w);
    r.prim_sub = q3.x;
    r.v[0] = q3.y; r.v[1] = q3.z; r.v[2] = q3.w;
    return r;
}

// The record setup_snapped produced for an unclipped primitive (v1 <-> v2 swapped), rebuilt from
// its snapped vertices instead of being stored and re-read.
__device__ __forceinline__ TriRec rec_from_snaps(uint32_t p, const uint32_t sl[3], const TriSnap& a0,
                                                 const TriSnap& a1, const TriSnap& a2) {
    TriRec r;
    r.X[0] = snap_X(a0); r.X[1] = snap_X(a2); r.X[2] = snap_X(a1);
    r.Y[0] = snap_Y(a0); r.Y[1] = snap_Y(a2); r.Y[2] = snap_Y(a1);
    r.z[0] = a0.z; r.z[1] = a2.z; r.z[2] = a1.z;
    r.iw[0] = a0.iw; r.iw[1] = a2.iw; r.iw[2] = a1.iw;
    r.v[0] = sl[0]; r.v[1] = sl[2]; r.v[2] = sl[1];
    r.prim_sub = p << 3;
    return r;
}

// The vertex slots and draw of primitive p: on a single-draw frame straight from the index buffer (slot =
// index - min_index, as k_setup computed them; k_setup writes no prim_vs then), else its prim_vs record.
// ONE (k_raster_plain's single-draw, 1x1-texture instantiation): fp.one_draw and fp.shade_solid are known
// to be set, so the other paths and their uniform flags compile away.
// IDX: the instantiation may take the index route (not the shadow pre-pass's kernels: the draw search cost the C5
// fragment stage 4 spilled VGPRs and 1.3 % of C5's frame rate, more than the records' writes it saves; the host
// keeps idx_route off on shadow frames)
template <bool ONE = false, bool IDX = true>
__device__ __forceinline__ void prim_slots(const TriFrameParams& fp, const TriDeviceBuffers& b, uint32_t p,
                                           uint32_t sl[3], uint32_t& d) {
    if (ONE || fp.one_draw) {
        const u32x3v q = rec96<12>(rec_buf(b.indices + fp.draw0.first_index, 12u, fp.nprims), p, 0u);
        sl[0] = q[0] - fp.draw0.min_index; sl[1] = q[1] - fp.draw0.min_index; sl[2] = q[2] - fp.draw0.min_index;
        d = 0;
    } else if (IDX && fp.idx_route) {  // (uniform) the index triple, the draw from the primitive bases
        const u32x3v q = rec96<12>(rec_buf(b.indices + fp.idx_k, 12u, fp.nprims), p, 0u);
        // the first active lane's draw by a scalar search; when every lane's primitive lies in it (a wave's pixels
        // are mostly one draw's) the draw and its slot offset stay scalar, else a compare-and-select per draw
        const uint32_t p0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)p);
        uint32_t d0 = 0;
        while (d0 + 1 < fp.ndraws && p0 >= fp.pbase[d0 + 1]) ++d0;
        const uint32_t hi = d0 + 1 < fp.ndraws ? fp.pbase[d0 + 1] : ~0u;
        uint32_t dd = d0, v = fp.vbd[d0];
        if (__ballot(p < fp.pbase[d0] || p >= hi) != 0ull) {
            dd = 0;
            v = fp.vbd[0];
            for (uint32_t i = 1; i < fp.ndraws; ++i) {  // uniform trip count, scalar operands
                const bool ge = p >= fp.pbase[i];
                dd = ge ? i : dd;
                v = ge ? fp.vbd[i] : v;
            }
        }
        sl[0] = q[0] + v; sl[1] = q[1] + v; sl[2] = q[2] + v;
        d = dd;
    } else {
        const uint4 pv = rec128<16>(rec_buf(b.prim_vs, 16u, fp.nprims), p, 0u);
        sl[0] = pv.x; sl[1] = pv.y; sl[2] = pv.z;
        d = pv.w & ~TRI_PRIM_CLIPPED;
    }
}

// A bin-queue entry -> its triangle (and the primitive's draw: 0 for a clipped entry, whose record names its slots).
template <bool ONE = false, bool IDX = true>
__device__ __forceinline__ TriRec load_entry_d(const TriFrameParams& fp, const TriDeviceBuffers& b, uint32_t e, uint32_t& d) {
    d = 0;
    if (e & TRI_ENTRY_CLIPPED) return load_rec(b.recs, e & ~TRI_ENTRY_CLIPPED);
    const FetchBufs fb = fetch_bufs(fp, b);
    uint32_t sl[3];
    prim_slots<ONE, IDX>(fp, b, e, sl, d);
    return rec_from_snaps(e, sl, ld_snap(fb, sl[0]), ld_snap(fb, sl[1]), ld_snap(fb, sl[2]));
}
template <bool ONE = false, bool IDX = true>
__device__ __forceinline__ TriRec load_entry(const TriFrameParams& fp, const TriDeviceBuffers& b, uint32_t e) {
    uint32_t d;
    return load_entry_d<ONE, IDX>(fp, b, e, d);
}

// Fragment depth at pixel centre: plane through the snapped vertices, fixed evaluation order.
__device__ __forceinline__ float frag_depth(const TriRec& r, const EdgeSetup& e, int32_t px, int32_t py) {
    const float fdx = (float)(256 * px + 128 - r.X[0]);
    const float fdy = (float)(256 * py + 128 - r.Y[0]);
    const float t1 = e.dzdX * fdx;
    const float t2 = e.dzdY * fdy;
    return (r.z[0] + t1) + t2;
}

// The far-plane test and the [0, 1] depth clamp on the float's bit pattern. Depth is finite here (the
// plane comes from snapped vertices with w >= WMIN and S != 0); non-negative floats order like their
// bits, and a negative depth (sign bit set, -0.0 included) clamps to +0.0 exactly like
// `if (!(z > 0)) z = 0`. One v_med3_i32 instead of two float compares and selects.
__device__ __forceinline__ bool depth_key(float z, bool far_clip, uint32_t lowbits, uint64_t& key) {
    const int32_t zb = __float_as_int(z);
    if (far_clip && zb > 0x3F800000) return false;  // per-pixel far-plane (z <= w) clip: z > 1
    key = ((uint64_t)(uint32_t)min(max(zb, 0), 0x3F800000) << 32) | lowbits;
    return true;
}

__device__ __forceinline__ void rec_bbox(const TriRec& r, int32_t ox, int32_t oy, int32_t bw, int32_t bh, int32_t& cx0,
                                         int32_t& cx1, int32_t& cy0, int32_t& cy1) {
    const int32_t xmin = min(r.X[0], min(r.X[1], r.X[2])), xmax = max(r.X[0], max(r.X[1], r.X[2]));
    const int32_t ymin = min(r.Y[0], min(r.Y[1], r.Y[2])), ymax = max(r.Y[0], max(r.Y[1], r.Y[2]));
    cx0 = max(-floor_shift8(128 - xmin), ox);
    cx1 = min(floor_shift8(xmax - 128), ox + bw - 1);
    cy0 = max(-floor_shift8(128 - ymin), oy);
    cy1 = min(floor_shift8(ymax - 128), oy + bh - 1);
}

__device__ __forceinline__ uint32_t key_low(uint32_t prim_sub) {
    return ((TRI_PRIM_MAX - (prim_sub >> 3)) << 3) | (prim_sub & 7u);
}

// The queue-position table (32x32 bins of the single-draw and the shadow instantiations, raster_bin's kQt): in a bin of
// at most kQtab entries on a frame of at most 2^20 primitives, a key's low word carries the winning entry's queue position as a payload BELOW its primitive order:
//   low = (kQPrimMax - prim) << 11 | sub << 8 | queue position
// so the minimum still resolves depth ties by primitive order exactly as key_low does (the position only separates
// entries of one primitive, which never share a pixel), and the fragment finds the entry's vertex slots in an LDS
// table the coverage pass filled, instead of gathering its index triple. No hash and no sort. The coverage code takes
// the record's prim_sub re-encoded so that key_low() of it yields this word (qenc).
// The shadow instantiation's table holds each entry's draw as a fourth word (its fragments then gather no 16-B
// prim_vs record).
constexpr uint32_t kQtab = 256, kQPrimMax = (1u << 20) - 1u;
__device__ __forceinline__ uint32_t qenc(uint32_t prim_sub, uint32_t qpos) {
    const uint32_t low = ((kQPrimMax - (prim_sub >> 3)) << 11) | ((prim_sub & 7u) << 8) | qpos;
    return (TRI_PRIM_MAX - (low >> 3)) << 3 | (low & 7u);  // key_low() of this is `low`
}

// Edge values at pixel (cx0, cy0) of the triangle's clipped bbox, the edge steps and the depth plane.
// A triangle under 64 px on a side (the common case) takes 32-bit arithmetic: |a|, |b| < 2^14 and every
// pixel centre of its bbox lies within 2^14 of each vertex, so a (Xc - Xi) + b (Yc - Yi) - bias fits int32
// and its floor division by 256 is the 64-bit form's A cx0 + B cy0 + D exactly (no clamp can trigger);
// the area is the same exact integer, so the depth plane gets the same floats. Returns false when the
// 64-bit form rejects the triangle.
__device__ __forceinline__ bool edge_start(const TriRec& r, int32_t cx0, int32_t cy0, int32_t A[3], int32_t B[3],
                                          int32_t F[3], float& dzdX, float& dzdY) {
    const int32_t xmin = min(r.X[0], min(r.X[1], r.X[2])), xmax = max(r.X[0], max(r.X[1], r.X[2]));
    const int32_t ymin = min(r.Y[0], min(r.Y[1], r.Y[2])), ymax = max(r.Y[0], max(r.Y[1], r.Y[2]));
    if (xmax - xmin < 16384 && ymax - ymin < 16384) {
        const int32_t Xc = 256 * cx0 + 128, Yc = 256 * cy0 + 128;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = k, j = (k + 1) % 3;
            const int32_t a = r.Y[i] - r.Y[j];
            const int32_t bb = r.X[j] - r.X[i];
            const bool tl = (a > 0) || (a == 0 && bb > 0);
            A[k] = a;
            B[k] = bb;
            F[k] = (__mul24(a, Xc - r.X[i]) + __mul24(bb, Yc - r.Y[i]) - (tl ? 0 : 1)) >> 8;
        }
        const int32_t X1 = r.X[1] - r.X[0], Y1 = r.Y[1] - r.Y[0], X2 = r.X[2] - r.X[0], Y2 = r.Y[2] - r.Y[0];
        const float fS = (float)(__mul24(X1, Y2) - __mul24(Y1, X2));
        const float fX1 = (float)X1, fY1 = (float)Y1, fX2 = (float)X2, fY2 = (float)Y2;
        const float dz1 = r.z[1] - r.z[0], dz2 = r.z[2] - r.z[0];
        const RcpRef rS = rcp_ref(fS);
        dzdX = div_rn(dz1 * fY2 - dz2 * fY1, rS);
        dzdY = div_rn(dz2 * fX1 - dz1 * fX2, rS);
        return true;
    }
    EdgeSetup e;
    edge_setup(r, e);
    bool rej = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[k] = e.A[k];
        B[k] = e.B[k];
        F[k] = clamp_edge((int64_t)e.A[k] * cx0 + (int64_t)e.B[k] * cy0 + e.D[k], rej);
    }
    dzdX = e.dzdX;
    dzdY = e.dzdY;
    return !rej;
}

// Rows cy0 + sub, cy0 + sub + step, ... of the bbox (sub < step: `step` lanes share a triangle). The
// row starts are stepped exactly (integer edge values; float offsets in multiples of 256), so any
// split gives the same keys as one lane walking every row.
template <int BL>
__device__ __forceinline__ void raster_serial(const TriRec& r, int32_t cx0, int32_t cx1, int32_t cy0, int32_t cy1,
                                              int32_t ox, int32_t oy, uint64_t* keys, int32_t sub = 0,
                                              int32_t step = 1) {
    struct {
        int32_t A[3], B[3];
        float dzdX, dzdY;
    } e;
    int32_t F[3];
    if (!edge_start(r, cx0, cy0, e.A, e.B, F, e.dzdX, e.dzdY)) return;
    const bool far_clip = (r.z[0] > 1.0f) || (r.z[1] > 1.0f) || (r.z[2] > 1.0f);
    const uint32_t low = key_low(r.prim_sub);
    // frag_depth's pixel offsets stepped incrementally: |256 p + 128 - X0| < 2^24, so the float steps
    // of 256 are exact and equal its int -> float conversions; same (z0 + dzdX dx) + dzdY dy order
    const float fdx0 = (float)(256 * cx0 + 128 - r.X[0]);
    float fdy = (float)(256 * (cy0 + sub) + 128 - r.Y[0]);
    uint32_t row = (uint32_t)(((cy0 + sub - oy) << BL) + (cx0 - ox));
#pragma unroll
    for (int k = 0; k < 3; ++k) F[k] += e.B[k] * sub;
    for (int32_t py = cy0 + sub; py <= cy1; py += step) {
        const float t2 = e.dzdY * fdy;
        int32_t f0 = F[0], f1 = F[1], f2 = F[2];
        float fdx = fdx0;
        const uint32_t rend = row + (uint32_t)(cx1 - cx0);
        for (uint32_t a = row; a <= rend; ++a) {
            if ((f0 | f1 | f2) >= 0) {
                uint64_t key;
                if (depth_key((r.z[0] + e.dzdX * fdx) + t2, far_clip, low, key)) atomicMin(&keys[a], key);
            }
            f0 += e.A[0]; f1 += e.A[1]; f2 += e.A[2];
            fdx += 256.0f;
        }
        F[0] += e.B[0] * step; F[1] += e.B[1] * step; F[2] += e.B[2] * step;
        fdy += 256.0f * (float)step;
        row += (uint32_t)step << BL;
    }
}

// Span walk (the per-lane path of 32x32 and 64x64 bins, triangles under 64 px on a side): each row's covered pixels
// are the integer x with f_k(x) = F_k + A_k (x - cx0) >= 0 for k = 0..2, an interval [L, R] found from the
// three crossings v_k = -F_k / A_k instead of testing every bbox pixel (the bbox of a C3 triangle is ~3x
// its area). Exact: with |A_k| < 2^14, |F_k| < 2^22 (exact in float, and stepped by B_k exactly) and v_rcp's 1-ulp
// reciprocal, t = fma(-F, 1/A, -/+delta) lies within 2^-16 of v -/+ delta for |v| <= 64, and a
// non-integer v is at least 1/|A| > 2^-14 from every integer, so with delta = 2^-15 ceil(t) = ceil(v) on
// the left (A > 0) and floor(t) = floor(v) on the right (A < 0), integer v included; crossings further
// than 64 px lie outside the bin either way, at 64-px bins too: x - cx0 runs over [0, wmax] with wmax <= 63, since
// cx0 >= the bin's first column, and the bounds on A_k and F_k come from the triangle's own box (under 64 px),
// not from the bin's (tests/test_raster_paths_gpu.py walks it at 64 px). A horizontal edge (A = 0) empties the row when F < 0
// (scale 2^100 on the left side). Then the same keys as raster_serial over [L, R] only.
template <int BL>
__device__ __forceinline__ void raster_span(const TriRec& r, int32_t cx0, int32_t cx1, int32_t cy0, int32_t cy1,
                                            int32_t ox, int32_t oy, uint64_t* keys, int32_t sub = 0,
                                            int32_t step = 1) {
    const int32_t xmin = min(r.X[0], min(r.X[1], r.X[2])), xmax = max(r.X[0], max(r.X[1], r.X[2]));
    const int32_t ymin = min(r.Y[0], min(r.Y[1], r.Y[2])), ymax = max(r.Y[0], max(r.Y[1], r.Y[2]));
    if (!(xmax - xmin < 16384 && ymax - ymin < 16384)) {
        raster_serial<BL>(r, cx0, cx1, cy0, cy1, ox, oy, keys, sub, step);
        return;
    }
    int32_t A[3], B[3], F[3];
    float dzdX, dzdY;
    edge_start(r, cx0, cy0, A, B, F, dzdX, dzdY);  // the 32-bit form: never rejects
    constexpr float kDelta = 0x1p-15f;
    float nrl[3], dl[3], nrr[3], dr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float rc = -__builtin_amdgcn_rcpf((float)A[k]);
        nrl[k] = A[k] > 0 ? rc : (A[k] == 0 ? -0x1p100f : 0.0f);
        dl[k] = A[k] >= 0 ? -kDelta : -INFINITY;
        nrr[k] = A[k] < 0 ? rc : 0.0f;
        dr[k] = A[k] < 0 ? kDelta : INFINITY;
    }
    const bool far_clip = (r.z[0] > 1.0f) || (r.z[1] > 1.0f) || (r.z[2] > 1.0f);
    const uint32_t low = key_low(r.prim_sub);
    const float wmax = (float)(cx1 - cx0);
    const int32_t fx0 = 256 * cx0 + 128 - r.X[0];
    float fdy = (float)(256 * (cy0 + sub) + 128 - r.Y[0]);
    uint32_t row = (uint32_t)(((cy0 + sub - oy) << BL) + (cx0 - ox));
    // the edge values stay exact integers below 2^22 over the bbox: stepped in float without rounding
    float Ff[3], Bs[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Ff[k] = (float)(F[k] + B[k] * sub);
        Bs[k] = (float)(B[k] * step);
    }
    for (int32_t py = cy0 + sub; py <= cy1; py += step) {
        const float f0 = Ff[0], f1 = Ff[1], f2 = Ff[2];
        const float tl = fmaxf(fmaxf(__builtin_fmaf(f0, nrl[0], dl[0]), __builtin_fmaf(f1, nrl[1], dl[1])),
                               __builtin_fmaf(f2, nrl[2], dl[2]));
        const float tr = fminf(fminf(__builtin_fmaf(f0, nrr[0], dr[0]), __builtin_fmaf(f1, nrr[1], dr[1])),
                               __builtin_fmaf(f2, nrr[2], dr[2]));
        const float Lf = fmaxf(ceilf(tl), 0.0f), Rf = fminf(floorf(tr), wmax);
        if (Lf <= Rf) {  // both in [0, wmax] here: the conversions are exact
            const int32_t L = (int32_t)Lf, R = (int32_t)Rf;
            const float t2 = dzdY * fdy;
            float fdx = (float)(fx0 + 256 * L);
            const uint32_t rend = row + (uint32_t)R;
            if (!far_clip) {  // (nearly every triangle: no per-pixel far-plane test)
                for (uint32_t a = row + (uint32_t)L; a <= rend; ++a) {
                    uint64_t key;
                    depth_key((r.z[0] + dzdX * fdx) + t2, false, low, key);
                    atomicMin(&keys[a], key);
                    fdx += 256.0f;
                }
            } else {
                for (uint32_t a = row + (uint32_t)L; a <= rend; ++a) {
                    uint64_t key;
                    if (depth_key((r.z[0] + dzdX * fdx) + t2, true, low, key)) atomicMin(&keys[a], key);
                    fdx += 256.0f;
                }
            }
        }
        Ff[0] += Bs[0]; Ff[1] += Bs[1]; Ff[2] += Bs[2];
        fdy += 256.0f * (float)step;
        row += (uint32_t)step << BL;
    }
}

// ------------------------------------------------------------------------------------------
// tile_raster_shade: Default.frag
// ------------------------------------------------------------------------------------------
struct f3 { float x, y, z; };
__device__ __forceinline__ f3 mk(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ f3 add(f3 a, f3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ f3 sub3(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ f3 mul(f3 a, f3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ f3 muls(f3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot3(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ f3 norm3(f3 v) { return muls(v, 1.0f / sqrtf(dot3(v, v))); }

// fast-path primitives (hardware v_rcp / v_rsq / v_exp / v_log, explicit FMA)
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float frsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float fdot(f3 a, f3 b) {
    return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x));
}
__device__ __forceinline__ f3 fnorm(f3 v) { return muls(v, frsq(fdot(v, v))); }
__device__ __forceinline__ float fpow(float x, float y) {  // x >= 0
    return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x));
}
__device__ __forceinline__ float sat(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

__device__ __forceinline__ uint32_t wrap_repeat(float f, uint32_t n) {  // REPEAT addressing of floor(f)
    const int32_t i = (int32_t)fminf(fmaxf(f, -1.0e9f), 1.0e9f);
    if ((n & (n - 1)) == 0) return (uint32_t)i & (n - 1);  // power-of-two size: the mask is the modulo
    int32_t r = i % (int32_t)n;                             // (two's complement: negative i wraps too)
    if (r < 0) r += (int32_t)n;
    return (uint32_t)r;
}

// The bilinear footprint of a texture / the shadow map as two 8-B row loads instead of four 4-B gathers (C5's
// fragment stage is bound by the texture units' data return, which costs per load instruction).
// Two adjacent 4-B texels as one 8-B load (4-B aligned: a dwordx2 load needs no more)
typedef uint32_t u32x2a __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ u32x2a ld_pair(TRI_G const uint32_t* p) { return *reinterpret_cast<TRI_G const u32x2a*>(p); }
// texture(): R8G8B8A8_SRGB decode before LINEAR filtering, REPEAT, level 0 (Renderer.cpp:3592-3607)
__device__ __forceinline__ float4 sample_tex(const TriTexDesc& t, float u0, float v0, const float* lut) {
    if (t.w == 1 && t.h == 1)  // 1x1 (the default white slot): all four taps are texel (0,0)
        return make_float4(t.solid[0], t.solid[1], t.solid[2], t.solid[3]);
    const float u = u0 * (float)t.w - 0.5f;
    const float v = v0 * (float)t.h - 0.5f;
    const float fu = floorf(u), fv = floorf(v);
    const float a = u - fu, bb = v - fv;
    const uint32_t x0 = wrap_repeat(fu, t.w), y0 = wrap_repeat(fv, t.h);
    const uint32_t x1 = (x0 + 1 == t.w) ? 0u : x0 + 1, y1 = (y0 + 1 == t.h) ? 0u : y0 + 1;
    TRI_G const uint32_t* tx = (TRI_G const uint32_t*)t.texels;  // device texture memory (global loads)
    uint32_t p00, p10, p01, p11;
    if (x1 == x0 + 1) {  // the two taps of a row are adjacent: one 8-B load per row
        const u32x2a r0 = ld_pair(tx + y0 * t.w + x0), r1 = ld_pair(tx + y1 * t.w + x0);
        p00 = r0.x; p10 = r0.y; p01 = r1.x; p11 = r1.y;
    } else {  // REPEAT wrapped x1 to column 0
        p00 = tx[y0 * t.w + x0]; p10 = tx[y0 * t.w + x1];
        p01 = tx[y1 * t.w + x0]; p11 = tx[y1 * t.w + x1];
    }
    float4 r;
    float* rp = &r.x;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        auto ch = [&](uint32_t px) -> float {
            const uint32_t by = (px >> (8 * c)) & 0xFFu;
            return lut[c == 3 ? 256 + by : by];
        };
        const float t00 = ch(p00), t10 = ch(p10), t01 = ch(p01), t11 = ch(p11);
        const float l0 = t00 + a * (t10 - t00);
        const float l1 = t01 + a * (t11 - t01);
        rp[c] = l0 + bb * (l1 - l0);
    }
    return r;
}

// Fast build's tone curve output (Default.frag:185-189 then the UNORM8 store): the channel comes back
// already scaled by 255 — 255 t^(1/2.2) as one exp2 with log2(255) folded into its argument (t = c / (c + 1)
// lies in [0, 1), so no clamp is needed), within a small fraction of an LSB of the IEEE value before rounding.
__device__ __forceinline__ float tone_out(float t) {
    constexpr float g = 1.0f / 2.2f;
    return __builtin_amdgcn_exp2f(__builtin_fmaf(g, __builtin_amdgcn_logf(t), 7.99435343685886f));
}
// The fast build's BGRA8 word from tone_out's channels (in [0, 255]) and the alpha byte:
// v_cvt_pk_u8_f32 rounds each channel to nearest (ties to even: it differs from floor(v + 0.5) only on an
// exact .5, inside the 1-LSB bar) and inserts it into its byte — one instruction per channel instead of a
// round, a conversion and a shift/or.
__device__ __forceinline__ uint32_t fast_bgra(float r, float g, float b, uint32_t a8) {
    return __builtin_amdgcn_cvt_pk_u8_f32(r, 2u, __builtin_amdgcn_cvt_pk_u8_f32(g, 1u, __builtin_amdgcn_cvt_pk_u8_f32(b, 0u, a8 << 24)));
}

struct __attribute__((aligned(16))) V4 {
    float x, y, z, w;
};

struct Frag {  // flat scalars: nested f3 members are ABI-coerced and defeat SROA in the pair path
    float wx, wy, wz;  // world position
    float nx, ny, nz;  // interpolated normal
    float cx, cy, cz;  // vertex colour
    float u, v;
    float sx, sy, sz, sw;  // sampled texel (linear rgb, alpha)
    float tx, ty, tz, tw;  // draw tint
    float vis;             // shadow pre-pass: fraction of the sun's light reaching the fragment (1 without it)
};
__device__ __forceinline__ f3 fworld(const Frag& f) { return mk(f.wx, f.wy, f.wz); }
__device__ __forceinline__ f3 fnrm(const Frag& f) { return mk(f.nx, f.ny, f.nz); }
__device__ __forceinline__ f3 fvcol(const Frag& f) { return mk(f.cx, f.cy, f.cz); }
__device__ __forceinline__ f3 ftex(const Frag& f) { return mk(f.sx, f.sy, f.sz); }
__device__ __forceinline__ f3 ftint(const Frag& f) { return mk(f.tx, f.ty, f.tz); }

// Default.frag's max(x, 0.0) is "0.0 if x < 0.0, otherwise x", which keeps a NaN, where fmaxf (v_max_f32) drops it. A
// fragment whose N.V is NaN (an interpolated normal that cannot be normalised: normalize(0) of a vertex that no bone
// skins, reaching a pixel through a clipped sliver) gets a NaN from every light Default.frag evaluates: the sun if
// there is one, whatever its visibility, and each point light farther than 1e-4, whatever its range. The colour is
// then NaN and the UNORM store writes 0. True when some light is evaluated for a fragment at wp.
__device__ __forceinline__ bool nan_reaches_colour(const TriShadeConst& sc, f3 wp) {
    bool lit = sc.has_sun != 0u;
    for (uint32_t i = 0; i < sc.npt && !lit; ++i) {
        const f3 to = sub3(mk(sc.pl[i].pos[0], sc.pl[i].pos[1], sc.pl[i].pos[2]), wp);
        lit = !(sqrtf(dot3(to, to)) <= 1e-4f);
    }
    return lit;
}

// ---- EXACT build: Default.frag with IEEE div/sqrt/powf in the oracle's operation order ----------
__device__ __forceinline__ float schlick_ggx(float NdotV, float roughness) {
    const float r = roughness + 1.0f;
    const float k = (r * r) / 8.0f;
    const float denom = NdotV * (1.0f - k) + k;
    return NdotV / fmaxf(denom, 1e-4f);
}

__device__ __forceinline__ f3 eval_pbr_exact(f3 L, f3 rad, f3 N, f3 V, f3 albedo, float metallic, float roughness,
                                             f3 F0) {
    const f3 H = norm3(add(V, L));
    const float a = roughness * roughness;
    const float a2 = a * a;
    const float NdotH = fmaxf(dot3(N, H), 0.0f);
    const float NdotH2 = NdotH * NdotH;
    const float dd = (NdotH2 * (a2 - 1.0f) + 1.0f);
    const float NDF = a2 / ((kPi * dd) * dd);
    const float NdotV = fmaxf(dot3(N, V), 0.0f);
    const float NdotL = fmaxf(dot3(N, L), 0.0f);
    const float G = schlick_ggx(NdotL, roughness) * schlick_ggx(NdotV, roughness);
    const float p = powf(sat(1.0f - fmaxf(dot3(H, V), 0.0f)), 5.0f);
    const f3 F = mk(F0.x + (1.0f - F0.x) * p, F0.y + (1.0f - F0.y) * p, F0.z + (1.0f - F0.z) * p);
    const f3 num = muls(F, NDF * G);
    const float den = fmaxf((4.0f * NdotV) * NdotL, 1e-4f);
    const f3 spec = mk(num.x / den, num.y / den, num.z / den);
    const f3 kD = muls(mk(1.0f - F.x, 1.0f - F.y, 1.0f - F.z), 1.0f - metallic);
    const f3 diff = mk((kD.x * albedo.x) / kPi, (kD.y * albedo.y) / kPi, (kD.z * albedo.z) / kPi);
    return muls(mul(add(diff, spec), rad), NdotL);
}

__device__ __forceinline__ float4 fs_exact(const TriFrameParams& fp, const Frag& f) {
    const tri_global_ubo& g = fp.ubo;
    const tri_material_record& mat = fp.mat0;
    const f3 N = norm3(norm3(fnrm(f)));
    const f3 V = norm3(sub3(mk(g.camera_position[0], g.camera_position[1], g.camera_position[2]), fworld(f)));
    const f3 albedo = mul(mul(mul(ftex(f), mk(mat.base_color_factor[0], mat.base_color_factor[1],
                                                               mat.base_color_factor[2])),
                              ftint(f)),
                          fvcol(f));
    const float metallic = sat(mat.material_factors[0]);
    const float roughness = fminf(fmaxf(mat.material_factors[1], 0.045f), 1.0f);
    const float amb_s = sat(mat.material_factors[2]);
    const float om = 0.04f * (1.0f - metallic);
    const f3 F0 = mk(om + albedo.x * metallic, om + albedo.y * metallic, om + albedo.z * metallic);
    f3 direct = mk(0.f, 0.f, 0.f);
    if (g.light_counts[0] > 0u) {
        const f3 L = norm3(mk(-g.directional_light_direction[0], -g.directional_light_direction[1],
                              -g.directional_light_direction[2]));
        const f3 rad = muls(muls(mk(g.directional_light_color[0], g.directional_light_color[1], g.directional_light_color[2]),
                                 g.directional_light_color[3]),
                            f.vis);
        direct = add(direct, eval_pbr_exact(L, rad, N, V, albedo, metallic, roughness, F0));
    }
    const uint32_t np = min(g.light_counts[1], 8u);
    for (uint32_t i = 0; i < np; ++i) {
        const tri_point_light& pl = g.point_lights[i];
        const f3 to = sub3(mk(pl.position_range[0], pl.position_range[1], pl.position_range[2]), fworld(f));
        const float dist = sqrtf(dot3(to, to));
        if (dist <= 1e-4f) continue;
        const f3 L = mk(to.x / dist, to.y / dist, to.z / dist);
        const float radius = fmaxf(pl.position_range[3], 1e-4f);
        const float nd = sat(dist / radius);
        float att = 1.0f - nd;
        att = att * att;
        const f3 rad = muls(muls(mk(pl.color_intensity[0], pl.color_intensity[1], pl.color_intensity[2]),
                                 pl.color_intensity[3]),
                            att);
        direct = add(direct, eval_pbr_exact(L, rad, N, V, albedo, metallic, roughness, F0));
    }
    const f3 amb = muls(mul(muls(mk(g.ambient_color_intensity[0], g.ambient_color_intensity[1],
                                    g.ambient_color_intensity[2]),
                                 g.ambient_color_intensity[3]),
                            albedo),
                        amb_s);
    f3 col = add(amb, direct);
    const float NdotV = dot3(N, V);
    if (NdotV != NdotV && nan_reaches_colour(fp.sc, fworld(f))) col.x = col.y = col.z = NdotV;  // NaN: stored as 0
    col = mk(col.x / (col.x + 1.0f), col.y / (col.y + 1.0f), col.z / (col.z + 1.0f));
    const float gamma = 1.0f / 2.2f;
    col = mk(powf(col.x, gamma), powf(col.y, gamma), powf(col.z, gamma));
    const float alpha = (mat.base_color_factor[3] * f.tw) * f.sw;
    return make_float4(col.x, col.y, col.z, alpha);
}

// ---- fast build: same algebra, frame constants hoisted, hardware transcendental approximations ---
// Per light: one v_rsq (half vector) and ONE v_rcp for NDF * G_L / (4 NdotV NdotL) together. For unit
// V and L, |V + L|^2 = 2 + 2 L.V, N.H = (N.V + N.L) / |V + L| and H.V = (1 + L.V) / |V + L|.
// G_V NdotL / max(4 NdotV NdotL, 1e-4) (the NDF's a2 / pi and G_L's 1 / (1 - k) folded in), the part of the
// specular weight before the per-light denominator dd^2 gden. For N.L > 0,
// NdotL / max(4 NdotV NdotL, 1e-4) = min(1 / (4 NdotV), 1e4 NdotL), so with spA = gVa / (4 NdotV) (formed
// without NdotV: a2 / (4 pi (1 - k) gden_V), finite at NdotV = 0) and spB = 1e4 gVa it is min(spA, spB NdotL):
// two operations per light instead of four, and one product fewer inside the reciprocal. Both
// operands are non-negative and not NaN (spA > 0; spB >= 0 and N.L > 0 here), so their minimum is the integer
// minimum of their bits — v_min_i32, which needs no canonicalising v_max of spA in every light as the
// IEEE-mode v_min_f32 does.
__device__ __forceinline__ float spec_num(float spA, float spB, float NdotL) {
    return __int_as_float(min(__float_as_int(spA), __float_as_int(spB * NdotL)));
}
// Point-light attenuation (1 - min(d / r, 1))^2's base, max(1 - d / r, 0) as one fma
__device__ __forceinline__ float att_base(float d, float ir) { return fmaxf(__builtin_fmaf(-d, ir, 1.0f), 0.0f); }

struct PbrPix {
    f3 N, V, F0, omF0, diffK;
    float NdotVr;   // unclamped N.V
    float spA, spB; // spec_num's per-pixel factors
};

// One light with unclamped N.L and L.V given (the caller forms them without normalising L first).
__device__ __forceinline__ void eval_pbr_fast(float a2m1, float kgo, const PbrPix& px, float NdotLr, float LdotV,
                                              f3 rad, float scale, f3& c) {  // a2m1, kgo: TriShadeConst's
#pragma clang fp contract(fast)  // fast build only: FMA contraction is inside the 1-LSB budget
    // N.L <= 0 makes the light's weight 0 and every term finite: c + X * 0 == c exactly, so a wave
    // whose lanes all face away skips the rest (Default.frag evaluates it to the same zero)
    if (!(NdotLr > 0.0f)) return;
    const float ih = frsq(fmaxf(__builtin_fmaf(2.0f, LdotV, 2.0f), 1e-30f));
    const float NdotH = fmaxf((px.NdotVr + NdotLr) * ih, 0.0f);
    const float NdotL = NdotLr;  // > 0 here: max(N.L, 0) is the identity
    const float dd = __builtin_fmaf(NdotH * NdotH, a2m1, 1.0f);
    // Default.frag's max(., 1e-4) on G_L's denominator is the identity here: N.L > 0 and k = (r + 1)^2 / 8
    // >= 0.136 for roughness >= 0.045, so N.L (1 - k) + k >= k
    const float gden = NdotL + kgo;  // G_L's denominator divided through by 1 - k (sc.a2pio carries 1 / (1 - k))
    // NDF * G_L * G_V / den with NDF = a2 / (pi dd^2), G_L = NdotL / gden
    const float sp = spec_num(px.spA, px.spB, NdotL) * frcp((dd * dd) * gden);
    // 1 - max(H.V, 0), clamped to [0, 1]: one clamped subtract
    const float q = sat(1.0f - __builtin_fmaf(LdotV, ih, ih));
    const float q2 = q * q;
    const float p5 = q2 * q2 * q;
    const float w = NdotL * scale;
    // (kD albedo / pi + F s) = diffK + F (s - diffK), F = F0 + (1 - F0) p5
    c.x = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(px.omF0.x, p5, px.F0.x), sp - px.diffK.x, px.diffK.x), rad.x * w, c.x);
    c.y = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(px.omF0.y, p5, px.F0.y), sp - px.diffK.y, px.diffK.y), rad.y * w, c.y);
    c.z = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(px.omF0.z, p5, px.F0.z), sp - px.diffK.z, px.diffK.z), rad.z * w, c.z);
}

// ONE: the texel, base colour and tint are uniform and their product is a kernel argument (sc.sbt)
// TRI_PK_SHADE (the includer's, see the top of the file): packed colour pairs for the shadow instantiation, scalar
// channels for k_raster_plain.
#if TRI_PK_SHADE
// Colour channels x, y as one packed-FP32 pair (v_pk_fma_f32 / v_pk_mul_f32: two IEEE operations per
// instruction, the same bits as the scalar form) and z on its own; written out by hand, not left to the SLP
// vectoriser, so that only these values occupy register pairs (raster_plain.hip is built without SLP).
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2v pk_fma(f2v a, f2v b, f2v c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2v splat(float x) { return f2v{x, x}; }
struct PbrPixP {
    f3 N, V;
    f2v F0xy, omF0xy, diffKxy;
    float F0z, omF0z, diffKz;
    float NdotVr;
    float spA, spB;
};
__device__ __forceinline__ void eval_pbr_fast_p(const TriShadeConst& sc, const PbrPixP& px, float NdotLr, float LdotV,
                                                f2v radxy, float radz, float scale, f2v& cxy, float& cz) {
#pragma clang fp contract(fast)
    if (!(NdotLr > 0.0f)) return;  // (see eval_pbr_fast)
    const float ih = frsq(fmaxf(__builtin_fmaf(2.0f, LdotV, 2.0f), 1e-30f));
    const float NdotH = fmaxf((px.NdotVr + NdotLr) * ih, 0.0f);
    const float NdotL = NdotLr;
    const float dd = __builtin_fmaf(NdotH * NdotH, sc.a2m1, 1.0f);
    // Default.frag's max(., 1e-4) on G_L's denominator is the identity here: N.L > 0 and k = (r + 1)^2 / 8
    // >= 0.136 for roughness >= 0.045, so N.L (1 - k) + k >= k
    const float gden = NdotL + sc.kgo;
    const float sp = spec_num(px.spA, px.spB, NdotL) * frcp((dd * dd) * gden);
    const float q = sat(1.0f - __builtin_fmaf(LdotV, ih, ih));
    const float q2 = q * q;
    const float p5 = q2 * q2 * q;
    const float w = NdotL * scale;
    cxy = pk_fma(pk_fma(pk_fma(px.omF0xy, splat(p5), px.F0xy), splat(sp) - px.diffKxy, px.diffKxy), radxy * splat(w), cxy);
    cz = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(px.omF0z, p5, px.F0z), sp - px.diffKz, px.diffKz), radz * w, cz);
}
#endif

// The scalar form's single-draw solid frames shade from the vertex colour with host-folded factors (TriShadeConst::
// sbtm / sbtkd / sbtamb), never forming the albedo (-6 VALU per pixel).
// One point light's 32-B record as one scalar load
typedef float f8v __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f8v ld_light(const TriShadeConst& sc, uint32_t i) {
    return *reinterpret_cast<const f8v*>(sc.pl[i].pos);
}
// KIND (frame kinds): the sun and the point lights are compile-time on or off; each light's record is loaded while
// the light before it is evaluated.
template <bool ONE = false, int KIND = kKindGeneric>
__device__ __forceinline__ float4 fs_fast(const TriShadeConst& sc, const Frag& f, uint32_t npt_k = 0u) {
#pragma clang fp contract(fast)
#if TRI_PK_SHADE
    PbrPixP px;
    px.N = fnorm(fnrm(f));
    px.V = fnorm(sub3(mk(sc.cam[0], sc.cam[1], sc.cam[2]), fworld(f)));
    f2v albxy;
    float albz;
    if (ONE) {
        albxy = f2v{sc.sbt[0], sc.sbt[1]} * f2v{f.cx, f.cy};
        albz = sc.sbt[2] * f.cz;
    } else {
        albxy = ((f2v{f.sx, f.sy} * f2v{sc.base[0], sc.base[1]}) * f2v{f.tx, f.ty}) * f2v{f.cx, f.cy};
        albz = ((f.sz * sc.base[2]) * f.tz) * f.cz;
    }
    const float m = sc.metallic;
    const float om = sc.om;
    px.F0xy = pk_fma(albxy, splat(m), splat(om));
    px.F0z = __builtin_fmaf(albz, m, om);
    px.omF0xy = splat(1.0f) - px.F0xy;
    px.omF0z = 1.0f - px.F0z;
    const float kd = sc.kd;
    px.diffKxy = albxy * splat(kd);
    px.diffKz = albz * kd;
    px.NdotVr = fdot(px.N, px.V);
    const float NdotV = fmaxf(px.NdotVr, 0.0f);
    const float rgV = frcp(fmaxf(__builtin_fmaf(NdotV, sc.omkg, sc.kg), 1e-4f));
    px.spA = sc.spAk * rgV;                   // 0.25 a2 / pi / (1 - k) / max(G_V's denominator, 1e-4)
    px.spB = sc.spBk * (NdotV * rgV);         // 1e4 a2 / pi * G_V / (1 - k)
    f2v cxy = (f2v{sc.amb[0], sc.amb[1]} * albxy) * splat(sc.amb_strength);
    float cz = (sc.amb[2] * albz) * sc.amb_strength;
    if (kAblate & 64) return make_float4(cxy.x, cxy.y, cz, 1.0f);  // diagnostics: 64 = no lights
    if (sc.has_sun && f.vis > 0.0f) {  // vis = 0 (fully shadowed): the sun adds exactly nothing
        const f3 L = mk(sc.sun_l[0], sc.sun_l[1], sc.sun_l[2]);
        eval_pbr_fast_p(sc, px, fdot(px.N, L), fdot(L, px.V), f2v{sc.sun_rad[0], sc.sun_rad[1]}, sc.sun_rad[2], f.vis,
                        cxy, cz);
    }
    const f3 wp = fworld(f);
    for (uint32_t i = 0; i < sc.npt; ++i) {
        const f3 to = sub3(mk(sc.pl[i].pos[0], sc.pl[i].pos[1], sc.pl[i].pos[2]), wp);
        const float d2 = fdot(to, to);
        const float inv = frsq(d2);
        const float att0 = att_base(d2 * inv, sc.pl[i].pos[3]);
        if (!(d2 > 1e-8f && att0 > 0.0f)) continue;  // dist <= 1e-4, or beyond the range (see below)
        eval_pbr_fast_p(sc, px, fdot(px.N, to) * inv, fdot(to, px.V) * inv, f2v{sc.pl[i].rad[0], sc.pl[i].rad[1]},
                        sc.pl[i].rad[2], att0 * att0, cxy, cz);
    }
    if (__builtin_expect(__ballot(px.NdotVr != px.NdotVr) != 0ull, 0)) {  // (see below)
        if (px.NdotVr != px.NdotVr && nan_reaches_colour(sc, wp)) { cxy = splat(0.0f); cz = 0.0f; }
    }
    const f2v c1 = cxy + splat(1.0f);
    const f2v txy = cxy * f2v{frcp(c1.x), frcp(c1.y)};
    const float tz = cz * frcp(cz + 1.0f);
    return make_float4(tone_out(txy.x), tone_out(txy.y), tone_out(tz), ONE ? sc.sbt[3] : (sc.base[3] * f.tw) * f.sw);
#else
    PbrPix px;
    px.N = fnorm(fnrm(f));
    px.V = fnorm(sub3(mk(sc.cam[0], sc.cam[1], sc.cam[2]), fworld(f)));
    const float m = sc.metallic;
    const float om = sc.om;  // 0.04 (1 - metallic), folded on the host with the other frame constants
    f3 c;
    if (ONE) {  // albedo = sbt * colour: every term from the colour and a folded factor (TriShadeConst::sbtm)
        const f3 col = fvcol(f);
        px.F0 = mk(__builtin_fmaf(col.x, sc.sbtm[0], om), __builtin_fmaf(col.y, sc.sbtm[1], om),
                   __builtin_fmaf(col.z, sc.sbtm[2], om));
        px.diffK = mul(col, mk(sc.sbtkd[0], sc.sbtkd[1], sc.sbtkd[2]));
        c = mul(col, mk(sc.sbtamb[0], sc.sbtamb[1], sc.sbtamb[2]));
    } else {
        const f3 albedo = mul(mul(mul(ftex(f), mk(sc.base[0], sc.base[1], sc.base[2])), ftint(f)), fvcol(f));
        px.F0 = mk(__builtin_fmaf(albedo.x, m, om), __builtin_fmaf(albedo.y, m, om), __builtin_fmaf(albedo.z, m, om));
        px.diffK = muls(albedo, sc.kd);
        c = mk(sc.amb[0] * albedo.x * sc.amb_strength, sc.amb[1] * albedo.y * sc.amb_strength,
               sc.amb[2] * albedo.z * sc.amb_strength);
    }
    px.omF0 = mk(1.0f - px.F0.x, 1.0f - px.F0.y, 1.0f - px.F0.z);
    px.NdotVr = fdot(px.N, px.V);
    const float NdotV = fmaxf(px.NdotVr, 0.0f);
    const float rgV = frcp(fmaxf(__builtin_fmaf(NdotV, sc.omkg, sc.kg), 1e-4f));
    px.spA = sc.spAk * rgV;                   // 0.25 a2 / pi / (1 - k) / max(G_V's denominator, 1e-4)
    px.spB = sc.spBk * (NdotV * rgV);         // 1e4 a2 / pi * G_V / (1 - k)
    if (kAblate & 64) return make_float4(c.x, c.y, c.z, 1.0f);  // diagnostics: 64 = no lights
    // A kind reads the lights' uniform terms where the fragment's other constants are read, ahead of the lanes' skip
    // tests (behind a skip each would be a scalar load and a wait of its own): the empty asm pins them there.
    float a2m1 = sc.a2m1, kgo = sc.kgo;
    f3 srad = mk(sc.sun_rad[0], sc.sun_rad[1], sc.sun_rad[2]);
    f8v nxt{};  // the next point light's record
    if constexpr (KIND >= 0) {
        asm volatile("" : "+s"(a2m1), "+s"(kgo));
        if constexpr ((KIND & TRI_KIND_SUN) != 0) asm volatile("" : "+s"(srad.x), "+s"(srad.y), "+s"(srad.z));
        // (the first light's record is not pinned there with them: its eight SGPRs across the sun's evaluation
        // made the compiler read the other constants a few at a time, each behind a wait of its own)
        if constexpr ((KIND & TRI_KIND_LIGHTS) != 0) nxt = ld_light(sc, 0);  // (at least one light)
    }
    if (kind_flag<KIND>(TRI_KIND_SUN, sc.has_sun) && f.vis > 0.0f) {  // vis = 0 (fully shadowed): the sun adds exactly nothing
        const f3 L = mk(sc.sun_l[0], sc.sun_l[1], sc.sun_l[2]);
        eval_pbr_fast(a2m1, kgo, px, fdot(px.N, L), fdot(L, px.V), srad, f.vis, c);
    }
    const f3 wp = fworld(f);
    // (a kind's light count is read once per workgroup, ahead of the pixel loop: npt_k)
    const uint32_t npt = KIND >= 0 ? (kind_flag<KIND>(TRI_KIND_LIGHTS, false) ? npt_k : 0u) : sc.npt;
    for (uint32_t i = 0; i < npt; ++i) {
        float lp[8];
        if (KIND >= 0) {  // this light's record was loaded a light ahead; the last light loads itself again (no branch)
#pragma unroll
            for (int k = 0; k < 8; ++k) lp[k] = nxt[k];
            nxt = ld_light(sc, min(i + 1u, (uint32_t)TRI_MAX_POINT_LIGHTS - 1u));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) { lp[k] = sc.pl[i].pos[k]; lp[4 + k] = sc.pl[i].rad[k]; }
        }
        const f3 to = sub3(mk(lp[0], lp[1], lp[2]), wp);
        const float d2 = fdot(to, to);
        const float inv = frsq(d2);
        const float att0 = att_base(d2 * inv, lp[3]);
        // dist <= 1e-4 (Default.frag skips it; d2 = 0 gives att0 = 0 here too), or beyond the light's
        // range: (1 - d/r)^2 = 0 adds exactly nothing. One exact skip instead of two.
        if (!(d2 > 1e-8f && att0 > 0.0f)) continue;
        // L = to / |to| is never formed: N.L and L.V are the dot products with `to`, scaled once
        eval_pbr_fast(a2m1, kgo, px, fdot(px.N, to) * inv, fdot(to, px.V) * inv, mk(lp[4], lp[5], lp[6]), att0 * att0, c);
    }
    // A NaN colour in Default.frag (nan_reaches_colour) is stored as 0: so is a zero colour here (tone_out(0) = 0). The
    // test is wave-uniform, so a wave without such a fragment pays one compare and a scalar branch.
    if (__builtin_expect(__ballot(px.NdotVr != px.NdotVr) != 0ull, 0)) {
        if (px.NdotVr != px.NdotVr && nan_reaches_colour(sc, wp)) c = mk(0.0f, 0.0f, 0.0f);
    }
    const f3 t = mk(c.x * frcp(c.x + 1.0f), c.y * frcp(c.y + 1.0f), c.z * frcp(c.z + 1.0f));
    return make_float4(tone_out(t.x), tone_out(t.y), tone_out(t.z), ONE ? sc.sbt[3] : (sc.base[3] * f.tw) * f.sw);
#endif
}

// fs_fast's own test again, for the AI blend (which must not mix a colour that Default.frag has as NaN)
__device__ __forceinline__ bool fs_fast_nan(const TriShadeConst& sc, const Frag& f) {
#pragma clang fp contract(fast)
    const float NdotV = fdot(fnorm(fnrm(f)), fnorm(sub3(mk(sc.cam[0], sc.cam[1], sc.cam[2]), fworld(f))));
    return NdotV != NdotV && nan_reaches_colour(sc, fworld(f));
}

__device__ __forceinline__ float interp_exact(float w0, float w1, float w2, float x0, float x1, float x2) {
    return (w0 * x0 + w1 * x1) + w2 * x2;  // the oracle's order, no contraction
}
__device__ __forceinline__ float interp_fast(float w0, float w1, float w2, float x0, float x1, float x2) {
    return __builtin_fmaf(w2, x2, __builtin_fmaf(w1, x1, w0 * x0));
}

// Fast build's perspective-correct weights from the pixel-centre offsets (dx, dy) to vertex 0: the three
// edge functions at the pixel, e0 = S + (y1 - y2) dx + (x2 - x1) dy, e1 = y2 dx - x2 dy, e2 = x1 dy - y1 dx
// (S the exact doubled area, so e0 + e1 + e2 = S), weighted by 1/w: q_k = e_k iw_k, w_k = q_k / (q0 + q1 + q2).
// This is the barycentric form scaled by S iw0, which cancels in the normalisation, so the only reciprocal is
// that of the sum (no 1/S, no 1/iw0). e0 is formed about vertex 1, e0 = (x2 - x1)(dy - y1) - (y2 - y1)(dx - x1)
// (the same function: its constant term is S), so no area product is needed. Every offset is an exact
// integer below 2^24 inside the guard band, converted once. Relative to the triangle's own vertices, not to a
// bin: every bin, band and code path gives a pixel the same bits.
__device__ __forceinline__ void fast_weights(const TriRec& r, int32_t px, int32_t py, float& w0, float& w1, float& w2) {
    const int32_t x1 = r.X[1] - r.X[0], y1 = r.Y[1] - r.Y[0], x2 = r.X[2] - r.X[0], y2 = r.Y[2] - r.Y[0];
    const float fx1 = (float)x1, fy1 = (float)y1, fx2 = (float)x2, fy2 = (float)y2;
    const int32_t idx = 256 * px + 128 - r.X[0], idy = 256 * py + 128 - r.Y[0];
    const float dx = (float)idx, dy = (float)idy;
    const float e1 = __builtin_fmaf(-fx2, dy, fy2 * dx);
    const float e2 = __builtin_fmaf(fx1, dy, -fy1 * dx);
    // e0 = S - e1 - e2 with the area in float (a weight then carries an absolute error of a few 2^-24, far
    // inside the colour bar; depth never uses these weights)
    const float e0 = (__builtin_fmaf(fx1, fy2, -fy1 * fx2) - e1) - e2;
    const float q0 = e0 * r.iw[0], q1 = e1 * r.iw[1], q2 = e2 * r.iw[2];
    const float iq = frcp((q0 + q1) + q2);
    w0 = q0 * iq; w1 = q1 * iq; w2 = q2 * iq;
}

// fast_weights of the unclipped triangle rec_from_snaps(a0, a1, a2) would build (v1 <-> v2 swapped), straight
// from the snaps' floats: the vertex differences and the pixel-centre offsets are exact in float either way,
// so the weights are the same bits without the integer sign extensions and conversions.
__device__ __forceinline__ void fast_weights_snaps(const TriSnap& a0, const TriSnap& a1, const TriSnap& a2, int32_t px,
                                                   int32_t py, float& w0, float& w1, float& w2) {
    const float X0 = snap_Xf(a0), Y0 = snap_Yf(a0);
    const float fx1 = snap_Xf(a2) - X0, fy1 = snap_Yf(a2) - Y0, fx2 = snap_Xf(a1) - X0, fy2 = snap_Yf(a1) - Y0;
    const float dx = (float)(256 * px + 128) - X0, dy = (float)(256 * py + 128) - Y0;
    const float e1 = __builtin_fmaf(-fx2, dy, fy2 * dx);
    const float e2 = __builtin_fmaf(fx1, dy, -fy1 * dx);
    const float e0 = (__builtin_fmaf(fx1, fy2, -fy1 * fx2) - e1) - e2;
    const float q0 = e0 * a0.iw, q1 = e1 * a2.iw, q2 = e2 * a1.iw;
    const float iq = frcp((q0 + q1) + q2);
    w0 = q0 * iq; w1 = q1 * iq; w2 = q2 * iq;
}

// Perspective-correct barycentric weights of pixel (px, py) in the oracle's order: exact int64 edge
// functions at the pixel centre, IEEE divides (the EXACT build's interpolation; the shadow lookup uses
// them in both builds so its compare sees the oracle's light-space depth bit for bit).
__device__ __forceinline__ void exact_weights(const TriRec& r, int32_t px, int32_t py, float& w0, float& w1, float& w2) {
    // The edge functions and the area are exact integers converted to float once (round to nearest):
    // a triangle under 125 px on a side (the common case) has every product below 2^30, so 32-bit
    // arithmetic gives the same integers, and so the same floats, as the 64-bit form.
    float fe[3], fS;
    const int32_t xmin = min(r.X[0], min(r.X[1], r.X[2])), xmax = max(r.X[0], max(r.X[1], r.X[2]));
    const int32_t ymin = min(r.Y[0], min(r.Y[1], r.Y[2])), ymax = max(r.Y[0], max(r.Y[1], r.Y[2]));
    if (xmax - xmin < 32000 && ymax - ymin < 32000) {  // |a|, |b|, |pixel - vertex| < 2^15 for a covered pixel
        const int32_t Xp = 256 * px + 128, Yp = 256 * py + 128;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = k, j = (k + 1) % 3;
            fe[k] = (float)((r.Y[i] - r.Y[j]) * (Xp - r.X[i]) + (r.X[j] - r.X[i]) * (Yp - r.Y[i]));
        }
        fS = (float)((r.X[1] - r.X[0]) * (r.Y[2] - r.Y[0]) - (r.Y[1] - r.Y[0]) * (r.X[2] - r.X[0]));
    } else {
        const int64_t Xp = 256 * (int64_t)px + 128, Yp = 256 * (int64_t)py + 128;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = k, j = (k + 1) % 3;
            const int64_t a = (int64_t)r.Y[i] - r.Y[j];
            const int64_t bb = (int64_t)r.X[j] - r.X[i];
            const int64_t c = -(a * r.X[i] + bb * r.Y[i]);
            fe[k] = (float)(a * Xp + bb * Yp + c);
        }
        fS = (float)((int64_t)(r.X[1] - r.X[0]) * (int64_t)(r.Y[2] - r.Y[0]) -
                     (int64_t)(r.Y[1] - r.Y[0]) * (int64_t)(r.X[2] - r.X[0]));
    }
    const RcpRef rS = rcp_ref(fS);
    const float l0 = div_rn(fe[1], rS), l1 = div_rn(fe[2], rS), l2 = div_rn(fe[0], rS);
    const float q0 = l0 * r.iw[0], q1 = l1 * r.iw[1], q2 = l2 * r.iw[2];
    const float qs = (q0 + q1) + q2;
    const RcpRef rq = rcp_ref(qs);
    w0 = div_rn(q0, rq); w1 = div_rn(q1, rq); w2 = div_rn(q2, rq);
}

// Shadow lookup (oracle shadow_visibility): the fraction of the 2x2 bilinear depth compare
// (zref - bias <= map) that passes at light-NDC point (lx, ly, lz); 1 outside the map. IEEE mul/add in
// the oracle's order (this file is compiled without contraction).
__device__ __forceinline__ float shadow_vis(const TriFrameParams& fp, const uint32_t* smap, float lx, float ly, float lz) {
    const float u = lx * 0.5f + 0.5f, v = ly * 0.5f + 0.5f;
    if (!(u >= 0.0f && u <= 1.0f && v >= 0.0f && v <= 1.0f)) return 1.0f;
    const int32_t n = (int32_t)fp.s_size;
    const float fx = u * (float)n - 0.5f, fy = v * (float)n - 0.5f;
    const float x0 = floorf(fx), y0 = floorf(fy);
    const float a = fx - x0, bb = fy - y0;
    const int32_t i0 = (int32_t)x0, j0 = (int32_t)y0;
    const float zref = lz - fp.s_bias;
    const int32_t ia = min(max(i0, 0), n - 1), ib = min(max(i0 + 1, 0), n - 1);
    const int32_t ja = min(max(j0, 0), n - 1), jb = min(max(j0 + 1, 0), n - 1);
    float m00, m10, m01, m11;
    TRI_G const uint32_t* sm = (TRI_G const uint32_t*)smap;
    if (ib == ia + 1) {  // adjacent columns: one 8-B load per row (as sample_tex)
        const u32x2a r0 = ld_pair(sm + (size_t)ja * n + ia), r1 = ld_pair(sm + (size_t)jb * n + ia);
        m00 = __uint_as_float(r0.x); m10 = __uint_as_float(r0.y);
        m01 = __uint_as_float(r1.x); m11 = __uint_as_float(r1.y);
    } else {  // a clamped column at the map's edge
        m00 = __uint_as_float(sm[(size_t)ja * n + ia]); m10 = __uint_as_float(sm[(size_t)ja * n + ib]);
        m01 = __uint_as_float(sm[(size_t)jb * n + ia]); m11 = __uint_as_float(sm[(size_t)jb * n + ib]);
    }
    const float c00 = zref <= m00 ? 1.0f : 0.0f;
    const float c10 = zref <= m10 ? 1.0f : 0.0f;
    const float c01 = zref <= m01 ? 1.0f : 0.0f;
    const float c11 = zref <= m11 ? 1.0f : 0.0f;
    const float l0 = c00 + a * (c10 - c00), l1 = c01 + a * (c11 - c01);
    return l0 + bb * (l1 - l0);
}

// The varyings of the triangle's three vertex slots: 16-B gathers, issued before the weights are
// computed (their addresses need only the slots, the weights need the snapped vertices too). The
// three colour gathers are issued late, once the weights are done and the snapped vertices' registers are free:
// the peak register count falls enough for 7 waves/SIMD. Both translation units (round 4: the shadow instantiation
// too, 92 -> 86 VGPRs, which with 6 waves/SIMD spills 6 instead of 20: C5 k_raster 166.5 -> 158.7 us).
// EARLY (fetch_fragment_to's kEarly): the fast single-draw solid instantiation (C3's) issues its colour gathers with
// the other varyings after all: within its 56-VGPR cap the scheduler keeps them without a spill, and their latency no
// longer sits between the weights and the shading (C3 10.89k -> 11.03k frames/s, same box; every other instantiation
// spills with them early, so keeps them late)
struct Taps {
    V4 a0, a1, a2, b0, b1, b2, c0, c1, c2;
};
// SRC: an unclipped primitive's vertex (fb.src), else a clipped polygon's (fb.vary); the same buffer unless ONE.
template <bool ONE = false, bool SRC = false>
__device__ __forceinline__ V4 ld_vary(const FetchBufs& fb, uint32_t slot, uint32_t j) {
    if (ONE) {  // 36-B prefixes: 12-B pieces, no texture coordinate (the stride is the buffer's)
        const u32x3v q = rec96<36>(SRC ? fb.src : fb.vary, slot, j * 12u);
        return V4{__uint_as_float(q[0]), __uint_as_float(q[1]), __uint_as_float(q[2]), 0.0f};
    }
    // plain-float views (HIP vector unions defeat SROA); fb.src is fb.vary unless obj48 (the input records)
    const uint4 q = rec128<48>(SRC ? fb.src : fb.vary, slot, j * 16u);
    return V4{__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w)};
}
template <bool ONE = false, bool SRC = false, bool EARLY = false>
__device__ __forceinline__ Taps load_taps(const FetchBufs& fb, uint32_t v0, uint32_t v1, uint32_t v2, bool colour = true) {
    Taps t;
    t.a0 = ld_vary<ONE, SRC>(fb, v0, 0); t.a1 = ld_vary<ONE, SRC>(fb, v0, 1);
    t.b0 = ld_vary<ONE, SRC>(fb, v1, 0); t.b1 = ld_vary<ONE, SRC>(fb, v1, 1);
    t.c0 = ld_vary<ONE, SRC>(fb, v2, 0); t.c1 = ld_vary<ONE, SRC>(fb, v2, 1);
    if (EARLY && colour) {
        t.a2 = ld_vary<ONE, SRC>(fb, v0, 2); t.b2 = ld_vary<ONE, SRC>(fb, v1, 2); t.c2 = ld_vary<ONE, SRC>(fb, v2, 2);
    }
    return t;
}

// The draw's 48-B shade record (tint, texture descriptor).
struct ShadeRec {
    uint4 st, sd, ss;
};
// When every lane of the wave shades the same draw (the common case: a bin is mostly one mesh), the record comes
// through three scalar buffer loads instead of three wave-wide gathers (the texture units' data return is what C5's
// fragment stage waits on).
__device__ __forceinline__ ShadeRec load_shade(const FetchBufs& fb, uint32_t d) {
    // (d0 in the test's own scope: declared in the function's, the !ONE kernels' register allocation changes)
    if (const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d); __ballot(d != d0) == 0ull) {  // wave-uniform draw
        const uint64_t base = (uint64_t)fb.shade_base;  // a raw descriptor: base, 0 stride, size, flags
        const u32x4v r = u32x4v{(uint32_t)base, (uint32_t)(base >> 32) & 0xFFFFu, fb.shade_bytes, 0x00020000u};
        const int off = (int)(d0 * (uint32_t)sizeof(TriDrawShade));
        const u32x4v a = tri_s_buffer_load_v4(r, off, 0), b = tri_s_buffer_load_v4(r, off + 16, 0),
                     c = tri_s_buffer_load_v4(r, off + 32, 0);
        return ShadeRec{make_uint4(a[0], a[1], a[2], a[3]), make_uint4(b[0], b[1], b[2], b[3]),
                        make_uint4(c[0], c[1], c[2], c[3])};
    }
    return ShadeRec{rec128<48>(fb.shade, d, 0u), rec128<48>(fb.shade, d, 16u), rec128<48>(fb.shade, d, 32u)};
}

// The varyings at weights (w0, w1, w2), the draw d's texture sample and tint: Frag fields 0..18 through
// `put`.
// XF48: the instantiation may apply obj48's per-draw model and normal matrices (not the shadow instantiation: the
// host keeps frames with the pre-pass and a non-identity obj48 draw on world-space varyings, so that kernel carries
// none of this code's registers)
template <bool EXACT, bool ONE, bool XF48, int KIND = kKindGeneric, typename Put>
__device__ __forceinline__ void fetch_attrs(const TriFrameParams& fp, const TriDeviceBuffers& b, const FetchBufs& fb,
                                            const Taps& t, uint32_t d, float w0, float w1, float w2, const float* lut,
                                            Put&& put) {
    auto ip = [&](float x0, float x1, float x2) {
        return EXACT ? interp_exact(w0, w1, w2, x0, x1, x2) : interp_fast(w0, w1, w2, x0, x1, x2);
    };
    const V4 &a0 = t.a0, &a1 = t.a1, &a2 = t.a2, &b0 = t.b0, &b1 = t.b1, &b2 = t.b2, &c0 = t.c0, &c1 = t.c1, &c2 = t.c2;
    // field-wise stores (a struct-valued f3 store is ABI-coerced to <2 x float> + float, which
    // keeps the pixel-pair path's fragments from being promoted to registers)
    auto row = [](float c0v, float c1v, float c2v, float x, float y, float z, float w) {
        return __builtin_fmaf(c0v, x, __builtin_fmaf(c1v, y, __builtin_fmaf(c2v, z, w)));
    };
    if (ONE && kind_flag<KIND>(TRI_KIND_XFORM, obj_mode(fp) && fp.obj_xform)) {  // object-space position and normal: the model / normal matrices
        const float px = ip(a0.x, b0.x, c0.x), py = ip(a0.y, b0.y, c0.y), pz = ip(a0.z, b0.z, c0.z);
        const float nx = ip(a1.x, b1.x, c1.x), ny = ip(a1.y, b1.y, c1.y), nz = ip(a1.z, b1.z, c1.z);
        const float* m = fp.draw0.model;  // column-major, affine (vary_obj)
        const float* n = fp.draw0.nm;     // NM[c*3+r]
        put(0, row(m[0], m[4], m[8], px, py, pz, m[12]));
        put(1, row(m[1], m[5], m[9], px, py, pz, m[13]));
        put(2, row(m[2], m[6], m[10], px, py, pz, m[14]));
        put(3, row(n[0], n[3], n[6], nx, ny, nz, 0.0f));
        put(4, row(n[1], n[4], n[7], nx, ny, nz, 0.0f));
        put(5, row(n[2], n[5], n[8], nx, ny, nz, 0.0f));
    } else if (!ONE && XF48 && obj48_mode(fp) && fp.obj48_xform) {
        // obj48: the fragment's own draw's matrices, one draw of the wave at a time (a waterfall: usually one
        // pass), read with scalar loads, so they live in SGPRs
        const float px = ip(a0.x, b0.x, c0.x), py = ip(a0.y, b0.y, c0.y), pz = ip(a0.z, b0.z, c0.z);
        const float nx = ip(a1.x, b1.x, c1.x), ny = ip(a1.y, b1.y, c1.y), nz = ip(a1.z, b1.z, c1.z);
        float o[6];
        for (;;) {
            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
            if (d == d0) {
                TRI_G const TriDrawDev& dr = b.draws[d0];
                TRI_G const float* m = dr.model;
                TRI_G const float* n = dr.nm;
                o[0] = row(m[0], m[4], m[8], px, py, pz, m[12]);
                o[1] = row(m[1], m[5], m[9], px, py, pz, m[13]);
                o[2] = row(m[2], m[6], m[10], px, py, pz, m[14]);
                o[3] = row(n[0], n[3], n[6], nx, ny, nz, 0.0f);
                o[4] = row(n[1], n[4], n[7], nx, ny, nz, 0.0f);
                o[5] = row(n[2], n[5], n[8], nx, ny, nz, 0.0f);
                break;
            }
        }
        for (int i = 0; i < 6; ++i) put(i, o[i]);
    } else {
        put(0, ip(a0.x, b0.x, c0.x)); put(1, ip(a0.y, b0.y, c0.y)); put(2, ip(a0.z, b0.z, c0.z));
        put(3, ip(a1.x, b1.x, c1.x)); put(4, ip(a1.y, b1.y, c1.y)); put(5, ip(a1.z, b1.z, c1.z));
    }
    if (ONE && kind_flag<KIND>(TRI_KIND_UCOL, obj_mode(fp) && fp.obj_ucol)) {  // one colour for every vertex (its interpolation is the colour)
        put(6, fp.ucol[0]); put(7, fp.ucol[1]); put(8, fp.ucol[2]);
    } else {
        put(6, ip(a2.x, b2.x, c2.x)); put(7, ip(a2.y, b2.y, c2.y)); put(8, ip(a2.z, b2.z, c2.z));
    }
    const float u = ip(a0.w, b0.w, c0.w), v = ip(a1.w, b1.w, c1.w);
    put(9, u); put(10, v);
    if (ONE || fp.shade_solid) {  // uniform: one draw with a 1x1 slot, its texel and tint are kernel arguments
        for (int i = 0; i < 4; ++i) put(11 + i, fp.sc.solid[i]);
        for (int i = 0; i < 4; ++i) put(15 + i, fp.sc.tint[i]);
        return;
    }
    const ShadeRec sh = load_shade(fb, d);
    const uint4 &st = sh.st, &sd = sh.sd, &ss = sh.ss;
    TriTexDesc td;
    td.texels = reinterpret_cast<const uint32_t*>(((uint64_t)sd.y << 32) | sd.x);
    td.w = sd.z; td.h = sd.w;
    td.solid[0] = __uint_as_float(ss.x); td.solid[1] = __uint_as_float(ss.y);
    td.solid[2] = __uint_as_float(ss.z); td.solid[3] = __uint_as_float(ss.w);
    const float4 tx = (kAblate & 128) ? make_float4(u, v, u, 1.0f) : sample_tex(td, u, v, lut);  // 128: no texture
    const float4 tint = make_float4(__uint_as_float(st.x), __uint_as_float(st.y), __uint_as_float(st.z), __uint_as_float(st.w));
    put(11, tx.x); put(12, tx.y); put(13, tx.z); put(14, tx.w);
    put(15, tint.x); put(16, tint.y); put(17, tint.z); put(18, tint.w);
}

// Interpolate the visible triangle's varyings at pixel (px, py) (perspective-correct).
// Writes the fragment through `put(field_index, value)` (fields in Frag order), so one body serves
// the single-pixel Frag and the lane-pair FragP without an intermediate in scratch memory.
// Rejected (round 4): the sun visibility of every visible pixel in a pass of its own before shading, so that
// the shading loop would not hold the light-space gathers and the map taps in its registers: C5 k_raster
// 188.6 -> 206.4 us (the pass fetches each fragment's index and snapped vertices a second time).
// The fast build's shadow instantiation shades with the exact weights its lookup needs (one weight
// computation per fragment instead of two; C5 +1 % over both). Rejected (round 4): the lookup from
// the fast weights, recomputed with the exact ones only where a depth compare or the map border is within a few
// ulps: the fallback's registers cost 5 spilled VGPRs and C5 -3 %.
//
// CLIPM: 0 = the key may name a clipped sub-triangle (tested per pixel), 1 = it never does (the shading loop
// defers clipped pixels, raster_bin's kDefer), 2 = it always does (the deferred pass).
// KIND (frame kinds): `fbk` names the gather descriptors, built once per workgroup; a kind with one vertex colour
// issues no colour gathers at all (the generic instantiation issues them and never waits for them).
template <bool EXACT, bool SHADOW, bool ONE, int CLIPM = 0, int KIND = kKindGeneric, typename Put>
__device__ __forceinline__ void fetch_fragment_to(const TriFrameParams& fp, const TriDeviceBuffers& b, uint64_t key,
                                                  int32_t px, int32_t py, const float* lut, Put&& put,
                                                  const uint32_t* qtab = nullptr, const FetchBufs* fbk = nullptr) {
    constexpr bool kInlineVis = SHADOW;
    const uint32_t low = (uint32_t)key;
    // qtab (bins with the queue-position table, uniform): the key names the primitive above its queue position (qenc)
    const uint32_t prim = qtab ? kQPrimMax - (low >> 11) : TRI_PRIM_MAX - (low >> 3);
    const uint32_t sub = CLIPM == 1 ? 0u : (qtab ? (low >> 8) & 7u : low & 7u);  // >= 1: sub-triangle of a clipped primitive
    const FetchBufs fb = (KIND >= 0 && fbk) ? *fbk : fetch_bufs<ONE, KIND>(fp, b);
    constexpr bool kEarly = ONE && !EXACT && !SHADOW;  // the colour gathers with the other varyings (load_taps)
    const bool ucol = ONE && kind_flag<KIND>(TRI_KIND_UCOL, obj_mode(fp) && fp.obj_ucol);
    // (issued early, the colour gathers are unconditional: on a frame with one vertex colour (obj_ucol) they read the
    // records' colours beside their positions, unused; a uniform branch around them cost the instantiation 4 spills)
    const bool vcol = KIND >= 0 ? !ucol : (kEarly || !ucol);
    uint32_t sl[3] = {0, 0, 0}, d = 0;
    TriSnap a0{}, a1{}, a2{};
    uint32_t v0 = 0, v1 = 0, v2 = 0, dl = 0;
    Taps taps;
    if (CLIPM != 2) {
        if (qtab) {  // the coverage pass's table: three LDS words (four with the draw), no index gather
            const uint32_t q = low & 0xFFu;
            sl[0] = qtab[q]; sl[1] = qtab[kQtab + q]; sl[2] = qtab[2 * kQtab + q];
            if (!ONE) d = qtab[3 * kQtab + q];
        } else {
            prim_slots<ONE, !SHADOW>(fp, b, prim, sl, d);
        }
        // Every gather that needs only the slots is issued before the first wait: the snapped vertices and
        // the varyings are one round trip after the index fetch (the snaps are loaded for a clipped primitive
        // too, unused: its sub-triangle's record names its slots).
        a0 = ld_snap_xyw(fb, sl[0]); a1 = ld_snap_xyw(fb, sl[1]); a2 = ld_snap_xyw(fb, sl[2]);
        v0 = sl[0]; v1 = sl[2]; v2 = sl[1];  // set-up orientation (rec_from_snaps swaps v1 and v2)
        // obj48: the geometry's input records at slot + vdelta[draw]
        if (!ONE) dl = obj_delta(fp, d);  // (0 unless obj48: the host zeroes vdelta)
        // the varyings are gathered before the (rare) clipped branch: its record loads are waited for inside
        // it, and a wait at the join would otherwise hold the snaps and varyings in two round trips
        taps = load_taps<ONE, true, kEarly>(fb, v0 + dl, v1 + dl, v2 + dl, vcol);
    } else if (!ONE) {
        prim_slots<ONE, !SHADOW>(fp, b, prim, sl, d);  // the draw (its shade record); the slots come from the record
    }
    TriRec rc;
    if (CLIPM == 2 || (CLIPM == 0 && sub)) {  // a clipped primitive's sub-triangle: its own slots and varyings
        rc = load_rec(b.recs, b.clip_slot[prim] + sub - 1u);
        v0 = rc.v[0]; v1 = rc.v[1]; v2 = rc.v[2];
        taps = load_taps<ONE, false, kEarly>(fb, v0, v1, v2, vcol);
    }
    const bool from_rec = CLIPM == 2 || (CLIPM == 0 && sub);
    // the three vertices' light-space positions (rejected in round 4: recomputing them from the varyings' world
    // positions, k_vertex's own operations and so the same bits, instead of three 16-B gathers: 63 VALU per pixel
    // for 3 gathers, C5 k_raster +3.5 us)
    uint4 L0, L1, L2;
    if constexpr (kInlineVis) {
        const RecBuf lr = rec_buf(b.lpos, 16u, (uint64_t)fp.nslots + fp.ovf_vert_cap);
        L0 = rec128<16>(lr, v0, 0u); L1 = rec128<16>(lr, v1, 0u); L2 = rec128<16>(lr, v2, 0u);
    }
    const TriRec r = from_rec ? rc : rec_from_snaps(prim, sl, a0, a1, a2);
    // obj48: past the light-space gathers (slot-indexed) an unclipped primitive's vertices are only needed as
    // input-record indices (one register each instead of the slot and the offset)
    if (!ONE && !from_rec) { v0 += dl; v1 += dl; v2 += dl; }
    float w0, w1, w2;
    // exact int64 edge functions, IEEE divides (oracle order). The shadow lookup needs these weights in both
    // builds (the fast build shades with them too instead of forming its own)
    if (EXACT || (kInlineVis && !(kAblate & 2048))) {
        exact_weights(r, px, py, w0, w1, w2);
    } else if (CLIPM == 1) {  // never clipped here: the floats of the snaps directly
        fast_weights_snaps(a0, a1, a2, px, py, w0, w1, w2);
    } else {
        fast_weights(r, px, py, w0, w1, w2);
    }
    if (kAblate & 1024) {  // diagnostics: 1024 = no colour gathers (3 of the fragment's 13 loads; same VALU)
        taps.a2 = V4{w0, w1, w2, 0.0f}; taps.b2 = taps.a2; taps.c2 = taps.a2;
    } else if (ucol) {
        // one colour for every vertex: fetch_attrs takes it from the frame arguments
    } else if (!kEarly) {
        if (!from_rec) {  // an unclipped primitive's vertices: fb.src (fb.vary unless ONE or obj48; with CLIPM 0 a
                          // per-lane choice: both masked)
            taps.a2 = ld_vary<ONE, true>(fb, v0, 2); taps.b2 = ld_vary<ONE, true>(fb, v1, 2);
            taps.c2 = ld_vary<ONE, true>(fb, v2, 2);
        } else {
            taps.a2 = ld_vary<ONE>(fb, v0, 2); taps.b2 = ld_vary<ONE>(fb, v1, 2); taps.c2 = ld_vary<ONE>(fb, v2, 2);
        }
    }

    float vis = 1.0f;
    if constexpr (kInlineVis && !(kAblate & 2048)) {  // light-space position at the pixel with the oracle's weights,
                                                       // then the compare (diagnostics: 2048 = no lookup)
        auto ix = [&](uint32_t a, uint32_t bq, uint32_t c) {
            return interp_exact(w0, w1, w2, __uint_as_float(a), __uint_as_float(bq), __uint_as_float(c));
        };
        vis = shadow_vis(fp, b.shadow_map, ix(L0.x, L1.x, L2.x), ix(L0.y, L1.y, L2.y), ix(L0.z, L1.z, L2.z));
    }
    put(19, vis);
    fetch_attrs<EXACT, ONE, !SHADOW, KIND>(fp, b, fb, taps, d, w0, w1, w2, lut, put);
}

template <bool EXACT, bool SHADOW, bool ONE, int CLIPM = 0, int KIND = kKindGeneric>
__device__ __forceinline__ void fetch_fragment(const TriFrameParams& fp, const TriDeviceBuffers& b, uint64_t key,
                                               int32_t px, int32_t py, const float* lut, Frag& f,
                                               const uint32_t* qtab = nullptr, const FetchBufs* fbk = nullptr) {
    fetch_fragment_to<EXACT, SHADOW, ONE, CLIPM, KIND>(fp, b, key, px, py, lut, [&](int i, float x) { (&f.wx)[i] = x; },
                                                       qtab, fbk);
}

// ------------------------------------------------------------------------------------------
// skybox pass (Skybox.cpp:13-79, Skybox.vert:30-41, Skybox.frag:28-35, cull FRONT / depth LEQUAL
// without writes, recorded before the meshes, Renderer.cpp:5076-5082). Same arithmetic as the
// oracle's sky_pixel(): a background pixel's interpolated direction is the view-space point where
// its ray leaves the 20-unit cube; Vulkan cube sampling with seamless LINEAR filtering.
// ------------------------------------------------------------------------------------------
template <bool FAST = false>
__device__ __forceinline__ int cube_face(f3 d, float& s, float& t) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    int face;
    float ma, sc, tc;
    if (ax >= ay && ax >= az) {
        face = d.x >= 0.0f ? 0 : 1; ma = ax; sc = d.x >= 0.0f ? -d.z : d.z; tc = -d.y;
    } else if (ay >= az) {
        face = d.y >= 0.0f ? 2 : 3; ma = ay; sc = d.x; tc = d.y >= 0.0f ? d.z : -d.z;
    } else {
        face = d.z >= 0.0f ? 4 : 5; ma = az; sc = d.z >= 0.0f ? d.x : -d.x; tc = -d.y;
    }
    if (!(ma > 0.0f)) { s = 0.5f; t = 0.5f; return face; }
    if (FAST) {
        const float h = 0.5f * frcp(ma);
        s = sc * h + 0.5f;
        t = tc * h + 0.5f;
    } else {
        s = 0.5f * (sc / ma) + 0.5f;
        t = 0.5f * (tc / ma) + 0.5f;
    }
    return face;
}

__device__ __forceinline__ f3 face_dir(int face, float sc, float tc) {
    switch (face) {
        case 0: return mk(1.0f, -tc, -sc);
        case 1: return mk(-1.0f, -tc, sc);
        case 2: return mk(sc, 1.0f, tc);
        case 3: return mk(sc, -1.0f, -tc);
        case 4: return mk(sc, -tc, 1.0f);
        default: return mk(-sc, -tc, -1.0f);
    }
}

struct SkyTex {
    TRI_G const uint32_t* t;
    int32_t n;
    const float* lut;
    __device__ __forceinline__ f3 decode(uint32_t p) const {
        return mk(lut[p & 0xFFu], lut[(p >> 8) & 0xFFu], lut[(p >> 16) & 0xFFu]);
    }
    __device__ __forceinline__ f3 texel(int face, int32_t i, int32_t j) const {
        return decode(t[((uint32_t)face * (uint32_t)n + (uint32_t)j) * (uint32_t)n + (uint32_t)i]);
    }
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
        const int32_t ci = min(max(i, 0), n - 1), cj = min(max(j, 0), n - 1);
        const f3 a = texel(face, ci, cj), b = across(face, i, cj), c = across(face, ci, j);
        return mk(((a.x + b.x) + c.x) / 3.0f, ((a.y + b.y) + c.y) / 3.0f, ((a.z + b.z) + c.z) / 3.0f);
    }
    template <bool FAST = false>
    __device__ __forceinline__ f3 sample(f3 d) const {
        float s, tt;
        const int face = cube_face<FAST>(d, s, tt);
        const float u = s * (float)n - 0.5f, v = tt * (float)n - 0.5f;
        const float fu = floorf(u), fv = floorf(v);
        const float a = u - fu, bb = v - fv;
        const int32_t i0 = (int32_t)fu, j0 = (int32_t)fv;
        f3 t00, t10, t01, t11;
        if (i0 >= 0 && i0 + 1 < n && j0 >= 0 && j0 + 1 < n) {  // inside the face: 8-B row loads
            TRI_G const uint32_t* r = t + ((uint32_t)face * (uint32_t)n + (uint32_t)j0) * (uint32_t)n + (uint32_t)i0;
            const u32x2a r0 = ld_pair(r), r1 = ld_pair(r + n);
            t00 = decode(r0.x); t10 = decode(r0.y); t01 = decode(r1.x); t11 = decode(r1.y);
        } else {  // a tap across an edge or corner of the face (seamless filtering)
            t00 = fetch(face, i0, j0); t10 = fetch(face, i0 + 1, j0);
            t01 = fetch(face, i0, j0 + 1); t11 = fetch(face, i0 + 1, j0 + 1);
        }
        auto lp = [](float x, float y, float w) { return x + w * (y - x); };
        return mk(lp(lp(t00.x, t10.x, a), lp(t01.x, t11.x, a), bb), lp(lp(t00.y, t10.y, a), lp(t01.y, t11.y, a), bb),
                  lp(lp(t00.z, t10.z, a), lp(t01.z, t11.z, a), bb));
    }
};

// The sky ray of pixel (px, py), shared by k_raster's sky pass (sky_bgra) and k_sky_fill (sky_fill.hip): unproject
// both clip planes (m: sky_ip), intersect the 20-unit cube in view space (R: sky_R) and return hit(h) for the point h
// where the ray leaves it, or miss() where the ray misses the cube or h has w <= 0 (pw: sky_pw). Continuations, not a
// result the caller tests: inlined, sky_bgra is the code it was before the direction had a second user.
template <class Miss, class Hit>
__device__ __forceinline__ auto sky_ray(int32_t W, int32_t H, const float* m, const float* R, const float* pw, int32_t px,
                                        int32_t py, Miss miss, Hit hit) {
    const float xn = (float)(2 * px + 1) / (float)W - 1.0f;
    const float yn = (float)(2 * py + 1) / (float)H - 1.0f;
    auto unproject = [&](float zn) {
        const float x = ((m[0] * xn + m[4] * yn) + m[8] * zn) + m[12];
        const float y = ((m[1] * xn + m[5] * yn) + m[9] * zn) + m[13];
        const float z = ((m[2] * xn + m[6] * yn) + m[10] * zn) + m[14];
        const float w = ((m[3] * xn + m[7] * yn) + m[11] * zn) + m[15];
        return mk(x / w, y / w, z / w);
    };
    const f3 o = unproject(0.0f), o1 = unproject(1.0f);
    const f3 r = sub3(o1, o);
    const float oa[3] = {(R[0] * o.x + R[1] * o.y) + R[2] * o.z, (R[3] * o.x + R[4] * o.y) + R[5] * o.z,
                         (R[6] * o.x + R[7] * o.y) + R[8] * o.z};
    const float ra[3] = {(R[0] * r.x + R[1] * r.y) + R[2] * r.z, (R[3] * r.x + R[4] * r.y) + R[5] * r.z,
                         (R[6] * r.x + R[7] * r.y) + R[8] * r.z};
    const float half = 20.0f;
    float t_in = -INFINITY, t_out = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (ra[a] != 0.0f) {
            const float t0 = (-half - oa[a]) / ra[a], t1 = (half - oa[a]) / ra[a];
            t_in = fmaxf(t_in, fminf(t0, t1));
            t_out = fminf(t_out, fmaxf(t0, t1));
        } else if (oa[a] < -half || oa[a] > half) {
            return miss();
        }
    }
    if (!(t_out >= t_in)) return miss();
    const f3 h = mk(o.x + r.x * t_out, o.y + r.y * t_out, o.z + r.z * t_out);
    const float w = ((pw[0] * h.x + pw[1] * h.y) + pw[2] * h.z) + pw[3];
    if (!(w > 0.0f)) return miss();
    return hit(h);
}

// BGRA8 sky colour of pixel (px, py), or the clear colour where the skybox does not cover it.
// Inlined into its own pass of k_raster (a call here costs the whole kernel a scratch stack and the
// callee-saved register set: measured 5x slower at C3).
__device__ __forceinline__ uint32_t sky_bgra(const TriFrameParams& fp, const TriDeviceBuffers& b, int32_t px, int32_t py,
                                          const float* lut) {
    return sky_ray(
        fp.W, fp.H, fp.sky_ip, fp.sky_R, fp.sky_pw, px, py, [&]() { return fp.clear_bgra; },
        [&](f3 h) {
            const SkyTex sky{b.sky, (int32_t)fp.sky_size, lut};
            const f3 c = sky.sample(norm3(h));
            return unorm8(c.z) | (unorm8(c.y) << 8) | (unorm8(c.x) << 16) | (255u << 24);
        });
}

// TRI_SKY_PERSP (fast build): the ray of a pixel starts at the eye, the centre of the skybox cube,
// so it always leaves the cube and its exit point has the direction of the far-plane point; cube
// sampling only uses direction ratios, so no normalisation and no cube intersection is needed. (m: sky_far)
__device__ __forceinline__ f3 sky_persp_dir(int32_t W, int32_t H, const float* m, int32_t px, int32_t py) {
    const float xn = (float)(2 * px + 1) / (float)W - 1.0f;
    const float yn = (float)(2 * py + 1) / (float)H - 1.0f;
    f3 d = mk(m[0] * xn + m[1] * yn + m[2], m[4] * xn + m[5] * yn + m[6], m[8] * xn + m[9] * yn + m[10]);
    if (m[12] * xn + m[13] * yn + m[14] < 0.0f) d = mk(-d.x, -d.y, -d.z);  // homogeneous w < 0
    return d;
}
__device__ __forceinline__ uint32_t sky_bgra_persp(const TriFrameParams& fp, const TriDeviceBuffers& b, int32_t px,
                                                   int32_t py, const float* lut) {
    const f3 d = sky_persp_dir(fp.W, fp.H, fp.sky_far, px, py);
    const SkyTex sky{b.sky, (int32_t)fp.sky_size, lut};
    const f3 c = sky.sample<true>(d);
    return unorm8(c.z) | (unorm8(c.y) << 8) | (unorm8(c.x) << 16) | (255u << 24);
}

// bbox∩bin pixels above which a triangle is rasterized by the whole workgroup (TRI_BIG_AREA*, above)
template <int BL>
constexpr int big_area() { return BL == 4 ? TRI_BIG_AREA16 : TRI_BIG_AREA; }
constexpr int kBigQueue = 1024;

// Bijective XCD-aware block -> bin remap (cdna_hip_programming.md §5 "XCD swizzle must be
// bijective"): workgroups b, b+8, b+16 ... share an XCD's L2, so give them consecutive bins — each
// XCD then rasterizes one contiguous band of the screen and re-reads neighbours' records from L2.
__device__ __forceinline__ int xcd_bin(int b, int nb) {
    const int xcd = b & 7, q = nb >> 3, r = nb & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// Balanced coverage (16x16 bins, i.e. sparse frames; dense 32x32 bands keep the per-lane walk, where
// C3's ~4-px rows made the per-job overhead cost more than the divergence it removed: 127 -> 136 us,
// while C2 went 16.8k -> 19.0k fps): a pass takes up to kCovPass queue entries; each entry's edge/depth constants at its
// clipped bbox corner go to LDS, and its bbox rows become jobs spread evenly over the workgroup, so a
// wave no longer issues its longest triangle's whole bbox walk while most lanes idle. A row job steps
// exactly like raster_serial (integer edge functions, float depth offsets in steps of 256: exact), so
// the keys are bit-identical.
// 32x32 bins: one lane per triangle (two lanes per triangle paid with the per-pixel bbox walk in round 2; with
// the span walk one lane per triangle is faster: C3 k_raster 95.3 -> 94.0 us, four lanes 94.5), and the per-lane
// walk visits each row's covered span only (raster_span).
// Raised wave priority (s_setprio 1 + TRI_RASTER_PRIO) from a 32x32 bin's start to the end of its coverage: the
// latency-bound init and coverage phases issue ahead of other workgroups' shading waves (C3 k_raster 101.7 -> 99.6 us,
// round 3 A/B; at 16x16 bins it was slower, so BL == 5 only). Scheduling only: output unchanged.
constexpr int kCovPass = 160;   // entries per pass (LDS: 64 B each)
constexpr int kCovJobs = 1024;  // row jobs per pass (u16: entry << 6 | row); rows beyond stay with their lane
struct __attribute__((aligned(16))) CovEntry {
    int32_t A[3], B[3], F[3];
    float dzdX, dzdY, z0, fdx0, fdy0;
    uint32_t low;
    uint32_t pk;  // row0 (12 bits) | width - 1 (6 bits) << 12 | far_clip << 18
};
static_assert(sizeof(CovEntry) == 64, "CovEntry: 64 bytes");

template <int BL>
__device__ __forceinline__ void cov_row(const CovEntry& c, uint32_t r, uint64_t* keys) {
    int32_t f0 = c.F[0] + c.B[0] * (int32_t)r, f1 = c.F[1] + c.B[1] * (int32_t)r, f2 = c.F[2] + c.B[2] * (int32_t)r;
    const float t2 = c.dzdY * (c.fdy0 + 256.0f * (float)r);
    const bool far_clip = (c.pk >> 18) & 1u;
    const uint32_t row = (c.pk & 0xFFFu) + (r << BL);
    const uint32_t rend = row + ((c.pk >> 12) & 0x3Fu);
    float fdx = c.fdx0;
    for (uint32_t a = row; a <= rend; ++a) {
        if ((f0 | f1 | f2) >= 0) {
            uint64_t key;
            if (depth_key((c.z0 + c.dzdX * fdx) + t2, far_clip, c.low, key)) atomicMin(&keys[a], key);
        }
        f0 += c.A[0]; f1 += c.A[1]; f2 += c.A[2];
        fdx += 256.0f;
    }
}

// texture(AiBlendTexture, gl_FragCoord.xy * AiBlendConfig.yz) (Default.frag:186-188): R8G8B8A8_UNORM (the UNORM
// decode b / 255, no sRGB), LINEAR, CLAMP_TO_EDGE, level 0 (the sampler of EnsureAiTextureResources,
// Renderer.cpp:1462-1470). Same float operations as the oracle's ai_sample.
__device__ __forceinline__ float4 sample_ai(const TriFrameParams& fp, const TriDeviceBuffers& b, int32_t px, int32_t py) {
    const float u = ((float)px + 0.5f) * fp.ai_sx, v = ((float)py + 0.5f) * fp.ai_sy;
    const float x = u * (float)fp.ai_tw - 0.5f, y = v * (float)fp.ai_th - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    const float a = x - fx, bb = y - fy;
    const int32_t i0 = (int32_t)fminf(fmaxf(fx, -1.0f), 1.0e9f), j0 = (int32_t)fminf(fmaxf(fy, -1.0f), 1.0e9f);
    const int32_t tw = (int32_t)fp.ai_tw, th = (int32_t)fp.ai_th;
    const int32_t xa = min(max(i0, 0), tw - 1), xb = min(max(i0 + 1, 0), tw - 1);
    const int32_t ya = min(max(j0, 0), th - 1), yb = min(max(j0 + 1, 0), th - 1);
    TRI_G const uint32_t* t = b.ai_frame;
    const uint32_t p00 = t[(size_t)ya * tw + xa], p10 = t[(size_t)ya * tw + xb];
    const uint32_t p01 = t[(size_t)yb * tw + xa], p11 = t[(size_t)yb * tw + xb];
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        auto ch = [&](uint32_t q) { return (float)((q >> (8 * c)) & 0xFFu) / 255.0f; };
        const float t00 = ch(p00), t10 = ch(p10), t01 = ch(p01), t11 = ch(p11);
        const float l0 = t00 + a * (t10 - t00), l1 = t01 + a * (t11 - t01);
        r[c] = l0 + bb * (l1 - l0);
    }
    return make_float4(r[0], r[1], r[2], r[3]);
}
// mix(x, y, a) = x * (1 - a) + y * a (GLSL)
__device__ __forceinline__ float mix_ai(float x, float y, float w) { return x * (1.0f - w) + y * w; }

// Default.frag for one fragment at pixel (px, py), stored as B8G8R8A8_UNORM. AI: the instantiation for frames with
// the AI frame blend (k_raster_ai; the other kernels carry none of its registers)
template <bool EXACT, bool ONE, bool AI, int KIND = kKindGeneric>
__device__ __forceinline__ uint32_t shade_bgra(const TriFrameParams& fp, const TriDeviceBuffers& b, const Frag& f,
                                               int32_t px, int32_t py, uint32_t npt_k = 0u) {
    if (EXACT) {
        float4 c = fs_exact(fp, f);
        if (AI && fp.ai_on) {  // (an AI frame-generation model is loaded) the blend with the AI frame's sample
            const float4 ai = sample_ai(fp, b, px, py);
            const float w = fp.ai_wgt;
            c = make_float4(mix_ai(c.x, ai.x, w), mix_ai(c.y, ai.y, w), mix_ai(c.z, ai.z, w), mix_ai(c.w, ai.w, w));
        }
        return unorm8(c.z) | (unorm8(c.y) << 8) | (unorm8(c.x) << 16) | (unorm8(c.w) << 24);
    }
    uint32_t a8 = fp.sc.a8;
    if constexpr (KIND >= 0) asm volatile("" : "+s"(a8));  // (a kind: read ahead of the shading, not in front of the store)
    float4 c = fs_fast<ONE, KIND>(fp.sc, f, npt_k);
    if (AI && fp.ai_on) {  // the fast build's channels are already scaled by 255 (tone_out): mix there
        const float4 ai = sample_ai(fp, b, px, py);
        const float w = fp.ai_wgt;
        const float alpha = ONE ? fp.sc.sbt[3] : c.w;
        if (fs_fast_nan(fp.sc, f)) return unorm8(mix_ai(alpha, ai.w, w)) << 24;  // mix(NaN, ., w) is NaN: stored as 0
        return fast_bgra(mix_ai(c.x, 255.0f * ai.x, w), mix_ai(c.y, 255.0f * ai.y, w), mix_ai(c.z, 255.0f * ai.z, w),
                         unorm8(mix_ai(alpha, ai.w, w)));
    }
    return fast_bgra(c.x, c.y, c.z, ONE ? a8 : unorm8(c.w));  // ONE: the uniform alpha byte, host-folded
}

// One bin: coverage into the LDS key tile, then shading and stores. Reached by the whole workgroup.
// KIND (frame kinds, k_raster_kind): the shading loops test no frame-uniform switch and read the gather
// descriptors, the store bases and the light count from values formed once per workgroup.
template <bool EXACT, int BL, bool SHADOW, bool ONE = false, bool AI = false, int KIND = kKindGeneric>
__device__ __forceinline__ void raster_bin(const TriFrameParams& fp, const TriDeviceBuffers& b, const int bin) {
    constexpr int BIN = 1 << BL;
    __shared__ uint64_t keys[BIN * BIN];
    constexpr bool kBalanced = BL == 4;                    // balanced coverage (cov_row), else the per-lane walk
    constexpr bool kQt = BL == 5 && (ONE || SHADOW);       // the queue-position table (qenc)
    constexpr uint32_t kQw = ONE ? 3u : 4u;  // table words per entry: the slots (and the draw)
    // (the table's 3 KB come from the large-triangle queue: TRI_QTAB_BIGN, above)
    constexpr int kBigN = kBalanced ? kBigQueue / 2 : ((kQt && ONE) ? TRI_QTAB_BIGN : kBigQueue);
    __shared__ uint32_t bigq[kBigN];  // queue entries of the large triangles
    __shared__ float lut[512];
    constexpr int kJobWords = (kBalanced && kCovJobs > BIN * BIN ? kCovJobs : BIN * BIN);
    __shared__ uint16_t skyq[kJobWords];  // the coverage pass's row jobs, then the skybox queue
    __shared__ CovEntry cov[kBalanced ? kCovPass : 1];
    __shared__ uint32_t wsum[TRI_BLOCK / 64];
    __shared__ uint32_t nbig, nsky;
    __shared__ uint32_t qtab[kQt ? kQw * kQtab : 1];  // per queue position, the entry's vertex slots
    __shared__ uint16_t bigqp[kQt ? kBigN : 1];      // ... and the large triangles' queue positions
    const int tid = threadIdx.x;
    TRI_STAMP(0);
    if constexpr (BL == 5) __builtin_amdgcn_s_setprio(1 + TRI_RASTER_PRIO);  // (to the end of the coverage)
    const int bx = bin % fp.nbx, by = bin / fp.nbx;
    const int32_t ox = bx * BIN, oy = fp.y0 + by * BIN;
    const int32_t bw = min(BIN, fp.W - ox), bh = min(BIN, fp.y1 - oy);
    // Every lane loads the bin's entry count with a vector (buffer) load issued before the key-tile clear:
    // the barrier below fences LDS only, so the load stays in flight across it instead of being waited for
    // in front of it (a scalar or a lane-0 load would sit on the barrier's critical path).
    const uint32_t cnt_v = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(b.bin_count, 4ull * fp.nbins), (uint32_t)bin * 4u, 0, 0);
    // the lane's first queue entry of the per-lane walk, in flight likewise (entries past the count are loaded
    // and ignored: the queue holds bin_cap >= 256 slots; round-3 A/B: C3 k_raster 98.9 -> 98.0 us, C5 195.6 -> 193.3 us)
    uint32_t pre1 = 0;
    if constexpr (!kBalanced) {
        const Rsrc qr = make_rsrc(b.bin_list + (size_t)bin * fp.bin_cap, 4ull * fp.bin_cap);
        pre1 = __builtin_amdgcn_raw_buffer_load_b32(qr, (uint32_t)tid * 4u, 0, 0);
    }
    for (int i = tid; i < BIN * BIN; i += TRI_BLOCK) keys[i] = kBgKey;
    if (fp.need_lut)
        for (int i = tid; i < 512; i += TRI_BLOCK) lut[i] = b.srgb_lut[i];
    if (tid == 0) {
        nbig = 0;
        nsky = 0;
    }
    lds_barrier();
    TRI_STAMP(1);
    const uint32_t cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt_v);
    const uint32_t* queue = b.bin_list + (size_t)bin * fp.bin_cap;
    uint32_t s0 = 0, s1 = min(cnt, fp.bin_cap);
    // this bin's keys carry queue positions (uniform: small bins of frames within kQPrimMax primitives)
    const bool qmode = kQt && cnt <= kQtab && fp.nprims <= kQPrimMax;
    if (kAblate & 2) {  // diagnostics: no coverage; every pixel shades the bin's first triangle
        if (s1 > s0) {
            const TriRec r = load_entry<ONE, !SHADOW>(fp, b, queue[0]);
            const uint64_t key = (0x3F000000ull << 32) | key_low(r.prim_sub);
            for (int i = tid; i < BIN * BIN; i += TRI_BLOCK) keys[i] = key;
        }
        s1 = s0;
    }
  if constexpr (kBalanced) {
    uint16_t* jobs = skyq;
    const uint32_t lane = lanes_below(~0ull);
    for (uint32_t base = s0; base < s1; base += kCovPass) {  // uniform trip count
        const uint32_t i = base + tid;
        uint32_t nrows = 0;
        TriRec r;
        int32_t cx0 = 0, cx1 = -1, cy0 = 0, cy1 = -1;
        if (tid < kCovPass && i < s1) {
            const uint32_t ri = queue[i];
            r = load_entry<ONE, !SHADOW>(fp, b, ri);
            rec_bbox(r, ox, oy, bw, bh, cx0, cx1, cy0, cy1);
            if (cx0 <= cx1 && cy0 <= cy1) {
                bool big = false;
                if ((cx1 - cx0 + 1) * (cy1 - cy0 + 1) > big_area<BL>()) {
                    const uint32_t q = atomicAdd(&nbig, 1u);
                    if (q < (uint32_t)kBigN) { bigq[q] = ri; big = true; }
                }
                if (!big) {
                    EdgeSetup e;
                    edge_setup(r, e);
                    bool rej = false;
                    CovEntry c;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        c.F[k] = clamp_edge((int64_t)e.A[k] * cx0 + (int64_t)e.B[k] * cy0 + e.D[k], rej);
                        c.A[k] = e.A[k];
                        c.B[k] = e.B[k];
                    }
                    if (!rej) {
                        c.dzdX = e.dzdX; c.dzdY = e.dzdY; c.z0 = r.z[0];
                        c.fdx0 = (float)(256 * cx0 + 128 - r.X[0]);
                        c.fdy0 = (float)(256 * cy0 + 128 - r.Y[0]);
                        c.low = key_low(r.prim_sub);
                        const bool far_clip = (r.z[0] > 1.0f) || (r.z[1] > 1.0f) || (r.z[2] > 1.0f);
                        c.pk = (uint32_t)(((cy0 - oy) << BL) + (cx0 - ox)) | ((uint32_t)(cx1 - cx0) << 12) |
                               (far_clip ? 1u << 18 : 0u);
                        cov[tid] = c;
                        nrows = (uint32_t)(cy1 - cy0 + 1);
                    }
                }
            }
        }
        // exclusive prefix sum of the row counts over the workgroup
        const uint32_t incl = wave_incl_sum(nrows);
        if (lane == 63) wsum[tid >> 6] = incl;
        __syncthreads();
        uint32_t start = incl - nrows, total = 0;
#pragma unroll
        for (int w = 0; w < TRI_BLOCK / 64; ++w) {
            const uint32_t ws = wsum[w];
            if (w < (tid >> 6)) start += ws;
            total += ws;
        }
        for (uint32_t k = 0; k < nrows && start + k < (uint32_t)kCovJobs; ++k)
            jobs[start + k] = (uint16_t)((tid << 6) | k);
        __syncthreads();
        const uint32_t njobs = min(total, (uint32_t)kCovJobs);
        for (uint32_t j = tid; j < njobs; j += TRI_BLOCK) {
            const uint32_t jb = jobs[j];
            cov_row<BL>(cov[jb >> 6], jb & 63u, keys);
        }
        for (uint32_t k = (start < (uint32_t)kCovJobs ? (uint32_t)kCovJobs - start : 0u); k < nrows; ++k)
            cov_row<BL>(cov[tid], k, keys);  // rows past the job table: the owner walks them
        __syncthreads();  // cov / jobs / wsum are reused by the next pass
    }
  } else {
    auto cover = [&](uint32_t i, int32_t sub, int32_t step, bool first) {
        const uint32_t ri = first ? pre1 : queue[i];
        uint32_t dq;
        TriRec r = load_entry_d<ONE, !SHADOW>(fp, b, ri, dq);
        if (kQt && qmode) {  // the entry's slots (set-up orientation undone) at its queue position; the key's payload
            if (!(ri & TRI_ENTRY_CLIPPED)) {
                qtab[i] = r.v[0]; qtab[kQtab + i] = r.v[2]; qtab[2 * kQtab + i] = r.v[1];
                if (!ONE) qtab[3 * kQtab + i] = dq;
            }
            r.prim_sub = qenc(r.prim_sub, i);
        }
        int32_t cx0, cx1, cy0, cy1;
        rec_bbox(r, ox, oy, bw, bh, cx0, cx1, cy0, cy1);
        if (cx0 > cx1 || cy0 > cy1) return;
        if ((cx1 - cx0 + 1) * (cy1 - cy0 + 1) > big_area<BL>()) {
            if (sub != 0) return;  // the first lane of the group hands it over
            const uint32_t q = atomicAdd(&nbig, 1u);
            if (q < (uint32_t)kBigN) {
                bigq[q] = ri;
                if (kQt) bigqp[q] = (uint16_t)i;
                return;
            }
            raster_serial<BL>(r, cx0, cx1, cy0, cy1, ox, oy, keys);  // queue full: this lane walks it all
            return;
        }
        raster_span<BL>(r, cx0, cx1, cy0, cy1, ox, oy, keys, sub, step);
    };
    // (Pairing only as many entries as there are spare lanes when the bin holds 129..256 entries, so that
    // every lane works, measured slower: 105.5 -> 109.8 us at C3. The duplicated fetch and set-up of a
    // pair costs issue slots the CU's other workgroups would use; a wave with no entry costs none.)
    for (uint32_t i = s0 + tid; i < s1; i += TRI_BLOCK) cover(i, 0, 1, i < (uint32_t)TRI_BLOCK);
    __syncthreads();
  }
    TRI_STAMP(2);
    const uint32_t nb = min(nbig, (uint32_t)kBigN);
    for (uint32_t q = 0; q < nb; ++q) {  // large triangles: all lanes share the pixels
        TriRec r = load_entry<ONE, !SHADOW>(fp, b, bigq[q]);
        if (kQt && qmode) r.prim_sub = qenc(r.prim_sub, bigqp[q]);
        int32_t cx0, cx1, cy0, cy1;
        rec_bbox(r, ox, oy, bw, bh, cx0, cx1, cy0, cy1);
        EdgeSetup e;
        edge_setup(r, e);
        bool rej = false;
        int32_t F[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) F[k] = clamp_edge((int64_t)e.A[k] * cx0 + (int64_t)e.B[k] * cy0 + e.D[k], rej);
        if (rej) continue;  // uniform across the workgroup
        const bool far_clip = (r.z[0] > 1.0f) || (r.z[1] > 1.0f) || (r.z[2] > 1.0f);
        const uint32_t low = key_low(r.prim_sub);
        const int32_t rw = cx1 - cx0 + 1, rh = cy1 - cy0 + 1;
        for (int j = tid; j < rw * rh; j += TRI_BLOCK) {
            const int32_t dy = j / rw, dx = j - dy * rw;
            const int32_t f0 = F[0] + e.A[0] * dx + e.B[0] * dy;
            const int32_t f1 = F[1] + e.A[1] * dx + e.B[1] * dy;
            const int32_t f2 = F[2] + e.A[2] * dx + e.B[2] * dy;
            if ((f0 | f1 | f2) >= 0) {
                const int32_t px = cx0 + dx, py = cy0 + dy;
                uint64_t key;
                if (depth_key(frag_depth(r, e, px, py), far_clip, low, key))
                    atomicMin(&keys[((py - oy) << BL) + (px - ox)], key);
            }
        }
    }
    __syncthreads();
    TRI_STAMP(3);
    // queue consumed (every wave's count load has completed: each waited for it, and the barrier's fence
    // covers this workgroup's global accesses): ready for the next frame
    if (tid == 0) {
        if (!kDiagKeepQueues) b.bin_count[bin] = 0;
        if (cnt > fp.bin_cap) note_bin_overflow(b, cnt);
    }
    if constexpr (BL == 5) __builtin_amdgcn_s_setprio(TRI_RASTER_PRIO);
    // shade + store: each wave covers whole BIN-pixel row pieces -> coalesced colour/depth stores.
    // Background pixels go to an LDS queue for the skybox pass below (lane-dense, and its registers
    // are not live during shading).
    const int lx = tid & (BIN - 1);
    const bool sky_on = fp.sky_size != 0;
    const bool sky_const = sky_on && !EXACT && fp.sky_mode == TRI_SKY_UNIFORM;
    const bool sky_queue = kind_flag<KIND>(TRI_KIND_SKYQ, sky_on && !sky_const);
    const bool write_depth = kind_flag<KIND>(TRI_KIND_DEPTH, fp.write_depth != 0u);
    // A kind's per-workgroup values: the gather descriptors, the light count, and the stores' addressing: the colour
    // and depth bases stay in SGPRs and each lane keeps a 32-bit byte offset that advances by a constant per
    // iteration (the host gives a kind only frames whose targets stay below 4 GiB: tri_raster_kind).
    FetchBufs fbk{};
    uint32_t npt_k = 0u, so = 0u, so_step = 0u;
    TRI_G char* cbase = nullptr;
    TRI_G char* dbase = nullptr;
    if constexpr (KIND >= 0) {
        fbk = fetch_bufs<ONE, KIND>(fp, b);
        npt_k = fp.sc.npt;
        cbase = (TRI_G char*)b.color;
        dbase = (TRI_G char*)b.depth;
        so = (uint32_t)((oy - fp.y0 + (tid >> BL)) * fp.W + ox + lx) * 4u;
        so_step = (uint32_t)((TRI_BLOCK / BIN) * fp.W) * 4u;
    }
    // the pixel at band offset `o` (a kind: at byte offset `o32` from the resident bases)
    auto store_c = [&](size_t o, uint32_t o32, uint32_t colour) {
        if constexpr (KIND >= 0) *(TRI_G uint32_t*)(cbase + o32) = colour;
        else b.color[o] = colour;
    };
    auto store_z = [&](size_t o, uint32_t o32, float z) {
        if (!write_depth) return;
        if constexpr (KIND >= 0) *(TRI_G float*)(dbase + o32) = z;
        else b.depth[o] = z;
    };
    // the background colour stays a scalar to its store (its VGPR copy, hoisted out of the loop, was the shadow
    // instantiation's one spilled register)
    const uint32_t bg_sgpr = sky_const ? fp.sky_bgra : fp.clear_bgra;
    auto bg_bgra = [&]() {
        uint32_t v = bg_sgpr;
        asm volatile("" : "+s"(v));
        return v;
    };
    // Clipped sub-triangles' pixels (rare: near-plane and guard-band crossings) are shaded after the loop, from
    // a per-wave LDS queue (a wave shades exactly BIN * BIN / 4 pixels, so its slice never overflows): the
    // loop then carries no clipped branch and no register merge at its join.
    constexpr bool kDefer = BL <= 5;
    static_assert(!kQt || kDefer, "the queue-position table holds no clipped entry: their pixels must be deferred");
    constexpr int kWaveQ = BIN * BIN / (TRI_BLOCK / 64);
    __shared__ uint16_t clipq[kDefer ? BIN * BIN : 1];
    uint32_t nclip = 0;  // this wave's deferred pixels (wave-uniform)
    // (kQt: the loop compiled twice, for bins with and without the queue-position keys, so that neither
    // carries the other's registers)
    auto shade_loop = [&](auto QT) {
        constexpr bool kq = decltype(QT)::value;
        // (a kind: the vector-memory counter drained once ahead of the loop (vmcnt(0), the other counters untouched), so
        // that the loop's header inherits no pending load from the code before it and need not drain the previous
        // iteration's stores)
        if constexpr (KIND >= 0) __builtin_amdgcn_s_waitcnt(0x0F70);
        uint32_t so_it = so - so_step;  // (a kind's store offset of this iteration's pixel)
        for (int ly = tid >> BL; ly < bh; ly += TRI_BLOCK / BIN) {
            so_it += so_step;
            const bool in = lx < bw;
            const uint64_t key = in ? keys[(ly << BL) + lx] : 0ull;
            const bool bg = in && key == kBgKey;
            if constexpr (kDefer) {
                const bool clipped = in && !bg && (((uint32_t)key >> (kq ? 8 : 0)) & 7u) != 0u;
                const uint64_t m = __ballot(clipped);
                if (m) {  // uniform
                    if (clipped) clipq[(tid >> 6) * kWaveQ + nclip + lanes_below(m)] = (uint16_t)((ly << BL) + lx);
                    nclip += (uint32_t)__builtin_popcountll(m);
                }
                if (clipped) continue;
            }
            if (sky_queue) {  // wave-aggregated append (uniform control flow here)
                const uint64_t m = __ballot(bg);
                if (m) {
                    const uint32_t lane = lanes_below(~0ull);
                    const uint32_t leader = (uint32_t)__builtin_ctzll(m);
                    uint32_t base = 0;
                    if (lane == leader) base = atomicAdd(&nsky, (uint32_t)__builtin_popcountll(m));
                    base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)leader);  // leader: uniform
                    if (bg) skyq[base + lanes_below(m)] = (uint16_t)((ly << BL) + lx);
                }
            }
    #ifdef TRI_PRIM_GROUPS
            {
                const bool shade = in && !bg;
                uint64_t m = __ballot(shade);
                const uint32_t pid = shade ? ((uint32_t)key >> 3) : 0u;
                const uint32_t active = (uint32_t)__builtin_popcountll(m);
                uint32_t groups = 0;
                while (m) {
                    const uint32_t lp = (uint32_t)__shfl((int)pid, (int)__builtin_ctzll(m));
                    m &= ~__ballot(shade && pid == lp);
                    ++groups;
                }
                if ((uint32_t)(tid & 63) == (uint32_t)__builtin_ctzll(__ballot(true)) && active) {
                    atomicAdd(&g_tri_groups[0], 1ull);
                    atomicAdd(&g_tri_groups[1], (unsigned long long)groups);
                    atomicAdd(&g_tri_groups[2], (unsigned long long)active);
                }
            }
    #endif
            if (!in) continue;
            int32_t px = ox + lx;
            const int32_t py = oy + ly;
            // (the shadow instantiation: px re-formed each pixel, so that 256 px + 128, loop-invariant, is not hoisted
            // into a register held across the loop, the one its table-reading variant had to spill)
            if constexpr (SHADOW) asm volatile("" : "+v"(px));
            uint32_t out;
            float z;
            if (bg) {
                const size_t o = KIND >= 0 ? 0 : (size_t)(py - fp.y0) * fp.W + px;
                if (!sky_queue) store_c(o, so_it, bg_bgra());
                store_z(o, so_it, 1.0f);
                continue;
            } else if (kAblate & 1) {  // diagnostics: coverage only
                z = __uint_as_float((uint32_t)(key >> 32));
                out = (uint32_t)key;
            } else {
                z = __uint_as_float((uint32_t)(key >> 32));
                Frag f;
                if (kAblate & 256) {  // diagnostics: 256 = no varyings fetch (a fragment made from the key)
                    const float k0 = __uint_as_float(((uint32_t)key & 0x7FFFFFu) | 0x3F000000u);
                    for (int q = 0; q < 20; ++q) (&f.wx)[q] = k0 + 0.01f * q;
                } else {
                    fetch_fragment<EXACT, SHADOW, ONE, kDefer ? 1 : 0, KIND>(fp, b, key, px, py, lut, f, kq ? qtab : nullptr, &fbk);
                }
                out = shade_bgra<EXACT, ONE, AI, KIND>(fp, b, f, px, py, npt_k);
            }
            const size_t o = KIND >= 0 ? 0 : (size_t)(py - fp.y0) * fp.W + px;
            store_c(o, so_it, out);
            store_z(o, so_it, z);
        }
    };
    if (kQt && qmode) shade_loop(std::true_type{});
    else shade_loop(std::false_type{});
    if constexpr (kDefer) {  // this wave's clipped pixels (its own LDS slice: no workgroup barrier)
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = (uint32_t)(tid & 63); i < nclip; i += 64) {
            const uint32_t li = clipq[(tid >> 6) * kWaveQ + i];
            const int32_t qx = (int32_t)(li & (BIN - 1)), qy = (int32_t)(li >> BL);
            const uint64_t key = keys[li];
            const int32_t px = ox + qx, py = oy + qy;
            Frag f;
            fetch_fragment<EXACT, SHADOW, ONE, 2, KIND>(fp, b, key, px, py, lut, f, (kQt && qmode) ? qtab : nullptr, &fbk);
            const size_t o = (size_t)(py - fp.y0) * fp.W + px;
            const uint32_t o32 = KIND >= 0 ? (uint32_t)((py - fp.y0) * fp.W + px) * 4u : 0u;
            store_c(o, o32, shade_bgra<EXACT, ONE, AI, KIND>(fp, b, f, px, py, npt_k));
            store_z(o, o32, __uint_as_float((uint32_t)(key >> 32)));
        }
    }
#ifdef TRI_PHASE_TIMING
    __syncthreads();
    TRI_STAMP(4);
    if (!sky_queue || fp.sky_mode == TRI_SKY_PREFILLED) { TRI_STAMP(5); return; }
#endif
    // (TRI_SKY_PREFILLED: k_sky_fill wrote every background pixel ahead of this kernel, and the loop above stored none)
    if (!sky_queue || fp.sky_mode == TRI_SKY_PREFILLED) return;
    __syncthreads();
    const uint32_t ns = nsky;
    if (fp.sky_lut && !fp.need_lut && ns > 0) {  // uniform: only bins showing sky stage the LUT
        for (int i = tid; i < 512; i += TRI_BLOCK) lut[i] = b.srgb_lut[i];
        __syncthreads();
    }
    const bool persp = !EXACT && fp.sky_mode == TRI_SKY_PERSP;
    for (uint32_t i = tid; i < ns; i += TRI_BLOCK) {  // skybox pass over the queued background pixels
        const uint32_t li = skyq[i];
        const int32_t px = ox + (int32_t)(li & (BIN - 1)), py = oy + (int32_t)(li >> BL);
        b.color[(size_t)(py - fp.y0) * fp.W + px] =
            persp ? sky_bgra_persp(fp, b, px, py, lut) : sky_bgra(fp, b, px, py, lut);
    }
#ifdef TRI_PHASE_TIMING
    __syncthreads();
    TRI_STAMP(5);
#endif
}

}  // namespace
