// vertex_stage.hip — the frame's first kernels, in a translation unit of their own so that they take their own
// scheduling strategy (Makefile: VERTEX_SCHED):
//
//   k_vertex       vs_transform   Default.vert:60-105, one lane per (draw, referenced vertex)
//   k_vertex_band  the same for row bands of single-draw frames (a workgroup per four vertex blocks)
//   k_reset        a frame with no vertex work
//
// Each takes the frame's arguments by value and publishes them for the later kernels (raster_device.h).
#define TRI_KERNEL_TU 1  // device pointers in TriDeviceBuffers carry the global address space (raster_launch.h)
#include "raster_device.h"

namespace {

// Shadow pre-pass, per vertex slot: the light-NDC position (light_view_proj is affine, so w = 1 and the
// main pass's perspective divide is the identity), kept for the fragment lookup, and its snap to the
// s_size x s_size map (oracle shadow_raster_triangle: X = rint((x * S/2 + S/2) * 256)) with outcode
// bits for the map's four sides and TRI_OC_CLIP beyond the guard band (such casters are dropped).
__device__ __forceinline__ void shadow_vertex(const TriFrameParams& fp, const TriDeviceBuffers& b, uint32_t slot,
                                              float4 world) {
    const float4 l = mat_vec_seq(fp.lvp, world);
    b.lpos[slot] = make_float4(l.x, l.y, l.z, 0.0f);
    uint32_t oc = 0;
    if (l.x + 1.0f < 0.0f) oc |= TRI_OC_XNEG;
    if (1.0f - l.x < 0.0f) oc |= TRI_OC_XPOS;
    if (l.y + 1.0f < 0.0f) oc |= TRI_OC_YNEG;
    if (1.0f - l.y < 0.0f) oc |= TRI_OC_YPOS;
    if (l.x < -fp.s_g || l.x > fp.s_g || l.y < -fp.s_g || l.y > fp.s_g) oc |= TRI_OC_CLIP;
    TriSnap sn{(int32_t)(oc << 24), 0, 1.0f, l.z};
    if (!(oc & TRI_OC_CLIP)) {
        const int32_t X = (int32_t)rintf((l.x * fp.s_hw + fp.s_hw) * 256.0f);
        sn.xo = (X & 0x00FFFFFF) | (int32_t)(oc << 24);
        sn.y = (int32_t)rintf((l.y * fp.s_hw + fp.s_hw) * 256.0f);
    }
    b.lsnap[slot] = sn;
}

__device__ __forceinline__ void reset_counters(TriCounters* c) {
    c->ovf_records = 0; c->ovf_verts = 0; c->tris_setup = 0; c->tris_clipped = 0;
    c->bin_entries = 0;  // `flags` / `bin_max` are sticky (cleared by the host)
}

__global__ __launch_bounds__(TRI_BLOCK) void k_reset(TRI_FIRST_KARGS) {  // a frame with no vertex work
    if (threadIdx.x == 0) reset_counters(a_.b.counters);
    publish_args(a_, pub_);
}

// The clip position, outcode and snap of a vertex at `world` (its clip position kept when the clipper needs it).
__device__ __forceinline__ void store_snap(const TriFrameParams& fp, const TriDeviceBuffers& b, uint32_t slot,
                                           const TriDrawDev& dr, float4 world) {
    const float4 clip = mat_vec_seq(fp.pv, world);
    uint32_t oc = outcode(fp, clip);
    // clip_from_world draws: a vertex without an outcode has world.w == 1 and its clip position is
    // recomputed by the clipper from `vary` (or its record); a non-finite position (w != 1) is marked for clipping
    if (dr.clip_from_world && oc == 0u && !(world.w == 1.0f)) oc = TRI_OC_CLIP;
    if (oc != 0u || !dr.clip_from_world) b.clip[slot] = clip;
    TriSnap sn{0, 0, 0.0f, 0.0f};
    if (!(oc & TRI_OC_CLIP)) {
        int32_t X, Y;
        snap_compute(fp, clip, X, Y, sn.z, sn.iw);
        sn.xo = __float_as_int((float)X);  // |X|, |Y| < 2^22 inside the guard band: exact as floats
        sn.y = __float_as_int((float)Y);
    }
    b.snap[slot] = sn;
    b.oc[slot] = (uint8_t)oc;
}

// Default.vert for vertex slot `slot` of draw `dr` (whose first slot is `vbase`).
__device__ __forceinline__ void vertex_slot(const TriFrameParams& fp, const TriDeviceBuffers& b, uint32_t slot,
                                            const TriDrawDev& dr, uint32_t vbase) {
    const int64_t gi = (int64_t)dr.base_vertex + (int64_t)(dr.min_index + (slot - vbase));
    if (gi < 0 || (uint64_t)gi >= b.vertex_count) {
        b.snap[slot] = TriSnap{0, 0, 0.0f, 0.0f};
        b.oc[slot] = (uint8_t)TRI_OC_BAD;
        if (fp.shadow_on) b.lsnap[slot] = TriSnap{(int32_t)(TRI_OC_BAD << 24), 0, 0.0f, 0.0f};
        return;
    }
    if (obj_mode(fp) || obj48_mode(fp)) {  // no varyings to write: the position stream alone (12 B), then the snap
        const Rsrc pr = make_rsrc(b.vpos, 12ull * b.vertex_count);
        const auto q = __builtin_amdgcn_raw_buffer_load_b96(pr, (uint32_t)gi * 12u, 0, 0);
        const float4 world = mat_vec_seq(dr.model, make_float4(__uint_as_float(q[0]), __uint_as_float(q[1]),
                                                               __uint_as_float(q[2]), 1.0f));
        store_snap(fp, b, slot, dr, world);
        // (obj48 with the pre-pass: the same world position as the input-record path below, so the same map)
        if (fp.shadow_on) shadow_vertex(fp, b, slot, world);
        return;
    }
    // three 16-byte loads (a plain struct load is split into overlapping per-field loads)
    const Rsrc vr = make_rsrc(b.vin, 48ull * b.vertex_count);
    const uint4 q0 = ld128(vr, (uint32_t)gi * 48u), q1 = ld128(vr, (uint32_t)gi * 48u + 16u),
                q2 = ld128(vr, (uint32_t)gi * 48u + 32u);
    TriVsIn in;  // {pos, u}{normal, v}{colour, 0}
    in.px = __uint_as_float(q0.x); in.py = __uint_as_float(q0.y); in.pz = __uint_as_float(q0.z);
    in.u = __uint_as_float(q0.w); in.nx = __uint_as_float(q1.x); in.ny = __uint_as_float(q1.y);
    in.nz = __uint_as_float(q1.z); in.v = __uint_as_float(q1.w); in.cr = __uint_as_float(q2.x);
    in.cg = __uint_as_float(q2.y); in.cb = __uint_as_float(q2.z);
    float4 sp = make_float4(in.px, in.py, in.pz, 1.0f);
    float snx = in.nx, sny = in.ny, snz = in.nz;
    if (dr.bone_count > 0 && b.vskin) {  // Default.vert:64-85
        const TriVsSkin sk = b.vskin[gi];
        float s[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float w = sk.w[k];
            if (w <= 0.0f) continue;
            const int bi = sk.idx[k];
            if (bi < 0 || bi >= dr.bone_count) continue;
            const uint32_t buf = (uint32_t)(dr.bone_offset + bi);
            if (buf >= fp.bone_count) continue;
            TRI_G const float* bm = b.bones + 16ull * buf;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = s[i] + w * bm[i];
        }
        sp = mat_vec_seq(s, sp);
        const float nx = (s[0] * snx + s[4] * sny) + s[8] * snz;
        const float ny = (s[1] * snx + s[5] * sny) + s[9] * snz;
        const float nz = (s[2] * snx + s[6] * sny) + s[10] * snz;
        snx = nx; sny = ny; snz = nz;
    }
    const float4 world = mat_vec_seq(dr.model, sp);
    const float* nm = dr.nm;  // NM[c*3+r]; N' = NM * n
    float nnx = (nm[0] * snx + nm[3] * sny) + nm[6] * snz;
    float nny = (nm[1] * snx + nm[4] * sny) + nm[7] * snz;
    float nnz = (nm[2] * snx + nm[5] * sny) + nm[8] * snz;
    const float inv = 1.0f / sqrtf((nnx * nnx + nny * nny) + nnz * nnz);
    nnx = nnx * inv; nny = nny * inv; nnz = nnz * inv;
    const float u = (in.u * dr.tex_scale[0]) * dr.tiling + dr.tex_offset[0];
    const float v = (in.v * dr.tex_scale[1]) * dr.tiling + dr.tex_offset[1];
    store_snap(fp, b, slot, dr, world);
    if (vary36_mode(fp)) {  // 36-B record: three 12-B stores (the slot's bytes are 4-B aligned)
        TRI_G F3* vo = reinterpret_cast<TRI_G F3*>(b.vary) + 3u * slot;
        vo[0] = F3{world.x, world.y, world.z};
        vo[1] = F3{nnx, nny, nnz};
        vo[2] = F3{in.cr, in.cg, in.cb};
    } else {  // the input records' layout (TriVsIn), so that obj48 frames read those records with the same code
        float4* vo = b.vary + 3u * slot;
        vo[0] = make_float4(world.x, world.y, world.z, u);
        vo[1] = make_float4(nnx, nny, nnz, v);
        vo[2] = make_float4(in.cr, in.cg, in.cb, 0.0f);
    }
    if (fp.shadow_on) shadow_vertex(fp, b, slot, world);
}

// Cluster culling (row bands). A cluster's object-space box goes through (P * V) * M; when every corner
// is in front of the eye (w > 0 over the whole box, w being affine) the box's image is bounded by its
// corners' images, and a cluster whose bound misses the context's rows or columns (2-pixel margin), or
// lies wholly before z = 0 or beyond z = w, has no fragment here: k_setup skips its primitives (exactly
// what their set-up would conclude). Skinned draws move their vertices off the boxes and are kept.
__device__ __forceinline__ bool cluster_visible(const TriFrameParams& fp, const TriDrawDev& dr, const TriCluster& c) {
    if (c.lo[0] > c.hi[0]) return false;  // no valid vertex: every primitive of the cluster is dropped anyway
    if (dr.bone_count > 0) return true;
    float m[16];  // (P * V) * M, column-major
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            m[4 * j + r] = fp.pv[r] * dr.model[4 * j] + fp.pv[4 + r] * dr.model[4 * j + 1] +
                           fp.pv[8 + r] * dr.model[4 * j + 2] + fp.pv[12 + r] * dr.model[4 * j + 3];
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY, z0 = INFINITY, z1 = -INFINITY;
    bool front = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float px = (k & 1) ? c.hi[0] : c.lo[0], py = (k & 2) ? c.hi[1] : c.lo[1], pz = (k & 4) ? c.hi[2] : c.lo[2];
        const float cx = m[0] * px + m[4] * py + m[8] * pz + m[12];
        const float cy = m[1] * px + m[5] * py + m[9] * pz + m[13];
        const float cz = m[2] * px + m[6] * py + m[10] * pz + m[14];
        const float cw = m[3] * px + m[7] * py + m[11] * pz + m[15];
        front = front && cw > 1e-4f;
        const float iw = 1.0f / cw;
        x0 = fminf(x0, cx * iw); x1 = fmaxf(x1, cx * iw);
        y0 = fminf(y0, cy * iw); y1 = fmaxf(y1, cy * iw);
        z0 = fminf(z0, cz * iw); z1 = fmaxf(z1, cz * iw);
    }
    if (!front) return true;
    const float wx0 = x0 * fp.hw + fp.hw, wx1 = x1 * fp.hw + fp.hw;
    const float wy0 = y0 * fp.hh + fp.hh, wy1 = y1 * fp.hh + fp.hh;
    // the margins (2 px, 1e-4 in depth) cover the rounding difference between the box corners' (P V) M
    // product and the vertices' P V (M p): the test is never stricter than the vertices' own
    return !(wy1 < (float)fp.y0 - 2.0f || wy0 > (float)fp.y1 + 2.0f || wx1 < -2.0f || wx0 > (float)fp.W + 2.0f ||
             z1 < -1e-4f || z0 > 1.0f + 1e-4f);
}

// One lane per vertex slot. With cluster culling on: lanes 0 .. ncl_total-1 of the grid (the first few
// waves) test one (draw, cluster) box each and store its flag for k_setup; every wave then tests the union
// box of its 256-slot vertex block (the clusters referencing it, precomputed at upload: one load) and,
// unless the shadow pre-pass needs every caster, skips a block whose box misses the rows. A vertex of any
// visible primitive is always transformed: its cluster's box lies inside the block's union box.
__global__ __launch_bounds__(TRI_BLOCK) void k_vertex(TRI_FIRST_KARGS) {
    TRI_BIND_FIRST_ARGS;
    publish_args(a_, pub_);
    const uint32_t slot = blockIdx.x * TRI_BLOCK + threadIdx.x;
    if (slot == 0) reset_counters(b.counters);  // per-frame counters, consumed from k_setup on
    const bool valid = slot < fp.nslots;
    int d = 0;
    uint32_t vbase = 0;
    if (valid && !fp.one_draw) {
        d = find_range(b.draw_vbase, (int)fp.ndraws, slot);
        vbase = b.draw_vbase[d];
    }
    bool needed = true;
    if (fp.cull_on) {  // uniform
        if (slot < fp.ncl_total) {  // this lane's (draw, cluster) flag
            const int cd = fp.one_draw ? 0 : find_range(b.draw_cbase, (int)fp.ndraws, slot);
            const uint32_t lc = slot - (fp.one_draw ? 0u : b.draw_cbase[cd]);
            const bool vis = fp.one_draw ? cluster_visible(fp, fp.draw0, b.clusters[fp.draw0.cl_first + lc])
                                         : cluster_visible(fp, b.draws[cd], b.clusters[b.draws[cd].cl_first + lc]);
            b.cvis[slot] = vis ? 1u : 0u;
        }
        const uint32_t blk = (slot - vbase) / TRI_VBLOCK;
        uint64_t pending = __ballot(valid);
        while (pending) {  // the wave's distinct (draw, block) groups, usually one
            const int l = __builtin_ctzll(pending);
            const int gd = __builtin_amdgcn_readlane(d, l);
            const uint32_t gb = (uint32_t)__builtin_amdgcn_readlane((int)blk, l);
            const bool mine = valid && d == gd && blk == gb;
            pending &= ~__ballot(mine);
            const bool any = fp.one_draw ? cluster_visible(fp, fp.draw0, b.vbox[fp.draw0.vblk_first + gb])
                                         : cluster_visible(fp, b.draws[gd], b.vbox[b.draws[gd].vblk_first + gb]);
            if (mine) needed = any;
        }
    }
    if (!valid || (fp.cull_vertex && !needed)) return;
    // two calls, not one through a selected reference: each sees its draw's address space (kernel arguments or
    // global memory), so a single draw's constants are scalar loads
    if (fp.one_draw) vertex_slot(fp, b, slot, fp.draw0, vbase);
    else vertex_slot(fp, b, slot, b.draws[d], vbase);
}

// Row bands of single-draw frames (cull_vertex && one_draw): a quarter of k_vertex's workgroups, each owning
// the four 256-slot vertex blocks blockIdx.x + i * gridDim.x (i = 0..3). Wave i tests block i's union box
// (the four tests run side by side instead of four waves repeating one), the flags meet in LDS, and the
// whole workgroup transforms the visible blocks one after another. A band's visible blocks are contiguous
// in slot order (its rows' clusters), so the stride spreads them over different workgroups: at N = 8 a
// workgroup holds at most one, and 3/4 of the launch's dispatches (all empty) are gone. The cluster flags
// for k_setup are the same lanes' work as in k_vertex, grid-strided.
static_assert(TRI_VBLOCK == TRI_BLOCK, "k_vertex_band: one workgroup-wide pass per vertex block");
__global__ __launch_bounds__(TRI_BLOCK) void k_vertex_band(TRI_FIRST_KARGS) {
    TRI_BIND_FIRST_ARGS;
    publish_args(a_, pub_);
    __shared__ uint32_t blk_vis[TRI_BLOCK / 64];
    const uint32_t tid = threadIdx.x, G = gridDim.x;
    if (blockIdx.x == 0 && tid == 0) reset_counters(b.counters);
    const TriDrawDev& dr = fp.draw0;
    for (uint32_t c = blockIdx.x * TRI_BLOCK + tid; c < fp.ncl_total; c += G * TRI_BLOCK)
        b.cvis[c] = cluster_visible(fp, dr, b.clusters[dr.cl_first + c]) ? 1u : 0u;
    const uint32_t nblk = (fp.nslots + TRI_VBLOCK - 1) / TRI_VBLOCK;
    const uint32_t w = tid / 64u, blk = blockIdx.x + w * G;
    const bool vis = blk < nblk && cluster_visible(fp, dr, b.vbox[dr.vblk_first + blk]);
    if ((tid & 63u) == 0) blk_vis[w] = vis ? 1u : 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < TRI_BLOCK / 64; ++i) {
        if (!blk_vis[i]) continue;  // uniform
        const uint32_t slot = (blockIdx.x + i * G) * TRI_VBLOCK + tid;
        if (slot < fp.nslots) vertex_slot(fp, b, slot, dr, 0u);
    }
}

}  // namespace

const void* tri_vertex_stage_kernel(TriFrontKernel k) {
    auto f = [](auto kernel) { return reinterpret_cast<const void*>(kernel); };
    return k == kFrontVertex ? f(k_vertex) : k == kFrontBand ? f(k_vertex_band) : f(k_reset);
}
