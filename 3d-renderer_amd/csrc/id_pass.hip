// id_pass.hip — the entity-id pass (include/tri_raster.h "entity ids"): which draw owns each pixel, the distinct draws
// of a rectangle, and the selection outline.
//
//   k_id_raster<BL>  one workgroup per bin of the frame's bin grid, between the frame's set-up and its raster kernel.
//                    Coverage only, like k_shadow_raster: the bin's queue is walked with the raster's own helpers
//                    (load_entry_d, rec_bbox, raster_span / raster_serial, then the cooperative large-triangle loop)
//                    into an LDS tile of 64-bit (depth, primitive order) keys, so every pixel's winner is the one
//                    the raster kernel will shade. The plain per-lane walk at every bin size: the balanced 16-px walk
//                    and the queue-position table are optimisations of the shading kernels and produce the same keys.
//                    Then per pixel: background -> 0, else the key's primitive -> its draw through prim_slots (the
//                    single-draw frame, the index route's search, or the prim_vs record; a clipped piece's key names
//                    its parent primitive) -> draw + 1. The kernel reads counts and queues and writes neither; a
//                    count above bin_cap is clamped as the raster clamps it (the raster reports the overflow).
//   k_id_collect     one lane per pixel of a rectangle, atomicOr of bit id - 1 into a per-draw bitmap; a lane whose
//                    left neighbour in the wave holds the same id leaves the atomic to it.
//   k_id_outline     one workgroup per 32 x 32 tile: the tile's selected bits with an 8-pixel halo staged in LDS, the
//                    (2r + 1)^2 neighbourhood as two separable passes over it, and the text pass's blend at coverage 1
//                    on the outline pixels. Tiles without a selected pixel in reach leave after the staging.
#define TRI_KERNEL_TU 1
#define TRI_PK_SHADE 0
#include "raster_bin.h"

namespace {

template <int BL>
__global__ __launch_bounds__(TRI_BLOCK) void k_id_raster(TRI_KARGS, TriIdArgs ia) {
    TRI_BIND_ARGS;
    constexpr int BIN = 1 << BL;
    __shared__ uint64_t keys[BIN * BIN];
    __shared__ uint32_t bigq[kBigQueue];  // queue entries of the large triangles
    __shared__ uint32_t nbig;
    const int tid = threadIdx.x;
    const int bin = xcd_bin(blockIdx.x, fp.nbins);
    const int bx = bin % fp.nbx, by = bin / fp.nbx;
    const int32_t ox = bx * BIN, oy = fp.y0 + by * BIN;
    const int32_t bw = min(BIN, fp.W - ox), bh = min(BIN, fp.y1 - oy);
    for (int i = tid; i < BIN * BIN; i += TRI_BLOCK) keys[i] = kBgKey;
    if (tid == 0) nbig = 0;
    __syncthreads();
    const uint32_t n = min(b.bin_count[bin], fp.bin_cap);
    const uint32_t* queue = b.bin_list + (size_t)bin * fp.bin_cap;
    for (uint32_t i = tid; i < n; i += TRI_BLOCK) {
        const uint32_t ri = queue[i];
        uint32_t dq;
        const TriRec r = load_entry_d<false, true>(fp, b, ri, dq);
        int32_t cx0, cx1, cy0, cy1;
        rec_bbox(r, ox, oy, bw, bh, cx0, cx1, cy0, cy1);
        if (cx0 > cx1 || cy0 > cy1) continue;
        if ((cx1 - cx0 + 1) * (cy1 - cy0 + 1) > big_area<BL>()) {
            const uint32_t q = atomicAdd(&nbig, 1u);
            if (q < (uint32_t)kBigQueue) {
                bigq[q] = ri;
                continue;
            }
            raster_serial<BL>(r, cx0, cx1, cy0, cy1, ox, oy, keys);  // queue full: this lane walks it all
            continue;
        }
        raster_span<BL>(r, cx0, cx1, cy0, cy1, ox, oy, keys);
    }
    __syncthreads();
    const uint32_t nb = min(nbig, (uint32_t)kBigQueue);
    for (uint32_t q = 0; q < nb; ++q) {  // large triangles: all lanes share the pixels
        const TriRec r = load_entry<false, true>(fp, b, bigq[q]);
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
    // each wave covers whole BIN-pixel row pieces: coalesced id stores. lx < bw <= W - ox and ly < bh <= y1 - oy keep
    // every store inside the W x (y1 - y0) buffer.
    for (int i = tid; i < BIN * BIN; i += TRI_BLOCK) {
        const int32_t ly = i >> BL, lx = i & (BIN - 1);
        if (lx >= bw || ly >= bh) continue;
        const uint64_t key = keys[i];
        uint32_t id = 0u;
        if (key != kBgKey) {
            // (sub-triangles of a clipped primitive carry their parent's number: its draw is theirs)
            const uint32_t prim = TRI_PRIM_MAX - ((uint32_t)key >> 3);
            uint32_t sl[3], d;
            prim_slots<false, true>(fp, b, prim, sl, d);
            id = d + 1u;
        }
        ia.ids[(size_t)(oy - fp.y0 + ly) * (size_t)fp.W + (size_t)(ox + lx)] = id;
    }
}

__global__ __launch_bounds__(TRI_BLOCK) void k_id_collect(const uint32_t* __restrict__ ids, int32_t W, int32_t x0,
                                                          int32_t row0, int32_t w, int32_t h,
                                                          uint32_t* __restrict__ bits, uint32_t nwords) {
    const uint64_t i = (uint64_t)blockIdx.x * TRI_BLOCK + threadIdx.x;
    uint32_t id = 0u;
    if (i < (uint64_t)w * (uint64_t)h) {
        const int32_t y = (int32_t)(i / (uint32_t)w), x = (int32_t)(i - (uint64_t)y * (uint32_t)w);
        id = ids[(size_t)(row0 + y) * (size_t)W + (size_t)(x0 + x)];
    }
    // a run of one id inside the wave: its first lane speaks for it
    const uint32_t left = (uint32_t)__shfl_up((int)id, 1);
    const bool first = (threadIdx.x & 63u) == 0u || left != id;
    if (id && first && (id - 1u) / 32u < nwords) {
        // a bit some earlier wave set needs no atomic (a stale read only repeats one): a full 4K frame of a few draws
        // otherwise sends 130 000 atomics to one word
        const uint32_t bit = 1u << ((id - 1u) & 31u);
        uint32_t* word = &bits[(id - 1u) / 32u];
        // (a device-scope load: read where the atomics land, not from this CU's vector cache)
        if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(word, bit);
    }
}

constexpr int kOutTile = 32;                          // pixels per tile edge
constexpr int kOutHalo = 8;                           // the widest outline (idsel::kMaxOutlineWidth)
constexpr int kOutSpan = kOutTile + 2 * kOutHalo;     // the staged square's edge

struct OutlineArgs {
    const uint32_t* ids;
    const uint32_t* sel;  // ndraws flags
    uint32_t* color;      // the context's first row
    int32_t W, rows, r;
    uint32_t ndraws;
    float rgba[4];
};

__global__ __launch_bounds__(TRI_BLOCK) void k_id_outline(OutlineArgs a) {
    __shared__ uint8_t s[kOutSpan * kOutSpan];   // S over the tile and its halo of r pixels
    __shared__ uint8_t hs[kOutSpan * kOutTile];  // per staged row: OR of S over the 2r + 1 columns around each tile column
    const int tid = threadIdx.x;
    const int32_t r = a.r, span = kOutTile + 2 * r;
    const int32_t tx0 = (int32_t)blockIdx.x * kOutTile, ty0 = (int32_t)blockIdx.y * kOutTile;
    int any = 0;
    for (int i = tid; i < span * span; i += TRI_BLOCK) {
        const int32_t ly = i / span, lx = i - ly * span;
        const int32_t x = tx0 - r + lx, y = ty0 - r + ly;
        uint8_t v = 0;
        if (x >= 0 && x < a.W && y >= 0 && y < a.rows) {  // pixels outside the rendered rows select nothing
            const uint32_t id = a.ids[(size_t)y * (size_t)a.W + (size_t)x];
            if (id >= 1u && id - 1u < a.ndraws) v = a.sel[id - 1u] != 0u ? 1 : 0;
        }
        s[ly * kOutSpan + lx] = v;
        any |= v;
    }
    if (!__syncthreads_or(any)) return;  // (uniform) no selected pixel within reach of this tile
    for (int i = tid; i < span * kOutTile; i += TRI_BLOCK) {
        const int32_t ly = i / kOutTile, lx = i - ly * kOutTile;
        uint8_t v = 0;
        for (int32_t k = 0; k <= 2 * r; ++k) v |= s[ly * kOutSpan + lx + k];
        hs[ly * kOutTile + lx] = v;
    }
    __syncthreads();
    const float sr = fminf(fmaxf(a.rgba[0], 0.0f), 1.0f), sg = fminf(fmaxf(a.rgba[1], 0.0f), 1.0f),
                sb = fminf(fmaxf(a.rgba[2], 0.0f), 1.0f), sa = fminf(fmaxf(a.rgba[3], 0.0f), 1.0f);
    if (sa == 0.0f) return;  // reproduces dst exactly
    for (int i = tid; i < kOutTile * kOutTile; i += TRI_BLOCK) {
        const int32_t ly = i / kOutTile, lx = i - ly * kOutTile;
        const int32_t x = tx0 + lx, y = ty0 + ly;
        if (x >= a.W || y >= a.rows) continue;
        if (s[(ly + r) * kOutSpan + lx + r]) continue;  // a selected pixel is not an outline pixel
        uint8_t v = 0;
        for (int32_t k = 0; k <= 2 * r; ++k) v |= hs[(ly + k) * kOutTile + lx];
        if (!v) continue;
        const size_t o = (size_t)y * (size_t)a.W + (size_t)x;
        const uint32_t p = a.color[o];
        // k_text_overlay's blend (text_overlay.hip) for a pixel of coverage 1
        const float db = (float)(p & 0xFFu) / 255.0f, dg = (float)((p >> 8) & 0xFFu) / 255.0f,
                    dr = (float)((p >> 16) & 0xFFu) / 255.0f, da = (float)(p >> 24) / 255.0f;
        const float om = 1.0f - sa;
        const float ob = sb * sa + db * om, og = sg * sa + dg * om, orr = sr * sa + dr * om;
        const float oa = sa + da * om;  // ONE / ONE_MINUS_SRC_ALPHA
        a.color[o] = unorm8(ob) | (unorm8(og) << 8) | (unorm8(orr) << 16) | (unorm8(oa) << 24);
    }
}

}  // namespace

const void* tri_id_raster_kernel(const TriFrameParams& fp) {
    return fp.bin_log2 == 5   ? reinterpret_cast<const void*>(k_id_raster<5>)
           : fp.bin_log2 == 4 ? reinterpret_cast<const void*>(k_id_raster<4>)
                              : reinterpret_cast<const void*>(k_id_raster<6>);
}

hipError_t tri_launch_id_collect(const uint32_t* ids, int32_t W, int32_t x0, int32_t row0, int32_t w, int32_t h,
                                 uint32_t* bits, uint32_t nwords, hipStream_t stream) {
    if (w <= 0 || h <= 0 || !nwords) return hipSuccess;
    const uint64_t px = (uint64_t)w * (uint64_t)h;
    hipLaunchKernelGGL(k_id_collect, dim3((uint32_t)((px + TRI_BLOCK - 1) / TRI_BLOCK)), dim3(TRI_BLOCK), 0, stream, ids, W,
                       x0, row0, w, h, bits, nwords);
    return hipGetLastError();
}

hipError_t tri_launch_id_outline(const uint32_t* ids, const uint32_t* sel, uint32_t ndraws, uint32_t* color, int32_t W,
                                 int32_t rows, int32_t r, const float rgba[4], hipStream_t stream) {
    if (r < 1 || r > kOutHalo) return hipErrorInvalidValue;
    OutlineArgs a;
    a.ids = ids; a.sel = sel; a.color = color;
    a.W = W; a.rows = rows; a.r = r;
    a.ndraws = ndraws;
    for (int k = 0; k < 4; ++k) a.rgba[k] = rgba[k];
    const dim3 g((uint32_t)((W + kOutTile - 1) / kOutTile), (uint32_t)((rows + kOutTile - 1) / kOutTile));
    hipLaunchKernelGGL(k_id_outline, g, dim3(TRI_BLOCK), 0, stream, a);
    return hipGetLastError();
}
