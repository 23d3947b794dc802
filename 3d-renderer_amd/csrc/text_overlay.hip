// text_overlay.hip — the viewport's text pass (TextRenderer::RecordViewport with Text.vert / Text.frag) as an ordered,
// alpha-blended 2D pass over the B8G8R8A8 colour target, on the device behind the frame (include/tri_raster.h
// "text overlay" states the pass exactly).
//
// Nothing else in this library blends: k_raster is order-free through its depth key. Text is the opposite case — no
// depth, submission order decides — so the pass is built around keeping that order without atomics:
//
//   host (tri_text_build, once per tri_set_text, O(quads), nothing per pixel): snaps every quad's corners
//       (X = rint(x * 256)), resolves mirroring, derives the inclusive pixel box its centres can cover, drops quads
//       that miss the context's rows, and files the rest — in submission order — into one list per screen bin
//       (TRI_TEXT_BIN x TRI_TEXT_BIN pixels) of the union box: a CSR of 16-B references {quad, x box, y box}. A quad
//       large enough to sit in many bins is filed in each; if that would grow the lists beyond 8 references per quad
//       on average (+ 1024: a few screen-filling quads), every bin shares the one full list instead (same kernel,
//       longer scans; the device image stays below 8 references per quad either way). The union of the boxes, in
//       bins, is the launch.
//   k_text_overlay: one 256-thread workgroup per TRI_TEXT_BIN x TRI_TEXT_BIN bin inside the union box; its four waves
//       are independent (no barrier after the workgroup's UNORM decode table is in LDS): wave w owns the bin's rows
//       8w .. 8w + 7, a 32 x 8 strip whose rows are whole 128-B lines, four pixels per lane kept in registers. The
//       wave scans its bin's list
//       TRI_TEXT_SCAN_CHUNK references at a time, one per lane, tests each box against its strip, and takes the ballot:
//       the set bits, walked from the lowest, are the strip's quads in submission order (the ballot is the per-round
//       list, TRI_TEXT_LIST_CAP entries; a strip under more quads simply takes more rounds). Every hit lane fetches
//       its quad's 48-B record into registers at once (the round's records arrive together, one memory latency), and
//       the walk broadcasts one lane's record at a time (v_readlane); every lane then blends the pixels of its four
//       whose centres the quad covers, rounding to UNORM8 after each quad as a ROP does. A strip loads its pixels at
//       its first hit, beside the records, and stores only the pixels some quad covered.
// Cost: colour read + write over the strips under text, 16 B per reference scanned per wave of the bin, the atlas
// taps (L2-resident: a 1024^2 A8 atlas is 1 MiB). DESIGN.md §5h has the measurements and the alternatives.
#include "raster_launch.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

static_assert(TRI_TEXT_SCAN_CHUNK == 64 && TRI_TEXT_LIST_CAP == 64, "one reference per lane, one ballot per round");
static_assert(TRI_TEXT_BIN == 32, "a strip row is 32 pixels: one 128-B line");

namespace {

constexpr uint32_t kTextBlock = 256;
constexpr int32_t kStripRows = 8;  // rows per wave: TRI_TEXT_BIN / 4 waves

struct TextArgs {
    uint32_t* color;  // the context's first row (row y0 of the frame)
    const TriTextQuadDev* quads;
    const uint4* refs;
    const uint2* rows;  // per bin of the launch (row-major over the grid): its references [x, y)
    const uint8_t* atlas;
    int32_t W, y0, y1;  // frame width, the context's rows
    int32_t bx0, by0;   // the launch's first bin
    int32_t aw, ah;     // atlas extent
};

__device__ __forceinline__ uint32_t unorm8(float c) {  // as raster_device.h's
    const float cc = fminf(fmaxf(c, 0.0f), 1.0f);
    return (uint32_t)(int)(cc * 255.0f + 0.5f);
}

// The atlas at (u, v): A8 UNORM (byte / 255), LINEAR, CLAMP_TO_EDGE, level 0 — sample_ai's arithmetic
// (raster_bin.h) on one channel.
__device__ __forceinline__ float sample_atlas(const TextArgs& a, const float* unorm, float u, float v) {
    const float x = u * (float)a.aw - 0.5f, y = v * (float)a.ah - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    const float wa = x - fx, wb = y - fy;
    const int32_t i0 = (int32_t)fminf(fmaxf(fx, -1.0f), 1.0e9f), j0 = (int32_t)fminf(fmaxf(fy, -1.0f), 1.0e9f);
    const int32_t xa = min(max(i0, 0), a.aw - 1), xb = min(max(i0 + 1, 0), a.aw - 1);
    const int32_t ya = min(max(j0, 0), a.ah - 1), yb = min(max(j0 + 1, 0), a.ah - 1);
    const uint8_t* t = a.atlas;
    const float t00 = unorm[t[(size_t)ya * a.aw + xa]], t10 = unorm[t[(size_t)ya * a.aw + xb]];
    const float t01 = unorm[t[(size_t)yb * a.aw + xa]], t11 = unorm[t[(size_t)yb * a.aw + xb]];
    const float l0 = t00 + wa * (t10 - t00), l1 = t01 + wa * (t11 - t01);
    return l0 + wb * (l1 - l0);
}

__device__ __forceinline__ float sat(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// Lane j's value in every lane (j wave-uniform).
__device__ __forceinline__ int32_t bcast(int32_t v, int32_t j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ float bcastf(float v, int32_t j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

__global__ __launch_bounds__(kTextBlock) void k_text_overlay(TextArgs a) {
    // the UNORM8 decode byte / 255.0f (IEEE division) of every byte, once per workgroup: a covered pixel decodes four
    // atlas taps and its four channels per quad, and the divisions were most of the pass's instructions
    __shared__ float unorm[256];
    unorm[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();  // (before any wave leaves: the only barrier)
    const int32_t wave = (int32_t)(threadIdx.x >> 6), lane = (int32_t)(threadIdx.x & 63u);
    const uint2 range = a.rows[blockIdx.y * gridDim.x + blockIdx.x];
    if (range.x >= range.y) return;
    const int32_t sx0 = (a.bx0 + (int32_t)blockIdx.x) * TRI_TEXT_BIN;
    const int32_t sy0 = (a.by0 + (int32_t)blockIdx.y) * TRI_TEXT_BIN + wave * kStripRows;
    // the strip's pixels inside the frame and the context's rows (inclusive)
    const int32_t xlo = sx0, xhi = min(sx0 + TRI_TEXT_BIN - 1, a.W - 1);
    const int32_t ylo = max(sy0, a.y0), yhi = min(sy0 + kStripRows - 1, a.y1 - 1);
    if (xlo > xhi || ylo > yhi) return;  // (whole waves: no barrier follows)

    // lane -> pixels: column lane & 31 of rows (lane >> 5) + 2k: each row of the strip is one 128-B line
    const int32_t x = sx0 + (lane & 31);
    const int32_t cx = x * 256 + 128;
    int32_t py[4];
    bool valid[4];
    uint32_t pix[4] = {0u, 0u, 0u, 0u};
    bool dirty[4] = {false, false, false, false};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        py[k] = sy0 + (lane >> 5) + 2 * k;
        valid[k] = x < a.W && py[k] >= a.y0 && py[k] < a.y1;
    }
    bool loaded = false;

    for (uint32_t base = range.x; base < range.y; base += TRI_TEXT_SCAN_CHUNK) {
        const uint32_t i = base + (uint32_t)lane;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        bool hit = false;
        if (i < range.y) {
            r = a.refs[i];
            hit = (int32_t)(r.y & 0xFFFFu) <= xhi && (int32_t)(r.y >> 16) >= xlo && (int32_t)(r.z & 0xFFFFu) <= yhi &&
                  (int32_t)(r.z >> 16) >= ylo;
        }
        uint64_t m = __ballot(hit);
        TriTextQuadDev mine = {};  // this lane's hit
        if (hit) mine = a.quads[r.x];
        if (m && !loaded) {
            loaded = true;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (valid[k]) pix[k] = a.color[(size_t)(py[k] - a.y0) * (size_t)a.W + (size_t)x];
        }
        while (m) {  // lowest bit first: submission order
            const int32_t j = __builtin_amdgcn_readfirstlane((int32_t)__builtin_ctzll(m));
            m &= m - 1;
            TriTextQuadDev q;  // lane j's record, for the whole wave
            q.X0 = bcast(mine.X0, j); q.Y0 = bcast(mine.Y0, j); q.X1 = bcast(mine.X1, j); q.Y1 = bcast(mine.Y1, j);
            q.u0 = bcastf(mine.u0, j); q.du = bcastf(mine.du, j); q.v0 = bcastf(mine.v0, j); q.dv = bcastf(mine.dv, j);
#pragma unroll
            for (int k = 0; k < 4; ++k) q.rgba[k] = bcastf(mine.rgba[k], j);
            const bool inx = cx >= q.X0 && cx < q.X1;
            const float tx = (float)(cx - q.X0) / (float)(q.X1 - q.X0);
            const float u = q.u0 + tx * q.du;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int32_t cy = py[k] * 256 + 128;
                if (!(valid[k] && inx && cy >= q.Y0 && cy < q.Y1)) continue;
                const float ty = (float)(cy - q.Y0) / (float)(q.Y1 - q.Y0);
                const float v = q.v0 + ty * q.dv;
                const float al = sample_atlas(a, unorm, u, v);
                // Text.frag: outColor = vec4(color.rgb * alpha, color.a * alpha), clamped by the fixed-point attachment
                const float sr = sat(q.rgba[0] * al), sg = sat(q.rgba[1] * al), sb = sat(q.rgba[2] * al),
                            sa = sat(q.rgba[3] * al);
                dirty[k] = true;          // covered (a pixel no quad covers is not written)
                if (sa == 0.0f) continue;  // reproduces dst exactly
                const uint32_t p = pix[k];
                const float db = unorm[p & 0xFFu], dg = unorm[(p >> 8) & 0xFFu], dr = unorm[(p >> 16) & 0xFFu],
                            da = unorm[p >> 24];
                // SRC_ALPHA / ONE_MINUS_SRC_ALPHA on a colour the shader already multiplied by alpha: the colour is
                // multiplied by alpha twice. That is the reference's pipeline state (TextRenderer.cpp:807-837) with
                // its shader, kept as it is.
                const float om = 1.0f - sa;
                const float ob = sb * sa + db * om, og = sg * sa + dg * om, orr = sr * sa + dr * om;
                const float oa = sa + da * om;  // ONE / ONE_MINUS_SRC_ALPHA
                pix[k] = unorm8(ob) | (unorm8(og) << 8) | (unorm8(orr) << 16) | (unorm8(oa) << 24);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (dirty[k]) a.color[(size_t)(py[k] - a.y0) * (size_t)a.W + (size_t)x] = pix[k];
}

// ceil(a / 256) for any sign
inline int32_t ceil256(int64_t a) { return (int32_t)((a + 255) >> 8); }

inline int32_t snap256(float x) {
    // (int32_t)rintf(x * 256): coordinates beyond +-2^21 pixels are pinned there (far outside any frame; keeps the
    // differences of two snapped values inside int32; stated in include/tri_raster.h)
    const float s = std::fmin(std::fmax(x * 256.0f, -536870912.0f), 536870912.0f);
    return (int32_t)std::rint(s);
}

}  // namespace

bool tri_text_quads_finite(const tri_text_quad* q, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        const float* f = &q[i].x0;
        for (int k = 0; k < 8; ++k)
            if (!std::isfinite(f[k])) return false;
    }
    return true;
}

void tri_text_build(const tri_text_quad* quads, uint32_t count, int32_t W, int32_t y0, int32_t y1, TriTextPlan& plan) {
    plan = TriTextPlan{};
    std::vector<TriTextQuadDev> dev;
    std::vector<uint4> box;  // per kept quad: {index in dev, x box, y box, 0}
    dev.reserve(count);
    box.reserve(count);
    int32_t ux0 = INT32_MAX, ux1 = -1, uy0 = INT32_MAX, uy1 = -1;  // union, in bins
    uint64_t filed = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const tri_text_quad& s = quads[i];
        TriTextQuadDev d;
        d.X0 = snap256(s.x0); d.Y0 = snap256(s.y0); d.X1 = snap256(s.x1); d.Y1 = snap256(s.y1);
        float u0 = s.u0, u1 = s.u1, v0 = s.v0, v1 = s.v1;
        if (d.X1 < d.X0) { std::swap(d.X0, d.X1); std::swap(u0, u1); }  // cull NONE: drawn mirrored
        if (d.Y1 < d.Y0) { std::swap(d.Y0, d.Y1); std::swap(v0, v1); }
        // pixel centres px * 256 + 128 in [X0, X1)
        const int32_t px0 = std::max(ceil256((int64_t)d.X0 - 128), 0), px1 = std::min(ceil256((int64_t)d.X1 - 128) - 1, W - 1);
        const int32_t py0 = std::max(ceil256((int64_t)d.Y0 - 128), y0), py1 = std::min(ceil256((int64_t)d.Y1 - 128) - 1, y1 - 1);
        if (px0 > px1 || py0 > py1) continue;  // zero area, or outside the context's rows
        d.u0 = u0; d.du = u1 - u0; d.v0 = v0; d.dv = v1 - v0;
        std::memcpy(d.rgba, s.rgba, sizeof d.rgba);
        box.push_back(make_uint4((uint32_t)dev.size(), (uint32_t)px0 | ((uint32_t)px1 << 16),
                                 (uint32_t)py0 | ((uint32_t)py1 << 16), 0u));
        dev.push_back(d);
        ux0 = std::min(ux0, px0 / TRI_TEXT_BIN); ux1 = std::max(ux1, px1 / TRI_TEXT_BIN);
        uy0 = std::min(uy0, py0 / TRI_TEXT_BIN); uy1 = std::max(uy1, py1 / TRI_TEXT_BIN);
        filed += (uint64_t)(py1 / TRI_TEXT_BIN - py0 / TRI_TEXT_BIN + 1) * (uint64_t)(px1 / TRI_TEXT_BIN - px0 / TRI_TEXT_BIN + 1);
    }
    if (dev.empty()) return;
    const uint32_t nq = (uint32_t)dev.size();
    const uint32_t nbx = (uint32_t)(ux1 - ux0 + 1), nby = (uint32_t)(uy1 - uy0 + 1);
    const uint32_t ncells = nbx * nby;
    std::vector<uint2> rows(ncells);
    std::vector<uint4> refs;
    // the bins of a box, row-major over the launch grid
    auto cells = [&](const uint4& b, auto&& f) {
        const uint32_t bx0 = (b.y & 0xFFFFu) / TRI_TEXT_BIN - (uint32_t)ux0, bx1 = (b.y >> 16) / TRI_TEXT_BIN - (uint32_t)ux0;
        const uint32_t by0 = (b.z & 0xFFFFu) / TRI_TEXT_BIN - (uint32_t)uy0, by1 = (b.z >> 16) / TRI_TEXT_BIN - (uint32_t)uy0;
        for (uint32_t r = by0; r <= by1; ++r)
            for (uint32_t c = bx0; c <= bx1; ++c) f(r * nbx + c);
    };
    if (filed <= 8ull * nq + 1024ull) {  // one list per bin, each in submission order
        std::vector<uint32_t> at(ncells + 1, 0u);
        for (const uint4& b : box) cells(b, [&](uint32_t cell) { ++at[cell + 1]; });
        for (uint32_t c = 0; c < ncells; ++c) at[c + 1] += at[c];
        for (uint32_t c = 0; c < ncells; ++c) rows[c] = make_uint2(at[c], at[c + 1]);
        refs.resize(at[ncells]);
        for (const uint4& b : box) cells(b, [&](uint32_t cell) { refs[at[cell]++] = b; });
    } else {  // many large quads: every bin scans the one full list
        refs = box;
        for (uint32_t c = 0; c < ncells; ++c) rows[c] = make_uint2(0u, nq);
    }
    plan.nquads = nq;
    plan.nrefs = (uint32_t)refs.size();
    plan.bx0 = (uint32_t)ux0; plan.by0 = (uint32_t)uy0;
    plan.nbx = nbx; plan.nby = nby;
    plan.off_refs = (size_t)nq * sizeof(TriTextQuadDev);  // 48 B records: a multiple of 16
    plan.off_rows = plan.off_refs + refs.size() * sizeof(uint4);
    plan.blob.resize(plan.off_rows + rows.size() * sizeof(uint2));
    std::memcpy(plan.blob.data(), dev.data(), plan.off_refs);
    std::memcpy(plan.blob.data() + plan.off_refs, refs.data(), refs.size() * sizeof(uint4));
    std::memcpy(plan.blob.data() + plan.off_rows, rows.data(), rows.size() * sizeof(uint2));
}

hipError_t tri_launch_text(uint32_t* color, int32_t W, int32_t y0, int32_t y1, const TriTextPlan& plan,
                           const uint8_t* d_blob, const uint8_t* atlas, uint32_t aw, uint32_t ah, hipStream_t stream) {
    if (!plan.nquads) return hipSuccess;
    TextArgs a;
    a.color = color;
    a.quads = reinterpret_cast<const TriTextQuadDev*>(d_blob);
    a.refs = reinterpret_cast<const uint4*>(d_blob + plan.off_refs);
    a.rows = reinterpret_cast<const uint2*>(d_blob + plan.off_rows);
    a.atlas = atlas;
    a.W = W; a.y0 = y0; a.y1 = y1;
    a.bx0 = (int32_t)plan.bx0; a.by0 = (int32_t)plan.by0;
    a.aw = (int32_t)aw; a.ah = (int32_t)ah;
    hipLaunchKernelGGL(k_text_overlay, dim3(plan.nbx, plan.nby), dim3(kTextBlock), 0, stream, a);
    return hipGetLastError();
}
