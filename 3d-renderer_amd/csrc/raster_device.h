// raster_device.h — device code shared by the three kernel translation units (vertex_stage.hip, raster_kernels.hip,
// raster_plain.hip): the diagnostics plumbing, the launch-argument binding, buffer-resource loads, the frame-mode
// predicates, the snapped-vertex accessors and the small helpers that more than one stage uses. Everything else
// lives with its stage: vertex_stage.hip (Default.vert), raster_kernels.hip (set-up, clipping, the shadow kernels,
// the blit, the frame plan), raster_bin.h (coverage and Default.frag: one bin of a k_raster* kernel).
//
// Raster rules (shared with oracle/tri_oracle.cpp) are reproduced with the same float evaluation
// order; the units are compiled with -ffp-contract=off so depth is bit-exact.
#pragma once

#ifndef TRI_KERNEL_TU
#error "raster_device.h: define TRI_KERNEL_TU before the first include (raster_launch.h's address-space qualifier)"
#endif
#include "raster_launch.h"

#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

// LLVM's structured / scalar buffer loads, bound by name (declared at namespace scope: they have no definition)
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x3v __attribute__((ext_vector_type(3)));
__device__ u32x4v tri_sbuf_load_b128(__amdgpu_buffer_rsrc_t r, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.ptr.buffer.load.v4i32");
__device__ u32x3v tri_sbuf_load_b96(__amdgpu_buffer_rsrc_t r, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.ptr.buffer.load.v3i32");
__device__ u32x4v tri_s_buffer_load_v4(u32x4v rsrc, int offset, int aux) __asm("llvm.amdgcn.s.buffer.load.v4i32");

namespace {

// Diagnostics builds only (tools/build_variant.sh NAME -DTRI_ABLATE=N): 1 = coverage without shading,
// 2 = shading without coverage, 4 = set-up without binning, 8 = one reservation round per batch,
// 16 = no reservation atomics, 32 = no queue stores, 64 = no lights, 128 = no texture sample, 256 = no varyings
// fetch, 1024 = no fragment colour gathers, 2048 = no shadow lookup (and the fast weights); 512 is unused. The shipped
// library is built with 0, so none of these tests survives into its ISA.
#ifndef TRI_ABLATE
#define TRI_ABLATE 0
#endif
constexpr uint32_t kAblate = TRI_ABLATE;
// Diagnostics builds only (-DTRI_DIAG_FRONT=1..3, tri_render): later frames re-raster the first frame's queues, so
// k_raster leaves their counts
#ifdef TRI_DIAG_FRONT
constexpr bool kDiagKeepQueues = true;
#else
constexpr bool kDiagKeepQueues = false;
#endif

// Diagnostics builds only (-DTRI_PHASE_TIMING): k_raster's wave 0 of every workgroup stamps s_memtime at
// its phase boundaries (start, init, coverage, large triangles, shading, end) for tools/phase_times.py.
// Diagnostics builds only (-DTRI_PRIM_GROUPS): the shading loop counts, per wave-iteration, the distinct primitives
// among its shaded lanes (tools/prim_groups.py): {iterations, distinct primitives, shaded lanes}.
#ifdef TRI_PRIM_GROUPS
__device__ unsigned long long g_tri_groups[3];
#endif
#ifdef TRI_PHASE_TIMING
constexpr int kPhaseSlots = 65536;
__device__ unsigned long long g_tri_phase[kPhaseSlots][6];
#define TRI_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < kPhaseSlots) g_tri_phase[blockIdx.x][k] = __builtin_amdgcn_s_memtime(); } while (0)
// k_setup: start, primitives of the first round set up, first round binned, end
__device__ unsigned long long g_tri_setup_phase[kPhaseSlots][4];
#define TRI_SSTAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < kPhaseSlots) g_tri_setup_phase[blockIdx.x][k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define TRI_STAMP(k) do { } while (0)
#define TRI_SSTAMP(k) do { } while (0)
#endif

// Launch arguments (raster_launch.h): the frame's first kernel takes TriLaunchArgs by value and publishes it
// (TRI_FIRST_KARGS / TRI_PUBLISH_ARGS); the later kernels read the published copy through a read-only,
// non-aliased pointer (TRI_KARGS / TRI_BIND_ARGS: scalar loads).
#define TRI_FIRST_KARGS TriLaunchArgs a_, TriLaunchArgs* __restrict__ pub_
#define TRI_BIND_FIRST_ARGS                   \
    const TriFrameParams& fp = a_.fp;         \
    const TriDeviceBuffers& b = a_.b
#define TRI_KARGS const TriLaunchArgs* __restrict__ args_
#define TRI_BIND_ARGS                         \
    const TriFrameParams& fp = args_->fp;     \
    const TriDeviceBuffers& b = args_->b
// Workgroup 0 of the first kernel copies its by-value arguments to the device copy, 16 B per lane.
__device__ __forceinline__ void publish_args(const TriLaunchArgs& a, TriLaunchArgs* dst) {
    if (blockIdx.x != 0) return;
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const u4* src = reinterpret_cast<const u4*>(&a);
    u4* d = reinterpret_cast<u4*>(dst);
    for (uint32_t i = threadIdx.x; i < sizeof(TriLaunchArgs) / 16; i += blockDim.x) d[i] = src[i];
}

__device__ __forceinline__ int find_range_lds(const uint32_t* base, int n, uint32_t x) {  // base in LDS
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (base[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int find_range(const uint32_t* base, int n, uint32_t x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (base[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Raw buffer loads for k_raster's per-fragment gathers: a wave-uniform descriptor built from kernel
// arguments (SGPRs) and a 32-bit byte offset per lane, so a 16-byte record is ONE load instruction
// with no 64-bit address arithmetic (the compiler splits a plain struct load into per-field loads
// when fields are used on different paths, and serialises the prim_vs -> vertex chain on it).
// The host keeps every buffer read this way below 4 GiB (ensure_work_buffers).
typedef __amdgpu_buffer_rsrc_t Rsrc;
__device__ __forceinline__ Rsrc make_rsrc(const void* p, uint64_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)(uint32_t)bytes, 0x00020000);
}
__device__ __forceinline__ uint4 ld128(Rsrc r, uint32_t off) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    return make_uint4(v[0], v[1], v[2], v[3]);
}
// Record gathers by index: a structured buffer resource carries the record stride, so a load names its record by
// index (buffer_load ... idxen) and the texture unit forms index * stride + offset; no VALU multiply per address
// (the per-pixel gathers of k_raster otherwise spend seven quarter-rate v_mul_lo_u32 on their x12 / x48 offsets).
// The LLVM intrinsic is bound by name (tri_sbuf_load_*, above): the compiler sees an ordinary buffer load.
// A buffer of `n` records of `stride` bytes (stride < 2^14).
struct RecBuf {
    Rsrc r;
};
__device__ __forceinline__ RecBuf rec_buf(const void* p, uint32_t stride, uint64_t n) {
    return RecBuf{__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)stride, (int)(uint32_t)n, 0x00020000)};
}
template <uint32_t STRIDE>
__device__ __forceinline__ uint4 rec128(const RecBuf& b, uint32_t i, uint32_t off) {  // off: a constant < STRIDE
    const u32x4v v = tri_sbuf_load_b128(b.r, (int)i, (int)off, 0, 0);
    return make_uint4(v[0], v[1], v[2], v[3]);
}
template <uint32_t STRIDE>
__device__ __forceinline__ u32x3v rec96(const RecBuf& b, uint32_t i, uint32_t off) {
    return tri_sbuf_load_b96(b.r, (int)i, (int)off, 0, 0);
}
// The varying record: 48 B {world, u}{N, v}{colour, 0}, or 36 B {world}{N}{colour} on single-draw solid frames
// (TriFrameParams::vary36 — exactly the frames k_raster_plain<.., ONE> shades); vary_obj: no varyings at all, the
// fragment stage reads the draw's own object-space records.
__device__ __forceinline__ bool vary36_mode(const TriFrameParams& fp) { return fp.vary36; }
__device__ __forceinline__ bool obj_mode(const TriFrameParams& fp) { return fp.vary_obj; }
struct F3 {
    float x, y, z;
};
__device__ __forceinline__ F3 ldF3(TRI_G const F3* p) { return F3{p->x, p->y, p->z}; }
__device__ __forceinline__ bool obj48_mode(const TriFrameParams& fp) { return fp.obj48; }

// The main pass's snapped vertex fields: X and Y as exact floats (raster_common.h TriSnap; the outcode is a byte of
// its own, TriDeviceBuffers::oc).
__device__ __forceinline__ float snap_Xf(const TriSnap& s) { return __int_as_float(s.xo); }
__device__ __forceinline__ float snap_Yf(const TriSnap& s) { return __int_as_float(s.y); }
__device__ __forceinline__ int32_t snap_X(const TriSnap& s) { return (int32_t)snap_Xf(s); }
__device__ __forceinline__ int32_t snap_Y(const TriSnap& s) { return (int32_t)snap_Yf(s); }

// ((c0*x + c1*y) + c2*z) + c3*w, column-major, no FMA (matches the oracle bit-for-bit)
__device__ __forceinline__ float4 mat_vec_seq(const float* m, float4 v) {
    float4 r;
    r.x = ((m[0] * v.x + m[4] * v.y) + m[8] * v.z) + m[12] * v.w;
    r.y = ((m[1] * v.x + m[5] * v.y) + m[9] * v.z) + m[13] * v.w;
    r.z = ((m[2] * v.x + m[6] * v.y) + m[10] * v.z) + m[14] * v.w;
    r.w = ((m[3] * v.x + m[7] * v.y) + m[11] * v.z) + m[15] * v.w;
    return r;
}

// Lanes of mask m below this lane (v_mbcnt).
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ int32_t floor_shift8(int32_t v) { return v >> 8; }

// Perspective divide (x * (1/w), one correctly rounded divide), viewport transform
// (Renderer.cpp:5062-5069) and 8-bit sub-pixel snap of one vertex. Mirrors oracle setup_triangle().
__device__ __forceinline__ void snap_compute(const TriFrameParams& fp, float4 c, int32_t& X, int32_t& Y, float& z,
                                             float& iw) {
    iw = 1.0f / c.w;
    const float xd = c.x * iw, yd = c.y * iw;
    z = c.z * iw;
    const float xf = xd * fp.hw + fp.hw;
    const float yf = yd * fp.hh + fp.hh;
    X = (int32_t)rintf(xf * 256.0f);
    Y = (int32_t)rintf(yf * 256.0f);
}

__device__ __forceinline__ uint32_t outcode(const TriFrameParams& fp, float4 c) {
    uint32_t oc = 0;
    if (c.z < 0.0f) oc |= TRI_OC_ZNEG;
    if (c.w - c.z < 0.0f) oc |= TRI_OC_ZFAR;
    if (c.x + c.w < 0.0f) oc |= TRI_OC_XNEG;
    if (c.w - c.x < 0.0f) oc |= TRI_OC_XPOS;
    if (c.y + c.w < 0.0f) oc |= TRI_OC_YNEG;
    if (c.w - c.y < 0.0f) oc |= TRI_OC_YPOS;
    if ((c.w < TRI_WMIN) || (c.z < 0.0f) || (c.x < -fp.gx * c.w) || (c.x > fp.gx * c.w) ||
        (c.y < -fp.gy * c.w) || (c.y > fp.gy * c.w))
        oc |= TRI_OC_CLIP;
    return oc;
}

// A bin queue past its capacity (k_setup's reservations, k_raster's entry count): the sticky flag and the need
__device__ __forceinline__ void note_bin_overflow(const TriDeviceBuffers& b, uint32_t needed) {
    atomicOr(&b.counters->flags, TRI_OVF_BIN_LIST);
    atomicMax(&b.counters->bin_max, needed);
}

__device__ __forceinline__ uint32_t unorm8(float c) {
    const float cc = fminf(fmaxf(c, 0.0f), 1.0f);
    return (uint32_t)(int)(cc * 255.0f + 0.5f);
}

}  // namespace
