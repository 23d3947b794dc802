// raster_plain.hip — k_raster for frames without the shadow pre-pass, in a translation unit of its own so that it
// is compiled without SLP vectorisation and under LLVM's max-ILP scheduler (Makefile): packed-FP32 pairs need their
// uniform operands copied into VGPR pairs, and without them the fast build fits 7 waves/SIMD with no spill (C3
// k_raster 117 -> 112 us). Frames with the pre-pass keep k_raster<.., true> (raster_kernels.hip: SLP, faster there).
//
//   k_raster_plain<EXACT, BL, ONE>   the general and the single-draw solid (ONE) instantiations
//   k_raster_kind*                   ONE's fast build with the frame-uniform switches as constants (frame kinds)
//   k_raster_ai<EXACT, BL>           the general instantiation plus Default.frag's AI frame blend
#define TRI_KERNEL_TU 1  // device pointers in TriDeviceBuffers carry the global address space (raster_launch.h)
#define TRI_PK_SHADE 0   // scalar colour channels (raster_bin.h)
#include "raster_bin.h"

// Tunables (numeric; -D overrides them for A/B builds).
#ifndef TRI_RASTER_WAVES_PLAIN
#define TRI_RASTER_WAVES_PLAIN 7  // k_raster_plain's occupancy target at 16- and 32-px bins: 69 VGPRs, no spill
#endif
// The fast single-draw solid instantiation (C3's) at 8 waves/SIMD: with its parameters read through the frame's
// argument pointer the compiler fills a 7-wave budget (71 VGPRs) where 8 waves fit in 58 with a few SGPRs
// spilled to VGPR lanes.
#ifndef TRI_RASTER_WAVES_PLAIN_ONE
#define TRI_RASTER_WAVES_PLAIN_ONE 8
#endif
// TRI_RASTER_ONE_VGPRS: cap the fast single-draw instantiation's VGPRs below the 64 that 8 waves/SIMD allow, so that a
// concurrent frame's front-end wave (k_setup within 64, TRI_SETUP_WAVES_ONE) fits the register file beside 8 raster
// waves instead of displacing one. On gfx950's unified register file the attribute's value is doubled: 28 caps at 56
// VGPRs; 0 = no cap.
#ifndef TRI_RASTER_ONE_VGPRS
#define TRI_RASTER_ONE_VGPRS 28
#endif
// occupancy and VGPR cap of the 32x32-bin kinds (as TRI_RASTER_WAVES_PLAIN_ONE / TRI_RASTER_ONE_VGPRS above: the
// attribute's value is doubled on gfx950, 0 = no cap). Round 10, same box, two interleaved rounds: at the
// generic instantiation's 56 VGPRs the values held across the loop cost spilled VGPRs (24 B of scratch, a reload per
// pixel) and the constants are read a few at a time (C3 10.49k frames/s, below the parent's 10.85-10.97k); at 64 VGPRs (59 used, no
// scratch) every constant is read in one batch behind the gathers (11.27-11.31k); 7 waves/SIMD with 96 SGPRs and no
// cap 11.17-11.19k.
#ifndef TRI_KIND_WAVES
#define TRI_KIND_WAVES 8
#endif
#ifndef TRI_KIND_VGPRS
#define TRI_KIND_VGPRS 32
#endif

namespace {

template <bool EXACT, int BL, bool ONE>
__global__ __launch_bounds__(TRI_BLOCK) __attribute__((amdgpu_waves_per_eu(BL <= 5 ? ((ONE && !EXACT) ? TRI_RASTER_WAVES_PLAIN_ONE : TRI_RASTER_WAVES_PLAIN) : 3))) void k_raster_plain(TRI_KARGS) {
    TRI_BIND_ARGS;
    raster_bin<EXACT, BL, false, ONE>(fp, b, xcd_bin(blockIdx.x, fp.nbins));
}
#if TRI_RASTER_ONE_VGPRS  // C3's instantiation as an explicit specialization: the cap takes no template-dependent value
template <>
__global__ __launch_bounds__(TRI_BLOCK) __attribute__((amdgpu_waves_per_eu(8))) __attribute__((amdgpu_num_vgpr(TRI_RASTER_ONE_VGPRS))) void k_raster_plain<false, 5, true>(TRI_KARGS) {
    TRI_BIND_ARGS;
    raster_bin<false, 5, false, true>(fp, b, xcd_bin(blockIdx.x, fp.nbins));
}
#endif
// Frame kinds: the fast single-draw instantiation compiled once per combination of the frame-uniform switches its
// pixel loop tests (TRI_KIND_*), for the combinations the benchmark's frames and the common scenes take; every other
// frame keeps k_raster_plain<false, BL, true>. Plain functions, not a template: the register attributes take no
// template-dependent value.
#if TRI_KIND_VGPRS
#define TRI_KIND_VGPR_ATTR __attribute__((amdgpu_num_vgpr(TRI_KIND_VGPRS)))
#else
#define TRI_KIND_VGPR_ATTR
#endif
#define TRI_KIND_KERNEL(NAME, BL, ATTR, KIND)                                                                      \
    __global__ __launch_bounds__(TRI_BLOCK) ATTR void NAME(TRI_KARGS) {                                            \
        TRI_BIND_ARGS;                                                                                             \
        raster_bin<false, BL, false, true, false, (int)(KIND)>(fp, b, xcd_bin(blockIdx.x, fp.nbins));              \
    }
#define TRI_KIND_ATTR5 __attribute__((amdgpu_waves_per_eu(TRI_KIND_WAVES))) TRI_KIND_VGPR_ATTR
#define TRI_KIND_ATTR4 __attribute__((amdgpu_waves_per_eu(TRI_RASTER_WAVES_PLAIN_ONE)))
constexpr uint32_t kKindLit = TRI_KIND_SUN | TRI_KIND_LIGHTS | TRI_KIND_DEPTH;  // a sun, point lights, a depth target
// 32x32 bins: vertex colours under a sun and point lights, with a sampled or a uniform sky, plain or under a TRS draw
TRI_KIND_KERNEL(k_raster_kind5_lit_sky, 5, TRI_KIND_ATTR5, kKindLit | TRI_KIND_SKYQ)
TRI_KIND_KERNEL(k_raster_kind5_lit_sky_xf, 5, TRI_KIND_ATTR5, kKindLit | TRI_KIND_SKYQ | TRI_KIND_XFORM)
TRI_KIND_KERNEL(k_raster_kind5_lit, 5, TRI_KIND_ATTR5, kKindLit)
// 16x16 bins: one vertex colour under point lights alone, a sampled sky
TRI_KIND_KERNEL(k_raster_kind4_ucol_pl_sky, 4, TRI_KIND_ATTR4, TRI_KIND_UCOL | TRI_KIND_LIGHTS | TRI_KIND_DEPTH | TRI_KIND_SKYQ)
// Frames with Default.frag's AI frame blend (AiBlendConfig.w > 0, an uploaded AI frame; never with the shadow
// pre-pass, which the reference does not have): the general instantiation plus the blend
template <bool EXACT, int BL>
__global__ __launch_bounds__(TRI_BLOCK) __attribute__((amdgpu_waves_per_eu(BL <= 5 ? TRI_RASTER_WAVES_PLAIN : 3))) void k_raster_ai(TRI_KARGS) {
    TRI_BIND_ARGS;
    raster_bin<EXACT, BL, false, false, true>(fp, b, xcd_bin(blockIdx.x, fp.nbins));
}

// The frame-kind kernel for the frame's switches at its bin size, or null (no such kind is built)
const void* kind_kernel(int bl, uint32_t kind) {
    auto f = [](auto kernel) { return reinterpret_cast<const void*>(kernel); };
    if (bl == 5) {
        if (kind == (kKindLit | TRI_KIND_SKYQ)) return f(k_raster_kind5_lit_sky);
        if (kind == (kKindLit | TRI_KIND_SKYQ | TRI_KIND_XFORM)) return f(k_raster_kind5_lit_sky_xf);
        if (kind == kKindLit) return f(k_raster_kind5_lit);
    }
    if (bl == 4 && kind == (TRI_KIND_UCOL | TRI_KIND_LIGHTS | TRI_KIND_DEPTH | TRI_KIND_SKYQ)) return f(k_raster_kind4_ucol_pl_sky);
    return nullptr;
}

// The instantiation at bin size 2^BL for (exact, one) — ONE: a single draw over a 1x1 texture slot (the common
// untextured mesh) — or, with `ai`, for the AI blend (the host keeps such frames off ONE's 36-B varyings)
template <int BL>
const void* plain_kernel(bool exact, bool one, bool ai) {
    auto f = [](auto kernel) { return reinterpret_cast<const void*>(kernel); };
    if (ai) return exact ? f(k_raster_ai<true, BL>) : f(k_raster_ai<false, BL>);
    if (one) return exact ? f(k_raster_plain<true, BL, true>) : f(k_raster_plain<false, BL, true>);
    return exact ? f(k_raster_plain<true, BL, false>) : f(k_raster_plain<false, BL, false>);
}

}  // namespace

int tri_raster_kind(const TriFrameParams& fp) {
    // the fast single-draw solid instantiation's frames with object-space varyings, outside the shadow pre-pass and
    // the AI blend, whose colour and depth targets a 32-bit byte offset spans
    if (!(fp.one_draw && fp.shade_solid && fp.vary_obj) || fp.exact_shading || fp.ai_on || fp.shadow_on) return -1;
    if ((uint64_t)fp.W * (uint64_t)(fp.y1 - fp.y0) * 4ull >= (1ull << 32)) return -1;
    const bool sky_on = fp.sky_size != 0;
    const uint32_t kind = (fp.obj_xform ? TRI_KIND_XFORM : 0u) | (fp.obj_ucol ? TRI_KIND_UCOL : 0u) |
                          (fp.sc.has_sun ? TRI_KIND_SUN : 0u) | (fp.write_depth ? TRI_KIND_DEPTH : 0u) |
                          (sky_on && fp.sky_mode != TRI_SKY_UNIFORM ? TRI_KIND_SKYQ : 0u) |
                          (fp.sc.npt ? TRI_KIND_LIGHTS : 0u);
    return kind_kernel(fp.bin_log2, kind) ? (int)kind : -1;
}
const void* tri_raster_plain_kernel(const TriFrameParams& fp) {
    const int kind = tri_raster_kind(fp);
    if (kind >= 0) return kind_kernel(fp.bin_log2, (uint32_t)kind);
    const bool exact = fp.exact_shading != 0, one = fp.one_draw && fp.shade_solid, ai = fp.ai_on != 0;
    return fp.bin_log2 == 5   ? plain_kernel<5>(exact, one, ai)
           : fp.bin_log2 == 4 ? plain_kernel<4>(exact, one, ai)
                              : plain_kernel<6>(exact, one, ai);
}
#ifdef TRI_PRIM_GROUPS
extern "C" int tri_debug_prim_groups(unsigned long long* out3, int reset) {  // k_raster_plain's counts
    if (reset) {
        const unsigned long long z[3] = {0, 0, 0};
        return hipMemcpyToSymbol(HIP_SYMBOL(g_tri_groups), z, sizeof(z)) == hipSuccess ? 0 : -1;
    }
    return hipMemcpyFromSymbol(out3, HIP_SYMBOL(g_tri_groups), 3 * sizeof(unsigned long long), 0,
                               hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
#ifdef TRI_PHASE_TIMING
extern "C" int tri_debug_phase_times(unsigned long long* out, int nslots) {  // k_raster_plain's stamps
    const size_t n = (size_t)(nslots < kPhaseSlots ? nslots : kPhaseSlots) * 6 * sizeof(unsigned long long);
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tri_phase), n, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
