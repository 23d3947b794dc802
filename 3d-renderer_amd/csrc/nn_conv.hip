// nn_conv.hip — the frame generator's convolutions on the f32-input matrix cores (include/tri_raster.h "the frame
// generator"): k_nn_conv, one implicit GEMM for the network's three layer kinds, and tri_nn_conv / tri_nn_pack_weights.
//
// Activations are channels-last float32. A 256-thread block owns a spatial tile of kM = 128 * MB pixels and NT = 32 * NB
// output channels; M = the tile's pixels, N = the channels, K = taps x input channels, walked CK input channels at a
// time. Per K chunk the block stages in LDS
//   the input patch   the tile's footprint with its halo, [pixel][CK + 1] — the odd pixel stride keeps the A reads
//                     (32 consecutive pixels at one channel) on distinct banks; zeros outside the image and beyond Cin;
//   the weight slab   [tap][CK][NT] of the packed weights ([tap][ci][co]): a wave's B read is contiguous in co; zeros
//                     beyond Cin and Cout.
// Each of the four waves owns MB 32-pixel sub-tiles by NB 32-channel sub-tiles, MB * NB = 4 accumulators of
// v_mfma_f32_32x32x2_f32 (A: lane l holds pixel l & 31 at k = l >> 5; B: channel l & 31 at k = l >> 5; D: channel on
// the lane, pixel (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r). The arithmetic is exact float32, a k-ordered fma
// chain per output: taps outer, input channels inner.
//
//   kind        stride  tile (rows x cols)       patch        notes
//   Conv1       1       4 MB x 32                (4MB+2) x 34
//   Conv2       2       16 x 16 (MB 2, CK 8)     33 x 33      output ceil(H/2) x ceil(W/2)
//   ConvT       —       4 MB x 32 of one parity  as Conv1     ConvTranspose2d(4, 2, 1): four 2 x 2-tap convolutions,
//                                                             one per output parity (py, px) in blockIdx.z; output
//                                                             (2s + py, 2t + px) takes input rows s + py - a, a = 0, 1
// Channel counts that are no multiple of the shapes (Cin 4 or 6, Cout 3) are zero-padded in LDS, never in memory.
// Staging loads four channels at a time (VEC) when Cin and Cout are multiples of 4 and the tensors 16-B aligned.
// The epilogue is y = act(acc * scale[c] + shift[c] + res1) + res2, stores 128 B contiguous per pixel and sub-tile.
#include "capi_util.h"
#include "raster_launch.h"
#include "framegen_container.h"

#include <hip/hip_runtime.h>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kConvBlock = 256;
enum ConvKind : int { kConv1 = 0, kConv2 = 1, kConvT = 2 };

struct ConvArgs {
    const float* in;
    const float* w;
    const float* scale;
    const float* shift;
    const float* res1;
    const float* res2;
    float* out;
    int in_h, in_w, cin, cout;
    int grid_h, grid_w;  // the pixels the tiles cover: the output (Conv1, Conv2) or one parity of it = the input (ConvT)
    int out_w;
    int act;
};

template <int KIND, int MB, int NB, int TW, int CK>
struct ConvShape {
    static constexpr int S = KIND == kConv2 ? 2 : 1;
    static constexpr int TH = 128 * MB / TW;
    static constexpr int PH = (TH - 1) * S + 3, PW = (TW - 1) * S + 3;
    static constexpr int CKP = CK + 1;
    static constexpr int NT = 32 * NB;
    static constexpr int TAPS = KIND == kConvT ? 4 : 9;
    static constexpr int PATCH = PH * PW * CKP, SLAB = TAPS * CK * NT;
    static_assert((PATCH + SLAB) * 4 <= 64 * 1024, "static LDS");
    static_assert(MB * NB == 4 && 128 * MB % TW == 0 && CK % 4 == 0, "tile shape");
};

template <int KIND, int MB, int NB, int TW, int CK, bool VEC>
__global__ __launch_bounds__(kConvBlock) void k_nn_conv(const ConvArgs a) {
    using Sh = ConvShape<KIND, MB, NB, TW, CK>;
    constexpr int S = Sh::S, PW = Sh::PW, CKP = Sh::CKP, NT = Sh::NT, TAPS = Sh::TAPS;
    __shared__ float patch[Sh::PATCH];
    __shared__ __attribute__((aligned(16))) float slab[Sh::SLAB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile_x0 = blockIdx.x * TW, tile_y0 = blockIdx.y * Sh::TH;
    int z = blockIdx.z, py = 0, px = 0;
    if (KIND == kConvT) {
        py = (z >> 1) & 1;
        px = z & 1;
        z >>= 2;
    }
    const int n0 = z * NT;
    const int iy0 = tile_y0 * S - 1, ix0 = tile_x0 * S - 1;  // the patch's origin in the input
    const float* __restrict__ wsrc = a.w + (KIND == kConvT ? (size_t)(py * 2 + px) * 4 * a.cin * a.cout : 0);

    int abase[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int p = (wave * MB + m) * 32 + (lane & 31);
        abase[m] = ((p / TW) * S * PW + (p % TW) * S) * CKP + (lane >> 5);
    }
    const int bbase = (lane >> 5) * NT + (lane & 31);

    f32x16 acc[MB][NB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;

    for (int c0 = 0; c0 < a.cin; c0 += CK) {
        __syncthreads();  // the previous chunk's reads are done
        if (VEC) {  // Cin and Cout multiples of 4, 16-B aligned tensors: four channels per load
            for (int i = tid; i < Sh::PH * PW * (CK / 4); i += kConvBlock) {
                const int c = (i % (CK / 4)) * 4, pix = i / (CK / 4);
                const int gy = iy0 + pix / PW, gx = ix0 + pix % PW, ci = c0 + c;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (gy >= 0 && gy < a.in_h && gx >= 0 && gx < a.in_w && ci < a.cin)
                    v = *reinterpret_cast<const float4*>(a.in + ((size_t)gy * a.in_w + gx) * a.cin + ci);
                float* p = patch + pix * CKP + c;  // (the odd pixel stride: four dword stores)
                p[0] = v.x;
                p[1] = v.y;
                p[2] = v.z;
                p[3] = v.w;
            }
            for (int i = tid; i < Sh::SLAB / 4; i += kConvBlock) {
                const int n = (i % (NT / 4)) * 4, c = (i / (NT / 4)) % CK, t = i / ((NT / 4) * CK);
                const int ci = c0 + c, co = n0 + n;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (ci < a.cin && co < a.cout) v = *reinterpret_cast<const float4*>(wsrc + ((size_t)t * a.cin + ci) * a.cout + co);
                *reinterpret_cast<float4*>(slab + 4 * i) = v;
            }
        } else {
        for (int i = tid; i < Sh::PH * PW * CK; i += kConvBlock) {
            const int c = i % CK, pix = i / CK;
            const int gy = iy0 + pix / PW, gx = ix0 + pix % PW, ci = c0 + c;
            float v = 0.0f;
            if (gy >= 0 && gy < a.in_h && gx >= 0 && gx < a.in_w && ci < a.cin)
                v = a.in[((size_t)gy * a.in_w + gx) * a.cin + ci];
            patch[pix * CKP + c] = v;
        }
        for (int i = tid; i < Sh::SLAB; i += kConvBlock) {
            const int n = i % NT, c = (i / NT) % CK, t = i / (NT * CK);
            const int ci = c0 + c, co = n0 + n;
            slab[i] = (ci < a.cin && co < a.cout) ? wsrc[((size_t)t * a.cin + ci) * a.cout + co] : 0.0f;
        }
        }
        __syncthreads();
        const int kmax = min(CK, (a.cin - c0 + 1) & ~1);  // the chunk's channels, to the MFMA's two per step
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int toff = KIND == kConvT ? ((1 + py - (t >> 1)) * PW + (1 + px - (t & 1))) * CKP : ((t / 3) * PW + t % 3) * CKP;
            for (int k = 0; k < kmax; k += 2) {
                float av[MB], bv[NB];
#pragma unroll
                for (int m = 0; m < MB; ++m) av[m] = patch[abase[m] + toff + k];
#pragma unroll
                for (int n = 0; n < NB; ++n) bv[n] = slab[(t * CK + k) * NT + bbase + n * 32];
#pragma unroll
                for (int m = 0; m < MB; ++m)
#pragma unroll
                    for (int n = 0; n < NB; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[n], acc[m][n], 0, 0, 0);
            }
        }
    }

#pragma unroll
    for (int n = 0; n < NB; ++n) {
        const int co = n0 + n * 32 + (lane & 31);
        if (co >= a.cout) continue;
        const float scale = a.scale[co], shift = a.shift[co];
#pragma unroll
        for (int m = 0; m < MB; ++m) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = (wave * MB + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int gy = tile_y0 + p / TW, gx = tile_x0 + p % TW;
                if (gy >= a.grid_h || gx >= a.grid_w) continue;
                const int oy = KIND == kConvT ? 2 * gy + py : gy, ox = KIND == kConvT ? 2 * gx + px : gx;
                const size_t idx = ((size_t)oy * a.out_w + ox) * a.cout + co;
                float v = acc[m][n][r] * scale + shift;
                if (a.res1) v += a.res1[idx];
                if (a.act == (int)TRI_NN_ACT_RELU) v = fmaxf(v, 0.0f);
                else if (a.act == (int)TRI_NN_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
                if (a.res2) v += a.res2[idx];
                a.out[idx] = v;
            }
        }
    }
}

template <int KIND, int MB, int NB, int TW, int CK>
void launch_conv(const ConvArgs& a, hipStream_t stream) {
    using Sh = ConvShape<KIND, MB, NB, TW, CK>;
    const dim3 grid((a.grid_w + TW - 1) / TW, (a.grid_h + Sh::TH - 1) / Sh::TH,
                    ((a.cout + Sh::NT - 1) / Sh::NT) * (KIND == kConvT ? 4 : 1));
    const bool vec = a.cin % 4 == 0 && a.cout % 4 == 0 && (((uintptr_t)a.in | (uintptr_t)a.w) & 15u) == 0;
    if (vec) hipLaunchKernelGGL((k_nn_conv<KIND, MB, NB, TW, CK, true>), grid, dim3(kConvBlock), 0, stream, a);
    else hipLaunchKernelGGL((k_nn_conv<KIND, MB, NB, TW, CK, false>), grid, dim3(kConvBlock), 0, stream, a);
}

// One lane = one pixel: up to four loads, the host path's clamp and round, one dword store.
__global__ __launch_bounds__(256) void k_ai_pack(const float* __restrict__ src, uint64_t pixels, uint32_t channels,
                                                 uint32_t* __restrict__ dst) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    uint32_t packed = 0;
#pragma unroll
    for (uint32_t ch = 0; ch < 4; ++ch) {
        const uint32_t from = (channels >= 3 && ch == 0) ? 2u : (channels >= 3 && ch == 2) ? 0u : ch;
        float v = ch < channels ? src[p * channels + from] : ch == 3 ? 1.0f : 0.0f;
        v = fminf(fmaxf(v, 0.0f), 1.0f);
        packed |= (uint32_t)roundf(v * 255.0f) << (8 * ch);
    }
    dst[p] = packed;
}

}  // namespace

hipError_t tri_launch_nn_conv(const tri_nn_conv_desc& d, const float* in, const float* w, const float* scale,
                              const float* shift, const float* res1, const float* res2, float* out, hipStream_t stream) {
    ConvArgs a;
    a.in = in;
    a.w = w;
    a.scale = scale;
    a.shift = shift;
    a.res1 = res1;
    a.res2 = res2;
    a.out = out;
    a.in_h = (int)d.in_height;
    a.in_w = (int)d.in_width;
    a.cin = (int)d.in_channels;
    a.cout = (int)d.out_channels;
    a.act = (int)d.activation;
    const bool narrow = d.out_channels <= 32;  // one 32-channel sub-tile: the wave's four accumulators go to pixels
    if (d.op == TRI_NN_CONVT4X4) {
        a.grid_h = a.in_h;
        a.grid_w = a.in_w;
        a.out_w = 2 * a.in_w;
        if (narrow) launch_conv<kConvT, 4, 1, 32, 16>(a, stream);
        else launch_conv<kConvT, 2, 2, 32, 16>(a, stream);
    } else if (d.stride == 2) {
        a.grid_h = (a.in_h + 1) / 2;
        a.grid_w = (a.in_w + 1) / 2;
        a.out_w = a.grid_w;
        launch_conv<kConv2, 2, 2, 16, 8>(a, stream);
    } else {
        a.grid_h = a.in_h;
        a.grid_w = a.in_w;
        a.out_w = a.in_w;
        if (narrow) launch_conv<kConv1, 4, 1, 32, 16>(a, stream);
        else launch_conv<kConv1, 2, 2, 32, 16>(a, stream);
    }
    return hipGetLastError();
}

hipError_t tri_launch_ai_pack(const float* src, uint64_t pixels, uint32_t channels, uint32_t* dst, hipStream_t stream) {
    if (pixels == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ai_pack, dim3((uint32_t)((pixels + 255) / 256)), dim3(256), 0, stream, src, pixels, channels, dst);
    return hipGetLastError();
}

namespace {

int check_conv_desc(const char* who, const tri_nn_conv_desc* d) {
    char msg[160];
    if (!d) {
        snprintf(msg, sizeof msg, "%s: null descriptor", who);
        return tri_internal_fail(TRI_E_INVALID, msg);
    }
    const char* what = nullptr;
    if (d->op != TRI_NN_CONV3X3 && d->op != TRI_NN_CONVT4X4) what = "unknown op";
    else if (d->op == TRI_NN_CONVT4X4 ? d->stride != 2 : (d->stride != 1 && d->stride != 2)) what = "unsupported stride";
    else if (d->activation > TRI_NN_ACT_SIGMOID) what = "unknown activation";
    else if (d->in_channels < 1 || d->in_channels > TRI_NN_MAX_CHANNELS || d->out_channels < 1 ||
             d->out_channels > TRI_NN_MAX_CHANNELS)
        what = "channels outside 1..1024";
    else if (d->reserved != 0) what = "reserved must be 0";
    if (what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return tri_internal_fail(TRI_E_INVALID, msg);
    }
    if (const int rc = tri_check_extent(who, d->in_width, d->in_height, "input extent")) return rc;
    if (d->op == TRI_NN_CONVT4X4 && (d->in_width > TRI_MAX_DIM / 2 || d->in_height > TRI_MAX_DIM / 2)) {
        snprintf(msg, sizeof msg, "%s: the transposed convolution's output extent exceeds %d", who, TRI_MAX_DIM);
        return tri_internal_fail(TRI_E_INVALID, msg);
    }
    return TRI_OK;
}

}  // namespace

extern "C" {

int tri_nn_pack_weights(const tri_nn_conv_desc* d, const float* torch_weights, float* packed) {
    if (const int rc = check_conv_desc("tri_nn_pack_weights", d)) return rc;
    if (!torch_weights || !packed) return tri_internal_fail(TRI_E_INVALID, "tri_nn_pack_weights: null pointer");
    fgc::pack_weights(d->op == TRI_NN_CONVT4X4 ? fgc::kConvT4 : fgc::kConv3, d->in_channels, d->out_channels, torch_weights,
                      packed);
    return TRI_OK;
}

int tri_nn_conv(const tri_nn_conv_desc* d, const void* input, const void* packed_weights, const void* scale, const void* shift,
                const void* res1, const void* res2, void* output, void* stream) {
    if (const int rc = check_conv_desc("tri_nn_conv", d)) return rc;
    if (!input || !packed_weights || !scale || !shift || !output)
        return tri_internal_fail(TRI_E_INVALID, "tri_nn_conv: null pointer");
    const uintptr_t bits = (uintptr_t)input | (uintptr_t)packed_weights | (uintptr_t)scale | (uintptr_t)shift |
                           (uintptr_t)res1 | (uintptr_t)res2 | (uintptr_t)output;
    if (bits & 3u) return tri_internal_fail(TRI_E_INVALID, "tri_nn_conv: pointers must be 4-B aligned");
    if (output == input || output == res1 || output == res2)
        return tri_internal_fail(TRI_E_INVALID, "tri_nn_conv: the output may not alias an input");
    auto f = [](const void* p) { return static_cast<const float*>(p); };
    TRI_HIP_TRY(tri_launch_nn_conv(*d, f(input), f(packed_weights), f(scale), f(shift), f(res1), f(res2),
                                   static_cast<float*>(output), static_cast<hipStream_t>(stream)));
    return TRI_OK;
}

}  // extern "C"
