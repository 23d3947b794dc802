// frame_tensor.hip — B8G8R8A8 -> channels-last RGBA float32 for AI consumers (the frame readback tensor), on the device.
//
// The reference builds the tensor on the host (ResolvePendingReadback, Renderer.cpp:1111-1389): per byte,
// float(byte) * (1.0f / 255.0f), the channels reordered {2, 1, 0, 3} (QuerySwapchainFormatInfo, :253-256). The factor
// is the float 0x3B808081 and the product one fp32 multiply: a division by 255 rounds differently on 126 of the 256
// byte values, so the kernel multiplies. 255 * 0x3B808081 rounds to exactly 1.0f.
//
//   k_bgra_to_rgba_f32<true, .>   one lane = one pixel: a 4-B load, four byte-to-float conversions, four multiplies
//                                 and one 16-B store. Consecutive lanes own consecutive pixels, so a wave reads 256 B
//                                 and writes 1 KiB contiguous per instruction. Needs a 16-B aligned output.
//   k_bgra_to_rgba_f32<false, .>  one lane = one float of the output, for an output that is only 4-B aligned: lane e
//                                 reads the dword of pixel e / 4 (four lanes share it), converts channel e % 4 and
//                                 stores one dword. A wave writes 256 B contiguous per instruction.
// The second parameter says whether the rows are pitched (the pixel's row is found by a division) or the image is one
// tightly packed run. Every lane handles kTensorUnroll items a block's width apart (all loads first, then the stores),
// so each instruction of a wave still covers one span. A streaming kernel: 20 B per pixel (4 read + 16 written).
#include "raster_launch.h"

#include <hip/hip_runtime.h>

namespace {

constexpr uint32_t kTensorBlock = 256;
constexpr uint32_t kTensorUnroll = 4;
constexpr float kInv255 = 1.0f / 255.0f;
static_assert(__builtin_bit_cast(uint32_t, kInv255) == 0x3B808081u, "1.0f / 255.0f as the reference's compiler folds it");

// The dword of pixel `pixel` of a width-wide image whose rows are pitch_bytes apart (kPitched) or tightly packed.
// Bytes beyond `width` in a pitched row are never addressed.
template <bool kPitched>
__device__ __forceinline__ uint32_t load_pixel(const uint8_t* __restrict__ src, uint32_t width, uint32_t pitch_bytes,
                                               uint32_t pixel) {
    if (!kPitched) return reinterpret_cast<const uint32_t*>(src)[pixel];
    const uint32_t row = pixel / width;
    const uint32_t x = pixel - row * width;
    return *reinterpret_cast<const uint32_t*>(src + (size_t)row * pitch_bytes + (size_t)x * 4u);
}

// `items`: pixels (kVec) or floats (!kVec) of the whole output; dst + items * (kVec ? 4 : 1) floats is its end.
template <bool kVec, bool kPitched>
__global__ __launch_bounds__(kTensorBlock) void k_bgra_to_rgba_f32(const uint8_t* __restrict__ src, uint32_t width,
                                                                   uint32_t pitch_bytes, uint32_t items,
                                                                   float* __restrict__ dst) {
    const uint32_t first = blockIdx.x * (kTensorBlock * kTensorUnroll) + threadIdx.x;
    uint32_t px[kTensorUnroll];
#pragma unroll
    for (uint32_t u = 0; u < kTensorUnroll; ++u) {
        const uint32_t i = first + u * kTensorBlock;
        px[u] = i < items ? load_pixel<kPitched>(src, width, pitch_bytes, kVec ? i : i >> 2) : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < kTensorUnroll; ++u) {
        const uint32_t i = first + u * kTensorBlock;
        if (i >= items) continue;
        if (kVec) {
            float4 o;  // memory order B, G, R, A -> R, G, B, A
            o.x = (float)((px[u] >> 16) & 0xFFu) * kInv255;
            o.y = (float)((px[u] >> 8) & 0xFFu) * kInv255;
            o.z = (float)(px[u] & 0xFFu) * kInv255;
            o.w = (float)(px[u] >> 24) * kInv255;
            reinterpret_cast<float4*>(dst)[i] = o;
        } else {
            const uint32_t c = i & 3u;
            const uint32_t shift = c == 3u ? 24u : 16u - 8u * c;
            dst[i] = (float)((px[u] >> shift) & 0xFFu) * kInv255;
        }
    }
}

}  // namespace

hipError_t tri_launch_bgra_to_rgba_f32(const void* src, uint32_t width, uint32_t height, uint32_t pitch_bytes, float* dst,
                                       hipStream_t stream) {
    if (width == 0 || height == 0) return hipSuccess;
    // a tightly packed image is one row of width * height pixels (<= TRI_MAX_DIM^2 = 2^26): no row to find per pixel
    const bool pitched = pitch_bytes != width * 4u;
    if (!pitched) {
        width *= height;
        height = 1;
    }
    const uint32_t pixels = width * height;  // <= 2^26, so the floats (<= 2^28) fit 32 bits too
    const bool vec = (reinterpret_cast<uintptr_t>(dst) & 15u) == 0;
    const uint32_t items = vec ? pixels : pixels * 4u;
    const uint32_t per_block = kTensorBlock * kTensorUnroll;
    const dim3 grid((items + per_block - 1) / per_block);
    const uint8_t* s = static_cast<const uint8_t*>(src);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kTensorBlock), 0, stream, s, width, pitch_bytes, items, dst);
    };
    if (vec && pitched) launch(k_bgra_to_rgba_f32<true, true>);
    else if (vec) launch(k_bgra_to_rgba_f32<true, false>);
    else if (pitched) launch(k_bgra_to_rgba_f32<false, true>);
    else launch(k_bgra_to_rgba_f32<false, false>);
    return hipGetLastError();
}
