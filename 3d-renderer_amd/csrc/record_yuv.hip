// record_yuv.hip — B8G8R8A8 -> planar YUV 4:4:4 for viewport recording (the Y4M frame payload), on the device.
//
// The reference converts on the host (VideoEncoder::ConvertRgbaToYuv444, VideoEncoder.cpp:701-736): per pixel, in
// double precision and in this operation order,
//     Y =  0.299 R + 0.587 G + 0.114 B
//     U = -0.169 R - 0.331 G + 0.5   B + 128
//     V =  0.5   R - 0.419 G - 0.081 B + 128
// each clamped to [0, 255] and truncated to a byte. The truncated double sum differs from the exact rational floor on
// thousands of RGB triples (and from a float32 evaluation on more), so the kernel does the same IEEE fp64 multiplies
// and adds, unfused (-ffp-contract=off, and the pragma below for this file on its own).
//
//   k_bgra_to_yuv444  one lane = one run of 16 horizontally consecutive pixels: four 16-B loads, 16 x 3 fp64
//                     expressions, the bytes packed into four dwords per plane and written with one 16-B store per
//                     plane (a wave writes 1 KiB contiguous per plane). A run whose plane address is only 4-B aligned
//                     writes four dwords; a ragged run (a row's last 1-15 pixels) or an unaligned plane address writes
//                     bytes. A source run that is not 16-B aligned is read as dwords.
// A streaming kernel: 7 B per pixel (4 read + 3 written), about 17 fp64 operations per pixel.
#include "raster_launch.h"

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kYuvBlock = 256;
constexpr uint32_t kYuvRun = 16;  // pixels per lane

// ClampChannel (VideoEncoder.cpp:701-714): below 0 -> 0, above 255 -> 255, else truncation toward zero.
__device__ __forceinline__ uint32_t yuv_byte(double v) {
    return (uint32_t)(int32_t)fmin(fmax(v, 0.0), 255.0);
}

// One run's bytes of one plane: w[i >> 2] holds pixel i's byte at bits 8 * (i & 3).
__device__ __forceinline__ void store_run(uint8_t* __restrict__ p, const uint32_t (&w)[4], uint32_t n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (n == kYuvRun && (a & 15u) == 0) {
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (n == kYuvRun && (a & 3u) == 0) {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) q[i] = w[i];
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kYuvRun; ++i)
            if (i < n) p[i] = (uint8_t)(w[i >> 2] >> (8u * (i & 3u)));
    }
}

__global__ __launch_bounds__(kYuvBlock) void k_bgra_to_yuv444(const uint8_t* __restrict__ src, uint32_t width,
                                                              uint32_t height, uint32_t pitch_bytes,
                                                              uint8_t* __restrict__ dst, uint32_t runs_per_row) {
    const uint32_t t = blockIdx.x * kYuvBlock + threadIdx.x;
    const uint32_t row = t / runs_per_row;
    if (row >= height) return;
    const uint32_t x0 = (t - row * runs_per_row) * kYuvRun;
    const uint32_t n = min(kYuvRun, width - x0);  // (x0 < width: runs_per_row = ceil(width / 16))
    const uint8_t* s = src + (size_t)row * pitch_bytes + (size_t)x0 * 4u;
    uint32_t px[kYuvRun];
    if (n == kYuvRun && (reinterpret_cast<uintptr_t>(s) & 15u) == 0) {
        const uint4* s4 = reinterpret_cast<const uint4*>(s);
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint4 v = s4[i];
            px[4 * i + 0] = v.x;
            px[4 * i + 1] = v.y;
            px[4 * i + 2] = v.z;
            px[4 * i + 3] = v.w;
        }
    } else {  // a ragged run never reads the bytes beyond `width` in a pitched row
        const uint32_t* s1 = reinterpret_cast<const uint32_t*>(s);
#pragma unroll
        for (uint32_t i = 0; i < kYuvRun; ++i) px[i] = i < n ? s1[i] : 0u;
    }
    uint32_t yw[4] = {}, uw[4] = {}, vw[4] = {};
#pragma unroll
    for (uint32_t i = 0; i < kYuvRun; ++i) {
        const double b = (double)(px[i] & 0xFFu), g = (double)((px[i] >> 8) & 0xFFu), r = (double)((px[i] >> 16) & 0xFFu);
        const double y = 0.299 * r + 0.587 * g + 0.114 * b;
        const double u = -0.169 * r - 0.331 * g + 0.5 * b + 128.0;
        const double v = 0.5 * r - 0.419 * g - 0.081 * b + 128.0;
        const uint32_t sh = 8u * (i & 3u);
        yw[i >> 2] |= yuv_byte(y) << sh;
        uw[i >> 2] |= yuv_byte(u) << sh;
        vw[i >> 2] |= yuv_byte(v) << sh;
    }
    const size_t plane = (size_t)width * height;
    uint8_t* o = dst + (size_t)row * width + x0;
    store_run(o, yw, n);
    store_run(o + plane, uw, n);
    store_run(o + 2 * plane, vw, n);
}

}  // namespace

hipError_t tri_launch_bgra_to_yuv444(const void* src, uint32_t width, uint32_t height, uint32_t pitch_bytes, uint8_t* dst,
                                     hipStream_t stream) {
    if (width == 0 || height == 0) return hipSuccess;
    // a tightly packed image is one row of width * height pixels (<= TRI_MAX_DIM^2 = 2^26): only the plane bases,
    // not every row start, decide the store width then
    if (pitch_bytes == width * 4u) {
        width *= height;
        height = 1;
    }
    const uint32_t runs_per_row = (width + kYuvRun - 1) / kYuvRun;
    const uint64_t threads = (uint64_t)runs_per_row * height;  // <= 2^22 + TRI_MAX_DIM
    const dim3 grid((uint32_t)((threads + kYuvBlock - 1) / kYuvBlock));
    hipLaunchKernelGGL(k_bgra_to_yuv444, grid, dim3(kYuvBlock), 0, stream, static_cast<const uint8_t*>(src), width, height,
                       pitch_bytes, dst, runs_per_row);
    return hipGetLastError();
}
