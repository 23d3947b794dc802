// jpeg_encode.hip — B8G8R8A8 -> a baseline JPEG (4:2:0, restart intervals) on the device, for Motion-JPEG recording.
// The rule is csrc/jpeg_math.h, compiled here and by the host encoder: the bytes are the same from both.
//
//   k_jpeg_blocks   one wave = one 16 x 16 MCU, four MCUs per 256-lane workgroup. A lane loads four pixels of one MCU
//                   row (one 16-B load; per-pixel clamped loads at the right edge and for an unaligned row), converts
//                   them, and the 2 x 2 chroma means come from a lane exchange (the row partner is lane ^ 4). The six
//                   blocks go through LDS twice: 48 lanes do one 8-point row pass each, then one column pass each,
//                   quantise and put the results at their zig-zag positions. Blocks are 8 rows of 9 dwords, 72 per
//                   block: both passes touch 48 distinct banks of the 64 (8 b + 9 r and 8 b + c). The MCU's 768 B of
//                   int16 leave as three coalesced dword stores per lane.
//   k_jpeg_entropy  one wave (a workgroup of its own) = one restart interval, 64 blocks at a time: the blocks'
//                   coefficients come into LDS with 16-B loads, each lane sizes its block (the rule's symbols, lengths
//                   only), a wave scan of the bit counts places it, and the lane ORs its symbols into the batch's bit
//                   buffer in LDS. The whole bytes are then stuffed: per 64 bytes a ballot of the 0xFF bytes places
//                   every byte in the interval's segment of the scratch (byte stores, consecutive lanes consecutive
//                   addresses); up to 7 pending bits carry over to the next batch. The code tables are in LDS.
//   k_jpeg_offsets  one workgroup: the exclusive scan of the intervals' byte counts (each but the last followed by
//                   its 2-byte RSTn) gives every interval's place behind the header; EOI and the size word.
//   k_jpeg_gather   one wave per interval copies its bytes to their place, in dwords once the destination is aligned, and
//                   appends RST(k mod 8).
// No global atomics; every store is bounded by the extent or by jpeg_math.h's size bound (see each store).
#include "jpeg_math.h"
#include "raster_launch.h"

#include <hip/hip_runtime.h>

namespace {

constexpr uint32_t kBlocksWg = 256;  // k_jpeg_blocks: four waves, four MCUs
constexpr uint32_t kBlockPitch = 72;  // dwords per 8 x 8 block in LDS: 8 rows of 9
constexpr uint32_t kBatch = 64;       // k_jpeg_entropy: blocks per pass, one per lane
constexpr uint32_t kCoefPitch = 33;   // dwords per block of 64 int16 in LDS (odd: lanes on distinct banks)
// the batch's bit buffer: 7 carried bits and 64 worst-case blocks, one word of slack for a symbol's second half
constexpr uint32_t kBitWords = (7 + kBatch * jpeg::kMaxBlockBits + 31) / 32 + 1;

__global__ __launch_bounds__(kBlocksWg) void k_jpeg_blocks(const uint8_t* __restrict__ src, uint32_t pitch_bytes, uint32_t width,
                                                           uint32_t height, uint32_t mcus_x, uint32_t mcus,
                                                           const jpeg::Tables* __restrict__ tables, int16_t* __restrict__ coef) {
    __shared__ int s_block[4][6 * kBlockPitch];
    __shared__ int16_t s_zz[4][jpeg::kCoefPerMcu];
    __shared__ uint16_t s_q[2][64];
    __shared__ uint8_t s_izz[64];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    if (t < 128) s_q[t >> 6][t & 63u] = tables->q[t >> 6][t & 63u];
    if (t < 64) s_izz[t] = tables->izz[t];
    const uint32_t mcu = blockIdx.x * 4 + wave;
    const bool live = mcu < mcus;  // (no early return: the barriers below are the workgroup's)
    int* blk = s_block[wave];
    if (live) {
        const uint32_t my = mcu / mcus_x, mx = mcu - my * mcus_x;
        const uint32_t row = lane >> 2, x0 = (lane & 3u) * 4u;
        // edge replication: the row and every column are clamped into the image, so every load is inside it
        const uint32_t sy = min(my * 16 + row, height - 1), sx = mx * 16 + x0;
        const uint8_t* p = src + (size_t)sy * pitch_bytes;
        uint32_t px[4];
        if (sx + 3 < width && ((reinterpret_cast<uintptr_t>(p) + (size_t)sx * 4) & 15u) == 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + (size_t)sx * 4);
            px[0] = v.x; px[1] = v.y; px[2] = v.z; px[3] = v.w;
        } else {
            const uint32_t* p1 = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) px[i] = p1[min(sx + i, width - 1)];
        }
        int cb[4], cr[4];
        const uint32_t ybase = ((row >> 3) * 2 + (x0 >> 3)) * kBlockPitch + (row & 7u) * 9 + (x0 & 7u);
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const jpeg::Ycc c = jpeg::ycc((int)((px[i] >> 16) & 0xFFu), (int)((px[i] >> 8) & 0xFFu), (int)(px[i] & 0xFFu));
            blk[ybase + i] = c.y - 128;
            cb[i] = c.cb;
            cr[i] = c.cr;
        }
        // horizontal pair sums, then the row partner's (rows 2 j and 2 j + 1 are lanes l and l ^ 4)
        const int b0 = cb[0] + cb[1], b1 = cb[2] + cb[3], r0 = cr[0] + cr[1], r1 = cr[2] + cr[3];
        const int pb0 = __shfl_xor(b0, 4), pb1 = __shfl_xor(b1, 4), pr0 = __shfl_xor(r0, 4), pr1 = __shfl_xor(r1, 4);
        if ((row & 1u) == 0) {
            const uint32_t c = (row >> 1) * 9 + (x0 >> 1);
            blk[4 * kBlockPitch + c] = ((b0 + pb0 + 2) >> 2) - 128;
            blk[4 * kBlockPitch + c + 1] = ((b1 + pb1 + 2) >> 2) - 128;
            blk[5 * kBlockPitch + c] = ((r0 + pr0 + 2) >> 2) - 128;
            blk[5 * kBlockPitch + c + 1] = ((r1 + pr1 + 2) >> 2) - 128;
        }
    }
    __syncthreads();
    const uint32_t b = lane >> 3, i = lane & 7u;  // lanes 0..47: block b, row (then column) i
    if (live && lane < 48) {
        int a[8];
        jpeg::dct8(blk + b * kBlockPitch + i * 9, 1, a);
#pragma unroll
        for (int u = 0; u < 8; ++u) blk[b * kBlockPitch + i * 9 + u] = jpeg::row_round(a[u]);
    }
    __syncthreads();
    if (live && lane < 48) {
        int c[8];
        jpeg::dct8(blk + b * kBlockPitch + i, 9, c);
        const uint16_t* q = s_q[b < 4 ? 0 : 1];
#pragma unroll
        for (uint32_t v = 0; v < 8; ++v)
            s_zz[wave][b * 64 + s_izz[v * 8 + i]] = (int16_t)jpeg::quantise(c[v], q[v * 8 + i], v * 8 + i == 0);
    }
    __syncthreads();
    if (live) {
        // mcu < mcus: the MCU's 192 dwords are inside the plane of mcus * 192
        uint32_t* out = reinterpret_cast<uint32_t*>(coef) + (size_t)mcu * (jpeg::kCoefPerMcu / 2);
        const uint32_t* z = reinterpret_cast<const uint32_t*>(s_zz[wave]);
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) out[lane + 64 * k] = z[lane + 64 * k];
    }
}

// OR `count` <= 26 bits into the bit buffer at bit `pos`, most significant first within big-endian dwords.
__device__ __forceinline__ void or_bits(uint32_t* bits, uint32_t pos, uint32_t v, uint32_t count) {
    const uint64_t w = (uint64_t)v << (64u - count - (pos & 31u));
    atomicOr(&bits[pos >> 5], (uint32_t)(w >> 32));
    if ((uint32_t)w) atomicOr(&bits[(pos >> 5) + 1], (uint32_t)w);
}
__device__ __forceinline__ uint32_t bit_byte(const uint32_t* bits, uint32_t j) {
    return (bits[j >> 2] >> (24u - 8u * (j & 3u))) & 0xFFu;
}

__global__ __launch_bounds__(kBatch) void k_jpeg_entropy(const int16_t* __restrict__ coef, uint32_t mcus, uint32_t restart,
                                                         uint32_t segment_bytes, const jpeg::Tables* __restrict__ tables,
                                                         uint8_t* __restrict__ scratch, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_huff[4][256];
    __shared__ uint32_t s_bits[kBitWords];
    __shared__ uint32_t s_coef[kBatch * kCoefPitch];
    const uint32_t lane = threadIdx.x, k = blockIdx.x;  // one workgroup = one wave = interval k < intervals (the grid)
    for (uint32_t i = lane; i < 1024; i += kBatch) (&s_huff[0][0])[i] = (&tables->huff[0][0])[i];
    for (uint32_t i = lane; i < kBitWords; i += kBatch) s_bits[i] = 0;
    const uint32_t first = k * restart, end = min(first + restart, mcus);
    const uint32_t nblocks = (end - first) * 6;
    const int16_t* icoef = coef + (size_t)first * jpeg::kCoefPerMcu;
    uint8_t* seg = scratch + (size_t)k * segment_bytes;
    uint32_t written = 0, carry = 0;  // uniform: bytes in the segment; bits pending at the buffer's start (< 8)
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += kBatch) {
        const uint32_t n = min(kBatch, nblocks - base);
        // the batch's n * 8 16-B pieces, contiguous in the plane (all inside it: base + n <= the interval's blocks)
        const uint4* g = reinterpret_cast<const uint4*>(icoef + (size_t)base * 64);
        for (uint32_t j = lane; j < n * 8; j += kBatch) {
            const uint4 v = g[j];
            uint32_t* d = s_coef + (j >> 3) * kCoefPitch + (j & 7u) * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        __syncthreads();
        const uint32_t blk = base + lane;
        const bool valid = lane < n;
        const int16_t* zz = reinterpret_cast<const int16_t*>(s_coef + lane * kCoefPitch);
        const uint32_t b = blk % 6u;
        const uint32_t tab = b < 4 ? 0u : 1u;
        int pred = 0;
        if (valid) {
            // the component's previous block in the interval: Y01..Y11 follow their neighbour, Y00 the last MCU's Y11,
            // Cb and Cr the last MCU's; none before the interval's first MCU
            const uint32_t back = b == 0 ? 3u : (b < 4 ? 1u : 6u);
            if (blk >= back && !(b == 0 && blk < 6)) pred = icoef[(size_t)(blk - back) * 64];
        }
        uint32_t len = 0;
        if (valid) jpeg::encode_block(zz, pred, s_huff[tab], s_huff[2 + tab], [&](uint32_t, uint32_t c) { len += c; });
        uint32_t incl = len;  // inclusive wave scan
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        uint32_t total = carry + __shfl(incl, 63);
        if (valid) {
            // pos + count <= 7 + 64 * kMaxBlockBits, and the slack word takes a second half: inside s_bits
            uint32_t pos = carry + incl - len;
            jpeg::encode_block(zz, pred, s_huff[tab], s_huff[2 + tab], [&](uint32_t v, uint32_t c) {
                or_bits(s_bits, pos, v, c);
                pos += c;
            });
        }
        __syncthreads();
        const bool last = base + kBatch >= nblocks;
        if (last && (total & 7u)) {  // one-bits to the byte boundary
            const uint32_t padn = 8u - (total & 7u);
            if (lane == 0) or_bits(s_bits, total, (1u << padn) - 1u, padn);
            total += padn;
            __syncthreads();
        }
        const uint32_t nbytes = total >> 3;
        for (uint32_t j0 = 0; j0 < nbytes; j0 += kBatch) {
            const uint32_t j = j0 + lane;
            const bool have = j < nbytes;
            const uint32_t v = have ? bit_byte(s_bits, j) : 0u;
            const bool ff = have && v == 0xFFu;
            const uint64_t mask = __ballot(ff);
            const uint32_t before = __popcll(mask & ((1ull << lane) - 1ull));
            // written + (bytes so far) + (stuffing so far) <= twice the interval's unstuffed bytes <= segment_bytes
            if (have) {
                uint8_t* o = seg + written + lane + before;
                o[0] = (uint8_t)v;
                if (ff) o[1] = 0;
            }
            written += min(kBatch, nbytes - j0) + (uint32_t)__popcll(mask);
        }
        if (!last) {  // the pending bits move to the front of a cleared buffer
            const uint32_t rem = total & 7u;
            const uint32_t part = rem ? bit_byte(s_bits, nbytes) : 0u;
            const uint32_t used = (total + 31) / 32 + 1;
            __syncthreads();
            for (uint32_t i = lane; i < used; i += kBatch) s_bits[i] = 0;
            __syncthreads();
            if (lane == 0) s_bits[0] = part << 24;
            carry = rem;
            __syncthreads();
        }
    }
    if (lane == 0) counts[k] = written;
}

__global__ __launch_bounds__(256) void k_jpeg_offsets(const uint32_t* __restrict__ counts, uint32_t intervals, uint32_t header_bytes,
                                                      uint32_t* __restrict__ offsets, uint8_t* __restrict__ out,
                                                      uint32_t* __restrict__ size_word) {
    __shared__ uint32_t s_scan[256];
    const uint32_t t = threadIdx.x;
    uint32_t run = header_bytes;  // uniform: where the chunk's first interval starts
    for (uint32_t c0 = 0; c0 < intervals; c0 += 256) {
        const uint32_t k = c0 + t;
        const uint32_t mine = k < intervals ? counts[k] + (k + 1 < intervals ? 2u : 0u) : 0u;
        s_scan[t] = mine;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {
            const uint32_t v = t >= d ? s_scan[t - d] : 0u;
            __syncthreads();
            s_scan[t] += v;
            __syncthreads();
        }
        if (k < intervals) offsets[k] = run + s_scan[t] - mine;
        run += s_scan[255];
        __syncthreads();
    }
    if (t == 0) {
        // run <= header + every interval's bound + its RST: the stream's bound less EOI, so both bytes are inside `out`
        out[run] = 0xFF;
        out[run + 1] = 0xD9;
        size_word[0] = run + 2;
    }
}

__global__ __launch_bounds__(256) void k_jpeg_gather(const uint8_t* __restrict__ scratch, uint32_t segment_bytes,
                                                     const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                     uint32_t intervals, uint8_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= intervals) return;
    const uint8_t* s = scratch + (size_t)k * segment_bytes;
    const uint32_t n = counts[k];
    // offsets[k] + n (+ 2) is where the next interval, or EOI, starts: inside the stream's bound
    uint8_t* d = out + offsets[k];
    // up to 3 bytes to the destination's dword boundary, whole dwords (a wave stores 256 contiguous bytes; the source
    // sits at another alignment and is read as bytes), up to 3 bytes behind them: every index is below n
    const uint32_t head = min(n, (uint32_t)((4u - (reinterpret_cast<uintptr_t>(d) & 3u)) & 3u));
    if (lane < head) d[lane] = s[lane];
    const uint32_t words = (n - head) >> 2;
    uint32_t* dw = reinterpret_cast<uint32_t*>(d + head);
    const uint8_t* sb = s + head;
    for (uint32_t j = lane; j < words; j += 64)
        dw[j] = (uint32_t)sb[4 * j] | ((uint32_t)sb[4 * j + 1] << 8) | ((uint32_t)sb[4 * j + 2] << 16) | ((uint32_t)sb[4 * j + 3] << 24);
    const uint32_t done = head + 4 * words;
    if (lane < n - done) d[done + lane] = s[done + lane];
    if (lane == 0 && k + 1 < intervals) {
        d[n] = 0xFF;
        d[n + 1] = (uint8_t)(0xD0u + (k & 7u));
    }
}

}  // namespace

hipError_t tri_launch_jpeg_encode(const tri_jpeg_job& j, hipStream_t stream) {
    const uint32_t mcus_x = (j.width + 15) / 16, mcus = mcus_x * ((j.height + 15) / 16);
    const uint32_t intervals = (mcus + j.restart - 1) / j.restart;
    const jpeg::Tables* tables = static_cast<const jpeg::Tables*>(j.tables);
    hipLaunchKernelGGL(k_jpeg_blocks, dim3((mcus + 3) / 4), dim3(kBlocksWg), 0, stream, static_cast<const uint8_t*>(j.src),
                       j.pitch_bytes, j.width, j.height, mcus_x, mcus, tables, j.coef);
    hipLaunchKernelGGL(k_jpeg_entropy, dim3(intervals), dim3(kBatch), 0, stream, j.coef, mcus, j.restart, j.segment_bytes, tables,
                       j.scratch, j.counts);
    hipLaunchKernelGGL(k_jpeg_offsets, dim3(1), dim3(256), 0, stream, j.counts, intervals, j.header_bytes, j.offsets, j.out,
                       j.size_word);
    hipLaunchKernelGGL(k_jpeg_gather, dim3((intervals + 3) / 4), dim3(256), 0, stream, j.scratch, j.segment_bytes, j.counts,
                       j.offsets, intervals, j.out);
    return hipGetLastError();
}
