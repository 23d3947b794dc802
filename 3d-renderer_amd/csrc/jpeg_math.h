// jpeg_math.h — the plain-C++ part of the Motion-JPEG recorder (include/tri_raster.h "JPEG recording"): the whole
// baseline encoder as inline functions, and the argument rules of its entry points. k_jpeg_blocks / k_jpeg_entropy
// (jpeg_encode.hip), the host encoder (Trident::VideoEncoder, tri_jpeg_header) and host/tools/jpeg_check.cpp compile
// this text; tests/jpeg_ref.py restates it in numpy. Everything is integer arithmetic, so for the same pixels and
// parameters the device, the host and the restatement produce the same bytes. No HIP header is needed; under hipcc
// the functions are marked for both sides.
//
// Frame. Baseline sequential DCT (SOF0), 8 bit, components Y (2 x 2), Cb, Cr (1 x 1): an MCU is 16 x 16 pixels, six
// 8 x 8 blocks in the order Y00 Y01 Y10 Y11 Cb Cr. Extents 1..65535; pixel (x, y) beyond the extent is pixel
// (min(x, W - 1), min(y, H - 1)) (T.81 A.2.4). Alpha is ignored.
//
// Colour. JFIF full-range BT.601 in 16-bit fixed point (the matrix rows times 65536, each row's constants summing to
// 65536 or to 0 exactly), per pixel:
//     Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//     Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//     Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
// All three are within 0..255 for every R, G, B (the largest chroma sum is 2^24 - 1), so nothing is clamped. A chroma
// sample is (c00 + c10 + c01 + c11 + 2) >> 2 over the 2 x 2 pixels' own Cb (Cr), taken after the edge replication.
//
// DCT. s = sample - 128. With K[k] = round(4096 cos(k pi / 16)) = 4096 4017 3784 3406 2896 2276 1567 799 0 and
// C(u, x) = K[4] for u = 0, else +-K[..] for cos((2 x + 1) u pi / 16) (dct_c below): 2^13 times the orthonormal
// DCT-II matrix. Rows first, then columns, every sum in int32 in index order x = 0..7:
//     a[u] = sum_x C(u, x) s[x]          r[u] = (a[u] + 512) >> 10            (3 fraction bits; >> is arithmetic)
//     b[v] = sum_y C(v, y) r[y]                                               (the coefficient times 2^16)
// |a| <= 8 * 4096 * 128 = 2^22, |r| <= 2^12 + 1, |b| <= 8 * 4096 * 4097 < 2^27.1: no overflow, also not with the
// quantiser's half (255 * 2^15 < 2^23) added.
//
// Quantiser. Q = clamp((K_table * s + 50) / 100, 1, 255), s = q < 50 ? 5000 / q : 200 - 2 q (integer divisions), from
// T.81 K.1 (luma) and K.2 (chroma). Round half away from zero: n = (|b| + (Q << 15)) / (Q << 16), the sign of b
// restored; AC clamped to +-1023, DC to -1024..1023 (differences then lie within +-2047: category 11).
//
// Entropy. The Annex K.3 tables. DC: category c of the difference (bit length of its magnitude), then c bits (the
// value, or value + 2^c - 1 when negative). AC in zig-zag order: run / size symbols, ZRL (0xF0) per 16 zeros before
// a non-zero coefficient, EOB (0x00) when the block ends in zeros. Bits go out most significant first; an interval's
// last byte is padded with one-bits; 0xFF is followed by 0x00.
//
// Restart intervals. DRI = R MCUs (restart_mcus, or kDefaultRestartMcus for 0). Interval k holds MCUs k R ..
// min((k + 1) R, total) - 1 in raster order, starts with DC predictions of 0, and is followed by RST(k mod 8) unless
// it is the last one.
//
// Size bound. A DC symbol is at most 11 + 11 bits (chroma category 11), an AC coefficient at most 16 + 10 bits (a ZRL,
// at most 11 bits, stands for 16 coefficients, and EOB replaces at least one), so a block is at most
// kMaxBlockBits = 22 + 63 * 26 = 1660 bits (jpeg_check verifies the two maxima against the built tables), an interval
// of n MCUs at most ceil(6 n * 1660 / 8) bytes before stuffing and twice that after. Every buffer is sized from it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/tri_raster.h"

#if defined(__HIPCC__)
#define TRI_JPEG_FN __host__ __device__ inline
#else
#define TRI_JPEG_FN inline
#endif

namespace jpeg {

constexpr uint32_t kMcu = 16, kBlocksPerMcu = 6, kCoefPerMcu = 384;
constexpr uint32_t kMaxBlockBits = 22 + 63 * 26;
constexpr uint32_t kHeaderBytes = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 6 + 14;  // 629, for every extent
constexpr uint32_t kDefaultQuality = 90;
// measured on the MI355X: one wave encodes an interval 64 blocks at a time, 10 MCUs are 60 blocks
constexpr uint32_t kDefaultRestartMcus = 10;

struct Msg {
    char text[160] = {0};
};

// zig-zag position -> natural (row-major) index
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// T.81 Annex K.1 and K.2, natural order
constexpr uint8_t kLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                  99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// T.81 Annex K.3: BITS (codes per length 1..16) and HUFFVAL, in the order DC luma, DC chroma, AC luma, AC chroma
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
    0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1,
    0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
    0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
    0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};

// What the kernels read (copied to the device once per recorder, then into LDS): the scaled quantisers in natural
// order, each natural index's zig-zag position, and the four code tables as (length << 16) | code per symbol
// (0 for a symbol the table does not have). Table indices: 0 DC luma, 1 DC chroma, 2 AC luma, 3 AC chroma.
struct Tables {
    uint16_t q[2][64];
    uint8_t izz[64];
    uint32_t huff[4][256];
};

// ---- argument rules ------------------------------------------------------------------------------------------------

inline int check_quality(uint32_t quality, Msg& m) {
    if (quality < 1 || quality > 100) {
        std::snprintf(m.text, sizeof m.text, "a quality of %u (1..100)", quality);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}
inline int check_restart(uint32_t restart_mcus, Msg& m) {
    if (restart_mcus > 65535) {
        std::snprintf(m.text, sizeof m.text, "a restart interval of %u MCUs (1..65535, 0 = default)", restart_mcus);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}
inline int check_extent(uint32_t width, uint32_t height, Msg& m) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535) {
        std::snprintf(m.text, sizeof m.text, "an extent of %u x %u (1..65535 each)", width, height);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}
inline int check_params(const tri_record_params* p, Msg& m) {
    if (!p) {
        std::snprintf(m.text, sizeof m.text, "null parameters");
        return TRI_E_INVALID;
    }
    if (p->format != TRI_RECORD_YUV444 && p->format != TRI_RECORD_JPEG420) {
        std::snprintf(m.text, sizeof m.text, "an unknown format %u", p->format);
        return TRI_E_INVALID;
    }
    if (p->flags) {
        std::snprintf(m.text, sizeof m.text, "unknown flag bits 0x%x", p->flags);
        return TRI_E_INVALID;
    }
    if (p->format == TRI_RECORD_JPEG420) {
        if (const int rc = check_quality(p->quality, m)) return rc;
        if (const int rc = check_restart(p->restart_mcus, m)) return rc;
    }
    return TRI_OK;
}

// ---- geometry and the size bound -----------------------------------------------------------------------------------

struct Layout {
    uint32_t width, height;
    uint32_t mcus_x, mcus_y, mcus;  // mcus <= 4096^2 = 2^24
    uint32_t restart;               // DRI
    uint32_t intervals;             // ceil(mcus / restart)
    uint32_t segment_bytes;         // an interval's stride in the scratch: its stuffed worst case, a multiple of 16
};
inline uint32_t interval_bound_bytes(uint32_t mcus) {  // stuffed worst case of `mcus` <= 65535 MCUs (< 2^28)
    const uint64_t bits = (uint64_t)mcus * kBlocksPerMcu * kMaxBlockBits;
    return (uint32_t)(2 * ((bits + 7) / 8));
}
inline Layout make_layout(uint32_t width, uint32_t height, uint32_t restart_mcus) {
    Layout l{};
    l.width = width;
    l.height = height;
    l.mcus_x = (width + kMcu - 1) / kMcu;
    l.mcus_y = (height + kMcu - 1) / kMcu;
    l.mcus = l.mcus_x * l.mcus_y;
    l.restart = restart_mcus ? restart_mcus : kDefaultRestartMcus;
    l.intervals = (l.mcus + l.restart - 1) / l.restart;
    const uint32_t longest = l.restart < l.mcus ? l.restart : l.mcus;
    l.segment_bytes = (interval_bound_bytes(longest) + 15u) & ~15u;
    return l;
}
// The largest complete stream: header, every MCU's stuffed worst case (each interval rounds its bits up to a byte
// before the doubling), an RST per interval but the last, EOI.
inline uint64_t max_bytes(const Layout& l) {
    const uint32_t last = l.mcus - (l.intervals - 1) * l.restart;
    return (uint64_t)kHeaderBytes + (uint64_t)(l.intervals - 1) * (interval_bound_bytes(l.restart) + 2) +
           interval_bound_bytes(last) + 2;
}
inline int check_capacity(uint64_t need, uint64_t capacity, Msg& m) {
    if (capacity < need) {
        std::snprintf(m.text, sizeof m.text, "a capacity of %llu bytes, %llu are needed", (unsigned long long)capacity,
                      (unsigned long long)need);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}

// ---- tables ----------------------------------------------------------------------------------------------------------

inline uint32_t scaled_q(uint32_t base, uint32_t quality) {
    const uint32_t s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const uint32_t q = (base * s + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}
inline void build_huffman(const uint8_t* bits, const uint8_t* vals, uint32_t* table) {
    for (int i = 0; i < 256; ++i) table[i] = 0;
    uint32_t code = 0, k = 0;
    for (uint32_t len = 1; len <= 16; ++len) {
        for (uint32_t i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = (len << 16) | code++;
        code <<= 1;
    }
}
inline void build_tables(uint32_t quality, Tables& t) {
    for (int i = 0; i < 64; ++i) {
        t.q[0][i] = (uint16_t)scaled_q(kLumaQ[i], quality);
        t.q[1][i] = (uint16_t)scaled_q(kChromaQ[i], quality);
        t.izz[kZigzag[i]] = (uint8_t)i;
    }
    build_huffman(kDcLumaBits, kDcVals, t.huff[0]);
    build_huffman(kDcChromaBits, kDcVals, t.huff[1]);
    build_huffman(kAcLumaBits, kAcLumaVals, t.huff[2]);
    build_huffman(kAcChromaBits, kAcChromaVals, t.huff[3]);
}

// ---- the header bytes --------------------------------------------------------------------------------------------

// SOI, APP0 (JFIF 1.01, density 1:1, no thumbnail), DQT luma, DQT chroma, SOF0, DHT x 4, DRI, SOS: kHeaderBytes
// into `out`.
inline uint32_t write_header(const Layout& l, const Tables& t, uint8_t* out) {
    uint8_t* p = out;
    auto put = [&](uint32_t b) { *p++ = (uint8_t)b; };
    auto put16 = [&](uint32_t v) { put(v >> 8); put(v & 255); };
    put16(0xFFD8);
    put16(0xFFE0); put16(16);
    const char jfif[5] = {'J', 'F', 'I', 'F', '\0'};
    for (const char c : jfif) put((uint8_t)c);
    put16(0x0101); put(0); put16(1); put16(1); put(0); put(0);
    for (uint32_t k = 0; k < 2; ++k) {
        put16(0xFFDB); put16(67); put(k);
        for (int i = 0; i < 64; ++i) put(t.q[k][kZigzag[i]]);
    }
    put16(0xFFC0); put16(17); put(8); put16(l.height); put16(l.width); put(3);
    put(1); put(0x22); put(0);
    put(2); put(0x11); put(1);
    put(3); put(0x11); put(1);
    const struct { uint32_t id; const uint8_t *bits, *vals; uint32_t n; } dht[4] = {
        {0x00, kDcLumaBits, kDcVals, 12}, {0x01, kDcChromaBits, kDcVals, 12},
        {0x10, kAcLumaBits, kAcLumaVals, 162}, {0x11, kAcChromaBits, kAcChromaVals, 162}};
    for (const auto& h : dht) {
        put16(0xFFC4); put16(2 + 1 + 16 + h.n); put(h.id);
        for (int i = 0; i < 16; ++i) put(h.bits[i]);
        for (uint32_t i = 0; i < h.n; ++i) put(h.vals[i]);
    }
    put16(0xFFDD); put16(4); put16(l.restart);
    put16(0xFFDA); put16(12); put(3);
    put(1); put(0x00); put(2); put(0x11); put(3); put(0x11);
    put(0); put(63); put(0);
    return (uint32_t)(p - out);
}

// ---- the per-pixel and per-block rule ----------------------------------------------------------------------------

struct Ycc {
    int y, cb, cr;
};
TRI_JPEG_FN Ycc ycc(int r, int g, int b) {
    Ycc o;
    o.y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    o.cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    o.cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
    return o;
}
TRI_JPEG_FN int chroma_mean(int c00, int c10, int c01, int c11) { return (c00 + c10 + c01 + c11 + 2) >> 2; }

// 2^13 times the orthonormal DCT-II matrix entry (u, x).
TRI_JPEG_FN constexpr int dct_c(int u, int x) {
    constexpr int K[9] = {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799, 0};
    if (u == 0) return K[4];
    int m = ((2 * x + 1) * u) & 31;
    if (m > 16) m = 32 - m;
    return m > 8 ? -K[16 - m] : K[m];
}
// One 8-point pass over in[0], in[stride], ...: out[u] = sum_x C(u, x) in[x], unrounded.
TRI_JPEG_FN void dct8(const int* in, int stride, int (&out)[8]) {
    int s[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int x = 0; x < 8; ++x) s[x] = in[x * stride];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int u = 0; u < 8; ++u) {
        int a = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int x = 0; x < 8; ++x) a += dct_c(u, x) * s[x];
        out[u] = a;
    }
}
TRI_JPEG_FN int row_round(int a) { return (a + 512) >> 10; }
// b: the coefficient times 2^16; Q: the scaled quantiser; dc: natural index 0.
TRI_JPEG_FN int quantise(int b, int Q, bool dc) {
    const int mag = b < 0 ? -b : b;
    int n = (mag + (Q << 15)) / (Q << 16);
    if (b < 0) n = -n;
    if (n > 1023) n = 1023;
    const int lo = dc ? -1024 : -1023;
    return n < lo ? lo : n;
}
// An 8 x 8 block of level-shifted samples (row-major) -> quantised coefficients in zig-zag order.
TRI_JPEG_FN void block_coefficients(const int* samples, const uint16_t* q, const uint8_t* izz, int16_t* zz) {
    int rows[64];
    for (int y = 0; y < 8; ++y) {
        int a[8];
        dct8(samples + 8 * y, 1, a);
        for (int u = 0; u < 8; ++u) rows[8 * y + u] = row_round(a[u]);
    }
    for (int x = 0; x < 8; ++x) {
        int b[8];
        dct8(rows + x, 8, b);
        for (int v = 0; v < 8; ++v) zz[izz[8 * v + x]] = (int16_t)quantise(b[v], q[8 * v + x], (8 * v + x) == 0);
    }
}

TRI_JPEG_FN int bit_length(int mag) {  // 0 for 0; mag <= 2047
    int n = 0;
    while (mag) {
        ++n;
        mag >>= 1;
    }
    return n;
}
// The block's symbols, in order, as put(bits, count): each call is one Huffman code with its value bits behind it
// (count <= 26). zz: 64 coefficients in zig-zag order; pred: the component's previous DC in the interval (0 first).
template <class Put>
TRI_JPEG_FN void encode_block(const int16_t* zz, int pred, const uint32_t* dc_table, const uint32_t* ac_table, Put&& put) {
    {
        const int diff = (int)zz[0] - pred;
        const int cat = bit_length(diff < 0 ? -diff : diff);
        const uint32_t h = dc_table[cat];
        const uint32_t v = (uint32_t)(diff < 0 ? diff + (1 << cat) - 1 : diff);
        put(((h & 0xFFFFu) << cat) | v, (h >> 16) + (uint32_t)cat);
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int c = zz[k];
        if (c == 0) {
            ++run;
            continue;
        }
        while (run >= 16) {
            put(ac_table[0xF0] & 0xFFFFu, ac_table[0xF0] >> 16);
            run -= 16;
        }
        const int cat = bit_length(c < 0 ? -c : c);
        const uint32_t h = ac_table[(run << 4) | cat];
        const uint32_t v = (uint32_t)(c < 0 ? c + (1 << cat) - 1 : c);
        put(((h & 0xFFFFu) << cat) | v, (h >> 16) + (uint32_t)cat);
        run = 0;
    }
    if (run) put(ac_table[0] & 0xFFFFu, ac_table[0] >> 16);
}

// ---- the host encoder ----------------------------------------------------------------------------------------------

// Bits into bytes with the stuffing, for one interval after the other. The caller guarantees the capacity (max_bytes).
struct BitWriter {
    uint8_t* p;
    uint32_t acc = 0, n = 0;  // n < 8 bits pending in acc's low bits
    explicit BitWriter(uint8_t* out) : p(out) {}
    void byte(uint32_t b) {
        *p++ = (uint8_t)b;
        if (b == 0xFF) *p++ = 0;
    }
    void put(uint32_t bits, uint32_t count) {
        uint64_t a = ((uint64_t)acc << count) | bits;
        uint32_t m = n + count;
        while (m >= 8) {
            m -= 8;
            byte((uint32_t)(a >> m) & 0xFFu);
        }
        acc = (uint32_t)(a & ((1u << m) - 1u));
        n = m;
    }
    void pad() {
        if (n) put((1u << (8 - n)) - 1u, 8 - n);
    }
    void marker(uint32_t m) {
        *p++ = 0xFF;
        *p++ = (uint8_t)m;
    }
};

// One MCU's level-shifted samples, blocks in MCU order, from 4-byte pixels (rows pitch_bytes apart) whose red, green
// and blue are at byte r_at, 1, b_at of a pixel (B8G8R8A8: 2, 0; R8G8B8A8: 0, 2).
inline void mcu_samples(const uint8_t* pixels, uint32_t pitch_bytes, uint32_t width, uint32_t height, uint32_t r_at,
                        uint32_t b_at, uint32_t mx, uint32_t my, int (&s)[6][64]) {
    int cb[16][16], cr[16][16];
    for (uint32_t y = 0; y < 16; ++y) {
        const uint32_t sy = my * 16 + y < height ? my * 16 + y : height - 1;
        for (uint32_t x = 0; x < 16; ++x) {
            const uint32_t sx = mx * 16 + x < width ? mx * 16 + x : width - 1;
            const uint8_t* px = pixels + (size_t)sy * pitch_bytes + (size_t)sx * 4;
            const Ycc c = ycc(px[r_at], px[1], px[b_at]);
            s[(y >> 3) * 2 + (x >> 3)][(y & 7) * 8 + (x & 7)] = c.y - 128;
            cb[y][x] = c.cb;
            cr[y][x] = c.cr;
        }
    }
    for (uint32_t y = 0; y < 8; ++y)
        for (uint32_t x = 0; x < 8; ++x) {
            s[4][y * 8 + x] = chroma_mean(cb[2 * y][2 * x], cb[2 * y][2 * x + 1], cb[2 * y + 1][2 * x], cb[2 * y + 1][2 * x + 1]) - 128;
            s[5][y * 8 + x] = chroma_mean(cr[2 * y][2 * x], cr[2 * y][2 * x + 1], cr[2 * y + 1][2 * x], cr[2 * y + 1][2 * x + 1]) - 128;
        }
}

// The entropy-coded part behind the header: `coef` holds mcus x 6 x 64 coefficients in zig-zag order. Returns the
// end (EOI included).
inline uint8_t* encode_scan(const int16_t* coef, const Layout& l, const Tables& t, uint8_t* out) {
    BitWriter w(out);
    for (uint32_t k = 0; k < l.intervals; ++k) {
        int pred[3] = {0, 0, 0};
        const uint32_t end = (k + 1) * l.restart < l.mcus ? (k + 1) * l.restart : l.mcus;
        for (uint32_t m = k * l.restart; m < end; ++m)
            for (uint32_t b = 0; b < 6; ++b) {
                const int16_t* zz = coef + ((size_t)m * 6 + b) * 64;
                const uint32_t comp = b < 4 ? 0 : b - 3, tab = comp ? 1 : 0;
                encode_block(zz, pred[comp], t.huff[tab], t.huff[2 + tab], [&](uint32_t bits, uint32_t n) { w.put(bits, n); });
                pred[comp] = zz[0];
            }
        w.pad();
        if (k + 1 < l.intervals) w.marker(0xD0 + (k & 7));
    }
    w.marker(0xD9);
    return w.p;
}

// A whole image. `coef` is scratch of mcus x 384 coefficients, `out` has max_bytes(l). Returns the stream's size.
inline uint64_t encode_image(const uint8_t* pixels, uint32_t pitch_bytes, uint32_t r_at, uint32_t b_at, const Layout& l,
                             const Tables& t, int16_t* coef, uint8_t* out) {
    for (uint32_t my = 0; my < l.mcus_y; ++my)
        for (uint32_t mx = 0; mx < l.mcus_x; ++mx) {
            int s[6][64];
            mcu_samples(pixels, pitch_bytes, l.width, l.height, r_at, b_at, mx, my, s);
            for (uint32_t b = 0; b < 6; ++b)
                block_coefficients(s[b], t.q[b < 4 ? 0 : 1], t.izz, coef + ((size_t)(my * l.mcus_x + mx) * 6 + b) * 64);
        }
    const uint32_t h = write_header(l, t, out);
    return (uint64_t)(encode_scan(coef, l, t, out + h) - out);
}

}  // namespace jpeg
