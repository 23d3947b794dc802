// SkyboxLoader.cpp — the skybox cubemaps that are not loose LDR faces: KTX 1 files (SkyboxTextureLoader::LoadFromKtx,
// TextureLoader.cpp:417-563, which the reference parses by hand) and six OpenEXR faces (LoadFromExrFaces, :565-736,
// which the reference reads through tinyexr; here a scanline reader of its own). Both parse untrusted
// files: every read is checked against the end of the buffer (make sky-check runs them over damaged files under the
// address and undefined-behaviour sanitizers).
#include "trident/ModelLoader.h"

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>

namespace Trident {
namespace Loader {

namespace {

namespace fs = std::filesystem;

void LogError(const char* what, const std::string& detail) {
    std::fprintf(stderr, "[Trident][SkyboxLoader] %s: %s\n", what, detail.c_str());
}

bool ReadFileBytes(const std::string& path, std::vector<uint8_t>& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        LogError("cannot open file", path);
        return false;
    }
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

// A bounds-checked little-endian reader over a byte range.
struct Reader {
    const uint8_t* p;
    size_t n, at = 0;
    bool Has(size_t k) const { return k <= n - at; }
    bool Skip(size_t k) {
        if (!Has(k)) return false;
        at += k;
        return true;
    }
    bool U8(uint8_t& v) {
        if (!Has(1)) return false;
        v = p[at++];
        return true;
    }
    bool U32(uint32_t& v) {
        if (!Has(4)) return false;
        v = (uint32_t)p[at] | ((uint32_t)p[at + 1] << 8) | ((uint32_t)p[at + 2] << 16) | ((uint32_t)p[at + 3] << 24);
        at += 4;
        return true;
    }
    bool I32(int32_t& v) {
        uint32_t u;
        if (!U32(u)) return false;
        std::memcpy(&v, &u, 4);
        return true;
    }
    bool U64(uint64_t& v) {
        uint32_t lo, hi;
        if (!U32(lo) || !U32(hi)) return false;
        v = (uint64_t)lo | ((uint64_t)hi << 32);
        return true;
    }
    // a NUL-terminated string of at most `cap` characters
    bool Str(std::string& s, size_t cap = 255) {
        s.clear();
        while (at < n && p[at] != 0 && s.size() <= cap) s.push_back((char)p[at++]);
        if (at >= n || p[at] != 0) return false;
        ++at;
        return true;
    }
};

constexpr uint32_t kKtxLittle = 0x04030201u;
constexpr uint32_t kGlUnsignedByte = 0x1401u, kGlHalfFloat = 0x140Bu, kGlFloat = 0x1406u;
constexpr uint32_t kGlRgba = 0x1908u, kGlSrgb8Alpha8 = 0x8C43u, kGlRgba16f = 0x881Au;

size_t AlignToDword(size_t v) { return (v + 3u) & ~(size_t)3u; }

}  // namespace

// FloatToHalf (TextureLoader.cpp:162-204), rule for rule: 13 mantissa bits are dropped and one is added when the highest
// dropped bit is set, so a tie rounds away from zero (the reference's comment says "nearest even"; its code does not).
uint16_t FloatToHalf(float value) {
    uint32_t bits;
    std::memcpy(&bits, &value, 4);
    const uint32_t sign = (bits >> 16) & 0x8000u;
    const int32_t exponent = (int32_t)((bits >> 23) & 0xFFu) - 127 + 15;
    uint32_t mantissa = bits & 0x7FFFFFu;
    if (exponent <= 0) {
        if (exponent < -10) return (uint16_t)sign;  // underflow: a signed zero
        mantissa |= 0x800000u;
        const uint32_t shift = (uint32_t)(1 - exponent);
        uint16_t denorm = (uint16_t)(mantissa >> (13u + shift));
        if ((mantissa >> (12u + shift)) & 1u) denorm = (uint16_t)(denorm + 1u);
        return (uint16_t)(sign | denorm);
    }
    if (exponent >= 31) return (uint16_t)(sign | 0x7C00u | (mantissa ? 1u : 0u));  // infinity; a NaN keeps one bit
    uint16_t result = (uint16_t)(sign | ((uint32_t)exponent << 10) | (mantissa >> 13));
    if (mantissa & 0x1000u) result = (uint16_t)(result + 1u);
    return result;
}

CubemapTextureData SkyboxTextureLoader::LoadKtxFromMemory(const uint8_t* data, size_t size, const std::string& name) {
    Reader r{data, size};
    uint32_t h[13];  // the 13 words after the 12-byte identifier
    if (!r.Skip(12)) {
        LogError("KTX file is too small to contain a header", name);
        return {};
    }
    for (uint32_t& w : h)
        if (!r.U32(w)) {
            LogError("KTX file is too small to contain a header", name);
            return {};
        }
    const uint32_t endianness = h[0], glType = h[1], glFormat = h[3], glInternalFormat = h[4];
    const uint32_t width = h[6], height = h[7], faces = h[10], levels = h[11], kvBytes = h[12];
    if (endianness != kKtxLittle) {
        LogError("KTX file uses unsupported endianness", name);
        return {};
    }
    if (faces != 6u) {
        LogError("KTX file does not contain 6 faces", name);
        return {};
    }
    if (width == 0u || height == 0u) {
        LogError("KTX file has invalid dimensions", name);
        return {};
    }
    // (deviation: the reference never checks; Vulkan would reject either)
    if (width != height || width > CubemapTextureData::kMaxSize) {
        LogError("KTX cubemap faces must be square and at most 16384 wide", name);
        return {};
    }
    CubemapTextureData out;
    if (glType == kGlUnsignedByte && glInternalFormat == kGlSrgb8Alpha8) {
        out.m_BytesPerPixel = 4;
        out.m_Format = CubemapFormat::Rgba8Srgb;
    } else if (glType == kGlUnsignedByte && glFormat == kGlRgba) {
        out.m_BytesPerPixel = 4;
        out.m_Format = CubemapFormat::Rgba8Unorm;
    } else if ((glType == kGlHalfFloat || glType == kGlFloat) && glInternalFormat == kGlRgba16f) {
        // (GL_FLOAT with RGBA16F still reads 8 bytes per texel: the reference's quirk, kept)
        out.m_BytesPerPixel = 8;
        out.m_Format = CubemapFormat::Rgba16Sfloat;
        out.m_IsHdr = true;
    } else {
        LogError("KTX file uses unsupported pixel format", name);
        return {};
    }
    const uint32_t mips = levels == 0u ? 1u : levels;
    uint32_t maxMips = 1;
    while ((width >> maxMips) != 0u) ++maxMips;
    if (mips > maxMips) {  // (the device's limit: floor(log2(size)) + 1)
        LogError("KTX file has more mip levels than its size allows", name);
        return {};
    }
    if (!r.Skip(kvBytes)) {
        LogError("KTX key/value data runs past the end of the file", name);
        return {};
    }
    out.m_Width = width;
    out.m_Height = height;
    out.m_MipCount = mips;
    out.m_FaceRegions.resize(mips);
    uint32_t w = width;
    for (uint32_t mip = 0; mip < mips; ++mip) {
        uint32_t imageSize = 0;
        if (!r.U32(imageSize)) {
            LogError("KTX file ended unexpectedly while reading a mip level", name);
            return {};
        }
        if (imageSize == 0u) {  // (otherwise ignored, as in the reference)
            LogError("KTX file reported a zero-sized mip level", name);
            return {};
        }
        const size_t levelStart = r.at;
        const size_t faceSize = (size_t)w * w * out.m_BytesPerPixel;
        for (int f = 0; f < 6; ++f) {
            if (!r.Has(faceSize)) {
                LogError("KTX file ended unexpectedly while reading a face", name);
                return {};
            }
            out.m_FaceRegions[mip][f] = CubemapFaceRegion{out.m_PixelData.size(), faceSize};
            out.m_PixelData.insert(out.m_PixelData.end(), data + r.at, data + r.at + faceSize);
            r.at += faceSize;
            if (!r.Skip(AlignToDword(faceSize) - faceSize)) {
                LogError("KTX file missing padding bytes", name);
                return {};
            }
        }
        const size_t consumed = r.at - levelStart;
        if (!r.Skip(AlignToDword(consumed) - consumed)) {
            LogError("KTX file missing mip padding", name);
            return {};
        }
        w = std::max(1u, w / 2u);
    }
    return out;
}

CubemapTextureData SkyboxTextureLoader::LoadFromKtx(const std::string& filePath) {
    std::vector<uint8_t> bytes;
    if (!ReadFileBytes(filePath, bytes)) return {};
    return LoadKtxFromMemory(bytes.data(), bytes.size(), filePath);
}

// ---- OpenEXR faces ----------------------------------------------------------------------------------------------------
namespace {

enum ExrCompression : uint8_t { kExrNone = 0, kExrRle = 1, kExrZips = 2, kExrZip = 3 };
const char* const kExrCodecNames[] = {"NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB"};

struct ExrChannel {
    std::string name;
    int32_t type = 0;  // 0 UINT, 1 HALF, 2 FLOAT
    size_t offset = 0;  // of its samples in an uncompressed scanline
};

bool Refuse(const std::string& what, const std::string& name) {
    LogError(("EXR face refused: " + what).c_str(), name);
    return false;
}

float HalfToFloat(uint16_t h) {
    const uint32_t s = ((uint32_t)h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    uint32_t bits;
    if (e == 0u) {
        const float v = (float)m * 5.9604644775390625e-8f;  // m * 2^-24, exact
        std::memcpy(&bits, &v, 4);
        bits |= s;
    } else if (e == 31u) {
        bits = s | 0x7F800000u | (m << 13);
    } else {
        bits = s | ((e + 112u) << 23) | (m << 13);
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

// the RLE codec's run-length layer: a count byte c, then -c literal bytes (c < 0) or one byte repeated c + 1 times
bool RleDecode(const uint8_t* in, size_t inSize, std::vector<uint8_t>& out, size_t expected) {
    out.clear();
    size_t i = 0;
    while (i < inSize) {
        const int c = (int8_t)in[i++];
        if (c < 0) {
            const size_t k = (size_t)(-c);
            if (k > inSize - i || k > expected - out.size()) return false;
            out.insert(out.end(), in + i, in + i + k);
            i += k;
        } else {
            const size_t k = (size_t)c + 1;
            if (i >= inSize || k > expected - out.size()) return false;
            out.insert(out.end(), k, in[i++]);
        }
    }
    return out.size() == expected;
}

bool ZipDecode(const uint8_t* in, size_t inSize, std::vector<uint8_t>& out, size_t expected) {
    out.resize(expected);
    uLongf got = (uLongf)expected;
    if (uncompress(out.data(), &got, in, (uLong)inSize) != Z_OK) return false;
    return (size_t)got == expected;
}

// the predictor and the byte interleave the RLE and ZIP codecs apply in front of their coder, undone
void Unfilter(std::vector<uint8_t>& buf, std::vector<uint8_t>& scratch) {
    for (size_t i = 1; i < buf.size(); ++i) buf[i] = (uint8_t)(buf[i - 1] + buf[i] - 128);
    scratch.resize(buf.size());
    const size_t half = (buf.size() + 1) / 2;
    for (size_t i = 0; i < buf.size(); ++i) scratch[i] = (i & 1) ? buf[half + i / 2] : buf[i / 2];
    buf.swap(scratch);
}

// One face: width x height RGBA halves (FloatToHalf of every channel), rows top to bottom.
bool DecodeExrFace(const uint8_t* data, size_t size, const std::string& name, uint32_t& width, uint32_t& height,
                   std::vector<uint16_t>& rgba) {
    Reader r{data, size};
    uint32_t magic = 0, version = 0;
    if (!r.U32(magic) || !r.U32(version) || magic != 20000630u) return Refuse("not an OpenEXR file", name);
    if ((version & 0xFFu) != 2u) return Refuse("unknown OpenEXR version", name);
    if (version & 0x200u) return Refuse("tiled images are not read", name);
    if (version & 0x800u) return Refuse("deep images are not read", name);
    if (version & 0x1000u) return Refuse("multi-part files are not read", name);
    const size_t nameCap = (version & 0x400u) ? 255 : 31;
    std::vector<ExrChannel> channels;
    int32_t win[4] = {0, 0, -1, -1};
    uint8_t compression = 255, lineOrder = 255;
    bool haveChannels = false, haveWindow = false;
    for (;;) {
        std::string attr, type;
        if (!r.Str(attr, nameCap)) return Refuse("truncated header", name);
        if (attr.empty()) break;
        int32_t len = 0;
        if (!r.Str(type, nameCap) || !r.I32(len) || len < 0 || !r.Has((size_t)len)) return Refuse("truncated header", name);
        Reader a{data + r.at, (size_t)len};
        r.at += (size_t)len;
        if (attr == "channels") {
            if (type != "chlist") return Refuse("channels attribute of another type", name);
            size_t offset = 0;
            for (;;) {
                ExrChannel c;
                if (!a.Str(c.name, nameCap)) return Refuse("truncated channel list", name);
                if (c.name.empty()) break;
                int32_t xs = 0, ys = 0;
                if (!a.I32(c.type) || !a.Skip(4) || !a.I32(xs) || !a.I32(ys)) return Refuse("truncated channel list", name);
                if (c.type == 0) return Refuse("UINT channels are not read", name);
                if (c.type != 1 && c.type != 2) return Refuse("unknown channel type", name);
                if (xs != 1 || ys != 1) return Refuse("subsampled channels are not read", name);
                if (channels.size() >= 64) return Refuse("more than 64 channels", name);
                c.offset = offset;
                offset += c.type == 1 ? 2 : 4;
                channels.push_back(c);
            }
            haveChannels = true;
        } else if (attr == "compression") {
            if (!a.U8(compression)) return Refuse("truncated header", name);
        } else if (attr == "dataWindow") {
            for (int32_t& v : win)
                if (!a.I32(v)) return Refuse("truncated header", name);
            haveWindow = true;
        } else if (attr == "lineOrder") {
            if (!a.U8(lineOrder)) return Refuse("truncated header", name);
        }
    }
    if (!haveChannels || !haveWindow || compression == 255 || lineOrder == 255) return Refuse("a required attribute is missing", name);
    if (compression > kExrZip) {
        const std::string codec = compression < sizeof kExrCodecNames / sizeof *kExrCodecNames ? kExrCodecNames[compression] : "unknown";
        return Refuse(codec + " compression is not read", name);
    }
    if (lineOrder > 1) return Refuse("random-order scanlines are not read", name);  // (both scanline orders are)
    const int64_t w64 = (int64_t)win[2] - win[0] + 1, h64 = (int64_t)win[3] - win[1] + 1;
    if (w64 <= 0 || h64 <= 0 || w64 > (int64_t)CubemapTextureData::kMaxSize || h64 > (int64_t)CubemapTextureData::kMaxSize)
        return Refuse("zero or over-large dimensions", name);
    if (channels.size() < 3) return Refuse("fewer than three channels", name);
    width = (uint32_t)w64;
    height = (uint32_t)h64;
    size_t sampleBytes = 0;
    for (const ExrChannel& c : channels) sampleBytes += c.type == 1 ? 2 : 4;
    const size_t lineBytes = sampleBytes * width;
    // the first channel whose name begins with R, G, B or A (TextureLoader.cpp:660-690)
    int pick[4] = {-1, -1, -1, -1};
    for (size_t i = 0; i < channels.size(); ++i) {
        const char c0 = channels[i].name[0];
        if (c0 == 'R' && pick[0] < 0) pick[0] = (int)i;
        else if (c0 == 'G' && pick[1] < 0) pick[1] = (int)i;
        else if (c0 == 'B' && pick[2] < 0) pick[2] = (int)i;
        else if (c0 == 'A' && pick[3] < 0) pick[3] = (int)i;
    }
    const uint32_t linesPerChunk = compression == kExrZip ? 16u : 1u;
    const uint32_t chunks = (height + linesPerChunk - 1) / linesPerChunk;
    std::vector<uint64_t> offsets(chunks);
    for (uint64_t& o : offsets)
        if (!r.U64(o)) return Refuse("truncated offset table", name);
    rgba.assign((size_t)width * height * 4, 0);
    std::vector<uint8_t> seen(height, 0), buf, scratch;
    for (uint32_t k = 0; k < chunks; ++k) {
        if (offsets[k] > size) return Refuse("a chunk offset lies past the end of the file", name);
        Reader c{data, size, (size_t)offsets[k]};
        int32_t y = 0, packed = 0;
        if (!c.I32(y) || !c.I32(packed) || packed < 0 || !c.Has((size_t)packed)) return Refuse("truncated chunk", name);
        const int64_t row0 = (int64_t)y - win[1];
        if (row0 < 0 || row0 >= (int64_t)height || row0 % linesPerChunk != 0) return Refuse("a chunk outside the data window", name);
        const uint32_t rows = std::min<uint32_t>(linesPerChunk, height - (uint32_t)row0);
        const size_t expected = lineBytes * rows;
        const uint8_t* src = data + c.at;
        if ((size_t)packed == expected) {  // stored raw (no codec, or the coder did not shrink it)
            buf.assign(src, src + expected);
        } else if (compression == kExrNone || (size_t)packed > expected) {
            return Refuse("a chunk's size contradicts its header", name);
        } else {
            const bool ok = compression == kExrRle ? RleDecode(src, (size_t)packed, buf, expected)
                                                   : ZipDecode(src, (size_t)packed, buf, expected);
            if (!ok) return Refuse("a chunk fails to decode", name);
            Unfilter(buf, scratch);
        }
        for (uint32_t l = 0; l < rows; ++l) {
            const uint32_t row = (uint32_t)row0 + l;
            if (seen[row]) return Refuse("a scanline stored twice", name);
            seen[row] = 1;
            const uint8_t* line = buf.data() + lineBytes * l;
            uint16_t* dst = rgba.data() + (size_t)row * width * 4;
            for (int ch = 0; ch < 4; ++ch) {
                if (pick[ch] < 0) {  // a missing colour channel reads 0, missing alpha 1
                    const uint16_t fill = FloatToHalf(ch == 3 ? 1.0f : 0.0f);
                    for (uint32_t x = 0; x < width; ++x) dst[4 * x + ch] = fill;
                    continue;
                }
                const ExrChannel& e = channels[(size_t)pick[ch]];
                const uint8_t* s = line + e.offset * width;
                for (uint32_t x = 0; x < width; ++x) {
                    float v;
                    if (e.type == 1) {
                        v = HalfToFloat((uint16_t)(s[2 * x] | (s[2 * x + 1] << 8)));
                    } else {
                        const uint32_t b = (uint32_t)s[4 * x] | ((uint32_t)s[4 * x + 1] << 8) | ((uint32_t)s[4 * x + 2] << 16) |
                                           ((uint32_t)s[4 * x + 3] << 24);
                        std::memcpy(&v, &b, 4);
                    }
                    dst[4 * x + ch] = FloatToHalf(v);  // (tinyexr hands the reference floats; every channel goes through this)
                }
            }
        }
    }
    for (uint32_t row = 0; row < height; ++row)
        if (!seen[row]) return Refuse("a scanline is missing", name);
    return true;
}

}  // namespace

bool SkyboxTextureLoader::DecodeExrFaceFromMemory(const uint8_t* data, size_t size, const std::string& name, uint32_t& width,
                                                  uint32_t& height, std::vector<uint16_t>& rgbaHalf) {
    return DecodeExrFace(data, size, name, width, height, rgbaHalf);
}

CubemapTextureData SkyboxTextureLoader::LoadFromExrFaces(const std::array<std::string, 6>& faces) {
    CubemapTextureData out;
    out.m_FaceRegions.resize(1);
    for (int f = 0; f < 6; ++f) {
        std::vector<uint8_t> bytes;
        std::vector<uint16_t> rgba;
        uint32_t w = 0, h = 0;
        if (!ReadFileBytes(faces[f], bytes) || !DecodeExrFace(bytes.data(), bytes.size(), faces[f], w, h, rgba)) return {};
        if (f == 0) {
            out.m_Width = w;
            out.m_Height = h;
        } else if (w != out.m_Width || h != out.m_Height) {
            LogError("EXR cubemap faces must share the same resolution", faces[f]);
            return {};
        }
        const uint8_t* raw = reinterpret_cast<const uint8_t*>(rgba.data());
        out.m_FaceRegions[0][f] = CubemapFaceRegion{out.m_PixelData.size(), rgba.size() * 2};
        out.m_PixelData.insert(out.m_PixelData.end(), raw, raw + rgba.size() * 2);
    }
    if (out.m_Width != out.m_Height) {  // (the reference never checks; Vulkan would reject it)
        LogError("EXR cubemap faces must be square", faces[0]);
        return {};
    }
    out.m_MipCount = 1;
    out.m_BytesPerPixel = 8;
    out.m_IsHdr = true;
    out.m_Format = CubemapFormat::Rgba16Sfloat;
    return out;
}

}  // namespace Loader
}  // namespace Trident
