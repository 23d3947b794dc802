// framegen_container.h — the frame generator's weights container, its network plan and the weight re-lay. Plain C++17,
// no HIP: frame_generator.hip includes it, and so does the stand-alone check (host/tools/framegen_check.cpp).
//
// The container (little-endian; tools/export_frame_generator.py writes it, DESIGN 5k describes it):
//     0   char[8]  magic "TRIFGEN\0"
//     8   u32      version (1)
//    12   u32      input channels (1..8)
//    16   u32      tensor count (<= 4096)
//    20   u32[3]   reserved (0)
//    32   tensor count entries of 96 bytes:
//           0  char[64] name, NUL-terminated and NUL-padded: the checkpoint's state_dict key
//          64  u32      rank (1..4)
//          68  u32[4]   dims (each 1..65536; 1 beyond the rank)
//          84  u32      reserved (0)
//          88  u64      offset of the data from the start of the file: a multiple of 4, behind the table
//     then the float32 data of every tensor, row-major.
// Tensors whose name ends in "num_batches_tracked" are ignored, as is every tensor the plan does not name.
//
// The network is the reference's InterpolationUNet (20 convolutions); kFgPlan lists its layers in launch order with
// the buffers frame_generator.hip routes them through.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace fgc {

constexpr uint32_t kVersion = 1, kHeaderBytes = 32, kEntryBytes = 96, kNameBytes = 64;
constexpr uint32_t kMaxTensors = 4096, kMaxDim = 65536, kMaxInputChannels = 8;
constexpr float kBatchNormEps = 1.0e-5f;

enum Op : uint32_t { kConv3 = 0, kConvT4 = 1 };
enum Act : uint32_t { kNone = 0, kRelu = 1, kSigmoid = 2 };
// The activation buffers: the input, four per full- and half-resolution level (A, T, S = the skip, B), three at the
// bottleneck, the output.
enum Buf : int { X, A1, T1, S1, B1, A2, T2, S2, B2, A3, T3, B3, OUT, kBufCount, NONE = -1 };

struct LayerPlan {
    const char* conv;  // the convolution's state_dict prefix
    const char* norm;  // its BatchNorm's prefix, or nullptr: the convolution has a bias
    Op op;
    uint32_t stride;
    uint32_t cin;  // 0: the model's input channels
    uint32_t cout;
    Act act;
    Buf in, out, res1, res2;
    int level;  // of the INPUT: 0 = full resolution, 1 = half, 2 = quarter
};

// y = act(scale * conv(x) + shift + res1) + res2: a residual block's second layer takes the block's input as res1, and a
// decoder stage's last layer the encoder's skip as res2 (added after the block's ReLU, as the reference does).
constexpr LayerPlan kFgPlan[20] = {
    {"m_EncoderStage1.0", nullptr, kConv3, 1, 0, 32, kRelu, X, A1, NONE, NONE, 0},
    {"m_EncoderStage1.2.m_Block.0", "m_EncoderStage1.2.m_Block.1", kConv3, 1, 32, 32, kRelu, A1, T1, NONE, NONE, 0},
    {"m_EncoderStage1.2.m_Block.3", "m_EncoderStage1.2.m_Block.4", kConv3, 1, 32, 32, kRelu, T1, S1, A1, NONE, 0},
    {"m_EncoderStage2.0", nullptr, kConv3, 2, 32, 64, kRelu, S1, A2, NONE, NONE, 0},
    {"m_EncoderStage2.2.m_Block.0", "m_EncoderStage2.2.m_Block.1", kConv3, 1, 64, 64, kRelu, A2, T2, NONE, NONE, 1},
    {"m_EncoderStage2.2.m_Block.3", "m_EncoderStage2.2.m_Block.4", kConv3, 1, 64, 64, kRelu, T2, S2, A2, NONE, 1},
    {"m_EncoderStage3.0", nullptr, kConv3, 2, 64, 128, kRelu, S2, A3, NONE, NONE, 1},
    {"m_EncoderStage3.2.m_Block.0", "m_EncoderStage3.2.m_Block.1", kConv3, 1, 128, 128, kRelu, A3, T3, NONE, NONE, 2},
    {"m_EncoderStage3.2.m_Block.3", "m_EncoderStage3.2.m_Block.4", kConv3, 1, 128, 128, kRelu, T3, B3, A3, NONE, 2},
    {"m_Bottleneck.0.m_Block.0", "m_Bottleneck.0.m_Block.1", kConv3, 1, 128, 128, kRelu, B3, T3, NONE, NONE, 2},
    {"m_Bottleneck.0.m_Block.3", "m_Bottleneck.0.m_Block.4", kConv3, 1, 128, 128, kRelu, T3, A3, B3, NONE, 2},
    {"m_Bottleneck.1.m_Block.0", "m_Bottleneck.1.m_Block.1", kConv3, 1, 128, 128, kRelu, A3, T3, NONE, NONE, 2},
    {"m_Bottleneck.1.m_Block.3", "m_Bottleneck.1.m_Block.4", kConv3, 1, 128, 128, kRelu, T3, B3, A3, NONE, 2},
    {"m_DecodeStage2.0", nullptr, kConvT4, 2, 128, 64, kRelu, B3, A2, NONE, NONE, 2},
    {"m_DecodeStage2.2.m_Block.0", "m_DecodeStage2.2.m_Block.1", kConv3, 1, 64, 64, kRelu, A2, T2, NONE, NONE, 1},
    {"m_DecodeStage2.2.m_Block.3", "m_DecodeStage2.2.m_Block.4", kConv3, 1, 64, 64, kRelu, T2, B2, A2, S2, 1},
    {"m_DecodeStage1.0", nullptr, kConvT4, 2, 64, 32, kRelu, B2, A1, NONE, NONE, 1},
    {"m_DecodeStage1.2.m_Block.0", "m_DecodeStage1.2.m_Block.1", kConv3, 1, 32, 32, kRelu, A1, T1, NONE, NONE, 0},
    {"m_DecodeStage1.2.m_Block.3", "m_DecodeStage1.2.m_Block.4", kConv3, 1, 32, 32, kRelu, T1, B1, A1, S1, 0},
    {"m_OutputLayer.0", nullptr, kConv3, 1, 32, 3, kSigmoid, B1, OUT, NONE, NONE, 0},
};

// Channels of an activation buffer (X: the model's input channels).
constexpr uint32_t buffer_channels(Buf b, uint32_t input_channels) {
    return b == X ? input_channels : b == OUT ? 3u : b <= B1 ? 32u : b <= B2 ? 64u : 128u;
}
constexpr int buffer_level(Buf b) { return (b == X || b == OUT || b <= B1) ? 0 : b <= B2 ? 1 : 2; }

// torch's weights -> the kernels' layout (include/tri_raster.h, tri_nn_pack_weights): the same number of floats.
inline void pack_weights(Op op, uint32_t cin, uint32_t cout, const float* src, float* dst) {
    if (op == kConv3) {  // [co][ci][ky][kx] -> [ky][kx][ci][co]
        for (uint32_t t = 0; t < 9; ++t)
            for (uint32_t ci = 0; ci < cin; ++ci)
                for (uint32_t co = 0; co < cout; ++co)
                    dst[((size_t)t * cin + ci) * cout + co] = src[((size_t)co * cin + ci) * 9 + t];
        return;
    }
    // ConvTranspose2d [ci][co][ky][kx], not flipped: output row 2s + py takes input row s + py - a through ky = 1 - py + 2a
    for (uint32_t py = 0; py < 2; ++py)
        for (uint32_t px = 0; px < 2; ++px)
            for (uint32_t a = 0; a < 2; ++a)
                for (uint32_t b = 0; b < 2; ++b) {
                    const uint32_t ky = 1 - py + 2 * a, kx = 1 - px + 2 * b;
                    const size_t slab = (size_t)(((py * 2 + px) * 2 + a) * 2 + b) * cin * cout;
                    for (uint32_t ci = 0; ci < cin; ++ci)
                        for (uint32_t co = 0; co < cout; ++co)
                            dst[slab + (size_t)ci * cout + co] = src[(((size_t)ci * cout + co) * 4 + ky) * 4 + kx];
                }
}

struct Tensor {
    std::string name;
    uint32_t rank = 0;
    uint32_t dims[4] = {1, 1, 1, 1};
    size_t elements = 0;
    const uint8_t* data = nullptr;  // elements little-endian floats, at any alignment
};

struct Layer {
    std::vector<float> weights;  // packed
    std::vector<float> scale, shift;
    uint32_t cin = 0, cout = 0;
};

struct Model {
    uint32_t input_channels = 0;
    Layer layers[20];
};

namespace detail {
inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }
inline float rdf(const uint8_t* p) {
    const uint32_t u = rd32(p);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
inline bool ends_with(const std::string& s, const char* tail) {
    const size_t n = std::strlen(tail);
    return s.size() >= n && s.compare(s.size() - n, n, tail) == 0;
}
inline bool set(std::string& err, const std::string& msg) {
    err = msg;
    return false;
}
}  // namespace detail

// The table of a container; the tensors point into `file`. False with `err` for a damaged file.
inline bool parse(const uint8_t* file, size_t bytes, uint32_t& input_channels, std::vector<Tensor>& tensors, std::string& err) {
    using namespace detail;
    tensors.clear();
    if (!file || bytes < kHeaderBytes) return set(err, "the container is shorter than its header");
    if (std::memcmp(file, "TRIFGEN\0", 8) != 0) return set(err, "not a frame generator container (magic)");
    if (rd32(file + 8) != kVersion) return set(err, "unsupported container version " + std::to_string(rd32(file + 8)));
    input_channels = rd32(file + 12);
    if (input_channels < 1 || input_channels > kMaxInputChannels)
        return set(err, "input channels " + std::to_string(input_channels) + " outside 1..8");
    const uint32_t count = rd32(file + 16);
    if (count > kMaxTensors) return set(err, "tensor count " + std::to_string(count) + " beyond 4096");
    const size_t table_end = (size_t)kHeaderBytes + (size_t)count * kEntryBytes;
    if (table_end > bytes) return set(err, "the tensor table runs beyond the end of the file (truncated)");
    for (uint32_t i = 0; i < count; ++i) {
        const uint8_t* e = file + kHeaderBytes + (size_t)i * kEntryBytes;
        if (!std::memchr(e, 0, kNameBytes)) return set(err, "tensor " + std::to_string(i) + ": the name is not terminated");
        Tensor t;
        t.name = reinterpret_cast<const char*>(e);
        if (t.name.empty()) return set(err, "tensor " + std::to_string(i) + ": empty name");
        t.rank = rd32(e + 64);
        if (t.rank < 1 || t.rank > 4) return set(err, "tensor " + t.name + ": rank " + std::to_string(t.rank) + " outside 1..4");
        uint64_t n = 1;
        for (uint32_t d = 0; d < 4; ++d) {
            t.dims[d] = rd32(e + 68 + 4 * d);
            if (t.dims[d] < 1 || t.dims[d] > kMaxDim || (d >= t.rank && t.dims[d] != 1))
                return set(err, "tensor " + t.name + ": dimension " + std::to_string(d) + " is " + std::to_string(t.dims[d]) +
                                    " (outside 1..65536)");
            n *= t.dims[d];  // <= 2^64 only at four dims of 2^16: checked against the file below before the fourth matters
            if (n > ((uint64_t)1 << 40)) return set(err, "tensor " + t.name + ": too many elements");
        }
        const uint64_t off = rd64(e + 88);
        if (off & 3u) return set(err, "tensor " + t.name + ": data offset " + std::to_string(off) + " is not a multiple of 4");
        if (off < table_end || off > bytes || n * 4 > bytes - off)
            return set(err, "tensor " + t.name + ": data outside the file (truncated)");
        t.elements = (size_t)n;
        t.data = file + off;
        tensors.push_back(t);
    }
    return true;
}

namespace detail {
inline const Tensor* find(const std::vector<Tensor>& tensors, const std::string& name, std::string& err) {
    for (const Tensor& t : tensors)
        if (t.name == name && !ends_with(t.name, "num_batches_tracked")) return &t;
    err = "tensor " + name + ": missing from the container";
    return nullptr;
}
inline const Tensor* find_vector(const std::vector<Tensor>& tensors, const std::string& name, uint32_t n, std::string& err) {
    const Tensor* t = find(tensors, name, err);
    if (!t) return nullptr;
    if (t->rank != 1 || t->dims[0] != n) {
        err = "tensor " + name + ": expected shape [" + std::to_string(n) + "]";
        return nullptr;
    }
    return t;
}
}  // namespace detail

// The container as the network's 20 layers: shapes checked against the plan, weights packed, bias / BatchNorm folded
// into scale and shift. False with `err` naming the tensor.
inline bool load(const uint8_t* file, size_t bytes, Model& model, std::string& err) {
    using namespace detail;
    std::vector<Tensor> tensors;
    if (!parse(file, bytes, model.input_channels, tensors, err)) return false;
    std::vector<float> raw;
    for (int l = 0; l < 20; ++l) {
        const LayerPlan& p = kFgPlan[l];
        Layer& L = model.layers[l];
        L.cin = p.cin ? p.cin : model.input_channels;
        L.cout = p.cout;
        const std::string wname = std::string(p.conv) + ".weight";
        const Tensor* w = find(tensors, wname, err);
        if (!w) return false;
        const uint32_t k = p.op == kConv3 ? 3 : 4;
        const uint32_t d0 = p.op == kConv3 ? L.cout : L.cin, d1 = p.op == kConv3 ? L.cin : L.cout;
        if (w->rank != 4 || w->dims[0] != d0 || w->dims[1] != d1 || w->dims[2] != k || w->dims[3] != k)
            return set(err, "tensor " + wname + ": expected shape [" + std::to_string(d0) + ", " + std::to_string(d1) + ", " +
                                std::to_string(k) + ", " + std::to_string(k) + "]");
        raw.resize(w->elements);
        for (size_t i = 0; i < w->elements; ++i) {
            raw[i] = rdf(w->data + 4 * i);
            if (!std::isfinite(raw[i])) return set(err, "tensor " + wname + ": a value is not finite");
        }
        L.weights.resize(w->elements);
        pack_weights(p.op, L.cin, L.cout, raw.data(), L.weights.data());
        L.scale.assign(L.cout, 1.0f);
        L.shift.assign(L.cout, 0.0f);
        if (!p.norm) {
            const std::string bname = std::string(p.conv) + ".bias";
            const Tensor* b = find_vector(tensors, bname, L.cout, err);
            if (!b) return false;
            for (uint32_t c = 0; c < L.cout; ++c) {
                L.shift[c] = rdf(b->data + 4 * c);
                if (!std::isfinite(L.shift[c])) return set(err, "tensor " + bname + ": a value is not finite");
            }
            continue;
        }
        const std::string n = p.norm;
        const Tensor* gamma = find_vector(tensors, n + ".weight", L.cout, err);
        const Tensor* beta = gamma ? find_vector(tensors, n + ".bias", L.cout, err) : nullptr;
        const Tensor* mean = beta ? find_vector(tensors, n + ".running_mean", L.cout, err) : nullptr;
        const Tensor* var = mean ? find_vector(tensors, n + ".running_var", L.cout, err) : nullptr;
        if (!var) return false;
        for (uint32_t c = 0; c < L.cout; ++c) {
            const float g = rdf(gamma->data + 4 * c), b = rdf(beta->data + 4 * c), m = rdf(mean->data + 4 * c);
            const float v = rdf(var->data + 4 * c);
            if (!(v >= 0.0f) || !std::isfinite(v))
                return set(err, "tensor " + n + ".running_var: channel " + std::to_string(c) + " is negative or not finite");
            if (!std::isfinite(g)) return set(err, "tensor " + n + ".weight: a value is not finite");
            if (!std::isfinite(b)) return set(err, "tensor " + n + ".bias: a value is not finite");
            if (!std::isfinite(m)) return set(err, "tensor " + n + ".running_mean: a value is not finite");
            // eval-mode BatchNorm, in float32
            L.scale[c] = g / std::sqrt(v + kBatchNormEps);
            L.shift[c] = b - m * L.scale[c];
            if (!std::isfinite(L.scale[c]) || !std::isfinite(L.shift[c]))
                return set(err, "tensor " + n + ".running_var: the folded scale of channel " + std::to_string(c) + " is not finite");
        }
    }
    return true;
}

}  // namespace fgc
