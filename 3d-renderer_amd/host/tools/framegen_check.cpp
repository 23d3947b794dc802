// framegen_check — host-only check of the frame generator's weights container parser, the BatchNorm fold and the weight
// re-lay (csrc/framegen_container.h), built under the address and undefined-behaviour sanitizers (make framegen-check).
// It writes a good container into memory (or reads the file named on the command line), loads it, and then feeds the
// loader damaged copies: truncated at every table boundary and inside the data, an oversized dimension, a missing
// tensor, a wrong shape, a misaligned offset, an offset beyond the file, a NaN and a negative variance. Every damaged
// copy must be refused with a message that names what is wrong; nothing may read out of bounds.
#include "../../csrc/framegen_container.h"

#include <cstdlib>
#include <fstream>
#include <iterator>

namespace {

int g_failures = 0;

void expect(bool ok, const char* what, const std::string& detail = "") {
    if (ok) return;
    std::fprintf(stderr, "FAIL: %s %s\n", what, detail.c_str());
    ++g_failures;
}

void put32(std::vector<uint8_t>& b, size_t at, uint32_t v) {
    for (int i = 0; i < 4; ++i) b[at + i] = (uint8_t)(v >> (8 * i));
}
void put64(std::vector<uint8_t>& b, size_t at, uint64_t v) {
    put32(b, at, (uint32_t)v);
    put32(b, at + 4, (uint32_t)(v >> 32));
}
void putf(std::vector<uint8_t>& b, size_t at, float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    put32(b, at, u);
}

struct Spec {
    std::string name;
    std::vector<uint32_t> dims;
};

// Every tensor the plan names, in the checkpoint's shapes.
std::vector<Spec> plan_tensors(uint32_t input_channels) {
    std::vector<Spec> specs;
    for (const fgc::LayerPlan& p : fgc::kFgPlan) {
        const uint32_t cin = p.cin ? p.cin : input_channels;
        const std::string conv = p.conv;
        if (p.op == fgc::kConv3) specs.push_back({conv + ".weight", {p.cout, cin, 3, 3}});
        else specs.push_back({conv + ".weight", {cin, p.cout, 4, 4}});
        if (!p.norm) {
            specs.push_back({conv + ".bias", {p.cout}});
            continue;
        }
        const std::string n = p.norm;
        for (const char* leaf : {".weight", ".bias", ".running_mean", ".running_var"}) specs.push_back({n + leaf, {p.cout}});
    }
    return specs;
}

float value_of(uint32_t& state, bool positive) {  // a small LCG: values in [-0.5, 0.5), or [0.5, 1.5)
    state = state * 1664525u + 1013904223u;
    const float u = (float)(state >> 8) * (1.0f / 16777216.0f);
    return positive ? u + 0.5f : u - 0.5f;
}

std::vector<uint8_t> good_container(uint32_t input_channels) {
    const std::vector<Spec> specs = plan_tensors(input_channels);
    size_t offset = fgc::kHeaderBytes + specs.size() * fgc::kEntryBytes;
    std::vector<uint8_t> b(offset, 0);
    std::memcpy(b.data(), "TRIFGEN", 8);
    put32(b, 8, fgc::kVersion);
    put32(b, 12, input_channels);
    put32(b, 16, (uint32_t)specs.size());
    uint32_t rng = 12345;
    for (size_t i = 0; i < specs.size(); ++i) {
        const size_t e = fgc::kHeaderBytes + i * fgc::kEntryBytes;
        std::memcpy(b.data() + e, specs[i].name.c_str(), specs[i].name.size());
        put32(b, e + 64, (uint32_t)specs[i].dims.size());
        size_t n = 1;
        for (uint32_t d = 0; d < 4; ++d) {
            const uint32_t dim = d < specs[i].dims.size() ? specs[i].dims[d] : 1;
            put32(b, e + 68 + 4 * d, dim);
            n *= dim;
        }
        put64(b, e + 88, offset);
        const bool variance = specs[i].name.find("running_var") != std::string::npos;
        b.resize(offset + 4 * n);
        for (size_t k = 0; k < n; ++k) putf(b, offset + 4 * k, value_of(rng, variance));
        offset += 4 * n;
    }
    return b;
}

size_t entry_of(const std::vector<uint8_t>& b, const std::string& name) {
    const uint32_t count = fgc::detail::rd32(b.data() + 16);
    for (uint32_t i = 0; i < count; ++i) {
        const size_t e = fgc::kHeaderBytes + (size_t)i * fgc::kEntryBytes;
        if (name == reinterpret_cast<const char*>(b.data() + e)) return e;
    }
    std::fprintf(stderr, "framegen_check: no tensor %s in the good container\n", name.c_str());
    std::exit(2);
}

// The loader must refuse `b` and name `needle` in its message. The bytes are copied into an exactly sized heap block,
// so a read beyond them is the sanitizer's to catch.
void refuse(const std::vector<uint8_t>& b, const char* what, const std::string& needle) {
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(b.size() ? b.size() : 1));
    if (!b.empty()) std::memcpy(exact, b.data(), b.size());
    fgc::Model model;
    std::string err;
    const bool ok = fgc::load(exact, b.size(), model, err);
    std::free(exact);
    expect(!ok, what, "was accepted");
    expect(ok || err.find(needle) != std::string::npos, what, "message: " + err);
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<uint8_t> good;
    if (argc > 1) {
        std::ifstream f(argv[1], std::ios::binary);
        good.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    } else {
        good = good_container(4);
    }

    fgc::Model model;
    std::string err;
    expect(fgc::load(good.data(), good.size(), model, err), "the good container loads", err);
    if (g_failures) return 1;
    const uint32_t cin = model.input_channels;

    // the fold and the re-lay, recomputed from the file
    {
        const std::string n = "m_Bottleneck.1.m_Block.4";
        const fgc::Layer& L = model.layers[12];
        const uint8_t* gamma = good.data() + fgc::detail::rd64(good.data() + entry_of(good, n + ".weight") + 88);
        const uint8_t* beta = good.data() + fgc::detail::rd64(good.data() + entry_of(good, n + ".bias") + 88);
        const uint8_t* mean = good.data() + fgc::detail::rd64(good.data() + entry_of(good, n + ".running_mean") + 88);
        const uint8_t* var = good.data() + fgc::detail::rd64(good.data() + entry_of(good, n + ".running_var") + 88);
        bool same = L.scale.size() == 128 && L.shift.size() == 128;
        for (uint32_t c = 0; same && c < 128; ++c) {
            const float s = fgc::detail::rdf(gamma + 4 * c) / std::sqrt(fgc::detail::rdf(var + 4 * c) + 1.0e-5f);
            same = L.scale[c] == s && L.shift[c] == fgc::detail::rdf(beta + 4 * c) - fgc::detail::rdf(mean + 4 * c) * s;
        }
        expect(same, "the BatchNorm fold");
        // the first layer's bias is its shift, its scale 1
        const uint8_t* bias = good.data() + fgc::detail::rd64(good.data() + entry_of(good, "m_EncoderStage1.0.bias") + 88);
        expect(model.layers[0].scale[5] == 1.0f && model.layers[0].shift[5] == fgc::detail::rdf(bias + 20), "the bias fold");
        // conv: packed[ky][kx][ci][co] == torch[co][ci][ky][kx]
        const uint8_t* w0 = good.data() + fgc::detail::rd64(good.data() + entry_of(good, "m_EncoderStage1.0.weight") + 88);
        const uint32_t co = 7, ci = cin - 1, ky = 2, kx = 0;
        expect(model.layers[0].weights[(((size_t)ky * 3 + kx) * cin + ci) * 32 + co] ==
                   fgc::detail::rdf(w0 + 4 * ((((size_t)co * cin + ci) * 3 + ky) * 3 + kx)),
               "the 3x3 re-lay");
        // transposed: output parity (1, 0), tap (a, b) = (1, 0) is ky = 1 - 1 + 2 = 2, kx = 1 - 0 + 0 = 1
        const uint8_t* wt = good.data() + fgc::detail::rd64(good.data() + entry_of(good, "m_DecodeStage2.0.weight") + 88);
        const uint32_t tci = 100, tco = 33;
        const size_t slab = (size_t)(((1 * 2 + 0) * 2 + 1) * 2 + 0) * 128 * 64;
        expect(model.layers[13].weights[slab + (size_t)tci * 64 + tco] ==
                   fgc::detail::rdf(wt + 4 * ((((size_t)tci * 64 + tco) * 4 + 2) * 4 + 1)),
               "the transposed re-lay");
    }

    // truncated: inside the header, inside the table, at the data's start, one byte short
    const size_t table_end = fgc::kHeaderBytes + (size_t)fgc::detail::rd32(good.data() + 16) * fgc::kEntryBytes;
    for (size_t cut : {(size_t)0, (size_t)7, (size_t)31, (size_t)32, table_end - 1, table_end, table_end + 1000, good.size() - 1}) {
        std::vector<uint8_t> b(good.begin(), good.begin() + cut);
        refuse(b, "a truncated container", cut < fgc::kHeaderBytes ? "shorter than its header" : "truncated");
    }
    {
        std::vector<uint8_t> b = good;
        b[3] ^= 0x20;
        refuse(b, "a wrong magic", "magic");
        b = good;
        put32(b, 8, 2);
        refuse(b, "an unknown version", "version");
        b = good;
        put32(b, 12, 9);
        refuse(b, "nine input channels", "input channels");
        b = good;
        put32(b, 16, 0xFFFFFFFFu);
        refuse(b, "a huge tensor count", "tensor count");
    }
    const std::string victim = "m_EncoderStage3.2.m_Block.0.weight";
    {
        std::vector<uint8_t> b = good;  // oversized dimension: beyond the limit, and within it but beyond the file
        put32(b, entry_of(b, victim) + 68, 0x80000000u);
        refuse(b, "an oversized dimension", victim);
        b = good;
        put32(b, entry_of(b, victim) + 68, 65536);
        put32(b, entry_of(b, victim) + 72, 65536);
        refuse(b, "an oversized tensor", victim);
        b = good;
        put32(b, entry_of(b, victim) + 64, 5);
        refuse(b, "rank 5", victim);
    }
    {
        std::vector<uint8_t> b = good;  // missing tensor: renamed away
        b[entry_of(b, victim)] = 'x';
        refuse(b, "a missing tensor", victim);
        b = good;
        std::memset(b.data() + entry_of(b, victim), 'n', 64);
        refuse(b, "an unterminated name", "not terminated");
    }
    {
        std::vector<uint8_t> b = good;  // wrong shape: [128, 128, 3, 3] -> [128, 64, 3, 3] (still inside the file)
        put32(b, entry_of(b, victim) + 72, 64);
        refuse(b, "a wrong shape", victim);
        b = good;
        put32(b, entry_of(b, "m_OutputLayer.0.bias") + 68, 2);
        refuse(b, "a wrong bias length", "m_OutputLayer.0.bias");
    }
    {
        std::vector<uint8_t> b = good;  // misaligned offset, an offset into the table, an offset beyond the file
        const size_t e = entry_of(b, victim);
        put64(b, e + 88, fgc::detail::rd64(b.data() + e + 88) + 2);
        refuse(b, "a misaligned offset", victim);
        b = good;
        put64(b, e + 88, 32);
        refuse(b, "an offset into the table", victim);
        b = good;
        put64(b, e + 88, 0xFFFFFFFFFFFFFFF0ull);
        refuse(b, "an offset beyond the file", victim);
    }
    {
        const std::string var = "m_DecodeStage1.2.m_Block.1.running_var";
        std::vector<uint8_t> b = good;
        const size_t at = (size_t)fgc::detail::rd64(b.data() + entry_of(b, var) + 88) + 4 * 3;
        putf(b, at, std::nanf(""));
        refuse(b, "a NaN variance", var);
        putf(b, at, -0.25f);
        refuse(b, "a negative variance", var);
        putf(b, at, INFINITY);
        refuse(b, "an infinite variance", var);
        b = good;
        putf(b, (size_t)fgc::detail::rd64(b.data() + entry_of(b, victim) + 88) + 40, std::nanf(""));
        refuse(b, "a NaN weight", victim);
    }

    if (g_failures) return 1;
    std::printf("framegen_check ok: %u input channels, %zu bytes\n", cin, good.size());
    return 0;
}
