// dataset_recorder_check.cpp — stand-alone host check of Trident::FrameDatasetRecorder, built with sanitizers
// (make dataset-check: address + undefined behaviour; make dataset-check-tsan: thread). It drives the recorder the
// way the renderer does — inputs and outputs queued faster than the worker writes them, capture disabled with jobs
// still queued, a second session, destruction with jobs queued — and re-reads every file it wrote.
//
//   dataset_recorder_check <scratch directory>
#include "trident/FrameDatasetRecorder.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

using Trident::FrameDatasetRecorder;

namespace {

int g_failures = 0;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                      \
        }                                                                      \
    } while (0)

std::string ReadAll(const std::filesystem::path& p) {
    std::ifstream in(p, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

std::vector<float> Sample(uint32_t w, uint32_t h, uint32_t c, uint32_t seed) {
    std::vector<float> v((size_t)w * h * c);
    for (size_t i = 0; i < v.size(); ++i) v[i] = (float)((i * 31u + seed * 7u) % 256u) * (1.0f / 255.0f);
    return v;
}

// The NPY 1.0 file the recorder must have written, restated here.
std::string ExpectedNpy(const std::vector<float>& data, const std::string& shape) {
    std::string header = "{'descr': '<f4', 'fortran_order': False, 'shape': " + shape + ", }";
    while ((10 + header.size() + 1) % 16 != 0) header.push_back(' ');
    header.push_back('\n');
    std::string out = "\x93NUMPY";
    out.push_back(1);
    out.push_back(0);
    out.push_back((char)(header.size() & 0xFF));
    out.push_back((char)(header.size() >> 8));
    out += header;
    out.append(reinterpret_cast<const char*>(data.data()), data.size() * sizeof(float));
    return out;
}

std::string Name(const char* format, unsigned long long index) {
    char b[40];
    std::snprintf(b, sizeof b, format, index);
    return b;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]);
        return 2;
    }
    const std::filesystem::path root = std::filesystem::path(argv[1]) / "capture";
    constexpr uint32_t kW = 37, kH = 19, kC = 4, kSamples = 24;

    {  // session 1: many samples queued, then disabled mid-queue — every file must be complete
        FrameDatasetRecorder rec;
        rec.SetCaptureDirectory(root);
        rec.SetSampleInterval(1);
        rec.EnableCapture(true);
        for (uint32_t i = 0; i < kSamples; ++i) {
            const std::vector<float> in = Sample(kW, kH, kC, i);
            rec.RecordInputFrame(in.data(), in.size(), kW, kH, kC);
            if (i % 2 == 1) {  // outputs lag: each pairs with the oldest input waiting
                const std::vector<float> out = Sample(kW, kH, 3, 1000 + i);
                const int64_t shape[3] = {kH, kW, 3};
                rec.RecordAiOutput(out.data(), out.size(), shape, 3);
            }
        }
        CHECK(rec.GetNextSampleIndex() == kSamples);
        CHECK(rec.GetPendingSampleCount() == kSamples / 2);
        rec.EnableCapture(false);  // the queue is flushed, the worker joined, the numbering reset
        CHECK(rec.GetNextSampleIndex() == 0 && rec.GetPendingSampleCount() == 0);
        const std::string in_shape = "(1, " + std::to_string(kH) + ", " + std::to_string(kW) + ", 4)";
        for (uint32_t i = 0; i < kSamples; ++i) {
            CHECK(ReadAll(root / "inputs" / Name("frame_%06llu.npy", i)) == ExpectedNpy(Sample(kW, kH, kC, i), in_shape));
            const std::string meta = ReadAll(root / "metadata" / Name("frame_%06llu.json", i));
            CHECK(meta == "{\n  \"width\": 37,\n  \"height\": 19,\n  \"channels\": 4,\n  \"layout\": \"" + in_shape +
                              "\",\n  \"channelsLast\": true,\n  \"colorOrder\": \"BGRA\",\n  \"normalised\": true\n}\n");
        }
        const std::string out_shape = "(1, " + std::to_string(kH) + ", " + std::to_string(kW) + ", 3)";
        for (uint32_t k = 0; k < kSamples / 2; ++k)  // output k came with input 2k + 1 and pairs with sample k
            CHECK(ReadAll(root / "outputs" / Name("ai_%06llu.npy", k)) == ExpectedNpy(Sample(kW, kH, 3, 1000 + 2 * k + 1), out_shape));
        CHECK(!std::filesystem::exists(root / "outputs" / Name("ai_%06llu.npy", kSamples / 2)));

        // session 2 on the same object: interval 3, numbering from 0 again; refusals leave no file
        rec.SetSampleInterval(3);
        rec.EnableCapture(true);
        for (uint32_t i = 0; i < 7; ++i) {
            const std::vector<float> in = Sample(5, 3, 1, 500 + i);
            rec.RecordInputFrame(in.data(), in.size(), 5, 3, 1);
        }
        CHECK(rec.GetNextSampleIndex() == 2);  // calls 3 and 6
        const std::vector<float> bad = Sample(5, 3, 1, 0);
        rec.RecordInputFrame(bad.data(), bad.size() - 1, 5, 3, 1);  // call 8: not sampled
        rec.RecordInputFrame(bad.data(), bad.size() - 1, 5, 3, 1);  // call 9: sampled, wrong count -> dropped
        CHECK(rec.GetNextSampleIndex() == 2);
        rec.RecordAiOutput(nullptr, 0, nullptr, 0);  // empty: dropped, nothing paired
        CHECK(rec.GetPendingSampleCount() == 2);
        const std::vector<float> flat = Sample(6, 1, 1, 77);
        rec.RecordAiOutput(flat.data(), flat.size(), nullptr, 0);  // rank 1 -> (1, 6, 1, 1)
        rec.Flush();
        CHECK(ReadAll(root / "inputs" / Name("frame_%06llu.npy", 0)) == ExpectedNpy(Sample(5, 3, 1, 502), "(1, 3, 5, 1)"));
        CHECK(ReadAll(root / "inputs" / Name("frame_%06llu.npy", 1)) == ExpectedNpy(Sample(5, 3, 1, 505), "(1, 3, 5, 1)"));
        CHECK(ReadAll(root / "outputs" / Name("ai_%06llu.npy", 0)) == ExpectedNpy(flat, "(1, 6, 1, 1)"));
        // destroyed while enabled, with jobs queued: the destructor writes them
        for (uint32_t i = 0; i < 6; ++i) {
            const std::vector<float> in = Sample(kW, kH, kC, 900 + i);
            rec.RecordInputFrame(in.data(), in.size(), kW, kH, kC);
        }
        CHECK(rec.GetNextSampleIndex() == 4);  // calls 12 and 15 of this session
    }
    {
        const std::string in_shape = "(1, 19, 37, 4)";
        CHECK(ReadAll(root / "inputs" / Name("frame_%06llu.npy", 2)) == ExpectedNpy(Sample(kW, kH, kC, 902), in_shape));
        CHECK(ReadAll(root / "inputs" / Name("frame_%06llu.npy", 3)) == ExpectedNpy(Sample(kW, kH, kC, 905), in_shape));
    }
    {  // the writer alone: rank 1, refusals
        const std::filesystem::path p = std::filesystem::path(argv[1]) / "one.npy";
        const std::vector<float> v = Sample(9, 1, 1, 3);
        const int64_t s1[1] = {9}, zero[2] = {0, 9}, wrong[2] = {2, 5};
        CHECK(FrameDatasetRecorder::WriteNpyFile(p, v.data(), v.size(), s1, 1));
        CHECK(ReadAll(p) == ExpectedNpy(v, "(9,)"));
        const std::filesystem::path q = std::filesystem::path(argv[1]) / "refused.npy";
        CHECK(!FrameDatasetRecorder::WriteNpyFile(q, v.data(), v.size(), zero, 2));
        CHECK(!FrameDatasetRecorder::WriteNpyFile(q, v.data(), v.size(), wrong, 2));
        CHECK(!FrameDatasetRecorder::WriteNpyFile(q, v.data(), v.size(), nullptr, 0));
        CHECK(!std::filesystem::exists(q));
    }
    {  // never enabled: nothing is written, nothing to join
        FrameDatasetRecorder idle;
        idle.SetCaptureDirectory(std::filesystem::path(argv[1]) / "idle");
        const std::vector<float> v = Sample(2, 2, 4, 1);
        idle.RecordInputFrame(v.data(), v.size(), 2, 2, 4);
        idle.Flush();
        idle.EnableCapture(false);
        CHECK(!std::filesystem::exists(std::filesystem::path(argv[1]) / "idle"));
    }
    if (g_failures) {
        std::fprintf(stderr, "dataset_recorder_check: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("dataset_recorder_check: ok\n");
    return 0;
}
