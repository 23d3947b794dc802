// FrameDatasetRecorder.cpp — dataset samples on disk (see the header). Behaviour follows the reference's
// AI/FrameDatasetRecorder.cpp: interval counting (:454-460), validation and pairing (:71-186), the NPY preamble
// (:275-340), the metadata text (:342-366) and the draining worker (:368-452).
#include "trident/FrameDatasetRecorder.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <system_error>

namespace Trident {

namespace {

void Log(const char* detail) { std::fprintf(stderr, "[Trident] FrameDatasetRecorder: %s\n", detail); }
void Log(const std::string& detail) { Log(detail.c_str()); }

}  // namespace

FrameDatasetRecorder::~FrameDatasetRecorder() { StopWorker(); }

void FrameDatasetRecorder::SetCaptureDirectory(const std::filesystem::path& directory) {
    m_CaptureDirectory = directory;
    m_DirectoryPrepared = false;
}

void FrameDatasetRecorder::EnableCapture(bool enable) {
    m_CaptureEnabled = enable;
    if (enable) {
        StartWorker();
        m_FrameCounter = 0;
    } else {
        StopWorker();  // every queued job is written first
        Reset();
    }
}

void FrameDatasetRecorder::SetSampleInterval(uint32_t interval) { m_CaptureSampleInterval = std::max<uint32_t>(1u, interval); }

void FrameDatasetRecorder::Reset() {
    m_PendingSamples.clear();
    m_NextSampleIndex = 0;
    m_FrameCounter = 0;
}

void FrameDatasetRecorder::RecordInputFrame(const float* frameData, size_t count, uint32_t width, uint32_t height,
                                            uint32_t channelCount, const int64_t* tensorShape, size_t rank) {
    if (!m_CaptureEnabled) return;
    if (++m_FrameCounter % m_CaptureSampleInterval != 0) return;
    if (width == 0 || height == 0 || channelCount == 0) {
        Log("rejected a frame with an empty extent or no channels");
        return;
    }
    const size_t expected = (size_t)width * height * channelCount;
    if (count != expected || !frameData) {
        Log("rejected a frame: " + std::to_string(count) + " elements, " + std::to_string(expected) + " expected");
        return;
    }
    EnsureDirectoryReady();
    const uint64_t index = m_NextSampleIndex++;
    CaptureJob job;
    job.m_IsInput = true;
    job.m_TargetPath = BuildPath("inputs", "frame_%06llu.npy", index);
    job.m_MetadataPath = BuildPath("metadata", "frame_%06llu.json", index);
    job.m_Data.assign(frameData, frameData + count);
    if (tensorShape && rank) job.m_Shape.assign(tensorShape, tensorShape + rank);
    else job.m_Shape = {1, (int64_t)height, (int64_t)width, (int64_t)channelCount};  // NHWC with an explicit batch
    job.m_Width = width;
    job.m_Height = height;
    job.m_ChannelCount = channelCount;
    EnqueueJob(std::move(job));
    m_PendingSamples.push_back(index);
}

void FrameDatasetRecorder::RecordAiOutput(const float* outputData, size_t count, const int64_t* outputShape, size_t rank) {
    if (!m_CaptureEnabled) return;
    if (!outputData || count == 0) {
        Log("skipped an empty AI output");
        return;
    }
    if (m_PendingSamples.empty()) {
        Log("no input frame is waiting for this AI output: record inputs before outputs");
        return;
    }
    const uint64_t index = m_PendingSamples.front();  // the oldest input
    m_PendingSamples.pop_front();
    EnsureDirectoryReady();
    std::vector<int64_t> shape;
    if (outputShape && rank) shape.assign(outputShape, outputShape + rank);
    else shape = {(int64_t)count};
    // an explicit batch, channels last
    if (shape.size() == 3) shape.insert(shape.begin(), 1);
    else if (shape.size() >= 4) shape[0] = shape[0] <= 0 ? 1 : shape[0];
    else if (shape.size() == 1) shape = {1, shape[0], 1, 1};
    CaptureJob job;
    job.m_IsInput = false;
    job.m_TargetPath = BuildPath("outputs", "ai_%06llu.npy", index);
    job.m_Data.assign(outputData, outputData + count);
    job.m_Shape = std::move(shape);
    EnqueueJob(std::move(job));
}

std::filesystem::path FrameDatasetRecorder::BuildPath(const char* subdirectory, const char* format, uint64_t index) const {
    char name[40];
    std::snprintf(name, sizeof name, format, (unsigned long long)index);
    return m_CaptureDirectory / subdirectory / name;
}

void FrameDatasetRecorder::EnsureDirectoryReady() {
    if (m_DirectoryPrepared) return;
    if (m_CaptureDirectory.empty()) m_CaptureDirectory = std::filesystem::current_path() / "DatasetCapture";
    for (const char* sub : {"inputs", "outputs", "metadata"}) {
        std::error_code ec;
        std::filesystem::create_directories(m_CaptureDirectory / sub, ec);
        if (ec) Log("could not create " + (m_CaptureDirectory / sub).string() + ": " + ec.message());
    }
    m_DirectoryPrepared = true;
}

std::string FrameDatasetRecorder::BuildShapeString(const int64_t* shape, size_t rank) {
    std::string s = "(";
    for (size_t i = 0; i < rank; ++i) {
        s += std::to_string((long long)shape[i]);
        if (i + 1 != rank) s += ", ";
    }
    if (rank == 1) s += ',';
    return s + ")";
}

bool FrameDatasetRecorder::WriteNpyFile(const std::filesystem::path& path, const float* data, size_t count,
                                        const int64_t* shape, size_t rank) {
    if (!shape || rank == 0) {
        Log("refused " + path.string() + ": empty shape");
        return false;
    }
    size_t expected = 1;
    for (size_t i = 0; i < rank; ++i) {
        if (shape[i] <= 0) {
            Log("refused " + path.string() + ": non-positive dimension");
            return false;
        }
        expected *= (size_t)shape[i];
    }
    if (expected != count) {
        Log("refused " + path.string() + ": the shape holds " + std::to_string(expected) + " elements, " +
            std::to_string(count) + " given");
        return false;
    }
    // magic (6) + version (2) + header length (2) + header: a multiple of 16, the header ending in '\n'
    std::string header = "{'descr': '<f4', 'fortran_order': False, 'shape': " + BuildShapeString(shape, rank) + ", }";
    const size_t unpadded = 10 + header.size() + 1;
    header.append((16 - unpadded % 16) % 16, ' ');
    header.push_back('\n');
    if (header.size() > 65535) {
        Log("refused " + path.string() + ": header beyond the 16-bit length field");
        return false;
    }
    std::ofstream out(path, std::ios::binary | std::ios::trunc);
    if (!out.is_open()) {
        Log("could not open " + path.string());
        return false;
    }
    const unsigned char preamble[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(header.size() & 0xFF),
                                        (unsigned char)(header.size() >> 8)};
    out.write(reinterpret_cast<const char*>(preamble), sizeof preamble);
    out.write(header.data(), (std::streamsize)header.size());
    out.write(reinterpret_cast<const char*>(data), (std::streamsize)(count * sizeof(float)));  // (a little-endian host)
    out.close();
    return true;
}

void FrameDatasetRecorder::WriteMetadataFile(const std::filesystem::path& path, uint32_t width, uint32_t height,
                                             uint32_t channelCount, const int64_t* tensorShape, size_t rank,
                                             const std::string& colorOrder, bool normalised) {
    std::ofstream out(path, std::ios::trunc);
    if (!out.is_open()) {
        Log("could not write metadata " + path.string());
        return;
    }
    out << "{\n";
    out << "  \"width\": " << width << ",\n";
    out << "  \"height\": " << height << ",\n";
    out << "  \"channels\": " << channelCount << ",\n";
    if (tensorShape && rank) out << "  \"layout\": \"" << BuildShapeString(tensorShape, rank) << "\",\n";
    out << "  \"channelsLast\": true,\n";
    out << "  \"colorOrder\": \"" << colorOrder << "\",\n";
    out << "  \"normalised\": " << (normalised ? "true" : "false") << "\n";
    out << "}\n";
}

void FrameDatasetRecorder::StartWorker() {
    if (m_WorkerThread.joinable()) return;
    {
        std::lock_guard<std::mutex> lock(m_QueueMutex);
        m_StopWorker = false;
    }
    m_WorkerThread = std::thread([this] { WorkerLoop(); });
}

void FrameDatasetRecorder::StopWorker() {
    if (!m_WorkerThread.joinable()) return;
    {
        std::lock_guard<std::mutex> lock(m_QueueMutex);
        m_StopWorker = true;
    }
    m_QueueCondition.notify_all();
    m_WorkerThread.join();  // (the loop leaves only with an empty queue)
}

void FrameDatasetRecorder::WorkerLoop() {
    std::unique_lock<std::mutex> lock(m_QueueMutex);
    for (;;) {
        m_QueueCondition.wait(lock, [this] { return m_StopWorker || !m_WriteQueue.empty(); });
        if (m_WriteQueue.empty()) return;  // asked to stop, and drained
        CaptureJob job = std::move(m_WriteQueue.front());
        m_WriteQueue.pop_front();
        m_JobInFlight = true;
        lock.unlock();
        ProcessJob(job);
        lock.lock();
        m_JobInFlight = false;
        m_QueueCondition.notify_all();  // (Flush may be waiting)
    }
}

void FrameDatasetRecorder::EnqueueJob(CaptureJob&& job) {
    {
        std::lock_guard<std::mutex> lock(m_QueueMutex);
        m_WriteQueue.push_back(std::move(job));
    }
    m_QueueCondition.notify_all();
}

void FrameDatasetRecorder::Flush() {
    if (!m_WorkerThread.joinable()) return;
    std::unique_lock<std::mutex> lock(m_QueueMutex);
    m_QueueCondition.wait(lock, [this] { return m_WriteQueue.empty() && !m_JobInFlight; });
}

void FrameDatasetRecorder::ProcessJob(const CaptureJob& job) {
    if (!WriteNpyFile(job.m_TargetPath, job.m_Data.data(), job.m_Data.size(), job.m_Shape.data(), job.m_Shape.size())) {
        Log("could not persist " + job.m_TargetPath.string());
        return;
    }
    // "BGRA" although the tensor's channels are R, G, B, A: the reference labels its samples so (a quirk of its
    // recorder, FrameDatasetRecorder.cpp:121), and the files here are its files byte for byte
    if (job.m_IsInput)
        WriteMetadataFile(job.m_MetadataPath, job.m_Width, job.m_Height, job.m_ChannelCount, job.m_Shape.data(),
                          job.m_Shape.size(), "BGRA", true);
}

}  // namespace Trident
