// FrameDatasetRecorder.h — Trident::FrameDatasetRecorder, the reference's AI::FrameDatasetRecorder
// (Trident/src/AI/FrameDatasetRecorder.h:28-127): the frame generator's training samples on disk.
//
//   <directory>/inputs/frame_%06llu.npy     the tensor offered to the generator (float32, NHWC)
//   <directory>/metadata/frame_%06llu.json  its extent, channel count and layout
//   <directory>/outputs/ai_%06llu.npy       the generator's answer, paired with the oldest input still waiting
//
// Width and height replace the VkExtent2D, and pointer + count the std::span (C++17). The files are the reference's
// byte for byte: NPY version 1.0 whose preamble is padded to a multiple of 16 (numpy's own writer pads to 64, and
// reads either), and the metadata text. File writes happen on a worker thread, in submission order; one thread
// drives the recorder's interface.
#pragma once

#include <condition_variable>
#include <cstdint>
#include <deque>
#include <filesystem>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace Trident {

class FrameDatasetRecorder {
public:
    FrameDatasetRecorder() = default;
    ~FrameDatasetRecorder();  // writes what is queued, then joins the worker
    FrameDatasetRecorder(const FrameDatasetRecorder&) = delete;
    FrameDatasetRecorder& operator=(const FrameDatasetRecorder&) = delete;

    // The root of the three sub-directories; they are created by the next recorded sample. An empty path falls back
    // to current_path()/DatasetCapture at that point.
    void SetCaptureDirectory(const std::filesystem::path& directory);
    const std::filesystem::path& GetCaptureDirectory() const { return m_CaptureDirectory; }
    // Enabling starts the worker and restarts the interval count. Disabling writes every queued job, joins the worker
    // and resets (the next session numbers its samples from 0 again and forgets the inputs still waiting).
    void EnableCapture(bool enable);
    bool IsCaptureEnabled() const { return m_CaptureEnabled; }
    void SetSampleInterval(uint32_t interval);  // at least 1
    uint32_t GetSampleInterval() const { return m_CaptureSampleInterval; }
    void Reset();  // forgets the waiting inputs; sample index and interval count back to 0

    // The frame offered to the generator. Every call while enabled counts towards the interval (++counter % interval
    // == 0 records); a zero extent or channel count, or count != width * height * channels, drops the frame with a
    // log line. rank 0 means the shape {1, height, width, channels}.
    void RecordInputFrame(const float* frameData, size_t count, uint32_t width, uint32_t height, uint32_t channelCount,
                          const int64_t* tensorShape = nullptr, size_t rank = 0);
    // The generator's output for the oldest waiting input (an empty output, or one with no input waiting, is dropped
    // with a log line). rank 0 means {count}; a rank-3 shape gets a leading 1, rank >= 4 a batch of at least 1, rank 1
    // becomes {1, n, 1, 1}.
    void RecordAiOutput(const float* outputData, size_t count, const int64_t* outputShape, size_t rank);

    void Flush();  // returns once every queued job has been written
    uint64_t GetNextSampleIndex() const { return m_NextSampleIndex; }
    size_t GetPendingSampleCount() const { return m_PendingSamples.size(); }

    // "(1, 2, 3)"; rank 1: "(n,)".
    static std::string BuildShapeString(const int64_t* shape, size_t rank);
    // One NPY 1.0 file of little-endian float32. Refused (false, with a log line, no file): an empty shape, a
    // non-positive dimension, a shape whose element count is not `count`, a header beyond 65535 bytes.
    static bool WriteNpyFile(const std::filesystem::path& path, const float* data, size_t count, const int64_t* shape,
                             size_t rank);
    static void WriteMetadataFile(const std::filesystem::path& path, uint32_t width, uint32_t height, uint32_t channelCount,
                                  const int64_t* tensorShape, size_t rank, const std::string& colorOrder, bool normalised);

private:
    struct CaptureJob {
        bool m_IsInput = true;
        std::filesystem::path m_TargetPath, m_MetadataPath;  // (metadata: inputs only)
        std::vector<float> m_Data;                           // the worker owns a copy
        std::vector<int64_t> m_Shape;
        uint32_t m_Width = 0, m_Height = 0, m_ChannelCount = 0;
    };

    std::filesystem::path m_CaptureDirectory;
    bool m_CaptureEnabled = false;
    bool m_DirectoryPrepared = false;
    uint64_t m_NextSampleIndex = 0;
    std::deque<uint64_t> m_PendingSamples;  // indices of the inputs whose output has not arrived, oldest first
    uint64_t m_FrameCounter = 0;
    uint32_t m_CaptureSampleInterval = 1;

    // the worker: everything below is guarded by m_QueueMutex
    std::mutex m_QueueMutex;
    std::condition_variable m_QueueCondition;  // a job arrived, a job was finished, or the worker shall stop
    std::deque<CaptureJob> m_WriteQueue;
    bool m_StopWorker = false;
    bool m_JobInFlight = false;
    std::thread m_WorkerThread;  // (joinable exactly while the worker runs; touched by the interface thread only)

    std::filesystem::path BuildPath(const char* subdirectory, const char* format, uint64_t index) const;
    void EnsureDirectoryReady();
    void StartWorker();
    void StopWorker();
    void WorkerLoop();
    void EnqueueJob(CaptureJob&& job);
    static void ProcessJob(const CaptureJob& job);
};

}  // namespace Trident
