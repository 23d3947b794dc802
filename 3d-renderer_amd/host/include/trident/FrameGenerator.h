// Trident::AI::FrameGenerator — the reference's frame generator (AI/FrameGenerator.h: an ONNX Runtime session and a
// worker thread around the InterpolationUNet) as a thin owner of a tri_framegen: the network runs on the device, on
// the generator's own stream, so no worker thread is needed. The surface is the reference's; what differs:
//   - the model is a weights container (tools/export_frame_generator.py), not ONNX;
//   - ProcessFrame takes the tensor where the renderer made it, on the device, with the stream that made it; the output
//     stays on the device too (TryConsumeOutput reports it, GetOutputDevice hands it out, ReadOutput copies it);
//   - the container does not freeze the extent: the device generator is made for the first frame's extent and made
//     again when the extent changes (width and height multiples of 4), so GetPrimaryInputShape reads
//     {1, -1, -1, channels} until then; an extent the network cannot take is refused and leaves the present
//     generator and its last output as they are;
//   - one job at a time: ProcessFrame is refused (false) while one is in flight.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../../../include/tri_raster.h"

namespace Trident {
namespace AI {

class FrameGenerator {
public:
    FrameGenerator() = default;
    ~FrameGenerator() { Shutdown(); }
    FrameGenerator(const FrameGenerator&) = delete;
    FrameGenerator& operator=(const FrameGenerator&) = delete;

    // Reads and checks the container (no device needed). false with GetLastError() for a missing or damaged file; a
    // model that was loaded before stays in that case.
    bool Initialise(const std::string& modelPath);
    void Shutdown();  // waits for a job in flight
    bool IsInitialised() const { return !m_Container.empty(); }
    const std::string& GetLastError() const { return m_LastError; }
    const std::string& GetModelPath() const { return m_ModelPath; }
    uint32_t GetInputChannels() const { return m_InputChannels; }

    // Submit [height][width][channels] floats on `device`; the copy is ordered on producerStream (a hipStream_t).
    // false: not initialised, a job in flight, another channel count than the model's, an extent the network cannot
    // take, or a device error (GetLastError()).
    bool ProcessFrame(int32_t device, const float* deviceTensor, uint32_t width, uint32_t height, uint32_t channels,
                      void* producerStream);
    // true once per job, when it has finished (never blocks); with `wait`, blocks for the job in flight first.
    bool TryConsumeOutput(bool wait = false);
    bool HasJobInFlight() const { return m_InFlight; }
    // The last finished job's output, [height][width][3]: valid until the next ProcessFrame that is accepted.
    bool GetOutputDevice(const float** device, uint32_t& width, uint32_t& height) const;
    bool ReadOutput(std::vector<float>& out) const;
    tri_framegen* GetHandle() const { return m_Gen; }

    std::vector<int64_t> GetPrimaryInputShape() const;
    std::vector<int64_t> GetPrimaryOutputShape() const;
    size_t GetPendingJobCount() const { return m_InFlight ? 1 : 0; }
    uint64_t GetCompletedInferenceCount() const { return m_Completed; }
    double GetLastInferenceMilliseconds() const { return m_LastMs; }
    double GetAverageInferenceMilliseconds() const { return m_Completed ? m_TotalMs / (double)m_Completed : 0.0; }

private:
    std::vector<uint8_t> m_Container;
    std::string m_ModelPath, m_LastError;
    uint32_t m_InputChannels = 0;
    tri_framegen* m_Gen = nullptr;
    int32_t m_Device = -1;
    uint32_t m_Width = 0, m_Height = 0;
    bool m_InFlight = false, m_HasOutput = false;
    bool m_CreateFailed = false;  // tri_framegen_create refused m_FailedWidth x m_FailedHeight on m_FailedDevice
    uint32_t m_FailedWidth = 0, m_FailedHeight = 0;
    int32_t m_FailedDevice = -1;
    uint64_t m_Completed = 0;
    double m_LastMs = 0.0, m_TotalMs = 0.0;
};

}  // namespace AI
}  // namespace Trident
