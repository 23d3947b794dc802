// Trident::AI::FrameGenerator over tri_framegen (see the header for what differs from the reference's class).
#include "trident/FrameGenerator.h"

#include "../../csrc/framegen_container.h"

#include <fstream>
#include <iterator>

namespace Trident {
namespace AI {

bool FrameGenerator::Initialise(const std::string& modelPath) {
    std::ifstream f(modelPath, std::ios::binary);
    if (!f) {
        m_LastError = "cannot open '" + modelPath + "'";
        return false;
    }
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    // the parser's own verdict, here on the host: a damaged model is refused when it is named, not at the first frame
    fgc::Model model;
    std::string err;
    if (!fgc::load(bytes.data(), bytes.size(), model, err)) {
        m_LastError = err;
        return false;
    }
    Shutdown();
    m_Container = std::move(bytes);
    m_ModelPath = modelPath;
    m_InputChannels = model.input_channels;
    m_LastError.clear();
    return true;
}

void FrameGenerator::Shutdown() {
    tri_framegen_destroy(m_Gen);  // (waits for a job in flight)
    m_Gen = nullptr;
    m_Container.clear();
    m_ModelPath.clear();
    m_InputChannels = 0;
    m_Width = m_Height = 0;
    m_InFlight = m_HasOutput = m_CreateFailed = false;
    m_Completed = 0;
    m_LastMs = m_TotalMs = 0.0;
}

bool FrameGenerator::ProcessFrame(int32_t device, const float* deviceTensor, uint32_t width, uint32_t height, uint32_t channels,
                                  void* producerStream) {
    if (!IsInitialised() || m_InFlight) return false;
    if (channels != m_InputChannels) {
        m_LastError = "the model takes " + std::to_string(m_InputChannels) + " channels, the frame has " + std::to_string(channels);
        return false;
    }
    if (!m_Gen || width != m_Width || height != m_Height || device != m_Device) {  // the first frame, or another extent
        // (refused before, with the message: not parsed again per frame)
        if (m_CreateFailed && width == m_FailedWidth && height == m_FailedHeight && device == m_FailedDevice) return false;
        // the present generator, and with it the output that new targets still pack, stays until the next one stands
        tri_framegen* gen = nullptr;
        if (tri_framegen_create(device, m_Container.data(), m_Container.size(), width, height, &gen) != TRI_OK) {
            m_LastError = tri_last_error();
            m_CreateFailed = true;
            m_FailedWidth = width;
            m_FailedHeight = height;
            m_FailedDevice = device;
            return false;
        }
        tri_framegen_destroy(m_Gen);
        m_Gen = gen;
        m_HasOutput = false;
        m_Width = width;
        m_Height = height;
        m_Device = device;
        m_CreateFailed = false;
    }
    if (tri_framegen_submit(m_Gen, deviceTensor, producerStream) != TRI_OK) {
        m_LastError = tri_last_error();
        m_HasOutput = false;  // (the library drops the output of a submit that failed half way)
        return false;
    }
    m_InFlight = true;
    m_HasOutput = false;
    return true;
}

bool FrameGenerator::TryConsumeOutput(bool wait) {
    if (!m_Gen || !m_InFlight) return false;
    int32_t done = 0;
    if (wait) {
        if (tri_framegen_wait(m_Gen) != TRI_OK) {
            m_LastError = tri_last_error();
            m_InFlight = false;  // (a device error: the job is lost)
            return false;
        }
        done = 1;
    } else if (tri_framegen_poll(m_Gen, &done) != TRI_OK) {
        m_LastError = tri_last_error();
        m_InFlight = false;
        return false;
    }
    if (!done) return false;
    m_InFlight = false;
    m_HasOutput = true;
    float ms = 0.0f;
    if (tri_framegen_last_ms(m_Gen, &ms) == TRI_OK) m_LastMs = ms;
    m_TotalMs += m_LastMs;
    ++m_Completed;
    return true;
}

bool FrameGenerator::GetOutputDevice(const float** device, uint32_t& width, uint32_t& height) const {
    if (!m_Gen || !m_HasOutput || !device || tri_framegen_output(m_Gen, device) != TRI_OK) return false;
    width = m_Width;
    height = m_Height;
    return true;
}

bool FrameGenerator::ReadOutput(std::vector<float>& out) const {
    if (!m_Gen || !m_HasOutput) return false;
    out.resize((size_t)m_Width * m_Height * 3);
    return tri_framegen_read_output(m_Gen, out.data()) == TRI_OK;
}

std::vector<int64_t> FrameGenerator::GetPrimaryInputShape() const {
    if (!IsInitialised()) return {};
    if (!m_Gen) return {1, -1, -1, (int64_t)m_InputChannels};
    return {1, (int64_t)m_Height, (int64_t)m_Width, (int64_t)m_InputChannels};
}

std::vector<int64_t> FrameGenerator::GetPrimaryOutputShape() const {
    if (!IsInitialised()) return {};
    if (!m_Gen) return {1, -1, -1, 3};
    return {1, (int64_t)m_Height, (int64_t)m_Width, 3};
}

}  // namespace AI
}  // namespace Trident
