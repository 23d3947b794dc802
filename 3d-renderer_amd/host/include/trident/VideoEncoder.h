// VideoEncoder.h — Trident::VideoEncoder (Trident/src/Renderer/VideoEncoder.h:27-100) for the Y4M container: the
// session rules, the header and the FRAME records of the reference, and its RGBA -> YUV 4:4:4 conversion restated
// in the same double-precision operation order. The reference hands .mp4 / .mov / .avi to FFmpeg; FFmpeg is not part
// of this project, so those containers are refused with a log line that says so (a documented deviation).
// SubmitPlanes is this project's addition: frames the device has converted already (tri_recorder).
#pragma once

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace Trident {

class VideoEncoder {
public:
    struct RecordedFrame {  // VideoEncoder.h:32-37, the extent as two integers instead of VkExtent2D
        std::vector<uint8_t> m_Pixels;  // RGBA8, rows top to bottom
        uint32_t m_Width = 0, m_Height = 0;
        std::chrono::system_clock::time_point m_Timestamp{};
    };

    VideoEncoder() = default;
    ~VideoEncoder();
    VideoEncoder(const VideoEncoder&) = delete;
    VideoEncoder& operator=(const VideoEncoder&) = delete;

    // Ends any session in progress, then opens `path` (binary, truncating) and writes the header. False, without
    // creating a file, for a zero extent, an FFmpeg container or any extension but .y4m (compared lower-cased).
    // targetFps 0 means 30.
    bool BeginSession(const std::string& path, uint32_t width, uint32_t height, uint32_t targetFps);
    // One FRAME record from RGBA pixels, converted here on the host. False (nothing written) without a session, for
    // an empty pixel buffer, or an extent that is not the session's.
    bool SubmitFrame(const RecordedFrame& frame);
    // One FRAME record from 3 * width * height bytes converted already (Y, U, V planes). Same refusals.
    bool SubmitPlanes(const uint8_t* yuv, uint32_t width, uint32_t height);
    // Flushes and closes the file; false when no session is active.
    bool EndSession();
    bool IsSessionActive() const { return m_File != nullptr; }
    uint64_t GetFrameCount() const { return m_Frames; }  // FRAME records written by the current or last session
    uint32_t GetWidth() const { return m_Width; }
    uint32_t GetHeight() const { return m_Height; }

    // The conversion alone (ConvertRgbaToYuv444, VideoEncoder.cpp:716-736): `pixels` RGBA8 pixels -> 3 * pixels
    // bytes, planar. Y = 0.299 R + 0.587 G + 0.114 B, U = -0.169 R - 0.331 G + 0.5 B + 128,
    // V = 0.5 R - 0.419 G - 0.081 B + 128 in double, left to right, clamped to [0, 255] and truncated.
    static void ConvertRgbaToYuv444(const uint8_t* rgba, uint64_t pixels, uint8_t* yuv);

private:
    bool WriteRecord(const uint8_t* yuv);

    std::FILE* m_File = nullptr;
    uint32_t m_Width = 0, m_Height = 0;
    uint64_t m_Frames = 0;
    std::vector<uint8_t> m_Planes;  // SubmitFrame's conversion scratch
};

}  // namespace Trident
