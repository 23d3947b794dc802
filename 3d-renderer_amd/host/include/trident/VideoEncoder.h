// VideoEncoder.h — Trident::VideoEncoder (Trident/src/Renderer/VideoEncoder.h:27-100) for the Y4M container: the
// session rules, the header and the FRAME records of the reference, and its RGBA -> YUV 4:4:4 conversion restated
// in the same double-precision operation order. The reference hands .mp4 / .mov / .avi to FFmpeg; FFmpeg is not part
// of this project, so those containers are refused with a log line that says so (a documented deviation).
// SubmitPlanes is this project's addition: frames the device has converted already (tri_recorder).
//
// A second container is this project's own: .mkv, Matroska with one V_MJPEG track. Every frame is a baseline JPEG by
// csrc/jpeg_math.h's rule, encoded here on the host from RGBA (SubmitFrame) or taken as the device encoded it
// (SubmitJpeg). The writer follows the Matroska specification with no library: EBML header, a Segment of unknown
// size with Info and Tracks, then Clusters (a new one at least once per second of video) of SimpleBlocks, every frame
// a keyframe with the timecode round(1000 n / fps) ms. Segment and Cluster sizes and the Duration are patched when
// the element closes, so a file whose session was never ended is still a valid live-style stream.
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
    // creating a file, for a zero extent, an FFmpeg container or any extension but .y4m and .mkv (compared
    // lower-cased; .mkv also for an extent side above 65535). targetFps 0 means 30.
    bool BeginSession(const std::string& path, uint32_t width, uint32_t height, uint32_t targetFps);
    // One FRAME record (.y4m) or one SimpleBlock (.mkv) from RGBA pixels, converted or encoded here on the host. False
    // (nothing written) without a session, for an empty pixel buffer, or an extent that is not the session's.
    bool SubmitFrame(const RecordedFrame& frame);
    // One FRAME record from 3 * width * height bytes converted already (Y, U, V planes). Same refusals, and refused
    // by an .mkv session.
    bool SubmitPlanes(const uint8_t* yuv, uint32_t width, uint32_t height);
    // One SimpleBlock from a complete JPEG of the session's extent, encoded already (tri_recorder_wait_ex). Same
    // refusals, and refused by a .y4m session and for a stream that does not run from SOI to EOI.
    bool SubmitJpeg(const uint8_t* jpeg, uint64_t bytes, uint32_t width, uint32_t height);
    // The JPEG parameters of SubmitFrame on an .mkv session: sticky across sessions. Quality 1..100 (default 90);
    // the restart interval in MCUs, 1..65535, 0 = the rule's default. False (unchanged) outside the range.
    bool SetQuality(uint32_t quality);
    bool SetRestartInterval(uint32_t restartMcus);
    uint32_t GetQuality() const { return m_Quality; }
    uint32_t GetRestartInterval() const { return m_RestartMcus; }
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
    // the Matroska writer
    bool MkvWrite(const void* data, size_t bytes);
    bool MkvPatch(long at, const void* data, size_t bytes);
    bool MkvWriteHeader();
    bool MkvWriteBlock(const uint8_t* jpeg, uint64_t bytes);
    bool MkvCloseCluster();
    bool MkvFinish();
    void Abandon(const char* why);  // a failed write: log, close the file, end the session

    std::FILE* m_File = nullptr;
    uint32_t m_Width = 0, m_Height = 0;
    uint64_t m_Frames = 0;
    std::vector<uint8_t> m_Planes;  // SubmitFrame's conversion scratch
    bool m_Mkv = false;
    uint32_t m_Fps = 30, m_Quality = 90, m_RestartMcus = 0;
    uint64_t m_Pos = 0;                        // bytes written so far (the file offset of the next byte)
    long m_SegmentSizeAt = 0, m_DurationAt = 0;  // where the patched fields are
    long m_ClusterSizeAt = -1;                 // -1: no cluster is open
    uint64_t m_ClusterMs = 0, m_SegmentDataAt = 0, m_ClusterDataAt = 0;
    std::vector<int16_t> m_Coefficients;       // SubmitFrame's JPEG scratch
    std::vector<uint8_t> m_Jpeg;
};

}  // namespace Trident
