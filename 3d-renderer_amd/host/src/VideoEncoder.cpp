// VideoEncoder.cpp — the Y4M writer and the host-side colour conversion (see VideoEncoder.h).
#include "trident/VideoEncoder.h"

#include <cctype>

namespace Trident {

namespace {

void LogWarn(const char* what, const std::string& detail) {
    std::fprintf(stderr, "[Trident] VideoEncoder: %s%s\n", what, detail.c_str());
}

// The path's extension (from the last '.' of its last component), lower-cased; empty without one.
std::string LowerExtension(const std::string& path) {
    const size_t slash = path.find_last_of("/\\");
    const size_t dot = path.find_last_of('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return {};
    std::string ext = path.substr(dot);
    for (char& c : ext) c = (char)std::tolower((unsigned char)c);
    return ext;
}

inline uint8_t ToByte(double v) {  // ClampChannel (VideoEncoder.cpp:701-714): clamp, then truncate
    if (v < 0.0) return 0;
    if (v > 255.0) return 255;
    return (uint8_t)v;
}

}  // namespace

VideoEncoder::~VideoEncoder() { EndSession(); }

void VideoEncoder::ConvertRgbaToYuv444(const uint8_t* rgba, uint64_t pixels, uint8_t* yuv) {
    uint8_t* yp = yuv;
    uint8_t* up = yuv + pixels;
    uint8_t* vp = yuv + 2 * pixels;
    for (uint64_t i = 0; i < pixels; ++i) {
        const double r = rgba[4 * i + 0], g = rgba[4 * i + 1], b = rgba[4 * i + 2];
        yp[i] = ToByte(0.299 * r + 0.587 * g + 0.114 * b);
        up[i] = ToByte(-0.169 * r - 0.331 * g + 0.5 * b + 128.0);
        vp[i] = ToByte(0.5 * r - 0.419 * g - 0.081 * b + 128.0);
    }
}

bool VideoEncoder::BeginSession(const std::string& path, uint32_t width, uint32_t height, uint32_t targetFps) {
    EndSession();
    m_Frames = 0;
    if (width == 0 || height == 0) {
        LogWarn("session refused, the extent has a zero side: ", path);
        return false;
    }
    const std::string ext = LowerExtension(path);
    if (ext == ".mp4" || ext == ".mov" || ext == ".avi") {
        LogWarn("session refused, this container needs FFmpeg, which this build does not include (use .y4m): ", path);
        return false;
    }
    if (ext != ".y4m") {
        LogWarn("session refused, only .y4m output is written: ", path);
        return false;
    }
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) {
        LogWarn("could not open the output file: ", path);
        return false;
    }
    const uint32_t fps = targetFps == 0 ? 30u : targetFps;
    if (std::fprintf(f, "YUV4MPEG2 W%u H%u F%u:1 Ip A0:0 C444\n", width, height, fps) < 0) {
        LogWarn("could not write the stream header: ", path);
        std::fclose(f);
        return false;
    }
    m_File = f;
    m_Width = width;
    m_Height = height;
    return true;
}

bool VideoEncoder::WriteRecord(const uint8_t* yuv) {
    const size_t bytes = (size_t)3 * m_Width * m_Height;
    if (std::fwrite("FRAME\n", 1, 6, m_File) != 6 || std::fwrite(yuv, 1, bytes, m_File) != bytes) {
        LogWarn("a frame record could not be written", "");
        return false;
    }
    ++m_Frames;
    return true;
}

bool VideoEncoder::SubmitFrame(const RecordedFrame& frame) {
    if (!m_File) return false;
    if (frame.m_Pixels.empty()) return false;
    if (frame.m_Width != m_Width || frame.m_Height != m_Height) return false;
    const uint64_t pixels = (uint64_t)m_Width * m_Height;
    if (frame.m_Pixels.size() < pixels * 4) return false;  // fewer bytes than the extent says
    m_Planes.resize(pixels * 3);
    ConvertRgbaToYuv444(frame.m_Pixels.data(), pixels, m_Planes.data());
    return WriteRecord(m_Planes.data());
}

bool VideoEncoder::SubmitPlanes(const uint8_t* yuv, uint32_t width, uint32_t height) {
    if (!m_File || !yuv) return false;
    if (width != m_Width || height != m_Height) return false;
    return WriteRecord(yuv);
}

bool VideoEncoder::EndSession() {
    if (!m_File) return false;
    const bool ok = std::fflush(m_File) == 0;
    const bool closed = std::fclose(m_File) == 0;
    m_File = nullptr;
    return ok && closed;
}

}  // namespace Trident
