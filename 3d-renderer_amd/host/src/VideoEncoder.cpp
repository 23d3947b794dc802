// VideoEncoder.cpp — the Y4M writer with the host-side colour conversion, and the Matroska Motion-JPEG writer with
// the host-side JPEG encoder (see VideoEncoder.h).
#include "trident/VideoEncoder.h"

#include <cctype>
#include <cstring>

#include "../../csrc/jpeg_math.h"

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

// EBML: an element is its id (as given, big-endian), its size as a variable-length integer, its payload.
struct Ebml {
    std::vector<uint8_t> b;
    void Id(uint32_t id) {
        for (int s = 24; s >= 0; s -= 8)
            if ((id >> s) != 0) b.push_back((uint8_t)(id >> s));
    }
    void Size(uint64_t n) {  // the shortest form; all-ones payloads are reserved ("unknown"), so 127 takes two bytes
        int len = 1;
        while (len < 8 && n >= (1ull << (7 * len)) - 1) ++len;
        b.push_back((uint8_t)((1u << (8 - len)) | (n >> (8 * (len - 1)))));
        for (int s = 8 * (len - 2); s >= 0; s -= 8) b.push_back((uint8_t)(n >> s));
    }
    void UInt(uint32_t id, uint64_t v) {
        int len = 1;
        while (len < 8 && (v >> (8 * len)) != 0) ++len;
        Id(id);
        Size(len);
        for (int s = 8 * (len - 1); s >= 0; s -= 8) b.push_back((uint8_t)(v >> s));
    }
    void String(uint32_t id, const char* text) {
        Id(id);
        Size(std::strlen(text));
        b.insert(b.end(), text, text + std::strlen(text));
    }
    void Float64(uint32_t id, double v) {
        uint64_t u;
        std::memcpy(&u, &v, 8);
        Id(id);
        Size(8);
        for (int s = 56; s >= 0; s -= 8) b.push_back((uint8_t)(u >> s));
    }
    void Master(uint32_t id, const Ebml& body) {
        Id(id);
        Size(body.b.size());
        b.insert(b.end(), body.b.begin(), body.b.end());
    }
    void UnknownSize() { b.insert(b.end(), {0x01, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF}); }
};

void Size8(uint64_t n, uint8_t (&out)[8]) {  // the 8-byte form of a size, for a patched field
    out[0] = 0x01;
    for (int i = 1; i < 8; ++i) out[i] = (uint8_t)(n >> (8 * (7 - i)));
}

}  // namespace

VideoEncoder::~VideoEncoder() { EndSession(); }

bool VideoEncoder::SetQuality(uint32_t quality) {
    jpeg::Msg m;
    if (jpeg::check_quality(quality, m)) return false;
    m_Quality = quality;
    return true;
}

bool VideoEncoder::SetRestartInterval(uint32_t restartMcus) {
    jpeg::Msg m;
    if (jpeg::check_restart(restartMcus, m)) return false;
    m_RestartMcus = restartMcus;
    return true;
}

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
    if (ext != ".y4m" && ext != ".mkv") {
        LogWarn("session refused, only .y4m and .mkv output is written: ", path);
        return false;
    }
    const bool mkv = ext == ".mkv";
    jpeg::Msg msg;
    if (mkv && jpeg::check_extent(width, height, msg)) {
        LogWarn("session refused, a JPEG frame cannot have ", std::string(msg.text) + ": " + path);
        return false;
    }
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) {
        LogWarn("could not open the output file: ", path);
        return false;
    }
    const uint32_t fps = targetFps == 0 ? 30u : targetFps;
    if (mkv) {
        m_File = f;
        m_Mkv = true;
        m_Width = width;
        m_Height = height;
        m_Fps = fps;
        m_Pos = 0;
        m_ClusterSizeAt = -1;
        if (!MkvWriteHeader() || std::fflush(m_File) != 0) {
            Abandon("could not write the stream header");
            return false;
        }
        return true;
    }
    m_Mkv = false;
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

void VideoEncoder::Abandon(const char* why) {
    LogWarn(why, ": the session was ended");
    std::fclose(m_File);
    m_File = nullptr;
}

bool VideoEncoder::MkvWrite(const void* data, size_t bytes) {
    if (std::fwrite(data, 1, bytes, m_File) != bytes) return false;
    m_Pos += bytes;
    return true;
}

// Overwrite `bytes` at file offset `at`, then return to the end.
bool VideoEncoder::MkvPatch(long at, const void* data, size_t bytes) {
    if (std::fseek(m_File, at, SEEK_SET) != 0) return false;
    const bool ok = std::fwrite(data, 1, bytes, m_File) == bytes;
    return std::fseek(m_File, 0, SEEK_END) == 0 && ok;
}

bool VideoEncoder::MkvWriteHeader() {
    Ebml head, file;
    head.UInt(0x4286, 1);  // EBMLVersion
    head.UInt(0x42F7, 1);  // EBMLReadVersion
    head.UInt(0x42F2, 4);  // EBMLMaxIDLength
    head.UInt(0x42F3, 8);  // EBMLMaxSizeLength
    head.String(0x4282, "matroska");
    head.UInt(0x4287, 4);  // DocTypeVersion
    head.UInt(0x4285, 2);  // DocTypeReadVersion
    file.Master(0x1A45DFA3, head);
    file.Id(0x18538067);  // Segment
    m_SegmentSizeAt = (long)file.b.size();
    file.UnknownSize();
    m_SegmentDataAt = file.b.size();
    Ebml info;
    info.UInt(0x2AD7B1, 1000000);  // TimecodeScale: milliseconds
    info.String(0x4D80, "trident_renderer");
    info.String(0x5741, "trident_renderer");
    info.Float64(0x4489, 0.0);  // Duration, patched by EndSession
    file.Id(0x1549A966);
    file.Size(info.b.size());
    m_DurationAt = (long)(file.b.size() + info.b.size() - 8);
    file.b.insert(file.b.end(), info.b.begin(), info.b.end());
    Ebml video, entry, tracks;
    video.UInt(0xB0, m_Width);
    video.UInt(0xBA, m_Height);
    entry.UInt(0xD7, 1);    // TrackNumber
    entry.UInt(0x73C5, 1);  // TrackUID
    entry.UInt(0x83, 1);    // TrackType: video
    entry.UInt(0x9C, 0);    // FlagLacing
    entry.String(0x86, "V_MJPEG");
    entry.UInt(0x23E383, (1000000000ull + m_Fps / 2) / m_Fps);  // DefaultDuration: round(1e9 / fps) ns
    entry.Master(0xE0, video);
    tracks.Master(0xAE, entry);
    file.Master(0x1654AE6B, tracks);
    return MkvWrite(file.b.data(), file.b.size());
}

bool VideoEncoder::MkvCloseCluster() {
    if (m_ClusterSizeAt < 0) return true;
    uint8_t size[8];
    Size8(m_Pos - m_ClusterDataAt, size);
    const long at = m_ClusterSizeAt;
    m_ClusterSizeAt = -1;
    return MkvPatch(at, size, 8);
}

bool VideoEncoder::MkvWriteBlock(const uint8_t* data, uint64_t bytes) {
    const uint64_t ms = (2000ull * m_Frames + m_Fps) / (2ull * m_Fps);  // round(1000 n / fps)
    if (m_ClusterSizeAt >= 0 && ms - m_ClusterMs >= 1000) {
        if (!MkvCloseCluster()) return false;
    }
    Ebml e;
    if (m_ClusterSizeAt < 0) {
        e.Id(0x1F43B675);
        m_ClusterSizeAt = (long)(m_Pos + e.b.size());
        e.UnknownSize();
        m_ClusterDataAt = m_Pos + e.b.size();
        m_ClusterMs = ms;
        e.UInt(0xE7, ms);  // Timecode
    }
    const uint32_t rel = (uint32_t)(ms - m_ClusterMs);  // < 1000
    e.Id(0xA3);
    e.Size(bytes + 4);
    e.b.insert(e.b.end(), {0x81, (uint8_t)(rel >> 8), (uint8_t)rel, 0x80});
    if (!MkvWrite(e.b.data(), e.b.size()) || !MkvWrite(data, (size_t)bytes) || std::fflush(m_File) != 0) return false;
    ++m_Frames;
    return true;
}

bool VideoEncoder::MkvFinish() {
    bool ok = MkvCloseCluster();
    uint8_t size[8];
    Size8(m_Pos - m_SegmentDataAt, size);
    ok = MkvPatch(m_SegmentSizeAt, size, 8) && ok;
    const double ms = 1000.0 * (double)m_Frames / (double)m_Fps;
    Ebml d;
    uint64_t u;
    std::memcpy(&u, &ms, 8);
    for (int s = 56; s >= 0; s -= 8) d.b.push_back((uint8_t)(u >> s));
    return MkvPatch(m_DurationAt, d.b.data(), 8) && ok;
}

bool VideoEncoder::SubmitJpeg(const uint8_t* data, uint64_t bytes, uint32_t width, uint32_t height) {
    if (!m_File || !m_Mkv || !data) return false;
    if (width != m_Width || height != m_Height) return false;
    if (bytes < 4 || data[0] != 0xFF || data[1] != 0xD8 || data[bytes - 2] != 0xFF || data[bytes - 1] != 0xD9) return false;
    if (!MkvWriteBlock(data, bytes)) {
        Abandon("a frame could not be written");
        return false;
    }
    return true;
}

bool VideoEncoder::SubmitFrame(const RecordedFrame& frame) {
    if (!m_File) return false;
    if (frame.m_Pixels.empty()) return false;
    if (frame.m_Width != m_Width || frame.m_Height != m_Height) return false;
    const uint64_t pixels = (uint64_t)m_Width * m_Height;
    if (frame.m_Pixels.size() < pixels * 4) return false;  // fewer bytes than the extent says
    if (m_Mkv) {
        const jpeg::Layout l = jpeg::make_layout(m_Width, m_Height, m_RestartMcus);
        jpeg::Tables t;
        jpeg::build_tables(m_Quality, t);
        m_Coefficients.resize((size_t)l.mcus * jpeg::kCoefPerMcu);
        m_Jpeg.resize((size_t)jpeg::max_bytes(l));
        const uint64_t n = jpeg::encode_image(frame.m_Pixels.data(), m_Width * 4u, 0, 2, l, t, m_Coefficients.data(), m_Jpeg.data());
        return SubmitJpeg(m_Jpeg.data(), n, m_Width, m_Height);
    }
    m_Planes.resize(pixels * 3);
    ConvertRgbaToYuv444(frame.m_Pixels.data(), pixels, m_Planes.data());
    return WriteRecord(m_Planes.data());
}

bool VideoEncoder::SubmitPlanes(const uint8_t* yuv, uint32_t width, uint32_t height) {
    if (!m_File || !yuv || m_Mkv) return false;
    if (width != m_Width || height != m_Height) return false;
    return WriteRecord(yuv);
}

bool VideoEncoder::EndSession() {
    if (!m_File) return false;
    const bool finished = !m_Mkv || MkvFinish();
    if (!finished) LogWarn("the Matroska sizes could not be patched", "");
    const bool ok = std::fflush(m_File) == 0 && finished;
    const bool closed = std::fclose(m_File) == 0;
    m_File = nullptr;
    return ok && closed;
}

}  // namespace Trident
