// jpeg_check — host-only check of the Motion-JPEG recorder's plain-C++ part (csrc/jpeg_math.h, the text the kernels
// compile) and of Trident::VideoEncoder's Matroska writer, built under the address and undefined-behaviour sanitizers
// (make jpeg-check). No device, no Python. Every output buffer is a heap array of exactly the size the header's bound
// gives, so a byte beyond the bound is an error the address sanitizer reports. Groups:
//   1. the argument rules; the header bytes; the code tables against the size bound's two maxima;
//   2. blocks built to approach the bound (every AC coefficient of category 10 behind a category-11 DC difference),
//      whole planes of them through the scan writer; every symbol class with its bit count written out by hand;
//   3. stuffing, padding and the RST sequence with its wrap-around;
//   4. images of 1 x 1, 17 x 9, 16 x 16 and 33 x 31 decoded again by the shim's own JPEG decoder;
//   5. the Matroska writer: a good file's layout, a path that cannot be opened, and a device that takes no bytes.
// argv[1]: a scratch directory for the files.
#include "../../csrc/jpeg_math.h"
#include "trident/ImageDecoder.h"
#include "trident/VideoEncoder.h"

#include <unistd.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

int g_failures = 0;

#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++g_failures;                                                         \
        }                                                                         \
    } while (0)

uint32_t block_bits(const int16_t* zz, int pred, const jpeg::Tables& t, uint32_t tab, uint32_t* symbols = nullptr) {
    uint32_t bits = 0, n = 0;
    jpeg::encode_block(zz, pred, t.huff[tab], t.huff[2 + tab], [&](uint32_t v, uint32_t c) {
        EXPECT(c >= 2 && c <= 26 && (c == 32 || (v >> c) == 0));
        bits += c;
        ++n;
    });
    if (symbols) *symbols = n;
    return bits;
}

void argument_rules() {
    jpeg::Msg m;
    EXPECT(jpeg::check_quality(0, m) == TRI_E_INVALID && m.text[0]);
    EXPECT(jpeg::check_quality(101, m) == TRI_E_INVALID);
    EXPECT(jpeg::check_quality(1, m) == TRI_OK && jpeg::check_quality(100, m) == TRI_OK);
    EXPECT(jpeg::check_restart(0, m) == TRI_OK && jpeg::check_restart(65535, m) == TRI_OK);
    EXPECT(jpeg::check_restart(65536, m) == TRI_E_INVALID);
    EXPECT(jpeg::check_extent(0, 1, m) == TRI_E_INVALID && jpeg::check_extent(1, 0, m) == TRI_E_INVALID);
    EXPECT(jpeg::check_extent(65536, 1, m) == TRI_E_INVALID && jpeg::check_extent(1, 65536, m) == TRI_E_INVALID);
    EXPECT(jpeg::check_extent(1, 1, m) == TRI_OK && jpeg::check_extent(65535, 65535, m) == TRI_OK);
    EXPECT(jpeg::check_capacity(10, 9, m) == TRI_E_INVALID && jpeg::check_capacity(10, 10, m) == TRI_OK);
    tri_record_params p{TRI_RECORD_JPEG420, 90, 0, 0};
    EXPECT(jpeg::check_params(&p, m) == TRI_OK);
    EXPECT(jpeg::check_params(nullptr, m) == TRI_E_INVALID);
    p.flags = 1;
    EXPECT(jpeg::check_params(&p, m) == TRI_E_INVALID);
    p = {2, 90, 0, 0};
    EXPECT(jpeg::check_params(&p, m) == TRI_E_INVALID);
    p = {TRI_RECORD_YUV444, 0, 70000, 0};  // the JPEG fields do not matter to the other format
    EXPECT(jpeg::check_params(&p, m) == TRI_OK);
    p = {TRI_RECORD_JPEG420, 0, 0, 0};
    EXPECT(jpeg::check_params(&p, m) == TRI_E_INVALID);
    // the layout: the largest extent's counts fit their types, intervals and segments as stated
    const jpeg::Layout big = jpeg::make_layout(65535, 65535, 1);
    EXPECT(big.mcus_x == 4096 && big.mcus == 4096u * 4096u && big.intervals == big.mcus);
    const jpeg::Layout l = jpeg::make_layout(48, 32, 4);
    EXPECT(l.mcus == 6 && l.intervals == 2 && l.restart == 4 && l.segment_bytes % 16 == 0);
    EXPECT(l.segment_bytes >= jpeg::interval_bound_bytes(4));
    EXPECT(jpeg::make_layout(48, 32, 65535).segment_bytes >= jpeg::interval_bound_bytes(6));
    EXPECT(jpeg::make_layout(48, 32, 0).restart == jpeg::kDefaultRestartMcus);
    EXPECT(jpeg::max_bytes(l) == jpeg::kHeaderBytes + jpeg::interval_bound_bytes(4) + 2 + jpeg::interval_bound_bytes(2) + 2);
}

void header_and_tables() {
    jpeg::Tables t;
    jpeg::build_tables(50, t);
    for (int i = 0; i < 64; ++i) EXPECT(t.q[0][i] == jpeg::kLumaQ[i] && t.q[1][i] == jpeg::kChromaQ[i]);  // quality 50: s = 100
    jpeg::build_tables(100, t);
    for (int i = 0; i < 64; ++i) EXPECT(t.q[0][i] == 1 && t.q[1][i] == 1);
    jpeg::build_tables(1, t);
    EXPECT(t.q[0][0] == 255 && t.q[1][63] == 255);
    jpeg::build_tables(90, t);
    EXPECT(t.q[0][0] == 3 && t.q[0][63] == 20);
    for (int i = 0; i < 64; ++i) EXPECT(jpeg::kZigzag[t.izz[i]] == i);
    // the bound's two maxima: a DC code with its bits, an AC code with its bits
    uint32_t dc = 0, ac = 0;
    for (int tab = 0; tab < 2; ++tab) {
        for (uint32_t c = 0; c <= 11; ++c) {
            EXPECT(t.huff[tab][c] != 0);
            if ((t.huff[tab][c] >> 16) + c > dc) dc = (t.huff[tab][c] >> 16) + c;
        }
        for (uint32_t r = 0; r < 16; ++r)
            for (uint32_t c = 1; c <= 10; ++c) {
                EXPECT(t.huff[2 + tab][(r << 4) | c] != 0);
                if ((t.huff[2 + tab][(r << 4) | c] >> 16) + c > ac) ac = (t.huff[2 + tab][(r << 4) | c] >> 16) + c;
            }
        EXPECT((t.huff[2 + tab][0xF0] >> 16) <= 16 * 26 && t.huff[2 + tab][0x00] != 0);
    }
    EXPECT(dc == 22 && ac == 26 && jpeg::kMaxBlockBits == dc + 63 * ac);
    // the header
    const jpeg::Layout l = jpeg::make_layout(321, 203, 7);
    std::unique_ptr<uint8_t[]> h(new uint8_t[jpeg::kHeaderBytes]);
    EXPECT(jpeg::write_header(l, t, h.get()) == jpeg::kHeaderBytes);
    EXPECT(h[0] == 0xFF && h[1] == 0xD8 && h[2] == 0xFF && h[3] == 0xE0 && std::memcmp(h.get() + 6, "JFIF", 5) == 0);
    EXPECT(h[20] == 0xFF && h[21] == 0xDB && h[24] == 0 && h[25] == 3);        // luma DQT, Q[0] at quality 90
    EXPECT(h[89] == 0xFF && h[90] == 0xDB && h[93] == 1);                      // chroma DQT
    EXPECT(h[158] == 0xFF && h[159] == 0xC0 && h[163] == 0 && h[164] == 203 && h[165] == 1 && h[166] == 65);  // 203 x 321
    EXPECT(h[168] == 1 && h[169] == 0x22 && h[171] == 2 && h[172] == 0x11);
    EXPECT(h[609] == 0xFF && h[610] == 0xDD && h[613] == 0 && h[614] == 7);    // DRI
    EXPECT(h[615] == 0xFF && h[616] == 0xDA && h[626] == 0 && h[627] == 63 && h[628] == 0);
}

void blocks_at_the_bound() {
    jpeg::Tables t;
    jpeg::build_tables(100, t);
    int16_t zz[64];
    // the heaviest block: a category-11 DC difference, every AC coefficient of category 10
    zz[0] = -1024;
    for (int i = 1; i < 64; ++i) zz[i] = (int16_t)((i & 1) ? 1023 : -1023);
    uint32_t symbols = 0;
    EXPECT(block_bits(zz, 1023, t, 0, &symbols) == 9 + 11 + 63 * 26 && symbols == 64);  // luma: 1658 bits
    const uint32_t chroma = block_bits(zz, 1023, t, 1);
    EXPECT(chroma == 11 + 11 + 63 * ((t.huff[3][0x0A] >> 16) + 10) && chroma <= jpeg::kMaxBlockBits);
    // planes of such blocks, DC alternating between the extremes, through the scan writer into exactly max_bytes
    for (const uint32_t restart : {1u, 3u, 65535u}) {
        const jpeg::Layout l = jpeg::make_layout(80, 48, restart);
        std::vector<int16_t> coef((size_t)l.mcus * jpeg::kCoefPerMcu);
        for (size_t b = 0; b < (size_t)l.mcus * 6; ++b)
            for (int i = 0; i < 64; ++i)
                coef[b * 64 + i] = i == 0 ? (int16_t)((b & 1) ? 1023 : -1024) : (int16_t)(((i + b) % 3) ? -1023 : 1023);
        const uint64_t cap = jpeg::max_bytes(l);
        std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
        const uint32_t h = jpeg::write_header(l, t, out.get());
        const uint8_t* end = jpeg::encode_scan(coef.data(), l, t, out.get() + h);
        const uint64_t n = (uint64_t)(end - out.get());
        EXPECT(n <= cap && end[-2] == 0xFF && end[-1] == 0xD9);
        EXPECT(n > jpeg::kHeaderBytes + (uint64_t)l.mcus * 6 * 1500 / 8);  // and it does approach the bound
    }
    // the symbol classes, bit counts by hand from Annex K.3
    int16_t z[64] = {0};
    EXPECT(block_bits(z, 0, t, 0, &symbols) == 2 + 4 && symbols == 2);          // all zero: DC category 0, EOB
    EXPECT(block_bits(z, 0, t, 1) == 2 + 2);
    z[63] = 1;                                                                    // three ZRL, then run 14 size 1; no EOB
    EXPECT(block_bits(z, 0, t, 0, &symbols) == 2 + 3 * 11 + (t.huff[2][0xE1] >> 16) + 1 && symbols == 5);
    EXPECT((t.huff[2][0xF0] >> 16) == 11 && (t.huff[3][0xF0] >> 16) == 10 && (t.huff[2][0xE1] >> 16) == 16);
    z[63] = 0;
    z[17] = -5;                                                                   // one ZRL, run 0 size 3, EOB
    EXPECT(block_bits(z, 0, t, 0, &symbols) == 2 + 11 + (t.huff[2][0x03] >> 16) + 3 + 4 && symbols == 4);
    z[17] = 0;
    z[0] = 1023;                                                                  // DC: -1024 -> 1023 is category 11
    EXPECT(block_bits(z, -1024, t, 0) == 9 + 11 + 4);
    EXPECT(jpeg::bit_length(2047) == 11 && jpeg::bit_length(1023) == 10 && jpeg::bit_length(1) == 1 && jpeg::bit_length(0) == 0);
    // the quantiser: half away from zero, the clamps
    EXPECT(jpeg::quantise(3 << 15, 3, false) == 1 && jpeg::quantise(-(3 << 15), 3, false) == -1);
    EXPECT(jpeg::quantise((3 << 15) - 1, 3, false) == 0 && jpeg::quantise(-(3 << 15) + 1, 3, false) == 0);
    EXPECT(jpeg::quantise(-1024 * 65536, 1, true) == -1024 && jpeg::quantise(-1024 * 65536, 1, false) == -1023);
    EXPECT(jpeg::quantise(1024 << 16, 1, true) == 1023);
    // the colour rule's range, on every corner and along the axes
    for (int r = 0; r < 256; r += 51)
        for (int g = 0; g < 256; g += 51)
            for (int b = 0; b < 256; b += 51) {
                const jpeg::Ycc c = jpeg::ycc(r, g, b);
                EXPECT(c.y >= 0 && c.y <= 255 && c.cb >= 0 && c.cb <= 255 && c.cr >= 0 && c.cr <= 255);
                if (r == g && g == b) EXPECT(c.y == r && c.cb == 128 && c.cr == 128);
            }
    // a flat block: the DC alone, 8 x the level-shifted sample
    int s[64];
    for (int& v : s) v = -128;
    int16_t c[64];
    jpeg::block_coefficients(s, t.q[0], t.izz, c);
    EXPECT(c[0] == -1024);
    for (int i = 1; i < 64; ++i) EXPECT(c[i] == 0);
    for (int& v : s) v = 127;
    jpeg::block_coefficients(s, t.q[0], t.izz, c);
    EXPECT(c[0] == 1016);
}

void stuffing_and_restarts() {
    std::unique_ptr<uint8_t[]> buf(new uint8_t[8]);
    jpeg::BitWriter w(buf.get());
    w.put(0xFF, 8);
    w.put(0x3, 2);
    w.pad();
    w.marker(0xD3);
    // (0b11 padded with six one-bits is 0xFF too: it is stuffed like any other byte)
    EXPECT(w.p - buf.get() == 6 && buf[0] == 0xFF && buf[1] == 0x00 && buf[2] == 0xFF && buf[3] == 0x00 && buf[4] == 0xFF &&
           buf[5] == 0xD3);
    std::unique_ptr<uint8_t[]> buf2(new uint8_t[6]);
    jpeg::BitWriter w2(buf2.get());
    w2.put(0x3, 2);
    w2.pad();
    EXPECT(w2.p - buf2.get() == 2 && buf2[0] == 0xFF && buf2[1] == 0x00);
    // 32 x 176 with 2 MCUs per interval: 22 MCUs, 11 intervals, 10 markers: RST0..RST7, then RST0 and RST1 again
    const uint32_t W = 32, H = 176;
    std::vector<uint8_t> px((size_t)W * H * 4);
    uint32_t seed = 12345;
    for (uint8_t& v : px) v = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
    const jpeg::Layout l = jpeg::make_layout(W, H, 2);
    jpeg::Tables t;
    jpeg::build_tables(100, t);
    std::vector<int16_t> coef((size_t)l.mcus * jpeg::kCoefPerMcu);
    const uint64_t cap = jpeg::max_bytes(l);
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
    const uint64_t n = jpeg::encode_image(px.data(), W * 4, 2, 0, l, t, coef.data(), out.get());
    EXPECT(n <= cap && l.intervals == 11);
    uint32_t next = 0, stuffed = 0;
    for (uint64_t i = jpeg::kHeaderBytes; i + 1 < n; ++i) {
        if (out[i] != 0xFF) continue;
        if (out[i + 1] == 0) ++stuffed;
        else if (out[i + 1] >= 0xD0 && out[i + 1] <= 0xD7) EXPECT(out[i + 1] == 0xD0 + (next++ & 7));
        else EXPECT(out[i + 1] == 0xD9 && i + 2 == n);
        ++i;
    }
    EXPECT(next == 10 && stuffed > 0);  // (the loop checked marker 8 against RST0 and marker 9 against RST1)
}

void round_trips() {
    struct Case { uint32_t w, h, restart; };
    for (const Case c : {Case{1, 1, 0}, Case{17, 9, 1}, Case{16, 16, 0}, Case{33, 31, 2}}) {
        std::vector<uint8_t> rgba((size_t)c.w * c.h * 4);
        for (uint32_t y = 0; y < c.h; ++y)
            for (uint32_t x = 0; x < c.w; ++x) {  // smooth, so that 4:2:0 keeps it
                uint8_t* p = &rgba[((size_t)y * c.w + x) * 4];
                p[0] = (uint8_t)(40 + 5 * x);
                p[1] = (uint8_t)(200 - 4 * y);
                p[2] = (uint8_t)(90 + 2 * x + 2 * y);
                p[3] = (uint8_t)(x * 7 + y);  // alpha is ignored
            }
        const jpeg::Layout l = jpeg::make_layout(c.w, c.h, c.restart);
        jpeg::Tables t;
        jpeg::build_tables(95, t);
        std::vector<int16_t> coef((size_t)l.mcus * jpeg::kCoefPerMcu);
        const uint64_t cap = jpeg::max_bytes(l);
        std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
        const uint64_t n = jpeg::encode_image(rgba.data(), c.w * 4, 0, 2, l, t, coef.data(), out.get());
        EXPECT(n <= cap);
        int w = 0, h = 0;
        std::vector<uint8_t> back;
        std::string error;
        const std::string bytes(reinterpret_cast<const char*>(out.get()), (size_t)n);
        EXPECT(Trident::Loader::IsJpeg(bytes));
        const bool ok = Trident::Loader::DecodeJpeg(bytes, w, h, back, error);
        EXPECT(ok && w == (int)c.w && h == (int)c.h && back.size() == rgba.size());
        if (!ok || back.size() != rgba.size()) {
            std::fprintf(stderr, "  %u x %u: %s\n", c.w, c.h, error.c_str());
            continue;
        }
        long worst = 0, sum = 0;
        for (size_t i = 0; i < rgba.size(); ++i) {
            if ((i & 3) == 3) continue;
            const long d = std::labs((long)rgba[i] - (long)back[i]);
            worst = d > worst ? d : worst;
            sum += d;
        }
        // quality 95 on a smooth image: quantisers of 1..10, so a few levels at most
        EXPECT(worst <= 12 && sum <= 3 * (long)rgba.size() * 3 / 4);
        // the BGRA reading of the same bytes is the RGBA reading with red and blue exchanged
        std::vector<uint8_t> bgra(rgba);
        for (size_t i = 0; i < bgra.size(); i += 4) std::swap(bgra[i], bgra[i + 2]);
        std::unique_ptr<uint8_t[]> out2(new uint8_t[cap]);
        const uint64_t n2 = jpeg::encode_image(bgra.data(), c.w * 4, 2, 0, l, t, coef.data(), out2.get());
        EXPECT(n2 == n && std::memcmp(out.get(), out2.get(), (size_t)n) == 0);
    }
}

std::vector<uint8_t> read_file(const std::string& path) {
    std::vector<uint8_t> d;
    if (std::FILE* f = std::fopen(path.c_str(), "rb")) {
        uint8_t b[4096];
        size_t n;
        while ((n = std::fread(b, 1, sizeof b, f)) > 0) d.insert(d.end(), b, b + n);
        std::fclose(f);
    }
    return d;
}

void matroska(const std::string& dir) {
    Trident::VideoEncoder enc;
    Trident::VideoEncoder::RecordedFrame frame;
    frame.m_Width = 17;
    frame.m_Height = 9;
    frame.m_Pixels.assign(17 * 9 * 4, 0x60);
    EXPECT(!enc.SetQuality(0) && !enc.SetQuality(101) && enc.SetQuality(75) && enc.GetQuality() == 75);
    EXPECT(!enc.SetRestartInterval(65536) && enc.SetRestartInterval(1) && enc.GetRestartInterval() == 1);
    const std::string good = dir + "/good.MkV";
    EXPECT(enc.BeginSession(good, 17, 9, 0));
    const uint8_t planes[17 * 9 * 3] = {0};
    EXPECT(!enc.SubmitPlanes(planes, 17, 9));  // the wrong kind for this container
    for (int i = 0; i < 3; ++i) EXPECT(enc.SubmitFrame(frame));
    const uint8_t not_jpeg[4] = {0, 1, 2, 3};
    EXPECT(!enc.SubmitJpeg(not_jpeg, 4, 17, 9) && !enc.SubmitJpeg(nullptr, 4, 17, 9));
    EXPECT(enc.GetFrameCount() == 3 && enc.EndSession() && !enc.IsSessionActive());
    const std::vector<uint8_t> d = read_file(good);
    EXPECT(d.size() > 100 && d[0] == 0x1A && d[1] == 0x45 && d[2] == 0xDF && d[3] == 0xA3);
    // the Segment's patched size covers the rest of the file exactly
    size_t seg = 0;
    for (size_t i = 4; i + 12 < d.size() && !seg; ++i)
        if (d[i] == 0x18 && d[i + 1] == 0x53 && d[i + 2] == 0x80 && d[i + 3] == 0x67) seg = i;
    EXPECT(seg != 0 && d[seg + 4] == 0x01);
    uint64_t size = 0;
    for (int i = 1; i < 8; ++i) size = (size << 8) | d[seg + 4 + i];
    EXPECT(seg + 12 + size == d.size());
    // a .y4m session refuses a JPEG
    EXPECT(enc.BeginSession(dir + "/a.y4m", 17, 9, 30));
    const uint8_t tiny[4] = {0xFF, 0xD8, 0xFF, 0xD9};
    EXPECT(!enc.SubmitJpeg(tiny, 4, 17, 9) && enc.EndSession());
    // a path that cannot be opened; an extent a JPEG cannot have
    EXPECT(!enc.BeginSession(dir + "/no/such/dir/a.mkv", 17, 9, 30) && !enc.IsSessionActive());
    EXPECT(!enc.BeginSession(dir + "/wide.mkv", 65536, 9, 30) && read_file(dir + "/wide.mkv").empty());
    // a device that takes no bytes: every flush fails, the session ends and nothing crashes
    const std::string full = dir + "/full.mkv";
    if (symlink("/dev/full", full.c_str()) == 0) {
        const bool began = enc.BeginSession(full, 17, 9, 30);
        EXPECT(!began && !enc.IsSessionActive());
        EXPECT(!enc.SubmitFrame(frame) && !enc.EndSession());
        unlink(full.c_str());
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: jpeg_check <scratch directory>\n");
        return 2;
    }
    argument_rules();
    header_and_tables();
    blocks_at_the_bound();
    stuffing_and_restarts();
    round_trips();
    matroska(argv[1]);
    if (g_failures) {
        std::fprintf(stderr, "jpeg_check: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("jpeg_check: ok\n");
    return 0;
}
