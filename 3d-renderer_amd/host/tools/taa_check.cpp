// taa_check — host-only check of temporal anti-aliasing's plain-C++ part (csrc/taa_math.h), built under the address and
// undefined-behaviour sanitizers (make taa-check). No device. The per-pixel rule here is the very function k_taa_resolve
// compiles; every plane is a heap array of exactly W x H elements, so an index outside the frame is an error the address
// sanitizer reports. Groups:
//   1. rows that send the previous position anywhere: NaN, +-infinity, huge and negative u and v, q_3 <= 0 and NaN;
//   2. frames of 1 x 1, 3 x 200 and 200 x 3, every pixel — all borders and corners of both 3 x 3 windows;
//   3. the accumulation: alpha = 1, a flat pixel over 100 steps, a 0 -> 255 step, the clamp and its bit, the id test;
//   4. the jitter; the set bookkeeping (plain calls, a redo, a reset, a redo first); the argument rules.
#include "../../csrc/taa_math.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
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

void identity(float* m) {
    for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

// R that moves every point by (dx, dy) pixels of a W x H frame
void shift_row(float* m, uint32_t W, uint32_t H, float dx, float dy) {
    identity(m);
    m[3] = dx * 2.0f / (float)W;
    m[7] = dy * 2.0f / (float)H;
}

uint32_t grey(uint32_t v) { return v | v << 8 | v << 16 | v << 24; }
taa::Texel grey16(uint32_t v) { return taa::Texel{v | v << 16, v | v << 16}; }

// The current frame and the stored history, each plane of exactly W x H elements.
struct Planes {
    uint32_t W, H;
    std::vector<uint32_t> colour, prev_ids;
    std::vector<taa::Texel> prev_acc;
    Planes(uint32_t w, uint32_t h) : W(w), H(h), colour((size_t)w * h), prev_ids((size_t)w * h, 1u), prev_acc((size_t)w * h) {
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t p = (size_t)y * w + x;
                colour[p] = 0xFF000000u | ((x * 16u) & 0xFFu) << 8 | ((y * 16u) & 0xFFu);
                prev_acc[p] = taa::restart(colour[p], 0).acc;
            }
    }
    size_t at(uint32_t x, uint32_t y) const { return (size_t)y * W + x; }
};

taa::Pixel run(const Planes& p, const float* R, uint32_t x, uint32_t y, uint32_t id, float alpha = 0.1f, bool reject = true,
               bool has_prev = true) {
    const history::Frame f = history::make_frame(p.W, p.H, 0.0f);
    return taa::resolve_pixel(R, x, y, id, 0.5f, p.colour.data(), f, has_prev, reject, alpha, p.prev_ids.data(), p.prev_acc.data());
}

bool restarted(const taa::Pixel& o, uint32_t c) {
    const taa::Pixel r = taa::restart(c, o.mask);
    return o.resolved == c && o.acc.bg == r.acc.bg && o.acc.ra == r.acc.ra;
}

const float kNaN = std::numeric_limits<float>::quiet_NaN();
const float kInf = std::numeric_limits<float>::infinity();

void wild_positions() {
    Planes p(7, 5);
    float R[16];
    const float wild[] = {1e30f, -1e30f, 3.0e38f, -3.0e38f, 1e9f, -1e9f, -1.0f, 7.0f, 1e-30f};
    for (float a : wild)
        for (float b : wild)
            for (uint32_t y = 0; y < p.H; ++y)
                for (uint32_t x = 0; x < p.W; ++x) {
                    shift_row(R, p.W, p.H, a, b);
                    const taa::Pixel o = run(p, R, x, y, 1);
                    EXPECT((o.mask & ~taa::kClamped) == 0 || o.mask == taa::kOutside || o.mask == taa::kNoProj);
                    EXPECT((o.mask & 15u) == 0 || restarted(o, p.colour[p.at(x, y)]));
                }
    for (float bad : {kNaN, kInf, -kInf})
        for (int at : {0, 3, 5, 7, 2, 6}) {
            identity(R);
            R[at] = bad;
            for (uint32_t x = 0; x < p.W; ++x) {
                const taa::Pixel o = run(p, R, x, 2, 1);
                EXPECT(o.mask == taa::kNoProj || (o.mask & 15u) == 0);
                EXPECT((o.mask & 15u) == 0 || restarted(o, p.colour[p.at(x, 2)]));
            }
        }
    identity(R);
    R[3] = kNaN;
    EXPECT(run(p, R, 3, 2, 1).mask == taa::kNoProj);
    for (float q3 : {0.0f, -0.0f, -1.0f, kNaN, -kInf, 1e-45f}) {  // q_3 <= 0, NaN, and so small that 1 / q_3 overflows
        identity(R);
        R[15] = q3;
        const taa::Pixel o = run(p, R, 3, 2, 1);
        EXPECT(o.mask == taa::kNoProj && restarted(o, p.colour[p.at(3, 2)]));
    }
    shift_row(R, 8, 4, 0.5f, 0.0f);
    Planes q(8, 4);
    EXPECT(run(q, R, 7, 0, 1).mask == taa::kOutside);  // u = 7.5 + 0.5 = 8 = W
    shift_row(R, 8, 4, 0.0f, -1.0f);
    EXPECT(run(q, R, 0, 0, 1).mask == taa::kOutside);  // v = -0.5
}

// Every pixel of small and thin frames, still and under shifts that put the taps and both windows on every border.
void borders() {
    const uint32_t extents[][2] = {{1, 1}, {3, 200}, {200, 3}, {2, 2}, {8, 4}};
    float R[16];
    for (const auto& e : extents) {
        Planes p(e[0], e[1]);
        for (uint32_t k = 0; k < p.W * p.H; k += 3) p.prev_ids[k] = 2;  // a third of the previous ids are another draw's
        for (float dx : {0.0f, -0.49f, 0.49f, 1.0f, -1.0f})
            for (float dy : {0.0f, -0.49f, 0.49f, 1.0f, -1.0f}) {
                shift_row(R, p.W, p.H, dx, dy);
                for (uint32_t y = 0; y < p.H; ++y)
                    for (uint32_t x = 0; x < p.W; ++x)
                        for (uint32_t id : {1u, 2u, 3u}) {
                            const taa::Pixel o = run(p, R, x, y, id);
                            const uint32_t known = taa::kNoProj | taa::kOutside | taa::kId | taa::kClamped;
                            EXPECT((o.mask & ~known) == 0);
                            if (id == 3) EXPECT((o.mask & 15u) != 0);  // no previous pixel shows id 3
                            if (o.mask & 15u) EXPECT(restarted(o, p.colour[p.at(x, y)]));
                            if (dx == 0.0f && dy == 0.0f && !(o.mask & 15u)) {
                                // still: the tap is the pixel itself, whose stored value is its own colour: nothing moves
                                EXPECT(o.mask == 0 && restarted(o, p.colour[p.at(x, y)]));
                            }
                        }
            }
    }
    // the neighbourhood's range at a corner and in the interior, by hand
    Planes p(8, 4);
    const taa::Range c = taa::neighbourhood(p.colour.data(), 0, 0, p.W, p.H);
    EXPECT(c.lo == 0xFF000000u && c.hi == (0xFF000000u | 16u << 8 | 16u));  // pixels (0..1, 0..1)
    const taa::Range m = taa::neighbourhood(p.colour.data(), 3, 2, p.W, p.H);
    EXPECT(m.lo == (0xFF000000u | 32u << 8 | 16u) && m.hi == (0xFF000000u | 64u << 8 | 48u));
    // the id window: only the far corner of the 3 x 3 shows the id
    std::fill(p.prev_ids.begin(), p.prev_ids.end(), 5u);
    p.prev_ids[p.at(4, 3)] = 9;
    EXPECT(taa::id_nearby(p.prev_ids.data(), (uint32_t)p.at(3, 2), 9, p.W, p.H));
    EXPECT(!taa::id_nearby(p.prev_ids.data(), (uint32_t)p.at(2, 2), 9, p.W, p.H));
    EXPECT(taa::id_nearby(p.prev_ids.data(), (uint32_t)p.at(7, 3), 5, p.W, p.H));
    identity(R);
    EXPECT(run(p, R, 2, 2, 9).mask == taa::kId);
    EXPECT((run(p, R, 2, 2, 9, 0.1f, false).mask & 15u) == 0);  // without the flag no id is looked at
    EXPECT((run(p, R, 3, 2, 9).mask & 15u) == 0);
}

// One pixel of a 1 x 1 frame stepped n times: the colour c over a history that starts at `start`.
uint32_t step(uint32_t start16, uint32_t c8, float alpha, int n, uint32_t* out8 = nullptr, uint32_t* mask = nullptr) {
    Planes p(1, 1);
    float R[16];
    identity(R);
    p.colour[0] = grey(c8);
    p.prev_acc[0] = grey16(start16);
    taa::Pixel o{};
    for (int k = 0; k < n; ++k) {
        o = run(p, R, 0, 0, 1, alpha);
        p.prev_acc[0] = o.acc;
    }
    if (out8) *out8 = o.resolved;
    if (mask) *mask = o.mask;
    EXPECT(o.acc.bg == o.acc.ra && (o.acc.bg & 0xFFFFu) == o.acc.bg >> 16);  // all four channels follow one rule
    return o.acc.bg & 0xFFFFu;
}

void accumulation() {
    // alpha = 1: the current frame, whatever the history held (a 1 x 1 frame's range is the pixel: the history is clamped)
    uint32_t out8 = 0, mask = 0;
    EXPECT(step(12345, 200, 1.0f, 1, &out8, &mask) == 200u * 257u && out8 == grey(200) && mask == taa::kClamped);
    // ... and in a frame with a wide range, where nothing is clamped
    {
        Planes p(3, 3);
        float R[16];
        identity(R);
        for (uint32_t k = 0; k < 9; ++k) p.colour[k] = grey(k * 30u);
        p.prev_acc[4] = grey16(100u * 257u + 77u);
        const taa::Pixel o = run(p, R, 1, 1, 1, 1.0f);
        EXPECT(o.mask == 0 && o.resolved == p.colour[4] && o.acc.bg == taa::restart(p.colour[4], 0).acc.bg);
        const taa::Pixel h = run(p, R, 1, 1, 1, 0.5f);  // half of each, by hand: (25777 + 30840) / 2 = 28308.5 -> 28309
        EXPECT(h.mask == 0 && (h.acc.bg & 0xFFFFu) == 28309u && (h.resolved & 0xFFu) == 110u);
    }
    // a flat pixel stays exactly c * 257 over 100 steps, for every c
    for (uint32_t c = 0; c < 256; ++c) {
        EXPECT(step(c * 257u, c, 0.1f, 100, &out8, &mask) == c * 257u);
        EXPECT(out8 == grey(c) && mask == 0);
    }
    // a 0 -> 255 step: the 16-bit history gets within 4 steps of 65535 (an 8-bit one stalls at 251)
    {
        Planes p(3, 1);
        float R[16];
        identity(R);
        p.colour = {grey(0), grey(255), grey(255)};  // the range round the middle pixel is 0 .. 255: nothing is clamped
        p.prev_acc[1] = grey16(0);
        uint32_t s = 0, n = 0;
        for (; n < 200 && s < 65531u; ++n) {
            const taa::Pixel o = run(p, R, 1, 0, 1, 0.1f);
            EXPECT(o.mask == 0);
            EXPECT((o.acc.bg & 0xFFFFu) > s);  // it never stalls on the way
            s = o.acc.bg & 0xFFFFu;
            p.prev_acc[1] = o.acc;
        }
        EXPECT(s >= 65531u && n < 200);
        const taa::Pixel o = run(p, R, 1, 0, 1, 0.1f);
        EXPECT((o.resolved & 0xFFu) == 255u);
    }
    // the clamp: history far above the neighbourhood comes down to hi, far below goes up to lo
    {
        Planes p(3, 1);
        float R[16];
        identity(R);
        p.colour = {grey(10), grey(20), grey(30)};
        p.prev_acc[1] = grey16(65535);
        taa::Pixel o = run(p, R, 1, 0, 1, 0.5f);  // hc = 30 * 257 = 7710; r = 3855 + 2570 = 6425 = 25 * 257
        EXPECT(o.mask == taa::kClamped && (o.acc.bg & 0xFFFFu) == 6425u && (o.resolved & 0xFFu) == 25u);
        p.prev_acc[1] = grey16(0);
        o = run(p, R, 1, 0, 1, 0.5f);  // hc = 2570; r = 1285 + 2570 = 3855 = 15 * 257
        EXPECT(o.mask == taa::kClamped && (o.acc.bg & 0xFFFFu) == 3855u && (o.resolved & 0xFFu) == 15u);
        p.prev_acc[1] = grey16(25u * 257u);
        EXPECT(run(p, R, 1, 0, 1, 0.5f).mask == 0);
    }
    // no history: 1, the current colour, and none of the (here: null) previous planes is read
    {
        Planes p(2, 2);
        float R[16];
        identity(R);
        const history::Frame f = history::make_frame(2, 2, 0.0f);
        const taa::Pixel o = taa::resolve_pixel(R, 1, 1, 1u, 0.5f, p.colour.data(), f, false, true, 0.1f, (const uint32_t*)nullptr,
                                                (const taa::Texel*)nullptr);
        EXPECT(o.mask == taa::kNoHistory && restarted(o, p.colour[3]));
    }
    // never above 65535 / 255
    EXPECT(step(65535, 255, 0.3f, 3, &out8) == 65535u && out8 == grey(255));
}

void jitter_sets_and_arguments() {
    taa::Msg m;
    float xy[2] = {9.0f, 9.0f};
    EXPECT(taa::jitter(5, 0, xy, m) == TRI_OK && xy[0] == 0.0f && xy[1] == 0.0f);
    EXPECT(taa::jitter(0, 8, xy, m) == TRI_OK && xy[0] == 0.0f && xy[1] == (float)(1.0 / 3.0 - 0.5));
    EXPECT(taa::jitter(1, 8, xy, m) == TRI_OK && xy[0] == -0.25f && xy[1] == (float)(2.0 / 3.0 - 0.5));
    EXPECT(taa::jitter(2, 8, xy, m) == TRI_OK && xy[0] == 0.25f && xy[1] == (float)(1.0 / 9.0 - 0.5));
    float again[2];
    EXPECT(taa::jitter(10, 8, again, m) == TRI_OK && again[0] == xy[0] && again[1] == xy[1]);  // index % period
    for (uint32_t period : {1u, 8u, 16u, 64u})
        for (uint32_t k = 0; k < 2 * period; ++k) {
            EXPECT(taa::jitter(k, period, xy, m) == TRI_OK);
            EXPECT(xy[0] >= -0.5f && xy[0] < 0.5f && xy[1] >= -0.5f && xy[1] < 0.5f);
        }
    EXPECT(taa::jitter(0xFFFFFFFFu, 64, xy, m) == TRI_OK);
    EXPECT(taa::jitter(0, 65, xy, m) == TRI_E_INVALID && m.text[0]);
    EXPECT(taa::jitter(0, 8, nullptr, m) == TRI_E_INVALID);
    // the jittered projection: rows 0 and 1 gain a multiple of row 3, rows 2 and 3 are copied bitwise
    float P[16], J[16];
    for (int i = 0; i < 16; ++i) P[i] = 0.25f * (float)(i + 1);
    EXPECT(taa::jitter_projection(P, 0.25f, -0.5f, 8, 4, J, m) == TRI_OK);
    for (int c = 0; c < 4; ++c) {
        EXPECT(J[4 * c + 0] == P[4 * c + 0] + 0.0625f * P[4 * c + 3]);  // (2 * 0.25 / 8, exact in binary)
        EXPECT(J[4 * c + 1] == P[4 * c + 1] - 0.25f * P[4 * c + 3]);
        EXPECT(std::memcmp(&J[4 * c + 2], &P[4 * c + 2], 8) == 0);
    }
    EXPECT(taa::jitter_projection(P, 0.0f, 0.0f, 8, 4, J, m) == TRI_OK && std::memcmp(J, P, sizeof P) == 0);
    EXPECT(taa::jitter_projection(P, 0.25f, -0.5f, 8, 4, P, m) == TRI_OK);  // in place
    EXPECT(taa::jitter_projection(nullptr, 0, 0, 8, 4, J, m) == TRI_E_INVALID);
    EXPECT(taa::jitter_projection(P, 0, 0, 8, 4, nullptr, m) == TRI_E_INVALID);
    EXPECT(taa::jitter_projection(P, 0, 0, 0, 4, J, m) == TRI_E_INVALID);
    EXPECT(taa::jitter_projection(P, 0, 0, 8, 0, J, m) == TRI_E_INVALID);

    // the set sequence: plain, redo, reset, redo first
    history::Sets s;
    bool valid = true;
    uint32_t r = s.begin(false, &valid);
    EXPECT(r == 0 && !valid);
    r = s.begin(false, &valid);
    EXPECT(r == 1 && valid);
    r = s.begin(true, &valid);
    EXPECT(r == 1 && valid);
    r = s.begin(false, &valid);
    EXPECT(r == 0 && valid);
    s.reset();
    r = s.begin(true, &valid);
    EXPECT(!valid);
    const uint32_t first = r;
    r = s.begin(true, &valid);
    EXPECT(r == first && !valid);
    r = s.begin(false, &valid);
    EXPECT(r == (first ^ 1u) && valid);
    history::Sets fresh;
    r = fresh.begin(true, &valid);
    EXPECT(r == 0 && !valid);

    // every argument rule
    EXPECT(history::check_extent(0, 4, m) == TRI_E_INVALID && history::check_extent(4, 0, m) == TRI_E_INVALID);
    EXPECT(history::check_extent(1, 1, m) == TRI_OK && history::check_extent(65536, 32768, m) == TRI_OK);
    EXPECT(history::check_extent(65536, 32769, m) == TRI_E_INVALID);
    EXPECT(history::check_context(0, 8, 4, 0, 8, 4, m) == TRI_OK);
    EXPECT(history::check_context(0, 8, 4, 1, 8, 4, m) == TRI_E_INVALID);
    EXPECT(history::check_context(0, 8, 4, 0, 4, 8, m) == TRI_E_INVALID);
    tri_taa_params q{};
    EXPECT(taa::check_params(nullptr, m) == TRI_E_INVALID);
    EXPECT(taa::check_params(&q, m) == TRI_E_INVALID);  // an alpha of 0
    for (float ok : {1.0f, 0.1f, 1e-30f}) {
        q.alpha = ok;
        for (uint32_t flags : {0u, 1u, 2u, 3u}) {
            q.flags = flags;
            EXPECT(taa::check_params(&q, m) == TRI_OK);
        }
    }
    q.flags = 0;
    for (float bad : {0.0f, -0.0f, -0.1f, 1.0000001f, 2.0f, kNaN, kInf, -kInf}) {
        q.alpha = bad;
        EXPECT(taa::check_params(&q, m) == TRI_E_INVALID);
    }
    q.alpha = 0.1f;
    for (uint32_t flags : {4u, 7u, 0x80000000u}) {
        q.flags = flags;
        EXPECT(taa::check_params(&q, m) == TRI_E_INVALID);
    }
}

}  // namespace

int main() {
    wild_positions();
    borders();
    accumulation();
    jitter_sets_and_arguments();
    if (g_failures) {
        std::fprintf(stderr, "taa_check: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("taa_check: ok\n");
    return 0;
}
