// history_check — host-only check of the history reprojection pass's plain-C++ part (csrc/history_math.h), built under
// the address and undefined-behaviour sanitizers (make history-check). No device. The per-pixel rule here is the very
// function k_reproject compiles; every previous plane is a heap array of exactly W x H elements, so an index outside the
// frame is an error the address sanitizer reports. Groups:
//   1. rows that send the previous position anywhere: NaN, +-infinity, huge and negative u and v, q_3 <= 0 and NaN;
//   2. a 1 x 1 frame; taps at all four borders and in the corners (the clamp), a half-pixel shift's blend by hand;
//   3. ids: a mismatch, the background, the id at the table's end; depth: a tolerance of 0, inside and outside it, NaN;
//   4. no history; the set bookkeeping (plain calls, a redo, a reset, a redo first); the argument rules.
#include "../../csrc/history_math.h"

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

struct Planes {
    uint32_t W, H;
    std::vector<uint32_t> ids, colour;
    std::vector<float> depth;
    Planes(uint32_t w, uint32_t h) : W(w), H(h), ids((size_t)w * h, 1u), colour((size_t)w * h), depth((size_t)w * h, 0.5f) {
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) colour[(size_t)y * w + x] = 0xFF000000u | ((x * 16u) & 0xFFu) << 8 | ((y * 16u) & 0xFFu);
    }
};

history::Pixel run(const Planes& p, const float* R, uint32_t x, uint32_t y, uint32_t id, float depth, float tol = 0.0f,
                   bool has_prev = true) {
    const history::Frame f = history::make_frame(p.W, p.H, tol);
    return history::reproject_pixel(R, x, y, id, depth, 0x11223344u, f, has_prev, p.ids.data(), p.depth.data(), p.colour.data());
}

const float kNaN = std::numeric_limits<float>::quiet_NaN();
const float kInf = std::numeric_limits<float>::infinity();

void wild_positions() {
    Planes p(7, 5);
    float R[16];
    // every pixel under rows that throw it far out, to infinity, or nowhere
    const float wild[] = {1e30f, -1e30f, 3.0e38f, -3.0e38f, 1e9f, -1e9f, -1.0f, 7.0f, 1e-30f};
    for (float a : wild)
        for (float b : wild)
            for (uint32_t y = 0; y < p.H; ++y)
                for (uint32_t x = 0; x < p.W; ++x) {
                    shift_row(R, p.W, p.H, a, b);
                    const history::Pixel o = run(p, R, x, y, 1, 0.5f);
                    EXPECT(o.mask == 0 || o.mask == history::kOutside || o.mask == history::kNoProj);
                    EXPECT(o.mask == 0 || o.colour == 0x11223344u);
                }
    // a non-finite motion vector: an infinite or NaN entry in the row
    for (float bad : {kNaN, kInf, -kInf})
        for (int at : {0, 3, 5, 7, 2, 6}) {
            identity(R);
            R[at] = bad;
            for (uint32_t x = 0; x < p.W; ++x) {
                const history::Pixel o = run(p, R, x, 2, 1, 0.5f);
                EXPECT(o.mask == history::kNoProj || o.mask == 0);  // (an infinite entry times a zero coordinate may be NaN or not hit)
                EXPECT(o.mask == 0 || o.colour == 0x11223344u);
            }
        }
    identity(R);
    R[3] = kNaN;
    EXPECT(run(p, R, 3, 2, 1, 0.5f).mask == history::kNoProj);
    // q_3 <= 0, NaN, and so small that 1 / q_3 overflows
    for (float q3 : {0.0f, -0.0f, -1.0f, kNaN, -kInf, 1e-45f}) {
        identity(R);
        R[15] = q3;
        const history::Pixel o = run(p, R, 3, 2, 1, 0.5f);
        EXPECT(o.mask == history::kNoProj);
        EXPECT(o.colour == 0x11223344u);
    }
    // exactly on the frame's edges: u = 0 is inside, u = W is not
    shift_row(R, 8, 4, -0.5f, 0.0f);
    Planes q(8, 4);
    EXPECT(run(q, R, 0, 0, 1, 0.5f).mask == 0);  // u = 0.5 - 0.5 = 0
    shift_row(R, 8, 4, 0.5f, 0.0f);
    EXPECT(run(q, R, 7, 0, 1, 0.5f).mask == history::kOutside);  // u = 7.5 + 0.5 = 8 = W
    shift_row(R, 8, 4, 0.0f, -1.0f);
    EXPECT(run(q, R, 0, 0, 1, 0.5f).mask == history::kOutside);  // v = -0.5
}

void borders_and_blend() {
    float R[16];
    identity(R);
    {  // a 1 x 1 frame: every tap is the one pixel
        Planes p(1, 1);
        const history::Pixel o = run(p, R, 0, 0, 1, 0.5f);
        EXPECT(o.mask == 0 && o.colour == p.colour[0]);
        shift_row(R, 1, 1, 0.25f, -0.25f);
        const history::Pixel s = run(p, R, 0, 0, 1, 0.5f);
        EXPECT(s.mask == 0 && s.colour == p.colour[0]);
        shift_row(R, 1, 1, 1.0f, 0.0f);
        EXPECT(run(p, R, 0, 0, 1, 0.5f).mask == history::kOutside);
    }
    Planes p(8, 4);
    identity(R);
    for (uint32_t y = 0; y < p.H; ++y)  // still: the previous pixel itself, every border and corner included
        for (uint32_t x = 0; x < p.W; ++x) {
            const history::Pixel o = run(p, R, x, y, 1, 0.5f);
            EXPECT(o.mask == 0 && o.colour == p.colour[(size_t)y * p.W + x]);
        }
    // a shift of up to just under half a pixel towards each border keeps the border pixels inside; their outer taps clamp
    for (float d : {0.49f, 0.25f})
        for (uint32_t y = 0; y < p.H; ++y)
            for (uint32_t x = 0; x < p.W; ++x) {
                const bool edge = x == 0 || y == 0 || x == p.W - 1 || y == p.H - 1;
                if (!edge) continue;
                const float dx = x == 0 ? -d : (x == p.W - 1 ? d : 0.0f), dy = y == 0 ? -d : (y == p.H - 1 ? d : 0.0f);
                shift_row(R, p.W, p.H, dx, dy);
                const history::Pixel o = run(p, R, x, y, 1, 0.5f);
                EXPECT(o.mask == 0 && o.colour == p.colour[(size_t)y * p.W + x]);  // (both clamped taps are the pixel itself)
            }
    // half a pixel to the right in the interior: the mean of two neighbours, rounded half up (power-of-two sizes: exact)
    shift_row(R, p.W, p.H, 0.5f, 0.0f);
    const history::Pixel h = run(p, R, 2, 1, 1, 0.5f);
    const uint32_t a = p.colour[(size_t)1 * p.W + 2], b = p.colour[(size_t)1 * p.W + 3];
    uint32_t want = 0;
    for (int sh = 0; sh < 32; sh += 8) {
        const float r = (float)((a >> sh) & 0xFF) * 0.5f + (float)((b >> sh) & 0xFF) * 0.5f;
        want |= (uint32_t)(int)(r + 0.5f) << sh;
    }
    EXPECT(h.mask == 0 && h.colour == want);
    EXPECT(history::blend(255, 255, 255, 255, 0, 0.3f, 0.7f) == 255u);  // never above 255
}

void ids_and_depth() {
    Planes p(8, 4);
    float R[16];
    identity(R);
    p.ids[(size_t)1 * p.W + 3] = 2;
    EXPECT(run(p, R, 3, 1, 1, 0.5f).mask == history::kId);
    EXPECT(run(p, R, 3, 1, 2, 0.5f).mask == 0);
    EXPECT(run(p, R, 3, 1, 0, 1.0f).mask == history::kId);  // the background now, a draw before
    p.ids[(size_t)1 * p.W + 3] = 0;
    EXPECT(run(p, R, 3, 1, 0, 1.0f, 1e-3f).mask == 0);  // background on background: no depth test
    // the id at the table's end: a table of 1025 rows, the last one a shift; the row is the caller's to pick
    std::vector<float> table((size_t)1025 * 16);
    for (uint32_t k = 0; k < 1025; ++k) identity(&table[(size_t)k * 16]);
    shift_row(&table[(size_t)1024 * 16], p.W, p.H, 1.0f, 0.0f);
    p.ids[(size_t)2 * p.W + 5] = 1024;
    EXPECT(run(p, &table[(size_t)1024 * 16], 4, 2, 1024, 0.5f).mask == 0);
    EXPECT(run(p, &table[(size_t)1023 * 16], 4, 2, 1024, 0.5f).mask == history::kId);
    // depth: identity row, zp = z. Stored 0.5
    EXPECT(run(p, R, 1, 1, 1, 0.75f, 0.0f).mask == 0);  // a tolerance of 0: no test
    EXPECT(run(p, R, 1, 1, 1, 0.75f, 0.1f).mask == history::kDepth);
    EXPECT(run(p, R, 1, 1, 1, 0.75f, 0.25f).mask == 0);  // |0.75 - 0.5| <= 0.25
    EXPECT(run(p, R, 1, 1, 1, 0.5f, 1e-30f).mask == 0);
    p.depth[(size_t)1 * p.W + 1] = kNaN;
    EXPECT(run(p, R, 1, 1, 1, 0.5f, 0.1f).mask == history::kDepth);  // NaN fails the comparison
    EXPECT(run(p, R, 1, 1, 1, 0.5f, 0.0f).mask == 0);
}

void sets_and_arguments() {
    Planes p(4, 4);
    float R[16];
    identity(R);
    // no history: 1, the current colour, and none of the (here: null) previous planes is read
    const history::Frame f = history::make_frame(4, 4, 0.0f);
    const history::Pixel o = history::reproject_pixel(R, 1, 1, 1u, 0.5f, 0xAABBCCDDu, f, false, (const uint32_t*)nullptr,
                                                      (const float*)nullptr, (const uint32_t*)nullptr);
    EXPECT(o.mask == history::kNoHistory && o.colour == 0xAABBCCDDu);

    history::Sets s;
    bool valid = true;
    uint32_t r = s.begin(false, &valid);
    EXPECT(r == 0 && !valid);  // first call: reads nothing, stores into set 1
    r = s.begin(false, &valid);
    EXPECT(r == 1 && valid);  // second: reads set 1, stores into 0
    r = s.begin(true, &valid);
    EXPECT(r == 1 && valid);  // a redo: the same again
    r = s.begin(false, &valid);
    EXPECT(r == 0 && valid);
    s.reset();
    r = s.begin(true, &valid);
    EXPECT(!valid);  // a redo after a reset is a plain first call
    const uint32_t first = r;
    r = s.begin(true, &valid);
    EXPECT(r == first && !valid);  // the redo of a first call has no history either
    r = s.begin(false, &valid);
    EXPECT(r == (first ^ 1u) && valid);
    history::Sets fresh;
    r = fresh.begin(true, &valid);
    EXPECT(r == 0 && !valid);

    history::Msg m;
    EXPECT(history::check_extent(0, 4, m) == TRI_E_INVALID && m.text[0]);
    EXPECT(history::check_extent(4, 0, m) == TRI_E_INVALID);
    EXPECT(history::check_extent(1, 1, m) == TRI_OK);
    EXPECT(history::check_extent(65536, 32768, m) == TRI_OK);  // 2^31 exactly
    EXPECT(history::check_extent(65536, 32769, m) == TRI_E_INVALID);
    EXPECT(history::check_extent(0xFFFFFFFFu, 0xFFFFFFFFu, m) == TRI_E_INVALID);
    tri_reproject_params q{};
    EXPECT(history::check_params(nullptr, m) == TRI_E_INVALID);
    EXPECT(history::check_params(&q, m) == TRI_OK);
    q.flags = TRI_HISTORY_REDO;
    q.depth_tolerance = 1e-3f;
    EXPECT(history::check_params(&q, m) == TRI_OK);
    q.flags = 2;
    EXPECT(history::check_params(&q, m) == TRI_E_INVALID);
    q.flags = 0;
    for (float bad : {-1.0f, -1e-30f, kNaN, kInf, -kInf}) {
        q.depth_tolerance = bad;
        EXPECT(history::check_params(&q, m) == TRI_E_INVALID);
    }
    q.depth_tolerance = -0.0f;
    EXPECT(history::check_params(&q, m) == TRI_OK);
    EXPECT(history::check_context(0, 8, 4, 0, 8, 4, m) == TRI_OK);
    EXPECT(history::check_context(0, 8, 4, 1, 8, 4, m) == TRI_E_INVALID);
    EXPECT(history::check_context(0, 8, 4, 0, 4, 8, m) == TRI_E_INVALID);
}

}  // namespace

int main() {
    wild_positions();
    borders_and_blend();
    ids_and_depth();
    sets_and_arguments();
    if (g_failures) {
        std::fprintf(stderr, "history_check: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("history_check: ok\n");
    return 0;
}
