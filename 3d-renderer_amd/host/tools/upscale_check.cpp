// upscale_check — host-only check of temporal upscaling's plain-C++ part (csrc/upscale_math.h), built under the address
// and undefined-behaviour sanitizers (make upscale-check). No device. The per-pixel rule here is the very pair of functions
// k_upscale_resolve compiles (upscale::sample, upscale::resolve_pixel); the render planes are heap arrays of exactly
// Wr x Hr elements and the history one of exactly Wo x Ho, so an index outside either frame is an error the address
// sanitizer reports. Groups:
//   1. rows that send the previous position anywhere: NaN, +-infinity, huge and negative u and v, q_3 <= 0 and NaN;
//   2. outputs of 1 x 1 from 1 x 1, 3 x 200 from 1 x 100, 200 x 3 from 100 x 1 and 64 x 48 from 43 x 32, every pixel, under
//      shifts that put both windows and the taps on every border and corner;
//   3. the jitter at -0.5 and at the largest float below 0.5 (xr, yr stay inside), the weight k by hand;
//   4. the accumulation: alpha = 1, a flat frame over 100 steps at 2 x for every colour, a sample of weight 0;
//   5. the jitter period; the set bookkeeping (plain calls, a redo, a reset, a redo first); the argument rules.
#include "../../csrc/upscale_math.h"

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

// The current frame and the previous ids at the render extent, the stored history at the output extent: each plane of
// exactly that many elements.
struct Planes {
    upscale::Scale s;
    history::Frame f;
    std::vector<uint32_t> colour, ids, prev_ids;
    std::vector<float> depth;
    std::vector<taa::Texel> prev_acc;
    Planes(uint32_t wr, uint32_t hr, uint32_t wo, uint32_t ho)
        : s(upscale::make_scale(wr, hr, wo, ho)), f(history::make_frame(wo, ho, 0.0f)), colour((size_t)wr * hr),
          ids((size_t)wr * hr, 1u), prev_ids((size_t)wr * hr, 1u), depth((size_t)wr * hr, 0.5f), prev_acc((size_t)wo * ho) {
        for (uint32_t y = 0; y < hr; ++y)
            for (uint32_t x = 0; x < wr; ++x)
                colour[(size_t)y * wr + x] = 0xFF000000u | ((x * 16u) & 0xFFu) << 8 | ((y * 16u) & 0xFFu);
        for (uint32_t y = 0; y < ho; ++y)
            for (uint32_t x = 0; x < wo; ++x)
                prev_acc[(size_t)y * wo + x] = taa::restart(0xFF000000u | ((x * 8u) & 0xFFu) << 8 | ((y * 8u) & 0xFFu), 0).acc;
    }
    size_t rat(uint32_t x, uint32_t y) const { return (size_t)y * s.Wr + x; }
    size_t oat(uint32_t x, uint32_t y) const { return (size_t)y * s.Wo + x; }
};

struct Out {
    taa::Pixel o;
    upscale::Sample sm;
    uint32_t c;  // the colour of the render pixel the sample names
};

// The kernel's sequence: the sample, the id and depth at it, the row, the rule. `id` overrides the frame's id (0: keep).
Out run(const Planes& p, const float* R, uint32_t X, uint32_t Y, float jx = 0.0f, float jy = 0.0f, float alpha = 0.1f,
        bool reject = true, bool has_prev = true, uint32_t id = 0) {
    const upscale::Sample sm = upscale::sample(X, Y, p.s, jx, jy);
    EXPECT(sm.xr < p.s.Wr && sm.yr < p.s.Hr);
    EXPECT(sm.k >= 0.0f && sm.k <= 1.0f);
    if (!(sm.xr < p.s.Wr && sm.yr < p.s.Hr)) std::exit(1);
    const size_t q = p.rat(sm.xr, sm.yr);
    const taa::Pixel o = upscale::resolve_pixel(R, X, Y, sm, id ? id : p.ids[q], p.depth[q], p.colour.data(), p.s, p.f, has_prev,
                                                reject, alpha, has_prev ? p.prev_ids.data() : nullptr,
                                                has_prev ? p.prev_acc.data() : nullptr);
    return Out{o, sm, p.colour[q]};
}

bool restarted(const Out& r) {
    const taa::Pixel w = taa::restart(r.c, r.o.mask);
    return r.o.resolved == r.c && r.o.acc.bg == w.acc.bg && r.o.acc.ra == w.acc.ra;
}

const float kNaN = std::numeric_limits<float>::quiet_NaN();
const float kInf = std::numeric_limits<float>::infinity();
const float kBelowHalf = std::nextafterf(0.5f, 0.0f);
const uint32_t kKnown = upscale::kNoProj | upscale::kOutside | upscale::kId | upscale::kClamped | upscale::kNoSample;

void wild_positions() {
    Planes p(7, 5, 14, 10);
    float R[16];
    const float wild[] = {1e30f, -1e30f, 3.0e38f, -3.0e38f, 1e9f, -1e9f, -1.0f, 14.0f, 1e-30f};
    for (float a : wild)
        for (float b : wild)
            for (uint32_t Y = 0; Y < p.s.Ho; ++Y)
                for (uint32_t X = 0; X < p.s.Wo; ++X) {
                    shift_row(R, p.s.Wo, p.s.Ho, a, b);
                    const Out r = run(p, R, X, Y, 0.25f, -0.25f);
                    EXPECT((r.o.mask & ~(upscale::kClamped | upscale::kNoSample)) == 0 || r.o.mask == upscale::kOutside ||
                           r.o.mask == upscale::kNoProj);
                    EXPECT((r.o.mask & 15u) == 0 || restarted(r));
                }
    for (float bad : {kNaN, kInf, -kInf})
        for (int at : {0, 3, 5, 7, 2, 6}) {
            identity(R);
            R[at] = bad;
            for (uint32_t X = 0; X < p.s.Wo; ++X) {
                const Out r = run(p, R, X, 4);
                EXPECT(r.o.mask == upscale::kNoProj || (r.o.mask & 15u) == 0);
                EXPECT((r.o.mask & 15u) == 0 || restarted(r));
            }
        }
    identity(R);
    R[3] = kNaN;
    EXPECT(run(p, R, 3, 2).o.mask == upscale::kNoProj);
    for (float q3 : {0.0f, -0.0f, -1.0f, kNaN, -kInf, 1e-45f}) {  // q_3 <= 0, NaN, and so small that 1 / q_3 overflows
        identity(R);
        R[15] = q3;
        const Out r = run(p, R, 3, 2);
        EXPECT(r.o.mask == upscale::kNoProj && restarted(r));
    }
    // the borders of the OUTPUT frame decide OUTSIDE, not the render frame's
    shift_row(R, 14, 10, 0.5f, 0.0f);
    EXPECT(run(p, R, 13, 0).o.mask == upscale::kOutside);  // u = 13.5 + 0.5 = 14 = Wo
    EXPECT((run(p, R, 7, 0).o.mask & 15u) == 0);           // u = 8 > Wr, inside the output
    shift_row(R, 14, 10, 0.0f, -1.0f);
    EXPECT(run(p, R, 0, 0).o.mask == upscale::kOutside);  // v = -0.5
}

// Every output pixel of small, thin and non-integer-ratio frames, still and under shifts and jitters that put the taps and
// both windows on every border.
void borders() {
    const uint32_t extents[][4] = {{1, 1, 1, 1}, {1, 100, 3, 200}, {100, 1, 200, 3}, {43, 32, 64, 48}, {1, 1, 3, 3}, {2, 2, 4, 4}};
    float R[16];
    for (const auto& e : extents) {
        Planes p(e[0], e[1], e[2], e[3]);
        for (size_t k = 0; k < p.prev_ids.size(); k += 3) p.prev_ids[k] = 2;  // a third of the previous ids are another draw's
        for (size_t k = 0; k < p.ids.size(); k += 5) p.ids[k] = 2;
        const float js[] = {0.0f, -0.5f, kBelowHalf, 0.25f};
        for (float dx : {0.0f, -0.49f, 0.49f, 1.0f, -1.0f, 2.5f})
            for (float dy : {0.0f, -0.49f, 0.49f, 1.0f, -1.0f})
                for (float jx : js)
                    for (float jy : js) {
                        if ((size_t)e[2] * e[3] > 1000 && jx != jy && dx != dy) continue;  // (the large case: a diagonal)
                        shift_row(R, p.s.Wo, p.s.Ho, dx, dy);
                        for (uint32_t Y = 0; Y < p.s.Ho; ++Y)
                            for (uint32_t X = 0; X < p.s.Wo; ++X)
                                for (uint32_t id : {0u, 3u}) {
                                    const Out r = run(p, R, X, Y, jx, jy, 0.1f, true, true, id);
                                    EXPECT((r.o.mask & ~kKnown) == 0);
                                    if (id == 3) EXPECT((r.o.mask & 15u) != 0);  // no previous pixel shows id 3
                                    if (r.o.mask & 15u) EXPECT(restarted(r) && !(r.o.mask & (upscale::kClamped | upscale::kNoSample)));
                                    else EXPECT(((r.o.mask & upscale::kNoSample) != 0) == (r.sm.k == 0.0f));
                                }
                    }
    }
    // the id window is looked up at the render extent: output pixel (6, 4) of 8 x 6 from 4 x 3 lies in render pixel (3, 2)
    Planes p(4, 3, 8, 6);
    identity(R);
    std::fill(p.prev_ids.begin(), p.prev_ids.end(), 5u);
    EXPECT(upscale::render_index((uint32_t)p.oat(6, 4), p.s) == p.rat(3, 2));
    EXPECT(upscale::render_index((uint32_t)p.oat(7, 5), p.s) == p.rat(3, 2));
    EXPECT(upscale::render_index((uint32_t)p.oat(0, 0), p.s) == p.rat(0, 0));
    EXPECT(upscale::render_index((uint32_t)p.oat(1, 1), p.s) == p.rat(0, 0));
    p.prev_ids[p.rat(3, 2)] = 9;
    EXPECT((run(p, R, 4, 2, 0, 0, 0.1f, true, true, 9).o.mask & 15u) == 0);          // render (2, 1): (3, 2) is a neighbour
    EXPECT(run(p, R, 3, 2, 0, 0, 0.1f, true, true, 9).o.mask == upscale::kId);       // render (1, 1): it is not
    EXPECT((run(p, R, 3, 2, 0, 0, 0.1f, false, true, 9).o.mask & 15u) == 0);         // without the flag no id is looked at
}

// The sample and its weight by hand.
void samples() {
    const upscale::Scale s2 = upscale::make_scale(32, 24, 64, 48);
    EXPECT(s2.rx == 0.5f && s2.ox == 2.0f);
    // no jitter at 2 x: output 10 -> px = 5.25 -> render 5, whose centre 5.5 lies at output 11.0: dx = 0.5
    upscale::Sample sm = upscale::sample(10, 11, s2, 0.0f, 0.0f);
    EXPECT(sm.xr == 5 && sm.yr == 5 && sm.k == 0.25f);  // (dy = 11.0 - 11.5 = -0.5)
    // a jitter of +0.25: render 5's sample lies at 5.25, output 10.5 = the centre of output pixel 10: k = 1 along x
    sm = upscale::sample(10, 10, s2, 0.25f, 0.25f);
    EXPECT(sm.xr == 5 && sm.yr == 5 && sm.k == 1.0f);
    sm = upscale::sample(11, 11, s2, 0.25f, 0.25f);  // px = 5.75 + 0.25 = 6: render 6, sample 6.25 -> 12.5: dx = 1: k = 0
    EXPECT(sm.xr == 6 && sm.yr == 6 && sm.k == 0.0f);
    // the extreme jitters keep xr, yr inside on every pixel of every extent
    const uint32_t extents[][4] = {{1, 1, 1, 1}, {1, 1, 3, 3}, {1, 100, 3, 200}, {100, 1, 200, 3}, {43, 32, 64, 48}, {37, 23, 101, 69}};
    for (const auto& e : extents) {
        const upscale::Scale s = upscale::make_scale(e[0], e[1], e[2], e[3]);
        for (float j : {-0.5f, kBelowHalf, 0.0f})
            for (uint32_t Y = 0; Y < s.Ho; ++Y)
                for (uint32_t X = 0; X < s.Wo; ++X) {
                    sm = upscale::sample(X, Y, s, j, j);
                    EXPECT(sm.xr < s.Wr && sm.yr < s.Hr && sm.k >= 0.0f && sm.k <= 1.0f);
                }
    }
    // at a scale of 1 the weight is (1 - |jx|)(1 - |jy|): not tri_taa's rule
    const upscale::Scale s1 = upscale::make_scale(8, 8, 8, 8);
    sm = upscale::sample(3, 4, s1, 0.25f, -0.5f);
    EXPECT(sm.xr == 3 && sm.yr == 4 && sm.k == 0.75f * 0.5f);
}

void accumulation() {
    float R[16];
    identity(R);
    // alpha = 1 with a sample on the centre: the current frame whatever the history held; nothing clamped in a wide range
    {
        Planes p(3, 3, 6, 6);
        for (uint32_t k = 0; k < 9; ++k) p.colour[k] = grey(k * 30u);
        p.prev_acc[p.oat(2, 2)] = grey16(100u * 257u + 77u);
        Out r = run(p, R, 2, 2, 0.25f, 0.25f, 1.0f);  // render (1, 1), k = 1
        EXPECT(r.sm.xr == 1 && r.sm.yr == 1 && r.sm.k == 1.0f);
        EXPECT(r.o.mask == 0 && r.o.resolved == p.colour[4] && r.o.acc.bg == taa::restart(p.colour[4], 0).acc.bg);
        r = run(p, R, 2, 2, 0.25f, 0.25f, 0.5f);  // half of each, by hand: (25777 + 30840) / 2 = 28308.5 -> 28309
        EXPECT(r.o.mask == 0 && (r.o.acc.bg & 0xFFFFu) == 28309u && (r.o.resolved & 0xFFu) == 110u);
        // k == 0: a valid pixel's history is left as it was (inside the range: no clamp), and the bit says so
        p.prev_acc[p.oat(3, 3)] = grey16(200u * 257u + 5u);
        r = run(p, R, 3, 3, 0.25f, 0.25f, 0.5f);  // render (2, 2), sample at output 4.5: dx = 1
        EXPECT(r.sm.xr == 2 && r.sm.yr == 2 && r.sm.k == 0.0f && r.o.mask == upscale::kNoSample);
        EXPECT(r.o.acc.bg == p.prev_acc[p.oat(3, 3)].bg && r.o.acc.ra == p.prev_acc[p.oat(3, 3)].ra);
        // ... apart from the clamp: history above the window's range comes down to hi
        p.prev_acc[p.oat(3, 3)] = grey16(65535);
        r = run(p, R, 3, 3, 0.25f, 0.25f, 0.5f);  // the window round render (2, 2) is 120 .. 240, alpha irrelevant
        EXPECT(r.o.mask == (upscale::kNoSample | upscale::kClamped) && (r.o.acc.bg & 0xFFFFu) == 240u * 257u);
        // an invalid pixel takes the nearest sample whatever k is
        r = run(p, R, 3, 3, 0.25f, 0.25f, 0.5f, true, true, 7);
        EXPECT(r.o.mask == upscale::kId && restarted(r));
    }
    // a flat frame stays exactly c * 257 over 100 steps at 2 x, for every c, under the period's jitters
    for (uint32_t c = 0; c < 256; ++c) {
        Planes p(2, 2, 4, 4);
        std::fill(p.colour.begin(), p.colour.end(), grey(c));
        std::fill(p.prev_acc.begin(), p.prev_acc.end(), grey16(c * 257u));
        std::vector<taa::Texel> next(p.prev_acc.size());
        bool exact = true;
        for (int n = 0; n < 100; ++n) {
            float xy[2];
            taa::Msg m;
            EXPECT(taa::jitter((uint32_t)n, 32, xy, m) == TRI_OK);
            for (uint32_t Y = 0; Y < 4; ++Y)
                for (uint32_t X = 0; X < 4; ++X) {
                    const Out r = run(p, R, X, Y, xy[0], xy[1], 0.1f);
                    exact &= (r.o.mask & ~upscale::kNoSample) == 0 && r.o.resolved == grey(c) && r.o.acc.bg == grey16(c * 257u).bg &&
                             r.o.acc.ra == grey16(c * 257u).ra;
                    next[p.oat(X, Y)] = r.o.acc;
                }
            p.prev_acc = next;
        }
        EXPECT(exact);
    }
    // no history: 1, the nearest sample, and none of the (here: null) previous planes is read
    {
        Planes p(2, 2, 4, 4);
        const Out r = run(p, R, 3, 3, -0.5f, kBelowHalf, 0.1f, true, false);
        EXPECT(r.o.mask == upscale::kNoHistory && restarted(r));
    }
}

void period_sets_and_arguments() {
    upscale::Msg m;
    uint32_t n = 99;
    EXPECT(upscale::jitter_period(32, 24, 32, 24, &n, m) == TRI_OK && n == 8);
    EXPECT(upscale::jitter_period(32, 24, 48, 36, &n, m) == TRI_OK && n == 18);
    EXPECT(upscale::jitter_period(32, 24, 64, 48, &n, m) == TRI_OK && n == 32);
    EXPECT(upscale::jitter_period(32, 24, 96, 72, &n, m) == TRI_OK && n == 64);
    EXPECT(upscale::jitter_period(43, 32, 64, 48, &n, m) == TRI_OK && n == 18);  // 8 * 1.488 * 1.5 = 17.86
    EXPECT(upscale::jitter_period(32, 24, 64, 24, &n, m) == TRI_OK && n == 16);
    EXPECT(upscale::jitter_period(32, 24, 64, 48, nullptr, m) == TRI_E_INVALID);
    EXPECT(upscale::jitter_period(32, 24, 97, 72, &n, m) == TRI_E_INVALID && n == 0 && m.text[0]);

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
    EXPECT(upscale::check_extents(1, 1, 1, 1, m) == TRI_OK && upscale::check_extents(1, 1, 3, 3, m) == TRI_OK);
    EXPECT(upscale::check_extents(43, 32, 64, 48, m) == TRI_OK && upscale::check_extents(1920, 1080, 3840, 2160, m) == TRI_OK);
    EXPECT(upscale::check_extents(0, 4, 4, 4, m) == TRI_E_INVALID && upscale::check_extents(4, 0, 4, 4, m) == TRI_E_INVALID);
    EXPECT(upscale::check_extents(4, 4, 0, 4, m) == TRI_E_INVALID && upscale::check_extents(4, 4, 4, 0, m) == TRI_E_INVALID);
    EXPECT(upscale::check_extents(4, 4, 3, 4, m) == TRI_E_INVALID && upscale::check_extents(4, 4, 4, 3, m) == TRI_E_INVALID);
    EXPECT(upscale::check_extents(4, 4, 13, 4, m) == TRI_E_INVALID && upscale::check_extents(4, 4, 4, 13, m) == TRI_E_INVALID);
    EXPECT(upscale::check_extents(4, 4, 12, 12, m) == TRI_OK);
    EXPECT(upscale::check_extents(65536, 32768, 65536, 32768, m) == TRI_OK);
    EXPECT(upscale::check_extents(65536, 32768, 65536, 32769, m) == TRI_E_INVALID);          // more than 2^31 output pixels
    EXPECT(upscale::check_extents(0x80000000u, 1, 0xFFFFFFFFu, 1, m) == TRI_E_INVALID);
    EXPECT(upscale::check_extents(0x80000000u, 1, 0x80000000u, 1, m) == TRI_E_INVALID);  // a side above 2^30
    EXPECT(upscale::check_extents(1, 0x80000000u, 1, 0x80000000u, m) == TRI_E_INVALID);
    EXPECT(upscale::check_extents(0x40000001u, 1, 0x40000001u, 1, m) == TRI_E_INVALID);
    EXPECT(upscale::check_extents(0x20000000u, 1, 0x40000001u, 1, m) == TRI_E_INVALID);
    EXPECT(upscale::check_extents(0x40000000u, 1, 0x40000000u, 1, m) == TRI_OK);
    {   // ... and the widest extent the rule admits: the sample and the render index of its last pixels, no overflow
        const upscale::Scale w = upscale::make_scale(0x40000000u, 1, 0x40000000u, 1);
        for (uint32_t X : {0u, 1u, 0x1FFFFFFFu, 0x3FFFFF00u, 0x3FFFFFFFu})
            for (float j : {-0.5f, kBelowHalf}) {
                const upscale::Sample sm = upscale::sample(X, 0, w, j, j);
                EXPECT(sm.xr < w.Wr && sm.yr == 0);
                EXPECT(upscale::render_index(X, w) < w.Wr);
            }
    }
    EXPECT(upscale::check_extents(0x60000000u, 1, 0x20000000u, 1, m) == TRI_E_INVALID);      // 3 Wr wraps in 32 bits
    tri_upscale_params q{};
    EXPECT(upscale::check_params(nullptr, m) == TRI_E_INVALID);
    EXPECT(upscale::check_params(&q, m) == TRI_E_INVALID);  // an alpha of 0
    for (float ok : {1.0f, 0.1f, 1e-30f}) {
        q.alpha = ok;
        for (uint32_t flags : {0u, 1u, 2u, 3u}) {
            q.flags = flags;
            EXPECT(upscale::check_params(&q, m) == TRI_OK);
        }
    }
    q.flags = 0;
    for (float bad : {0.0f, -0.0f, -0.1f, 1.0000001f, 2.0f, kNaN, kInf, -kInf}) {
        q.alpha = bad;
        EXPECT(upscale::check_params(&q, m) == TRI_E_INVALID);
    }
    q.alpha = 0.1f;
    for (int k = 0; k < 2; ++k) {
        for (float ok : {-0.5f, 0.5f, kBelowHalf, 0.0f, -0.0f}) {
            q.jitter[k] = ok;
            EXPECT(upscale::check_params(&q, m) == TRI_OK);
        }
        for (float bad : {std::nextafterf(0.5f, 1.0f), -std::nextafterf(0.5f, 1.0f), 1.0f, kNaN, kInf, -kInf}) {
            q.jitter[k] = bad;
            EXPECT(upscale::check_params(&q, m) == TRI_E_INVALID);
        }
        q.jitter[k] = 0.0f;
    }
    for (uint32_t flags : {4u, 7u, 0x80000000u}) {
        q.flags = flags;
        EXPECT(upscale::check_params(&q, m) == TRI_E_INVALID);
    }
}

}  // namespace

int main() {
    wild_positions();
    borders();
    samples();
    accumulation();
    period_sets_and_arguments();
    if (g_failures) {
        std::fprintf(stderr, "upscale_check: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("upscale_check: ok\n");
    return 0;
}
