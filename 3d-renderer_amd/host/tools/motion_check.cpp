// motion_check — host-only check of the motion pass's plain-C++ part (csrc/motion_math.h), built under the address and
// undefined-behaviour sanitizers (make motion-check). No device. Four groups:
//   1. the reprojection table: still frames (bitwise-equal matrices -> exact identities), no history, a draw count of 0,
//      a translated model against the product written out by hand, the background row without the views' translation;
//   2. matrices the table cannot invert or represent: singular models (a zero scale, two equal columns), NaN and
//      infinite matrices in the current and in the previous frame -> identity rows, never a non-finite entry;
//   3. the per-pixel rule on hand-made rows: the identity gives +0 exactly, a pixel translation comes back, q_3 <= 0, a
//      NaN row and an overflowing row give (0, 0);
//   4. the argument rules of tri_set_motion_history and tri_motion_matrices, the count-mismatch cases among them.
#include "../../csrc/motion_math.h"

#include <cstdlib>
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

tri_draw draw_at(float x, float y, float z, float s = 1.0f) {
    tri_draw d{};
    identity(d.pc.model);
    d.pc.model[0] = d.pc.model[5] = d.pc.model[10] = s;
    d.pc.model[12] = x; d.pc.model[13] = y; d.pc.model[14] = z;
    return d;
}

// a perspective projection (y flipped, depth 0..1) and a view translated by (-cx, -cy, -cz)
tri_global_ubo camera(float cx, float cy, float cz) {
    tri_global_ubo u{};
    const float f = 1.7320508f, aspect = 100.0f / 70.0f, n = 0.1f, fa = 60.0f;
    u.projection[0] = f / aspect;
    u.projection[5] = -f;
    u.projection[10] = fa / (n - fa);
    u.projection[11] = -1.0f;
    u.projection[14] = (n * fa) / (n - fa);
    identity(u.view);
    u.view[12] = -cx; u.view[13] = -cy; u.view[14] = -cz;
    return u;
}

tri_motion_history history_of(const tri_global_ubo& u, const float* models, uint32_t n) {
    tri_motion_history h{};
    std::memcpy(h.prev_view, u.view, 64);
    std::memcpy(h.prev_projection, u.projection, 64);
    h.prev_models = models;
    h.draw_count = n;
    return h;
}

bool is_identity(const float* r) {
    float id[16];
    identity(id);
    return std::memcmp(r, id, 64) == 0;  // bitwise: +0, not -0
}

bool all_finite(const std::vector<float>& t) {
    for (float v : t)
        if (!std::isfinite(v)) return false;
    return true;
}

void check_table() {
    const tri_global_ubo u = camera(0.0f, 0.5f, 5.0f);
    std::vector<tri_draw> draws{draw_at(0, 0, 0), draw_at(1, 0, -1, 2.0f), draw_at(-1, 1, 0.5f)};
    std::vector<float> prev;
    for (const tri_draw& d : draws) prev.insert(prev.end(), d.pc.model, d.pc.model + 16);
    std::vector<float> t(4 * 16, -7.0f);

    // no history
    motion::build_table(u, draws.data(), 3, nullptr, t.data());
    for (int k = 0; k < 4; ++k) EXPECT(is_identity(&t[16 * k]));
    // a still frame, with the models given and without
    tri_motion_history h = history_of(u, prev.data(), 3);
    t.assign(t.size(), -7.0f);
    motion::build_table(u, draws.data(), 3, &h, t.data());
    for (int k = 0; k < 4; ++k) EXPECT(is_identity(&t[16 * k]));
    h.prev_models = nullptr;
    h.draw_count = 0;
    t.assign(t.size(), -7.0f);
    motion::build_table(u, draws.data(), 3, &h, t.data());
    for (int k = 0; k < 4; ++k) EXPECT(is_identity(&t[16 * k]));
    // a draw count of 0: the background row alone, and nothing written behind it
    const tri_global_ubo u2 = camera(0.3f, 0.5f, 5.0f);
    tri_motion_history h2 = history_of(u2, nullptr, 0);
    t.assign(t.size(), -7.0f);
    motion::build_table(u, nullptr, 0, &h2, t.data());
    EXPECT(is_identity(&t[0]));  // a translated camera does not move a background at infinity
    EXPECT(t[16] == -7.0f);
    // one draw moved: its row is not the identity, the others' are
    prev[16 + 12] += 0.25f;
    h = history_of(u, prev.data(), 3);
    motion::build_table(u, draws.data(), 3, &h, t.data());
    EXPECT(is_identity(&t[0]) && is_identity(&t[16]) && !is_identity(&t[32]) && is_identity(&t[48]));
    EXPECT(all_finite(t));
    // ... and it is (P V M') inverse(P V M): applied to a clip-space point of the draw it gives the moved point
    {
        double P[16], V[16], M[16], Mp[16], PV[16], cur[16], was[16];
        motion::widen(u.projection, P);
        motion::widen(u.view, V);
        motion::widen(draws[1].pc.model, M);
        motion::widen(&prev[16], Mp);
        motion::mul(P, V, PV);
        motion::mul(PV, M, cur);
        motion::mul(PV, Mp, was);
        const double obj[4] = {0.3, -0.2, 0.1, 1.0};
        double c[4] = {0, 0, 0, 0}, w[4] = {0, 0, 0, 0}, got[4] = {0, 0, 0, 0};
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k) {
                c[i] += cur[4 * k + i] * obj[k];
                w[i] += was[4 * k + i] * obj[k];
            }
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k) got[i] += (double)t[32 + 4 * i + k] * c[k];
        for (int i = 0; i < 4; ++i) EXPECT(std::fabs(got[i] - w[i]) < 1e-5 * (1.0 + std::fabs(w[i])));
    }
}

void check_degenerate() {
    const tri_global_ubo u = camera(0.0f, 0.0f, 5.0f), u2 = camera(0.5f, 0.0f, 5.0f);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<tri_draw> draws{draw_at(0, 0, 0), draw_at(1, 0, 0, 0.0f), draw_at(0, 1, 0), draw_at(0, 0, 1), draw_at(2, 0, 0)};
    for (int i = 0; i < 4; ++i) draws[2].pc.model[4 + i] = draws[2].pc.model[i];  // two equal columns
    draws[3].pc.model[5] = nan;
    draws[4].pc.model[12] = inf;
    std::vector<float> prev;
    for (const tri_draw& d : draws) prev.insert(prev.end(), d.pc.model, d.pc.model + 16);
    identity(&prev[16]);  // the singular draws had good models a frame ago
    identity(&prev[32]);
    tri_motion_history h = history_of(u2, prev.data(), 5);
    std::vector<float> t(6 * 16, -7.0f);
    motion::build_table(u, draws.data(), 5, &h, t.data());
    EXPECT(all_finite(t));
    EXPECT(!is_identity(&t[16]));  // the good draw under a moved camera
    for (int k = 2; k <= 5; ++k) EXPECT(is_identity(&t[16 * k]));
    // good current matrices, a NaN / infinite previous model: no non-finite row
    std::vector<tri_draw> good{draw_at(0, 0, 0), draw_at(1, 0, 0)};
    std::vector<float> pm(32);
    identity(&pm[0]);
    identity(&pm[16]);
    pm[3] = nan;
    pm[16 + 13] = inf;
    h = history_of(u2, pm.data(), 2);
    t.assign(t.size(), -7.0f);
    motion::build_table(u, good.data(), 2, &h, t.data());
    EXPECT(is_identity(&t[16]) && is_identity(&t[32]));
    // a NaN camera, now and before
    tri_global_ubo bad = u;
    bad.view[5] = nan;
    h = history_of(u2, nullptr, 0);
    motion::build_table(bad, good.data(), 2, &h, t.data());
    for (int k = 0; k < 3; ++k) EXPECT(is_identity(&t[16 * k]));
    h = history_of(bad, nullptr, 0);
    motion::build_table(u, good.data(), 2, &h, t.data());
    for (int k = 0; k < 3; ++k) EXPECT(is_identity(&t[16 * k]));
    // an all-zero projection
    tri_global_ubo zero{};
    h = history_of(u, nullptr, 0);
    motion::build_table(zero, good.data(), 2, &h, t.data());
    for (int k = 0; k < 3; ++k) EXPECT(is_identity(&t[16 * k]));
}

void check_pixel_rule() {
    const float W = 101.0f, H = 70.0f, sx = 2.0f / W, sy = 2.0f / H, hw = 0.5f * W, hh = 0.5f * H;
    float R[16], mx, my;
    identity(R);
    for (int y = 0; y < 70; y += 23)
        for (int x = 0; x < 101; x += 9) {
            motion::pixel_motion(R, (float)x + 0.5f, (float)y + 0.5f, 0.37f, sx, sy, hw, hh, &mx, &my);
            uint32_t bx, by;
            std::memcpy(&bx, &mx, 4);
            std::memcpy(&by, &my, 4);
            EXPECT(bx == 0u && by == 0u);
        }
    R[3] = 3.0f * sx;  // three pixels right, two up, in NDC
    R[7] = -2.0f * sy;
    motion::pixel_motion(R, 40.5f, 30.5f, 0.5f, sx, sy, hw, hh, &mx, &my);
    EXPECT(std::fabs(mx - 3.0f) < 1e-4f && std::fabs(my + 2.0f) < 1e-4f);
    R[15] = -1.0f;  // behind the previous camera
    motion::pixel_motion(R, 40.5f, 30.5f, 0.5f, sx, sy, hw, hh, &mx, &my);
    EXPECT(mx == 0.0f && my == 0.0f);
    R[15] = 0.0f;   // on its plane
    motion::pixel_motion(R, 40.5f, 30.5f, 0.5f, sx, sy, hw, hh, &mx, &my);
    EXPECT(mx == 0.0f && my == 0.0f);
    R[15] = std::numeric_limits<float>::quiet_NaN();
    motion::pixel_motion(R, 40.5f, 30.5f, 0.5f, sx, sy, hw, hh, &mx, &my);
    EXPECT(mx == 0.0f && my == 0.0f);
    R[15] = 1e-38f;  // q_0 / q_3 overflows
    R[3] = 1e30f;
    motion::pixel_motion(R, 40.5f, 30.5f, 0.5f, sx, sy, hw, hh, &mx, &my);
    EXPECT(mx == 0.0f && my == 0.0f);
}

void check_arguments() {
    const tri_global_ubo u = camera(0, 0, 5);
    tri_draw d = draw_at(0, 0, 0);
    float models[16], out[32];
    identity(models);
    motion::Msg m;
    tri_motion_history h = history_of(u, models, 0);
    EXPECT(motion::check_history(h, m) == TRI_E_INVALID && m.text[0]);  // models with a count of 0
    h.draw_count = 1;
    EXPECT(motion::check_history(h, m) == TRI_OK);
    h.prev_models = nullptr;
    h.draw_count = 0;
    EXPECT(motion::check_history(h, m) == TRI_OK);
    // tri_render's rule
    EXPECT(motion::count_matches(true, 3, 3) && !motion::count_matches(true, 2, 3) && !motion::count_matches(true, 3, 0));
    EXPECT(motion::count_matches(false, 0, 3) && motion::count_matches(false, 9, 0));
    // tri_motion_matrices
    EXPECT(motion::check_matrices(nullptr, &d, 1, nullptr, out, m) == TRI_E_INVALID);
    EXPECT(motion::check_matrices(&u, &d, 1, nullptr, nullptr, m) == TRI_E_INVALID);
    EXPECT(motion::check_matrices(&u, nullptr, 1, nullptr, out, m) == TRI_E_INVALID);
    EXPECT(motion::check_matrices(&u, nullptr, 0, nullptr, out, m) == TRI_OK);
    h = history_of(u, models, 1);
    EXPECT(motion::check_matrices(&u, &d, 1, &h, out, m) == TRI_OK);
    h.draw_count = 2;
    EXPECT(motion::check_matrices(&u, &d, 1, &h, out, m) == TRI_E_INVALID);  // more models than draws
    h.draw_count = 1;
    EXPECT(motion::check_matrices(&u, nullptr, 0, &h, out, m) == TRI_E_INVALID);  // ... and fewer draws than models
    h.draw_count = 0;
    EXPECT(motion::check_matrices(&u, &d, 1, &h, out, m) == TRI_E_INVALID);  // models with a count of 0
    h.prev_models = nullptr;
    h.draw_count = 7;  // without models the count says nothing
    EXPECT(motion::check_matrices(&u, &d, 1, &h, out, m) == TRI_OK);
}

}  // namespace

int main() {
    check_table();
    check_degenerate();
    check_pixel_rule();
    check_arguments();
    if (g_failures) {
        std::fprintf(stderr, "motion_check: %d failure(s)\n", g_failures);
        return EXIT_FAILURE;
    }
    std::printf("motion_check ok\n");
    return EXIT_SUCCESS;
}
