// motion_math.h — the plain-C++ part of the motion-vector pass (include/tri_raster.h "motion vectors"): the argument
// rules of its entry points and the reprojection table tri_motion_matrices builds, in float64. No HIP:
// host/tools/motion_check.cpp runs all of it under the sanitizers, and the C-ABI (tri_motion.hip) calls the same code.
//
// Row k of the table is R_k, row-major in float32: R_0 for the background, R_{d+1} for draw d. With P, V the frame's
// projection and view, M_d the draw's model and primes for the previous frame,
//     R_{d+1} = (P' V' M'_d) inverse(P V M_d),        R_0 = (P' V'_0) inverse(P V_0)
// where V_0 is V with its translation column replaced by (0, 0, 0, 1): the background lies at infinity, and k_motion
// applies R_0 at z = 1. Products and the inverse are float64, rounded to float32 once. A row is the exact identity —
// motion bits 0 — when the current and previous matrices are bitwise equal, when there is no history, when P V M is
// singular or non-finite, and when the rounded row would hold a non-finite entry.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/tri_raster.h"

namespace motion {

struct Msg {
    char text[160] = {0};
};

// tri_set_motion_history / tri_motion_matrices: the descriptor alone.
inline int check_history(const tri_motion_history& h, Msg& m) {
    if (h.prev_models && h.draw_count == 0) {
        std::snprintf(m.text, sizeof m.text, "previous models given with a draw count of 0");
        return TRI_E_INVALID;
    }
    return TRI_OK;
}

// The stored history against the frame's draw list: previous models are per draw of the current list.
inline bool count_matches(bool have_models, uint32_t history_count, uint32_t draw_count) {
    return !have_models || history_count == draw_count;
}

// tri_motion_matrices' arguments.
inline int check_matrices(const tri_global_ubo* ubo, const tri_draw* draws, uint32_t draw_count, const tri_motion_history* h,
                          const float* out, Msg& m) {
    if (!ubo || !out) {
        std::snprintf(m.text, sizeof m.text, "null argument");
        return TRI_E_INVALID;
    }
    if (draw_count && !draws) {
        std::snprintf(m.text, sizeof m.text, "null draws with a count of %u", draw_count);
        return TRI_E_INVALID;
    }
    if (!h) return TRI_OK;
    if (const int rc = check_history(*h, m)) return rc;
    if (!count_matches(h->prev_models != nullptr, h->draw_count, draw_count)) {
        std::snprintf(m.text, sizeof m.text, "%u previous models for %u draws", h->draw_count, draw_count);
        return TRI_E_INVALID;
    }
    return TRI_OK;
}

// Column-major 4 x 4, as tri_global_ubo: element (row i, column j) at [4 * j + i].
inline void widen(const float* m, double* out) {
    for (int i = 0; i < 16; ++i) out[i] = (double)m[i];
}
inline void mul(const double* a, const double* b, double* out) {  // out = a b
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[4 * k + i] * b[4 * j + k];
            out[4 * j + i] = s;
        }
}
inline void at_infinity(double* v) {  // a view without its translation
    v[12] = 0.0; v[13] = 0.0; v[14] = 0.0; v[15] = 1.0;
}

// Gauss-Jordan with partial pivoting. False for a matrix that is non-finite, singular, or so close to it that the
// inverse means nothing in float32 (max|A| max|inverse(A)| beyond 1e12; the frames' own matrices stay below 1e6).
inline bool invert(const double* a, double* inv) {
    double w[4][8];
    double amax = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const double v = a[4 * j + i];
            if (!std::isfinite(v)) return false;
            w[i][j] = v;
            w[i][4 + j] = i == j ? 1.0 : 0.0;
            amax = std::fmax(amax, std::fabs(v));
        }
    if (!(amax > 0.0)) return false;
    for (int c = 0; c < 4; ++c) {
        int p = c;
        for (int r = c + 1; r < 4; ++r)
            if (std::fabs(w[r][c]) > std::fabs(w[p][c])) p = r;
        if (!(std::fabs(w[p][c]) > 0.0)) return false;
        if (p != c)
            for (int j = 0; j < 8; ++j) {
                const double t = w[c][j];
                w[c][j] = w[p][j];
                w[p][j] = t;
            }
        const double d = 1.0 / w[c][c];
        for (int j = 0; j < 8; ++j) w[c][j] *= d;
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double f = w[r][c];
            if (f == 0.0) continue;
            for (int j = 0; j < 8; ++j) w[r][j] -= f * w[c][j];
        }
    }
    double imax = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const double v = w[i][4 + j];
            if (!std::isfinite(v)) return false;
            inv[4 * j + i] = v;
            imax = std::fmax(imax, std::fabs(v));
        }
    return amax * imax < 1e12;
}

inline void identity_row(float* out) {
    for (int i = 0; i < 16; ++i) out[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

// out (row-major float32) = prev inverse(cur), or the identity where that is undefined.
inline void reprojection_row(const double* cur, const double* prev, float* out) {
    double inv[16], r[16];
    if (!invert(cur, inv)) {
        identity_row(out);
        return;
    }
    mul(prev, inv, r);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const float v = (float)r[4 * j + i];
            if (!std::isfinite(v)) {
                identity_row(out);
                return;
            }
            out[4 * i + j] = v;
        }
}

// The whole table: (draw_count + 1) x 16 floats. `hist` may be null (no history: identities). The caller has checked
// check_history and count_matches.
inline void build_table(const tri_global_ubo& ubo, const tri_draw* draws, uint32_t draw_count, const tri_motion_history* hist,
                        float* out) {
    if (!hist) {
        for (uint32_t k = 0; k <= draw_count; ++k) identity_row(out + 16 * (size_t)k);
        return;
    }
    const bool same_camera = std::memcmp(ubo.view, hist->prev_view, 64) == 0 &&
                             std::memcmp(ubo.projection, hist->prev_projection, 64) == 0;
    double P[16], V[16], Pp[16], Vp[16], PV[16], PVp[16];
    widen(ubo.projection, P);
    widen(ubo.view, V);
    widen(hist->prev_projection, Pp);
    widen(hist->prev_view, Vp);
    mul(P, V, PV);
    mul(Pp, Vp, PVp);
    if (same_camera) {
        identity_row(out);
    } else {
        double V0[16], Vp0[16], cur[16], prev[16];
        std::memcpy(V0, V, sizeof V0);
        std::memcpy(Vp0, Vp, sizeof Vp0);
        at_infinity(V0);
        at_infinity(Vp0);
        mul(P, V0, cur);
        mul(Pp, Vp0, prev);
        reprojection_row(cur, prev, out);
    }
    for (uint32_t d = 0; d < draw_count; ++d) {
        const float* m = draws[d].pc.model;
        const float* mp = hist->prev_models ? hist->prev_models + 16 * (size_t)d : m;
        float* row = out + 16 * (size_t)(d + 1);
        if (same_camera && std::memcmp(m, mp, 64) == 0) {
            identity_row(row);
            continue;
        }
        double M[16], Mp[16], cur[16], prev[16];
        widen(m, M);
        widen(mp, Mp);
        mul(PV, M, cur);
        mul(PVp, Mp, prev);
        reprojection_row(cur, prev, row);
    }
}

// k_motion's rule for one pixel, operation for operation (float32, no contraction): what the kernel computes, for the
// host check and for readers of the code. R: the pixel's table row.
inline void pixel_motion(const float* R, float fx, float fy, float z, float sx, float sy, float hw, float hh, float* mx,
                         float* my) {
    const float xn = fx * sx - 1.0f, yn = fy * sy - 1.0f;
    const float q0 = ((R[0] * xn + R[1] * yn) + R[2] * z) + R[3];
    const float q1 = ((R[4] * xn + R[5] * yn) + R[6] * z) + R[7];
    const float q3 = ((R[12] * xn + R[13] * yn) + R[14] * z) + R[15];
    *mx = 0.0f;
    *my = 0.0f;
    if (!(q3 > 0.0f)) return;
    const float iw = 1.0f / q3;
    const float x = (q0 * iw - xn) * hw, y = (q1 * iw - yn) * hh;
    if (!std::isfinite(x) || !std::isfinite(y)) return;
    *mx = x;
    *my = y;
}

}  // namespace motion
