"""References for the motion-vector pass (include/tri_raster.h "motion vectors").

Three independent things:
  restate()        the device's rule in numpy float32, operation for operation (every intermediate is a float32 array,
                   numpy contracts nothing, its divide is correctly rounded): bit-identical to k_motion when fed the
                   same table, ids and depth;
  geometric_f64()  the truth in float64 from the ORIGINAL matrices, not from R: unproject (pixel centre, z) through
                   inverse(P V M) of the pixel's draw, re-project through P' V' M', take the difference in pixels;
  table_f64()      the reprojection table in float64 with numpy.linalg.inv.

Matrices travel as the project's numpy [col][row] arrays (or 16 floats, column-major); mat() makes the mathematical
matrix of one.
"""
import numpy as np

F = np.float32
# The bound on |restatement - geometric_f64| in pixels: the next power of two at or above twice the largest error
# measured on the CPU over test_motion_cpu.py's scenes (e = 5.73e-5 px, 2e = 1.15e-4 <= 2^-13: DESIGN 5n). Never above
# 1/16 px.
BOUND_PX = 2.0 ** -13
assert BOUND_PX <= 1.0 / 16.0


def mat(a):
    """The mathematical 4 x 4 (float64) of a column-major matrix."""
    return np.asarray(a, np.float64).reshape(4, 4).T


def camera_of(ubo):
    """(view, projection) of a uniform block as flat float32 column-major arrays."""
    return np.array(ubo.view[:], F), np.array(ubo.projection[:], F)


def models_of(draws):
    return np.array([d.pc.model[:] for d in draws], F).reshape(-1, 16)


def history(prev_ubo, prev_models):
    """The argument tuple of raster.motion_matrices / TriRaster.set_motion_history."""
    v, p = camera_of(prev_ubo)
    return v, p, prev_models


# ---- the float32 restatement ----------------------------------------------------------------------------------------
def restate(table, ids, depth_bits, width, height, y0=0):
    """float32 [rows, W, 2] from the table (float32 [n + 1, 4, 4] row-major R_k), the ids and the depth bits of the
    context's rows [y0, y0 + rows) of a width x height frame."""
    rows, w = ids.shape
    assert w == width and depth_bits.shape == ids.shape
    R = np.asarray(table, F)[ids]  # [rows, W, 4, 4]
    x = np.broadcast_to(np.arange(w, dtype=np.int64)[None, :], ids.shape)
    y = np.broadcast_to(np.arange(y0, y0 + rows, dtype=np.int64)[:, None], ids.shape)
    sx, sy = F(2.0) / F(width), F(2.0) / F(height)
    hw, hh = F(0.5) * F(width), F(0.5) * F(height)
    fx = x.astype(F) + F(0.5)
    fy = y.astype(F) + F(0.5)
    xn = fx * sx - F(1.0)
    yn = fy * sy - F(1.0)
    z = np.where(ids != 0, np.ascontiguousarray(depth_bits, np.uint32).view(F), F(1.0)).astype(F)
    with np.errstate(all="ignore"):
        q = [((R[..., i, 0] * xn + R[..., i, 1] * yn) + R[..., i, 2] * z) + R[..., i, 3] for i in (0, 1, 3)]
        for a in q:
            assert a.dtype == F
        ok = q[2] > F(0.0)
        iw = F(1.0) / np.where(ok, q[2], F(1.0)).astype(F)
        mx = (q[0] * iw - xn) * hw
        my = (q[1] * iw - yn) * hh
    assert mx.dtype == F and my.dtype == F
    ok &= np.isfinite(mx) & np.isfinite(my)
    out = np.zeros(ids.shape + (2,), F)
    out[..., 0] = np.where(ok, mx, F(0.0))
    out[..., 1] = np.where(ok, my, F(0.0))
    return out


# ---- float64 ---------------------------------------------------------------------------------------------------------
def _no_translation(v):
    v = v.copy()
    v[:, 3] = (0.0, 0.0, 0.0, 1.0)
    return v


def _pairs(view, proj, models, prev_view, prev_proj, prev_models):
    """Per table row k the float64 pair (P V M, P' V' M'); row 0 is the background at infinity."""
    P, V, Pp, Vp = mat(proj), mat(view), mat(prev_proj), mat(prev_view)
    out = [(P @ _no_translation(V), Pp @ _no_translation(Vp))]
    for k in range(len(models)):
        M = mat(models[k])
        Mp = mat(prev_models[k]) if prev_models is not None else M
        out.append((P @ V @ M, Pp @ Vp @ Mp))
    return out


def table_f64(view, proj, models, prev_view, prev_proj, prev_models=None):
    """float64 [n + 1, 4, 4]: R_k = (P' V' M') inverse(P V M) with numpy.linalg.inv."""
    return np.array([prev @ np.linalg.inv(cur) for cur, prev in _pairs(view, proj, models, prev_view, prev_proj, prev_models)])


def geometric_f64(view, proj, models, prev_view, prev_proj, prev_models, ids, depth_bits, width, height, y0=0):
    """float64 [rows, W, 2]: the true motion of every pixel, and a bool mask of the pixels whose point lay in front of
    the previous camera (elsewhere the device stores zeros)."""
    rows, w = ids.shape
    x = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :] + 0.5, ids.shape)
    y = np.broadcast_to(np.arange(y0, y0 + rows, dtype=np.float64)[:, None] + 0.5, ids.shape)
    xn, yn = x * 2.0 / width - 1.0, y * 2.0 / height - 1.0
    z = np.where(ids != 0, np.ascontiguousarray(depth_bits, np.uint32).view(F).astype(np.float64), 1.0)
    ndc = np.stack([xn, yn, z, np.ones_like(xn)], axis=-1)  # [rows, W, 4]
    out = np.zeros(ids.shape + (2,), np.float64)
    front = np.zeros(ids.shape, bool)
    for k, (cur, prev) in enumerate(_pairs(view, proj, models, prev_view, prev_proj, prev_models)):
        sel = ids == k
        if not sel.any():
            continue
        obj = np.linalg.solve(cur, ndc[sel].T)  # object-space points (homogeneous, any scale)
        clip = prev @ obj
        wq = clip[3]
        f = wq > 0.0
        with np.errstate(all="ignore"):
            px = (clip[0] / wq + 1.0) * 0.5 * width
            py = (clip[1] / wq + 1.0) * 0.5 * height
        m = np.stack([np.where(f, px - x[sel], 0.0), np.where(f, py - y[sel], 0.0)], axis=-1)
        out[sel] = m
        front[sel] = f
    return out, front


# ---- a previous frame for any scene ---------------------------------------------------------------------------------
def to_cm(m):
    """A mathematical 4 x 4 back to the project's float32 [col][row] array."""
    return np.ascontiguousarray(np.asarray(m, np.float64).T.astype(F))


def rigid(translation=(0, 0, 0), rotation_deg=(0, 0, 0), scale=1.0):
    """A mathematical float64 T Rx Ry Rz S."""
    from math import cos, radians, sin

    rx, ry, rz = (radians(a) for a in rotation_deg)
    X = np.array([[1, 0, 0, 0], [0, cos(rx), -sin(rx), 0], [0, sin(rx), cos(rx), 0], [0, 0, 0, 1]], np.float64)
    Y = np.array([[cos(ry), 0, sin(ry), 0], [0, 1, 0, 0], [-sin(ry), 0, cos(ry), 0], [0, 0, 0, 1]], np.float64)
    Z = np.array([[cos(rz), -sin(rz), 0, 0], [sin(rz), cos(rz), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    T = np.eye(4)
    T[:3, 3] = translation
    return T @ X @ Y @ Z @ np.diag([scale, scale, scale, 1.0])


# how draw k (mod 3) lay one frame ago relative to now: translated, rotated, scaled — each draw differently
DRAW_MOVES = [rigid((0.12, -0.05, 0.0)), rigid((-0.05, 0.08, 0.1), (0.0, 7.0, 3.0)), rigid((0.0, 0.04, 0.0), (4.0, 0.0, 0.0), 0.93)]
# ... and the camera: moved and turned
CAMERA_MOVE = rigid((0.08, -0.03, 0.15), (1.0, -2.5, 0.8))


def previous_frame(scene, still=(), camera_move=CAMERA_MOVE):
    """(prev_view, prev_projection, prev_models) for any scene: the view is camera_move times the scene's, the
    projection the scene's, draw k's model DRAW_MOVES[k % 3] times its own — except the draws in `still`, whose models
    keep their bits."""
    v, p = camera_of(scene.ubo)
    pv = to_cm(camera_move @ mat(v)).reshape(16) if camera_move is not None else v
    models = models_of(scene.draws)
    prev = models.copy()
    for k in range(len(models)):
        if k not in still:
            prev[k] = to_cm(DRAW_MOVES[k % 3] @ mat(models[k])).reshape(16)
    return pv, p, prev


def mutants():
    """Wrong rules the bound must reject: name -> function (table, ids, depth, W, H, y0) -> motion. (The third, previous
    and current swapped, is a table built the other way round: the tests build it.)"""
    def transposed(t, *a):
        return restate(np.ascontiguousarray(np.swapaxes(np.asarray(t, F), 1, 2)), *a)

    def unflipped_y(t, ids, dep, w, h, y0=0):
        # a rule that takes NDC y up: yn -> -yn on the way in and on the way out
        flip = np.diag([1.0, -1.0, 1.0, 1.0]).astype(F)
        t2 = np.array([flip @ r @ flip for r in np.asarray(t, F)], F)
        return restate(t2, ids, dep, w, h, y0)

    return {"transposed R": transposed, "un-flipped y": unflipped_y}
