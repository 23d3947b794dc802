"""References for the history reprojection pass (include/tri_raster.h "history reprojection").

  restate()       the device's rule in numpy float32, operation for operation, on motion_ref.restate's conventions
                  (every intermediate a float32 array, nothing contracted, a correctly rounded divide): byte-identical to
                  k_reproject when fed the same table and the same two frames;
  classify_f64()  the truth in float64 from the ORIGINAL matrices (motion_ref.geometric_f64): each pixel's true previous
                  position, the pixel it falls into, that pixel's previous id;
  previous_scene() the scene one frame ago, for a history of motion_ref.previous_frame's kind.
"""
import copy

import numpy as np

import motion_ref as mr

F = np.float32
NO_HISTORY, NO_PROJ, OUTSIDE, ID, DEPTH = 1, 2, 4, 8, 16


def restate(table, ids, depth_bits, colour, prev, width, height, tolerance=0.0):
    """(warped uint8 [H, W, 4], mask uint8 [H, W]). table: float32 [n + 1, 4, 4]; ids, depth_bits uint32 [H, W] and
    colour uint8 [H, W, 4] (B G R A) of the current frame; prev: None (no history) or the previous frame's
    (ids, depth_bits, colour)."""
    h, w = ids.shape
    assert (w, h) == (width, height) and depth_bits.shape == ids.shape and colour.shape == ids.shape + (4,)
    if prev is None:
        return colour.copy(), np.full(ids.shape, NO_HISTORY, np.uint8)
    pids, pdep_bits, pcol = prev
    assert pids.shape == ids.shape and pdep_bits.shape == ids.shape and pcol.shape == colour.shape
    pdep = np.ascontiguousarray(pdep_bits, np.uint32).view(F)
    tol = F(tolerance)
    T = np.asarray(table, F)

    def Rij(i, j):  # R[i][j] of every pixel's row (entry by entry: a 4K frame's whole rows would be half a gigabyte)
        return np.ascontiguousarray(T[:, i, j])[ids]

    x =np.broadcast_to(np.arange(w, dtype=np.int64)[None, :], ids.shape)
    y = np.broadcast_to(np.arange(h, dtype=np.int64)[:, None], ids.shape)
    sx, sy = F(2.0) / F(width), F(2.0) / F(height)
    hw, hh = F(0.5) * F(width), F(0.5) * F(height)
    fx = x.astype(F) + F(0.5)
    fy = y.astype(F) + F(0.5)
    xn = fx * sx - F(1.0)
    yn = fy * sy - F(1.0)
    z = np.where(ids != 0, np.ascontiguousarray(depth_bits, np.uint32).view(F), F(1.0)).astype(F)
    with np.errstate(all="ignore"):
        q = [((Rij(i, 0) * xn + Rij(i, 1) * yn) + Rij(i, 2) * z) + Rij(i, 3) for i in range(4)]
        ok = q[3] > F(0.0)
        iw = F(1.0) / np.where(ok, q[3], F(1.0)).astype(F)
        mx = (q[0] * iw - xn) * hw
        my = (q[1] * iw - yn) * hh
        proj = ok & np.isfinite(mx) & np.isfinite(my)
        u = fx + np.where(proj, mx, F(0.0)).astype(F)
        v = fy + np.where(proj, my, F(0.0)).astype(F)
        inside = proj & (u >= F(0.0)) & (u < F(width)) & (v >= F(0.0)) & (v < F(height))
        zp = q[2] * iw
    for a in (mx, my, u, v, zp):
        assert a.dtype == F
    us = np.where(inside, u, F(0.5)).astype(F)  # no index from u or v before `inside` holds
    vs = np.where(inside, v, F(0.5)).astype(F)
    xi = np.floor(us).astype(np.int64)
    yi = np.floor(vs).astype(np.int64)
    assert xi.min() >= 0 and xi.max() < w and yi.min() >= 0 and yi.max() < h
    pid = pids[yi, xi]
    with np.errstate(all="ignore"):
        far = ~(np.abs(zp - pdep[yi, xi]) <= tol)
    mask = np.zeros(ids.shape, np.uint8)
    mask[~proj] = NO_PROJ
    mask[proj & ~inside] = OUTSIDE
    mask[inside & (pid != ids)] = ID
    if tol > 0:
        mask[inside & (pid == ids) & (ids != 0) & far] = DEPTH
    su = us - F(0.5)
    sv = vs - F(0.5)
    x0 = np.floor(su)
    y0 = np.floor(sv)
    fu = (su - x0)[..., None]
    fv = (sv - y0)[..., None]
    assert fu.dtype == F and fv.dtype == F
    xa = np.clip(x0.astype(np.int64), 0, w - 1)
    xb = np.clip(x0.astype(np.int64) + 1, 0, w - 1)
    ya = np.clip(y0.astype(np.int64), 0, h - 1)
    yb = np.clip(y0.astype(np.int64) + 1, 0, h - 1)
    c00, c10 = pcol[ya, xa].astype(F), pcol[ya, xb].astype(F)
    c01, c11 = pcol[yb, xa].astype(F), pcol[yb, xb].astype(F)
    one = F(1.0)
    t = c00 * (one - fu) + c10 * fu
    b = c01 * (one - fu) + c11 * fu
    r = t * (one - fv) + b * fv
    assert r.dtype == F
    out = np.minimum((r + F(0.5)).astype(np.int32), 255).astype(np.uint8)
    warped = np.where((mask == 0)[..., None], out, colour)
    return warped, mask


def classify_f64(scene, hist, ids, depth_bits, prev_ids):
    """dict of bool [H, W] arrays from float64 geometry: `outside` (the true previous position lies outside the frame),
    `id` (inside, and the pixel it falls into showed another id), `valid` (inside, same id), `near` (the true position
    is within motion_ref.BOUND_PX of a pixel boundary in x or y — the frame's borders are such boundaries — so float32
    may legitimately land in the neighbour), plus `xi`, `yi` (int64, meaningful where not outside)."""
    w, h = scene.width, scene.height
    v, p = mr.camera_of(scene.ubo)
    m64, front = mr.geometric_f64(v, p, mr.models_of(scene.draws), *hist, ids, depth_bits, w, h)
    assert front.all()
    x = np.arange(w, dtype=np.float64)[None, :] + 0.5 + m64[..., 0]
    y = np.arange(h, dtype=np.float64)[:, None] + 0.5 + m64[..., 1]
    near = (np.abs(x - np.round(x)) <= mr.BOUND_PX) | (np.abs(y - np.round(y)) <= mr.BOUND_PX)
    outside = ~((x >= 0) & (x < w) & (y >= 0) & (y < h))
    xi = np.clip(np.floor(x), 0, w - 1).astype(np.int64)
    yi = np.clip(np.floor(y), 0, h - 1).astype(np.int64)
    same = prev_ids[yi, xi] == ids
    return {"outside": outside, "id": ~outside & ~same, "valid": ~outside & same, "near": near, "xi": xi, "yi": yi}


def previous_scene(scene, hist):
    """The scene as it was one frame ago under hist = (prev_view, prev_projection, prev_models or None)."""
    from trident_raster import abi

    pv, pp, prev = hist
    was = copy.copy(scene)
    was.name = scene.name + "_prev"
    was.ubo = abi.TriGlobalUbo.from_buffer_copy(scene.ubo)
    was.ubo.view = abi.mat_to_c(pv)
    was.ubo.projection = abi.mat_to_c(pp)
    if prev is not None:
        was.draws = [abi.make_draw(d.mesh_index, prev[k]) for k, d in enumerate(scene.draws)]
    return was


def ndc_translation_table(width, height, dx, dy, rows=1):
    """A table whose every row moves a point by (dx, dy) pixels: a pure NDC translation."""
    t = np.broadcast_to(np.eye(4, dtype=F), (rows, 4, 4)).copy()
    t[:, 0, 3] = F(dx) * F(2.0) / F(width)
    t[:, 1, 3] = F(dy) * F(2.0) / F(height)
    return t
