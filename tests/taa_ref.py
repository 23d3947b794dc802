"""References for temporal anti-aliasing (include/tri_raster.h "temporal anti-aliasing").

  restate()       the device's rule in numpy integers and float32, operation for operation, on reproject_ref's and
                  motion_ref's conventions (every intermediate a float32 array, nothing contracted, a correctly rounded
                  divide): byte-identical to k_taa_resolve when fed the same table, the same frame and the same history;
  restate(..., id_test="nearest") and restate(..., clamp=False)   two wrong rules for the tests to kill: an id test on
                  the nearest previous pixel alone, and the neighbourhood clamp left out;
  halton(), jitter(), jitter_projection()   the jitter in float64;
  jittered(), still_history()   a scene under a jitter, and the motion history the jitter contract asks for.
"""
import copy

import numpy as np

import motion_ref as mr

F = np.float32
NO_HISTORY, NO_PROJ, OUTSIDE, ID, CLAMPED = 1, 2, 4, 8, 32


# ---- the jitter in float64 --------------------------------------------------------------------------------------------
def halton(k, base):
    """The radical inverse of k in `base`, float64: one division of two integers."""
    num, den = 0, 1
    while k:
        num = num * base + k % base
        den *= base
        k //= base
    return num / den


def jitter(index, period):
    """(x, y) in pixels, float64: the centred Halton (2, 3) point of index % period + 1; (0, 0) for a period of 0."""
    if period == 0:
        return 0.0, 0.0
    k = index % period + 1
    return halton(k, 2) - 0.5, halton(k, 3) - 0.5


def jitter_projection(proj, jx, jy, width, height):
    """float64 [16], column-major: rows 0 and 1 gain 2 j / extent times row 3."""
    p = np.asarray(proj, np.float64).reshape(16).copy()
    dx, dy = 2.0 * float(jx) / width, 2.0 * float(jy) / height
    for c in range(4):
        p[4 * c + 0] += dx * p[4 * c + 3]
        p[4 * c + 1] += dy * p[4 * c + 3]
    return p


def jittered(scene, jx, jy):
    """The scene with its projection jittered by the library (tri_taa_jitter_projection, host only)."""
    from trident_raster import abi, raster

    s = copy.copy(scene)
    s.ubo = abi.TriGlobalUbo.from_buffer_copy(scene.ubo)
    p = raster.taa_jitter_projection(np.array(scene.ubo.projection[:], F), jx, jy, scene.width, scene.height)
    s.ubo.projection = (abi.C.c_float * 16)(*p.tolist())
    return s


def contract_history(scene, jx, jy, prev_view=None, prev_projection=None, prev_models=None):
    """The motion history the jitter contract asks for behind jittered(scene, jx, jy): the previous view and the
    previous UNJITTERED projection under the CURRENT jitter (default: the scene's own — a still camera)."""
    from trident_raster import raster

    v, p = mr.camera_of(scene.ubo)
    pv = v if prev_view is None else np.asarray(prev_view, F).reshape(16)
    pp = p if prev_projection is None else np.asarray(prev_projection, F).reshape(16)
    return pv, raster.taa_jitter_projection(pp, jx, jy, scene.width, scene.height), prev_models


# ---- the float32 restatement ------------------------------------------------------------------------------------------
def _locate(table, ids, depth_bits, width, height):
    """history::locate for every pixel: (proj, inside, xi, yi, (xa, xb, ya, yb), fu, fv); the integer outputs are
    meaningful where inside (elsewhere they are those of the pixel itself)."""
    h, w = ids.shape
    T = np.asarray(table, F)

    def Rij(i, j):
        return np.ascontiguousarray(T[:, i, j])[ids]

    x = np.broadcast_to(np.arange(w, dtype=np.int64)[None, :], ids.shape)
    y = np.broadcast_to(np.arange(h, dtype=np.int64)[:, None], ids.shape)
    sx, sy = F(2.0) / F(width), F(2.0) / F(height)
    hw, hh = F(0.5) * F(width), F(0.5) * F(height)
    fx = x.astype(F) + F(0.5)
    fy = y.astype(F) + F(0.5)
    xn = fx * sx - F(1.0)
    yn = fy * sy - F(1.0)
    z = np.where(ids != 0, np.ascontiguousarray(depth_bits, np.uint32).view(F), F(1.0)).astype(F)
    with np.errstate(all="ignore"):
        q = [((Rij(i, 0) * xn + Rij(i, 1) * yn) + Rij(i, 2) * z) + Rij(i, 3) for i in (0, 1, 3)]
        ok = q[2] > F(0.0)
        iw = F(1.0) / np.where(ok, q[2], F(1.0)).astype(F)
        mx = (q[0] * iw - xn) * hw
        my = (q[1] * iw - yn) * hh
        proj = ok & np.isfinite(mx) & np.isfinite(my)
        u = fx + np.where(proj, mx, F(0.0)).astype(F)
        v = fy + np.where(proj, my, F(0.0)).astype(F)
        inside = proj & (u >= F(0.0)) & (u < F(width)) & (v >= F(0.0)) & (v < F(height))
    for a in (mx, my, u, v):
        assert a.dtype == F
    us = np.where(inside, u, fx).astype(F)  # no index from u or v before `inside` holds
    vs = np.where(inside, v, fy).astype(F)
    xi = np.floor(us).astype(np.int64)
    yi = np.floor(vs).astype(np.int64)
    assert xi.min() >= 0 and xi.max() < w and yi.min() >= 0 and yi.max() < h
    su = us - F(0.5)
    sv = vs - F(0.5)
    x0 = np.floor(su)
    y0 = np.floor(sv)
    fu = su - x0
    fv = sv - y0
    assert fu.dtype == F and fv.dtype == F
    xa = np.clip(x0.astype(np.int64), 0, w - 1)
    xb = np.clip(x0.astype(np.int64) + 1, 0, w - 1)
    ya = np.clip(y0.astype(np.int64), 0, h - 1)
    yb = np.clip(y0.astype(np.int64) + 1, 0, h - 1)
    return proj, inside, xi, yi, (xa, xb, ya, yb), fu, fv


def window(a, reduce):
    """reduce (np.minimum / np.maximum / np.logical_or) over the 3 x 3 window of a [H, W, ...] array, coordinates
    clamped to the frame."""
    h, w = a.shape[:2]
    ys = [np.clip(np.arange(h) + d, 0, h - 1) for d in (-1, 0, 1)]
    xs = [np.clip(np.arange(w) + d, 0, w - 1) for d in (-1, 0, 1)]
    out = None
    for yy in ys:
        for xx in xs:
            t = a[yy][:, xx]
            out = t if out is None else reduce(out, t)
    return out


def restate(table, ids, depth_bits, colour, prev, width, height, alpha=0.1, reject_ids=True, id_test="3x3", clamp=True):
    """(accumulated uint16 [H, W, 4], resolved uint8 [H, W, 4], mask uint8 [H, W]). table: float32 [n + 1, 4, 4]; ids,
    depth_bits uint32 [H, W] and colour uint8 [H, W, 4] (B G R A) of the current frame; prev: None (no history) or the
    previous pass's (accumulated uint16 [H, W, 4], ids uint32 [H, W]). The ids the pass stores are `ids`."""
    h, w = ids.shape
    assert (w, h) == (width, height) and depth_bits.shape == ids.shape and colour.shape == ids.shape + (4,)
    assert colour.dtype == np.uint8
    restart16 = (colour.astype(np.uint32) * 257).astype(np.uint16)
    if prev is None:
        return restart16, colour.copy(), np.full(ids.shape, NO_HISTORY, np.uint8)
    pacc, pids = prev
    assert pacc.shape == colour.shape and pacc.dtype == np.uint16 and pids.shape == ids.shape
    proj, inside, xi, yi, (xa, xb, ya, yb), fu, fv = _locate(table, ids, depth_bits, width, height)
    mask = np.zeros(ids.shape, np.uint8)
    mask[~proj] = NO_PROJ
    mask[proj & ~inside] = OUTSIDE
    if reject_ids:
        if id_test == "3x3":
            found = np.zeros(ids.shape, bool)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    found |= pids[np.clip(yi + dy, 0, h - 1), np.clip(xi + dx, 0, w - 1)] == ids
        else:
            assert id_test == "nearest"
            found = pids[yi, xi] == ids
        mask[inside & ~found] = ID
    lo16 = (window(colour, np.minimum).astype(np.uint32) * 257).astype(F)
    hi16 = (window(colour, np.maximum).astype(np.uint32) * 257).astype(F)
    cur16 = (colour.astype(np.uint32) * 257).astype(F)
    a = F(alpha)
    one = F(1.0)
    fu, fv = fu[..., None], fv[..., None]
    c00, c10 = pacc[ya, xa].astype(F), pacc[ya, xb].astype(F)
    c01, c11 = pacc[yb, xa].astype(F), pacc[yb, xb].astype(F)
    t = c00 * (one - fu) + c10 * fu
    b = c01 * (one - fu) + c11 * fu
    hh = t * (one - fv) + b * fv
    hc = np.minimum(np.maximum(hh, lo16), hi16) if clamp else hh
    r = hc * (one - a) + cur16 * a
    assert r.dtype == F
    s = np.minimum((r + F(0.5)).astype(np.int32), 65535)
    out8 = np.minimum((s.astype(F) * (one / F(257.0)) + F(0.5)).astype(np.int32), 255).astype(np.uint8)
    valid = (mask & 15) == 0
    mask[valid & (hc != hh).any(axis=-1)] |= CLAMPED
    acc = np.where(valid[..., None], s.astype(np.uint16), restart16)
    resolved = np.where(valid[..., None], out8, colour)
    return acc, resolved, mask


def silhouette(colour):
    """bool [H, W]: the pixels whose 3 x 3 neighbourhood of `colour` is not constant."""
    return (window(colour, np.minimum) != window(colour, np.maximum)).any(axis=-1)


def flat5(colour):
    """bool [H, W]: the pixels whose 5 x 5 neighbourhood of `colour` is constant."""
    lo, hi = window(window(colour, np.minimum), np.minimum), window(window(colour, np.maximum), np.maximum)
    return (lo == hi).all(axis=-1)
