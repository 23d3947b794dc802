"""References for temporal upscaling (include/tri_raster.h "temporal upscaling").

  sample()        which render pixel each output pixel takes, and the sample's weight k, in float32;
  restate()       the device's rule in numpy integers and float32, operation for operation, on taa_ref's and
                  reproject_ref's conventions (every intermediate a float32 array, nothing contracted, a correctly rounded
                  divide): byte-identical to k_upscale_resolve when fed the same table, the same frame and the same history;
  restate(..., weight="one") and restate(..., clamp=False)   two wrong rules for the tests to kill: k fixed at 1 (plain
                  nearest-sample accumulation) and the neighbourhood clamp left out;
  nearest()       the nearest-neighbour enlargement of a render-extent frame (the sample rule without jitter);
  jitter_period() the period in float64.
"""
import math

import numpy as np

import taa_ref as tr

F = np.float32
NO_HISTORY, NO_PROJ, OUTSIDE, ID, CLAMPED, NO_SAMPLE = 1, 2, 4, 8, 32, 64


def jitter_period(rw, rh, ow, oh):
    return min(64, math.ceil(8.0 * (ow / rw) * (oh / rh)))


def ratios(rw, rh, ow, oh):
    """rx, ry, ox, oy: one float32 division each."""
    return F(rw) / F(ow), F(rh) / F(oh), F(ow) / F(rw), F(oh) / F(rh)


def sample(rw, rh, ow, oh, jx=0.0, jy=0.0):
    """(xr int64 [Ho, Wo], yr, k float32 [Ho, Wo])."""
    rx, ry, ox, oy = ratios(rw, rh, ow, oh)
    jx, jy = F(jx), F(jy)
    cx = np.broadcast_to(np.arange(ow, dtype=np.int64)[None, :].astype(F) + F(0.5), (oh, ow))
    cy = np.broadcast_to(np.arange(oh, dtype=np.int64)[:, None].astype(F) + F(0.5), (oh, ow))
    px, py = cx * rx, cy * ry
    xr = np.clip(np.floor(px + jx).astype(np.int64), 0, rw - 1)
    yr = np.clip(np.floor(py + jy).astype(np.int64), 0, rh - 1)
    dx = ((xr.astype(F) + F(0.5)) - jx) * ox - cx
    dy = ((yr.astype(F) + F(0.5)) - jy) * oy - cy
    k = np.maximum(F(0.0), F(1.0) - np.abs(dx)) * np.maximum(F(0.0), F(1.0) - np.abs(dy))
    for a in (px, py, dx, dy, k):
        assert a.dtype == F
    return xr, yr, k


def nearest(img, ow, oh):
    """The render-extent image [Hr, Wr, ...] enlarged to [Ho, Wo, ...] by the unjittered sample rule."""
    xr, yr, _ = sample(img.shape[1], img.shape[0], ow, oh)
    return img[yr, xr]


def restate(table, ids, depth_bits, colour, prev, ow, oh, jitter=(0.0, 0.0), alpha=0.1, reject_ids=True, weight="rule",
            clamp=True):
    """(accumulated uint16 [Ho, Wo, 4], resolved uint8 [Ho, Wo, 4], mask uint8 [Ho, Wo]). table: float32 [n + 1, 4, 4]; ids,
    depth_bits uint32 [Hr, Wr] and colour uint8 [Hr, Wr, 4] (B G R A) of the current frame; prev: None (no history) or the
    previous pass's (accumulated uint16 [Ho, Wo, 4], ids uint32 [Hr, Wr]). The ids the pass stores are `ids`."""
    rh, rw = ids.shape
    assert depth_bits.shape == ids.shape and colour.shape == ids.shape + (4,) and colour.dtype == np.uint8
    rx, ry, _, _ = ratios(rw, rh, ow, oh)
    xr, yr, k = sample(rw, rh, ow, oh, *jitter)
    if weight == "one":
        k = np.ones_like(k)
    else:
        assert weight == "rule"
    c, i, d = colour[yr, xr], ids[yr, xr], depth_bits[yr, xr]
    restart16 = (c.astype(np.uint32) * 257).astype(np.uint16)
    if prev is None:
        return restart16, c.copy(), np.full((oh, ow), NO_HISTORY, np.uint8)
    pacc, pids = prev
    assert pacc.shape == (oh, ow, 4) and pacc.dtype == np.uint16 and pids.shape == ids.shape
    proj, inside, xi, yi, (xa, xb, ya, yb), fu, fv = tr._locate(table, i, d, ow, oh)
    mask = np.zeros((oh, ow), np.uint8)
    mask[~proj] = NO_PROJ
    mask[proj & ~inside] = OUTSIDE
    if reject_ids:
        xq = np.minimum(((xi.astype(F) + F(0.5)) * rx).astype(np.int64), rw - 1)
        yq = np.minimum(((yi.astype(F) + F(0.5)) * ry).astype(np.int64), rh - 1)
        found = np.zeros((oh, ow), bool)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                found |= pids[np.clip(yq + dy, 0, rh - 1), np.clip(xq + dx, 0, rw - 1)] == i
        mask[inside & ~found] = ID
    lo16 = (tr.window(colour, np.minimum)[yr, xr].astype(np.uint32) * 257).astype(F)
    hi16 = (tr.window(colour, np.maximum)[yr, xr].astype(np.uint32) * 257).astype(F)
    cur16 = (c.astype(np.uint32) * 257).astype(F)
    a = (F(alpha) * k)[..., None]
    assert a.dtype == F
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
    mask[valid & (k == F(0.0))] |= NO_SAMPLE
    acc = np.where(valid[..., None], s.astype(np.uint16), restart16)
    resolved = np.where(valid[..., None], out8, c)
    return acc, resolved, mask
