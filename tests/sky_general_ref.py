"""Float64 restatement of the skybox pass for every cubemap tri_upload_skybox_ex takes (k_sky_fill):
the direction (Skybox.vert's outDirection interpolated over the 20-unit cube, as f64_sky of test_oracle_clip_f64
rasterises it), major-axis face selection, fine quad differences of the normalised direction, the cube map derivative
transformation, lambda and the level blend, and seamless LINEAR taps per level, edge and corner taps included.

Nothing here reads the device's code or the oracle's: the direction is the perspective-correct interpolation of the
cube's vertices, the device's the exit point of a ray."""
import numpy as np

from test_oracle_clip_f64 import _SKY_IDX, _SKY_POS, _srgb_to_linear

FMT_SRGB, FMT_UNORM, FMT_16F = 0, 1, 2
TIE_EPS = 1e-6  # pixels whose two largest |direction components| are closer than this may be left out


def level_sizes(n, mips):
    return [max(1, n >> l) for l in range(mips)]


def chain_texels(n, mips):
    return sum(6 * e * e for e in level_sizes(n, mips))


def split_levels(texels, n, mips):
    """texels: [chain_texels, 4] (level-major, then face, then rows) -> list of [6, e, e, 4] views."""
    t = np.asarray(texels).reshape(-1, 4)
    assert t.shape[0] == chain_texels(n, mips)
    out, at = [], 0
    for e in level_sizes(n, mips):
        out.append(t[at:at + 6 * e * e].reshape(6, e, e, 4))
        at += 6 * e * e
    return out


def decode_levels(texels, fmt, n, mips):
    """The linear RGB of every level as float64 [6, e, e, 3]."""
    levels = split_levels(texels, n, mips)
    if fmt == FMT_16F:
        return [np.asarray(l).view(np.float16).astype(np.float64)[..., :3] for l in levels]
    if fmt == FMT_UNORM:
        return [l[..., :3].astype(np.float64) / 255.0 for l in levels]
    return [_srgb_to_linear(l[..., :3].astype(np.float64)) for l in levels]


def directions(ubo, W, H, xs, ys):
    """Normalised outDirection of the pixels (xs, ys) — integer coordinates of the frame's plane, inside it or not —
    float64 [N, 3]; NaN where the sky does not cover the pixel."""
    view = np.array(ubo.view, np.float64).reshape(4, 4).T
    proj = np.array(ubo.projection, np.float64).reshape(4, 4).T
    R = view[:3, :3]
    vpos = _SKY_POS @ R.T
    clip = np.c_[vpos, np.ones(8)] @ proj.T
    xn = ((np.asarray(xs, np.float64) + 0.5) - W / 2) / (W / 2)
    yn = ((np.asarray(ys, np.float64) + 0.5) - H / 2) / (H / 2)
    dirs = np.full((xn.size, 3), np.nan)
    for t in _SKY_IDX:
        C = clip[t]
        a = C[None, :, 0] - xn[:, None] * C[None, :, 3]
        c = C[None, :, 1] - yn[:, None] * C[None, :, 3]
        b = np.cross(a, c)
        s = b.sum(1, keepdims=True)
        ok = np.abs(s[:, 0]) > 1e-12
        b = b / np.where(ok[:, None], s, 1)
        hit = ok & np.all(b >= 0, axis=1) & (b @ C[:, 3] > 0)
        dirs[hit] = b[hit] @ vpos[t]
    return dirs / np.linalg.norm(dirs, axis=1, keepdims=True)


def face_coords(face, v):
    """(s_c, t_c, r_c) of the vectors v on `face` (Vulkan's cube map face selection table); linear in v."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    sc = np.select([face == 0, face == 1, face == 2, face == 3, face == 4], [-z, z, x, x, x], -x)
    tc = np.select([face == 0, face == 1, face == 2, face == 3, face == 4], [-y, -y, z, -z, -y], -y)
    rc = np.select([face <= 1, face <= 3], [x, y], z)
    return sc, tc, rc


def select_face(d):
    ax = np.abs(d)
    major = np.argmax(ax, axis=1)  # the first largest: x before y before z, as the device's >= tests
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.where(major == 0, np.where(x >= 0, 0, 1), np.where(major == 1, np.where(y >= 0, 2, 3), np.where(z >= 0, 4, 5)))


def face_st(d):
    face = select_face(d)
    sc, tc, rc = face_coords(face, d)
    ma = np.abs(rc)
    return face, 0.5 * sc / ma + 0.5, 0.5 * tc / ma + 0.5


def face_dir(face, sc, tc):
    one = np.ones_like(sc)
    opts = [np.stack(v, 1) for v in ((one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one))]
    return np.select([(face == k)[:, None] for k in range(5)], opts, np.stack((-sc, -tc, -one), 1))


def _across(lin, face, i, j):
    n = lin.shape[1]
    sc = 2.0 * ((i + 0.5) / n) - 1.0
    tc = 2.0 * ((j + 0.5) / n) - 1.0
    f2, s, t = face_st(face_dir(face, sc, tc))
    i2 = np.clip(np.floor(s * n).astype(np.int64), 0, n - 1)
    j2 = np.clip(np.floor(t * n).astype(np.int64), 0, n - 1)
    return lin[f2, j2, i2]


def _fetch(lin, face, i, j):
    """One tap per direction: inside the face its texel, across an edge the adjacent face's texel, at a corner the
    mean of the three texels that meet there."""
    n = lin.shape[1]
    in_i, in_j = (i >= 0) & (i < n), (j >= 0) & (j < n)
    ci, cj = np.clip(i, 0, n - 1), np.clip(j, 0, n - 1)
    inside = lin[face, cj, ci]
    edge = _across(lin, face, np.where(in_i, ci, i), np.where(in_j, cj, j))
    corner = (inside + _across(lin, face, i, cj) + _across(lin, face, ci, j)) / 3.0
    both, one = (in_i & in_j)[:, None], (in_i ^ in_j)[:, None]
    return np.where(both, inside, np.where(one, edge, corner))


def sample_level(lin, d):
    """Seamless LINEAR sample of one level (lin: float64 [6, n, n, 3]) along the directions d."""
    n = lin.shape[1]
    face, s, t = face_st(d)
    u, v = s * n - 0.5, t * n - 0.5
    i0, j0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    a, b = (u - i0)[:, None], (v - j0)[:, None]
    t00, t10 = _fetch(lin, face, i0, j0), _fetch(lin, face, i0 + 1, j0)
    t01, t11 = _fetch(lin, face, i0, j0 + 1), _fetch(lin, face, i0 + 1, j0 + 1)
    return (t00 * (1 - a) + t10 * a) * (1 - b) + (t01 * (1 - a) + t11 * a) * b


def lod(ubo, W, H, n, mips, xs, ys, P):
    """d = min(clamp(log2 rho_max, 0, mips), mips - 1) of the covered pixels (xs, ys) with directions P."""
    face = select_face(P)
    sc, tc, rc = face_coords(face, P)
    ma, sgn = np.abs(rc), np.where(rc >= 0, 1.0, -1.0)

    def rho(nx, ny, own_is_second):
        q = directions(ubo, W, H, nx, ny)
        dP = np.where(own_is_second[:, None], P - q, q - P)
        dP[np.isnan(q[:, 0])] = 0.0  # a neighbour without a sky direction: a zero derivative
        dsc, dtc, drc = face_coords(face, dP)
        dma = sgn * drc
        ds = 0.5 * (ma * dsc - sc * dma) / (rc * rc)
        dt = 0.5 * (ma * dtc - tc * dma) / (rc * rc)
        return n * np.hypot(ds, dt)

    rmax = np.maximum(rho(xs ^ 1, ys, (xs & 1) != 0), rho(xs, ys ^ 1, (ys & 1) != 0))
    lam = np.zeros_like(rmax)
    pos = rmax > 0
    lam[pos] = np.clip(np.log2(rmax[pos]), 0.0, float(mips))
    return np.minimum(lam, mips - 1.0)


def render(scene, texels, fmt, n, mips=1, band=None):
    """The frame's rows [band) as the skybox pass alone leaves them.
    Returns (rgb float64 [rows, W, 3] before the UNORM store: the clamped sky colour, or the clear colour's stored
    bytes / 255 where the sky does not cover the pixel; covered bool [rows, W]; tie bool [rows, W]; d float64 [rows, W],
    NaN where uncovered or for one level)."""
    W, H = scene.width, scene.height
    y0, y1 = band if band is not None else (0, H)
    ys, xs = np.mgrid[y0:y1, 0:W]
    xs, ys = xs.ravel(), ys.ravel()
    P = directions(scene.ubo, W, H, xs, ys)
    cov = ~np.isnan(P[:, 0])
    levels = decode_levels(texels, fmt, n, mips)
    clear = np.floor(np.clip(np.array(scene.clear[:3], np.float32), 0, 1) * np.float32(255.0) + np.float32(0.5)) / 255.0
    rgb = np.tile(clear.astype(np.float64), (xs.size, 1))
    dd = np.full(xs.size, np.nan)
    Pc = P[cov]
    if mips == 1:
        col = sample_level(levels[0], Pc)
    else:
        d = lod(scene.ubo, W, H, n, mips, xs[cov], ys[cov], Pc)
        dd[cov] = d
        l0 = np.floor(d).astype(np.int64)
        l1 = np.minimum(l0 + 1, mips - 1)
        delta = (d - l0)[:, None]
        col = np.zeros((Pc.shape[0], 3))
        for l in range(mips):
            m0, m1 = l0 == l, (l1 == l) & (delta[:, 0] > 0)
            if m0.any():
                col[m0] += (1 - delta[m0]) * sample_level(levels[l], Pc[m0])
            if m1.any():
                col[m1] += delta[m1] * sample_level(levels[l], Pc[m1])
    rgb[cov] = np.clip(col, 0.0, 1.0)
    srt = np.sort(np.abs(Pc), axis=1)
    tie = np.zeros(xs.size, bool)
    tie[cov] = srt[:, 2] - srt[:, 1] < TIE_EPS
    shape = (y1 - y0, W)
    return rgb.reshape(shape + (3,)), cov.reshape(shape), tie.reshape(shape), dd.reshape(shape)


def expected_bytes(rgb):
    """The UNORM8 store of `rgb` (round to nearest), float64 for differences."""
    return np.rint(rgb * 255.0)
