"""NumPy float64 restatement of the text overlay pass (include/tri_raster.h "text overlay"; the reference's Text.vert /
Text.frag under the pipeline state of TextRenderer::CreatePipeline) and of TextRenderer::RecordViewport's layout rule.
Written from the rules, not from the kernel.

Tolerance of a device frame against `composite`: 1 LSB per channel, at any stacking depth — two pixels that differ by at
most 1 LSB before a blend differ by at most (1 - src.a) LSB after it, and so by at most 1 after rounding. Pixels outside
`covered` are not written by the pass: they must be bit-identical to the frame without text."""
import numpy as np


def quad(x0, y0, x1, y1, u0=0.0, v0=0.0, u1=1.0, v1=1.0, rgba=(1.0, 1.0, 1.0, 1.0)):
    return [x0, y0, x1, y1, u0, v0, u1, v1, *rgba]


def snap(x):
    """X = (int32_t)rintf(x * 256.0f): the product in float32, pinned to [-2^29, 2^29], round half to even."""
    with np.errstate(over="ignore"):
        p = np.float32(x) * np.float32(256.0)
    return int(np.rint(np.clip(p, np.float32(-2.0 ** 29), np.float32(2.0 ** 29))))


def unorm8(c):
    """clamp, * 255 + 0.5, truncate."""
    return np.floor(np.clip(c, 0.0, 1.0) * 255.0 + 0.5).astype(np.int64)


def sample(atlas, u, v):
    """A8 UNORM, LINEAR, CLAMP_TO_EDGE, level 0; u, v arrays of one shape."""
    h, w = atlas.shape
    t = atlas.astype(np.float64) / 255.0
    x, y = u * w - 0.5, v * h - 0.5
    fx, fy = np.floor(x), np.floor(y)
    a, b = x - fx, y - fy
    i0, j0 = fx.astype(np.int64), fy.astype(np.int64)
    xa, xb = np.clip(i0, 0, w - 1), np.clip(i0 + 1, 0, w - 1)
    ya, yb = np.clip(j0, 0, h - 1), np.clip(j0 + 1, 0, h - 1)
    l0 = t[ya, xa] + a * (t[ya, xb] - t[ya, xa])
    l1 = t[yb, xa] + a * (t[yb, xb] - t[yb, xa])
    return l0 + b * (l1 - l0)


def composite(frame_bgra, atlas, quads):
    """frame_bgra: uint8 [H, W, 4] (B, G, R, A) before the pass; atlas: uint8 [h, w]; quads: rows of 12 floats in
    submission order. Returns (uint8 frame after the pass, bool [H, W] pixels some quad covers)."""
    out = frame_bgra.astype(np.int64).copy()
    H, W = out.shape[:2]
    covered = np.zeros((H, W), bool)
    for q in np.asarray(quads, np.float32).reshape(-1, 12):
        X0, Y0, X1, Y1 = snap(q[0]), snap(q[1]), snap(q[2]), snap(q[3])
        u0, v0, u1, v1 = (float(f) for f in q[4:8])
        if X1 < X0:  # cull NONE: drawn mirrored
            X0, X1, u0, u1 = X1, X0, u1, u0
        if Y1 < Y0:
            Y0, Y1, v0, v1 = Y1, Y0, v1, v0
        cx, cy = np.arange(W) * 256 + 128, np.arange(H) * 256 + 128
        xs, ys = np.nonzero((cx >= X0) & (cx < X1))[0], np.nonzero((cy >= Y0) & (cy < Y1))[0]
        if xs.size == 0 or ys.size == 0:
            continue
        tx = (cx[xs] - X0) / float(X1 - X0)
        ty = (cy[ys] - Y0) / float(Y1 - Y0)
        # (u1 - u0 in float32, as Text.vert's interpolants are)
        u = u0 + tx * float(np.float32(u1) - np.float32(u0))
        v = v0 + ty * float(np.float32(v1) - np.float32(v0))
        al = sample(atlas, np.broadcast_to(u[None, :], (ys.size, xs.size)), np.broadcast_to(v[:, None], (ys.size, xs.size)))
        r, g, b, a = (float(f) for f in q[8:12])
        src = np.clip(np.stack([b * al, g * al, r * al, a * al], axis=-1), 0.0, 1.0)  # B, G, R, A
        sa = src[..., 3:4]
        win = np.ix_(ys, xs)
        dst = out[win] / 255.0
        res = np.empty_like(dst)
        res[..., :3] = src[..., :3] * sa + dst[..., :3] * (1.0 - sa)  # the colour is multiplied by alpha twice
        res[..., 3:] = sa + dst[..., 3:] * (1.0 - sa)
        out[win] = unorm8(res)
        covered[win] = True
    return out.astype(np.uint8), covered


def check(got_bgra, base_bgra, atlas, quads):
    """The device frame against the restatement: 1 LSB where text is, bit-identical elsewhere. Returns the restated
    frame and the covered mask."""
    want, covered = composite(base_bgra, atlas, quads)
    diff = np.abs(got_bgra.astype(np.int64) - want.astype(np.int64))
    assert int(diff.max()) <= 1, f"max |device - restatement| = {int(diff.max())} LSB at {np.argwhere(diff > 1)[:4].tolist()}"
    assert np.array_equal(got_bgra[~covered], base_bgra[~covered]), "a pixel no quad covers was written"
    return want, covered


# ---- layout (TextRenderer::RecordViewport, TextRenderer.cpp:144-193; DecodeUtf8 / ResolveGlyph :981-1065) ----

def decode_utf8(data):
    """The reference's decoder: a sequence cut short by the end of the string stops decoding; a bad lead byte or
    continuation skips one byte."""
    out, i, n = [], 0, len(data)
    while i < n:
        b = data[i]
        if b < 0x80:
            out.append(b)
            i += 1
            continue
        if b >> 5 == 0b110:
            need, cp = 1, b & 0x1F
        elif b >> 4 == 0b1110:
            need, cp = 2, b & 0x0F
        elif b >> 3 == 0b11110:
            need, cp = 3, b & 0x07
        else:
            i += 1
            continue
        if i + need >= n:
            break
        ok = True
        for k in range(1, need + 1):
            c = data[i + k]
            if c & 0xC0 != 0x80:
                ok = False
                break
            cp = (cp << 6) | (c & 0x3F)
        if not ok:
            i += 1
            continue
        out.append(cp)
        i += need + 1
    return out


def layout(glyphs, line_advance, text, position, color):
    """glyphs: {code point: (offset_x, offset_y, size_x, size_y, u0, v0, u1, v1, advance)} for 32..127, float32
    values. Returns float32 [n, 12] quads."""
    f = np.float32
    data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    pen_x, pen_y = f(position[0]), f(position[1])
    rows = []
    for cp in decode_utf8(data):
        if cp == 0x0A:
            pen_x = f(position[0])
            pen_y = f(pen_y + f(line_advance))
            continue
        g = glyphs.get(cp)
        if g is None:
            g = glyphs.get(ord("?"))
            if g is None:
                continue
        ox, oy, sx, sy, u0, v0, u1, v1, adv = (f(t) for t in g)
        x0, y0 = f(pen_x + ox), f(pen_y + oy)
        rows.append([x0, y0, f(x0 + sx), f(y0 + sy), u0, v0, u1, v1, *[f(c) for c in color]])
        pen_x = f(pen_x + adv)
    return np.asarray(rows, np.float32).reshape(-1, 12)
