"""The recording tests' yardstick: the reference's RGBA -> YUV 4:4:4 conversion (VideoEncoder.cpp:701-736) restated
in numpy float64, whose elementwise multiplies and adds are the same IEEE double operations in the same order.
Per pixel: Y = 0.299 R + 0.587 G + 0.114 B, U = -0.169 R - 0.331 G + 0.5 B + 128, V = 0.5 R - 0.419 G - 0.081 B + 128,
each evaluated left to right, clamped to [0, 255] and truncated to a byte."""
import functools

import numpy as np


def yuv444(rgb):
    """uint8 [..., >= 3] (R, G, B first; anything after is ignored) -> uint8 [3, ...]: the Y, U and V planes."""
    rgb = np.asarray(rgb)
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    u = -0.169 * r - 0.331 * g + 0.5 * b + 128.0
    v = 0.5 * r - 0.419 * g - 0.081 * b + 128.0
    return np.stack([np.clip(p, 0.0, 255.0).astype(np.uint8) for p in (y, u, v)])  # astype truncates toward zero


@functools.lru_cache(maxsize=1)
def all_triples():
    """Every RGB triple once, row i = (i >> 16, (i >> 8) & 255, i & 255), and its planes [3, 2^24]. Computed once
    and shared; callers must not write to either array."""
    i = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(i >> 16).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8)], axis=1)
    yuv = np.empty((3, 1 << 24), np.uint8)
    step = 1 << 20  # (bounds the float64 temporaries)
    for s in range(0, 1 << 24, step):
        yuv[:, s:s + step] = yuv444(rgb[s:s + step])
    rgb.setflags(write=False)
    yuv.setflags(write=False)
    return rgb, yuv


def y4m_header(width, height, fps):
    return b"YUV4MPEG2 W%d H%d F%d:1 Ip A0:0 C444\n" % (width, height, fps)


def y4m_file(width, height, fps, frames_rgb):
    """The bytes of a Y4M C444 file holding `frames_rgb` (each uint8 [height, width, >= 3], RGB first)."""
    out = [y4m_header(width, height, fps)]
    for f in frames_rgb:
        assert f.shape[:2] == (height, width)
        out += [b"FRAME\n", yuv444(f).tobytes()]
    return b"".join(out)
