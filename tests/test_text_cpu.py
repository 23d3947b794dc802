"""CPU tests of the text overlay's host side: the C-ABI additions (layout, constants, symbols), the TrueType reader and
atlas baker of Trident::TextRenderer against values read independently with fontTools from the fixture font, the layout
rule against its restatement (tests/text_ref.py), and the stand-alone sanitizer check of the reader."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import text_ref
from trident_raster import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FONT = os.path.join(ROOT, "tests", "golden", "fonts", "JetBrainsMono-Regular.ttf")
PX = 32.0
ATLAS = 1024
CODEPOINTS = range(32, 128)


# ---- ABI ------------------------------------------------------------------------------------------------------

def _define(path, name):
    m = re.search(rf"^#define\s+{name}\s+(\d+)u?\b", open(path).read(), flags=re.M)
    assert m, (path, name)
    return int(m.group(1))


def test_text_quad_layout_and_constants(tmp_path):
    header = os.path.join(ROOT, "include", "tri_raster.h")
    launch = os.path.join(ROOT, "3d-renderer_amd", "csrc", "raster_launch.h")
    assert C.sizeof(abi.TriTextQuad) == 48 and abi.TEXT_QUAD_DTYPE.itemsize == 48
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void){",
             'printf("size %zu\\n", sizeof(tri_text_quad));']
    for fname, _ in abi.TriTextQuad._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(tri_text_quad, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "quad.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "quad"), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "quad")], capture_output=True, text=True,
                                                 check=True).stdout.strip().splitlines())
    assert int(out["size"]) == 48
    for fname, _ in abi.TriTextQuad._fields_:
        assert int(out[fname]) == getattr(abi.TriTextQuad, fname).offset, fname
    assert _define(header, "TRI_MAX_TEXT_QUADS") == abi.TRI_MAX_TEXT_QUADS == 65536
    assert _define(launch, "TRI_TEXT_SCAN_CHUNK") == abi.TRI_TEXT_SCAN_CHUNK
    assert _define(launch, "TRI_TEXT_LIST_CAP") == abi.TRI_TEXT_LIST_CAP
    assert _define(launch, "TRI_TEXT_BIN") == abi.TRI_TEXT_BIN


def test_new_symbols_are_exported(hiplib):
    from trident_raster import app

    out = subprocess.run(["nm", "-D", "--defined-only", hiplib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (tri_\w+)", out))
    assert {"tri_font_create", "tri_font_destroy", "tri_set_text", "tri_group_set_text"} <= exported
    assert hiplib.tri_abi_version() == 2  # the additions are additive
    shim = app.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", shim._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (trident_\w+)", out))
    assert {"trident_app_submit_text", "trident_app_set_font", "trident_font_create", "trident_font_destroy",
            "trident_font_load", "trident_font_load_memory", "trident_font_atlas", "trident_font_glyph",
            "trident_font_metrics", "trident_font_layout"} <= exported


def test_set_text_rejects_null_context(hiplib):
    assert hiplib.tri_set_text(None, None, None, 0) == abi.TRI_E_INVALID
    assert hiplib.tri_group_set_text(None, None, None, 0) == abi.TRI_E_INVALID
    assert hiplib.tri_font_destroy(None) == abi.TRI_OK


# ---- the font -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def font():
    from trident_raster import app

    return app.Font(FONT, PX)


@pytest.fixture(scope="module")
def baked(font):
    """The atlas and the 96 glyph rows, read once."""
    atlas = font.atlas()
    atlas.setflags(write=False)
    glyphs = {cp: font.glyph(cp) for cp in CODEPOINTS}
    return atlas, glyphs


@pytest.fixture(scope="module")
def tt():
    from fontTools.ttLib import TTFont

    return TTFont(FONT)


def _glyph_name(tt, cp):
    return tt.getBestCmap().get(cp, tt.getGlyphOrder()[0])  # no cmap entry: glyph 0


def _box(g):
    """The glyph's atlas box in texels: x0, y0, x1, y1 (exclusive)."""
    b = g[4:8] * ATLAS
    assert np.array_equal(b, np.round(b))
    return tuple(int(v) for v in b)


def test_metrics_against_fonttools(font, baked, tt):
    hhea = tt["hhea"]
    s = PX / (hhea.ascent - hhea.descent)
    line, scale, px = font.metrics()
    assert px == PX
    assert scale == np.float32(s)
    assert abs(line - (hhea.ascent - hhea.descent + hhea.lineGap) * s) <= 4e-6 * 32.0  # float32 product
    assert abs(line - 32.0) <= 4e-6 * 32.0  # the fixture's line gap is 0
    _, glyphs = baked
    for cp in CODEPOINTS:
        adv = tt["hmtx"][_glyph_name(tt, cp)][0]
        assert glyphs[cp][8] == np.float32(scale * np.float32(adv)), cp
        assert adv == 600 and abs(glyphs[cp][8] - 14.5454545) < 1e-5  # monospace


def test_glyph_boxes_follow_the_packer_rule(baked, tt):
    """ix0 = floor(xmin S) ... with S = 2 s; offset = i0 / 2 - 0.25, size = box / 2, uv = box corners / 1024."""
    _, glyphs = baked
    hhea = tt["hhea"]
    S = 2.0 * float(np.float32(PX / (hhea.ascent - hhea.descent)))
    glyf = tt["glyf"]
    for cp in CODEPOINTS:
        g = glyf[_glyph_name(tt, cp)]
        if g.numberOfContours == 0:
            ix0 = iy0 = ix1 = iy1 = 0
        else:
            ix0, iy0 = int(np.floor(g.xMin * S)), int(np.floor(-g.yMax * S))
            ix1, iy1 = int(np.ceil(g.xMax * S)), int(np.ceil(-g.yMin * S))
        x0, y0, x1, y1 = _box(glyphs[cp])
        assert (x1 - x0, y1 - y0) == (ix1 - ix0 + 1, iy1 - iy0 + 1), cp
        assert tuple(glyphs[cp][0:2]) == (ix0 * 0.5 - 0.25, iy0 * 0.5 - 0.25), cp
        assert tuple(glyphs[cp][2:4]) == ((x1 - x0) * 0.5, (y1 - y0) * 0.5), cp


def test_atlas_boxes_are_disjoint_and_padded(baked):
    atlas, glyphs = baked
    assert atlas.shape == (ATLAS, ATLAS)
    boxes = [_box(glyphs[cp]) for cp in CODEPOINTS]
    assert len(set(boxes)) == 96
    used = np.zeros((ATLAS, ATLAS), bool)
    for x0, y0, x1, y1 in boxes:
        assert 0 <= x0 < x1 <= ATLAS and 0 <= y0 < y1 <= ATLAS
        # the box grown by one texel touches no earlier box: at least 1 texel apart
        assert not used[max(y0 - 1, 0):y1 + 1, max(x0 - 1, 0):x1 + 1].any()
        used[y0:y1, x0:x1] = True
    assert not atlas[~used].any()  # nothing outside the boxes


def _flat_contours(glyph_set, name, tol):
    """The glyph's contours (composites resolved by the glyph set) as closed polylines in font units, quadratics cut
    into chords within `tol` font units of the curve (deviation of n chords: |p0 - 2 p1 + p2| / (4 n^2))."""
    from fontTools.pens.basePen import BasePen

    class Flatten(BasePen):
        def __init__(self, gs):
            super().__init__(gs)
            self.contours = []

        def _moveTo(self, pt):
            self.contours.append([pt])

        def _lineTo(self, pt):
            self.contours[-1].append(pt)

        def _qCurveToOne(self, p1, p2):
            p0 = self.contours[-1][-1]
            dev = np.hypot(p0[0] - 2 * p1[0] + p2[0], p0[1] - 2 * p1[1] + p2[1])
            n = max(1, int(np.ceil(np.sqrt(dev / (4.0 * tol)))))
            for i in range(1, n + 1):
                t = i / n
                self.contours[-1].append(((1 - t) ** 2 * p0[0] + 2 * (1 - t) * t * p1[0] + t * t * p2[0],
                                          (1 - t) ** 2 * p0[1] + 2 * (1 - t) * t * p1[1] + t * t * p2[1]))

        def _curveToOne(self, p1, p2, p3):
            raise AssertionError("a TrueType outline has no cubics")

    pen = Flatten(glyph_set)
    glyph_set[name].draw(pen)
    return [np.asarray(c, np.float64) for c in pen.contours if len(c) >= 3]


def _nonzero_area(contours):
    """The exact area of the set of points with a non-zero winding number about closed polylines. Between two
    consecutive event heights (vertex heights and the heights where two edges cross) no edges cross, so the filled
    set of a slab is a union of trapezoids between edges that are neighbours in x. For contours that do not overlap
    it is the sum of the signed areas; where two contours overlap (the fixture's 8 is two overlapping loops) the
    overlap counts once, as a non-zero fill paints it."""
    seg = np.concatenate([np.concatenate([c, np.roll(c, -1, axis=0)], axis=1) for c in contours])
    seg = seg[seg[:, 1] != seg[:, 3]]
    x0, y0, x1, y1 = seg.T
    direction = np.sign(y1 - y0)
    # proper crossings of every edge pair: p + t r = q + u s
    rx, ry = x1 - x0, y1 - y0
    den = rx[:, None] * ry[None, :] - ry[:, None] * rx[None, :]
    qpx, qpy = x0[None, :] - x0[:, None], y0[None, :] - y0[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (qpx * ry[None, :] - qpy * rx[None, :]) / den
        u = (qpx * ry[:, None] - qpy * rx[:, None]) / den
    cross = (den != 0) & (t > 1e-12) & (t < 1 - 1e-12) & (u > 1e-12) & (u < 1 - 1e-12)
    ys = np.unique(np.concatenate([y0, y1, (y0[:, None] + t * ry[:, None])[cross]]))
    ya, yb = ys[:-1], ys[1:]
    ym = 0.5 * (ya + yb)
    lo, hi = np.minimum(y0, y1), np.maximum(y0, y1)
    active = (lo[None, :] <= ya[:, None]) & (hi[None, :] >= yb[:, None])  # slab x edge
    slope = rx / ry

    def xat(y):
        return np.where(active, x0[None, :] + (y[:, None] - y0[None, :]) * slope[None, :], np.inf)

    order = np.argsort(xat(ym), axis=1, kind="stable")
    xa, xb = np.take_along_axis(xat(ya), order, 1), np.take_along_axis(xat(yb), order, 1)
    wind = np.cumsum(np.take_along_axis(np.where(active, direction[None, :], 0.0), order, 1), axis=1)
    inside = (wind[:, :-1] != 0) & np.isfinite(xa[:, 1:]) & np.isfinite(xb[:, 1:])
    with np.errstate(invalid="ignore"):
        width = 0.5 * ((xa[:, 1:] - xa[:, :-1]) + (xb[:, 1:] - xb[:, :-1]))
    return float((np.where(inside, width, 0.0) * (yb - ya)[:, None]).sum())


def test_coverage_equals_the_outline_area(baked, tt):
    """Sum(coverage) / 255 / 4 (2 x 2 oversampling) = the outline's analytic area * s^2. The area is that of the
    non-zero fill of the outline fontTools draws (composites resolved; _nonzero_area: equal to fontTools' AreaPen for
    the glyphs whose contours do not overlap, smaller for the others, such as the fixture's 8). The margin is derived from the baker's own
    steps, for a box of w x h raster texels inside its (w + 1) x (h + 1) atlas box:
      - flattening: chords within 0.01 texel of the curve (the reference polygon here: 0.001 texel), so the area changes
        by at most 0.011 * perimeter texel^2;
      - the coverage byte: round(c * 255) is off by at most 0.5 per raster texel -> 0.5 * w * h;
      - the two truncating 2-tap means keep the sum (every input goes half to each of two outputs, and the box has
        the extra column / row to receive them) but for the truncation, at most 0.5 per output texel and pass
        -> 1.0 * (w + 1) * (h + 1).
    In pixel^2: (0.5 w h + (w + 1)(h + 1)) / 255 / 4 + 0.011 * perimeter_texels / 4."""
    from fontTools.pens.areaPen import AreaPen
    from fontTools.pens.perimeterPen import PerimeterPen

    atlas, glyphs = baked
    gs = tt.getGlyphSet()
    hhea = tt["hhea"]
    s = float(np.float32(PX / (hhea.ascent - hhea.descent)))
    worst, overlapping = 0.0, []
    for cp in CODEPOINTS:
        name = _glyph_name(tt, cp)
        area_pen, per_pen = AreaPen(gs), PerimeterPen(gs)
        gs[name].draw(area_pen)
        gs[name].draw(per_pen)
        contours = _flat_contours(gs, name, 0.001 / (2.0 * s))
        units = _nonzero_area(contours) if contours else 0.0
        if abs(units - abs(area_pen.value)) > 1e-3 * max(units, 1.0):
            overlapping.append(name)  # its signed areas count an overlap twice
            assert units < abs(area_pen.value)
        want = units * s * s
        x0, y0, x1, y1 = _box(glyphs[cp])
        got = float(atlas[y0:y1, x0:x1].astype(np.int64).sum()) / 255.0 / 4.0
        w, h = x1 - x0 - 1, y1 - y0 - 1
        margin = (0.5 * w * h + (w + 1) * (h + 1)) / 255.0 / 4.0 + 0.011 * per_pen.value * 2.0 * s / 4.0
        print(f"cp {cp} {name}: area {want:.3f} px^2, baked {got:.3f}, margin {margin:.3f}")
        assert abs(got - want) <= margin, (cp, name, got, want, margin)
        if want > 0:
            worst = max(worst, abs(got - want) / margin)
    print("largest |difference| / margin:", worst, "overlapping contours:", overlapping)
    assert "eight" in overlapping and "o" not in overlapping  # two overlapping loops; one ring
    x0, y0, x1, y1 = _box(glyphs[32])
    assert not atlas[y0:y1, x0:x1].any() and glyphs[32][8] > 0  # space: no coverage, an advance


def _blobs(mask):
    """8-connected components of a small boolean image."""
    mask = mask.copy()
    n = 0
    for y, x in zip(*np.nonzero(mask)):
        if not mask[y, x]:
            continue
        n += 1
        stack = [(y, x)]
        mask[y, x] = False
        while stack:
            cy, cx = stack.pop()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < mask.shape[0] and 0 <= nx < mask.shape[1] and mask[ny, nx]:
                        mask[ny, nx] = False
                        stack.append((ny, nx))
    return n


def test_composites_fallback_and_missing_glyph(font, baked, tt):
    atlas, glyphs = baked
    glyf = tt["glyf"]
    assert glyf[_glyph_name(tt, ord("i"))].isComposite()  # the fixture's i is a composite: stem + dot
    x0, y0, x1, y1 = _box(glyphs[ord("i")])
    assert _blobs(atlas[y0:y1, x0:x1] > 0) == 2
    assert _blobs(atlas[slice(*_box(glyphs[ord("l")])[1::2]), slice(*_box(glyphs[ord("l")])[0::2])] > 0) == 1
    # code point 127 has no cmap entry: glyph 0, baked like any other (its own box, glyph 0's extent)
    assert 127 not in tt.getBestCmap()
    g0 = glyf[tt.getGlyphOrder()[0]]
    S = 2.0 * float(np.float32(PX / (tt["hhea"].ascent - tt["hhea"].descent)))
    x0, y0, x1, y1 = _box(glyphs[127])
    assert x1 - x0 == int(np.ceil(g0.xMax * S)) - int(np.floor(g0.xMin * S)) + 1
    assert atlas[y0:y1, x0:x1].any()
    # outside 32..127: the '?' fallback
    assert np.array_equal(font.glyph(0xE9), glyphs[ord("?")])
    assert np.array_equal(font.glyph(0x1F600), glyphs[ord("?")])
    assert not np.array_equal(glyphs[ord("?")], glyphs[ord("A")])


def test_malformed_fonts_are_refused():
    from trident_raster import app

    data = open(FONT, "rb").read()
    f = app.Font()
    assert not f.load(FONT + ".missing")
    for cut in (0, 11, 200, len(data) // 2):
        assert not f.load_memory(data[:cut]), cut
    assert not f.load_memory(b"\x00\x01\x00\x00" + b"\xff" * 400)
    assert f.load_memory(data) and f.atlas().any()
    assert not f.load_memory(data[:1000]) and f.atlas().any()  # a failed load keeps the font


# ---- layout ---------------------------------------------------------------------------------------------------

def _table(baked):
    return {cp: tuple(g) for cp, g in baked[1].items()}


def test_layout_matches_the_restated_rule(font, baked):
    color = (0.25, 0.5, 0.75, 1.0)
    got = font.layout("FPS: 60.0\nab", (10.0, 30.0), color)
    want = text_ref.layout(_table(baked), font.metrics()[0], "FPS: 60.0\nab", (10.0, 30.0), color)
    assert got.shape == (11, 12)  # the newline emits no quad
    assert np.array_equal(got, want)
    # the second line starts at the position's x again, one line advance lower
    a_row = baked[1][ord("a")]
    assert got[9, 0] == np.float32(np.float32(10.0) + a_row[0])
    assert got[9, 1] == np.float32(np.float32(np.float32(30.0) + font.metrics()[0]) + a_row[1])


def test_utf8_decoding_follows_the_reference(font, baked):
    table, line = _table(baked), font.metrics()[0]
    cases = {
        b"ab\xe2\x82": "ab",         # a 3-byte sequence cut short by the end stops decoding
        b"ab\xc3": "ab",             # likewise a 2-byte one
        b"a\xc3(b": "a(b",           # an invalid continuation skips one byte
        b"a\x80\xbfb": "ab",         # stray continuations are skipped
        "hé!".encode(): "h?!",  # U+00E9 is outside the table: the fallback
        b"": "",
    }
    for raw, same_as in cases.items():
        got = font.layout(raw, (3.0, 40.0))
        assert np.array_equal(got, text_ref.layout(table, line, raw, (3.0, 40.0), (1, 1, 1, 1))), raw
        assert np.array_equal(got, font.layout(same_as, (3.0, 40.0))), raw
    assert font.layout("", (0.0, 0.0)).shape == (0, 12)  # an empty string queues nothing


# ---- the sanitizer check --------------------------------------------------------------------------------------

def test_make_font_check():
    """The reader over the fixture and damaged copies of it, as a stand-alone program under the address and
    undefined-behaviour sanitizers (nothing is loaded into Python)."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "3d-renderer_amd"), "font-check", f"FONT={FONT}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "text_font_check: ok" in r.stdout
