"""The text overlay pass on the GPU through the C-ABI (tri_font, tri_set_text, tri_group_set_text): every rule of the
pass against the float64 restatement (tests/text_ref.py: 1 LSB where text is, bit-identical elsewhere), submission
order, more quads over one pixel than a scan round holds, row bands, text over geometry, tri_frame_alpha and the
argument checks."""
import ctypes as C

import numpy as np
import pytest

import scene_cases as sc
import text_ref
from text_ref import quad

pytestmark = pytest.mark.gpu

W, H = 96, 40
CLEAR = (0.2, 0.6, 0.4, 0.5)  # alpha 0.5: dst.a != 1


def atlas16():
    """A 16 x 16 gradient: every bilinear sample is non-trivial, the border texels differ from their neighbours."""
    j, i = np.mgrid[0:16, 0:16]
    return ((i * 13 + j * 29 + (i * j) % 7 * 5 + 40) % 256).astype(np.uint8)


def _scene(w=W, h=H):
    s = sc.empty_scene(w, h)
    s.clear = CLEAR
    return s


@pytest.fixture(scope="module")
def stage():
    """One 96 x 40 context over the cleared frame, its font, and the frame without text (shared, never modified)."""
    from trident_raster import raster, scenes

    atlas = atlas16()
    with raster.TriRaster(W, H) as r, raster.TriFont(atlas) as font:
        scenes.load_scene(r, _scene())
        r.render_frame()
        base, base_depth = r.readback()
        base.setflags(write=False)
        base_depth.setflags(write=False)
        yield r, font, atlas, base, base_depth
        r.set_text(None, None)


def _render(r, font, quads):
    r.set_text(font, np.asarray(quads, np.float32))
    r.render_frame()
    return r.readback()


RULE_CASES = {
    # corners at exact .5: X0 = 3.5 * 256 = px 3's centre (inclusive), X1 = px 7's centre (exclusive)
    "half_pixel_corners": [quad(3.5, 2.5, 7.5, 6.5, 0.1, 0.2, 0.8, 0.9, (1.0, 0.5, 0.25, 1.0))],
    "left_top_clipped": [quad(-9.25, -6.5, 14.75, 11.0, 0.0, 0.0, 1.0, 1.0, (0.9, 0.9, 0.1, 0.8))],
    "right_bottom_clipped": [quad(80.3, 30.2, 120.0, 55.9, 0.2, 0.1, 0.9, 0.7, (0.1, 0.9, 0.9, 0.9))],
    "mirrored": [quad(50.0, 30.0, 20.0, 5.0, 0.05, 0.1, 0.95, 0.8, (1.0, 1.0, 1.0, 1.0)),
                 quad(70.0, 4.0, 60.0, 20.0, 0.0, 0.0, 1.0, 1.0, (0.3, 0.2, 1.0, 0.7))],
    "zero_area": [quad(10.0, 10.0, 10.0, 30.0), quad(20.0, 12.0, 40.0, 12.0), quad(30.2, 5.1, 30.4, 5.3)],
    "clamped_colour": [quad(30.0, 8.0, 66.0, 36.0, 0.1, 0.1, 0.9, 0.9, (3.0, 1.5, -0.5, 0.5))],
    # the UV box touches the atlas border: the outer taps clamp to the edge texels
    "atlas_border": [quad(5.0, 3.0, 90.0, 38.0, 0.0, 0.0, 1.0, 1.0, (1.0, 1.0, 1.0, 1.0))],
    # one quad over several bins and strips, 33 px wide at an odd offset
    "several_bins": [quad(17.3, 1.2, 82.9, 39.6, 0.3, 0.3, 0.6, 0.7, (0.8, 0.4, 1.0, 0.9))],
}


@pytest.mark.parametrize("name", sorted(RULE_CASES))
def test_rule_cases(stage, name):
    r, font, atlas, base, base_depth = stage
    quads = RULE_CASES[name]
    got, depth = _render(r, font, quads)
    want, covered = text_ref.check(got, base, atlas, quads)
    assert np.array_equal(depth, base_depth)
    if name == "half_pixel_corners":
        assert covered[3, 3] and not covered[3, 7] and covered[2, 3] and not covered[6, 3] and covered[5, 6]
        assert int(covered.sum()) == 16
    if name == "zero_area":
        assert not covered.any() and np.array_equal(got, base)
    else:
        assert covered.any() and not np.array_equal(got, base)


def test_submission_order(stage):
    r, font, atlas, base, _ = stage
    a = quad(20.0, 6.0, 60.0, 30.0, 0.1, 0.1, 0.9, 0.9, (1.0, 0.1, 0.1, 0.9))
    b = quad(40.0, 14.0, 85.0, 37.0, 0.2, 0.0, 0.7, 1.0, (0.1, 0.2, 1.0, 0.8))
    ab, _ = _render(r, font, [a, b])
    ba, _ = _render(r, font, [b, a])
    text_ref.check(ab, base, atlas, [a, b])
    text_ref.check(ba, base, atlas, [b, a])
    assert not np.array_equal(ab, ba)


def test_more_quads_than_a_round_holds(stage):
    """More quads over one 8 x 8 pixel area than a scan chunk or a round's list holds; the area straddles the corner of
    four bins (and of their strips)."""
    from trident_raster import abi

    r, font, atlas, base, _ = stage
    n = max(abi.TRI_TEXT_LIST_CAP, abi.TRI_TEXT_SCAN_CHUNK) + 1
    assert n > abi.TRI_TEXT_LIST_CAP and n > abi.TRI_TEXT_SCAN_CHUNK
    c = abi.TRI_TEXT_BIN  # the corner (c, c)
    assert c + 4 <= min(W, H)
    quads = []
    for i in range(n):
        x0, y0 = c - 4 + (i % 3) * 0.75, c - 4 + (i % 5) * 0.5
        x1, y1 = c + 4 - (i % 4) * 0.5, c + 4 - (i % 2) * 1.25
        col = (1.0, 0.2, 0.1) if i % 2 == 0 else (0.1, 0.3, 1.0)
        quads.append(quad(x0, y0, x1, y1, 0.1, 0.1, 0.9, 0.9, (*col, 0.15 + 0.8 * ((i * 7) % 11) / 10.0)))
    got, _ = _render(r, font, quads)
    want, covered = text_ref.check(got, base, atlas, quads)
    assert covered[c - 1, c - 1] and covered[c, c] and covered[c - 1, c] and covered[c, c - 1]
    # the last quads decide the result: dropping the final one changes the restatement
    assert not np.array_equal(want, text_ref.composite(base, atlas, quads[:-1])[0])


BAND_QUADS = [quad(4.5, 3.0, 60.0, 30.0, 0.0, 0.1, 1.0, 0.9, (1.0, 0.8, 0.2, 0.9)),
              quad(30.0, 10.0, 93.0, 25.5, 0.2, 0.2, 0.7, 0.8, (0.2, 0.4, 1.0, 0.6)),
              quad(50.0, 15.0, 70.0, 39.0, 0.5, 0.0, 0.6, 1.0, (0.0, 1.0, 0.3, 1.0))]


def test_row_bands_under_bind_output(stage):
    """Bands [0, 17) and [17, 40) cut through the quads; each renders into caller-owned buffers."""
    import torch
    from trident_raster import raster, scenes

    r, font, atlas, base, _ = stage
    whole, _ = _render(r, font, BAND_QUADS)
    text_ref.check(whole, base, atlas, BAND_QUADS)
    parts = []
    for y0, y1 in ((0, 17), (17, H)):
        with raster.TriRaster(W, H, band=(y0, y1)) as b:
            col = torch.zeros((y1 - y0) * W, dtype=torch.int32, device="cuda:0")
            dep = torch.zeros((y1 - y0) * W, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            scenes.load_scene(b, _scene())
            b.bind_output(col.data_ptr(), dep.data_ptr())
            b.set_text(font, np.asarray(BAND_QUADS, np.float32))
            b.render_frame()
            parts.append(col.cpu().numpy().view(np.uint8).reshape(y1 - y0, W, 4))
            b.set_text(None, None)
    assert np.array_equal(np.concatenate(parts, axis=0), whole)


def test_group_forwards_text_to_every_band(stage):
    from trident_raster import raster, scenes

    r, font, atlas, base, _ = stage
    whole, _ = _render(r, font, BAND_QUADS)
    with raster.TriGroup(W, H, [0, 0]) as g:
        scenes.load_scene(g, _scene())
        g.set_text([font], np.asarray(BAND_QUADS, np.float32))
        g.render_frame()
        got, _ = g.readback(depth=False)
        assert np.array_equal(got, whole)
        g.set_text(None, None)
        g.render_frame()
        assert np.array_equal(g.readback(depth=False)[0], base)


def test_large_quads_share_one_list():
    """A few quads that fill a 1024 x 512 target: filed per bin they would need more than 8 references per quad + 1024,
    so every bin scans the one full list (the pass's second host layout). One of them reaches beyond 2^21 pixels,
    where the snap pins the coordinate."""
    from trident_raster import abi, raster, scenes

    w, h = 1024, 512
    atlas = atlas16()
    quads = [quad(-3.0e6, -40.0, 3.0e6, 300.5, 0.0, 0.0, 1.0, 1.0, (1.0, 0.4, 0.1, 0.5)),
             quad(0.0, 0.0, 1024.0, 512.0, 0.1, 0.1, 0.9, 0.9, (0.2, 1.0, 0.3, 0.4)),
             quad(1000.5, 500.25, 20.0, 10.0, 0.0, 1.0, 1.0, 0.0, (0.1, 0.2, 1.0, 0.6)),
             quad(300.0, 100.0, 340.0, 130.0, 0.2, 0.2, 0.8, 0.8, (1.0, 1.0, 1.0, 1.0)),
             quad(-50.0, 200.0, 1100.0, 600.0, 0.3, 0.0, 0.6, 1.0, (1.0, 1.0, 0.0, 0.3))]
    b = abi.TRI_TEXT_BIN
    filed = 0
    for q in quads:
        x0, x1 = sorted((max(min(q[0], w - 1), 0), max(min(q[2], w - 1), 0)))
        y0, y1 = sorted((max(min(q[1], h - 1), 0), max(min(q[3], h - 1), 0)))
        filed += (int(x1) // b - int(x0) // b + 1) * (int(y1) // b - int(y0) // b + 1)
    assert filed > 8 * len(quads) + 1024
    with raster.TriRaster(w, h) as r, raster.TriFont(atlas) as font:
        scenes.load_scene(r, _scene(w, h))
        r.render_frame()
        base, base_depth = r.readback()
        got, depth = _render(r, font, quads)
        want, covered = text_ref.check(got, base, atlas, quads)
        assert covered.all() and np.array_equal(depth, base_depth)
        assert not np.array_equal(want, text_ref.composite(base, atlas, quads[::-1])[0])  # order matters here too
        r.set_text(None, None)


def test_text_over_geometry():
    from trident_raster import raster, scenes

    atlas = atlas16()
    s = sc.c1_cube(0, 160, 120)
    quads = [quad(10.0, 30.0, 150.0, 62.0, 0.0, 0.0, 1.0, 1.0, (1.0, 1.0, 1.0, 1.0)),
             quad(60.5, 40.0, 100.5, 110.0, 0.1, 0.2, 0.9, 0.6, (1.0, 0.3, 0.1, 0.6))]
    with raster.TriRaster(160, 120) as r, raster.TriFont(atlas) as font:
        scenes.load_scene(r, s)
        r.render_frame()
        base, base_depth = r.readback()
        got, depth = _render(r, font, quads)
        _, covered = text_ref.check(got, base, atlas, quads)
        assert (base_depth[covered] != base_depth[0, 0]).any()  # the cube is there, under the quads
        assert np.array_equal(depth, base_depth)
        r.set_text(font, np.zeros((0, 12), np.float32))  # count 0
        r.render_frame()
        again, depth = r.readback()
        assert np.array_equal(again, base) and np.array_equal(depth, base_depth)


def test_frame_alpha_is_unproven_while_text_is_set(stage):
    r, font, atlas, base, _ = stage
    r.set_text(None, None)
    before = r.frame_alpha()
    assert before == int(base[0, 0, 3])  # the clear colour's alpha, proven uniform
    r.set_text(font, np.asarray(BAND_QUADS, np.float32))
    assert r.frame_alpha() == -1
    r.set_text(None, None)
    assert r.frame_alpha() == before


def test_invalid_arguments_keep_the_previous_text(stage, hiplib):
    import torch
    from trident_raster import abi, raster

    r, font, atlas, base, _ = stage
    want, _ = _render(r, font, BAND_QUADS)
    good = np.asarray(BAND_QUADS, np.float32)
    ptr = C.c_void_p(good.ctypes.data)
    call = hiplib.tri_set_text
    assert call(r._ctx, font._f, None, 3) == abi.TRI_E_INVALID
    assert call(r._ctx, font._f, ptr, abi.TRI_MAX_TEXT_QUADS + 1) == abi.TRI_E_INVALID
    for col, bad in ((0, np.nan), (3, np.inf), (5, -np.inf), (6, np.nan)):
        q = good.copy()
        q[1, col] = bad
        assert call(r._ctx, font._f, C.c_void_p(q.ctypes.data), 3) == abi.TRI_E_INVALID, (col, bad)
        assert hiplib.tri_last_error()
    assert call(None, font._f, ptr, 3) == abi.TRI_E_INVALID
    if torch.cuda.device_count() > 1:  # a font on another device
        with raster.TriFont(atlas, device=1) as other:
            assert call(r._ctx, other._f, ptr, 3) == abi.TRI_E_INVALID
    f = C.c_void_p()
    assert hiplib.tri_font_create(-1, None, 16, 16, C.byref(f)) == abi.TRI_E_INVALID
    assert hiplib.tri_font_create(-1, C.c_void_p(atlas.ctypes.data), 0, 16, C.byref(f)) == abi.TRI_E_INVALID
    assert hiplib.tri_font_destroy(None) == abi.TRI_OK
    r.render_frame()
    assert np.array_equal(r.readback()[0], want)
