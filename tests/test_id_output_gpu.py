"""GPU tests of the entity-id pass (include/tri_raster.h "entity ids"): k_id_raster at every bin size and on every
primitive -> draw route, the readers, tri_pick, tri_pick_rect and the selection outline.

The bar: device depth == the oracle's D (the project's standing bit-exact parity) and ids == tests/id_ref.py's
expected ids EVERYWHERE — zero mismatches allowed: both sides are decided by the same depth bits. Every case asserts the
bin grid (and, where the case is about a route, the path bits) so that a scene landing on another path fails rather than
passing there. The scenes are the smallest at which each path can still go wrong: 100 x 70 has a partial last bin
column and row at 16 and 32 px; 4100 x 4100 is the smallest 64-px grid with both (tests/test_raster_paths_gpu.py BIG).
"""
import os
import re

import numpy as np
import pytest

import id_ref
import scene_cases as sc
from test_raster_paths_gpu import BIG, OVF_BIN_LIST, expect_overflow

pytestmark = pytest.mark.gpu

RASTER_BIN_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-renderer_amd", "csrc",
                            "raster_bin.h")  # kBigQueue: the large-triangle queue k_id_raster shares with the raster
_REF = {}


def reference(oracle, scene, band=None):
    """(oracle colour, D, expected ids) of a scene, computed once, shared and never modified."""
    key = (scene.name, scene.width, scene.height, band)
    if key not in _REF:
        if len(_REF) >= 3:
            _REF.pop(next(iter(_REF)))
        col, dep, _ = oracle.render(scene, band=band)
        ids, _ = id_ref.expected_ids(oracle, scene, band=band, full_depth=dep)
        for a in (col, dep, ids):
            a.setflags(write=False)
        _REF[key] = (col, dep, ids)
    return _REF[key]


def compare(tag, r, ref, bin_size, path=0, not_path=0, min_ids=2):
    col, dep, ids = ref
    _, gdep = r.readback()
    gids = r.read_ids()
    st = r.frame_stats()
    bad_d, bad_i = int((gdep != dep).sum()), int((gids != ids).sum())
    print(f"IDS {tag}: bin_size {st['bin_size']} path {st['path']:#x} clipped {st['triangles_clipped']} "
          f"depth mismatches {bad_d} id mismatches {bad_i} distinct {np.unique(ids).tolist()[:8]}")
    assert st["bin_size"] == bin_size, (tag, st)
    assert st["path"] & path == path and st["path"] & not_path == 0, (tag, hex(st["path"]))
    assert bad_d == 0, f"{tag}: {bad_d} depth mismatches"
    assert bad_i == 0, f"{tag}: {bad_i} id mismatches"
    assert len(np.unique(ids)) >= min_ids, tag  # (the case shows more than background)
    return gids


def render_ids(oracle, scene, bin_size, band=None, flags=0, **kw):
    from trident_raster import raster, scenes

    rows = (band[1] - band[0]) if band else scene.height
    if bin_size is None:  # (a case about something else than the grid: whichever the rule gives)
        bin_size = sc.expected_bin_size(scene.width, rows, scene.height, id_ref.triangles(scene))
    assert sc.expected_bin_size(scene.width, rows, scene.height, id_ref.triangles(scene)) == bin_size
    ref = reference(oracle, scene, band)
    with raster.TriRaster(scene.width, scene.height, band=band, flags=flags) as r:
        scenes.load_scene(r, scene)
        r.set_id_output(True)
        r.render_frame()
        gids = compare(scene.name, r, ref, bin_size, **kw)
        img = r.id_image()
        assert (img.width, img.height, img.pitch_bytes, img.format) == (scene.width, rows, scene.width * 4, 98)
        assert img.device_ptr
    return gids


# ---- k_id_raster at each bin size ---------------------------------------------------------------------------------
def test_ids_at_16_px_bins(oracle):
    """100 x 70, two cubes and a quad: sparse, so 16-px bins with a 4-px last column and a 6-px last row."""
    from trident_raster import abi

    render_ids(oracle, id_ref.cubes_and_quad(), 16, path=abi.TRI_PATH_IDX_ROUTE, min_ids=4)


def test_ids_at_32_px_bins(oracle):
    """100 x 70 with a 768-triangle sphere and a quad: 0.11 triangles per pixel, 32-px bins."""
    render_ids(oracle, id_ref.sphere_and_quad(), 32, min_ids=3)


def test_ids_at_64_px_bins(oracle):
    """4100 x 4100 with two draws: 65 x 65 bins of 64 px whose last column and row are 4 px wide."""
    render_ids(oracle, sc.textured_two_draws(BIG, BIG), 64, min_ids=3)


# ---- the three primitive -> draw routes ---------------------------------------------------------------------------
@pytest.mark.parametrize("textured", [False, True])
def test_ids_of_a_single_draw(oracle, textured):
    """fp.one_draw: every id is 0 or 1, on the solid instantiation's frames and on a textured draw's."""
    from trident_raster import abi, scenes

    if textured:
        s = sc.textured_grid(100, 70, 20)
        s.skybox = None
        s.name = "id_textured_grid"
    else:
        s = scenes.scene_c1_cube(1, 100, 70, skybox="solid")
        s.name = "id_c1_cube"
    # (TRI_PATH_ONE_DRAW names the solid single-draw instantiation; a textured draw is shaded by the generic one, and
    # both frames carry fp.one_draw)
    gids = render_ids(oracle, s, None, path=0 if textured else abi.TRI_PATH_ONE_DRAW,
                      not_path=abi.TRI_PATH_ONE_DRAW if textured else 0)
    assert set(np.unique(gids)) == {0, 1}


def test_ids_without_the_index_route(oracle):
    """Three draws of one mesh (coincident quads among them): prim_vs records carry the draw."""
    from trident_raster import abi

    render_ids(oracle, id_ref.shared_mesh(), 16, not_path=abi.TRI_PATH_IDX_ROUTE | abi.TRI_PATH_ONE_DRAW, min_ids=3)


def test_ids_with_the_shadow_prepass(oracle):
    """The pre-pass's frames keep the index route off and run k_shadow_raster ahead of the id pass."""
    from trident_raster import abi

    render_ids(oracle, sc.shadow_scene(oracle, 120, 80, size=256), None, path=abi.TRI_PATH_SHADOW,
               not_path=abi.TRI_PATH_IDX_ROUTE, min_ids=4)


@pytest.mark.parametrize("form", ["single", "multi"])
def test_ids_across_the_near_plane(oracle, form):
    """Clipped pieces carry their parent's draw: the ground plane through the near plane, as one draw and as two."""
    from trident_raster import raster, scenes

    s = sc.near_clip_grid(160, 120, 30) if form == "single" else sc.near_clip_multi(160, 120, 30)
    s.name = f"id_near_clip_{form}"
    ref = reference(oracle, s)
    with raster.TriRaster(s.width, s.height) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.render_frame()
        compare(s.name, r, ref, sc.expected_bin_size(160, 120, 120, s.triangles), min_ids=2 if form == "single" else 3)
        assert r.frame_stats()["triangles_clipped"] > 0


# ---- large triangles ----------------------------------------------------------------------------------------------
def test_ids_of_full_frame_quads(oracle):
    """Two quads larger than the frame: every bin's entries go through the cooperative large-triangle loop."""
    render_ids(oracle, sc.large_quads(100, 70), 16, min_ids=2)


def test_ids_with_an_overfull_large_triangle_queue(oracle):
    """600 coincident quads as 600 draws over all four 32-px bins of a 64 x 48 frame: 1200 large triangles per bin,
    more than the 1024 the LDS queue holds, so the rest are walked per lane. The last draw owns every covered pixel."""
    from trident_raster import raster, scenes

    w, h, n = 64, 48, 600
    big_queue = int(re.search(r"constexpr int kBigQueue = (\d+);", open(RASTER_BIN_H).read()).group(1))
    assert 2 * n > big_queue, "the case needs more large triangles per bin than raster_bin.h's kBigQueue holds"
    rects = [(8, 8, 56, 40, 0.5)] * n
    s = id_ref.pixel_quads("id_coincident_600", w, h, rects)
    assert sc.expected_bin_size(w, h, h, s.triangles) == 32
    want = id_ref.ids_of_rects(w, h, rects)
    assert set(np.unique(want)) == {0, n}
    _, dep, _ = oracle.render(s)
    with raster.TriRaster(w, h) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.render_frame()  # (re-renders if the bins' first capacity is below 1200 entries)
        compare(s.name, r, (None, dep, want), 32)


# ---- draw lists, bands, groups ------------------------------------------------------------------------------------
def test_ids_count_the_callers_draws_over_a_skipped_one(oracle):
    gids = render_ids(oracle, id_ref.with_skipped_draw(id_ref.cubes_and_quad()), 16, min_ids=4)
    assert set(np.unique(gids)) == {0, 1, 3, 4}


def test_ids_of_a_row_band(oracle):
    """Rows [13, 57): 44 rows, no multiple of the 16-px bin."""
    render_ids(oracle, id_ref.cubes_and_quad(), 16, band=(13, 57), min_ids=4)


def test_ids_of_a_two_band_group(oracle):
    from trident_raster import abi, raster, scenes

    s = id_ref.cubes_and_quad()
    _, dep, ids = reference(oracle, s)
    with raster.TriGroup(s.width, s.height, [0, 0]) as g:
        scenes.load_scene(g, s)
        with pytest.raises(raster.TriError) as ei:
            g.read_ids()
        assert ei.value.code == abi.TRI_E_STATE
        g.set_id_output(True)
        g.render_frame()
        _, gdep = g.readback()
        gids = g.read_ids()
        assert np.array_equal(gdep, dep)
        assert int((gids != ids).sum()) == 0
        for x, y in [(0, 0), (99, 69), (50, 34), (50, 35), (30, 20), (70, 50)]:  # (rows 34 | 35: the band seam)
            assert g.pick(x, y) == (int(ids[y, x]), int(dep[y, x])), (x, y)
        with pytest.raises(raster.TriError) as ei:
            g.pick(10, 70)
        assert ei.value.code == abi.TRI_E_INVALID


def test_ids_after_a_bin_overflow(oracle):
    """2200 large triangles in one bin, three draws: TRI_E_OVERFLOW first, the right ids after the re-render."""
    from trident_raster import raster, scenes

    s = sc.stacked_quads(200, 120, draws=3, textured=True)
    ref = reference(oracle, s)
    with raster.TriRaster(s.width, s.height) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        expect_overflow(r, OVF_BIN_LIST)
        r.render_frame()
        compare(s.name, r, ref, 32, min_ids=2)


# ---- the id output leaves the frame alone -------------------------------------------------------------------------
def test_id_output_changes_neither_colour_nor_depth(oracle):
    from trident_raster import abi, raster, scenes

    s = id_ref.cubes_and_quad()
    _, dep, ids = reference(oracle, s)
    with raster.TriRaster(s.width, s.height) as r, raster.TriFont(np.full((8, 8), 255, np.uint8)) as font:
        scenes.load_scene(r, s)
        r.render_frame()
        col0, dep0 = r.readback()
        for reader in (r.read_ids, r.id_image, lambda: r.pick(1, 1), lambda: r.pick_rect(0, 0, 5, 5, 3)):
            with pytest.raises(raster.TriError) as ei:
                reader()
            assert ei.value.code == abi.TRI_E_STATE
        r.set_id_output(True)
        with pytest.raises(raster.TriError) as ei:  # on, but no frame yet
            r.read_ids()
        assert ei.value.code == abi.TRI_E_STATE
        r.render_frame()
        col1, dep1 = r.readback()
        assert np.array_equal(col0, col1) and np.array_equal(dep0, dep1) and np.array_equal(dep1, dep)
        assert np.array_equal(r.read_ids(), ids)
        # text over the frame: another colour, the same ids
        r.set_text(font, np.asarray([[20, 10, 80, 60, 0, 0, 1, 1, 0.2, 1.0, 0.3, 1.0]], np.float32))
        r.render_frame()
        col2, dep2 = r.readback()
        assert not np.array_equal(col2, col0) and np.array_equal(dep2, dep0)
        assert np.array_equal(r.read_ids(), ids)
        r.set_text(None, None)
        r.set_id_output(False)
        r.render_frame()
        col3, dep3 = r.readback()
        assert np.array_equal(col3, col0) and np.array_equal(dep3, dep0)
        with pytest.raises(raster.TriError) as ei:
            r.read_ids()
        assert ei.value.code == abi.TRI_E_STATE


def test_id_pass_is_timed_by_events_of_its_own(oracle):
    """tri_set_timing stamps k_id_raster on both sides: tri_get_id_timing reports it for exactly the timed frames that
    ran it, and nothing with the output off."""
    from trident_raster import raster, scenes

    s = id_ref.sphere_and_quad()
    with raster.TriRaster(s.width, s.height) as r:
        scenes.load_scene(r, s)
        r.render_frame()
        r.set_timing(True)
        for _ in range(4):
            r.render()
        assert r.timing()["frames"] == 4 and r.id_timing() == (0.0, 0)
        r.set_id_output(True)
        r.render_frame()
        r.set_timing(True)  # (restarts the sums)
        for _ in range(5):
            r.render()
        t = r.timing()
        ms_id, frames = r.id_timing()
        print(f"IDS timing: {1e3 * ms_id / 5:.1f} us per frame in k_id_raster, stages {t}")
        assert t["frames"] == 5 and frames == 5
        assert 0.0 < ms_id < t["ms_frame"] and t["ms_setup"] >= 0.0
        r.set_timing(False)


def test_frame_without_primitives_has_no_ids():
    from trident_raster import raster, scenes

    s = sc.empty_scene(100, 70)
    with raster.TriRaster(s.width, s.height) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.render_frame()
        assert not r.read_ids().any()
        assert r.pick(99, 69)[0] == 0 and r.pick_rect(0, 0, 99, 69, 0) == []


# ---- tri_pick, tri_pick_rect --------------------------------------------------------------------------------------
def test_pick_equals_the_buffers(oracle):
    from trident_raster import abi, raster, scenes

    s = id_ref.cubes_and_quad()
    _, dep, ids = reference(oracle, s)
    w, h = s.width, s.height
    pixels = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (50, 35), (30, 30), (64, 40), (15, 16), (48, 47)]
    with raster.TriRaster(w, h) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.render_frame()
        for x, y in pixels:
            assert r.pick(x, y) == (int(ids[y, x]), int(dep[y, x])), (x, y)
        assert len({r.pick(x, y)[0] for x, y in pixels}) >= 3
        for x, y in [(-1, 0), (w, 0), (0, -1), (0, h)]:
            with pytest.raises(raster.TriError) as ei:
                r.pick(x, y)
            assert ei.value.code == abi.TRI_E_INVALID, (x, y)
    band = (13, 57)
    _, bdep, bids = reference(oracle, s, band)
    with raster.TriRaster(w, h, band=band, flags=abi.TRI_FLAG_NO_DEPTH_OUTPUT) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.render_frame()
        for x, y in [(0, 13), (w - 1, 56), (50, 35)]:
            assert r.pick(x, y) == (int(bids[y - 13, x]), None), (x, y)
        for y in (12, 57):
            with pytest.raises(raster.TriError) as ei:
                r.pick(5, y)
            assert ei.value.code == abi.TRI_E_INVALID


def test_pick_rect_equals_numpy_unique(oracle):
    from trident_raster import abi, raster, scenes

    s = id_ref.with_skipped_draw(id_ref.cubes_and_quad())
    _, _, ids = reference(oracle, s)
    w, h, n = s.width, s.height, len(s.draws)
    rects = [(50, 35, 50, 35), (3, 2, 3, 2), (0, 0, w - 1, h - 1), (10, 10, 40, 30), (60, 20, 99, 69), (-20, -5, 500, 500),
             (0, 0, 15, 15)]
    with raster.TriRaster(w, h) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.render_frame()
        seen = set()
        for x0, y0, x1, y1 in rects:
            box = ids[max(y0, 0):min(y1, h - 1) + 1, max(x0, 0):min(x1, w - 1) + 1]
            want = sorted(int(i) - 1 for i in np.unique(box) if i)
            assert r.pick_rect(x0, y0, x1, y1, n) == want, (x0, y0, x1, y1)
            seen.update(want)
        assert seen == {0, 2, 3}
        import ctypes as C

        lib = raster.load_library()
        bits = (C.c_uint32 * 1)()
        assert lib.tri_pick_rect(r._ctx, 0, 0, 5, 5, bits, 0, None) == abi.TRI_E_INVALID   # too few words
        assert lib.tri_pick_rect(r._ctx, 5, 0, 4, 5, bits, 1, None) == abi.TRI_E_INVALID   # reversed
        assert lib.tri_pick_rect(r._ctx, 0, 0, 5, 5, None, 1, None) == abi.TRI_E_INVALID   # no bitmap
        assert lib.tri_pick_rect(r._ctx, 0, 0, w - 1, h - 1, bits, 1, None) == abi.TRI_OK and bits[0] == 0b1101


# ---- the selection outline ----------------------------------------------------------------------------------------
OUTLINE_RECTS = [(0, 0, 20, 15, 0.5),      # touches the frame's top and left edges
                 (25, 20, 75, 50, 0.4),    # spans the kernel's 32-px tile boundaries at x = 32, 64 and y = 32
                 (80, 55, 100, 70, 0.3),   # touches the bottom and right edges
                 (40, 30, 60, 40, 0.2)]    # in front of the second: the visible silhouette has a hole


@pytest.fixture(scope="module")
def outline_case(oracle):
    from trident_raster import raster, scenes

    s = id_ref.pixel_quads("id_outline", 100, 70, OUTLINE_RECTS)
    _, dep, ids = reference(oracle, s)
    assert np.array_equal(ids, id_ref.ids_of_rects(100, 70, OUTLINE_RECTS))
    r = raster.TriRaster(s.width, s.height)
    scenes.load_scene(r, s)
    r.set_id_output(True)
    r.render_frame()
    base, _ = r.readback()
    assert np.array_equal(r.read_ids(), ids)
    yield r, ids, base
    r.close()


@pytest.mark.parametrize("selected", [[0], [1], [0, 2], [3, 1]])
@pytest.mark.parametrize("width", [1, 3, 8])
def test_opaque_outline_is_exact(outline_case, width, selected):
    """Outline pixels hold the colour's bytes exactly; every other pixel is bit-identical to the frame without it."""
    r, ids, base = outline_case
    rgba = (1.0, 0.6, 0.0, 1.0)
    r.set_outline(selected, rgba, width)
    r.render_frame()
    col, _ = r.readback()
    mask = id_ref.outline_mask(ids, selected, width)
    assert mask.any()
    want = base.copy()
    want[mask] = id_ref.colour_bytes(rgba)
    bad = int((col != want).any(axis=-1).sum())
    print(f"OUTLINE width {width} selected {selected}: {int(mask.sum())} outline pixels, {bad} wrong")
    assert bad == 0
    assert np.array_equal(r.read_ids(), ids)  # the outline draws over colour only
    r.set_outline(None)
    r.render_frame()
    assert np.array_equal(r.readback()[0], base)


def test_empty_selection_draws_nothing(outline_case):
    r, ids, base = outline_case
    r.set_outline([], (1.0, 0.0, 0.0, 1.0), 3)
    r.render_frame()
    assert np.array_equal(r.readback()[0], base)
    r.set_outline(None)


@pytest.mark.parametrize("width", [1, 8])
def test_half_transparent_outline(outline_case, width):
    """Alpha 0.5: within 1 LSB of the float64 src-over on the outline pixels, untouched elsewhere."""
    r, ids, base = outline_case
    rgba = (0.9, 0.2, 0.7, 0.5)
    r.set_outline([1, 2], rgba, width)
    r.render_frame()
    col, _ = r.readback()
    r.set_outline(None)
    mask = id_ref.outline_mask(ids, [1, 2], width)
    exact = id_ref.src_over_f64(base[mask], rgba)
    err = float(np.abs(col[mask].astype(np.float64) - exact).max())
    print(f"OUTLINE alpha 0.5 width {width}: max error {err:.4f} LSB over {int(mask.sum())} pixels")
    assert err <= 1.0
    assert np.array_equal(col[~mask], base[~mask])


def test_outline_argument_errors(outline_case):
    from trident_raster import abi, raster

    r, ids, base = outline_case
    for draws, width in [([0], 0), ([0], 9), ([4], 2), ([0, 99], 2)]:
        with pytest.raises(raster.TriError) as ei:
            r.set_outline(draws, (1, 1, 1, 1), width)
        assert ei.value.code == abi.TRI_E_INVALID, (draws, width)
    with pytest.raises(raster.TriError) as ei:
        r.set_outline([0], (1, float("nan"), 1, 1), 2)
    assert ei.value.code == abi.TRI_E_INVALID
    r.render_frame()
    assert np.array_equal(r.readback()[0], base)  # a refused outline leaves none behind
    with raster.TriRaster(100, 70, band=(0, 35)) as b:
        b.set_id_output(True)
        with pytest.raises(raster.TriError) as ei:
            b.set_outline([], (1, 1, 1, 1), 2)
        assert ei.value.code == abi.TRI_E_UNSUPPORTED
    with raster.TriRaster(100, 70) as c:
        with pytest.raises(raster.TriError) as ei:  # needs the id output
            c.set_outline([], (1, 1, 1, 1), 2)
        assert ei.value.code == abi.TRI_E_STATE
