"""GPU tests of the motion-vector pass (include/tri_raster.h "motion vectors"): k_motion, the C-ABI around it and its
place in the frame.

The bar: device motion == tests/motion_ref.py's float32 restatement, fed with the library's own table
(tri_motion_matrices) and the device's own ids and depth, compared as uint32 — ZERO mismatches: the rule fixes every
operation. Device depth == the oracle's D is asserted in the same case. The cases are the smallest at which the kernel
can go wrong: 100 x 70 (7000 pixels: 1750 whole vectors), 101 x 70 (rows that are not 16-B aligned, vectors that straddle
a row end, and 7070 = 4 * 1767 + 2 pixels: a two-pixel tail), one draw (the wave-uniform lookup), a row band (the
full-frame y), 1024 draws of 2 x 2 px (every lane gathers another row), a previous camera turned round (q_3 <= 0).
"""
import ctypes as C

import numpy as np
import pytest

import id_ref
import motion_ref as mr
import scene_cases as sc
from test_raster_paths_gpu import OVF_BIN_LIST, expect_overflow

pytestmark = pytest.mark.gpu
F = np.float32
_DEPTH = {}


def oracle_depth(oracle, scene, band=None):
    """The oracle's D of a scene, computed once, shared and never modified."""
    key = (scene.name, scene.width, scene.height, band)
    if key not in _DEPTH:
        if len(_DEPTH) >= 4:
            _DEPTH.pop(next(iter(_DEPTH)))
        dep = oracle.render(scene, band=band)[1]
        dep.setflags(write=False)
        _DEPTH[key] = dep
    return _DEPTH[key]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def compare(tag, r, scene, hist, dep=None, band=None, min_px=2.0):
    """Device motion against the restatement over the library's table and the device's ids and depth; returns
    (motion, ids)."""
    from trident_raster import raster

    _, gdep = r.readback()
    gids = r.read_ids()
    got = r.read_motion()
    table = raster.motion_matrices(scene.ubo, scene.draws, hist)
    want = mr.restate(table, gids, gdep, scene.width, scene.height, y0=band[0] if band else 0)
    bad = int((bits(got) != bits(want)).any(axis=-1).sum())
    bad_d = -1 if dep is None else int((gdep != dep).sum())
    print(f"MOTION {tag}: {got.shape[1]} x {got.shape[0]}, distinct ids {len(np.unique(gids))}, max |m| "
          f"{np.abs(want).max():.2f} px, depth mismatches {bad_d}, motion mismatches {bad}")
    assert got.shape == want.shape == (r.rows, scene.width, 2)
    if dep is not None:
        assert bad_d == 0, f"{tag}: {bad_d} depth mismatches"
    assert bad == 0, f"{tag}: {bad} motion mismatches"
    assert np.abs(want).max() >= min_px, tag  # (the case shows motion)
    return got, gids


def render_motion(oracle, scene, hist, band=None, **kw):
    from trident_raster import raster, scenes

    dep = oracle_depth(oracle, scene, band)
    rows = (band[1] - band[0]) if band else scene.height
    with raster.TriRaster(scene.width, scene.height, band=band) as r:
        scenes.load_scene(r, scene)
        r.set_id_output(True)
        r.set_motion_output(True)
        r.set_motion_history(*hist)
        r.render_frame()
        out = compare(scene.name, r, scene, hist, dep, band, **kw)
        img = r.motion_image()
        assert (img.width, img.height, img.pitch_bytes, img.format) == (scene.width, rows, scene.width * 8, 103)
        assert img.device_ptr
    return out


# ---- k_motion -------------------------------------------------------------------------------------------------------
def test_motion_of_three_moved_draws(oracle):
    """100 x 70, two cubes and a quad, every draw moved differently, the camera moved and turned: mixed waves."""
    s = id_ref.cubes_and_quad()
    _, gids = render_motion(oracle, s, mr.previous_frame(s))
    assert len(np.unique(gids)) == 4


def test_motion_at_a_width_of_101(oracle):
    """Rows of 404 B: no row but every fourth starts on a 16-B boundary, vectors straddle row ends, and the image ends
    in a partial vector."""
    s = id_ref.cubes_and_quad(101, 70)
    assert (s.width * s.height) % 4 == 2
    got, gids = render_motion(oracle, s, mr.previous_frame(s))
    assert len(np.unique(gids)) == 4
    assert bits(got[-1, -2:]).any()  # the tail pixels were written (the turned camera moves the background)


def test_motion_of_one_draw(oracle):
    """A single-draw frame: whole waves under one id take the wave-uniform lookup."""
    from trident_raster import scenes

    s = scenes.scene_c1_cube(1, 100, 70, skybox="solid")
    s.name = "motion_c1_cube"
    _, gids = render_motion(oracle, s, mr.previous_frame(s))
    assert set(np.unique(gids)) == {0, 1}
    waves = gids.reshape(-1)[: gids.size // 256 * 256].reshape(-1, 256)  # a wave's 64 lanes x 4 pixels
    uniform = (waves == waves[:, :1]).all(axis=1)
    assert uniform.any() and not uniform.all()  # both lookups ran


def test_motion_of_a_row_band(oracle):
    """Rows [16, 48) of the frame: y is the full-frame row."""
    s = id_ref.cubes_and_quad()
    band = (16, 48)
    got, _ = render_motion(oracle, s, mr.previous_frame(s), band=band)
    from trident_raster import raster, scenes

    with raster.TriRaster(s.width, s.height) as r:  # ... and equals those rows of the whole frame
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.set_motion_output(True)
        r.set_motion_history(*mr.previous_frame(s))
        r.render_frame()
        assert np.array_equal(bits(r.read_motion()[band[0]:band[1]]), bits(got))


def test_motion_of_1024_small_draws(oracle):
    """64 x 64 covered by 1024 quads of 2 x 2 px, each its own draw with its own integer translation one frame ago:
    every lane of a wave gathers another table row, and 64 KiB of table is beyond any on-chip staging."""
    w = h = 64
    rects = [(2 * i, 2 * j, 2 * i + 2, 2 * j + 2, 0.25 + 0.5 * ((i * 7 + j * 3) % 16) / 16.0) for j in range(32) for i in range(32)]
    s = id_ref.pixel_quads("motion_1024_quads", w, h, rects)
    assert len(s.draws) == 1024
    v, p = mr.camera_of(s.ubo)
    shifts = [((k * 5) % 13 - 6, (k * 11) % 9 - 4) for k in range(1024)]
    prev = np.array([mr.to_cm(mr.rigid((tx, ty, 0.0))).reshape(16) for tx, ty in shifts], F)
    got, gids = render_motion(oracle, s, (v, p, prev))
    assert np.array_equal(gids, id_ref.ids_of_rects(w, h, rects)) and len(np.unique(gids)) == 1024
    want = np.array(shifts, np.float64)[gids.astype(np.int64) - 1]
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"MOTION 1024 draws: max error against the integer translations {err:.2e} px")
    assert err <= 8 * 2.0 ** -24 * (w / 2)  # (as test_motion_cpu.test_a_pixel_translation_comes_back derives it)


def test_motion_behind_the_previous_camera_is_zero(oracle):
    """The previous camera turned by 180 degrees about its y axis: every point lay behind it, q_3 <= 0, zeros."""
    s = id_ref.cubes_and_quad()
    hist = mr.previous_frame(s, camera_move=mr.rigid((0, 0, 0), (0.0, 180.0, 0.0)))
    got, _ = render_motion(oracle, s, hist, min_px=0.0)
    assert not bits(got).any()


def test_still_draws_beside_moving_ones_have_zero_bits(oracle):
    s = id_ref.cubes_and_quad()
    v, p, prev = mr.previous_frame(s, still=(0, 2), camera_move=None)
    got, gids = render_motion(oracle, s, (v, p, prev))
    assert not bits(got[(gids == 0) | (gids == 1) | (gids == 3)]).any()
    assert np.abs(got[gids == 2]).max() >= 2.0


def test_history_null_replaced_and_removed(oracle):
    """No history: all zero. A history, then another one: each frame follows the history it was rendered with."""
    from trident_raster import raster, scenes

    s = id_ref.cubes_and_quad()
    dep = oracle_depth(oracle, s)
    first = mr.previous_frame(s)
    second = mr.previous_frame(s, still=(1,), camera_move=mr.rigid((0.0, 0.1, 0.0), (0.0, 3.0, 0.0)))
    with raster.TriRaster(s.width, s.height) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.set_motion_output(True)
        r.render_frame()
        assert not bits(r.read_motion()).any()
        r.set_motion_history(*first)
        r.render_frame()
        a, _ = compare("history 1", r, s, first, dep)
        r.set_motion_history(*second)
        r.render_frame()
        b, _ = compare("history 2", r, s, second, dep)
        assert not np.array_equal(a, b)
        r.set_motion_history(second[0], second[1], None)  # the camera alone
        r.render_frame()
        compare("camera only", r, s, (second[0], second[1], None), dep)
        r.set_motion_history(None)
        r.render_frame()
        assert not bits(r.read_motion()).any()


def test_motion_after_a_bin_overflow(oracle):
    """2200 large triangles in one bin, three draws: TRI_E_OVERFLOW first (the readers report it), the right motion
    after the re-render."""
    from trident_raster import abi, raster, scenes

    s = sc.stacked_quads(200, 120, draws=3, textured=True)
    dep = oracle_depth(oracle, s)
    hist = mr.previous_frame(s)
    with raster.TriRaster(s.width, s.height) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.set_motion_output(True)
        r.set_motion_history(*hist)
        expect_overflow(r, OVF_BIN_LIST)
        r.render_frame()
        compare(s.name, r, s, hist, dep)


def test_motion_output_changes_neither_colour_nor_depth_nor_ids(oracle):
    from trident_raster import raster, scenes

    s = id_ref.cubes_and_quad()
    hist = mr.previous_frame(s)
    with raster.TriRaster(s.width, s.height) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.render_frame()
        col0, dep0 = r.readback()
        ids0 = r.read_ids()
        r.set_motion_output(True)
        r.set_motion_history(*hist)
        r.render_frame()
        col1, dep1 = r.readback()
        assert np.array_equal(col0, col1) and np.array_equal(dep0, dep1) and np.array_equal(ids0, r.read_ids())
        assert np.array_equal(dep1, oracle_depth(oracle, s))
        assert bits(r.read_motion()).any()
        r.set_motion_output(False)
        r.render_frame()
        col2, dep2 = r.readback()
        assert np.array_equal(col0, col2) and np.array_equal(dep0, dep2) and np.array_equal(ids0, r.read_ids())


def test_frame_without_primitives_moves_with_the_camera():
    from trident_raster import raster, scenes

    s = sc.empty_scene(100, 70)
    v, p = mr.camera_of(s.ubo)
    hist = (mr.to_cm(mr.rigid((0, 0, 0), (0.0, 3.0, 0.0)) @ mr.mat(v)).reshape(16), p, None)
    with raster.TriRaster(s.width, s.height) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.set_motion_output(True)
        r.set_motion_history(*hist)
        r.render_frame()
        compare("empty", r, s, hist)


# ---- the C-ABI's rules ----------------------------------------------------------------------------------------------
def test_error_codes():
    from trident_raster import abi, raster, scenes

    s = id_ref.cubes_and_quad()
    v, p, prev = mr.previous_frame(s)

    def code(call):
        with pytest.raises(raster.TriError) as ei:
            call()
        return ei.value.code

    with raster.TriRaster(s.width, s.height) as r:
        scenes.load_scene(r, s)
        assert code(lambda: r.set_motion_output(True)) == abi.TRI_E_STATE  # without the id output
        assert code(r.read_motion) == abi.TRI_E_STATE and code(r.motion_image) == abi.TRI_E_STATE
        r.set_id_output(True)
        r.set_motion_output(True)
        assert code(r.read_motion) == abi.TRI_E_STATE  # on, but no frame yet
        assert r.motion_image().format == 103
        lib = raster.load_library()
        assert lib.tri_read_motion(r._ctx, None) == abi.TRI_E_INVALID
        assert lib.tri_get_motion_output(r._ctx, None) == abi.TRI_E_INVALID
        assert lib.tri_get_motion_timing(r._ctx, None, None) == abi.TRI_E_INVALID
        assert code(lambda: r.set_motion_history(v, p, prev, draw_count=0)) == abi.TRI_E_INVALID
        r.set_motion_history(v, p, prev[:2])  # two previous models for three draws
        assert code(r.render) == abi.TRI_E_STATE
        r.set_motion_history(v, p, prev)
        r.render_frame()
        assert r.read_motion().shape == (70, 100, 2)
        r.set_draws(s.draws[:2])  # the draw list shrank under the stored history
        assert code(r.render) == abi.TRI_E_STATE
        r.set_motion_output(False)  # ... which only the motion pass minds
        r.render_frame()
        r.set_draws(s.draws)
        r.set_motion_output(True)
        r.render_frame()
        r.set_id_output(False)  # switching ids off switches motion off
        assert code(r.read_motion) == abi.TRI_E_STATE and code(r.motion_image) == abi.TRI_E_STATE
        r.render_frame()
        assert code(lambda: r.set_motion_output(True)) == abi.TRI_E_STATE
    with raster.TriRaster(s.width, s.height, flags=abi.TRI_FLAG_NO_DEPTH_OUTPUT) as r:
        r.set_id_output(True)
        assert code(lambda: r.set_motion_output(True)) == abi.TRI_E_UNSUPPORTED


def test_motion_pass_is_timed_by_events_of_its_own():
    """tri_set_timing stamps k_motion on both sides: tri_get_motion_timing reports it for exactly the timed frames that
    ran it, nothing with the output off, and tri_timing keeps its frame count."""
    from trident_raster import raster, scenes

    s = id_ref.sphere_and_quad()
    with raster.TriRaster(s.width, s.height) as r:
        scenes.load_scene(r, s)
        r.set_id_output(True)
        r.render_frame()
        r.set_timing(True)
        for _ in range(3):
            r.render()
        assert r.timing()["frames"] == 3 and r.motion_timing() == (0.0, 0)
        r.set_motion_output(True)
        r.set_motion_history(*mr.previous_frame(s))
        r.render_frame()
        r.set_timing(True)  # (restarts the sums)
        for _ in range(5):
            r.render()
        t = r.timing()
        ms, frames = r.motion_timing()
        print(f"MOTION timing: {1e3 * ms / 5:.1f} us per frame in k_motion, stages {t}")
        assert t["frames"] == 5 and frames == 5 and r.id_timing()[1] == 5
        assert 0.0 < ms < t["ms_frame"] and t["ms_raster"] >= 0.0
        r.set_timing(False)
