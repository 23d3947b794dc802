"""The fragment stage on the device over its parameter space: every algebraic form of Default.frag in
raster_bin.h (fs_exact; fs_fast scalar, packed-pair and host-folded ONE) under the materials, light rigs and
texture addressing of scene_cases.shading_sphere / sampler_grid, against the oracle (depth bit-exact, colour within
COLOR_TOL) and against the float64 frames of tests/test_fragment_sweep.py (2 LSB, as
test_parity_gpu.test_gpu_against_float64_pipeline states and justifies). Each test asserts the instantiation that shaded
its frame through frame_stats()["path"].
"""
import copy

import numpy as np
import pytest

import scene_cases as sc
import test_fragment_sweep as sweep
from test_parity_gpu import COLOR_TOL, assert_parity, render_gpu

pytestmark = pytest.mark.gpu

F64_TOL = 2  # LSB: the device within 1 of the oracle, the oracle within 1 of float64


@pytest.fixture(params=["fast", "exact"])
def flags(request):
    """fast: hardware rcp/rsq/exp/log shading (default); exact: IEEE div/sqrt/powf (TRI_FLAG_EXACT_SHADING)."""
    from trident_raster import abi

    return abi.TRI_FLAG_EXACT_SHADING if request.param == "exact" else 0


SHADING_CASES = sweep.SHADING_CASES + [(rig, m, "shadow") for rig in sc.SWEEP_SUN_RIGS
                                       for m in range(len(sc.SWEEP_MATERIALS))]


def expect_path(path, variant):
    from trident_raster import abi

    one, ucol, shadow = path & abi.TRI_PATH_ONE_DRAW, path & abi.TRI_PATH_OBJ_UCOL, path & abi.TRI_PATH_SHADOW
    if variant == "one":  # the host-folded ONE form from a uniform colour
        assert one and ucol and not shadow, hex(path)
    elif variant == "one_vcol":  # the ONE form from per-vertex colours
        assert one and not ucol and not shadow, hex(path)
    elif variant == "multi":  # the plain scalar form
        assert not one and not shadow, hex(path)
    else:  # the packed-pair form with f.vis
        assert shadow, hex(path)


def check_frame(got, scene, oracle, min_covered=1):
    """A (colour, depth) pair already rendered against the oracle's frame of `scene`, at assert_parity's bar."""
    gc, gd = got
    oc, od, _ = oracle.render(scene)
    assert int((gd != od).sum()) == 0, scene.name
    diff = np.abs(gc.astype(np.int16) - oc.astype(np.int16))
    assert int(diff.max(initial=0)) <= COLOR_TOL, f"{scene.name}: colour diff {diff.max()} (> {COLOR_TOL})"
    assert int((od != 0x3F800000).sum()) >= min_covered


@pytest.mark.parametrize("rig,material,variant", SHADING_CASES)
def test_shading_sweep(oracle, flags, rig, material, variant):
    from trident_raster import abi

    s = sc.shading_sphere(rig, material, variant)
    f64 = sweep.shading_f64(rig, material, variant) if variant != "shadow" else None
    covered = int(f64[1].sum()) if f64 else sweep.SPHERE_MIN_PIXELS
    assert covered >= sweep.SPHERE_MIN_PIXELS
    assert_parity(s, oracle, min_covered=covered, flags=flags)
    gc, _, stats = render_gpu(s, flags=flags)
    expect_path(stats["path"], variant)
    assert bool(stats["path"] & abi.TRI_PATH_EXACT) == bool(flags), hex(stats["path"])
    if f64:
        diff = sweep.lsb_diff(gc, *f64)
        assert diff.max() <= F64_TOL, (s.name, diff.max())


SAMPLER_CASES = list(sc.SAMPLER_MODERATE) + list(sc.SAMPLER_LARGE) + ["5x3_neg+shadow", "5x3_neg+near_clip"]


@pytest.mark.parametrize("case", SAMPLER_CASES)
def test_sampler_sweep(oracle, flags, case):
    from trident_raster import abi, scenes

    name, _, form = case.partition("+")
    s = sc.sampler_case(name)
    f64 = sweep.sampler_f64(name) if name in sc.SAMPLER_MODERATE and not form else None
    covered = sweep.GRID_MIN_PIXELS
    if form == "shadow":  # the sampler in the shadow instantiation
        scenes.with_shadow(s, 256)
    elif form == "near_clip":  # the fetch of a clipped fragment: near_clip_single's ground plane through the 5 x 3 texture
        s = sc.near_clip_single(320, 240, 24)
        s.textures = [(1, sc.checker_texture(5, 3, 7))]
    assert_parity(s, oracle, min_covered=int(f64[1].sum()) if f64 else covered, flags=flags)
    gc, _, stats = render_gpu(s, flags=flags)
    if f64:
        diff = sweep.lsb_diff(gc, *f64)
        assert diff.max() <= F64_TOL, (s.name, diff.max())
    path = stats["path"]
    assert not path & abi.TRI_PATH_ONE_DRAW, hex(path)  # a filtered texture: never the solid instantiation
    assert bool(path & abi.TRI_PATH_SHADOW) == (form == "shadow"), hex(path)
    # uvs in the thousands of texels: the oracle's operation order in either build (frame_select.h kUvFastTexels)
    assert bool(path & abi.TRI_PATH_EXACT) == (name in sc.SAMPLER_LARGE or bool(flags)), hex(path)
    if name == "3x5_identity":  # the identity uv transform keeps object-space varyings
        assert path & abi.TRI_PATH_OBJ48, hex(path)
    if form == "near_clip":
        assert stats["triangles_clipped"] > 0


def _load_case(r, s):
    """Move a context to another case of the sweep by its materials, textures, UBO and draws alone."""
    r.upload_materials(s.materials)
    for slot, tex in s.textures:
        r.upload_texture(slot, tex)
    r.set_frame(s.ubo, s.clear)
    r.set_draws(s.draws)


def test_one_context_through_the_sweep(flags):
    """One context renders every (rig, material) of the single-draw form, then of the two-draw form, back to back; only
    materials, UBO, draws and a texture change between frames. Each frame is byte-equal to a fresh context's: a
    hoisted or folded constant (TriShadeConst, sbtm / sbtkd / sbtamb, a8) that survived a change would show."""
    from trident_raster import abi, raster, scenes

    first = sc.shading_sphere(sc.SWEEP_RIGS[0], 0, "one")
    with raster.TriRaster(first.width, first.height, flags=flags) as r:
        scenes.load_scene(r, first)
        distinct = set()
        for variant in ("one", "multi"):
            for rig in sc.SWEEP_RIGS:
                for material in range(len(sc.SWEEP_MATERIALS)):
                    s = sc.shading_sphere(rig, material, variant)
                    assert np.array_equal(s.vertices, first.vertices) and np.array_equal(s.meshes, first.meshes)
                    _load_case(r, s)
                    r.render_frame()
                    col, dep = r.readback()
                    one = bool(r.frame_stats()["path"] & abi.TRI_PATH_ONE_DRAW)
                    assert one == (variant == "one"), s.name
                    fc, fd, _ = render_gpu(s, flags=flags)
                    assert np.array_equal(dep, fd), s.name
                    assert np.array_equal(col, fc), (s.name, int(np.abs(col.astype(np.int16) - fc.astype(np.int16)).max()))
                    distinct.add(col.tobytes())
    # the frames do differ from one another (eleven repeats eight; the black material's frames coincide under a rig)
    assert len(distinct) >= 2 * 4 * (len(sc.SWEEP_MATERIALS) - 1)


def test_texture_slot_lifecycle(oracle, flags):
    """One context through a texture slot's life. Slot 0 holds a 3x5 texture, so every unused or out-of-range slot
    (-1, 256, 300) aliases a filtered texture; then slot 3 goes 1x1 -> 5x3 -> 1x1 -> 16x8 under an untouched draw list:
    the solid instantiation must follow the extent. Each frame matches the oracle and a fresh context's frame."""
    from trident_raster import abi, raster, scenes

    base = sc.sampler_case("3x5")
    base.textures = [(0, sc.checker_texture(3, 5, 21))]
    with raster.TriRaster(base.width, base.height, flags=flags) as r:
        scenes.load_scene(r, base)
        for slot in (-1, 256, 300):
            s = copy.copy(base)
            s.draws = [copy.deepcopy(base.draws[0])]
            s.draws[0].pc.texture_slot = slot
            s.name = f"slot_{slot}"
            r.set_draws(s.draws)
            r.render_frame()
            got = r.readback()
            check_frame(got, s, oracle, sweep.GRID_MIN_PIXELS)
            resolved = copy.copy(s)  # the same frame as a draw of slot 0 itself
            resolved.draws = [copy.deepcopy(base.draws[0])]
            resolved.draws[0].pc.texture_slot = 0
            fc, fd, _ = render_gpu(resolved, flags=flags)
            assert np.array_equal(got[0], fc) and np.array_equal(got[1], fd), s.name
        r.set_draws(base.draws)  # slot 3 from here on: untouched below
        white = np.full((1, 1, 4), 255, np.uint8)
        grey = np.array([[[200, 120, 40, 180]]], np.uint8)
        for k, tex in enumerate((white, sc.checker_texture(5, 3, 7), grey, sc.checker_texture(16, 8, 7))):
            s = copy.copy(base)
            s.textures = base.textures + [(3, tex)]
            s.name = f"slot3_step{k}_{tex.shape[1]}x{tex.shape[0]}"
            r.upload_texture(3, tex)
            r.render_frame()
            got = r.readback()
            solid = tex.shape[:2] == (1, 1)
            assert bool(r.frame_stats()["path"] & abi.TRI_PATH_ONE_DRAW) == solid, s.name
            check_frame(got, s, oracle, sweep.GRID_MIN_PIXELS)
            fc, fd, _ = render_gpu(s, flags=flags)
            assert np.array_equal(got[0], fc) and np.array_equal(got[1], fd), s.name


def test_uv_magnitude_routes_the_frame(oracle):
    """The fast build keeps a textured frame while its uvs stay within 8192 texels of the origin and hands it to the exact
    instantiation beyond (the interpolation then follows the oracle's order); one context, either side of the threshold
    by its draw list alone, then back under it by the slot's extent. The mesh's uvs reach 4 and the texture is 64 wide, so
    an offset of 124 is 8192 texels exactly."""
    from trident_raster import abi, raster, scenes

    base = sc.sampler_grid((64, 64), (1.0, 1.0), (124.0, -124.0), 1.0)
    assert float(np.abs(base.vertices["texcoord"]).max()) == 4.0
    with raster.TriRaster(base.width, base.height) as r:
        scenes.load_scene(r, base)
        for offset, beyond in ((124.0, False), (124.5, True), (-124.0, False), (-124.25, True)):
            s = copy.copy(base)
            s.draws = [copy.deepcopy(base.draws[0])]
            s.draws[0].pc.texture_offset[0] = offset
            s.name = f"uv_threshold_{offset:g}"
            r.set_draws(s.draws)
            r.render_frame()
            check_frame(r.readback(), s, oracle, sweep.GRID_MIN_PIXELS)
            assert bool(r.frame_stats()["path"] & abi.TRI_PATH_EXACT) == beyond, s.name
        s.textures = [(3, np.full((1, 1, 4), 200, np.uint8))]  # a 1 x 1 slot has no taps to misplace
        r.upload_texture(*s.textures[0])
        r.render_frame()
        check_frame(r.readback(), s, oracle, sweep.GRID_MIN_PIXELS)
        assert not r.frame_stats()["path"] & abi.TRI_PATH_EXACT
