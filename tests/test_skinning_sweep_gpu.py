"""The skinning branch of vertex_slot (vertex_stage.hip) and the host decisions around it (frame_select.h, tri_render) on
the device, over the forms of scene_cases.skinned_sphere: against the oracle (depth bit-exact, colour within COLOR_TOL,
equal set-up counts) and against the float64 frames of tests/test_skinning_sweep.py (2 LSB, as
test_parity_gpu.test_gpu_against_float64_pipeline states and justifies); under the cull flag, in row bands and in a band
group; through a palette's life in one context; over geometry without weights; and from a palette that k_pose wrote.
tests/test_skinning_sweep.py shows on the CPU that these scenes move by more than 2 LSB under each mistake they guard
against.
"""
import copy

import numpy as np
import pytest

import scene_cases as sc
import test_shadow
import test_skinning_sweep as skin
from test_fragment_sweep import lsb_diff
from test_fragment_sweep_gpu import F64_TOL, check_frame
from test_parity_gpu import COLOR_TOL, assert_parity, render_gpu

pytestmark = pytest.mark.gpu

CLEAR_DEPTH = 0x3F800000
# every form under the three rigs; the pre-pass also under the other rig with a sun
CASES = [(rig, m, form) for rig, m in sc.SKIN_RIG_MATERIALS for form in sc.SKIN_FORMS] + [("back", 3, "shadow")]


@pytest.fixture(params=["fast", "exact"])
def flags(request):
    """fast: hardware rcp/rsq/exp/log shading (default); exact: IEEE div/sqrt/powf (TRI_FLAG_EXACT_SHADING)."""
    from trident_raster import abi

    return abi.TRI_FLAG_EXACT_SHADING if request.param == "exact" else 0


def assert_world_space_path(path, scene):
    """A frame with a skinned draw keeps world-space varyings: clip_from_world is off for the draw, so no object-space
    instantiation may shade it (frame_select.h: draw_obj_ok, resolve_draws' obj48)."""
    from trident_raster import abi

    assert not path & (abi.TRI_PATH_OBJ48 | abi.TRI_PATH_OBJ_UCOL | abi.TRI_PATH_VARY_OBJ), (scene.name, hex(path))


def with_palette(scene, bones, name):
    s = copy.copy(scene)
    s.bones, s.name = bones, name
    return s


def with_draws(scene, draws, name):
    s = copy.copy(scene)
    s.draws, s.name = draws, name
    return s


# ---- parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,material,form", CASES)
def test_skinning_sweep(oracle, flags, rig, material, form):
    """Every form under every rig in both builds: the float64 frame, the depth formula, the path bits and the clip count
    first, the oracle's whole frame (assert_parity) last.

    `skips` is the regression test of the fragment stage's NaN rule (raster_bin.h, nan_reaches_colour). The float32
    clipper of the oracle and of k_setup alike leaves slivers in the holes around the five vertices without influences
    (15 pixels of the 320 x 240 frame, 14 of them background in the float64 raster), whose clip vertices carry the dead
    vertex's attributes: the normal normalize(0) = NaN. Default.frag's max(N.L, 0) keeps that NaN, so the colour is NaN
    and black is stored; fmaxf (v_max_f32) dropped it, and the device stored the ambient term of the dead vertex's
    colour instead, up to 72 LSB away under headon and eight and 105 under touch, in both builds."""
    from trident_raster import abi

    s = sc.skinned_sphere(rig, material, form)
    f64 = skin.skin_f64(rig, form) if form != "shadow" else None
    covered = int(f64[1].sum()) if f64 else skin.MIN_PIXELS["one"]
    if form == "shadow":  # the map itself: shadow_vertex sees the skinned position
        gc, gd, gmap, stats = test_shadow.render_gpu(s, flags=flags)
        omap = np.zeros((s.shadow.size, s.shadow.size), np.uint32)
        oracle.render(s, shadow_map_out=omap)
        assert int((gmap != omap).sum()) == 0, f"{s.name}: shadow map mismatch"
        # casters landed in the map (found: 62500 texels under headon, 60270 under back, 14739 under the default
        # direction that eight and touch carry without a sun)
        assert int((omap != CLEAR_DEPTH).sum()) > 10000
    else:
        gc, gd, stats = render_gpu(s, flags=flags)
        diff = lsb_diff(gc, *f64)
        assert diff.max() <= F64_TOL, (s.name, diff.max())
        skin.check_depth(gd, form)
    path = stats["path"]
    assert_world_space_path(path, s)
    assert bool(path & abi.TRI_PATH_SHADOW) == (form == "shadow"), hex(path)
    assert bool(path & abi.TRI_PATH_EXACT) == bool(flags), hex(path)
    assert bool(path & abi.TRI_PATH_ONE_DRAW) == (form not in ("multi", "shadow")), hex(path)
    if form == "skips":
        assert stats["triangles_clipped"] > 0
    assert_parity(s, oracle, min_covered=covered, flags=flags)


# ---- the cull flag and row bands -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one", "multi"])
def test_cluster_cull_keeps_skinned_draws(oracle, form):
    """cluster_visible is always true for a skinned draw (its vertices leave the clusters' boxes): the frame under
    TRI_FLAG_CLUSTER_CULL is the unculled one, byte for byte. multi has an unskinned draw between two skinned ones."""
    from trident_raster import abi

    s = sc.skinned_sphere("eight", 0, form)
    plain_c, plain_d, plain_s = render_gpu(s)
    cull_c, cull_d, cull_s = render_gpu(s, flags=abi.TRI_FLAG_CLUSTER_CULL)
    assert np.array_equal(cull_d, plain_d) and np.array_equal(cull_c, plain_c)
    assert cull_s["triangles_setup"] == plain_s["triangles_setup"]
    assert_parity(s, oracle, min_covered=skin.MIN_PIXELS[form], flags=abi.TRI_FLAG_CLUSTER_CULL)


@pytest.mark.parametrize("form", ["one", "multi"])
def test_row_bands_of_skinned_frames(oracle, form):
    """Four row bands (k_vertex_band for the single draw, k_vertex for three) assemble to the full frame byte for byte,
    each at parity with the oracle's band."""
    s = sc.skinned_sphere("headon", 3, form)
    full_c, full_d, _ = render_gpu(s)
    cuts = np.linspace(0, s.height, 5).astype(int)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.append(render_gpu(s, band=(int(a), int(b))))
        assert_world_space_path(parts[-1][2]["path"], s)
        assert_parity(s, oracle, band=(int(a), int(b)), min_covered=0)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), full_d)
    assert np.array_equal(np.concatenate([p[0] for p in parts]), full_c)


@pytest.mark.parametrize("form", ["one", "multi"])
def test_band_group_uploads_the_palette(oracle, form):
    """raster.TriGroup over three bands of one device: the palette goes through the group's upload to every band."""
    from trident_raster import raster, scenes

    s = sc.skinned_sphere("touch", 5, form)
    with raster.TriGroup(s.width, s.height, [0] * 3) as g:
        scenes.load_scene(g, s)
        g.render_frame()
        col, dep = g.readback()
    check_frame((col, dep), s, oracle, skin.MIN_PIXELS[form])
    full_c, full_d, _ = render_gpu(s)
    assert np.array_equal(dep, full_d) and np.array_equal(col, full_c)


# ---- one context through a palette's life ------------------------------------------------------------------------------
def test_one_context_through_a_palettes_life(oracle, flags):
    """One context: the single skinned draw; another palette; the short palette; the draw unskinned (non-conformal, then
    conformal: the object-space path returns); skinned again over the short palette that is still there; then other
    geometry, palette and three draws. Each frame is byte-equal to a fresh context's and at parity with the oracle: a
    palette extent, a vskin pointer or an object-space decision that survived a change would show."""
    from trident_raster import abi, raster, scenes

    rig, material = "eight", 0
    one = sc.skinned_sphere(rig, material, "one")
    multi = sc.skinned_sphere(rig, material, "multi")
    other = with_palette(one, sc.skin_palette(sc.SKIN_BONES_2), "life_other_palette")
    short = with_palette(one, one.bones[:3], "life_short_palette")
    model = scenes.compose_transform(*sc.SKIN_MODEL)
    conformal = scenes.compose_transform(sc.SKIN_MODEL[0], sc.SKIN_MODEL[1], (0.9, 0.9, 0.9))
    plain = with_draws(short, [abi.make_draw(0, model, material_index=0)], "life_unskinned")
    plain_obj = with_draws(short, [abi.make_draw(0, conformal, material_index=0)], "life_unskinned_conformal")
    obj_bits = abi.TRI_PATH_VARY_OBJ | abi.TRI_PATH_OBJ_XFORM
    frames = []
    with raster.TriRaster(one.width, one.height, flags=flags) as r:
        scenes.load_scene(r, one)
        steps = [(one, lambda: None), (other, lambda: r.upload_bone_palette(other.bones)),
                 (short, lambda: r.upload_bone_palette(short.bones)), (plain, lambda: r.set_draws(plain.draws)),
                 (plain_obj, lambda: r.set_draws(plain_obj.draws)), (short, lambda: r.set_draws(short.draws)),
                 (multi, lambda: (r.upload_geometry(multi.vertices, multi.indices, multi.meshes),
                                  r.upload_bone_palette(multi.bones), r.set_draws(multi.draws)))]
        for scene, change in steps:
            change()
            r.render_frame()
            frames.append((scene, *r.readback(), r.frame_stats()))
    distinct = set()
    for scene, col, dep, stats in frames:
        check_frame((col, dep), scene, oracle, skin.MIN_PIXELS["one"])
        assert stats["triangles_setup"] == oracle.render(scene)[2]["triangles_setup"], scene.name
        fc, fd, fs = render_gpu(scene, flags=flags)
        assert np.array_equal(dep, fd), scene.name
        assert np.array_equal(col, fc), (scene.name, int(np.abs(col.astype(np.int16) - fc.astype(np.int16)).max()))
        path = stats["path"]
        assert path == fs["path"], (scene.name, hex(path), hex(fs["path"]))
        # frame_select.h: a single draw over the 1x1 default slot is shade_solid (ONE_DRAW) with 36-B varyings, so obj48
        # is off; vary_obj needs draw0_obj: an affine, unskinned draw whose normal matrix is conformal (draw_obj_ok).
        # SKIN_MODEL scales by (1, 0.9, 1.1): not conformal. The vertex colours vary: never OBJ_UCOL.
        if scene is plain_obj:
            assert path & obj_bits == obj_bits and not path & (abi.TRI_PATH_OBJ48 | abi.TRI_PATH_OBJ_UCOL), hex(path)
        else:
            assert_world_space_path(path, scene)
        assert bool(path & abi.TRI_PATH_ONE_DRAW) == (scene is not multi), (scene.name, hex(path))
        distinct.add(dep.tobytes())
    assert len(distinct) == 6  # the short palette's frame comes twice; every other step moves the surface


# ---- geometry without weights -------------------------------------------------------------------------------------------
def _assert_cleared(got, scene, oracle):
    col, dep, stats = got
    oc, od, os_ = oracle.render(scene)
    assert (dep == CLEAR_DEPTH).all() and np.array_equal(dep, od), scene.name
    assert (col == col[0, 0]).all(), scene.name
    assert int(np.abs(col.astype(np.int16) - oc.astype(np.int16)).max()) <= COLOR_TOL, scene.name
    assert stats["triangles_setup"] == os_["triangles_setup"], (stats, os_)


def test_skinned_draw_over_geometry_without_weights(oracle):
    """Every bone_weights zero under a draw with bone_count > 0: the skin matrix is zero, every vertex collapses to
    (0, 0, 0, 0) and the frame is the cleared one (tri_render fills the skin buffer with zeros). Weighted geometry
    uploaded into the same context then renders `one`. The same through a raster.TriGeometry that two contexts bind."""
    from trident_raster import raster, scenes

    one = sc.skinned_sphere("eight", 0, "one")
    bare = copy.copy(one)
    bare.vertices = one.vertices.copy()
    bare.vertices["bone_weights"] = 0.0
    bare.name = "skinned_without_weights"
    with raster.TriRaster(one.width, one.height) as r:
        scenes.load_scene(r, bare)
        r.render_frame()
        _assert_cleared((*r.readback(), r.frame_stats()), bare, oracle)
        r.upload_geometry(one.vertices, one.indices, one.meshes)
        r.render_frame()
        got = r.readback()
        check_frame(got, one, oracle, skin.MIN_PIXELS["one"])
        assert r.frame_stats()["triangles_setup"] == oracle.render(one)[2]["triangles_setup"]
    fc, fd, _ = render_gpu(one)
    assert np.array_equal(got[1], fd) and np.array_equal(got[0], fc)
    g = raster.TriGeometry(0)
    try:
        g.upload(bare.vertices, bare.indices, bare.meshes)
        with raster.TriRaster(one.width, one.height) as a, raster.TriRaster(one.width, one.height) as b:
            for r in (a, b):
                scenes.load_scene(r, bare, geometry=g)
            for r in (a, b, a):  # b finds the zeros that a's frame put there
                r.render_frame()
                _assert_cleared((*r.readback(), r.frame_stats()), bare, oracle)
            g.upload(one.vertices, one.indices, one.meshes)  # weights arrive in the shared object
            for r in (b, a):
                r.render_frame()
                shared = r.readback()
                assert np.array_equal(shared[1], fd) and np.array_equal(shared[0], fc)
    finally:
        g.close()


# ---- a palette that k_pose wrote ---------------------------------------------------------------------------------------
def test_device_posed_palette_feeds_the_vertex_stage(oracle, flags):
    """An uploaded prefix, then a suffix posed on the device (as test_pose_gpu.test_uploaded_prefix_then_posed_suffix sets
    it up); the palette read back is the oracle's scene.bones. The skinned sphere drawn from the posed rows is at parity:
    pose evaluation meets the vertex stage through the oracle, not through a second device frame."""
    import anim_cases
    import anim_ref
    from trident_raster import raster, scenes

    rig = next(r for r in anim_ref.kernel_rigs() if r.name == "chain3")
    s = sc.skinned_sphere("eight", 0, "one")
    prefix = np.arange(5 * 16, dtype=np.float32).reshape(5, 16) + 0.5
    s.draws[0].pc.bone_offset = 5  # the posed suffix: the prefix is never read
    s.name = "skinned_from_posed_palette"
    with raster.TriAnimSet(0) as aset, raster.TriRaster(s.width, s.height, device=0, flags=flags) as r:
        sk, clips = anim_cases.device_asset(aset, rig)
        s.bones = prefix
        scenes.load_scene(r, s)
        r.pose_palette(aset, [(sk, clips[1], 0.4, 5)])  # the "slerp" clip between its keys
        r.render_frame()
        col, dep = r.readback()
        stats = r.frame_stats()
        s.bones = r.read_bone_palette(5 + rig.bones)
    assert np.array_equal(s.bones[:5], prefix) and np.isfinite(s.bones).all()
    assert not np.array_equal(s.bones[5:], np.tile(np.eye(4, dtype=np.float32).reshape(16), (rig.bones, 1)))
    check_frame((col, dep), s, oracle, 2000)
    assert stats["triangles_setup"] == oracle.render(s)[2]["triangles_setup"]
    assert_world_space_path(stats["path"], s)
