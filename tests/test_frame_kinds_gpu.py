"""GPU parity of the frame-kind raster kernels (k_raster_kind*: the fast single-draw instantiation with its
frame-uniform switches as compile-time constants) and of the generic instantiation they fall back to.

Every frame is 80 x 72 pixels, so the right and bottom bins are partial at either bin size (80 = 2 * 32 + 16 = 5 * 16,
72 = 2 * 32 + 8 = 4 * 16 + 8), with at most 2k triangles: 288 triangles or more (0.05 per pixel) give 32-px bins, fewer
give 16-px bins. The bar is DESIGN §4's: depth bits equal as uint32, every B8G8R8A8 channel within COLOR_TOL. Each case
asserts the kind tri_frame_stats reports (TRI_PATH_KIND and the TRI_KIND_* switches above TRI_PATH_KIND_SHIFT), so a
frame that lands on another kernel fails rather than passing on the wrong path.
"""
import numpy as np
import pytest

import scene_cases as sc
from test_parity_gpu import COLOR_TOL

pytestmark = pytest.mark.gpu

W, H = 80, 72
BG = 0x3F800000
F = np.float32

SUN = {"type": "directional"}
POINTS = [{"type": "point", "position": (px, py, -2.5), "range": 8.0, "intensity": 3.0 + k,
           "color": (1.0, 0.9 - 0.1 * k, 0.7 + 0.1 * k)}
          for k, (px, py) in enumerate([(-3.0, 1.5), (3.0, 1.5), (-3.0, -1.5), (3.0, -1.5)])]


def grid_scene(name, n=20, half=(2.4, 2.1), lights=(SUN, *POINTS), sky="cube", model=None, offset=(0.0, 0.0),
               one_colour=False, near_tri=False):
    """The C3 grid shrunk to `half` world units about the view axis (the frame's half extent at its depth is 3.2 x 2.9,
    so sky shows around it), n x n vertices, shifted by `offset`; near_tri appends one triangle through the near plane."""
    from trident_raster import abi, scenes

    s = scenes.scene_c3_grid(W, H, n, skybox="solid")
    v, idx = scenes.displaced_grid_mesh(n, extent=half)
    v["position"][:, 0] += F(offset[0])
    v["position"][:, 1] += F(offset[1])
    if one_colour:
        v["color"] = F(1.0)
    if near_tri:  # from in front of the grid to behind the eye (the camera sits at the origin, looking down -z)
        t = v[:3].copy()
        t["position"] = np.array([(-0.6, -0.5, -3.0), (0.6, -0.5, -3.0), (0.0, 0.4, 1.0)], F)
        t["normal"] = np.array([0.0, 0.0, 1.0], F)
        t["color"] = np.array([(0.9, 0.6, 0.5), (0.5, 0.9, 0.6), (0.6, 0.5, 0.9)], F)
        idx = np.concatenate([idx, np.array([0, 1, 2, 0, 2, 1], np.uint32) + np.uint32(v.size)])  # either winding
        v = np.concatenate([v, t])
    s.vertices, s.indices = v, idx
    s.meshes = np.array([(0, idx.size, 0, 0)], abi.MESH_RANGE_DTYPE)
    s.draws = [abi.make_draw(0, np.eye(4, dtype=F) if model is None else model, material_index=0)]
    view, proj = scenes.editor_camera((0.0, 0.0, 0.0), (0, 0, 0), 60.0, (W, H), 0.1, 1000.0)
    s.ubo = scenes.pack_ubo(view, proj, (0.0, 0.0, 0.0), list(lights))
    s.skybox = {"cube": sc.cubemap_faces(16, seed=3), "solid": sc.SOLID_0x808080, None: None}[sky]
    s.name = name
    return s


def sphere_scene(name, lights, sky="cube"):
    """C2's sphere (no vertex colours: one colour for every vertex) with 192 triangles: a sparse frame, 16-px bins."""
    from trident_raster import scenes

    s = scenes.scene_c2_sphere(W, H, 8, 12, skybox="solid")
    view, proj = scenes.editor_camera((0.0, 0.0, 9.0), (0, 0, 0), 60.0, (W, H), 0.1, 1000.0)
    s.ubo = scenes.pack_ubo(view, proj, (0.0, 0.0, 9.0), list(lights))
    s.skybox = sc.cubemap_faces(16, seed=3) if sky == "cube" else sc.SOLID_0x808080
    s.name = name
    return s


def trs():
    from trident_raster import scenes

    return scenes.compose_transform((0.15, -0.1, -0.2), (0.0, 12.0, 0.0), (0.95, 0.95, 0.95))


def kind_of(*names):
    from trident_raster import abi

    k = 0
    for n in names:
        k |= getattr(abi, "TRI_KIND_" + n)
    return k


def run_case(oracle, scene, bin_size, kind, flags=0, depth=True, min_covered=300, min_sky=200, clipped=0, crowded=0):
    """Render, compare with the oracle and assert the reported kind (None: the generic instantiation)."""
    from trident_raster import abi, raster, scenes

    assert scene.width == W and scene.height == H and scene.indices.size // 3 <= 2000
    assert sc.expected_bin_size(W, H, H, scene.indices.size // 3) == bin_size
    ocol, odep, ostats = oracle.render(scene)
    with raster.TriRaster(W, H, flags=flags) as r:
        scenes.load_scene(r, scene)
        r.render_frame()
        col, dep = r.readback(depth=depth)
        st = r.frame_stats()
    path = st["path"]
    print(f"KINDS {scene.name}: bin_size {st['bin_size']} path {path:#x} setup {st['triangles_setup']} "
          f"clipped {st['triangles_clipped']}")
    assert st["bin_size"] == bin_size, st
    want = abi.TRI_PATH_ONE_DRAW | abi.TRI_PATH_VARY_OBJ
    assert path & want == want, hex(path)
    if kind is None:
        assert not path & abi.TRI_PATH_KIND and path >> abi.TRI_PATH_KIND_SHIFT == 0, hex(path)
    else:
        assert path & abi.TRI_PATH_KIND, hex(path)
        assert (path >> abi.TRI_PATH_KIND_SHIFT) & abi.TRI_KIND_MASK == kind, (hex(path), hex(kind))
    assert st["triangles_setup"] == ostats["triangles_setup"], (st, ostats)
    assert st["triangles_clipped"] >= clipped, st
    covered = int((odep != BG).sum())
    if crowded:  # the bins the mesh touches cannot all hold `crowded` entries or fewer
        ys, xs = np.nonzero(odep != BG)
        touched = (xs.max() // bin_size - xs.min() // bin_size + 1) * (ys.max() // bin_size - ys.min() // bin_size + 1)
        assert st["bin_entries"] > crowded * touched, (st, touched)
    assert covered >= min_covered and odep.size - covered >= min_sky, (covered, odep.size)
    if depth:
        bad = int((dep != odep).sum())
        assert bad == 0, f"{scene.name}: {bad} depth mismatches"
    worst = int(np.abs(col.astype(np.int16) - ocol.astype(np.int16)).max(initial=0))
    assert worst <= COLOR_TOL, f"{scene.name}: colour diff {worst} (> {COLOR_TOL})"


LIT = ("SUN", "LIGHTS", "DEPTH")


def test_kind_lit_sampled_sky(oracle):
    """C3's kind: vertex colours, a sun and four point lights, a sampled sky behind the grid (queued background)."""
    run_case(oracle, grid_scene("kinds_c3"), 32, kind_of(*LIT, "SKYQ"))


def test_kind_lit_one_point_light(oracle):
    """The same kind with one point light: the light loop's look-ahead load past the last light."""
    run_case(oracle, grid_scene("kinds_c3_1pt", lights=(SUN, POINTS[1])), 32, kind_of(*LIT, "SKYQ"))


def test_kind_lit_trs_draw(oracle):
    """C3 under a TRS draw: position and normal through the model and normal matrices per pixel."""
    run_case(oracle, grid_scene("kinds_c3trs", model=trs()), 32, kind_of(*LIT, "SKYQ", "XFORM"))


def test_kind_lit_uniform_sky(oracle):
    """A uniform sky: background pixels take its constant in the pixel loop, no skybox pass."""
    run_case(oracle, grid_scene("kinds_c3_solid", sky="solid"), 32, kind_of(*LIT))


def test_kind_lit_no_sky(oracle):
    """No skybox: the same kind, background pixels take the clear colour."""
    run_case(oracle, grid_scene("kinds_c3_nosky", sky=None), 32, kind_of(*LIT))


def test_kind_one_colour_point_lights_16px(oracle):
    """C2's kind at 16-px bins: one vertex colour (no colour gathers), two point lights, no sun, a sampled sky."""
    run_case(oracle, sphere_scene("kinds_c2", POINTS[:2]), 16, kind_of("UCOL", "LIGHTS", "DEPTH", "SKYQ"), min_covered=200)


def test_kind_crowded_bin(oracle):
    """1682 triangles over about 28 x 28 px: a 32-px bin with more than 256 entries, whose keys carry primitive
    numbers, not queue positions (the pixel loop without the queue-position table)."""
    s = grid_scene("kinds_crowded", n=30, half=(0.9, 0.9), offset=(0.68, 0.0))
    run_case(oracle, s, 32, kind_of(*LIT, "SKYQ"), crowded=256)


def test_kind_near_clipped_triangle(oracle):
    """One triangle through the near plane: its pixels are shaded by the deferred loop from the clipper's records."""
    run_case(oracle, grid_scene("kinds_clip", near_tri=True), 32, kind_of(*LIT, "SKYQ"), clipped=1)


@pytest.mark.parametrize("name,lights", [("nosun", tuple(POINTS)), ("nolights", (SUN,))])
def test_fallback_light_rigs(oracle, name, lights):
    """Four point lights without a sun, and a sun without point lights: no kind is built, the generic instantiation."""
    run_case(oracle, grid_scene("kinds_fb_" + name, lights=lights), 32, None)


def test_fallback_one_colour_32px(oracle):
    """One vertex colour under the full light rig at 32-px bins: generic (its colour gathers are issued and unused)."""
    run_case(oracle, grid_scene("kinds_fb_ucol", one_colour=True), 32, None)


def test_fallback_sun_16px(oracle):
    """The sparse sphere under a sun and point lights: 16-px bins have no kind with a sun."""
    run_case(oracle, sphere_scene("kinds_fb_c2sun", (SUN, *POINTS[:2])), 16, None, min_covered=200)


def test_fallback_no_depth_target(oracle):
    """TRI_FLAG_NO_DEPTH_OUTPUT (the C-ABI's frame without a depth target): no kind without depth stores is built."""
    from trident_raster import abi

    run_case(oracle, grid_scene("kinds_fb_nodepth"), 32, None, flags=abi.TRI_FLAG_NO_DEPTH_OUTPUT, depth=False)
