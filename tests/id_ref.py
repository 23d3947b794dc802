"""The reference for the entity-id pass (include/tri_raster.h "entity ids"), from the oracle as it is.

For a scene with draws 0..n-1 let D be the oracle's depth of the full frame and D_d the oracle's depth of the scene
with draw d alone. Then

    expected(p) = 1 + max{ d : D_d(p) == D(p) and D_d(p) != 0x3F800000 },   or 0 when the set is empty:

LESS_OR_EQUAL in primitive order — among the draws that reach the minimum the last one wins. Condition: the geometry
stays well inside the far plane, so that a covered pixel never has depth bits 0x3F800000 (the cleared depth).

Also here: the outline rule restated in numpy (dilate the selected pixels by a (2r + 1)^2 box inside the rendered rows,
minus the selected pixels), the float64 src-over the outline's blend is held against, and the small pixel-space scenes
whose ids are known by construction.
"""
import copy

import numpy as np

import scene_cases as sc
from trident_raster import abi, scenes

BG = 0x3F800000
F = np.float32


def ids_from_depths(full, singles):
    """expected(p) from D (uint32 [rows, W]) and the list of D_d, in draw order."""
    ids = np.zeros(full.shape, np.uint32)
    for d, dd in enumerate(singles):
        assert dd.shape == full.shape
        hit = (dd == full) & (dd != BG)
        ids[hit] = d + 1  # ascending d: the last draw that reaches the minimum stays
    return ids


def only_draw(scene, d):
    """The scene with draw d alone; what only colour depends on (sky, shadow map, textures) is dropped."""
    s = copy.copy(scene)
    s.draws = [scene.draws[d]]
    s.skybox = None
    s.shadow = None
    s.textures = []
    s.name = f"{scene.name}[draw {d}]"
    return s


def expected_ids(oracle, scene, band=None, full_depth=None):
    """(expected ids, D) of a scene through oracle.render; full_depth: D when the caller rendered it already."""
    if full_depth is None:
        full_depth = oracle.render(scene, band=band)[1]
    singles = [oracle.render(only_draw(scene, d), band=band)[1] for d in range(len(scene.draws))]
    covered = full_depth != BG
    union = np.zeros_like(covered)
    for dd in singles:
        union |= dd != BG
    assert np.array_equal(union, covered), "a draw alone covers what the frame does not (or the reverse)"
    return ids_from_depths(full_depth, singles), full_depth


def outline_mask(ids, selected, r):
    """bool [rows, W]: the outline pixels of width r around the draws in `selected` (indices into the draw list)."""
    sel = np.isin(ids, np.asarray(sorted(set(selected)), np.int64) + 1) if len(selected) else np.zeros(ids.shape, bool)
    rows, w = ids.shape
    pad = np.zeros((rows + 2 * r, w + 2 * r), bool)
    pad[r:r + rows, r:r + w] = sel
    near = np.zeros(ids.shape, bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            near |= pad[dy:dy + rows, dx:dx + w]
    return near & ~sel


def colour_bytes(rgba):
    """The B8G8R8A8 bytes of a colour: clamp, * 255 + 0.5 in float32, truncate (unorm8)."""
    c = np.clip(np.asarray(rgba, F), F(0), F(1))
    b = (c * F(255.0) + F(0.5)).astype(np.int32).astype(np.uint8)
    return np.array([b[2], b[1], b[0], b[3]], np.uint8)


def src_over_f64(dst_bgra, rgba):
    """float64 src-over of `rgba` on B8G8R8A8 pixels [..., 4], as real numbers in 0..255 (not rounded)."""
    c = np.clip(np.asarray(rgba, np.float64), 0.0, 1.0)
    a = c[3]
    d = dst_bgra.astype(np.float64) / 255.0
    out = np.empty(d.shape, np.float64)
    out[..., 0] = c[2] * a + d[..., 0] * (1.0 - a)
    out[..., 1] = c[1] * a + d[..., 1] * (1.0 - a)
    out[..., 2] = c[0] * a + d[..., 2] * (1.0 - a)
    out[..., 3] = a + d[..., 3] * (1.0 - a)
    return out * 255.0


# ---- scenes -------------------------------------------------------------------------------------------------------
def pixel_quads(name, w, h, rects, seed=3):
    """One draw per rectangle (x0, y0, x1, y1, z): a front-facing screen-aligned quad at constant depth z under the
    exact orthographic pixel mapping of scene_cases._pixel_scene (world x, y in pixels). Corners on whole pixels cover
    exactly the pixels x0 <= px < x1, y0 <= py < y1, at depth bits float32(z)."""
    rng = np.random.default_rng(seed)
    tris = []
    for x0, y0, x1, y1, z in rects:
        c = [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
        tris += [[c[0], c[2], c[1]], [c[0], c[3], c[2]]]
    s = sc._pixel_scene(name, w, h, np.asarray(tris, np.float64), rng)
    n = len(rects)
    s.meshes = np.array([(6 * k, 6, 0, 0) for k in range(n)], abi.MESH_RANGE_DTYPE)
    s.draws = [abi.make_draw(k, np.eye(4, dtype=F), material_index=0,
                             tint=(0.3 + 0.7 * ((k * 5) % 7) / 6.0, 0.3 + 0.7 * ((k * 3) % 5) / 4.0, 0.9, 1.0)) for k in range(n)]
    return s


def ids_of_rects(w, h, rects, band=None):
    """The ids of pixel_quads by construction: nearer wins, the later draw among equals."""
    y0, y1 = band if band is not None else (0, h)
    ids = np.zeros((h, w), np.uint32)
    z = np.full((h, w), np.inf)
    for k, (x0, ry0, x1, ry1, zz) in enumerate(rects):
        box = np.zeros((h, w), bool)
        box[max(ry0, 0):max(ry1, 0), max(x0, 0):max(x1, 0)] = True
        win = box & (np.float32(zz) <= z)
        ids[win] = k + 1
        z[win] = np.float32(zz)
    return ids[y0:y1]


def hand_made(w=40, h=24):
    """Two quads of different depth and a third coincident with the second."""
    return [(2, 3, 30, 20, 0.5), (10, 1, 38, 12, 0.25), (10, 1, 38, 12, 0.25)]


def mesh_scene(name, w, h, parts, cam=(0.0, 0.0, 5.0), rot=(0.0, 0.0, 0.0), far=60.0):
    """parts: (vertices, indices, model) per draw, each its own mesh, index rows in draw order (the index route's
    layout); a perspective editor camera whose far plane lies well behind everything."""
    view, proj = scenes.editor_camera(cam, rot, 60.0, (w, h), 0.1, far)
    verts, idxs, meshes, draws = [], [], [], []
    vbase = ibase = 0
    for k, (v, i, model) in enumerate(parts):
        meshes.append((ibase, i.size, vbase, 0))
        verts.append(v)
        idxs.append(i)
        vbase += v.size
        ibase += i.size
        draws.append(abi.make_draw(k, model, material_index=0, tint=(1.0 - 0.2 * (k % 3), 0.5 + 0.15 * (k % 4), 0.7, 1.0)))
    return scenes.Scene(name, w, h, np.concatenate(verts), np.concatenate(idxs),
                        np.array(meshes, abi.MESH_RANGE_DTYPE), draws, scenes.pack_ubo(view, proj, cam, []),
                        materials=[((1, 1, 1, 1), (0.1, 0.6, 1.0, 0.0))])


def quad_mesh():
    v = np.zeros(4, abi.VERTEX_DTYPE)
    v["position"] = [(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)]
    v["normal"] = (0, 0, 1)
    v["color"] = 1.0
    v["texcoord"] = [(0, 0), (1, 0), (1, 1), (0, 1)]
    return v, np.array([0, 1, 2, 0, 2, 3], np.uint32)


def cubes_and_quad(w=100, h=70):
    """Two cubes in front of a quad: 26 triangles, sparse (16-px bins at 100 x 70)."""
    cv, ci = scenes.cube_mesh()
    qv, qi = quad_mesh()
    return mesh_scene("id_cubes_quad", w, h, [
        (qv, qi, scenes.compose_transform((0.0, 0.0, -1.0), (0, 0, 0), (3.2, 2.2, 1.0))),
        (cv, ci, scenes.compose_transform((-1.0, 0.2, 0.5), (25.0, 35.0, 10.0), (1.5, 1.5, 1.5))),
        (cv, ci, scenes.compose_transform((0.9, -0.3, 1.2), (-15.0, 50.0, 0.0), (1.2, 1.2, 1.2)))])


def sphere_and_quad(w=100, h=70, rings=16, segments=24):
    """A UV sphere of 2 * rings * segments triangles in front of a quad: dense (32-px bins at 100 x 70)."""
    sv, si = scenes.uv_sphere_mesh(rings, segments, 1.6)
    qv, qi = quad_mesh()
    return mesh_scene("id_sphere_quad", w, h, [
        (sv, si, scenes.compose_transform((0.3, 0.1, 0.5), (20.0, 30.0, 0.0), (1, 1, 1))),
        (qv, qi, scenes.compose_transform((-0.5, 0.0, -0.5), (0, 0, 0), (2.5, 2.5, 1.0)))])


def triangles(scene):
    """The primitives the frame holds: scene.triangles, passing over draws of meshes that do not exist."""
    return int(sum(int(scene.meshes[d.mesh_index]["index_count"]) // 3 for d in scene.draws
                   if d.mesh_index < len(scene.meshes)))


def with_skipped_draw(scene):
    """The scene's draws with a draw of a mesh that does not exist in the middle: the draws behind it keep their
    place in the caller's list."""
    s = copy.copy(scene)
    bad = abi.make_draw(len(scene.meshes) + 5, np.eye(4, dtype=F))
    s.draws = [scene.draws[0], bad] + list(scene.draws[1:])
    s.name = scene.name + "_skip"
    return s


def shared_mesh(w=100, h=70):
    """Three draws of ONE mesh: their index rows coincide, so the frame cannot take the index route (prim_vs)."""
    s = sc.depth_ties(w, h)
    s.draws = s.draws[:3]  # (the fourth pokes through the far plane)
    s.name = "id_shared_mesh"
    return s
