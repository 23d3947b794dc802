"""Parity scenes shared by the CPU golden tests and the GPU parity tests.

Each builder returns a trident_raster.scenes.Scene whose inputs are fully determined (Forge-style
camera/entities, reference primitive meshes restated by the oracle, procedural meshes)."""
import numpy as np

from trident_raster import abi, scenes

F = np.float32


def c1_cube(frame=0, w=640, h=480):
    return scenes.scene_c1_cube(frame, w, h)


def primitives_row(oracle, w=320, h=240):
    """Cube, sphere and quad primitives side by side (CreatePrimitiveEntity), editor camera (0,3,8)."""
    cam = (0.0, 3.0, 8.0)
    view, proj, fwd = oracle.editor_camera(cam, (0, 0, 0), 60.0, (w, h))
    verts, idxs, meshes = [], [], []
    vbase = ibase = 0
    for kind in (1, 2, 3):
        v, i = oracle.build_primitive(kind)
        meshes.append((ibase, i.size, vbase, len(meshes)))
        verts.append(v)
        idxs.append(i)
        vbase += v.size
        ibase += i.size
    m = np.array(meshes, dtype=abi.MESH_RANGE_DTYPE)
    draws = []
    for k, x in enumerate((-1.6, 0.0, 1.6)):
        model = oracle.compose_transform((x, 3.0, 3.0), (20.0 * k, 35.0 + 10 * k, 5.0 * k), (1.0, 1.0, 1.0))
        draws.append(abi.make_draw(k, model, texture_slot=0, material_index=k))
    ubo = oracle.pack_ubo(view, proj, cam, [])
    return scenes.Scene("primitives", w, h, np.concatenate(verts), np.concatenate(idxs), m, draws, ubo,
                        materials=[((1, 1, 1, 1), (0.0, 1.0, 1.0, 0.0))] * 3)


def sphere_c2(w=1920, h=1080, rings=125, segments=200, oracle=None):
    s = scenes.scene_c2_sphere(w, h, rings, segments)
    if oracle is not None:  # reference sphere builder restated by the oracle (glibc sin/cos)
        v, i = oracle.build_uv_sphere(rings, segments, 3.0)
        s.vertices, s.indices = v, i
        s.meshes = np.array([(0, i.size, 0, 0)], dtype=abi.MESH_RANGE_DTYPE)
    return s


def grid_c3(w=1280, h=720, n=200):
    return scenes.scene_c3_grid(w, h, n)


def checker_texture(wt=16, ht=8, seed=7):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, size=(ht, wt, 4), dtype=np.uint8)
    t[..., 3] = rng.integers(128, 256, size=(ht, wt), dtype=np.uint8)
    return t


def textured_grid(w=640, h=360, n=40):
    s = scenes.scene_c3_grid(w, h, n)
    s.textures = [(3, checker_texture())]
    s.draws = [abi.make_draw(0, np.eye(4, dtype=F), texture_slot=3, material_index=0, tint=(1.0, 0.9, 0.8, 0.75),
                             texture_scale=(1.5, 0.75), texture_offset=(0.1, -0.2), tiling=1.25)]
    return s


def near_clip_grid(w=640, h=480, n=60):
    """Camera pitched down over a ground plane that passes through the near plane and behind the
    eye: exercises homogeneous clipping (w <= 0, z < 0) and the guard band."""
    cam = (0.0, 0.35, 0.0)
    view, proj = scenes.editor_camera(cam, (-28.0, 12.0, 0.0), 70.0, (w, h), 0.1, 40.0)
    v, idx = scenes.displaced_grid_mesh(n, extent=(30.0, 30.0), depth=0.0, amplitude=0.15)
    # grid lies in x-y; rotate it to the x-z ground plane facing +y
    model = scenes.compose_transform((0.0, 0.0, -5.0), (-90.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    lights = [{"type": "point", "position": (0.5, 1.0, -2.0), "range": 6.0, "intensity": 8.0}]
    return scenes.Scene("near_clip", w, h, v, idx, np.array([(0, idx.size, 0, 0)], abi.MESH_RANGE_DTYPE),
                        [abi.make_draw(0, model, material_index=0)], scenes.pack_ubo(view, proj, cam, lights),
                        materials=[((0.8, 0.8, 0.8, 1.0), (0.5, 0.3, 1.0, 0.0))])


def depth_ties(w=256, h=256):
    """Two coplanar quads: the later draw must win every tie (LESS_OR_EQUAL), plus a far-plane
    straddling quad (per-pixel far clip)."""
    quad_v, quad_i = scenes.cube_mesh()  # reuse vertex layout; build a quad by hand below
    v = np.zeros(4, abi.VERTEX_DTYPE)
    v["position"] = [(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)]
    v["normal"] = (0, 0, 1)
    v["color"] = 1.0
    v["texcoord"] = [(0, 0), (1, 0), (1, 1), (0, 1)]
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    meshes = np.array([(0, 6, 0, 0)], abi.MESH_RANGE_DTYPE)
    cam = (0.0, 0.0, 4.0)
    view, proj = scenes.editor_camera(cam, (0, 0, 0), 60.0, (w, h), 0.1, 6.0)
    m1 = scenes.compose_transform((0, 0, 0), (0, 0, 0), (1, 1, 1))
    m2 = scenes.compose_transform((0.3, 0.2, 0), (0, 0, 0), (1, 1, 1))
    m3 = scenes.compose_transform((0.0, -0.5, -1.0), (70.0, 0, 0), (3, 3, 3))  # pokes past far = 6
    draws = [abi.make_draw(0, m1, tint=(1, 0.2, 0.2, 1)), abi.make_draw(0, m2, tint=(0.2, 1, 0.2, 1)),
             abi.make_draw(0, m1, tint=(0.2, 0.2, 1, 1)), abi.make_draw(0, m3, tint=(1, 1, 0.3, 1))]
    return scenes.Scene("depth_ties", w, h, v, idx, meshes, draws, scenes.pack_ubo(view, proj, cam, []),
                        materials=[((1, 1, 1, 1), (0.2, 0.5, 1.0, 0.0))])


def pixel_aligned_triangles(w=512, h=256, n=8000, seed=11):
    """Triangles whose vertices sit on quarter-pixel positions under an exact orthographic mapping (world
    x, y in pixels: the snap lands on them exactly), so edges run through pixel centres and their row
    crossings are exact integers — the boundary cases of k_raster's span walk (ceil/floor of -F/A, the
    top-left bias) — plus horizontal and vertical edges, slivers, and triangles on both sides of the
    64-px limit of the 32-bit edge set-up. Random depths overlap them (key resolve); both windings are
    emitted at random, so about half are culled. 8000 triangles over 512x256 keep the frame on 32x32 bins
    (choose_bin_grid: density >= 0.05), the bin size whose per-lane walk is the span walk."""
    rng = np.random.default_rng(seed)
    tris = []
    for k in range(n):
        kind = k % 6
        size = [3, 10, 40, 62, 70, 24][kind] * (0.5 + rng.random())
        cx, cy = rng.uniform(-20, w + 20), rng.uniform(-20, h + 20)
        if kind == 5:  # axis-aligned right triangle (one horizontal, one vertical edge)
            a, b = size * rng.choice([-1, 1]), size * rng.choice([-1, 1])
            p = [(cx, cy), (cx + a, cy), (cx, cy + b)]
        elif kind == 3 and k % 12 == 3:  # sliver
            p = [(cx, cy), (cx + size, cy + 0.25 * rng.integers(1, 4)), (cx + size * 0.5, cy + 0.25)]
        else:
            p = [(cx + size * rng.uniform(-1, 1), cy + size * rng.uniform(-1, 1)) for _ in range(3)]
        q = np.round(np.asarray(p, np.float64) * 4.0) / 4.0  # quarter pixels: exact in float and on the snap
        z = rng.uniform(0.05, 0.95, size=3)
        if rng.random() < 0.3:
            z[:] = z[0]  # flat: depth ties between overlapping flat triangles at equal depth are rarer but exact
        tris.append([(q[i, 0], q[i, 1], z[i]) for i in range(3)])
    v = np.zeros(3 * n, abi.VERTEX_DTYPE)
    v["position"] = np.asarray(tris, F).reshape(-1, 3)
    v["normal"] = (0, 0, 1)
    v["color"] = rng.uniform(0.2, 1.0, size=(3 * n, 3)).astype(F)
    v["texcoord"] = rng.uniform(0, 1, size=(3 * n, 2)).astype(F)
    idx = np.arange(3 * n, dtype=np.uint32)
    meshes = np.array([(0, idx.size, 0, 0)], abi.MESH_RANGE_DTYPE)
    view = np.eye(4, dtype=F)
    proj = np.eye(4, dtype=F)  # [col][row]: clip = (2x/W - 1, 2y/H - 1, z, 1), powers of two, products exact
    proj[0, 0], proj[3, 0] = F(2.0 / w), F(-1.0)
    proj[1, 1], proj[3, 1] = F(2.0 / h), F(-1.0)
    cam = (w / 2.0, h / 2.0, 50.0)
    draws = [abi.make_draw(0, np.eye(4, dtype=F), material_index=0)]
    return scenes.Scene("pixel_aligned", w, h, v, idx, meshes, draws, scenes.pack_ubo(view, proj, cam, []),
                        materials=[((1, 1, 1, 1), (0.1, 0.5, 1.0, 0.0))])


def large_quads(w=1920, h=1080, one_draw=False):
    """Screen-filling quads over 1920x1080 (2040 bins of 32x32): a set-up round whose bins span more than
    k_setup's 1024-cell LDS grid, so binning takes the per-wave reservation path."""
    s = depth_ties(w, h)
    big = scenes.compose_transform((0.0, 0.0, 0.0), (0, 0, 0), (3.5, 3.5, 1.0))
    tilted = scenes.compose_transform((0.4, -0.3, 0.5), (25.0, 35.0, 0), (2.5, 2.5, 1.0))
    s.draws = [abi.make_draw(0, big, tint=(1, 0.3, 0.2, 1))] if one_draw else \
        [abi.make_draw(0, big, tint=(1, 0.3, 0.2, 1)), abi.make_draw(0, tilted, tint=(0.2, 0.9, 0.4, 1))]
    s.name = "large_quads_1" if one_draw else "large_quads_2"
    return s


def skinned_quad(oracle, w=256, h=256):
    """GPU skinning branch (Default.vert:64-85): 2-bone palette at an offset, weights per vertex,
    one out-of-range bone index (skipped)."""
    v, i = oracle.build_primitive(3)
    v["bone_indices"] = [(0, 1, 0, 0), (1, 0, 0, 0), (0, 5, 0, 0), (1, 1, 0, 0)]
    v["bone_weights"] = [(0.75, 0.25, 0, 0), (1.0, 0, 0, 0), (0.6, 0.4, 0, 0), (0.5, 0.5, 0, 0)]
    bones = np.stack([np.eye(4, dtype=F).reshape(16),
                      np.eye(4, dtype=F).reshape(16),
                      oracle.compose_transform((0.2, 0.1, 0.0), (0, 0, 25.0), (1.2, 0.9, 1.0)).reshape(16)])
    cam = (0.0, 0.0, 2.0)
    view, proj, _ = oracle.editor_camera(cam, (0, 0, 0), 60.0, (w, h))
    model = oracle.compose_transform((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1, 1, 1))
    d = abi.make_draw(0, model, bone_offset=1, bone_count=2)
    return scenes.Scene("skinned", w, h, v, i, np.array([(0, i.size, 0, 0)], abi.MESH_RANGE_DTYPE), [d],
                        oracle.pack_ubo(view, proj, cam, []), materials=[], bones=bones)


def invalid_inputs(oracle, w=200, h=150):
    """Bad mesh index, out-of-range vertex index, empty mesh: silently skipped (Renderer.cpp:2946-2956,
    :5118-5127); the valid cube still renders."""
    v, i = oracle.build_primitive(1)
    bad = np.concatenate([i, np.array([0, 1, 999], np.uint32)])
    meshes = np.array([(0, i.size, 0, 0), (i.size, 3, 0, 0), (0, 0, 0, 0)], abi.MESH_RANGE_DTYPE)
    cam = (0.0, 0.0, 3.0)
    view, proj, _ = oracle.editor_camera(cam, (0, 0, 0), 60.0, (w, h))
    model = oracle.compose_transform((0.0, 0.0, 0.0), (30.0, 40.0, 0.0), (1, 1, 1))
    draws = [abi.make_draw(7, model), abi.make_draw(1, model), abi.make_draw(2, model), abi.make_draw(0, model)]
    return scenes.Scene("invalid", w, h, v, bad, meshes, draws, oracle.pack_ubo(view, proj, cam, []))


def empty_scene(w=128, h=96):
    view, proj = scenes.editor_camera((0, 0, 5), (0, 0, 0), 60.0, (w, h))
    return scenes.Scene("empty", w, h, np.zeros(0, abi.VERTEX_DTYPE), np.zeros(0, np.uint32),
                        np.zeros(0, abi.MESH_RANGE_DTYPE), [], scenes.pack_ubo(view, proj, (0, 0, 5)),
                        clear=(0.1, 0.2, 0.3, 1.0))


# ---- skybox ----------------------------------------------------------------
SOLID_0x808080 = scenes.DEFAULT_SKYBOX  # CreateSolidColor(0x808080)


def cubemap_faces(n=16, seed=11):
    """A cubemap whose faces are distinct seeded gradients with noise (exercises filtering and the
    seamless edges), uint8 [6, n, n, 4] sRGB, faces +X,-X,+Y,-Y,+Z,-Z."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32) / max(n - 1, 1)
    faces = np.empty((6, n, n, 4), np.uint8)
    for f in range(6):
        base = rng.integers(30, 200, size=3)
        g = np.stack([base[0] + 50 * xx, base[1] + 50 * yy, base[2] + 25 * (xx + yy)], -1)
        g += rng.integers(-8, 9, size=g.shape)
        faces[f, ..., :3] = np.clip(g, 0, 255).astype(np.uint8)
        faces[f, ..., 3] = 255
    return faces


def skybox_only(w=320, h=240, fov=100.0, rot=(0.0, 0.0, 0.0), faces=None):
    """No meshes: every pixel is the skybox pass (Renderer.cpp:5076-5082 before any mesh draw)."""
    s = scenes.scene_c1_cube(0, w, h)
    view, proj = scenes.editor_camera((0.0, 3.0, 8.0), rot, fov, (w, h), 0.1, 1000.0)
    s.ubo = scenes.pack_ubo(view, proj, (0.0, 3.0, 8.0))
    s.draws = []
    s.name = f"skybox_only_{w}x{h}_fov{fov:g}"
    s.skybox = cubemap_faces() if faces is None else faces
    return s


def c1_cube_skybox(frame=1, w=640, h=480):
    s = scenes.scene_c1_cube(frame, w, h)
    s.skybox = cubemap_faces(32, seed=5)
    s.name = "c1_cube_skybox"
    return s


# ---- shadow-map pre-pass (BASELINE C5; tri_set_shadow) ------------------------------
def shadow_scene(oracle, w=480, h=320, size=256, sun=(-0.45, -1.0, -0.35), bias=0.001, slope=2.0):
    """A ground quad under a floating cube and sphere, lit by a shadow-casting sun (plus one point
    light): the primitives (Renderer.cpp:72-246) as Forge spawns them, light frustum fitted by
    tri_shadow_fit_ortho over the draws' world box."""
    cam = (0.0, 4.0, 8.0)
    view, proj, _ = oracle.editor_camera(cam, (-25.0, 0.0, 0.0), 60.0, (w, h))
    verts, idxs, meshes = [], [], []
    vbase = ibase = 0
    for kind in (1, 2, 3):
        v, i = oracle.build_primitive(kind)
        meshes.append((ibase, i.size, vbase, len(meshes)))
        verts.append(v)
        idxs.append(i)
        vbase += v.size
        ibase += i.size
    m = np.array(meshes, dtype=abi.MESH_RANGE_DTYPE)
    draws = [
        abi.make_draw(2, oracle.compose_transform((0.0, 0.0, 0.0), (-90.0, 0.0, 0.0), (12.0, 12.0, 1.0)), material_index=0),
        abi.make_draw(0, oracle.compose_transform((-1.2, 1.4, 0.5), (15.0, 30.0, 0.0), (1.2, 1.2, 1.2)), material_index=0),
        abi.make_draw(1, oracle.compose_transform((1.3, 1.0, -0.4), (0.0, 0.0, 0.0), (1.6, 1.6, 1.6)), material_index=0),
    ]
    lights = [{"type": "directional", "direction": sun, "intensity": 4.0},
              {"type": "point", "position": (2.0, 2.5, 2.0), "range": 7.0, "intensity": 3.0}]
    s = scenes.Scene("shadow", w, h, np.concatenate(verts), np.concatenate(idxs), m, draws,
                     oracle.pack_ubo(view, proj, cam, lights), materials=[((0.9, 0.85, 0.8, 1.0), (0.1, 0.6, 1.0, 0.0))],
                     skybox=SOLID_0x808080)
    return scenes.with_shadow(s, size, bias, slope)


def near_clip_multi(w=640, h=480, n=60, identity=False, shadow=False):
    """near_clip_grid as two textured draws (the grid's index halves, each with its own sRGB slot): clipped primitives
    on a frame outside the single-draw solid instantiation (obj48's object records through the clipper). identity:
    the ground-plane rotation baked into the vertices, so both draws have identity models (the C5 case); otherwise
    the second draw carries its own translation on top of the rotation (a per-draw transform per pixel)."""
    s = near_clip_grid(w, h, n)
    model = np.array(s.draws[0].pc.model, F).reshape(4, 4)  # [col][row]
    if identity:
        v = s.vertices.copy()
        p = v["position"].astype(F)
        nn = v["normal"].astype(F)
        v["position"] = (p @ model[:3, :3] + model[3, :3]).astype(F)
        v["normal"] = (nn @ model[:3, :3]).astype(F)
        s.vertices = v
        m0 = m1 = np.eye(4, dtype=F)
    else:
        m0 = model
        m1 = scenes.compose_transform((0.4, 0.05, -5.3), (-90.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    half = (s.indices.size // 6) * 3
    s.meshes = np.array([(0, half, 0, 0), (half, s.indices.size - half, 0, 0)], abi.MESH_RANGE_DTYPE)
    s.textures = [(1, checker_texture(16, 8, 3)), (2, checker_texture(8, 16, 4))]
    s.draws = [abi.make_draw(0, m0, texture_slot=1, material_index=0),
               abi.make_draw(1, m1, texture_slot=2, material_index=0)]
    s.ubo = scenes.pack_ubo(*scenes.editor_camera((0.0, 0.35, 0.0), (-28.0, 12.0, 0.0), 70.0, (w, h), 0.1, 40.0),
                            (0.0, 0.35, 0.0), [{"type": "directional", "direction": (-0.3, -1.0, -0.2), "intensity": 3.0},
                                               {"type": "point", "position": (0.5, 1.0, -2.0), "range": 6.0,
                                                "intensity": 8.0}])
    s.name = f"near_clip_multi{'_id' if identity else ''}{'_shadow' if shadow else ''}"
    if shadow:
        scenes.with_shadow(s, 512)
    return s


def near_clip_single(w=640, h=480, n=60, shadow=False):
    """near_clip_grid as ONE textured draw (a non-1x1 sRGB slot, the identity uv transform, the ground-plane rotation
    as its model): a single-draw frame outside the solid instantiation, so k_setup runs its single-draw form while
    k_vertex writes no varyings (obj48). The clipper must read the geometry's input records."""
    s = near_clip_grid(w, h, n)
    model = np.array(s.draws[0].pc.model, F).reshape(4, 4)
    s.textures = [(1, checker_texture(16, 8, 3))]
    s.draws = [abi.make_draw(0, model, texture_slot=1, material_index=0)]
    s.name = f"near_clip_single{'_shadow' if shadow else ''}"
    if shadow:
        scenes.with_shadow(s, 512)
    return s


# ---- raster paths chosen by a threshold (frame size, density, a queue capacity) --------------------
def expected_bin_size(w, band_rows, h, nprims):
    """The bin grid tri_render chooses (choose_bin_grid, restated): 64-px bins once the context would hold more than
    16384 bins of 32 px; 16-px bins on small grids (fewer than 4096 bins of 32 px) of sparse frames (fewer than 0.05
    triangles per pixel of the WHOLE frame, while the bins count the band's rows only); 32-px bins otherwise."""
    n32 = -(-w // 32) * -(-band_rows // 32)
    if n32 > 16384:
        return 64
    if n32 < 4096 and nprims / (w * h) < 0.05:
        return 16
    return 32


def counted_triangles(w=320, h=240, ntris=3840):
    """The spinning cube's twelve triangles repeated up to exactly `ntris` primitives: a frame whose only
    interesting property is its primitive count (the density threshold of the bin grid)."""
    s = scenes.scene_c1_cube(1, w, h)
    s.indices = np.tile(s.indices, -(-ntris // 12))[:3 * ntris].copy()
    s.meshes = np.array([(0, 3 * ntris, 0, 0)], abi.MESH_RANGE_DTYPE)
    s.skybox = None
    s.name = f"counted_{ntris}"
    return s


def _pixel_scene(name, w, h, pos, rng):
    """World x, y in pixels under the orthographic mapping of pixel_aligned_triangles; pos: float [n, 3, 3]."""
    n = pos.shape[0]
    v = np.zeros(3 * n, abi.VERTEX_DTYPE)
    v["position"] = np.asarray(pos, F).reshape(-1, 3)
    v["normal"] = (0, 0, 1)
    v["color"] = rng.uniform(0.2, 1.0, size=(3 * n, 3)).astype(F)
    v["texcoord"] = rng.uniform(0, 1, size=(3 * n, 2)).astype(F)
    idx = np.arange(3 * n, dtype=np.uint32)
    meshes = np.array([(0, idx.size, 0, 0)], abi.MESH_RANGE_DTYPE)
    view = np.eye(4, dtype=F)
    proj = np.eye(4, dtype=F)
    proj[0, 0], proj[3, 0] = F(2.0 / w), F(-1.0)
    proj[1, 1], proj[3, 1] = F(2.0 / h), F(-1.0)
    cam = (w / 2.0, h / 2.0, 50.0)
    draws = [abi.make_draw(0, np.eye(4, dtype=F), material_index=0)]
    return scenes.Scene(name, w, h, v, idx, meshes, draws, scenes.pack_ubo(view, proj, cam, []),
                        materials=[((1, 1, 1, 1), (0.1, 0.5, 1.0, 0.0))])


def snapped_xy(scene):
    """The 24.8 fixed-point vertex positions of an orthographic single-draw scene with identity model and view,
    recomputed in float32 from DESIGN §4's rules: clip = P * p summed term by term, x_d = x_c * (1 / w_c),
    x_f = x_d * W/2 + W/2, X = rint(x_f * 256). Returns int64 X, Y per vertex record."""
    P = np.array(scene.ubo.projection, F).reshape(4, 4)  # [col][row]
    p = scene.vertices["position"].astype(F)
    out = []
    for row, half in ((0, F(scene.width) * F(0.5)), (1, F(scene.height) * F(0.5))):
        c = F(P[0, row]) * p[:, 0]
        c = (c + F(P[1, row]) * p[:, 1]).astype(F)
        c = (c + F(P[2, row]) * p[:, 2]).astype(F)
        c = (c + F(P[3, row])).astype(F)
        f = ((c * F(1.0)).astype(F) * half + half).astype(F)
        out.append(np.rint((f * F(256.0)).astype(F)).astype(np.int64))
    return out[0], out[1]


def bin_entry_counts(scene, bin_px, big_area=96):
    """Per bin of bin_px pixels: how many set-up triangles (front-facing, a pixel centre inside the bounding box,
    as DESIGN §4 sets a triangle up) an orthographic scene queues there, and how many of them are 'large' there
    (bounding box inside the bin above big_area pixels). Counted from the snapped vertices alone."""
    X, Y = snapped_xy(scene)
    t = scene.indices.reshape(-1, 3).astype(np.int64)
    X, Y = X[t], Y[t]
    S = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    px0 = np.maximum(-((128 - X.min(1)) >> 8), 0)
    px1 = np.minimum((X.max(1) - 128) >> 8, scene.width - 1)
    py0 = np.maximum(-((128 - Y.min(1)) >> 8), 0)
    py1 = np.minimum((Y.max(1) - 128) >> 8, scene.height - 1)
    keep = (S < 0) & (px0 <= px1) & (py0 <= py1)
    nbx, nby = -(-scene.width // bin_px), -(-scene.height // bin_px)
    total = np.zeros((nby, nbx), np.int64)
    large = np.zeros((nby, nbx), np.int64)
    for a0, a1, b0, b1 in zip(px0[keep], px1[keep], py0[keep], py1[keep]):
        for by in range(b0 // bin_px, b1 // bin_px + 1):
            for bx in range(a0 // bin_px, a1 // bin_px + 1):
                total[by, bx] += 1
                cw = min(a1, bx * bin_px + bin_px - 1) - max(a0, bx * bin_px) + 1
                ch = min(b1, by * bin_px + bin_px - 1) - max(b0, by * bin_px) + 1
                large[by, bx] += cw * ch > big_area
    return total, large


def crowded_regions(w, h, bin_px=64):
    """An interior bin, one in the last (ragged) column, one in the last row and the corner bin, as (bx, by)."""
    nbx, nby = -(-w // bin_px), -(-h // bin_px)
    return [(nbx // 3, nby // 3), (nbx - 1, nby // 2), (nbx // 2, nby - 1), (nbx - 1, nby - 1)]


def crowded_bins(w=4100, h=4100, regions=None, per_region=640, seed=5, stack=1100, bin_px=64):
    """Bins that hold far more entries than a workgroup has lanes, in the style of pixel_aligned_triangles
    (orthographic, quarter-pixel vertices, random depths): per_region small triangles (2-12 px, both windings, so
    more are emitted than survive the cull) centred inside the frame's part of each listed bin_px region, and over
    the first region a stack of `stack` front-facing quads that each fill the bin (2 * stack large triangles in one
    bin: more than the large-triangle queue of any instantiation holds, so the rest take the per-lane fallback).
    Every region exceeds the initial per-bin capacity of the bin list (256 entries)."""
    rng = np.random.default_rng(seed)
    regions = crowded_regions(w, h, bin_px) if regions is None else regions
    tris = []
    for bx, by in regions:
        x0, y0 = bx * bin_px, by * bin_px
        x1, y1 = min(x0 + bin_px, w), min(y0 + bin_px, h)
        made = 0
        while made < per_region:
            size = rng.uniform(2.0, 12.0)
            cx, cy = rng.uniform(x0 + 0.5, x1 - 0.5), rng.uniform(y0 + 0.5, y1 - 0.5)
            p = np.array([(cx + size * rng.uniform(-0.5, 0.5), cy + size * rng.uniform(-0.5, 0.5)) for _ in range(3)])
            q = np.round(p * 4.0) / 4.0
            S = (q[1, 0] - q[0, 0]) * (q[2, 1] - q[0, 1]) - (q[1, 1] - q[0, 1]) * (q[2, 0] - q[0, 0])
            z = rng.uniform(0.05, 0.95, size=3)
            tris.append([(q[i, 0], q[i, 1], z[i]) for i in range(3)])
            # a front-facing triangle whose box holds a pixel centre of the region's own pixels is an entry
            inside = (np.floor(q[:, 0].max() - 0.5) >= np.ceil(max(q[:, 0].min(), x0) - 0.5)) and \
                     (np.floor(q[:, 1].max() - 0.5) >= np.ceil(max(q[:, 1].min(), y0) - 0.5)) and \
                     np.ceil(q[:, 0].min() - 0.5) <= x1 - 1 and np.ceil(q[:, 1].min() - 0.5) <= y1 - 1
            made += bool(S < 0 and inside)
    bx, by = regions[0]
    for _ in range(stack):
        j = rng.integers(0, 33, size=4) * 0.25  # the quad overhangs the bin by 0 .. 8 px on each side
        x0, y0 = bx * bin_px - j[0], by * bin_px - j[1]
        x1, y1 = bx * bin_px + bin_px + j[2], by * bin_px + bin_px + j[3]
        z = rng.uniform(0.05, 0.95, size=4)
        c = [(x0, y0, z[0]), (x1, y0, z[1]), (x1, y1, z[2]), (x0, y1, z[3])]
        tris.append([c[0], c[2], c[1]])
        tris.append([c[0], c[3], c[2]])
    order = rng.permutation(len(tris))  # large and small entries interleaved in primitive order
    s = _pixel_scene("crowded_bins", w, h, np.asarray(tris, np.float64)[order], rng)
    return s


def stacked_quads(w, h, n=1100, draws=1, textured=False, seed=9, box=None):
    """n front-facing quads (2 n large triangles) stacked over one box of the frame (default: the 40 x 40 px around
    its centre, overhanging by up to 6 px), random per-vertex depths: one bin holds more large triangles than the
    large-triangle queue of any instantiation (192, 512 or 1024 entries) and more entries than the initial bin-list
    capacity. draws > 1 splits the index range into that many draws."""
    rng = np.random.default_rng(seed)
    bx0, by0, bx1, by1 = box if box is not None else (w // 2 - 20, h // 2 - 20, w // 2 + 20, h // 2 + 20)
    tris = []
    for _ in range(n):
        j = rng.integers(0, 25, size=4) * 0.25
        x0, y0, x1, y1 = bx0 - j[0], by0 - j[1], bx1 + j[2], by1 + j[3]
        z = rng.uniform(0.05, 0.95, size=4)
        c = [(x0, y0, z[0]), (x1, y0, z[1]), (x1, y1, z[2]), (x0, y1, z[3])]
        tris.append([c[0], c[2], c[1]])
        tris.append([c[0], c[3], c[2]])
    s = _pixel_scene(f"stacked_quads_{draws}", w, h, np.asarray(tris, np.float64), rng)
    if draws > 1:
        cuts = [(k * 2 * n // draws) * 3 for k in range(draws + 1)]
        s.meshes = np.array([(a, b - a, 0, 0) for a, b in zip(cuts[:-1], cuts[1:])], abi.MESH_RANGE_DTYPE)
        s.draws = [abi.make_draw(k, np.eye(4, dtype=F), material_index=0,
                                 tint=(1.0 - 0.1 * k, 0.6 + 0.1 * k, 0.8, 1.0)) for k in range(draws)]
    if textured:
        s.textures = [(2, checker_texture(8, 16, 4))]
        for d in s.draws:
            d.pc.texture_slot = 2
    return s


# ---- dense homogeneous clipping ----------------------------------------------------------------------
CLIP_WMIN, CLIP_GUARD_PX = 1e-5, 16000.0  # the clip planes of DESIGN §4: w >= 1e-5, z >= 0, |x_fb|, |y_fb| <= 16000 px


def clip_polygon_sizes(scene):
    """Float64 Sutherland-Hodgman over the six clip planes (w >= WMIN, z >= 0, the guard band), per triangle of
    the scene that is not trivially rejected and has a vertex outside a plane: the clipped polygon's vertex
    count (0: nothing left). Written from the plane list alone, after tests/test_oracle_clip_f64.py's clipper."""
    W, H = scene.width, scene.height
    gx, gy = 2.0 * CLIP_GUARD_PX / W - 1.0, 2.0 * CLIP_GUARD_PX / H - 1.0
    planes = [lambda c: c[3] - CLIP_WMIN, lambda c: c[2], lambda c: c[0] + gx * c[3], lambda c: gx * c[3] - c[0],
              lambda c: c[1] + gy * c[3], lambda c: gy * c[3] - c[1]]
    reject = [lambda c: c[2], lambda c: c[3] - c[2], lambda c: c[0] + c[3], lambda c: c[3] - c[0],
              lambda c: c[1] + c[3], lambda c: c[3] - c[1]]
    view = np.array(scene.ubo.view, np.float64).reshape(4, 4).T
    proj = np.array(scene.ubo.projection, np.float64).reshape(4, 4).T
    pos = scene.vertices["position"].astype(np.float64)
    sizes = []
    for d in scene.draws:
        m = scene.meshes[d.mesh_index]
        mvp = proj @ view @ np.array(d.pc.model, np.float64).reshape(4, 4).T
        first, count, base = int(m["first_index"]), int(m["index_count"]), int(m["base_vertex"])
        tri = scene.indices[first:first + count - count % 3].reshape(-1, 3).astype(np.int64) + base
        clip = np.concatenate([pos, np.ones((pos.shape[0], 1))], 1) @ mvp.T
        for t in tri:
            c = [clip[i] for i in t]
            if any(all(f(v) < 0 for v in c) for f in reject):
                continue
            if all(f(v) >= 0 for v in c for f in planes):
                continue
            poly = c
            for f in planes:
                out = []
                for i in range(len(poly)):
                    a, b = poly[i], poly[(i + 1) % len(poly)]
                    da, db = f(a), f(b)
                    if da >= 0:
                        out.append(a)
                    if (da >= 0) != (db >= 0):
                        out.append(a + da / (da - db) * (b - a))
                poly = out
                if not poly:
                    break
            sizes.append(len(poly))
    return np.array(sizes, np.int64)


def dense_clip(w=320, h=240, cells=36, size=(3.0, 30.0), pairs=True, guard=True, seed=21, two_behind=True):
    """Thousands of small triangles cut by the near plane, interleaved on screen with unclipped ones.

    The camera sits at the origin looking down -z (world space is view space), near plane 0.1. Each of cells x cells
    jittered screen cells gets one triangle of size[0] .. size[1] pixels with one vertex behind the near plane and two
    in front of it (a 4-vertex polygon, two fan sub-triangles) and, with pairs, an unclipped triangle of like size
    overlapping it just beyond the plane, so bin rows hold both kinds. About four in five face the camera; with
    two_behind every fifth clipped one has two vertices behind the plane (a 3-vertex polygon). With guard, two more groups follow:
    16 slivers that reach beyond an x and a y guard-band plane (near + guard planes: 5-vertex polygons, fan
    sub-triangles 1..3), and four frame-filling sheets behind everything, cut by the near plane and all four guard
    planes (8 vertices, sub-triangles 1..6), so every pixel of the frame has a clipped fragment under the small
    triangles. TRI_MAX_CLIP_POLY = 9 vertices are out of reach of a scene: the sixth plane, w >= 1e-5, adds a vertex
    only where it cuts off a corner that the guard planes |x|, |y| <= g w leave, and those meet at w = 0, so its edge
    would be at most 2 g 1e-5 clip units long (and under a perspective projection z >= 0 implies w >= near)."""
    rng = np.random.default_rng(seed)
    fov, near, far = 70.0, 0.1, 40.0
    th = near * np.tan(np.radians(fov) / 2.0)  # half-height of the near rectangle
    tw = th * w / h
    px = 2.0 * th / h  # one pixel at the near plane, in world units

    def facing(p):
        """float [n, 3, 3] triangles: counter-clockwise as the camera sees them with probability 0.8 (the perspective
        divide keeps the sense of a triangle's part in front of the eye)."""
        q = p[..., :2] / -p[..., 2:3]
        ccw = (q[:, 1, 0] - q[:, 0, 0]) * (q[:, 2, 1] - q[:, 0, 1]) - (q[:, 1, 1] - q[:, 0, 1]) * (q[:, 2, 0] - q[:, 0, 0]) > 0
        flip = ccw != (rng.random(p.shape[0]) < 0.8)
        p[flip] = p[flip][:, [0, 2, 1]]
        return p

    n = cells * cells
    u = rng.random((13, n))
    jj, ii = np.divmod(np.arange(n), cells)
    cx = (-1.0 + 2.0 * (ii + 0.2 + 0.6 * u[0]) / cells) * tw
    cy = (-1.0 + 2.0 * (jj + 0.2 + 0.6 * u[1]) / cells) * th
    s = (size[0] + (size[1] - size[0]) * u[2]) * px
    ang = 2 * np.pi * u[3]
    zb = -(near - (0.002 + 0.008 * u[4])) * np.ones(n)  # behind the near plane
    behind = np.stack([cx, cy, zb], -1)
    front = [np.stack([cx + s * np.cos(ang + a), cy + s * np.sin(ang + a), -(near + 0.002 + 0.01 * u[5 + k])], -1)
             for k, a in enumerate((-0.5, 0.5))]
    clipped = np.stack([behind, front[0], front[1]], 1)
    if two_behind:  # every fifth: two vertices behind, one in front (a 3-vertex polygon)
        k5 = np.arange(n) % 5 == 4
        clipped[k5] = np.stack([front[0], np.stack([cx - 0.3 * s, cy + 0.2 * s, zb], -1), behind], 1)[k5]
    groups = [facing(clipped)]
    if pairs:  # an unclipped triangle of like size over each clipped one, just beyond the plane
        zz = -(near + 0.004 + 0.016 * u[7])
        s2 = (size[0] + (size[1] - size[0]) * u[8]) * px * (-zz / near)
        a2 = 2 * np.pi * u[9]
        ox, oy = (0.6 * u[10] - 0.3) * s, (0.6 * u[11] - 0.3) * s
        dz = 0.004 * rng.random((3, n))
        groups.append(facing(np.stack([np.stack([cx + ox + s2 * np.cos(a2 + a), cy + oy + s2 * np.sin(a2 + a), zz - dz[k]], -1)
                                       for k, a in enumerate((0.0, 2.1, 4.2))], 1)))
    tris = list(np.stack(groups, 1).reshape(-1, 3, 3))  # clipped, unclipped, clipped, ... in primitive order

    def facing1(p):
        return [tuple(q) for q in facing(np.array(p, np.float64)[None])[0]]

    if guard:
        gx, gy = 2.0 * CLIP_GUARD_PX / w - 1.0, 2.0 * CLIP_GUARD_PX / h - 1.0
        f = 1.0 / np.tan(np.radians(fov) / 2.0)
        wb = near + 0.05  # clip w of the far vertices

        def at_ndc(nx, ny, cw):  # the view-space point of clip w cw that projects to (nx, ny)
            return np.array([nx * cw * (w / h) / f, ny * cw / f, -cw])

        for k in range(16):  # slivers: near + one x and one y guard plane
            sx, sy = (1, -1)[k & 1], (1, -1)[(k >> 1) & 1]
            B = at_ndc(sx * 1.2 * gx, sy * 0.9 * gy, wb)
            C = at_ndc(sx * 0.9 * gx, sy * 1.2 * gy, wb)
            t = 0.01
            P = np.array([rng.uniform(-0.7, 0.7) * tw, rng.uniform(-0.7, 0.7) * th, -near])
            A = (P - t * 0.5 * (B + C)) / (1.0 - t)
            A[2] = -(near - t / (1.0 - t) * 0.05)
            tris.append(facing1([A, B, C]))
        # Four sheets behind everything else, each cut by the near plane and all four guard planes (8 vertices). In
        # guard-band units the visible part of a sheet projects to the quadrilateral N1 (0, -1.5), B (1.5, 0.3),
        # C (0.3, 1.5), N2 (-1.5, 0), whose every corner lies outside the guard square while every edge crosses it; N1
        # and N2 are where the edges from B and C towards A meet the near plane. A lies behind the eye (w < 0) and
        # projects to A' = (7.5, 7.5) = N1 + 5 (B - N1) = N2 + 5 (C - N2), so with w_B = w_C = 0.3 the near plane is
        # met at t * w_B = 1.25 * near, (1 - t) * w_A = -0.25 * near. The four are quarter turns of one sheet about
        # the view axis: the same depth at the frame's centre, tilted four ways, so each shows in a part of the frame;
        # their vertex order rotates, so the fan's first vertex differs.
        ws = 0.3
        t = 1.25 * near / ws
        wa = -0.25 * near / (1.0 - t)
        for k in range(4):
            rot = [lambda x, y: (x, y), lambda x, y: (-y, x), lambda x, y: (-x, -y), lambda x, y: (y, -x)][k]
            p = [at_ndc(*(np.array(rot(x, y)) * (gx, gy)), cw) for x, y, cw in ((7.5, 7.5, wa), (1.5, 0.3, ws), (0.3, 1.5, ws))]
            p = [tuple(q) for q in p]
            tris.append(p[k % 3:] + p[:k % 3])  # counter-clockwise as built: quarter turns keep the sense
    n = len(tris)
    v = np.zeros(3 * n, abi.VERTEX_DTYPE)
    v["position"] = np.asarray(tris, F).reshape(-1, 3)
    v["normal"] = (0, 0, 1)
    v["color"] = rng.uniform(0.3, 1.0, size=(3 * n, 3)).astype(F)
    v["texcoord"] = rng.uniform(0, 2, size=(3 * n, 2)).astype(F)
    idx = np.arange(3 * n, dtype=np.uint32)
    cam = (0.0, 0.0, 0.0)
    view, proj = scenes.editor_camera(cam, (0.0, 0.0, 0.0), fov, (w, h), near, far)
    lights = [{"type": "directional", "direction": (-0.3, -0.4, -1.0), "intensity": 3.0},
              {"type": "point", "position": (0.02, 0.03, 0.0), "range": 1.0, "intensity": 4.0}]
    return scenes.Scene(f"dense_clip_{w}x{h}_{cells}", w, h, v, idx, np.array([(0, idx.size, 0, 0)], abi.MESH_RANGE_DTYPE),
                        [abi.make_draw(0, np.eye(4, dtype=F), material_index=0)],
                        scenes.pack_ubo(view, proj, cam, lights), materials=[((0.9, 0.9, 0.9, 1.0), (0.3, 0.5, 1.0, 0.0))])


def dense_clip_multi(w=320, h=240, shadow=False, **kw):
    """dense_clip as three textured draws over thirds of its index range, the second and third under small
    translations of their own (the clipper reads prim_vs and the draw carried in the record); shadow: with the
    pre-pass for the scene's sun (the clipper interpolates light-space positions)."""
    s = dense_clip(w, h, **kw)
    n = s.indices.size // 3
    cuts = [0, (n // 3) * 3, (2 * n // 3) * 3, n * 3]
    s.meshes = np.array([(a, b - a, 0, 0) for a, b in zip(cuts[:-1], cuts[1:])], abi.MESH_RANGE_DTYPE)
    s.textures = [(1, checker_texture(16, 8, 3)), (2, checker_texture(8, 16, 4))]
    s.draws = [abi.make_draw(0, np.eye(4, dtype=F), texture_slot=1, material_index=0),
               abi.make_draw(1, scenes.compose_transform((0.0004, -0.0003, 0.0), (0, 0, 0)), texture_slot=2,
                             material_index=0, tint=(0.9, 1.0, 0.8, 1.0)),
               abi.make_draw(2, scenes.compose_transform((-0.0003, 0.0002, 0.0002), (0, 0, 0)), texture_slot=1,
                             material_index=0)]
    s.name = f"{s.name}_multi{'_shadow' if shadow else ''}"
    if shadow:
        scenes.with_shadow(s, 256)
    return s


def clip_flood(w=320, h=240, cells=185):
    """cells^2 thin triangles (1-4 px) that each cross the near plane with one vertex behind it (4
    polygon vertices, 2 clip records): 185^2 = 34225 triangles ask for more clip records than the initial 65536 and
    more polygon vertices than the initial 131072 (tri_ctx::ovf_rec_cap, ovf_vert_cap)."""
    s = dense_clip(w, h, cells=cells, size=(1.0, 4.0), pairs=False, guard=False, seed=23, two_behind=False)
    s.name = f"clip_flood_{cells}"
    return s


CLIP_RECORD_CAP, CLIP_VERTEX_CAP = 1 << 16, 1 << 17  # tri_ctx's initial ovf_rec_cap, ovf_vert_cap


def shadow_stack(w=320, h=240, size=256, n=400):
    """A ground quad under n small horizontal quads stacked along the sun's direction: in the light's view all 2 n
    caster triangles fall on the same few texels, so one 32 x 32 bin of the size^2 map holds more entries than the
    map queues' initial capacity (256), while on screen the stack is spread over many bins."""
    sun = np.array((-0.45, -1.0, -0.35))
    u = sun / np.linalg.norm(sun)
    quads = [np.array([(-6, 0, 6), (6, 0, 6), (6, 0, -6), (-6, 0, -6)], np.float64)]
    for k in range(n):
        c = np.array((0.5, 0.3, -0.5)) - u * (0.4 + 0.008 * k)
        r = 0.25 + 0.0003 * k
        quads.append(c + np.array([(-r, 0, r), (r, 0, r), (r, 0, -r), (-r, 0, -r)]))
    q = np.asarray(quads)
    v = np.zeros(4 * len(quads), abi.VERTEX_DTYPE)
    v["position"] = q.reshape(-1, 3).astype(F)
    v["normal"] = (0, 1, 0)
    v["color"] = np.random.default_rng(3).uniform(0.4, 1.0, size=(v.size, 3)).astype(F)
    v["texcoord"] = np.tile(np.array([(0, 0), (1, 0), (1, 1), (0, 1)], F), (len(quads), 1))
    base = 4 * np.arange(len(quads), dtype=np.uint32)[:, None]
    idx = (base + np.array([0, 1, 2, 0, 2, 3], np.uint32)).reshape(-1)
    cam = (0.0, 4.0, 8.0)
    view, proj = scenes.editor_camera(cam, (-25.0, 0.0, 0.0), 60.0, (w, h))
    lights = [{"type": "directional", "direction": tuple(sun), "intensity": 4.0}]
    s = scenes.Scene("shadow_stack", w, h, v, idx, np.array([(0, idx.size, 0, 0)], abi.MESH_RANGE_DTYPE),
                     [abi.make_draw(0, np.eye(4, dtype=F), material_index=0)], scenes.pack_ubo(view, proj, cam, lights),
                     materials=[((0.9, 0.85, 0.8, 1.0), (0.1, 0.6, 1.0, 0.0))], skybox=SOLID_0x808080)
    return scenes.with_shadow(s, size)


def grid_switch_pair(w=320, h=240, sparse_n=24, dense_n=60):
    """The C3 grid at two tessellations in ONE geometry (mesh 0: 2 (sparse_n - 1)^2 triangles, below 0.05 per pixel;
    mesh 1: 2 (dense_n - 1)^2, above), so that a draw list alone moves a context between the 16- and the 32-px bin
    grid. Returns (sparse scene, dense scene): the same buffers and mesh table, one draw each."""
    a, b = grid_c3(w, h, sparse_n), grid_c3(w, h, dense_n)
    verts = np.concatenate([a.vertices, b.vertices])
    idx = np.concatenate([a.indices, b.indices])
    meshes = np.array([(0, a.indices.size, 0, 0), (a.indices.size, b.indices.size, a.vertices.size, 0)],
                      abi.MESH_RANGE_DTYPE)
    out = []
    for k, s in enumerate((a, b)):
        s.vertices, s.indices, s.meshes = verts, idx, meshes
        s.draws = [abi.make_draw(k, np.eye(4, dtype=F), material_index=0)]
        s.skybox = None
        s.name = f"switch_{'dense' if k else 'sparse'}"
        out.append(s)
    return tuple(out)


def textured_two_draws(w=4100, h=4100, n=40):
    """textured_grid plus a second, tinted draw of the same mesh through another sRGB slot, pushed back and sideways
    so both show: several draws with a texture LUT and per-draw transforms."""
    s = textured_grid(w, h, n)
    s.textures = s.textures + [(5, checker_texture(8, 16, 4))]
    s.draws = s.draws + [abi.make_draw(0, scenes.compose_transform((1.1, 0.4, 0.35), (0.0, 8.0, 0.0), (1, 1, 1)),
                                       texture_slot=5, material_index=0, tint=(0.7, 1.0, 0.9, 1.0), tiling=0.5)]
    s.skybox = None
    s.name = f"textured_two_{w}x{h}"
    return s


def ai_multi(oracle, w=4100, h=4100, ai_extent=(96, 160), strength=0.35):
    """primitives_row (three draws) under the AI blend, the AI frame of another extent than the frame and addressed
    with the frame's own 1 / extent, so it is filtered up to the frame."""
    s = primitives_row(oracle, w, h)
    # a fourth draw: the quad primitive as a backdrop that fills the frame, so the blend reaches every bin
    s.draws = s.draws + [abi.make_draw(2, oracle.compose_transform((0.0, 3.0, -2.0), (0.0, 0.0, 0.0), (40.0, 40.0, 1.0)),
                                       texture_slot=0, material_index=1, tint=(0.6, 0.7, 0.9, 1.0))]
    ai =np.random.default_rng(0xA1).integers(0, 256, size=(ai_extent[0], ai_extent[1], 4), dtype=np.uint8)
    scenes.with_ai_blend(s, strength=strength, ai_frame=ai)
    s.ubo.ai_blend_config[1] = F(1.0) / F(w)
    s.ubo.ai_blend_config[2] = F(1.0) / F(h)
    s.name = f"ai_multi_{w}x{h}"
    return s


# ---- fragment-stage sweep: materials, light rigs, texture addressing ---------------------------------------------
# (base RGBA), (metallic, roughness, ambient strength, 0): metallic 0 and 1, the roughness clamp at either end, factors
# outside [0, 1] (clamped by Default.frag), HDR base colours, alpha above 1 and below
SWEEP_MATERIALS = [
    ((0.9, 0.75, 0.6, 1.0), (0.0, 0.0, 1.0, 0.0)),
    ((0.9, 0.75, 0.6, 1.3), (1.0, 0.045, 0.0, 0.0)),
    ((1.0, 1.0, 1.0, 0.4), (1.0, 1.0, 2.0, 0.0)),
    ((0.9, 0.75, 0.6, 1.0), (0.5, 0.3, 1.0, 0.0)),
    ((0.0, 0.0, 0.0, 1.0), (1.5, 1.7, -1.0, 0.0)),
    ((2.0, 1.5, 0.2, 1.0), (-0.5, 0.05, 0.5, 0.0)),
]
SWEEP_AMBIENT, SWEEP_AMBIENT_INTENSITY = (0.03, 0.05, 0.08), (1.0, 0.0, 3.0)  # the intensity rotates over the materials
SWEEP_RIGS = ("eight", "eleven", "headon", "back", "touch")
SWEEP_SUN_RIGS = ("headon", "back")
SWEEP_VARIANTS = ("one", "one_vcol", "multi", "shadow")
SWEEP_MULTI_TINT, SWEEP_MULTI_SLOT = (0.7, 1.0, 0.5, 1.2), 2
TOUCH_RANGE_LIGHT = ((1.0, 1.0, 3.2), 0.8)  # the touch rig's light whose range boundary crosses the visible sphere


def sweep_lights(rig):
    """The light list of a rig (see shading_sphere)."""
    if rig in ("eight", "eleven"):
        ranges = (15.0, 6.0, 0.0, 2.0, 30.0, 8.0, 1e-5, 12.0)
        intens = (6.0, 4.0, 5.0, 1e4, 0.0, 3.0, 5.0, 2.0)
        colours = ((1.0, 0.98, 0.92), (0.2, 0.9, 0.4), (1.0, 0.1, 0.1), (0.9, 0.9, 1.0), (1.0, 1.0, 1.0),
                   (0.0, 0.0, 0.0), (0.3, 0.3, 1.0), (1.0, 0.6, 0.1))
        lights = [{"type": "point", "position": (4.0 * np.cos(0.785 * k), 4.0 * np.sin(0.785 * k), 3.0 + 0.3 * k),
                   "range": ranges[k], "intensity": intens[k], "color": colours[k]} for k in range(8)]
        # three more than TRI_MAX_POINT_LIGHTS: bright and close, so a frame that shaded them would show it
        lights += [{"type": "point", "position": (0.5 * k - 0.5, -0.5, 4.0), "range": 20.0, "intensity": 40.0,
                    "color": (0.2, 1.0, 0.2)} for k in range(3)]
        return lights
    if rig == "headon":  # the GGX peak at the sphere's centre, HDR radiance into the tone curve
        return [{"type": "directional", "direction": (0.0, 0.0, -1.0), "intensity": 50.0}]
    if rig == "back":  # N.L <= 0 on almost every visible pixel, L nearly opposite V; a light 1e-3 off the surface
        return [{"type": "directional", "direction": (0.05, 0.03, 1.0), "intensity": 5.0},
                {"type": "point", "position": (0.0, 0.0, 3.001), "range": 5.0, "intensity": 8.0}]
    if rig == "touch":  # dist ~ 0, a range boundary across the visible surface, att reaching exactly 0
        return [{"type": "point", "position": (0.0, 0.0, 3.0), "range": 4.0, "intensity": 6.0},
                {"type": "point", "position": (0.0, 0.0, 0.0), "range": 3.5, "intensity": 20.0, "color": (0.4, 1.0, 0.6)},
                {"type": "point", "position": TOUCH_RANGE_LIGHT[0], "range": TOUCH_RANGE_LIGHT[1], "intensity": 30.0,
                 "color": (1.0, 0.5, 0.2)}]
    raise KeyError(rig)


def shading_sphere(rig, material, variant, w=320, h=240, rings=40, segments=60):
    """The C2 sphere (radius 3 at the origin, camera at (0, 0, 9)) under one light rig, one of SWEEP_MATERIALS and one
    instantiation of the fragment stage.

    Rigs: eight = 8 point lights on a spiral around the view axis (ranges 0 and 1e-5, intensities 0 and 1e4, a black
    one), three more behind them that the packer drops, no sun; eleven = the same UBO with light_counts[1] = 11 (the
    shader clamps to 8); headon / back / touch: sweep_lights. Variants: one = a single draw over the default 1x1 slot;
    one_vcol = with seeded vertex colours in [0, 1.5]; multi = the index range as two draws (a third and two thirds), the
    second tinted and through a 3x5 texture; shadow = one_vcol under the pre-pass for the rig's sun. Every variant has
    the same mesh table (mesh 0 the whole sphere, 1 and 2 its parts), so one context can move between them by its draw
    list alone."""
    s = scenes.scene_c2_sphere(w, h, rings, segments, skybox="solid")
    s.skybox = None
    cam = (0.0, 0.0, 9.0)
    view, proj = scenes.editor_camera(cam, (0, 0, 0), 60.0, (w, h), 0.1, 1000.0)
    s.ubo = scenes.pack_ubo(view, proj, cam, sweep_lights(rig), ambient=SWEEP_AMBIENT,
                            ambient_intensity=SWEEP_AMBIENT_INTENSITY[material % 3])
    if rig == "eleven":
        s.ubo.light_counts[1] = 11
    s.materials = [SWEEP_MATERIALS[material]]
    cut = (s.indices.size // 9) * 3
    s.meshes = np.array([(0, s.indices.size, 0, 0), (0, cut, 0, 0), (cut, s.indices.size - cut, 0, 0)],
                        abi.MESH_RANGE_DTYPE)
    if variant in ("one_vcol", "shadow"):
        v = s.vertices.copy()
        v["color"] = np.random.default_rng(17).uniform(0.0, 1.5, size=(v.shape[0], 3)).astype(F)
        s.vertices = v
    if variant == "multi":
        s.textures = [(SWEEP_MULTI_SLOT, checker_texture(3, 5, 13))]
        s.draws = [abi.make_draw(1, np.eye(4, dtype=F), material_index=0),
                   abi.make_draw(2, np.eye(4, dtype=F), texture_slot=SWEEP_MULTI_SLOT, material_index=0,
                                 tint=SWEEP_MULTI_TINT)]
    elif variant not in ("one", "one_vcol", "shadow"):
        raise KeyError(variant)
    s.name = f"sweep_{rig}_m{material}_{variant}"
    if variant == "shadow":
        if rig not in SWEEP_SUN_RIGS:
            raise ValueError(f"rig {rig} has no sun to cast a shadow")
        scenes.with_shadow(s, 256)
    return s


# (texture w x h, scale, offset, tiling): non-power-of-two extents, w x 1 and 1 x h, width 2, negative scales and
# offsets. MODERATE cases stay where float32 uv precision is below an LSB (compared with float64 too); LARGE ones carry
# uvs in the thousands (|u w|, |v h| < 2^20), where only the oracle's float32 order is the reference.
SAMPLER_MODERATE = {
    "3x5": ((3, 5), (1.5, 0.75), (0.1, -0.2), 1.25),
    "5x3_neg": ((5, 3), (-1.5, 0.75), (-3.3, 100.25), 7.0),
    "1x7": ((1, 7), (1.0, 1.0), (0.0, 0.0), 1.0),
    "7x1": ((7, 1), (2.0, -3.0), (0.5, 0.5), 1.0),
    "2x2": ((2, 2), (1.0, 1.0), (-0.25, -0.25), 1.0),
    "100x3": ((100, 3), (0.01, 1.0), (-0.005, 0.0), 1.0),
    "3x5_identity": ((3, 5), (1.0, 1.0), (0.0, 0.0), 1.0),
}
SAMPLER_LARGE = {
    "3x3_tiling1000": ((3, 3), (1.0, 1.0), (0.0, 0.0), 1000.0),
    "6x10_offset4096": ((6, 10), (1.0, 1.0), (-4096.0, 4096.0), 1.0),
}


def sampler_grid(tex_wh, scale, offset, tiling, w=320, h=180, n=30, seed=7):
    """textured_grid with a seeded tex_wh texture in slot 3 under the given uv transform (uv * scale * tiling + offset)."""
    s = textured_grid(w, h, n)
    s.skybox = None
    s.textures = [(3, checker_texture(tex_wh[0], tex_wh[1], seed))]
    s.draws = [abi.make_draw(0, np.eye(4, dtype=F), texture_slot=3, material_index=0, tint=(1.0, 0.9, 0.8, 0.75),
                             texture_scale=scale, texture_offset=offset, tiling=tiling)]
    s.name = f"sampler_{tex_wh[0]}x{tex_wh[1]}_s{scale[0]:g},{scale[1]:g}_o{offset[0]:g},{offset[1]:g}_t{tiling:g}"
    return s


def sampler_case(name, **kw):
    return sampler_grid(*{**SAMPLER_MODERATE, **SAMPLER_LARGE}[name], **kw)


# ---- skinned-vertex sweep: normals, palettes, several draws ------------------------------------------------------------
# each rig with a material that shows it (under the metallic, ambient-free material 1 the touch rig leaves most of
# the sphere black, and a wrong normal moved under 1 % of its pixels)
SKIN_RIG_MATERIALS = (("headon", 3), ("eight", 0), ("touch", 5))
SKIN_FORMS = ("one", "nonunit0.6", "nonunit1.5", "skips", "short_palette", "multi", "shadow")
SKIN_MODEL = ((0.1, -0.2, 0.0), (10.0, -15.0, 5.0), (1.0, 0.9, 1.1))  # non-conformal: the normal matrix is not a rotation
SKIN_BONES = (((0.4, 0.2, 0.3), (20.0, 35.0, 25.0), (1.2, 0.8, 1.1)),
              ((-0.3, 0.0, 0.2), (-40.0, 10.0, 0.0), (0.9, 1.1, 1.3)))  # palette rows 2 and 3; row 1 is the identity
SKIN_BONES_2 = (((0.2, -0.3, 0.4), (-25.0, 20.0, 30.0), (1.1, 1.2, 0.8)),
                ((-0.4, 0.3, 0.1), (30.0, -20.0, 15.0), (0.8, 1.0, 1.2)))  # rows 4 and 5: multi's second skinned draw
SKIN_SPARE_ROW = ((0.5, 0.5, 0.6), (0.0, 60.0, 0.0), (1.4, 1.4, 1.4))  # skips: the row behind the draw's three bones
SKIN_SENTINEL = 99.0  # row 0, below every draw's bone_offset: no draw may read it
SKIN_PATCH = (range(17, 24), range(11, 20))  # skips: (rings, segments) of the patch, facing the camera
SKIN_DEAD = ((10, 15), (30, 15), (20, 5), (20, 25), (28, 21))  # skips: (ring, segment) of the vertices with no influence
SKIN_MULTI_MODELS = (((-3.3, -0.2, 0.0), SKIN_MODEL[1], (0.8, 0.72, 0.88)),
                     ((3.2, 2.3, 0.0), (-20.0, 30.0, 10.0), (0.5, 0.45, 0.55)),
                     ((3.2, -2.3, 0.0), (15.0, -25.0, 0.0), (0.5, 0.55, 0.45)))
SKIN_SMALL_SPHERE = (16, 24)  # multi's second mesh: rings, segments (radius 3 like the first)
SKIN_GROUND_Z = -4.2  # shadow: the receiver's plane, behind the skinned sphere as the head-on sun sees it


def smooth_skin_weights(y):
    """Three bones blended along y in [-3, 3]: ((1 - t)(1 - w2), t (1 - w2), w2, 0) on indices (0, 1, 2, 0), with
    t = clip((y + 3) / 6, 0, 1) and w2 = 0.25 * 4 t (1 - t). Smooth in y, so the skinned surface does not fold."""
    t = np.clip((np.asarray(y, np.float64) + 3.0) / 6.0, 0.0, 1.0)
    w2 = 0.25 * 4.0 * t * (1.0 - t)
    w = np.stack([(1.0 - t) * (1.0 - w2), t * (1.0 - w2), w2, np.zeros_like(t)], -1)
    idx = np.tile(np.array([0, 1, 2, 0], np.int32), (len(t), 1))
    return idx, w, t


def skin_palette(*groups):
    """The sentinel row, the identity, then compose_transform of every (position, rotation, scale) of the groups."""
    rows = [np.full(16, SKIN_SENTINEL, F), np.eye(4, dtype=F).reshape(16)]
    rows += [scenes.compose_transform(*trs).reshape(16) for g in groups for trs in g]
    return np.stack(rows).astype(F)


def skinned_dead_vertices(segments=60):
    return [r * (segments + 1) + s for r, s in SKIN_DEAD]


def skinned_world_f64(scene):
    """World positions (x, y, z of the undivided model * skin * p) of every vertex a draw references, float64."""
    import test_oracle_clip_f64 as f64

    out = []
    for d in scene.draws:
        m = scene.meshes[d.mesh_index]
        idx = scene.indices[int(m["first_index"]):int(m["first_index"]) + int(m["index_count"])]
        used = np.unique(idx.astype(np.int64) + int(m["base_vertex"]))
        sp, _ = f64.f64_skin(scene, d)
        out.append((sp[used] @ np.array(d.pc.model, np.float64).reshape(4, 4))[:, :3])
    return np.concatenate(out)


def skinned_sphere(rig, material, form, w=320, h=240):
    """shading_sphere(rig, material, "one_vcol") (2501 vertex slots: ten 256-slot vertex blocks) skinned by three bones
    at palette offset 1 (smooth_skin_weights, skin_palette(SKIN_BONES)) under the non-conformal model SKIN_MODEL.

    Forms: one = that single draw; nonunit0.6 / nonunit1.5 = its weights multiplied by 1 + (k - 1) t, so they sum to
    1 .. k and a w != 1 reaches the clip stage; skips = a patch of vertices carries one skip rule each on its fourth
    influence (a negative weight, a zero weight, index -1, index == bone_count; the palette has a spare row behind the
    draw's bones, so only the draw's own bone_count keeps that last read out) and the five SKIN_DEAD vertices have every
    influence skipped, each by another rule; short_palette = one with the palette uploaded one row short (bone 2 lies
    past it for every vertex); multi = three draws (the sphere skinned from rows 1..3; a smaller sphere unskinned under
    its own affine model; that sphere again, skinned with bone_offset 4 and bone_count 2, so its index 2 is out of
    range), apart from one another on screen; shadow = one plus an unskinned ground quad behind the sphere under the
    pre-pass, the light box fitted to the skinned float64 positions."""
    s = shading_sphere(rig, material, "one_vcol", w, h)
    v = s.vertices.copy()
    idx, wgt, t = smooth_skin_weights(v["position"][:, 1])
    bones = skin_palette(SKIN_BONES)
    model = scenes.compose_transform(*SKIN_MODEL)
    s.draws = [abi.make_draw(0, model, material_index=0, bone_offset=1, bone_count=3)]
    if form.startswith("nonunit"):
        wgt = wgt * (1.0 + (float(form[len("nonunit"):]) - 1.0) * t)[:, None]
    elif form == "skips":
        bones = skin_palette(SKIN_BONES, (SKIN_SPARE_ROW,))
        row = 61
        rules = ((0, -0.4), (1, 0.0), (-1, 0.5), (3, 0.5))  # (index, weight) of the fourth influence, by vertex
        for n, (r, sg) in enumerate((r, sg) for r in SKIN_PATCH[0] for sg in SKIN_PATCH[1]):
            idx[r * row + sg, 3], wgt[r * row + sg, 3] = rules[n % 4]
        dead = ((0, 1, -1, 3), (-0.5, 0.0, 0.5, 0.5)), ((3, -1, 1, 0), (0.7, 0.3, 0.0, -1.0)), \
            ((-1, -2, 4, 3), (0.25, 0.25, 0.25, 0.25)), ((0, 1, 2, 0), (0.0, 0.0, 0.0, 0.0)), \
            ((0, 1, 2, 3), (-0.2, -0.3, -0.5, 1.0))
        for vi, (di, dw) in zip(skinned_dead_vertices(), dead):
            idx[vi], wgt[vi] = di, dw
    elif form == "short_palette":
        bones = bones[:3]
    elif form not in ("one", "multi", "shadow"):
        raise KeyError(form)
    v["bone_indices"], v["bone_weights"] = idx, wgt.astype(F)
    s.vertices = v
    if form == "multi":
        sv, si = scenes.uv_sphere_mesh(*SKIN_SMALL_SPHERE, 3.0)
        sv["color"] = np.random.default_rng(19).uniform(0.0, 1.5, size=(sv.shape[0], 3)).astype(F)
        sidx, swgt, _ = smooth_skin_weights(sv["position"][:, 1])
        sv["bone_indices"], sv["bone_weights"] = sidx, swgt.astype(F)
        small = len(s.meshes)
        s.meshes = np.concatenate([s.meshes, np.array([(s.indices.size, si.size, v.shape[0], 0)], abi.MESH_RANGE_DTYPE)])
        s.vertices, s.indices = np.concatenate([v, sv]), np.concatenate([s.indices, si])
        bones = skin_palette(SKIN_BONES, SKIN_BONES_2)
        m = [scenes.compose_transform(*trs) for trs in SKIN_MULTI_MODELS]
        s.draws = [abi.make_draw(0, m[0], material_index=0, bone_offset=1, bone_count=3),
                   abi.make_draw(small, m[1], material_index=0, tint=(0.8, 1.0, 0.7, 1.0)),
                   abi.make_draw(small, m[2], material_index=0, tint=(1.0, 0.7, 0.9, 1.0), bone_offset=4, bone_count=2)]
        ends = np.cumsum([v.shape[0], sv.shape[0], sv.shape[0]])
        # a 64-lane wave of k_vertex then holds slots of a skinned and of an unskinned draw
        assert any(e % 64 for e in ends[:2]), ends
    elif form == "shadow":
        g = np.zeros(4, abi.VERTEX_DTYPE)
        g["position"] = [(-9, -7, SKIN_GROUND_Z), (9, -7, SKIN_GROUND_Z), (9, 7, SKIN_GROUND_Z), (-9, 7, SKIN_GROUND_Z)]
        g["normal"] = (0, 0, 1)
        g["color"] = (0.9, 0.9, 0.9)
        g["texcoord"] = [(0, 0), (1, 0), (1, 1), (0, 1)]
        ground = len(s.meshes)
        s.meshes = np.concatenate([s.meshes, np.array([(s.indices.size, 6, v.shape[0], 0)], abi.MESH_RANGE_DTYPE)])
        s.vertices = np.concatenate([v, g])
        s.indices = np.concatenate([s.indices, np.array([0, 1, 2, 0, 2, 3], np.uint32)])
        s.draws = s.draws + [abi.make_draw(ground, np.eye(4, dtype=F), material_index=0)]
    s.bones = bones
    s.name = f"skinned_{rig}_m{material}_{form}"
    if form == "shadow":  # the box of the skinned positions, not of the bind pose: no caster leaves the map
        from trident_raster import raster

        world = skinned_world_f64(s)
        lvp = raster.shadow_fit_ortho(list(s.ubo.directional_light_direction)[:3], world.min(0).astype(F),
                                      world.max(0).astype(F))
        s.shadow = abi.make_shadow(lvp, 256, 0.001, 2.0)
    return s
