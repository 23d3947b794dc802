"""GPU parity where a THRESHOLD selects the code rather than a scene feature: the bin grid (16, 32 or 64 px, chosen by
frame size and triangle density), the 64 x 64-bin raster instantiations (frames above 16384 bins of 32 px), crowded
bins and overfull large-triangle queues, dense homogeneous clipping at every bin size, the recovery from each
internal-buffer overflow, and a context that changes its bin grid between frames.

The bar is DESIGN §4's, as in test_parity_gpu.py: depth bits equal as uint32, every B8G8R8A8 channel within COLOR_TOL,
triangles_setup equal. Every test also asserts frame_stats()["bin_size"], so a scene that lands on another grid fails
rather than passing on the wrong path. tests/test_raster_path_scenes.py shows on the CPU that the scenes have the
properties relied on here (ragged bins covered, entries per bin, clipped counts and polygon sizes, capacities exceeded).
"""
import re

import numpy as np
import pytest

import scene_cases as sc
from test_parity_gpu import COLOR_TOL

pytestmark = pytest.mark.gpu

BG = 0x3F800000
BIG = 4100  # 129 x 129 bins of 32 px > 16384: a 65 x 65 grid of 64-px bins whose last column and row are 4 px wide
OVF_CLIP_RECORDS, OVF_CLIP_VERTS, OVF_BIN_LIST, OVF_SHADOW_BIN_LIST = 0x1, 0x2, 0x4, 0x8  # raster_common.h TRI_OVF_*


@pytest.fixture(params=["fast", "exact"])
def flags(request):
    from trident_raster import abi

    return abi.TRI_FLAG_EXACT_SHADING if request.param == "exact" else 0


_REF = {}


def reference(oracle, scene, band=None):
    """The oracle's (colour, depth, stats, shadow map) of a scene, computed once and shared by the tests that follow
    each other with it (the fast and the exact build); never modified."""
    key = (scene.name, scene.width, scene.height, band)
    if key not in _REF:
        if len(_REF) >= 2:
            _REF.pop(next(iter(_REF)))
        smap = None
        if scene.shadow is not None:
            smap = np.zeros((scene.shadow.size, scene.shadow.size), np.uint32)
        col, dep, stats = oracle.render(scene, band=band, shadow_map_out=smap)
        for a in (col, dep):
            a.setflags(write=False)
        _REF[key] = (col, dep, stats, smap)
    return _REF[key]


def check_frame(tag, r, ref, bin_size, min_covered=1, path=0, not_path=0):
    """The context's last frame against the oracle's (the bar of test_parity_gpu.assert_parity), its bin grid and its
    path bits. Returns the frame."""
    from trident_raster import abi

    col, dep = r.readback()
    st = r.frame_stats()
    print(f"PATHS {tag}: bin_size {st['bin_size']} grid {st['bins_x']}x{st['bins_y']} path {st['path']:#x} "
          f"setup {st['triangles_setup']} clipped {st['triangles_clipped']}")
    assert st["bin_size"] == bin_size, (tag, st)
    assert st["bins_x"] == -(-r.width // bin_size) and st["bins_y"] == -(-r.rows // bin_size), (tag, st)
    assert st["path"] & path == path and st["path"] & not_path == 0, (tag, hex(st["path"]))
    oc, od, os_, om = ref
    assert dep.shape == od.shape and col.shape == oc.shape
    bad = int((dep != od).sum())
    assert bad == 0, f"{tag}: {bad} depth mismatches"
    worst = int(np.abs(col.astype(np.int16) - oc.astype(np.int16)).max(initial=0))
    assert worst <= COLOR_TOL, f"{tag}: colour diff {worst} (> {COLOR_TOL})"
    assert int((od != BG).sum()) >= min_covered, tag
    assert st["triangles_setup"] == os_["triangles_setup"], (tag, st, os_)
    if om is not None:
        assert np.array_equal(r.read_shadow_map(), om), f"{tag}: shadow map mismatch"
    assert abi.TRI_OK == 0
    return col, dep


def expect_overflow(r, want_bits):
    """render + synchronize must report TRI_E_OVERFLOW with one of want_bits among its flags; returns the flags."""
    from trident_raster import abi, raster

    r.render()
    with pytest.raises(raster.TriError) as ei:
        r.synchronize()
    assert ei.value.code == abi.TRI_E_OVERFLOW, ei.value
    m = re.search(r"flags (0x[0-9a-fA-F]+)", str(ei.value))
    assert m, str(ei.value)
    got = int(m.group(1), 16)
    assert got & want_bits, (hex(got), hex(want_bits))
    return got


def render_checked(scene, oracle, flags, bin_size, overflow=0, band=None, **kw):
    """One context: load, (expect the overflow,) render, compare; then a second frame, bit-identical to the first."""
    from trident_raster import raster, scenes

    assert sc.expected_bin_size(scene.width, (band[1] - band[0]) if band else scene.height, scene.height,
                                scene.triangles) == bin_size
    ref = reference(oracle, scene, band)
    with raster.TriRaster(scene.width, scene.height, band=band, flags=flags) as r:
        scenes.load_scene(r, scene)
        if overflow:
            expect_overflow(r, overflow)
        r.render_frame()
        col, dep = check_frame(scene.name, r, ref, bin_size, **kw)
        if overflow:
            r.render_frame()
            col2, dep2 = r.readback()
            assert np.array_equal(col, col2) and np.array_equal(dep, dep2), f"{scene.name}: second frame differs"


# ---- A. grid selection, pinned ---------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,band,want", [(2048, 2016, None, 16), (2048, 2048, None, 32), (4096, 4096, None, 32),
                                           (4097, 4096, None, 64), (BIG, BIG, (0, 2050), 32)])
def test_grid_selection_by_frame_size(w, h, band, want):
    """The edges of choose_bin_grid's size rule on frames without geometry: 4032 bins of 32 px are a small grid (16 px
    while sparse), 4096 are not; 16384 keep 32 px, 129 x 128 take 64 px; a band counts its own rows."""
    from trident_raster import raster, scenes

    s = sc.empty_scene(w, h)
    rows = (band[1] - band[0]) if band else h
    assert sc.expected_bin_size(w, rows, h, 0) == want
    with raster.TriRaster(w, h, band=band) as r:
        scenes.load_scene(r, s)
        r.render_frame()
        st = r.frame_stats()
    assert (st["bin_size"], st["bins_x"], st["bins_y"]) == (want, -(-w // want), -(-rows // want)), st


@pytest.mark.parametrize("ntris,want", [(3840, 32), (3839, 16)])
def test_grid_selection_by_density(oracle, ntris, want):
    """320 x 240 = 76800 pixels: 3840 triangles are exactly 0.05 per pixel (32 px), 3839 are sparse (16 px)."""
    s = sc.counted_triangles(320, 240, ntris)
    render_checked(s, oracle, 0, want, min_covered=500)


# ---- B. every 64 x 64-bin instantiation against the oracle -----------------------------------------------------
def test_big_single_solid_draw(oracle, flags):
    """k_raster_plain<.., 6, ONE>: near_clip_grid (4 clipped triangles) over 14.7 M pixels, ragged bins covered."""
    from trident_raster import abi

    render_checked(sc.near_clip_grid(BIG, BIG, 60), oracle, flags, 64, min_covered=10 ** 7, path=abi.TRI_PATH_ONE_DRAW)


def test_big_textured_draws(oracle, flags):
    """k_raster_plain<.., 6, general>: two textured draws (sRGB LUT in LDS, per-draw transforms)."""
    from trident_raster import abi

    render_checked(sc.textured_two_draws(BIG, BIG), oracle, flags, 64, min_covered=10 ** 7,
                   not_path=abi.TRI_PATH_ONE_DRAW | abi.TRI_PATH_SHADOW)


def test_big_ai_blend(oracle, flags):
    """k_raster_ai<.., 6>: four draws under the AI blend, the AI frame of another extent filtered up to the frame."""
    from trident_raster import abi

    render_checked(sc.ai_multi(oracle, BIG, BIG), oracle, flags, 64, min_covered=10 ** 7, not_path=abi.TRI_PATH_SHADOW)


def test_big_shadow_prepass(oracle, flags):
    """k_raster<.., 6, shadow>: the shadow scene (the map's own bins stay 32 px); the map is compared too."""
    from trident_raster import abi

    render_checked(sc.shadow_scene(oracle, BIG, BIG, size=256), oracle, flags, 64, min_covered=10 ** 6,
                   path=abi.TRI_PATH_SHADOW)


def test_big_sampled_skybox(oracle, flags):
    """The sky queue of a 64 x 64 tile (indices to 4095) and the per-pixel sky direction, behind the cube."""
    s = sc.c1_cube_skybox(1, BIG, BIG)
    s.skybox = sc.cubemap_faces()
    s.name = "c1_cube_skybox_big"
    render_checked(s, oracle, flags, 64, min_covered=100000)


@pytest.mark.parametrize("seed", [11, 13])
def test_big_pixel_aligned_span_walk(oracle, flags, seed):
    """raster_span<6>: edges through pixel centres on 64-px bins (seed 13 also reaches the 4 x 4 corner bin)."""
    s = sc.pixel_aligned_triangles(BIG, BIG, 8000, seed)
    s.name = f"pixel_aligned_big_{seed}"
    render_checked(s, oracle, flags, 64, min_covered=10 ** 6)


def test_big_crowded_bins(oracle, flags):
    """Bins of 640 and 2840 entries (the coverage loop past its prefetched first round), 2202 large triangles in one
    bin (the large-triangle queue full, the rest walked per lane), in an interior, a ragged-column, a ragged-row and
    the corner bin; the frame first overflows the bin list and recovers at 64 px."""
    render_checked(sc.crowded_bins(BIG, BIG), oracle, flags, 64, overflow=OVF_BIN_LIST, min_covered=5000)


def test_big_dense_clip(oracle, flags):
    """Clipped pixels shaded inline at 64 px (no deferred queue there): 1300 clipped triangles of 3 to 8 polygon
    vertices over sheets that give every pixel a clipped fragment, so waves mix clipped and unclipped lanes."""
    render_checked(sc.dense_clip(BIG, BIG), oracle, flags, 64, min_covered=BIG * BIG)


# ---- C. dense clipping at the other two bin sizes ---------------------------------------------------------------
@pytest.mark.parametrize("form", ["single", "multi", "single_shadow", "multi_shadow"])
@pytest.mark.parametrize("w,h,bin_size", [(320, 240, 16), (240, 180, 32)])
def test_dense_clip(oracle, flags, w, h, bin_size, form):
    """dense_clip as one solid draw (object-space records through the clipper), as three textured draws (prim_vs, the
    draw in the record) and with the shadow pre-pass (light-space positions interpolated by the clipper; in its map,
    fitted to the sheets, every small triangle meets in one bin, so render_frame also grows the map queues)."""
    from trident_raster import abi, scenes

    shadow = form.endswith("shadow")
    if form.startswith("single"):
        s = sc.dense_clip(w, h)
        if shadow:
            scenes.with_shadow(s, 256)
            s.name += "_shadow"
    else:
        s = sc.dense_clip_multi(w, h, shadow=shadow)
    render_checked(s, oracle, flags, bin_size, min_covered=w * h, path=abi.TRI_PATH_SHADOW if shadow else 0,
                   not_path=0 if shadow else abi.TRI_PATH_SHADOW)


def test_dense_clip_cluster_cull_is_exact(oracle):
    """TRI_FLAG_CLUSTER_CULL over dense_clip: bit-identical to the unculled frame, and to the bar."""
    from trident_raster import abi, raster, scenes

    s = sc.dense_clip(320, 240)
    frames = []
    for fl in (0, abi.TRI_FLAG_CLUSTER_CULL):
        with raster.TriRaster(s.width, s.height, flags=fl) as r:
            scenes.load_scene(r, s)
            r.render_frame()
            frames.append(check_frame(f"{s.name}_cull{fl}", r, reference(oracle, s), 16, min_covered=320 * 240))
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1])


# ---- D. overflow recovery, compared -----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,draws,bin_size", [(320, 240, 1, 16), (200, 120, 1, 32), (200, 120, 3, 32)])
def test_bin_overflow_with_overfull_large_queue(oracle, flags, w, h, draws, bin_size):
    """2200 large triangles in one bin: past the bin list's initial capacity and past the large-triangle queue of
    the instantiation (512 entries at 16 px, 192 for a single solid draw at 32 px, 1024 otherwise), whose overflow
    is rasterized per lane."""
    from trident_raster import abi

    s = sc.stacked_quads(w, h, draws=draws, textured=draws > 1)
    render_checked(s, oracle, flags, bin_size, overflow=OVF_BIN_LIST, min_covered=1600,
                   path=abi.TRI_PATH_ONE_DRAW if draws == 1 else 0, not_path=0 if draws == 1 else abi.TRI_PATH_ONE_DRAW)


def test_clip_record_and_vertex_overflow(oracle, flags):
    """34225 clipped triangles: more clip records than 65536 and more polygon vertices than 131072."""
    render_checked(sc.clip_flood(), oracle, flags, 32, overflow=OVF_CLIP_RECORDS | OVF_CLIP_VERTS, min_covered=30000)


def test_shadow_bin_list_overflow(oracle, flags):
    """802 caster triangles over one 32 x 32 bin of a 256^2 map: the map queues overflow and recover; the map and the
    frame are compared."""
    from trident_raster import abi

    render_checked(sc.shadow_stack(), oracle, flags, 16, overflow=OVF_SHADOW_BIN_LIST, min_covered=20000,
                   path=abi.TRI_PATH_SHADOW)


# ---- E. grid switches inside one context ------------------------------------------------------------------------
def _switch_sequence():
    sparse, dense = sc.grid_switch_pair()
    return [(sparse, 16), (dense, 32), (sparse, 16), (dense, 32)]


@pytest.mark.parametrize("how", ["upload", "draws", "enqueued"])
def test_grid_switches_in_one_context(oracle, how):
    """sparse (16 px) -> dense (32) -> sparse -> dense in one 320 x 240 context, every frame compared: by uploading
    each geometry anew, by set_draws alone over a shared TriGeometry, and with the frame before each switch only
    enqueued (render without synchronize) when the next one is rendered on the other grid."""
    from trident_raster import raster, scenes

    seq = _switch_sequence()
    geom = None
    if how != "upload":
        geom = raster.TriGeometry(0)
        geom.upload(seq[0][0].vertices, seq[0][0].indices, seq[0][0].meshes)
    with raster.TriRaster(320, 240, device=0) as r:
        scenes.load_scene(r, seq[0][0], geometry=geom)
        for k, (s, bin_size) in enumerate(seq):
            if how == "upload":
                first = int(s.meshes[s.draws[0].mesh_index]["first_index"])
                count = int(s.meshes[s.draws[0].mesh_index]["index_count"])
                own = sc.grid_c3(320, 240, 24 if bin_size == 16 else 60)
                assert np.array_equal(own.indices, s.indices[first:first + count])
                r.upload_geometry(own.vertices, own.indices, own.meshes)
                r.set_draws(own.draws)
            else:
                r.set_draws(s.draws)
            r.render_frame()
            check_frame(f"{how}[{k}] {s.name}", r, reference(oracle, s), bin_size, min_covered=320 * 240 // 2)
            if how == "enqueued":
                r.render()  # the same frame again, left in flight across the switch
        r.synchronize()
    if geom is not None:
        geom.close()


def test_grid_switch_grows_bin_counters_over_reused_memory(oracle):
    """dense (32 px, 80 bins) -> sparse (16 px, 300 bins): the switch allocates larger bin counters, which must be
    zeroed on the context's stream before the frame's set-up counts into them. Device memory is poisoned with 0xFF
    before the switch, as test_first_frame_over_reused_device_memory does for a context's first frame (a guard:
    whether the new buffer lands on poisoned memory is the allocator's choice)."""
    from test_multidevice_gpu import _poison_device_memory
    from trident_raster import raster, scenes

    sparse, dense = sc.grid_switch_pair()
    with raster.TriRaster(320, 240) as r:
        scenes.load_scene(r, dense)
        for k, (s, bin_size) in enumerate([(dense, 32), (sparse, 16), (dense, 32)]):
            assert _poison_device_memory(chunks=16) > 0
            r.set_draws(s.draws)
            r.render_frame()
            check_frame(f"poisoned[{k}] {s.name}", r, reference(oracle, s), bin_size, min_covered=320 * 240 // 2)


def test_grid_switch_after_bin_overflow(oracle):
    """A bin-list overflow grows the capacity on the 16-px grid; the switch to 32 px re-derives it, and the way back
    overflows and recovers again. Every frame is compared."""
    from trident_raster import raster, scenes

    crowded = sc.stacked_quads(320, 240)
    _, dense = sc.grid_switch_pair()
    with raster.TriRaster(320, 240) as r:
        scenes.load_scene(r, crowded)
        expect_overflow(r, OVF_BIN_LIST)
        r.render_frame()
        check_frame("overflow, 16 px", r, reference(oracle, crowded), 16)
        scenes.load_scene(r, dense)
        r.render_frame()
        check_frame("then dense, 32 px", r, reference(oracle, dense), 32)
        scenes.load_scene(r, crowded)
        r.render_frame()  # (grows again: the 16-px grid's capacity starts over)
        check_frame("and back, 16 px", r, reference(oracle, crowded), 16)


def test_grid_switches_in_a_two_band_group(oracle):
    """The same sequence through TriGroup([0, 0]): both band contexts switch grids (the density is the whole
    frame's), and the assembled frames equal the oracle's and a single context's."""
    import ctypes as C

    from trident_raster import abi, raster, scenes

    seq = _switch_sequence()
    singles = []
    with raster.TriRaster(320, 240) as r:
        scenes.load_scene(r, seq[0][0])
        for s, _ in seq:
            r.set_draws(s.draws)
            r.render_frame()
            singles.append(r.readback())
    with raster.TriGroup(320, 240, [0, 0]) as g:
        scenes.load_scene(g, seq[0][0])
        for k, (s, bin_size) in enumerate(seq):
            g.set_draws(s.draws)
            g.render_frame()
            col, dep = g.readback()
            for band in range(2):
                st = abi.TriFrameStats()
                assert raster.load_library().tri_get_frame_stats(g.context(band), C.byref(st)) == abi.TRI_OK
                assert (st.bin_size, st.bins_x, st.bins_y) == (bin_size, 320 // bin_size, -(-120 // bin_size)), (k, band)
            oc, od, _, _ = reference(oracle, s)
            assert np.array_equal(dep, od), k
            assert int(np.abs(col.astype(np.int16) - oc.astype(np.int16)).max()) <= COLOR_TOL, k
            assert np.array_equal(col, singles[k][0]) and np.array_equal(dep, singles[k][1]), k
