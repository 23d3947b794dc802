"""CPU companion of tests/test_raster_paths_gpu.py: the scenes those tests render really have the properties the tests
rely on, shown from the oracle and from the raster rules of DESIGN §4 alone (no GPU): which bin grid a frame gets, that
the 4100 x 4100 frames reach their ragged last column, last row and 4 x 4 corner bin, how many entries the crowded
bins hold, how many triangles the clipping scenes clip and how large their polygons get, and that the overflow scenes
exceed the capacities they are meant to exceed."""
import numpy as np
import pytest

import scene_cases as sc

BG = 0x3F800000
BIG = 4100  # 129 x 129 bins of 32 px = 16641 > 16384: the smallest square frame on 64-px bins (65 x 65, the last 4 px wide)


def test_expected_bin_size_edges():
    """choose_bin_grid's thresholds, at the shapes the GPU test renders."""
    assert sc.expected_bin_size(2048, 2016, 2016, 0) == 16  # 64 * 63 = 4032 bins of 32
    assert sc.expected_bin_size(2048, 2048, 2048, 0) == 32  # 4096 is not < 4096
    assert sc.expected_bin_size(4096, 4096, 4096, 0) == 32  # 16384 is not > 16384
    assert sc.expected_bin_size(4097, 4096, 4096, 0) == 64  # 129 * 128
    assert sc.expected_bin_size(320, 240, 240, 3840) == 32  # 3840 / 76800 == 0.05 exactly
    assert sc.expected_bin_size(320, 240, 240, 3839) == 16
    assert sc.expected_bin_size(BIG, 2050, BIG, 0) == 32  # a band's own rows count: 129 * 65 = 8385
    assert sc.expected_bin_size(BIG, BIG, BIG, 10 ** 7) == 64
    assert 3840 / 76800 == 0.05 and not (3840 / 76800 < 0.05)
    for n in (3839, 3840):
        assert sc.counted_triangles(320, 240, n).triangles == n


def ragged(depth):
    cov = depth != BG
    return int(cov[:, -4:].sum()), int(cov[-4:, :].sum()), int(cov[-4:, -4:].sum())


_BIG_SCENES = {
    "near_clip": lambda o: sc.near_clip_grid(BIG, BIG, 60),
    "textured_two": lambda o: sc.textured_two_draws(BIG, BIG),
    "ai_multi": lambda o: sc.ai_multi(o, BIG, BIG),
    "shadow": lambda o: sc.shadow_scene(o, BIG, BIG, size=256),
    "pixel_aligned": lambda o: sc.pixel_aligned_triangles(BIG, BIG, 8000, 13),  # (seed 11 misses the corner bin)
    "crowded": lambda o: sc.crowded_bins(BIG, BIG),
    "dense_clip": lambda o: sc.dense_clip(BIG, BIG),
}


@pytest.mark.parametrize("case", sorted(_BIG_SCENES))
def test_big_frames_reach_the_ragged_bins(oracle, case):
    """Every 4100 x 4100 scene of the 64-px tests covers pixels in the last 4 columns, the last 4 rows and the 4 x 4
    corner bin, and selects 64-px bins."""
    s = _BIG_SCENES[case](oracle)
    assert sc.expected_bin_size(s.width, s.height, s.height, s.triangles) == 64
    _, dep, stats = oracle.render(s)
    col, row, corner = ragged(dep)
    print(case, "columns", col, "rows", row, "corner", corner, stats)
    assert col > 0 and row > 0 and corner > 0, (col, row, corner)


def test_big_skybox_scene_has_sky_in_the_ragged_bins(oracle):
    """c1_cube_skybox at 4100 x 4100: the cube covers the middle, the sampled sky everything else (ragged bins
    included), so sky-queue indices reach the end of a 64 x 64 tile."""
    s = sc.c1_cube_skybox(1, BIG, BIG)
    s.skybox = sc.cubemap_faces()
    col, dep, _ = oracle.render(s)
    mesh = dep != BG
    assert mesh.sum() > 100000 and not mesh[:, -64:].any() and not mesh[-64:, :].any()
    sky = col[~mesh][:, :3].astype(np.int32)
    assert len(np.unique(sky[::997], axis=0)) > 50  # sampled, not uniform
    assert not mesh[63::64, 63::64].all()  # background at local pixel (63, 63) of some full tile: queue index 4095


def test_near_clip_big_measures(oracle):
    s = sc.near_clip_grid(BIG, BIG, 60)
    _, dep, stats = oracle.render(s)
    assert stats["triangles_clipped"] == 4 and stats["triangles_setup"] == 1183
    assert ragged(dep) == (14292, 16400, 16)


def test_pixel_aligned_big_snaps_to_quarter_pixels(oracle):
    """2 / 4100 is no power of two, so the products of the orthographic mapping are rounded; the float32 snap of
    DESIGN §4 still lands every vertex on its quarter pixel."""
    s = sc.pixel_aligned_triangles(BIG, BIG, 8000, 11)
    X, Y = sc.snapped_xy(s)
    assert (X % 64 == 0).all() and (Y % 64 == 0).all()
    p = s.vertices["position"].astype(np.float64)
    assert np.array_equal(X, np.rint(p[:, 0] * 256).astype(np.int64)) and np.array_equal(Y, np.rint(p[:, 1] * 256).astype(np.int64))
    _, dep, stats = oracle.render(s)
    assert stats["triangles_setup"] == 3871
    col, row, _ = ragged(dep)
    assert (col, row) == (1327, 908)
    total, _ = sc.bin_entry_counts(s, 64)
    assert int((total > 0).sum()) > 1000  # spread over the grid: the span walk runs in more than a thousand bins


def test_crowded_bins_entry_counts(oracle):
    """Per region at least 600 entries (three rounds of the 256-lane coverage loop, above the initial capacity of 256),
    and in the first region more large triangles than any large-triangle queue holds (1024)."""
    s = sc.crowded_bins(BIG, BIG)
    X, Y = sc.snapped_xy(s)
    assert (X % 64 == 0).all() and (Y % 64 == 0).all()
    total, large = sc.bin_entry_counts(s, 64)
    regions = sc.crowded_regions(BIG, BIG)
    assert regions[1][0] == 64 and regions[2][1] == 64 and regions[3] == (64, 64)  # ragged column, row, corner
    assert 0 < regions[0][0] < 64 and 0 < regions[0][1] < 64
    for bx, by in regions:
        print("region", bx, by, "entries", total[by, bx], "large", large[by, bx])
        assert total[by, bx] >= 600, (bx, by, total[by, bx])
    bx, by = regions[0]
    assert large[by, bx] >= 2200 > 1024
    _, dep, stats = oracle.render(s)
    assert stats["triangles_setup"] == _setup_count(s)  # the numpy set-up rules are the oracle's
    cov = dep != BG
    for bx, by in regions:
        assert cov[by * 64:by * 64 + 64, bx * 64:bx * 64 + 64].any()


def _setup_count(s):
    """Set-up triangles of an orthographic scene, from the snapped vertices (as bin_entry_counts keeps them)."""
    total, _ = sc.bin_entry_counts(s, max(s.width, s.height))
    return int(total[0, 0])


@pytest.mark.parametrize("w,h,draws,bin_px,big_area,queue", [(320, 240, 1, 16, 160, 512), (200, 120, 1, 32, 96, 192),
                                                              (200, 120, 3, 32, 96, 1024)])
def test_stacked_quads_overfill_the_large_queue(w, h, draws, bin_px, big_area, queue):
    """The bin-overflow scenes: the grid they select, and a bin with more large triangles than the instantiation's
    large-triangle queue (512 at 16 px, 192 for a single solid draw at 32 px, else 1024) and more entries than 256."""
    s = sc.stacked_quads(w, h, draws=draws, textured=draws > 1)
    assert sc.expected_bin_size(w, h, h, s.triangles) == bin_px
    total, large = sc.bin_entry_counts(s, bin_px, big_area)
    assert large.max() > queue and total.max() > 256, (large.max(), total.max())


@pytest.mark.parametrize("w,h,bin_px", [(320, 240, 16), (240, 180, 32), (BIG, BIG, 64)])
def test_dense_clip_properties(oracle, w, h, bin_px):
    s = sc.dense_clip(w, h)
    assert sc.expected_bin_size(w, h, h, s.triangles) == bin_px
    _, dep, stats = oracle.render(s)
    sizes = sc.clip_polygon_sizes(s)
    print(w, h, stats, np.bincount(sizes))
    assert stats["triangles_clipped"] >= 1000
    assert len(sizes) == stats["triangles_clipped"]  # the float64 clipper meets the same triangles
    assert (sizes == 3).sum() >= 100 and (sizes == 4).sum() >= 800
    assert (sizes >= 5).sum() >= 16  # near plane and guard-band planes: fan sub-triangles 3 and up
    assert (sizes == 8).sum() == 4 and sizes.max() == 8
    assert (dep != BG).all()  # the sheets: every pixel has a clipped fragment below the small triangles


def test_dense_clip_interleaves_clipped_and_unclipped(oracle):
    """Small clipped and unclipped triangles alternate in primitive order and overlap on screen: with the sheets taken
    out, most 64-pixel row pieces that hold a pixel of a clipped triangle also hold one of an unclipped triangle;
    and each of the four sheets is the visible one somewhere."""
    import copy

    w, h = 320, 240
    full = sc.dense_clip(w, h)
    n = full.indices.size // 3

    def only(keep):
        s = copy.copy(full)
        s.indices = full.indices.reshape(-1, 3)[keep].reshape(-1).copy()
        s.meshes = np.array([(0, s.indices.size, 0, 0)], s.meshes.dtype)
        return oracle.render(s)[1]

    small = np.arange(n) < n - 20
    clipped = only(small & (np.arange(n) % 2 == 0)) != BG
    plain = only(small & (np.arange(n) % 2 == 1)) != BG
    assert clipped.sum() > 5000 and plain.sum() > 5000
    pieces_c = clipped.reshape(h, w // 64, 64).any(-1)
    pieces_p = plain.reshape(h, w // 64, 64).any(-1)
    assert (pieces_c & pieces_p).sum() > 0.8 * pieces_c.sum()
    sheets = only(np.arange(n) >= n - 4)
    for k in range(4):
        mine = only(np.arange(n) == n - 4 + k)
        assert ((mine == sheets) & (mine != BG)).mean() > 0.05, k


def test_clip_flood_exceeds_both_clip_capacities(oracle):
    s = sc.clip_flood()
    assert sc.expected_bin_size(s.width, s.height, s.height, s.triangles) == 32
    _, _, stats = oracle.render(s)
    sizes = sc.clip_polygon_sizes(s)
    assert len(sizes) == stats["triangles_clipped"] >= 33000
    records, verts = int(np.maximum(sizes - 2, 0).sum()), int(sizes[sizes >= 3].sum())
    print("clip records", records, "polygon vertices", verts)
    assert records > sc.CLIP_RECORD_CAP and verts > sc.CLIP_VERTEX_CAP
    assert records <= 4 * sc.CLIP_RECORD_CAP and verts <= 4 * sc.CLIP_VERTEX_CAP  # one growth step (x4) suffices


def test_shadow_stack_overfills_a_map_bin(oracle, hiplib):
    """More than 256 caster triangles over one 32 x 32 texel bin of the map, counted from the light-space boxes."""
    s = sc.shadow_stack()
    assert sc.expected_bin_size(s.width, s.height, s.height, s.triangles) == 16
    lvp = np.array(s.shadow.light_view_proj, np.float64).reshape(4, 4).T
    p = s.vertices["position"].astype(np.float64)[s.indices.astype(np.int64)].reshape(-1, 3, 3)
    l = np.einsum("ij,tkj->tki", lvp[:, :3], p) + lvp[:, 3]
    size = s.shadow.size
    tx = (l[..., 0] * 0.5 + 0.5) * size
    ty = (l[..., 1] * 0.5 + 0.5) * size
    counts = np.zeros((size // 32, size // 32), np.int64)
    for t in range(p.shape[0]):
        x0, x1 = int(np.ceil(tx[t].min() - 0.5)), int(np.floor(tx[t].max() - 0.5))
        y0, y1 = int(np.ceil(ty[t].min() - 0.5)), int(np.floor(ty[t].max() - 0.5))
        if x0 > x1 or y0 > y1:
            continue
        counts[max(y0, 0) // 32:min(y1, size - 1) // 32 + 1, max(x0, 0) // 32:min(x1, size - 1) // 32 + 1] += 1
    print("map bin entries, largest", counts.max())
    assert counts.max() > 256
    smap = np.zeros((size, size), np.uint32)
    _, dep, stats = oracle.render(s, shadow_map_out=smap)
    assert (smap != BG).sum() > 1000 and (dep != BG).sum() > 20000


def test_grid_switch_pair_selects_both_grids(oracle):
    sparse, dense = sc.grid_switch_pair()
    assert sc.expected_bin_size(320, 240, 240, sparse.triangles) == 16
    assert sc.expected_bin_size(320, 240, 240, dense.triangles) == 32
    assert sparse.vertices is dense.vertices and sparse.indices is dense.indices
    a, b = oracle.render(sparse)[1], oracle.render(dense)[1]
    assert np.array_equal(a, oracle.render(sc.grid_c3(320, 240, 24))[1])
    assert np.array_equal(b, oracle.render(sc.grid_c3(320, 240, 60))[1])
    assert not np.array_equal(a, b)
