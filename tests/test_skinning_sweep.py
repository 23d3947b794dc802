"""The skinning branch of the vertex stage over its parameter space, on the CPU: the oracle against the float64
restatement of Default.vert:64-90 (test_oracle_clip_f64.f64_skin) for every form of scene_cases.skinned_sphere, and the
proof that those scenes can tell a wrong vertex stage from a right one: the float64 pipeline run with one defect at a
time must leave the true float64 frame by more than the 2 LSB that the device tests allow.
tests/test_skinning_sweep_gpu.py renders the same scenes on the device and shares the float64 frames cached here.

Measured on the default 320 x 240 frames (masked pixels: margin >= 0.5 and the winning triangle found again):

    form            masked   covered by the oracle   triangles clipped
    one               4882   14312                    0
    nonunit0.6        4882   14312                    0
    nonunit1.5        4882   14312                    0
    skips             4832   14142                   30
    short_palette     5284   15281                    0
    multi             6958   18360                    0

Every form is within 1 LSB of float64 under every rig, and the largest excess over the depth formula of
test_oracle_clipping_and_depth_match_float64_vulkan_rules is -2.2e-6 (inside it).

Share of the true frame's masked pixels that a defect moves by more than 2 LSB (pixels masked in both frames; a pixel
the defect uncovers counts as unmoved), rigs headon / eight / touch:

    normals not skinned (one)                        87.1 %   92.9 %   10.9 %
    mat3(S) transposed (one)                         90.2 %   96.6 %   10.2 %
    bone_offset ignored (one)                        32.0 %   32.0 %   32.0 %
    idx >= bone_count skip removed (skips)           21.9 %   23.8 %   23.4 %
    palette-length skip removed (short_palette)      37.2 %   37.9 %   38.0 %
    second skinned draw at the first's offset (multi) 11.4 %   11.4 %   11.4 %
"""
import copy
import functools

import numpy as np
import pytest

import scene_cases as sc
import test_oracle_clip_f64 as f64
from test_fragment_sweep import _frozen, lsb_diff

F64_FORMS = tuple(f for f in sc.SKIN_FORMS if f != "shadow")
CASES = [(rig, m, form) for rig, m in sc.SKIN_RIG_MATERIALS for form in F64_FORMS]
# the single-sphere forms: 4000 (measured 4832 .. 5284); multi: 6000 (measured 6958: the sphere at 0.8 of its size and
# two coarser ones at half)
MIN_PIXELS = {form: 6000 if form == "multi" else 4000 for form in F64_FORMS}
DEFECT_LSB, DEFECT_SHARE = 2, 0.01


def _material(rig):
    return dict(sc.SKIN_RIG_MATERIALS)[rig]


@functools.lru_cache(maxsize=None)
def skin_depth(form, defect=None):
    """f64_depth of a form (the rig and the material do not move it): (depth, margin, gradient)."""
    return _frozen(*f64.f64_depth(sc.skinned_sphere("headon", 3, form), defect)[:3])


@functools.lru_cache(maxsize=None)
def skin_f64(rig, form, defect=None):
    """(float64 colour before the UNORM store [H, W, 4] as R, G, B, A; mask) of a case, computed once."""
    fd, margin, _ = skin_depth(form, defect)
    return _frozen(*f64.f64_colour(sc.skinned_sphere(rig, _material(rig), form), fd, margin, defect))


def check_depth(od_bits, form):
    """The oracle's (or a device's) depth against float64 at the bar of
    test_oracle_clipping_and_depth_match_float64_vulkan_rules, on margin >= 0.5."""
    fd, margin, grad = skin_depth(form)
    od = od_bits.view(np.float32).astype(np.float64)
    interior = margin >= 0.5
    assert (od[interior] < 1.0).all()
    tol = grad * (2.0 / 256.0) + 4e-7 + 2e-6 * np.abs(fd)
    err = np.abs(od - fd)
    assert (err[interior] <= tol[interior]).all(), float((err - tol)[interior].max())


# ---- the oracle against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,material,form", CASES)
def test_oracle_matches_float64_skinning(oracle, rig, material, form):
    ref, mask = skin_f64(rig, form)
    assert mask.sum() >= MIN_PIXELS[form], mask.sum()
    assert np.isfinite(ref[mask]).all()
    s = sc.skinned_sphere(rig, material, form)
    bgra, od_bits, stats = oracle.render(s)
    diff = lsb_diff(bgra, ref, mask)
    print(f"{s.name}: {int(mask.sum())} masked pixels, largest difference {diff.max():g} LSB")
    assert diff.max() <= 1, (s.name, diff.max())  # the bar of test_oracle_clip_f64._check_colour
    check_depth(od_bits, form)
    if form == "skips":
        assert stats["triangles_clipped"] > 0  # the triangles around a vertex skinned to (0, 0, 0, 0)


def test_weights_reach_the_clip_stage_off_one():
    """What the forms claim about w, from the float64 skin alone."""
    for form, lo, hi in (("one", 1.0, 1.0), ("nonunit0.6", 0.6, 1.0), ("nonunit1.5", 1.0, 1.5)):
        s = sc.skinned_sphere("headon", 3, form)
        w = f64.f64_skin(s, s.draws[0])[0][:, 3]
        assert abs(w.min() - lo) < 1e-6 and abs(w.max() - hi) < 1e-6, (form, w.min(), w.max())
    s = sc.skinned_sphere("headon", 3, "short_palette")
    w = f64.f64_skin(s, s.draws[0])[0][:, 3]
    assert abs(w.min() - 0.75) < 1e-6 and w.max() == 1.0  # bone 2 dropped: 1 - w2, w2 up to 0.25
    s = sc.skinned_sphere("headon", 3, "multi")
    assert [d.pc.bone_count for d in s.draws] == [3, 0, 2] and [d.pc.bone_offset for d in s.draws] == [1, 0, 4]
    assert f64.f64_skin(s, s.draws[2])[0][:, 3].min() < 0.8  # index 2 is out of that draw's range
    assert (f64.f64_skin(s, s.draws[1])[0][:, 3] == 1.0).all()


def test_skips_patch_and_dead_vertices():
    s = sc.skinned_sphere("headon", 3, "skips")
    sp, sn = f64.f64_skin(s, s.draws[0])
    dead = sc.skinned_dead_vertices()
    assert (sp[dead] == 0.0).all() and (sn[dead] == 0.0).all()
    one = sc.skinned_sphere("headon", 3, "one")
    # the patch's fourth influences are all skipped: the skin of every live vertex is `one`'s
    live = np.setdiff1d(np.arange(len(sp)), dead)
    assert np.array_equal(sp[live], f64.f64_skin(one, one.draws[0])[0][live])
    idx, w = s.vertices["bone_indices"], s.vertices["bone_weights"]
    count = s.draws[0].pc.bone_count
    patch = [r * 61 + sg for r in sc.SKIN_PATCH[0] for sg in sc.SKIN_PATCH[1]]
    for rule in (w[patch, 3] < 0, (w[patch, 3] == 0) & (idx[patch, 3] == 1), idx[patch, 3] == -1, idx[patch, 3] == count):
        assert rule.sum() >= 15
    # the read that only bone_count keeps out lies inside the uploaded palette
    assert s.draws[0].pc.bone_offset + count < len(s.bones)
    assert (s.bones[0] == sc.SKIN_SENTINEL).all()


def test_dead_vertices_ignore_their_normals(oracle):
    """A vertex whose every influence is skipped collapses to (0, 0, 0, 0) and its triangles lose their area to the clip at
    w >= 1e-5: its normal must not reach the frame. (The float32 clipper leaves slivers of those triangles on 15 pixels
    of this frame; their normal is normalize(0) whatever the record holds, and the oracle stores black there, as
    the device must: tests/test_skinning_sweep_gpu.py, test_skinning_sweep.)"""
    s = sc.skinned_sphere("eight", 0, "skips")
    bgra, dep, _ = oracle.render(s)
    v = s.vertices.copy()
    v["normal"][sc.skinned_dead_vertices()] = [(0, 1, 0), (-1, 0, 0), (3, -2, 5), (0.6, 0.0, -0.8), (1e3, 1e3, 1e3)]
    s.vertices = v
    bgra2, dep2, _ = oracle.render(s)
    assert bgra.tobytes() == bgra2.tobytes() and dep.tobytes() == dep2.tobytes()


def test_shadow_box_holds_the_skinned_casters(oracle):
    """The light box is fitted to the skinned positions, so no caster leaves the map; and the map of the skinned sphere
    is not the bind pose's (a shadow_vertex fed the unskinned position would show in the map)."""
    s = sc.skinned_sphere("headon", 3, "shadow")
    lvp = np.array(s.shadow.light_view_proj, np.float64).reshape(4, 4)  # [col][row]
    world = sc.skinned_world_f64(s)
    ndc = np.c_[world, np.ones(len(world))] @ lvp
    assert (np.abs(ndc[:, :2]) <= 1.0).all() and (ndc[:, 2] >= 0.0).all() and (ndc[:, 2] <= 1.0).all()
    size = s.shadow.size
    skinned, bind = np.zeros((size, size), np.uint32), np.zeros((size, size), np.uint32)
    oracle.render(s, shadow_map_out=skinned)
    u = copy.copy(s)
    u.draws = [copy.deepcopy(d) for d in s.draws]
    u.draws[0].pc.bone_count = 0
    oracle.render(u, shadow_map_out=bind)
    assert (skinned != 0x3F800000).sum() > 50000  # the ground fills the map (found: 62500 of 65536 texels)
    assert (skinned != bind).mean() > 0.05  # (found: 9.9 % of the texels)


# ---- defect discrimination -----------------------------------------------------------------------------------------------
def _moved_share(true, defective):
    (ref, mask), (bad, bad_mask) = true, defective
    both = mask & bad_mask
    lsb = np.abs(np.rint(np.clip(ref, 0, 1) * 255.0) - np.rint(np.clip(bad, 0, 1) * 255.0)).max(-1)
    return float(((lsb > DEFECT_LSB) & both).sum()) / float(mask.sum())


def _defective_frame(rig, defect):
    """(true frame, defective frame) of the form that shows the defect, both from the float64 pipeline."""
    if defect in ("normals_unskinned", "mat3_transposed", "offset_ignored"):
        return skin_f64(rig, "one"), skin_f64(rig, "one", defect)
    if defect == "count_skip_removed":
        return skin_f64(rig, "skips"), skin_f64(rig, "skips", defect)
    if defect == "palette_skip_removed":
        # a vertex stage without the palette-length skip reads the row that lies behind the short palette: the full
        # palette's last row, so its frame is `one`'s
        return skin_f64(rig, "short_palette"), skin_f64(rig, "one")
    assert defect == "second_draw_first_offset"
    s = sc.skinned_sphere(rig, _material(rig), "multi")
    s.draws[2].pc.bone_offset = s.draws[0].pc.bone_offset
    fd, margin = f64.f64_depth(s)[:2]
    return skin_f64(rig, "multi"), f64.f64_colour(s, fd, margin)


@pytest.mark.parametrize("rig", [rig for rig, _ in sc.SKIN_RIG_MATERIALS])
@pytest.mark.parametrize("defect", list(f64.SKIN_DEFECTS) + ["palette_skip_removed", "second_draw_first_offset"])
def test_scenes_discriminate_defect(rig, defect):
    """A condition on the scenes, not on any implementation: each mistake the suite used to miss moves at least 1 % of
    the masked pixels by more than the 2 LSB that the device tests allow against float64. Measured shares: this module's
    docstring."""
    share = _moved_share(*_defective_frame(rig, defect))
    print(f"{defect} under {rig}: {100 * share:.1f} % of the masked pixels move by more than {DEFECT_LSB} LSB")
    assert share >= DEFECT_SHARE, (defect, rig, share)
