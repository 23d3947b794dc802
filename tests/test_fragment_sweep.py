"""The fragment stage over its parameter space, on the CPU: the oracle against the float64 restatement of Default.vert /
Default.frag (tests/test_oracle_clip_f64.py) for every scene of the sweep (scene_cases.shading_sphere, sampler_grid),
and the properties that make each scene what it claims to be (a head-on GGX peak, back-facing lights, fragments at a
light and on either side of a range boundary, every wrap branch of the sampler), computed in float64 from the scene
alone. tests/test_fragment_sweep_gpu.py renders the same scenes on the device and shares the float64 frames cached
here.
"""
import functools

import numpy as np
import pytest

import scene_cases as sc
import test_oracle_clip_f64 as f64

SHADING_CASES = [(rig, m, var) for rig in sc.SWEEP_RIGS for m in range(len(sc.SWEEP_MATERIALS))
                 for var in ("one", "one_vcol", "multi")]
SPHERE_MIN_PIXELS, GRID_MIN_PIXELS = 6000, 30000  # the counts the existing tests of these scenes assert


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def sphere_depth(variant):
    """f64_depth of the sweep's sphere (the rig and the material do not move it): (depth, margin)."""
    return _frozen(*f64.f64_depth(sc.shading_sphere("headon", 0, variant))[:2])


@functools.lru_cache(maxsize=None)
def shading_f64(rig, material, variant):
    """(float64 colour before the UNORM store [H, W, 4] as R, G, B, A; mask) of a shading case, computed once. The float64
    shader clamps the point-light count to 8 itself, so `eleven` is `eight`'s frame."""
    rig = "eight" if rig == "eleven" else rig
    return _frozen(*f64.f64_colour(sc.shading_sphere(rig, material, variant), *sphere_depth(variant)))


@functools.lru_cache(maxsize=None)
def sampler_depth():
    return _frozen(*f64.f64_depth(sc.sampler_case("3x5"))[:2])  # one grid under every uv transform


@functools.lru_cache(maxsize=None)
def sampler_f64(name):
    return _frozen(*f64.f64_colour(sc.sampler_case(name), *sampler_depth()))


def lsb_diff(bgra, ref, mask):
    """Per-channel |stored byte - rint(255 clamp(ref))| over the masked pixels of a B8G8R8A8 frame."""
    want = np.rint(np.clip(ref, 0, 1) * 255.0)
    return np.abs(bgra[..., [2, 1, 0, 3]].astype(np.float64) - want)[mask]


def interpolated(scene, fd, margin, pick):
    """The float64 pipeline's per-pixel varyings instead of its colour: f64_colour with its shader replaced by
    pick(P, N, vertex colour, uv) -> [n, <= 4] (the triangle search and the perspective-correct weights are f64_colour's
    own). Returns ([H, W, 4], mask)."""
    def varyings(scene_, draw, P, N, col, uv):
        out = np.zeros((len(P), 4))
        picked = pick(P, N, col, uv)
        out[:, :picked.shape[1]] = picked
        return out

    shade = f64._shade
    f64._shade = varyings
    try:
        return f64.f64_colour(scene, fd, margin)
    finally:
        f64._shade = shade


# ---- the oracle against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,material,variant", SHADING_CASES)
def test_oracle_matches_float64_shading(oracle, rig, material, variant):
    ref, mask = shading_f64(rig, material, variant)
    assert mask.sum() >= SPHERE_MIN_PIXELS
    assert np.isfinite(ref[mask]).all()
    bgra, _, _ = oracle.render(sc.shading_sphere(rig, material, variant))
    diff = lsb_diff(bgra, ref, mask)
    assert diff.max() <= 1, (rig, material, variant, diff.max())  # the bar of test_oracle_clip_f64._check_colour


@pytest.mark.parametrize("name", list(sc.SAMPLER_MODERATE))
def test_oracle_matches_float64_sampling(oracle, name):
    ref, mask = sampler_f64(name)
    assert mask.sum() >= GRID_MIN_PIXELS
    bgra, _, _ = oracle.render(sc.sampler_case(name))
    diff = lsb_diff(bgra, ref, mask)
    assert diff.max() <= 1, (name, diff.max())


@pytest.mark.parametrize("name", list(sc.SAMPLER_LARGE))
def test_large_uv_frames_are_not_constant(oracle, name):
    """uvs in the thousands leave float64 by tens of LSB (float32 uv precision, inherent to the shader), so these cases
    have the oracle alone as their reference: its frame must at least be a textured one."""
    s = sc.sampler_case(name)
    tw, th = s.textures[0][1].shape[1], s.textures[0][1].shape[0]
    d = s.draws[0].pc
    uv = s.vertices["texcoord"].astype(np.float64) * np.array(d.texture_scale) * d.tiling_factor + np.array(d.texture_offset)
    assert np.abs(uv * (tw, th)).max() < 2 ** 20
    assert np.abs(uv).max() > 1000
    bgra, dep, _ = oracle.render(s)
    colours = np.unique(bgra[dep != 0x3F800000].view(np.uint32))
    assert colours.size >= 100, colours.size


# ---- what the scenes claim, from the scene alone -------------------------------------------------------------------
# Over every pixel the float64 raster covers (margin >= 0: the GPU tests compare every pixel with the oracle, not only
# the half-pixel interior that the float64 colours mask). The counts beside the assertions are those of the default
# 320 x 240, 40 x 60 sphere and the 320 x 180, n = 30 grid.
@functools.lru_cache(maxsize=None)
def sphere_surface():
    """World position and unit normal [n, 3] of the covered pixels of the sweep's sphere, float64."""
    s = sc.shading_sphere("headon", 0, "one")
    fd, margin = sphere_depth("one")
    P, mask = interpolated(s, fd, margin + 0.5, lambda P, N, col, uv: P)
    N, mask_n = interpolated(s, fd, margin + 0.5, lambda P, N, col, uv: N)
    assert np.array_equal(mask, mask_n) and mask.sum() >= SPHERE_MIN_PIXELS
    P, N = P[mask][:, :3], N[mask][:, :3]
    return _frozen(P, N / np.linalg.norm(N, axis=1, keepdims=True))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _view(P):
    return _unit(np.array([0.0, 0.0, 9.0]) - P)


def _pre_tone(ref, mask):
    """The colour before Reinhard and the gamma, recovered from the float64 frame: c = t / (1 - t), t = stored^2.2."""
    t = ref[mask][:, :3] ** 2.2
    return t / (1.0 - t)


def test_headon_has_the_ggx_peak():
    P, N = sphere_surface()
    H = _unit(_view(P) + np.array([0.0, 0.0, 1.0]))
    assert ((N * H).sum(1) > 0.9999).sum() >= 4  # the four pixels around the frame's centre (found: 4)
    # and drives HDR radiance into the tone curve: roughness 0.045 under intensity 50 (found: 109 before the tone curve)
    assert (_pre_tone(*shading_f64("headon", 1, "one")) > 100.0).any()


def test_back_faces_away_from_the_sun():
    P, N = sphere_surface()
    L = -_unit(np.array([0.05, 0.03, 1.0]))
    assert ((N @ L) <= 0.0).mean() > 0.9  # (found: every covered pixel)
    assert np.linalg.norm(_view(P) + L, axis=1).min() >= 1e-3  # never exactly opposite (found: 1.4e-3, at the silhouette)
    near = np.linalg.norm(np.array([0.0, 0.0, 3.001]) - P, axis=1)
    assert (near < 0.05).sum() >= 4  # the point light 1e-3 off the surface (found: 12)


def test_touch_reaches_a_light_and_crosses_a_range():
    P, _ = sphere_surface()
    lights = sc.sweep_lights("touch")
    dist = [np.linalg.norm(np.array(L["position"]) - P, axis=1) for L in lights]
    assert (np.minimum.reduce(dist) < 0.05).sum() >= 4  # (found: 12, the nearest 0.02 away)
    pos, rng = sc.TOUCH_RANGE_LIGHT
    d = np.linalg.norm(np.array(pos) - P, axis=1)
    assert (d < rng).sum() >= 100 and (d >= rng).sum() >= 100  # (found: 939 inside, 15981 outside)
    # the light at the centre: every fragment at the same distance inside its range, facing away from it
    assert (dist[1] < lights[1]["range"]).all()


def test_eight_has_hdr_radiance_and_dead_lights():
    P, _ = sphere_surface()
    lights = sc.sweep_lights("eight")
    assert len(lights) == 11
    inside = [int((np.linalg.norm(np.array(L["position"]) - P, axis=1) < L["range"]).sum()) for L in lights]
    # ranges 0 and 1e-5 reach nothing; nor does the 1e4 light: the spiral keeps it 2.59 from the surface, beyond its
    # range of 2, so however bright, it must add exactly nothing (a kernel that dropped the range test would show it)
    assert inside[2] == inside[3] == inside[6] == 0
    assert all(inside[k] > 0 for k in (0, 1, 4, 5, 7))
    assert all(n == len(P) for n in inside[8:])  # the three dropped lights would light every pixel
    # HDR into the tone curve all the same: the grazing GGX peaks of roughness 0.045 (found: 2039 before the tone curve)
    assert (_pre_tone(*shading_f64("eight", 1, "one")) > 100.0).any()


def test_alpha_exceeds_one():
    for variant in ("one", "one_vcol", "multi"):
        ref, mask = shading_f64("headon", 1, variant)
        assert (ref[mask][:, 3] > 1.0).any()  # base 1.3 (x tint 1.2 x texel alpha in the second draw of multi)


@pytest.mark.parametrize("name", list(sc.SAMPLER_MODERATE) + list(sc.SAMPLER_LARGE))
def test_sampler_cases_take_every_wrap_branch(name):
    s = sc.sampler_case(name)
    fd, margin = sampler_depth()
    uv, mask = interpolated(s, fd, margin + 0.5, lambda P, N, col, uv: uv)
    assert mask.sum() >= GRID_MIN_PIXELS
    th, tw = s.textures[0][1].shape[:2]
    fx, fy = np.floor(uv[mask][:, 0] * tw - 0.5), np.floor(uv[mask][:, 1] * th - 0.5)
    x0, y0 = fx.astype(np.int64) % tw, fy.astype(np.int64) % th
    assert (x0 == tw - 1).sum() >= 100 and (y0 == th - 1).sum() >= 100  # x1, y1 wrap to 0 (found: >= 2748 each)
    if tw == 1:
        assert ((x0 + 1) % tw == x0).all()
    if th == 1:
        assert ((y0 + 1) % th == y0).all()
    # floor(u w - 0.5) < 0 and floor(v h - 0.5) < 0, wherever the case's transform takes the mesh's uvs ([0, 4]^2) below
    # half a texel at all (found: >= 66 pixels each). It cannot in u for 7x1 (u >= 0.5), in v for 5x3_neg (v >= 100.25)
    # and 6x10_offset4096 (v >= 4096), and in either for 3x3_tiling1000 beyond the two pixels at the grid's corner.
    if name not in ("7x1", "3x3_tiling1000"):
        assert (fx < 0).sum() >= 50, name
    if name not in ("5x3_neg", "3x3_tiling1000", "6x10_offset4096"):
        assert (fy < 0).sum() >= 50, name
