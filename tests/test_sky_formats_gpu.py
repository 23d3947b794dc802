"""GPU checks of tri_upload_skybox_ex and k_sky_fill: the skybox pass for R8G8B8A8_UNORM and
R16G16B16A16_SFLOAT cubemaps and for mip chains, run ahead of the raster kernels, which then store no background pixel.

The bar is the project's: every colour channel within 1 LSB, alpha 255 on sky pixels, depth bit-exact where meshes are
drawn. One-level sRGB with TRI_SKYBOX_PREFILL is checked against the oracle; the new formats and the chains against the
float64 restatement in sky_general_ref.py, which may leave out only the pixels whose two largest direction components
are within 1e-6 of each other (under 2 % of a frame, asserted). The cameras' aspect ratios differ slightly from their
frames', so that no diagonal of pixel centres lies exactly on a face boundary (a 48 x 32 frame with square pixels has 3 %
of its pixels there).

The 6 -> 3 -> 1 chain cannot show three values of floor(d): d = 2 needs rho >= 4, where a face of the 6-texel level
spans under two pixels. Its frame is asserted to reach d > 1.5 instead, so every one of its levels carries weight.
"""
import copy

import numpy as np
import pytest

import scene_cases as sc
import sky_general_ref as ref

pytestmark = pytest.mark.gpu

BG = 0x3F800000
CAM = (0.0, 3.0, 8.0)


def sky_scene(w, h, fov, aspect_w=None):
    """No meshes, no in-raster skybox: the editor camera over a w x h frame, its aspect ratio that of aspect_w x h."""
    from trident_raster import scenes

    s = sc.skybox_only(w, h, fov, (0.0, 0.0, 0.0), None)
    view, proj = scenes.editor_camera(CAM, (0.0, 0.0, 0.0), fov, (w if aspect_w is None else aspect_w, h), 0.1, 1000.0)
    s.ubo = scenes.pack_ubo(view, proj, CAM)
    s.skybox = None
    return s


def render_ex(scene, texels, fmt, n, mips=1, flags=0, band=None, ctx_flags=0, stats=None):
    """The scene on the GPU with the cubemap uploaded through tri_upload_skybox_ex."""
    from trident_raster import raster, scenes

    s = copy.copy(scene)
    s.skybox = None
    with raster.TriRaster(scene.width, scene.height, band=band, flags=ctx_flags) as r:
        scenes.load_scene(r, s)
        r.upload_skybox_ex(texels, fmt, n, mips, flags)
        r.render_frame()
        if stats is not None:
            stats.update(r.frame_stats())
        return r.readback()


def assert_oracle_parity(scene, oracle, ctx_flags=0):
    from trident_raster import abi

    n = scene.skybox.shape[1]
    gc, gd = render_ex(scene, scene.skybox, abi.TRI_SKY_FMT_RGBA8_SRGB, n, 1, abi.TRI_SKYBOX_PREFILL, ctx_flags=ctx_flags)
    oc, od, _ = oracle.render(scene)
    assert np.array_equal(gd, od)
    diff = np.abs(gc.astype(np.int16) - oc.astype(np.int16))
    print("max colour difference vs the oracle:", int(diff.max()), "LSB;", int((diff > 0).sum()), "channels differ")
    assert int(diff.max()) <= 1
    assert (gc[..., 3][od == BG] == oc[..., 3][od == BG]).all()
    return gc, oc, od


# ---- 1. forced prefill against the oracle ------------------------------------------------------------------------------
def test_prefill_sky_only_matches_oracle(oracle):
    s = sc.skybox_only(96, 64, 100.0, (0.0, 0.0, 0.0), sc.cubemap_faces(8, seed=5))
    gc, _, _ = assert_oracle_parity(s, oracle)
    assert (gc[..., 3] == 255).all()


@pytest.mark.parametrize("exact", [False, True])
def test_prefill_cube_over_sky_matches_oracle(oracle, exact):
    from trident_raster import abi

    s = sc.c1_cube_skybox(1, 96, 64)
    s.skybox = sc.cubemap_faces(8, seed=5)
    _, _, od = assert_oracle_parity(s, oracle, abi.TRI_FLAG_EXACT_SHADING if exact else 0)
    assert (od != BG).sum() > 40 and (od == BG).sum() > 100  # (the cube covers 48 pixels of this frame)


def test_prefill_orthographic_camera_keeps_clear_colour(oracle):
    from test_skybox import skybox_runtime_camera

    s = skybox_runtime_camera(1, 96, 64, ortho=30.0)
    s.skybox = sc.cubemap_faces(8, seed=5)
    gc, oc, _ = assert_oracle_parity(s, oracle)
    missed = np.all(oc == np.array([1, 1, 1, 255], np.uint8), axis=-1)  # unorm8(0.005) = 1
    assert missed.any() and (~missed).any()
    assert np.array_equal(gc[missed], oc[missed])


# ---- 2. the new formats against the float64 reference ------------------------------------------------------------------
def seeded_texels(fmt, n, mips=1, seed=7):
    """[chain, 4] texels: bytes for the 8-bit formats; for RGBA16F seeded values in [0, 4] (some saturate) with a few
    zeros and subnormal halves, no Inf or NaN."""
    rng = np.random.default_rng(seed + 31 * n + fmt)
    count = ref.chain_texels(n, mips)
    if fmt != ref.FMT_16F:
        return rng.integers(0, 256, size=(count, 4), dtype=np.uint8)
    t = rng.uniform(0.0, 4.0, size=(count, 4)).astype(np.float16)
    t[rng.random((count, 4)) < 0.5] *= np.float16(0.25)  # half of them below 1
    flat = t.reshape(-1)
    flat[::7] = np.float16(0.0)
    flat[3::11] = np.array(0x0155, np.uint16).view(np.float16)  # a subnormal
    return t.view(np.uint16)


def assert_reference_parity(scene, texels, fmt, n, mips=1, band=None, got=None):
    rgb, cov, tie, d = ref.render(scene, texels, fmt, n, mips, band=band)
    assert tie.mean() < 0.02, tie.mean()
    gc, gd = render_ex(scene, texels, fmt, n, mips, band=band) if got is None else got
    want = ref.expected_bytes(rgb)
    diff = np.abs(gc[..., [2, 1, 0]].astype(np.float64) - want)[~tie]
    print(f"fmt {fmt} n {n} mips {mips}: max difference {diff.max():g} LSB, {tie.sum()} pixels left out, "
          f"{int((want >= 255).any(axis=-1).sum())} saturated")
    assert diff.max() <= 1
    assert (gc[..., 3][cov] == 255).all()
    assert (gd == BG).all()
    return gc, d, cov


ONE_LEVEL = [(fmt, n, (96, 64)) for fmt in (ref.FMT_UNORM, ref.FMT_16F) for n in (1, 2, 6, 8)] + \
            [(fmt, n, (97, 63)) for fmt in (ref.FMT_UNORM, ref.FMT_16F) for n in (1, 6)]


@pytest.mark.parametrize("fmt,n,size", ONE_LEVEL)
def test_one_level_formats_match_reference(fmt, n, size):
    s = sky_scene(size[0], size[1], 100.0, aspect_w=size[0] + 5)
    assert_reference_parity(s, seeded_texels(fmt, n), fmt, n)


def test_unorm_and_srgb_decode_differ():
    from trident_raster import abi

    s = sky_scene(96, 64, 100.0, aspect_w=101)
    t = seeded_texels(ref.FMT_UNORM, 8)
    a, _ = render_ex(s, t, abi.TRI_SKY_FMT_RGBA8_UNORM, 8)
    b, _ = render_ex(s, t, abi.TRI_SKY_FMT_RGBA8_SRGB, 8, 1, abi.TRI_SKYBOX_PREFILL)
    assert (a[..., :3].astype(np.int16) - b[..., :3].astype(np.int16) >= 0).all()  # the sRGB decode darkens
    assert (a != b).mean() > 0.5


def test_hdr_values_saturate():
    s = sky_scene(96, 64, 100.0, aspect_w=101)
    t = np.full((ref.chain_texels(2, 1), 4), np.float16(3.5)).view(np.uint16)
    gc, _ = render_ex(s, t, ref.FMT_16F, 2)
    assert (gc == 255).all()


def test_frame_alpha_and_invalid_descriptors():
    """tri_frame_alpha keeps proving 255 under a k_sky_fill sky; TRI_E_INVALID for what the header lists."""
    from trident_raster import abi, raster

    s = sky_scene(96, 64, 100.0)
    t16 = seeded_texels(ref.FMT_16F, 8, 4)
    with raster.TriRaster(96, 64) as r:
        from trident_raster import scenes

        scenes.load_scene(r, s)
        r.upload_skybox_ex(t16, abi.TRI_SKY_FMT_RGBA16F, 8, 4)
        assert r.frame_alpha() == 255
        bad = [(t16[:-1], abi.TRI_SKY_FMT_RGBA16F, 8, 4),           # a wrong byte count
               (t16, abi.TRI_SKY_FMT_RGBA16F, 8, 3),
               (t16, abi.TRI_SKY_FMT_RGBA16F, 0, 1),                # a zero size with texels
               (t16, abi.TRI_SKY_FMT_RGBA16F, 16385, 1),            # over-large
               (seeded_texels(ref.FMT_16F, 8, 5), abi.TRI_SKY_FMT_RGBA16F, 8, 5),  # too many levels (8 has 4)
               (t16, abi.TRI_SKY_FMT_RGBA16F, 8, 0),
               (t16, 3, 8, 4)]                                      # an unknown format
        for texels, fmt, n, mips in bad:
            with pytest.raises(raster.TriError) as e:
                r.upload_skybox_ex(texels, fmt, n, mips)
            assert e.value.code == abi.TRI_E_INVALID, (fmt, n, mips)
        with pytest.raises(raster.TriError):
            r.upload_skybox_ex(t16, abi.TRI_SKY_FMT_RGBA16F, 8, 4, flags=0x2)
        r.render_frame()  # the refused uploads left the cubemap alone
        got = r.readback()
    assert_reference_parity(s, t16, ref.FMT_16F, 8, 4, got=got)


# ---- 3. mip chains against the reference -------------------------------------------------------------------------------
TINTS = np.array([(0.1, 0.1, 0.1), (0.4, 0.1, 0.7), (0.7, 0.4, 0.1), (0.1, 0.7, 0.4), (0.7, 0.7, 0.7), (0.1, 0.4, 0.4),
                  (0.4, 0.7, 0.1), (0.7, 0.1, 0.4)])  # any two at least 0.3 apart in some channel


def tinted_chain(n, mips, seed=3):
    """RGBA16F: level l is TINTS[l] plus seeded noise of 0.05, so a wrong level or blend weight shows."""
    rng = np.random.default_rng(seed)
    parts = []
    for l, e in enumerate(ref.level_sizes(n, mips)):
        t = np.ones((6 * e * e, 4))
        t[:, :3] = TINTS[l] + rng.uniform(0.0, 0.05, size=(6 * e * e, 3))
        parts.append(t)
    return np.concatenate(parts).astype(np.float16).view(np.uint16)


MINIFY = {128: (150.0, 53), 6: (150.0, 480)}  # (field of view, aspect width) of the 48 x 32 frame that minifies


@pytest.fixture(scope="module")
def chains():
    return {(128, 8): tinted_chain(128, 8), (6, 3): tinted_chain(6, 3)}


@pytest.mark.parametrize("n,mips", [(128, 8), (6, 3)])
def test_mip_chain_minified_matches_reference(chains, n, mips):
    fov, aw = MINIFY[n]
    _, d, cov = assert_reference_parity(sky_scene(48, 32, fov, aspect_w=aw), chains[(n, mips)], ref.FMT_16F, n, mips)
    floors = np.unique(np.floor(d[cov]))
    print("floor(d) takes", floors, "max d", d[cov].max())
    if n == 128:
        assert floors.size >= 3  # otherwise the frame proves nothing about the level choice
    else:
        assert floors.size >= 2 and d[cov].max() > 1.5  # (see the module's docstring)


@pytest.mark.parametrize("n,mips", [(128, 8), (6, 3)])
def test_mip_chain_magnified_matches_reference(chains, n, mips):
    _, d, cov = assert_reference_parity(sky_scene(48, 32, 12.0, aspect_w=53), chains[(n, mips)], ref.FMT_16F, n, mips)
    assert (d[cov] == 0.0).any()  # lambda = 0 occurs


def test_mip_chain_of_8_bit_formats_matches_reference():
    s = sky_scene(48, 32, 150.0, aspect_w=53)
    for fmt in (ref.FMT_SRGB, ref.FMT_UNORM):
        assert_reference_parity(s, seeded_texels(fmt, 16, 5), fmt, 16, 5)


# ---- 4. bands -----------------------------------------------------------------------------------------------------------
def test_bands_with_odd_first_rows_equal_the_full_frame(chains):
    s = sky_scene(48, 32, 150.0, aspect_w=53)
    t = chains[(128, 8)]
    full, _ = render_ex(s, t, ref.FMT_16F, 128, 8)
    for band in [(0, 5), (5, 18), (17, 32)]:
        part, _ = render_ex(s, t, ref.FMT_16F, 128, 8, band=band)
        assert np.array_equal(part, full[band[0]:band[1]]), band


# ---- 5. every raster family over a prefilled sky -----------------------------------------------------------------------
def family_scene(family):
    from test_frame_kinds_gpu import grid_scene
    from trident_raster import scenes

    s = grid_scene("sky_family_" + family)
    if family == "shadow":
        s = scenes.with_shadow(s, size=256)
    if family == "ai":
        s = scenes.with_ai_blend(s)
    return s


@pytest.mark.parametrize("family", ["plain", "kind", "shadow", "ai"])
def test_raster_families_over_a_prefilled_sky(family):
    from trident_raster import abi

    s = family_scene(family)
    faces, n = s.skybox, s.skybox.shape[1]
    ctx_flags = abi.TRI_FLAG_EXACT_SHADING if family == "plain" else 0  # no frame kind is built for the exact build
    srgb = abi.TRI_SKY_FMT_RGBA8_SRGB
    st_a, st_b = {}, {}
    a, da = render_ex(s, faces, srgb, n, 1, 0, ctx_flags=ctx_flags, stats=st_a)  # the in-raster sky pass
    b, db = render_ex(s, faces, srgb, n, 1, abi.TRI_SKYBOX_PREFILL, ctx_flags=ctx_flags, stats=st_b)
    assert st_a["path"] == st_b["path"]
    assert bool(st_b["path"] & abi.TRI_PATH_KIND) == (family == "kind")
    assert bool(st_b["path"] & abi.TRI_PATH_SHADOW) == (family == "shadow")
    sky_only = copy.copy(s)
    sky_only.draws = []
    sky_only.shadow = None
    c, _ = render_ex(sky_only, faces, srgb, n, 1, abi.TRI_SKYBOX_PREFILL, ctx_flags=ctx_flags)
    assert np.array_equal(da, db)
    mesh = db != BG
    assert mesh.sum() > 500 and (~mesh).sum() > 500
    assert np.array_equal(b[mesh], a[mesh])   # mesh pixels: the same frame with the in-raster sky, bit for bit
    assert np.array_equal(b[~mesh], c[~mesh])  # sky pixels: the sky-only frame
    assert int(np.abs(a[~mesh].astype(np.int16) - b[~mesh].astype(np.int16)).max()) <= 1
    assert (b[~mesh][:, 3] == 255).all()


# ---- 6. through the shim -----------------------------------------------------------------------------------------------
def test_shim_finds_and_renders_default_skybox_ktx(tmp_path):
    """Assets/Skyboxes/DefaultSkybox.ktx (RGBA16F with a chain) is found at Init; the rendered frame is the C-ABI frame,
    and ReadViewportPixels and the AI input tensor contain the sky."""
    import os
    import shutil

    import tensor_ref
    from trident_raster import app, scenes

    fixture = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sky", "rgba16f_n4_chain.ktx")
    sky_dir = tmp_path / "Assets" / "Skyboxes"
    sky_dir.mkdir(parents=True)
    shutil.copy(fixture, str(sky_dir / "DefaultSkybox.ktx"))
    info, texels, source = app.load_default_skybox_ex(str(tmp_path / "Assets"))
    assert source == "DefaultSkybox.ktx" and (info["format"], info["size"], info["mip_count"]) == (ref.FMT_16F, 4, 3)
    w, h = 96, 64
    a = app.TridentApp()
    assert a.set_assets_dir(str(tmp_path / "Assets")) == "DefaultSkybox.ktx"
    a.set_camera("editor", (0.0, 3.0, 8.0), (-10.0, 25.0, 0.0))
    a.set_viewport(1, w, h)
    a.add_mesh_entity("sphere", position=(0.0, 3.0, 4.0))
    assert a.set_ai_readback(True, 0, 0)
    a.draw_frame()
    a.draw_frame()
    a.finish_frame()
    tensor = a.acquire_frame()
    rgba, depth = a.read_pixels(1, w, h)
    ubo, draws = a.frame_inputs(1)
    vb, ib, ranges = a.geometry()
    s = scenes.Scene("shim_sky_ktx", w, h, vb, ib, ranges, draws, ubo, materials=[(m[0], m[1]) for m in a.materials()],
                     skybox=None)
    a.close()
    gc, gd = render_ex(s, texels.view(np.uint16).reshape(-1, 4), ref.FMT_16F, 4, 3)
    assert np.array_equal(depth.view(np.uint32), gd)
    assert np.array_equal(rgba, gc[..., [2, 1, 0, 3]])  # the shim's frame is the C-ABI frame
    sky = gd == BG
    assert sky.sum() > 1000 and (~sky).sum() > 100
    want, cov, tie, _ = ref.render(s, texels.view(np.uint16).reshape(-1, 4), ref.FMT_16F, 4, 3)
    assert cov.all() and tie.mean() < 0.02
    diff = np.abs(rgba[..., :3].astype(np.float64) - ref.expected_bytes(want))[sky & ~tie]
    assert diff.max() <= 1  # ... and its sky pixels are the reference's sky
    assert tensor is not None and np.array_equal(tensor.view(np.uint32), tensor_ref.tensor_from_rgba(rgba).view(np.uint32))
