"""CPU checks of the skybox loaders behind tri_upload_skybox_ex (host/src/SkyboxLoader.cpp): the KTX 1
parser (SkyboxTextureLoader::LoadFromKtx, TextureLoader.cpp:417-563), the OpenEXR face reader that stands in for tinyexr
(LoadFromExrFaces, :565-736), the reference's float-to-half routine (:162-204) and the discovery order of
Renderer::CreateSkyboxCubemap (Renderer.cpp:3818-3927).

The fixtures under tests/golden/sky/ are written by tests/golden/make_sky_fixture.py, which this module imports for the
values each file holds; the committed files must be what the script writes. No test reads the reference tree.
"""
import os
import shutil
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_sky_fixture as fx  # noqa: E402

SKY = os.path.join(ROOT, "tests", "golden", "sky")
FMT_SRGB, FMT_UNORM, FMT_16F = 0, 1, 2


@pytest.fixture(scope="module")
def app():
    from trident_raster import app as a

    a.load_library()
    return a


def ref_float_to_half(values):
    """The reference's rule for finite values below the overflow: normal halves drop 13 mantissa bits and add one when
    the highest dropped bit is set; below 2^-14 the magnitude in units of 2^-24 rounds half up (zero below 2^-25)."""
    v = np.asarray(values, np.float32)
    bits = v.view(np.uint32).astype(np.int64)
    mag = bits & 0x7FFFFFFF
    normal = (mag >> 13) - (112 << 10) + ((mag >> 12) & 1)
    small = np.floor(np.abs(v.astype(np.float64)) * 2.0 ** 24 + 0.5).astype(np.int64)
    h = np.where(np.abs(v) < np.float32(2.0 ** -14), small, normal)
    return (((bits >> 16) & 0x8000) | h).astype(np.uint16)


def test_committed_fixtures_are_what_the_script_writes():
    for name in fx.KTX_FILES:
        assert open(os.path.join(SKY, name), "rb").read() == fx.ktx_file(name)[0], name
    for name, (data, _) in fx.exr_files().items():  # (the ZIP files' bytes depend on the zlib that wrote them: the decode
        committed = open(os.path.join(SKY, name), "rb").read()  # tests below compare their content with the script's values)
        assert 0 < len(committed) < 1024, name
        if "zip" not in name:
            assert committed == data, name


# ---- KTX -----------------------------------------------------------------------------------------------------------------
def chain_bytes(levels):
    return np.concatenate([np.ascontiguousarray(l).view(np.uint8).ravel() for l in levels])


@pytest.mark.parametrize("name,fmt,bpp,hdr", [("srgb8_n4.ktx", FMT_SRGB, 4, 0), ("unorm8_n2.ktx", FMT_UNORM, 4, 0),
                                              ("rgba16f_n2.ktx", FMT_16F, 8, 1), ("unorm8_n6_chain.ktx", FMT_UNORM, 4, 0),
                                              ("rgba16f_n4_chain.ktx", FMT_16F, 8, 1),
                                              ("rgba16f_float_typed_n2.ktx", FMT_16F, 8, 1)])
def test_ktx_formats_and_chains_parse(app, name, fmt, bpp, hdr):
    """The three formats, chains (6 -> 3 -> 1 and 4 -> 2 -> 1), key/value data skipped (srgb8_n4.ktx carries some), and
    the FLOAT-typed RGBA16F quirk: 8 bytes per texel."""
    _, n, mips = fx.KTX_FILES[name][:3]
    info, texels = app.load_skybox_ktx(os.path.join(SKY, name))
    assert info is not None
    assert (info["format"], info["size"], info["mip_count"], info["bytes_per_pixel"], info["is_hdr"]) == (fmt, n, mips, bpp, hdr)
    assert info["region_levels"] == mips
    assert np.array_equal(texels, chain_bytes(fx.ktx_file(name)[1]))
    if name == "unorm8_n6_chain.ktx":
        assert info["bytes"] == 6 * 4 * (36 + 9 + 1)


def ktx_variant(tmp_path, data):
    p = tmp_path / "case.ktx"
    p.write_bytes(data)
    return str(p)


def header_word(data, index, value):
    """The KTX with header word `index` (0 = endianness, after the 12-byte identifier) replaced."""
    at = 12 + 4 * index
    return data[:at] + struct.pack("<I", value) + data[at + 4:]


WORD = {"endianness": 0, "glType": 1, "glFormat": 3, "glInternalFormat": 4, "width": 6, "height": 7, "faces": 10, "levels": 11,
        "kv": 12}


def test_ktx_refusals(app, tmp_path):
    good, _ = fx.ktx_file("rgba16f_n4_chain.ktx")
    assert app.load_skybox_ktx(ktx_variant(tmp_path, good))[0] is not None
    kv_good, _ = fx.ktx_file("srgb8_n4.ktx")
    first_level = 64  # the first level's size word (no key/value data in `good`)
    cases = {
        "big-endian": header_word(good, WORD["endianness"], 0x01020304),
        "five faces": header_word(good, WORD["faces"], 5),
        "one face": header_word(good, WORD["faces"], 1),
        "zero width": header_word(good, WORD["width"], 0),
        "zero height": header_word(good, WORD["height"], 0),
        "not square": header_word(good, WORD["height"], 2),
        "too wide": header_word(header_word(good, WORD["width"], 16385), WORD["height"], 16385),
        "huge": header_word(header_word(good, WORD["width"], 0xFFFFFFFF), WORD["height"], 0xFFFFFFFF),
        "unsupported type": header_word(good, WORD["glType"], 0x1403),
        "unsupported internal format": header_word(header_word(good, WORD["glInternalFormat"], 0x8814), WORD["glFormat"], 0x1907),
        "too many levels": header_word(good, WORD["levels"], 4),
        "zero image size": good[:first_level] + struct.pack("<I", 0) + good[first_level + 4:],
        "key/value past the end": header_word(kv_good, WORD["kv"], 1 << 20),
        "header only": good[:64],
        "short header": good[:40],
        "empty": b"",
    }
    # every truncation point class: inside the size word, a face, the last face of a level, a later level
    for cut in (66, 64 + 4 + 100, 64 + 4 + 6 * 128 - 1, 64 + 4 + 6 * 128 + 2, len(good) - 1):
        cases[f"truncated at {cut}"] = good[:cut]
    for what, data in cases.items():
        assert app.load_skybox_ktx(ktx_variant(tmp_path, data))[0] is None, what
    # the level's size word is otherwise ignored: a lying one changes nothing
    lying = good[:first_level] + struct.pack("<I", 7) + good[first_level + 4:]
    info, texels = app.load_skybox_ktx(ktx_variant(tmp_path, lying))
    assert info is not None and np.array_equal(texels, chain_bytes(fx.ktx_file("rgba16f_n4_chain.ktx")[1]))


# ---- EXR -----------------------------------------------------------------------------------------------------------------
def exr_dir(tmp_path, files):
    """A directory whose six faces are copies of the named fixtures (or bytes)."""
    d = tmp_path / "faces"
    if d.exists():
        shutil.rmtree(str(d))
    d.mkdir()
    for tok, src in zip(fx.FACES, files):
        if isinstance(src, bytes):
            (d / (tok + ".exr")).write_bytes(src)
        else:
            shutil.copy(os.path.join(SKY, src), str(d / (tok + ".exr")))
    return str(d)


def decoded(app, tmp_path, files):
    info, texels = app.load_skybox_directory(exr_dir(tmp_path, files))
    if info is None:
        return None
    assert (info["format"], info["mip_count"], info["bytes_per_pixel"], info["is_hdr"], info["region_levels"]) == (FMT_16F, 1, 8, 1, 1)
    n = info["size"]
    return texels.view(np.uint16).reshape(6, n, n, 4)


@pytest.mark.parametrize("name", ["none_half", "rle_half", "zips_half", "zip_half_px", "none_float", "rle_float", "zips_float",
                                  "zip_float", "zips_half_decreasing_y", "zip_half_bgr"])
def test_exr_codecs_types_and_orders_decode(app, tmp_path, name):
    """Each compression in both pixel types, both line orders (the decreasing-y file also has a data window away from
    the origin), channel order B, G, R without alpha: rows top to bottom, alpha 1 where missing."""
    want = fx.exr_files()[name + ".exr"][1]
    got = decoded(app, tmp_path, [name + ".exr"] * 6)
    assert got is not None and got.shape == (6, 4, 4, 4)
    assert np.array_equal(got[0], ref_float_to_half(want))
    if "float" in name:  # the float files hold values that are no halves: the rounding is the reference's
        assert got[0, 0, 0, 0] == 0x3C01  # 1 + 2^-11 -> 1 + 2^-10 (to even it would be 1.0)
        assert not np.array_equal(got[0], want.astype(np.float16).view(np.uint16))
    else:
        assert np.array_equal(got[0].view(np.float16).astype(np.float32), want)
    assert np.array_equal(got[5], got[0])


def test_exr_cubemap_faces_in_order(app, tmp_path):
    got = decoded(app, tmp_path, [f"zip_half_{t}.exr" for t in fx.FACES])
    for f in range(6):
        assert np.array_equal(got[f].view(np.float16).astype(np.float32), fx.face_values(f)), f


def test_exr_refusals(app, tmp_path, capfd):
    ok = "zip_half_px.exr"
    for bad, word in (("refused_two_channels.exr", "fewer than three channels"), ("refused_piz.exr", "PIZ"),
                      ("refused_uint.exr", "UINT"), ("refused_tiled.exr", "tiled")):
        capfd.readouterr()
        assert decoded(app, tmp_path, [ok, ok, bad, ok, ok, ok]) is None, bad
        assert word in capfd.readouterr().err, bad  # refused by name
    capfd.readouterr()
    assert decoded(app, tmp_path, [ok, ok, ok, "zip_half_2x2.exr", ok, ok]) is None  # mixed sizes
    assert "same resolution" in capfd.readouterr().err
    good = open(os.path.join(SKY, "zips_half.exr"), "rb").read()
    for cut in (3, 20, 200, len(good) - 40, len(good) - 1):  # the header, the offset table, a chunk
        assert decoded(app, tmp_path, [good[:cut]] * 6) is None, cut
    multipart = good[:4] + struct.pack("<I", 2 | 0x1000) + good[8:]
    assert decoded(app, tmp_path, [multipart] * 6) is None


# ---- the half conversion ----------------------------------------------------------------------------------------------------
def test_float_to_half_known_answers(app):
    f = np.float32
    cases = [
        (f(1.0), 0x3C00), (f(-2.0), 0xC000), (f(0.0), 0x0000), (f(-0.0), 0x8000),
        (f(1.0 + 2.0 ** -11), 0x3C01),          # a tie rounds away from zero: 1 + 2^-10 (to even: 0x3C00)
        (f(1.0 + 3 * 2.0 ** -11), 0x3C02),      # and so does the tie above an odd mantissa
        (f(1.0 + 2.0 ** -12), 0x3C00),          # below the tie: down
        (f(65504.0), 0x7BFF),                   # the largest half
        (f(65520.0), 0x7C00),                   # its tie rounds up into infinity's encoding
        (f(65536.0), 0x7C00), (f(-2.0 ** 20), 0xFC00),  # overflow: infinity
        (f(1.0e10), 0x7C01), (f(-1.0e10), 0xFC01),      # ... and the routine's "keeps one mantissa bit" holds for every
                                                        # mantissa that is not zero, finite values included (kept)
        (f(np.inf), 0x7C00), (f(-np.inf), 0xFC00),
        (f(2.0 ** -14), 0x0400),                # the smallest normal
        (f(2.0 ** -14 - 2.0 ** -25), 0x0400),   # the subnormal boundary: the largest subnormal's tie carries into it
        (f(2.0 ** -15), 0x0200), (f(2.0 ** -24), 0x0001),  # subnormals by the same shift-and-add
        (f(2.0 ** -25), 0x0001),                # rebiased exponent -10: half the smallest subnormal, a tie, rounds up
        (f(1.5 * 2.0 ** -26), 0x0000),          # rebiased exponent -11: below the cut-off, a signed zero
        (f(-1.5 * 2.0 ** -26), 0x8000),
        (f(2.0 ** -26), 0x0000),
    ]
    got = app.float_to_half(np.array([c[0] for c in cases], np.float32))
    for (value, want), g in zip(cases, got):
        assert int(g) == want, (float(value), hex(int(g)), hex(want))
    nan = app.float_to_half(np.array([np.nan, -np.nan], np.float32))
    assert int(nan[0]) & 0x7FFF == 0x7C01 and int(nan[1]) & 0x7FFF == 0x7C01  # a NaN keeps one mantissa bit
    rng = np.random.default_rng(1)
    v = rng.uniform(-60000.0, 60000.0, 4096).astype(np.float32)
    v = v[np.abs(v) >= 2.0 ** -14]
    assert np.array_equal(app.float_to_half(v), ref_float_to_half(v))


# ---- discovery --------------------------------------------------------------------------------------------------------------
def png_faces(directory, value):
    from PIL import Image

    for k, tok in enumerate(fx.FACES):
        img = np.full((4, 4, 4), value + k, np.uint8)
        Image.fromarray(img, "RGBA").save(os.path.join(directory, tok + ".png"))


def test_discovery_order(app, tmp_path):
    root = tmp_path / "Assets" / "Skyboxes"
    root.mkdir(parents=True)
    assets = str(tmp_path / "Assets")
    png_faces(str(root), 10)  # loose PNG faces
    d = root / "Default"
    d.mkdir()
    png_faces(str(d), 100)
    for tok in fx.FACES:  # six .exr faces beside the .png faces: HDR wins per face
        shutil.copy(os.path.join(SKY, f"zip_half_{tok}.exr"), str(d / (tok + ".exr")))
    shutil.copy(os.path.join(SKY, "rgba16f_n4_chain.ktx"), str(root / "DefaultSkybox.ktx"))

    info, texels, src = app.load_default_skybox_ex(assets)  # a valid DefaultSkybox.ktx wins over both
    assert src == "DefaultSkybox.ktx"
    assert (info["format"], info["size"], info["mip_count"], info["is_hdr"]) == (FMT_16F, 4, 3, 1)
    assert np.array_equal(texels, chain_bytes(fx.ktx_file("rgba16f_n4_chain.ktx")[1]))

    (root / "DefaultSkybox.ktx").write_bytes(open(os.path.join(SKY, "rgba16f_n4_chain.ktx"), "rb").read()[:200])
    info, _, src = app.load_default_skybox_ex(assets)  # present but invalid: the search does not go on
    assert info is None and src == "DefaultSkybox.ktx"

    os.remove(str(root / "DefaultSkybox.ktx"))
    info, texels, src = app.load_default_skybox_ex(assets)  # Default/: the .exr faces
    assert src == "Default directory"
    assert (info["format"], info["size"], info["mip_count"], info["bytes_per_pixel"], info["is_hdr"]) == (FMT_16F, 4, 1, 8, 1)
    got = texels.view(np.float16).reshape(6, 4, 4, 4).astype(np.float32)
    assert np.array_equal(got, np.stack([fx.face_values(f) for f in range(6)]))

    os.remove(str(d / "nz.exr"))  # five .exr faces and one .png: the LDR loader, where an .exr fails to decode
    info, _, src = app.load_default_skybox_ex(assets)
    assert info is None and src == "Default directory"

    for tok in fx.FACES[:5]:
        os.remove(str(d / (tok + ".exr")))
    info, texels, src = app.load_default_skybox_ex(assets)  # PNG faces alone in Default/
    assert src == "Default directory" and (info["format"], info["size"], info["is_hdr"]) == (FMT_SRGB, 4, 0)
    assert texels.reshape(6, 4, 4, 4)[3, 0, 0, 0] == 103

    shutil.rmtree(str(d))
    info, texels, src = app.load_default_skybox_ex(assets)
    assert src == "PNG fallback" and texels.reshape(6, 4, 4, 4)[2, 0, 0, 0] == 12
    faces, src2 = app.load_default_skybox(assets)  # the one-level LDR entry point sees the same
    assert src2 == src and np.array_equal(faces.ravel(), texels)
