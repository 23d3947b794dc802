"""Writes the skybox loader fixtures under tests/golden/sky/ (run from anywhere: python tests/golden/make_sky_fixture.py).

The project's own data, written by the small KTX 1 and OpenEXR writers below (no library): 4 x 4 EXR faces in every
compression the reader accepts and in both pixel types, and KTX cubemaps of 6 x 6 or smaller in the three formats, with
and without a mip chain. tests/test_sky_formats.py imports this module for the values each file holds.
"""
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sky")
FACES = ("px", "nx", "py", "ny", "pz", "nz")

GL_UNSIGNED_BYTE, GL_HALF_FLOAT, GL_FLOAT = 0x1401, 0x140B, 0x1406
GL_RGBA, GL_RGBA8, GL_SRGB8_ALPHA8, GL_RGBA16F = 0x1908, 0x8058, 0x8C43, 0x881A
KTX_ID = bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A])


# ---- values ------------------------------------------------------------------------------------------------------------
def face_values(face, n=4):
    """float32 [n, n, 4] RGBA of EXR face `face`: exact halves, some above 1, distinct per face, row and column."""
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    r = 0.25 * face + 0.125 * x + 0.5 * y
    g = 1.5 - 0.0625 * x * (face + 1)
    b = 0.03125 * (x + n * y) + 2.0 * (face % 2)
    a = 0.5 + 0.03125 * x
    return np.stack([r, g, b, a], -1).astype(np.float32)


def float_face_values(face, n=4):
    """float32 values that are no halves: the reader's float-to-half rounding shows (1 + 2^-11 is a tie)."""
    v = face_values(face, n) * np.float32(1.0 + 2.0 ** -11) + np.float32(3.0e-5)
    v[0, 0, 0] = np.float32(1.0 + 2.0 ** -11)
    return v.astype(np.float32)


def ktx_levels(fmt, n, mips, seed):
    """The texels of every level, [6, e, e, 4]: uint8 for the 8-bit formats, float16 for 'f16'."""
    rng = np.random.default_rng(seed)
    out = []
    for l in range(mips):
        e = max(1, n >> l)
        if fmt == "f16":
            out.append((rng.integers(0, 64, size=(6, e, e, 4)) / 16.0).astype(np.float16))
        else:
            out.append(rng.integers(0, 256, size=(6, e, e, 4), dtype=np.uint8))
    return out


# ---- KTX 1 ---------------------------------------------------------------------------------------------------------------
def ktx_bytes(levels, gl_type, gl_format, gl_internal, key_values=b"", faces=6, width=None, height=None, level_field=None):
    n = levels[0].shape[1]
    type_size = {GL_UNSIGNED_BYTE: 1, GL_HALF_FLOAT: 2, GL_FLOAT: 4}[gl_type]
    head = KTX_ID + struct.pack("<13I", 0x04030201, gl_type, type_size, gl_format, gl_internal, GL_RGBA,
                                n if width is None else width, n if height is None else height, 0, 0, faces,
                                len(levels) if level_field is None else level_field, len(key_values))
    body = b""
    for lv in levels:
        face_bytes = [np.ascontiguousarray(lv[f]).tobytes() for f in range(lv.shape[0])]
        body += struct.pack("<I", len(face_bytes[0]))  # cubemaps: the size of one face
        for fb in face_bytes:
            body += fb + b"\0" * (-len(fb) % 4)
        body += b"\0" * (-len(body) % 4)
    return head + key_values + body


def key_value(key, value):
    kv = key + b"\0" + value + b"\0"
    return struct.pack("<I", len(kv)) + kv + b"\0" * (-len(kv) % 4)


KTX_FILES = {  # name: (format, size, levels, seed, glType, glFormat, glInternalFormat, key/value data)
    "srgb8_n4.ktx": ("u8", 4, 1, 1, GL_UNSIGNED_BYTE, GL_RGBA, GL_SRGB8_ALPHA8, key_value(b"KTXorientation", b"S=r,T=d")),
    "unorm8_n6_chain.ktx": ("u8", 6, 3, 2, GL_UNSIGNED_BYTE, GL_RGBA, GL_RGBA8, b""),
    "unorm8_n2.ktx": ("u8", 2, 1, 3, GL_UNSIGNED_BYTE, GL_RGBA, GL_RGBA8, b""),
    "rgba16f_n4_chain.ktx": ("f16", 4, 3, 4, GL_HALF_FLOAT, GL_RGBA, GL_RGBA16F, b""),
    "rgba16f_n2.ktx": ("f16", 2, 1, 5, GL_HALF_FLOAT, GL_RGBA, GL_RGBA16F, b""),
    "rgba16f_float_typed_n2.ktx": ("f16", 2, 1, 6, GL_FLOAT, GL_RGBA, GL_RGBA16F, b""),
}


def ktx_file(name):
    fmt, n, mips, seed, gl_type, gl_format, gl_internal, kv = KTX_FILES[name]
    levels = ktx_levels(fmt, n, mips, seed)
    return ktx_bytes(levels, gl_type, gl_format, gl_internal, kv), levels


# ---- OpenEXR (single-part scanline files) --------------------------------------------------------------------------------
EXR_NONE, EXR_RLE, EXR_ZIPS, EXR_ZIP, EXR_PIZ = 0, 1, 2, 3, 4


def _attr(name, type_name, data):
    return name.encode() + b"\0" + type_name.encode() + b"\0" + struct.pack("<i", len(data)) + data


def _filter(raw):
    """The RLE / ZIP codecs' byte interleave (even bytes, then odd bytes) and predictor."""
    b = np.frombuffer(raw, np.uint8)
    t = np.concatenate([b[0::2], b[1::2]]).astype(np.int32)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128 + 256) & 0xFF
    return d.astype(np.uint8).tobytes()


def _rle(data):
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        run = 1
        while i + run < n and data[i + run] == data[i] and run < 128:
            run += 1
        if run >= 3:
            out += struct.pack("b", run - 1) + data[i:i + 1]
            i += run
            continue
        j = i
        while j < n and j - i < 127 and not (j + 2 < n and data[j] == data[j + 1] == data[j + 2]):
            j += 1
        out += struct.pack("b", -(j - i)) + data[i:j]
        i = j
    return bytes(out)


def exr_bytes(channels, compression, line_order=0, origin=(0, 0), version=2, tiled=False):
    """channels: {name: (array [h, w], 'half' | 'float' | 'uint')}; rows of the arrays run top to bottom."""
    names = sorted(channels)
    h, w = channels[names[0]][0].shape
    chlist = b""
    for nm in names:
        chlist += nm.encode() + b"\0" + struct.pack("<iB3xii", {"uint": 0, "half": 1, "float": 2}[channels[nm][1]], 0, 1, 1)
    chlist += b"\0"
    x0, y0 = origin
    box = struct.pack("<4i", x0, y0, x0 + w - 1, y0 + h - 1)
    header = struct.pack("<II", 20000630, version | (0x200 if tiled else 0))
    header += _attr("channels", "chlist", chlist) + _attr("compression", "compression", bytes([compression]))
    header += _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box)
    header += _attr("lineOrder", "lineOrder", bytes([line_order])) + _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    header += _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
    header += _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    per = 16 if compression == EXR_ZIP else 32 if compression == EXR_PIZ else 1
    blocks = []
    for first in range(0, h, per):
        raw = b""
        for y in range(first, min(first + per, h)):
            for nm in names:
                arr, kind = channels[nm]
                raw += arr[y].astype({"half": np.float16, "float": np.float32, "uint": np.uint32}[kind]).tobytes()
        packed = raw
        if compression in (EXR_RLE, EXR_ZIPS, EXR_ZIP):
            f = _filter(raw)
            c = _rle(f) if compression == EXR_RLE else zlib.compress(f, 9)
            packed = c if len(c) < len(raw) else raw
        blocks.append((y0 + first, packed))
    order = blocks if line_order == 0 else blocks[::-1]
    table_at = len(header)
    at = table_at + 8 * len(blocks)
    offsets, body = {}, b""
    for y, packed in order:
        offsets[y] = at + len(body)
        body += struct.pack("<ii", y, len(packed)) + packed
    table = b"".join(struct.pack("<Q", offsets[y]) for y, _ in blocks)  # the table is always in increasing y
    return header + table + body


def rgba_channels(v, kind, names="RGBA"):
    return {nm: (v[..., "RGBA".index(nm)], kind) for nm in names}


def exr_files():
    """name -> (bytes, expected float32 [4, 4, 4] RGBA before the half conversion, or None for a file to refuse)."""
    out = {}
    for f, tok in enumerate(FACES):  # a whole cubemap: ZIP, HALF
        out[f"zip_half_{tok}.exr"] = (exr_bytes(rgba_channels(face_values(f), "half"), EXR_ZIP), face_values(f))
    singles = [("none_half", EXR_NONE, "half"), ("rle_half", EXR_RLE, "half"), ("zips_half", EXR_ZIPS, "half"),
               ("none_float", EXR_NONE, "float"), ("rle_float", EXR_RLE, "float"), ("zips_float", EXR_ZIPS, "float"),
               ("zip_float", EXR_ZIP, "float")]
    for k, (name, comp, kind) in enumerate(singles):
        v = face_values(k) if kind == "half" else float_face_values(k)
        out[name + ".exr"] = (exr_bytes(rgba_channels(v, kind), comp), v)
    v = face_values(2)
    out["zips_half_decreasing_y.exr"] = (exr_bytes(rgba_channels(v, "half"), EXR_ZIPS, line_order=1, origin=(3, -2)), v)
    bgr = face_values(3).copy()
    bgr[..., 3] = 1.0  # missing alpha reads as 1
    out["zip_half_bgr.exr"] = (exr_bytes(rgba_channels(face_values(3), "half", "BGR"), EXR_ZIP), bgr)
    out["refused_two_channels.exr"] = (exr_bytes(rgba_channels(face_values(0), "half", "RG"), EXR_ZIP), None)
    out["refused_piz.exr"] = (exr_bytes(rgba_channels(face_values(0), "half"), EXR_PIZ), None)
    out["refused_uint.exr"] = (exr_bytes(rgba_channels(face_values(0), "uint"), EXR_NONE), None)
    out["refused_tiled.exr"] = (exr_bytes(rgba_channels(face_values(0), "half"), EXR_NONE, tiled=True), None)
    out["zip_half_2x2.exr"] = (exr_bytes(rgba_channels(face_values(0, 2), "half"), EXR_ZIP), face_values(0, 2))
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in KTX_FILES:
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(ktx_file(name)[0])
    for name, (data, _) in exr_files().items():
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
    print("wrote", len(KTX_FILES) + len(exr_files()), "files to", OUT)


if __name__ == "__main__":
    main()
