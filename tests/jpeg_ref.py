"""The numpy restatement of csrc/jpeg_math.h as an encoder: B8G8R8A8 pixels -> the bytes of a baseline JPEG (SOF0,
Y 2 x 2, Cb Cr 1 x 1, restart intervals). Integer arithmetic throughout, as the header's, so the device, the host
and this file produce the same bytes. Written from the header's comment, with the tables of T.81 Annex K.

encode(..., stats={}) also reports what the stream contains (DC categories, AC symbols, stuffed bytes, intervals, the
RSTn markers in order), so a
test can assert that its image reaches the case it is about; sabotage= breaks one step on purpose, for the tests
that must notice it."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
          54, 47, 55, 62, 63]
LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
          14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
          49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMA_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
            47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
    0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1,
    0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
    0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
    0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]

K = [4096, 4017, 3784, 3406, 2896, 2276, 1567, 799, 0]  # round(4096 cos(k pi / 16))
MAX_BLOCK_BITS = 22 + 63 * 26
HEADER_BYTES = 629
DEFAULT_QUALITY = 90
DEFAULT_RESTART_MCUS = 10


def dct_matrix():
    c = np.zeros((8, 8), np.int64)
    for u in range(8):
        for x in range(8):
            if u == 0:
                c[u, x] = K[4]
                continue
            m = ((2 * x + 1) * u) & 31
            if m > 16:
                m = 32 - m
            c[u, x] = -K[16 - m] if m > 8 else K[m]
    return c


def scaled_tables(quality):
    """(luma, chroma) quantisers in natural order: the IJG rule."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((np.array(t, np.int64) * s + 50) // 100, 1, 255) for t in (LUMA_Q, CHROMA_Q))


def huffman(bits, vals):
    """symbol -> (code, length), canonical (T.81 Annex C)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def restart_of(restart_mcus):
    return restart_mcus if restart_mcus else DEFAULT_RESTART_MCUS


def interval_bound(mcus):
    return 2 * ((mcus * 6 * MAX_BLOCK_BITS + 7) // 8)


def max_bytes(width, height, restart_mcus=0):
    mcus = ((width + 15) // 16) * ((height + 15) // 16)
    r = restart_of(restart_mcus)
    intervals = (mcus + r - 1) // r
    return HEADER_BYTES + (intervals - 1) * (interval_bound(r) + 2) + interval_bound(mcus - (intervals - 1) * r) + 2


def header(width, height, quality=DEFAULT_QUALITY, restart_mcus=0):
    ql, qc = scaled_tables(quality)
    o = bytearray(b"\xFF\xD8\xFF\xE0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for k, q in enumerate((ql, qc)):
        o += b"\xFF\xDB\x00\x43" + bytes([k]) + bytes(int(q[ZIGZAG[i]]) for i in range(64))
    o += b"\xFF\xC0\x00\x11\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    for ident, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x01, DC_CHROMA_BITS, DC_VALS),
                              (0x10, AC_LUMA_BITS, AC_LUMA_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        o += b"\xFF\xC4" + (19 + len(vals)).to_bytes(2, "big") + bytes([ident]) + bytes(bits) + bytes(vals)
    o += b"\xFF\xDD\x00\x04" + restart_of(restart_mcus).to_bytes(2, "big")
    o += b"\xFF\xDA\x00\x0C\x03\x01\x00\x02\x11\x03\x11\x00\x3F\x00"
    assert len(o) == HEADER_BYTES
    return bytes(o)


def coefficients(bgra, quality=DEFAULT_QUALITY, sabotage=None):
    """bgra uint8 [h, w, 4] -> int64 [mcus, 6, 64]: the quantised coefficients, MCUs in raster order, zig-zag order."""
    h, w = bgra.shape[:2]
    my, mx = (h + 15) // 16, (w + 15) // 16
    ys = np.minimum(np.arange(my * 16), h - 1)
    xs = np.minimum(np.arange(mx * 16), w - 1)
    p = bgra[ys][:, xs].astype(np.int64)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    assert min(y.min(), cb.min(), cr.min()) >= 0 and max(y.max(), cb.max(), cr.max()) <= 255
    mean = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2  # noqa: E731
    shift = 0 if sabotage == "no_level_shift" else 128
    yb = (y - shift).reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my * mx, 4, 8, 8)
    cbb = (mean(cb) - shift).reshape(my, 8, mx, 8).transpose(0, 2, 1, 3).reshape(my * mx, 1, 8, 8)
    crb = (mean(cr) - shift).reshape(my, 8, mx, 8).transpose(0, 2, 1, 3).reshape(my * mx, 1, 8, 8)
    s = np.concatenate([yb, cbb, crb], axis=1)  # [mcu, block, y, x]
    c = dct_matrix()
    a = np.einsum("ux,nbyx->nbyu", c, s)
    rows = (a + 512) >> 10
    coef = np.einsum("vy,nbyu->nbvu", c, rows)  # times 2^16
    if sabotage == "transposed_dct":
        coef = coef.transpose(0, 1, 3, 2)
    ql, qc = scaled_tables(quality)
    if sabotage == "chroma_tables_on_luma":
        ql = qc
    q = np.stack([ql] * 4 + [qc] * 2).reshape(1, 6, 8, 8)
    raw = ((np.abs(coef) + (q << 15)) // (q << 16) * np.sign(coef)).reshape(my * mx, 6, 64)  # half away from zero
    n = np.clip(raw, -1023, 1023)
    n[..., 0] = np.clip(raw[..., 0], -1024, 1023)
    return n[..., ZIGZAG]


def _value_bits(v, cat):
    return v + (1 << cat) - 1 if v < 0 else v


def encode(bgra, quality=DEFAULT_QUALITY, restart_mcus=0, stats=None, sabotage=None):
    """The complete stream, SOI to EOI."""
    h, w = bgra.shape[:2]
    coef = coefficients(np.asarray(bgra), quality, sabotage)
    tables = [huffman(DC_LUMA_BITS, DC_VALS), huffman(DC_CHROMA_BITS, DC_VALS), huffman(AC_LUMA_BITS, AC_LUMA_VALS),
              huffman(AC_CHROMA_BITS, AC_CHROMA_VALS)]
    restart = restart_of(restart_mcus)
    mcus = coef.shape[0]
    intervals = (mcus + restart - 1) // restart
    st = {"dc_categories": set(), "ac_symbols": {}, "stuffed": 0, "intervals": intervals, "rst_markers": [], "blocks_without_eob": 0,
          "dc_only_blocks": 0, "blocks": mcus * 6, "max_block_bits": 0}
    out = bytearray(header(w, h, quality, restart_mcus))
    for k in range(intervals):
        acc, nbits = 0, 0
        pred = [0, 0, 0]
        for m in range(k * restart, min((k + 1) * restart, mcus)):
            for b in range(6):
                comp = 0 if b < 4 else b - 3
                dc_t, ac_t = tables[1 if comp else 0], tables[3 if comp else 2]
                zz = [int(v) for v in coef[m, b]]
                start = nbits
                diff = zz[0] - pred[comp]
                pred[comp] = zz[0]
                cat = abs(diff).bit_length()
                st["dc_categories"].add(cat)
                code, length = dc_t[cat]
                acc = (acc << (length + cat)) | (code << cat) | _value_bits(diff, cat)
                nbits += length + cat
                run = 0
                for i in range(1, 64):
                    v = zz[i]
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        code, length = ac_t[0xF0]
                        acc = (acc << length) | code
                        nbits += length
                        st["ac_symbols"][0xF0] = st["ac_symbols"].get(0xF0, 0) + 1
                        run -= 16
                    cat = abs(v).bit_length()
                    sym = (run << 4) | cat
                    st["ac_symbols"][sym] = st["ac_symbols"].get(sym, 0) + 1
                    code, length = ac_t[sym]
                    acc = (acc << (length + cat)) | (code << cat) | _value_bits(v, cat)
                    nbits += length + cat
                    run = 0
                if run:
                    code, length = ac_t[0]
                    acc = (acc << length) | code
                    nbits += length
                    if run == 63:
                        st["dc_only_blocks"] += 1
                else:
                    st["blocks_without_eob"] += 1
                st["max_block_bits"] = max(st["max_block_bits"], nbits - start)
        pad = -nbits % 8
        acc = (acc << pad) | ((1 << pad) - 1)
        raw = acc.to_bytes((nbits + pad) // 8, "big")
        st["stuffed"] += raw.count(b"\xFF")
        out += raw.replace(b"\xFF", b"\xFF\x00")
        if k + 1 < intervals:
            out += bytes([0xFF, 0xD0 + (k & 7)])
            st["rst_markers"].append(0xD0 + (k & 7))
    out += b"\xFF\xD9"
    if stats is not None:
        stats.update(st)
    assert len(out) <= max_bytes(w, h, restart_mcus)
    return bytes(out)


# ---- the test images (B8G8R8A8, uint8 [h, w, 4]) -----------------------------------------------------------------

def noise(width, height, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (height, width, 4), dtype=np.uint8)


def checker(width, height):
    """8 x 8 blocks of black and white: DC differences of category 11 at quality 100."""
    y, x = np.mgrid[0:height, 0:width]
    v = (((x >> 3) + (y >> 3)) & 1) * 255
    return np.repeat(v[..., None], 4, axis=2).astype(np.uint8)


def high_frequency(width, height):
    """Grey, only the (7, 7) frequency in every block: runs of more than 16 zeros before it (ZRL)."""
    y, x = np.mgrid[0:height, 0:width]
    v = 128 + 100 * np.cos((2 * (x & 7) + 1) * 7 * np.pi / 16) * np.cos((2 * (y & 7) + 1) * 7 * np.pi / 16)
    return np.repeat(np.rint(v)[..., None], 4, axis=2).astype(np.uint8)


def black(width, height):
    return np.zeros((height, width, 4), np.uint8)


def gradient(width, height, seed=3):
    """A smooth coloured image with a little noise: what a rendered frame looks like to the coder."""
    y, x = np.mgrid[0:height, 0:width]
    rng = np.random.default_rng(seed)
    img = np.stack([(x * 5 + y) % 256, (y * 7) % 256, (x * 3 + y * 2) % 256, np.full_like(x, 255)], axis=2)
    return np.clip(img + rng.integers(-6, 7, img.shape), 0, 255).astype(np.uint8)
