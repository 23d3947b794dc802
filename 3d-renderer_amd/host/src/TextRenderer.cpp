// TextRenderer.cpp — a TrueType reader, an exact-area glyph rasteriser, the atlas packer and the text layout behind
// Trident::TextRenderer (host only, no external dependency).
//
// Reader: the sfnt table directory, head, maxp, hhea, hmtx, loca (both formats), glyf (simple glyphs; composites with
// offsets and the optional scale / 2x2 transform, to a fixed recursion depth) and cmap (format 4 and 12). Every read
// goes through Bytes::u8 / u16 / u32, which fail the whole load when an offset leaves the file.
//
// Baking (the arrangement the reference's packer documents): with s = pixelHeight / (ascent - descent) and S = 2s
// (2 x 2 oversampling), a glyph's box is ix0 = floor(xmin S), iy0 = floor(-ymax S), ix1 = ceil(xmax S),
// iy1 = ceil(-ymin S); its outline — quadratics flattened to 0.01 texel — is rendered into (ix1 - ix0) x (iy1 - iy0)
// texels with exact area coverage (signed areas accumulated per texel and summed along the row; overlapping contours
// saturate at full coverage, as a non-zero fill paints them), then the (ix1 - ix0 + 1) x (iy1 - iy0 + 1) atlas box is
// filtered with a truncating 2-tap running mean along rows, then along columns. Boxes sit on shelves with one texel
// between them.
#include "trident/TextRenderer.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

namespace Trident {

namespace {

// Big-endian reads that never leave the buffer: the first read outside it clears `ok`, and every later read gives 0.
struct Bytes {
    const uint8_t* data = nullptr;
    size_t size = 0;
    bool ok = true;

    bool has(size_t offset, size_t count) {
        if (offset > size || count > size - offset) ok = false;
        return ok;
    }
    uint32_t u8(size_t o) { return has(o, 1) ? data[o] : 0u; }
    uint32_t u16(size_t o) { return has(o, 2) ? (uint32_t)((data[o] << 8) | data[o + 1]) : 0u; }
    int32_t i16(size_t o) { return (int16_t)u16(o); }
    uint32_t u32(size_t o) {
        if (!has(o, 4)) return 0u;
        return ((uint32_t)data[o] << 24) | ((uint32_t)data[o + 1] << 16) | ((uint32_t)data[o + 2] << 8) | data[o + 3];
    }
};

struct Span {
    size_t offset = 0, length = 0;
};

struct Pt {
    double x = 0, y = 0;
};
using Ring = std::vector<Pt>;  // one closed polyline in font units (y up)

constexpr int kMaxCompositeDepth = 8;
constexpr size_t kOutlineBudget = 1u << 16;  // points plus glyph visits of one outline

struct TrueType {
    Bytes in;
    Span head, maxp, hhea, hmtx, loca, glyf, cmap;
    uint32_t glyphCount = 0, hMetricCount = 0;
    bool longLoca = false;
    int32_t ascent = 0, descent = 0, lineGap = 0;
    size_t cmapTable = 0;  // the chosen cmap subtable (absolute offset)
    uint32_t cmapFormat = 0;
    double chordTolerance = 1.0;  // quadratic flattening tolerance in font units (set by the baker)

    bool Locate(const char* tag, Span& out) {
        const uint32_t tables = in.u16(4);
        for (uint32_t i = 0; i < tables && in.ok; ++i) {
            const size_t rec = 12 + 16 * (size_t)i;
            if (!in.has(rec, 16)) return false;
            if (std::memcmp(in.data + rec, tag, 4) != 0) continue;
            out.offset = in.u32(rec + 8);
            out.length = in.u32(rec + 12);
            return in.has(out.offset, out.length);
        }
        return false;
    }

    bool Open(const uint8_t* bytes, size_t count) {
        in.data = bytes;
        in.size = count;
        const uint32_t version = in.u32(0);
        if (!in.ok || (version != 0x00010000u && version != 0x74727565u /* 'true' */)) return false;
        if (!Locate("head", head) || !Locate("maxp", maxp) || !Locate("hhea", hhea) || !Locate("hmtx", hmtx) ||
            !Locate("loca", loca) || !Locate("glyf", glyf) || !Locate("cmap", cmap))
            return false;
        if (head.length < 54 || maxp.length < 6 || hhea.length < 36) return false;
        const uint32_t locaFormat = in.u16(head.offset + 50);
        glyphCount = in.u16(maxp.offset + 4);
        ascent = in.i16(hhea.offset + 4);
        descent = in.i16(hhea.offset + 6);
        lineGap = in.i16(hhea.offset + 8);
        hMetricCount = in.u16(hhea.offset + 34);
        if (!in.ok || locaFormat > 1 || glyphCount == 0 || ascent - descent <= 0) return false;
        longLoca = locaFormat == 1;
        if (hMetricCount == 0 || hMetricCount > glyphCount || (size_t)hMetricCount * 4 > hmtx.length) return false;
        if (((size_t)glyphCount + 1) * (longLoca ? 4 : 2) > loca.length) return false;
        return ChooseCmap();
    }

    bool ChooseCmap() {
        if (cmap.length < 4) return false;
        const size_t tableEnd = cmap.offset + cmap.length;
        const uint32_t records = in.u16(cmap.offset + 2);
        int best = 0;  // 2: format 12 (the full repertoire), 1: format 4
        for (uint32_t i = 0; i < records; ++i) {
            const size_t rec = cmap.offset + 4 + 8 * (size_t)i;
            if (rec + 8 > tableEnd) return false;
            const uint32_t platform = in.u16(rec), encoding = in.u16(rec + 2), at = in.u32(rec + 4);
            if ((size_t)at + 4 > cmap.length) return false;
            const uint32_t format = in.u16(cmap.offset + at);
            const bool unicode = platform == 0 || (platform == 3 && (encoding == 1 || encoding == 10));
            const int rank = !unicode ? 0 : format == 12 ? 2 : format == 4 ? 1 : 0;
            if (rank > best) {
                best = rank;
                cmapTable = cmap.offset + at;
                cmapFormat = format;
            }
        }
        if (best == 0 || !in.ok) return false;
        // the subtable's own length stays inside the cmap table, and its arrays inside the subtable
        const size_t length = cmapFormat == 4 ? in.u16(cmapTable + 2) : in.u32(cmapTable + 4);
        if (!in.ok || length < 16 || cmapTable + length > tableEnd) return false;
        if (cmapFormat == 4) {
            const size_t segX2 = in.u16(cmapTable + 6);
            if ((segX2 & 1) || 16 + 4 * segX2 > length) return false;
        } else if (16 + 12 * (size_t)in.u32(cmapTable + 12) > length) {
            return false;
        }
        return in.ok;
    }

    // Code point -> glyph index; 0 (the missing glyph) when the cmap has no entry.
    uint32_t GlyphOf(uint32_t cp) {
        if (cmapFormat == 12) {
            const uint32_t groups = in.u32(cmapTable + 12);
            for (uint32_t g = 0; g < groups; ++g) {
                const size_t rec = cmapTable + 16 + 12 * (size_t)g;
                const uint32_t first = in.u32(rec), last = in.u32(rec + 4);
                if (cp < first || cp > last) continue;
                const uint64_t id = (uint64_t)in.u32(rec + 8) + (cp - first);
                return id < glyphCount ? (uint32_t)id : 0u;
            }
            return 0;
        }
        if (cp > 0xFFFF) return 0;
        const size_t length = in.u16(cmapTable + 2), segX2 = in.u16(cmapTable + 6);
        const size_t ends = cmapTable + 14, starts = ends + segX2 + 2, deltas = starts + segX2, ranges = deltas + segX2;
        for (size_t k = 0; k < segX2 / 2; ++k) {
            if (cp > in.u16(ends + 2 * k)) continue;
            const uint32_t first = in.u16(starts + 2 * k);
            if (cp < first) return 0;
            const uint32_t delta = in.u16(deltas + 2 * k), range = in.u16(ranges + 2 * k);
            uint32_t id;
            if (range == 0) {
                id = (cp + delta) & 0xFFFFu;
            } else {
                const size_t at = ranges + 2 * k + range + 2 * (size_t)(cp - first);
                if (at + 2 > cmapTable + length) return 0;
                id = in.u16(at);
                if (id != 0) id = (id + delta) & 0xFFFFu;
            }
            return id < glyphCount ? id : 0u;
        }
        return 0;
    }

    uint32_t AdvanceOf(uint32_t glyph) { return in.u16(hmtx.offset + 4 * (size_t)std::min(glyph, hMetricCount - 1)); }

    // The glyph's byte range inside the file; false when loca points outside glyf.
    bool GlyphBytes(uint32_t glyph, size_t& begin, size_t& end) {
        if (glyph >= glyphCount) return false;
        size_t a, b;
        if (longLoca) {
            a = in.u32(loca.offset + 4 * (size_t)glyph);
            b = in.u32(loca.offset + 4 * (size_t)glyph + 4);
        } else {
            a = 2 * (size_t)in.u16(loca.offset + 2 * (size_t)glyph);
            b = 2 * (size_t)in.u16(loca.offset + 2 * (size_t)glyph + 2);
        }
        if (!in.ok || a > b || b > glyf.length) return false;
        begin = glyf.offset + a;
        end = glyf.offset + b;
        return true;
    }

    // The glyph header's box in font units {xMin, yMin, xMax, yMax}; drawn = false for a glyph without an outline.
    bool HeaderBox(uint32_t glyph, bool& drawn, int32_t box[4]) {
        size_t begin, end;
        if (!GlyphBytes(glyph, begin, end)) return false;
        drawn = false;
        if (end == begin) return true;
        if (end - begin < 10) return false;
        for (int k = 0; k < 4; ++k) box[k] = in.i16(begin + 2 + 2 * (size_t)k);
        drawn = in.i16(begin) != 0;
        return in.ok;
    }

    // Appends the glyph's rings under the affine map (x, y) -> (m[0] x + m[2] y + m[4], m[1] x + m[3] y + m[5]).
    // `spent` counts points and glyph visits against kOutlineBudget (bounds nested composites too).
    bool Outline(uint32_t glyph, const double m[6], int depth, std::vector<Ring>& out, size_t& spent) {
        size_t begin, end;
        if (depth > kMaxCompositeDepth || ++spent > kOutlineBudget || !GlyphBytes(glyph, begin, end)) return false;
        if (end == begin) return true;  // no outline (space)
        if (end - begin < 10) return false;
        Bytes g = in;  // reads confined to this glyph's bytes
        g.size = end;
        const int32_t contours = g.i16(begin);
        size_t p = begin + 10;
        return contours >= 0 ? SimpleGlyph(g, p, contours, m, out, spent) : CompositeGlyph(g, p, m, depth, out, spent);
    }

    bool SimpleGlyph(Bytes& g, size_t p, int32_t contours, const double m[6], std::vector<Ring>& out, size_t& spent) {
        if (contours == 0) return g.ok;
        std::vector<uint32_t> lastPoint((size_t)contours);
        for (int32_t c = 0; c < contours; ++c, p += 2) {
            lastPoint[(size_t)c] = g.u16(p);
            if (c > 0 && lastPoint[(size_t)c] <= lastPoint[(size_t)c - 1]) return false;
        }
        const size_t count = (size_t)lastPoint.back() + 1;
        spent += count;
        if (!g.ok || spent > kOutlineBudget) return false;
        p += 2 + (size_t)g.u16(p);  // the instructions
        std::vector<uint8_t> flags(count);
        for (size_t i = 0; i < count && g.ok;) {
            const uint32_t f = g.u8(p++);
            flags[i++] = (uint8_t)f;
            if (f & 8)
                for (uint32_t repeat = g.u8(p++); repeat > 0 && i < count; --repeat) flags[i++] = (uint8_t)f;
        }
        if (!g.ok) return false;
        std::vector<Pt> pts(count);
        // x then y: a short (one byte, sign in the flag), a repeat of the previous value, or a signed word delta
        for (int axis = 0; axis < 2; ++axis) {
            const uint8_t isShort = axis ? 4 : 2, sameOrPositive = axis ? 32 : 16;
            int32_t value = 0;
            for (size_t i = 0; i < count; ++i) {
                const uint8_t f = flags[i];
                if (f & isShort) {
                    const int32_t d = (int32_t)g.u8(p++);
                    value += (f & sameOrPositive) ? d : -d;
                } else if (!(f & sameOrPositive)) {
                    value += g.i16(p);
                    p += 2;
                }
                (axis ? pts[i].y : pts[i].x) = value;
            }
        }
        if (!g.ok) return false;
        size_t first = 0;
        for (int32_t c = 0; c < contours; ++c) {
            AppendRing(pts, flags, first, lastPoint[(size_t)c], m, out);
            first = (size_t)lastPoint[(size_t)c] + 1;
        }
        return true;
    }

    bool CompositeGlyph(Bytes& g, size_t p, const double m[6], int depth, std::vector<Ring>& out, size_t& spent) {
        enum : uint32_t { kWords = 1, kOffsets = 2, kScale = 8, kMore = 0x20, kXYScale = 0x40, kMatrix = 0x80 };
        for (int parts = 0; parts < 256; ++parts) {
            const uint32_t flags = g.u16(p), child = g.u16(p + 2);
            p += 4;
            double dx, dy;
            if (flags & kWords) {
                dx = g.i16(p);
                dy = g.i16(p + 2);
                p += 4;
            } else {
                dx = (int8_t)g.u8(p);
                dy = (int8_t)g.u8(p + 1);
                p += 2;
            }
            if (!(flags & kOffsets)) return false;  // point-matched components are not supported
            double t[4] = {1.0, 0.0, 0.0, 1.0};
            auto f2dot14 = [&](size_t o) { return (double)g.i16(o) / 16384.0; };
            if (flags & kScale) {
                t[0] = t[3] = f2dot14(p);
                p += 2;
            } else if (flags & kXYScale) {
                t[0] = f2dot14(p);
                t[3] = f2dot14(p + 2);
                p += 4;
            } else if (flags & kMatrix) {
                for (int k = 0; k < 4; ++k) t[k] = f2dot14(p + 2 * (size_t)k);
                p += 8;
            }
            if (!g.ok) return false;
            // child point (x, y) -> parent (t0 x + t2 y + dx, t1 x + t3 y + dy), then the parent's map
            const double c[6] = {m[0] * t[0] + m[2] * t[1], m[1] * t[0] + m[3] * t[1],
                                 m[0] * t[2] + m[2] * t[3], m[1] * t[2] + m[3] * t[3],
                                 m[0] * dx + m[2] * dy + m[4], m[1] * dx + m[3] * dy + m[5]};
            if (!Outline(child, c, depth + 1, out, spent)) return false;
            if (!(flags & kMore)) return true;
        }
        return false;
    }

    // One TrueType contour (points first..last: on / off-curve, implied on-curve midpoints) as a flattened ring.
    void AppendRing(const std::vector<Pt>& pts, const std::vector<uint8_t>& flags, size_t first, size_t last,
                    const double m[6], std::vector<Ring>& out) const {
        const size_t n = last - first + 1;
        if (n < 2) return;
        auto onCurve = [&](size_t i) { return (flags[first + i % n] & 1) != 0; };
        auto at = [&](size_t i) {
            const Pt& q = pts[first + i % n];
            return Pt{m[0] * q.x + m[2] * q.y + m[4], m[1] * q.x + m[3] * q.y + m[5]};
        };
        auto mid = [](Pt a, Pt b) { return Pt{(a.x + b.x) * 0.5, (a.y + b.y) * 0.5}; };
        // start on an on-curve point: point 0, else the last point, else the midpoint between the two
        const size_t origin = onCurve(0) ? 0 : n - 1;
        const Pt start = onCurve(0) ? at(0) : onCurve(n - 1) ? at(n - 1) : mid(at(n - 1), at(0));
        Ring ring{start};
        Pt pen = start, control;
        bool pending = false;  // an off-curve point waits for the end of its curve
        auto curveTo = [&](Pt ctrl, Pt to) {
            // n chords stay within |p0 - 2 p1 + p2| / (4 n^2) of the curve
            const double bend = std::hypot(pen.x - 2.0 * ctrl.x + to.x, pen.y - 2.0 * ctrl.y + to.y);
            const int pieces = std::min(std::max((int)std::ceil(std::sqrt(bend / (4.0 * chordTolerance))), 1), 64);
            for (int i = 1; i <= pieces; ++i) {
                const double t = (double)i / pieces, u = 1.0 - t;
                ring.push_back(Pt{u * u * pen.x + 2.0 * u * t * ctrl.x + t * t * to.x,
                                  u * u * pen.y + 2.0 * u * t * ctrl.y + t * t * to.y});
            }
            pen = to;
        };
        for (size_t k = 1; k <= n; ++k) {
            const Pt q = at(origin + k);
            if (!onCurve(origin + k)) {
                if (pending) curveTo(control, mid(control, q));
                control = q;
                pending = true;
            } else if (pending) {
                curveTo(control, q);
                pending = false;
            } else {
                ring.push_back(q);
                pen = q;
            }
        }
        if (pending) curveTo(control, start);
        out.push_back(std::move(ring));
    }
};

// Exact area coverage of closed polylines (texel space, y down) over a w x h grid: every edge is cut where it crosses a
// texel boundary; a piece inside texel (i, j) with signed height dy and mean x offset fx adds dy (1 - fx) to the texel
// and dy fx to its right neighbour, and the running sum along the row is the signed covered area of each texel.
void Rasterise(const std::vector<Ring>& rings, int w, int h, std::vector<float>& cover) {
    const size_t stride = (size_t)w + 2;
    std::vector<double> acc(stride * (size_t)std::max(h, 1), 0.0);
    std::vector<double> cuts;
    // an outline of a malformed font may lie anywhere: edges with an end far outside the box are not drawn, which
    // also keeps every float -> int conversion below in range
    const double reach = 1.0e6;
    auto near = [&](const Pt& p) { return std::fabs(p.x) <= reach && std::fabs(p.y) <= reach; };
    for (const Ring& ring : rings) {
        for (size_t k = 0; k < ring.size(); ++k) {
            const Pt a = ring[k], b = ring[(k + 1) % ring.size()];
            if (a.y == b.y || !near(a) || !near(b)) continue;
            if (std::fabs(b.x - a.x) + std::fabs(b.y - a.y) > 65536.0) continue;  // (bounds the cuts of one edge)
            cuts.assign({0.0, 1.0});
            auto cutAtIntegers = [&](double p0, double p1) {
                if (p0 == p1) return;
                const double hi = std::max(p0, p1);
                for (double g = std::floor(std::min(p0, p1)) + 1.0; g < hi; g += 1.0) cuts.push_back((g - p0) / (p1 - p0));
            };
            cutAtIntegers(a.x, b.x);
            cutAtIntegers(a.y, b.y);
            std::sort(cuts.begin(), cuts.end());
            for (size_t t = 0; t + 1 < cuts.size(); ++t) {
                const double t0 = cuts[t], t1 = cuts[t + 1];
                if (t1 <= t0) continue;
                const double xm = a.x + (b.x - a.x) * 0.5 * (t0 + t1), ym = a.y + (b.y - a.y) * 0.5 * (t0 + t1);
                const double row = std::floor(ym);
                if (row < 0.0 || row >= (double)h) continue;  // outside the header box: not drawn
                // left of the box: full weight on texel 0; right of it: on the column past the last texel
                const double col = std::min(std::max(std::floor(xm), 0.0), (double)w);
                const double fx = (xm < 0.0 || xm >= (double)w) ? 0.0 : xm - col;
                const double dy = (b.y - a.y) * (t1 - t0);
                double* line = acc.data() + (size_t)row * stride;
                line[(size_t)col] += dy * (1.0 - fx);
                line[(size_t)col + 1] += dy * fx;
            }
        }
    }
    cover.assign((size_t)w * (size_t)h, 0.0f);
    for (int j = 0; j < h; ++j) {
        double sum = 0.0;
        for (int i = 0; i < w; ++i) {
            sum += acc[(size_t)j * stride + (size_t)i];
            cover[(size_t)j * (size_t)w + (size_t)i] = (float)std::min(std::fabs(sum), 1.0);
        }
    }
}

// The oversampling filter over a bw x bh box, in place: a truncating 2-tap running mean along rows, then columns.
void BoxFilter2(std::vector<uint8_t>& box, uint32_t bw, uint32_t bh) {
    auto pass = [&](uint32_t lines, uint32_t length, size_t lineStep, size_t step) {
        for (uint32_t l = 0; l < lines; ++l) {
            uint32_t before = 0;
            for (uint32_t i = 0; i < length; ++i) {
                uint8_t& texel = box[l * lineStep + i * step];
                const uint32_t here = texel;
                texel = (uint8_t)((before + here) / 2);
                before = here;
            }
        }
    };
    pass(bh, bw, bw, 1);
    pass(bw, bh, 1, bw);
}

}  // namespace

bool TextRenderer::LoadFontFile(const std::string& path, float pixelHeight) {
    std::ifstream file(path, std::ios::binary);
    if (!file) {
        std::fprintf(stderr, "[Trident] TextRenderer: could not open the font file %s\n", path.c_str());
        return false;
    }
    const std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
    if (bytes.empty() || !LoadFontMemory(bytes.data(), bytes.size(), pixelHeight)) {
        std::fprintf(stderr, "[Trident] TextRenderer: %s is not a TrueType file this reader accepts\n", path.c_str());
        return false;
    }
    return true;
}

bool TextRenderer::LoadFontMemory(const uint8_t* data, size_t size, float pixelHeight) {
    if (!data || size < 12 || !(pixelHeight > 0.0f) || !(pixelHeight <= 256.0f)) return false;
    TrueType font;
    if (!font.Open(data, size)) return false;
    const float scale = pixelHeight / (float)(font.ascent - font.descent);  // pixels per font unit
    const double S = 2.0 * (double)scale;                                  // 2 x 2 oversampling
    font.chordTolerance = 0.01 / S;                                        // 0.01 texel

    std::vector<uint8_t> atlas((size_t)s_AtlasSize * s_AtlasSize, 0);
    std::unordered_map<char32_t, Glyph> table;
    table.reserve(s_CodepointCount);
    uint32_t shelfX = 1, shelfY = 1, shelfHeight = 0;  // one texel of padding around every box
    std::vector<Ring> rings;
    std::vector<float> cover;
    std::vector<uint8_t> box;
    for (uint32_t cp = s_FirstCodepoint; cp < s_FirstCodepoint + s_CodepointCount; ++cp) {
        const uint32_t glyph = font.GlyphOf(cp);  // 0 when the cmap has no entry (127)
        bool drawn = false;
        int32_t units[4] = {0, 0, 0, 0};
        if (!font.HeaderBox(glyph, drawn, units)) return false;
        int ix0 = 0, iy0 = 0, ix1 = 0, iy1 = 0;
        rings.clear();
        if (drawn) {
            const double identity[6] = {1, 0, 0, 1, 0, 0};
            size_t spent = 0;
            if (!font.Outline(glyph, identity, 0, rings, spent)) return false;
            ix0 = (int)std::floor(units[0] * S);
            iy0 = (int)std::floor(-units[3] * S);
            ix1 = (int)std::ceil(units[2] * S);
            iy1 = (int)std::ceil(-units[1] * S);
            if (ix1 < ix0 || iy1 < iy0) return false;
        }
        const int w = ix1 - ix0, h = iy1 - iy0;
        const uint32_t bw = (uint32_t)w + 1, bh = (uint32_t)h + 1;  // the atlas box
        if (bw + 2 > s_AtlasSize) return false;
        if (shelfX + bw + 1 > s_AtlasSize) {  // next shelf
            shelfX = 1;
            shelfY += shelfHeight + 1;
            shelfHeight = 0;
        }
        if (shelfY + bh + 1 > s_AtlasSize) return false;  // the range does not fit the atlas at this size
        box.assign((size_t)bw * bh, 0);
        if (w > 0 && h > 0 && !rings.empty()) {
            for (Ring& ring : rings)
                for (Pt& p : ring) p = Pt{p.x * S - (double)ix0, -p.y * S - (double)iy0};
            Rasterise(rings, w, h, cover);
            for (int j = 0; j < h; ++j)
                for (int i = 0; i < w; ++i)
                    box[(size_t)j * bw + (size_t)i] = (uint8_t)(int)(cover[(size_t)j * (size_t)w + (size_t)i] * 255.0f + 0.5f);
            BoxFilter2(box, bw, bh);
        }
        for (uint32_t j = 0; j < bh; ++j)
            std::memcpy(&atlas[(size_t)(shelfY + j) * s_AtlasSize + shelfX], &box[(size_t)j * bw], bw);
        Glyph entry;
        entry.m_Offset = {(float)ix0 * 0.5f - 0.25f, (float)iy0 * 0.5f - 0.25f};
        entry.m_Size = {(float)bw * 0.5f, (float)bh * 0.5f};
        entry.m_UVMin = {(float)shelfX / (float)s_AtlasSize, (float)shelfY / (float)s_AtlasSize};
        entry.m_UVMax = {(float)(shelfX + bw) / (float)s_AtlasSize, (float)(shelfY + bh) / (float)s_AtlasSize};
        entry.m_Advance = scale * (float)font.AdvanceOf(glyph);
        table[(char32_t)cp] = entry;
        shelfX += bw + 1;
        shelfHeight = std::max(shelfHeight, bh);
        if (!font.in.ok) return false;
    }

    m_Glyphs = std::move(table);
    m_Atlas = std::move(atlas);
    m_FontPixelHeight = pixelHeight;
    m_Scale = scale;
    m_LineAdvance = (float)(font.ascent - font.descent + font.lineGap) * scale;
    m_Loaded = true;
    ++m_FontVersion;
    return true;
}

void TextRenderer::BeginFrame() { m_Queue.clear(); }

void TextRenderer::QueueText(uint32_t viewportId, const glm::vec2& position, const glm::vec4& color, std::string_view text) {
    if (!m_Loaded) return;
    std::u32string codepoints = DecodeUtf8(text);
    if (!codepoints.empty()) m_Queue[viewportId].push_back(Queued{position, color, std::move(codepoints)});
}

// The reference's vertex loop (TextRenderer.cpp:144-193) per glyph quad: the pen starts at the origin, a line feed
// returns it to the origin's x one line advance lower, every other code point emits its glyph's box at pen + offset
// with the glyph's UV box and moves the pen by the glyph's advance.
void TextRenderer::Layout(const glm::vec2& origin, const glm::vec4& color, const std::u32string& codepoints,
                          std::vector<tri_text_quad>& out) const {
    glm::vec2 pen = origin;
    for (const char32_t cp : codepoints) {
        if (cp == U'\n') {
            pen.x = origin.x;
            pen.y += m_LineAdvance;
            continue;
        }
        const Glyph& g = ResolveGlyph(cp);
        tri_text_quad q;
        q.x0 = pen.x + g.m_Offset.x;
        q.y0 = pen.y + g.m_Offset.y;
        q.x1 = q.x0 + g.m_Size.x;
        q.y1 = q.y0 + g.m_Size.y;
        q.u0 = g.m_UVMin.x;
        q.v0 = g.m_UVMin.y;
        q.u1 = g.m_UVMax.x;
        q.v1 = g.m_UVMax.y;
        for (int k = 0; k < 4; ++k) q.rgba[k] = color[k];
        out.push_back(q);
        pen.x += g.m_Advance;
    }
}

void TextRenderer::LayoutViewport(uint32_t viewportId, std::vector<tri_text_quad>& out) const {
    const auto queued = m_Queue.find(viewportId);
    if (!m_Loaded || queued == m_Queue.end()) return;
    for (const Queued& q : queued->second) Layout(q.origin, q.color, q.codepoints, out);
}

void TextRenderer::LayoutText(const glm::vec2& position, const glm::vec4& color, std::string_view text,
                              std::vector<tri_text_quad>& out) const {
    if (m_Loaded) Layout(position, color, DecodeUtf8(text), out);
}

// UTF-8 -> code points with the reference's handling of bad input (TextRenderer.cpp:981-1046), which the tests pin:
// a byte that cannot start a sequence is skipped; a multi-byte sequence that the end of the string cuts short ends
// the decoding; a sequence with a byte that is no continuation loses its lead byte only (decoding resumes at the next
// byte). Overlong forms and surrogates are not rejected, as there.
std::u32string TextRenderer::DecodeUtf8(std::string_view text) {
    std::u32string out;
    const size_t n = text.size();
    for (size_t i = 0; i < n;) {
        const uint8_t lead = (uint8_t)text[i];
        if (lead < 0x80) {
            out.push_back(lead);
            ++i;
            continue;
        }
        // 110xxxxx, 1110xxxx, 11110xxx: 1, 2, 3 continuation bytes
        const size_t tail = (lead >> 5) == 0x6 ? 1 : (lead >> 4) == 0xE ? 2 : (lead >> 3) == 0x1E ? 3 : 0;
        if (tail == 0) {
            ++i;
            continue;
        }
        if (i + tail >= n) break;
        char32_t cp = lead & (0x3Fu >> tail);
        size_t good = 0;
        while (good < tail && ((uint8_t)text[i + 1 + good] & 0xC0u) == 0x80u) {
            cp = (cp << 6) | ((uint8_t)text[i + 1 + good] & 0x3Fu);
            ++good;
        }
        if (good == tail) {
            out.push_back(cp);
            i += tail + 1;
        } else {
            ++i;
        }
    }
    return out;
}

const TextRenderer::Glyph& TextRenderer::ResolveGlyph(char32_t codepoint) const {
    static const Glyph kNoGlyph{};
    auto it = m_Glyphs.find(codepoint);
    if (it == m_Glyphs.end()) it = m_Glyphs.find(U'?');  // outside the baked range
    return it != m_Glyphs.end() ? it->second : kNoGlyph;
}

}  // namespace Trident
