// TextRenderer.h — font loading, atlas baking and text layout for the viewport text overlay: the host half of the
// reference's Trident::TextRenderer (Trident/src/Renderer/TextRenderer.h), under its public names (LoadFontFile,
// BeginFrame, QueueText). The device half is the library's text pass (tri_set_text, include/tri_raster.h); this class
// produces its inputs: one A8 atlas and, per viewport and frame, the glyph quads of the queued strings.
//
// The reference bakes its atlas with a third-party TrueType library. This is an independent implementation with no
// external dependency (TextRenderer.cpp): the glyph table and metrics follow the arrangement the reference's packer
// documents (code points 32..127, 1024 x 1024 atlas, 1 texel of padding, 2 x 2 oversampling), the coverage values are
// this rasteriser's own — parity-unpinned against the reference, pinned by the properties the tests state.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "../../../../include/tri_raster.h"
#include "glm_subset.h"

namespace Trident {

class TextRenderer {
public:
    // One entry of the glyph table, in viewport pixels and normalised atlas coordinates: the quad of a glyph drawn
    // with the pen at p spans [p + m_Offset, p + m_Offset + m_Size] and samples [m_UVMin, m_UVMax]; the pen then
    // moves right by m_Advance (unrounded).
    struct Glyph {
        glm::vec2 m_Offset{0.0f}, m_Size{0.0f};
        glm::vec2 m_UVMin{0.0f}, m_UVMax{0.0f};
        float m_Advance = 0.0f;
    };

    static constexpr uint32_t s_AtlasSize = 1024;
    static constexpr uint32_t s_FirstCodepoint = 32;
    static constexpr uint32_t s_CodepointCount = 96;

    // Reads a TrueType file and bakes code points 32..127 at pixelHeight. False (with the previous font kept) when
    // the file is missing or malformed: every offset, count and recursion depth is bounds-checked.
    bool LoadFontFile(const std::string& path, float pixelHeight);
    bool LoadFontMemory(const uint8_t* data, size_t size, float pixelHeight);
    bool IsLoaded() const { return m_Loaded; }

    void BeginFrame();  // empties the queue
    // Ignored until a font is loaded, and for text that decodes to nothing.
    void QueueText(uint32_t viewportId, const glm::vec2& position, const glm::vec4& color, std::string_view text);
    // The quads of everything queued for the viewport id, one tri_text_quad per glyph, appended to `out` in
    // submission order. Text queued for other ids is left alone.
    void LayoutViewport(uint32_t viewportId, std::vector<tri_text_quad>& out) const;
    // One string, without the queue.
    void LayoutText(const glm::vec2& position, const glm::vec4& color, std::string_view text,
                    std::vector<tri_text_quad>& out) const;
    bool HasPendingText() const { return !m_Queue.empty(); }

    static std::u32string DecodeUtf8(std::string_view text);
    const Glyph& ResolveGlyph(char32_t codepoint) const;  // the '?' entry for code points outside the table

    const std::vector<uint8_t>& AtlasPixels() const { return m_Atlas; }  // s_AtlasSize^2 coverage bytes
    float GetLineAdvance() const { return m_LineAdvance; }
    float GetFontPixelHeight() const { return m_FontPixelHeight; }
    float GetScale() const { return m_Scale; }  // pixels per font unit
    // Bumped by every successful load (the device atlas is re-created when it changes).
    uint64_t GetFontVersion() const { return m_FontVersion; }

private:
    struct Queued {  // one QueueText call, decoded
        glm::vec2 origin;
        glm::vec4 color;
        std::u32string codepoints;
    };
    void Layout(const glm::vec2& origin, const glm::vec4& color, const std::u32string& codepoints,
                std::vector<tri_text_quad>& out) const;

    std::unordered_map<char32_t, Glyph> m_Glyphs;
    std::unordered_map<uint32_t, std::vector<Queued>> m_Queue;  // per viewport id, in submission order
    std::vector<uint8_t> m_Atlas;
    float m_FontPixelHeight = 32.0f;
    float m_LineAdvance = 32.0f;
    float m_Scale = 0.0f;
    uint64_t m_FontVersion = 0;
    bool m_Loaded = false;
};

}  // namespace Trident
