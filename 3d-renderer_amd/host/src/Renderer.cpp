// Renderer.cpp — Trident::Renderer's draw path over the HIP rasterizer C-ABI.
//
// Mirrors the reference's CPU side of the hot path: primitive meshes (Renderer.cpp:72-246),
// ComposeTransform (:417-427), UploadMesh/AppendMeshes/UploadMeshFromCache (:1784-2116), texture
// slots (:3404-3804), GatherMeshDraws (:2910-2994), UpdateUniformBuffer (:5822-6051), the per-draw
// push-constant loop (:5110-5151), per-viewport camera routing (:4545-4574), readback (:1299-1389)
// and frame timing (:6286-6343). Vulkan command recording is replaced by tri_set_frame /
// tri_set_draws / tri_render on one tri_ctx per viewport.
#include "trident/Renderer.h"
#include "trident/Animation.h"
#include "trident/ModelLoader.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <limits>
#include <thread>

namespace Trident {

namespace {

constexpr const char* kDefaultTextureKey = "renderer://default-white";
constexpr size_t kInvalidMeshIndex = std::numeric_limits<size_t>::max();

void LogError(const char* what, const char* detail) { std::fprintf(stderr, "[Trident] %s: %s\n", what, detail); }

// The readers' byte order (QuerySwapchainFormatInfo): the device's BGRA as RGBA.
void BgraToRgba(const std::vector<uint8_t>& bgra, std::vector<uint8_t>& rgba) {
    rgba.resize(bgra.size());
    for (size_t i = 0; i < bgra.size(); i += 4) {
        rgba[i + 0] = bgra[i + 2];
        rgba[i + 1] = bgra[i + 1];
        rgba[i + 2] = bgra[i + 0];
        rgba[i + 3] = bgra[i + 3];
    }
}

// The objects of m_Reprojection, m_Taa or m_Upscale go with the targets: the new targets' first frames have no history.
template <typename Map, typename Destroy>
void DropObjects(Map& records, Destroy destroy) {
    for (auto& it : records) {
        destroy(it.second.m_Object);  // (waits for its last pass)
        it.second.m_Object = nullptr;
        it.second.m_LastTarget = nullptr;
        it.second.m_FrameIndex = 0;
    }
}

// A viewport's object for a target's extent (matches: the one there is was made for it): made at the first frame, and
// again, with no history, after a resize; create(device, &object).
template <typename Object, typename Destroy, typename Create>
bool EnsureObject(Object*& object, bool matches, tri_ctx* ctx, Destroy destroy, Create create, const char* what) {
    if (object && !matches) {
        destroy(object);
        object = nullptr;
    }
    if (object) return true;
    tri_image img{};
    if (tri_get_output(ctx, &img) != TRI_OK || create(img.device, &object) != TRI_OK) {
        LogError(what, tri_last_error());
        object = nullptr;
        return false;
    }
    return true;
}

std::string DefaultDatasetDirectory() {  // current_path()/DatasetCapture (Renderer.cpp:551, :2508-2511)
    std::error_code ec;
    const std::filesystem::path cwd = std::filesystem::current_path(ec);
    return ((ec ? std::filesystem::path(".") : cwd) / "DatasetCapture").string();
}

Geometry::Mesh BuildPrimitiveQuadMesh() {
    Geometry::Mesh mesh;
    Vertex v[4]{};
    v[0].Position = {-0.5f, -0.5f, 0.0f};
    v[1].Position = {0.5f, -0.5f, 0.0f};
    v[2].Position = {0.5f, 0.5f, 0.0f};
    v[3].Position = {-0.5f, 0.5f, 0.0f};
    for (Vertex& it : v) {
        it.Normal = {0.0f, 0.0f, 1.0f};
        it.Tangent = {1.0f, 0.0f, 0.0f};
        it.Bitangent = {0.0f, 1.0f, 0.0f};
        it.Color = {1.0f, 1.0f, 1.0f};
    }
    v[0].TexCoord = {0.0f, 0.0f};
    v[1].TexCoord = {1.0f, 0.0f};
    v[2].TexCoord = {1.0f, 1.0f};
    v[3].TexCoord = {0.0f, 1.0f};
    mesh.Vertices.assign(v, v + 4);
    mesh.Indices = {0, 1, 2, 0, 2, 3};  // counter clockwise with the projection Y flip
    return mesh;
}

// BuildSpriteGeometry (Renderer.cpp:2853-2890): a unit quad facing -Z with indices {0, 2, 1, 0, 3, 2}
// (the opposite winding of the quad primitive: a sprite seen from +Z is back-facing and culled, as in
// the reference, whose Default pipeline culls BACK for sprites too).
Geometry::Mesh BuildSpriteQuadMesh() {
    Geometry::Mesh mesh;
    Vertex v[4]{};
    v[0].Position = {-0.5f, -0.5f, 0.0f};
    v[1].Position = {0.5f, -0.5f, 0.0f};
    v[2].Position = {0.5f, 0.5f, 0.0f};
    v[3].Position = {-0.5f, 0.5f, 0.0f};
    for (Vertex& it : v) {
        it.Normal = {0.0f, 0.0f, -1.0f};
        it.Tangent = {1.0f, 0.0f, 0.0f};
        it.Bitangent = {0.0f, 1.0f, 0.0f};
        it.Color = {1.0f, 1.0f, 1.0f};
    }
    v[0].TexCoord = {0.0f, 0.0f};
    v[1].TexCoord = {1.0f, 0.0f};
    v[2].TexCoord = {1.0f, 1.0f};
    v[3].TexCoord = {0.0f, 1.0f};
    mesh.Vertices.assign(v, v + 4);
    mesh.Indices = {0, 2, 1, 0, 3, 2};
    return mesh;
}

Geometry::Mesh BuildPrimitiveCubeMesh() {
    struct Face {
        glm::vec3 n, t, b;
        glm::vec3 p[4];
    };
    const Face faces[6] = {
        {{0, 0, 1}, {1, 0, 0}, {0, 1, 0}, {{-0.5f, -0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.5f, 0.5f, 0.5f}, {-0.5f, 0.5f, 0.5f}}},
        {{0, 0, -1}, {-1, 0, 0}, {0, 1, 0}, {{0.5f, -0.5f, -0.5f}, {-0.5f, -0.5f, -0.5f}, {-0.5f, 0.5f, -0.5f}, {0.5f, 0.5f, -0.5f}}},
        {{1, 0, 0}, {0, 0, -1}, {0, 1, 0}, {{0.5f, -0.5f, 0.5f}, {0.5f, -0.5f, -0.5f}, {0.5f, 0.5f, -0.5f}, {0.5f, 0.5f, 0.5f}}},
        {{-1, 0, 0}, {0, 0, 1}, {0, 1, 0}, {{-0.5f, -0.5f, -0.5f}, {-0.5f, -0.5f, 0.5f}, {-0.5f, 0.5f, 0.5f}, {-0.5f, 0.5f, -0.5f}}},
        {{0, 1, 0}, {1, 0, 0}, {0, 0, -1}, {{-0.5f, 0.5f, 0.5f}, {0.5f, 0.5f, 0.5f}, {0.5f, 0.5f, -0.5f}, {-0.5f, 0.5f, -0.5f}}},
        {{0, -1, 0}, {1, 0, 0}, {0, 0, 1}, {{-0.5f, -0.5f, -0.5f}, {0.5f, -0.5f, -0.5f}, {0.5f, -0.5f, 0.5f}, {-0.5f, -0.5f, 0.5f}}},
    };
    const glm::vec2 uv[4] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
    Geometry::Mesh mesh;
    uint32_t off = 0;
    for (const Face& f : faces) {
        for (int k = 0; k < 4; ++k) {
            Vertex v{};
            v.Position = f.p[k];
            v.Normal = f.n;
            v.Tangent = f.t;
            v.Bitangent = f.b;
            v.Color = {1.0f, 1.0f, 1.0f};
            v.TexCoord = uv[k];
            mesh.Vertices.push_back(v);
        }
        for (uint32_t i : {0u, 2u, 1u, 0u, 3u, 2u}) mesh.Indices.push_back(off + i);  // CW from outside
        off += 4;
    }
    return mesh;
}

Geometry::Mesh BuildPrimitiveSphereMesh() {
    const uint32_t rings = 16, segments = 24;
    const float radius = 0.5f;
    Geometry::Mesh mesh;
    for (uint32_t r = 0; r <= rings; ++r) {
        const float V = (float)r / (float)rings;
        const float phi = V * glm::pi<float>();
        for (uint32_t s = 0; s <= segments; ++s) {
            const float U = (float)s / (float)segments;
            const float theta = U * glm::two_pi<float>();
            const float sp = std::sin(phi), cp = std::cos(phi), st = std::sin(theta), ct = std::cos(theta);
            const glm::vec3 p{radius * sp * ct, radius * cp, radius * sp * st};
            const glm::vec3 n = glm::normalize(p);
            glm::vec3 t{-st, 0.0f, ct};
            if (glm::length(t) < 0.0001f) t = {1.0f, 0.0f, 0.0f};
            t = glm::normalize(t);
            glm::vec3 b = glm::normalize(glm::cross(n, t));
            if (glm::length(b) < 0.0001f) b = {0.0f, 1.0f, 0.0f};
            Vertex v{};
            v.Position = p;
            v.Normal = n;
            v.Tangent = t;
            v.Bitangent = b;
            v.Color = {1.0f, 1.0f, 1.0f};
            v.TexCoord = {U, 1.0f - V};
            mesh.Vertices.push_back(v);
        }
    }
    const uint32_t row = segments + 1;
    for (uint32_t r = 0; r < rings; ++r)
        for (uint32_t s = 0; s < segments; ++s) {
            const uint32_t i0 = r * row + s, i1 = (r + 1) * row + s, i2 = (r + 1) * row + s + 1, i3 = r * row + s + 1;
            for (uint32_t i : {i0, i2, i1, i0, i3, i2}) mesh.Indices.push_back(i);
        }
    return mesh;
}

glm::mat4 ComposeTransform(const Transform& t) {  // T * Rx * Ry * Rz * S, degrees
    glm::mat4 m{1.0f};
    m = glm::translate(m, t.Position);
    m = glm::rotate(m, glm::radians(t.Rotation.x), glm::vec3{1.0f, 0.0f, 0.0f});
    m = glm::rotate(m, glm::radians(t.Rotation.y), glm::vec3{0.0f, 1.0f, 0.0f});
    m = glm::rotate(m, glm::radians(t.Rotation.z), glm::vec3{0.0f, 0.0f, 1.0f});
    return glm::scale(m, t.Scale);
}

std::string NormalizeTexturePath(const std::string& path) {
    std::string s = path;
    std::replace(s.begin(), s.end(), '\\', '/');
    return s;
}

void CopyMat(const glm::mat4& m, float* out) {
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) out[c * 4 + r] = m[c][r];
}

// A viewport's render target: one context, or a group of row bands on several devices (SetDeviceCount).
// Every per-context call of the draw path goes to the context or is broadcast to the group's bands.
struct Target {
    tri_ctx* c;
    tri_group* g;
    int Materials(const tri_material_record* r, uint32_t n) const {
        return g ? tri_group_upload_materials(g, r, n) : tri_upload_materials(c, r, n);
    }
    // (a one-level sRGB cubemap is tri_upload_skybox itself; desc = nullptr removes the skybox)
    int Skybox(const tri_skybox_desc* d) const {
        if (!d) return g ? tri_group_upload_skybox(g, nullptr, 0) : tri_upload_skybox(c, nullptr, 0);
        return g ? tri_group_upload_skybox_ex(g, d) : tri_upload_skybox_ex(c, d);
    }
    int AiFrame(const uint8_t* p, uint32_t w, uint32_t h) const {
        return g ? tri_group_upload_ai_frame(g, p, w, h) : tri_upload_ai_frame(c, p, w, h);
    }
    int Texture(uint32_t slot, const uint8_t* p, uint32_t w, uint32_t h) const {
        return g ? tri_group_upload_texture(g, slot, p, w, h) : tri_upload_texture(c, slot, p, w, h);
    }
    int Shadow(const tri_shadow_config* s) const { return g ? tri_group_set_shadow(g, s) : tri_set_shadow(c, s); }
    int Bones(const float* m, uint32_t n) const {
        return g ? tri_group_upload_bone_palette(g, m, n) : tri_upload_bone_palette(c, m, n);
    }
    int Pose(tri_animset* const* sets, const tri_pose_instance* i, uint32_t n) const {
        return g ? tri_group_pose_palette(g, sets, i, n) : tri_pose_palette(c, n ? sets[0] : nullptr, i, n);
    }
    int PoseGraph(tri_animset* const* sets, const tri_pose_graph_instance* i, uint32_t n, const tri_pose_op* ops, uint32_t nops) const {
        return g ? tri_group_pose_graph(g, sets, i, n, ops, nops) : tri_pose_graph(c, n ? sets[0] : nullptr, i, n, ops, nops);
    }
    int Frame(const tri_global_ubo* u, const float* clear) const {
        return g ? tri_group_set_frame(g, u, clear) : tri_set_frame(c, u, clear);
    }
    int Draws(const tri_draw* d, uint32_t n) const { return g ? tri_group_set_draws(g, d, n) : tri_set_draws(c, d, n); }
    int Render() const { return g ? tri_group_render(g) : tri_render(c); }
    int Sync() const { return g ? tri_group_synchronize(g) : tri_synchronize(c); }
    int Output(tri_image* o) const { return g ? tri_group_get_output(g, o) : tri_get_output(c, o); }
    int Blit(uint32_t w, uint32_t h) const { return g ? tri_group_blit_linear(g, nullptr, w, h) : tri_blit_linear(c, nullptr, w, h); }
    int ReadPresent(uint8_t* p) const { return g ? tri_group_read_present(g, p) : tri_read_present(c, p); }
    int Readback(uint8_t* bgra, uint32_t* depth) const {
        return g ? tri_group_readback(g, bgra, depth) : tri_readback(c, bgra, depth);
    }
    int IdOutput(bool on) const { return g ? tri_group_set_id_output(g, on ? 1 : 0) : tri_set_id_output(c, on ? 1 : 0); }
    int ReadIds(uint32_t* ids) const { return g ? tri_group_read_ids(g, ids) : tri_read_ids(c, ids); }
    int Pick(int32_t x, int32_t y, tri_pick_result* out) const { return g ? tri_group_pick(g, x, y, out) : tri_pick(c, x, y, out); }
};

}  // namespace

Renderer::Renderer() = default;
Renderer::~Renderer() { Shutdown(); }

void Renderer::Init() {
    if (m_Initialised) return;
    m_TextureSlots.clear();
    m_TextureSlotLookup.clear();
    TextureSlot white;  // CreateDefaultTexture (Renderer.cpp:3404-3436)
    white.m_SourcePath = kDefaultTextureKey;
    white.m_Data.Width = white.m_Data.Height = 1;
    white.m_Data.Pixels = {0xFF, 0xFF, 0xFF, 0xFF};
    m_TextureSlots.push_back(white);
    m_TextureSlotLookup.emplace(kDefaultTextureKey, 0u);
    m_PerformanceHistory.assign(s_PerformanceHistorySize, FrameTimingSample{});
    CreateSkyboxCubemap();  // CreateDefaultSkybox (Renderer.cpp:3806-3816)
    // dataset capture starts disabled at the default directory; the environment can enable it (Renderer.cpp:551-576)
    m_FrameDatasetCaptureDirectory = DefaultDatasetDirectory();
    m_FrameDatasetCaptureInterval = 1;
    const char* enableCapture = std::getenv("TRIDENT_DATASET_CAPTURE_ENABLE");
    if (enableCapture && *enableCapture) {
        const char* directory = std::getenv("TRIDENT_DATASET_CAPTURE_DIR");
        if (directory && *directory) SetFrameDatasetCaptureDirectory(directory);
        SetFrameDatasetCaptureEnabled(true);
        LogError("frame dataset capture enabled, writing samples to", m_FrameDatasetCaptureDirectory.c_str());
    } else {
        SetFrameDatasetCaptureEnabled(false);
    }
    m_Initialised = true;
    m_Shutdown = false;
}

void Renderer::DestroyViewportTargets() {
    m_Pending.clear();  // (its targets go; tri_destroy / tri_group_destroy wait for their streams)
    DropObjects(m_Reprojection, tri_history_destroy);
    DropObjects(m_Taa, tri_taa_destroy);
    DropObjects(m_Upscale, tri_upscale_destroy);
    tri_recorder_destroy(m_Recorder);  // (waits for its captures; the next recorded DrawFrame makes a new one)
    m_Recorder = nullptr;
    DropGrab();  // (likewise; the next captured DrawFrame makes a new one)
    auto drop = [](ViewportContext& vc) {
        tri_destroy(vc.m_Ctx);
        tri_group_destroy(vc.m_Group);
        vc.m_Ctx = nullptr;
        vc.m_Group = nullptr;
        vc.m_HasImage = false;
        vc.m_Width = vc.m_Height = 0;
    };
    for (auto& it : m_Viewports) drop(it.second);
    for (auto& it : m_RingTargets)
        for (ViewportContext& vc : it.second) drop(vc);
    m_RingTargets.clear();
    m_LatestTarget.clear();
    tri_destroy(m_LegacyTarget.m_Ctx);
    tri_group_destroy(m_LegacyTarget.m_Group);
    m_LegacyTarget = ViewportContext{};
    m_PresentSource = nullptr;
    m_PresentGroup = nullptr;
    m_PresentLegacy = false;
    // after every context that bound them
    tri_geometry_destroy(m_SharedGeometry);
    m_SharedGeometry = nullptr;
    m_SharedGeometryGeneration = 0;
    for (tri_geometry* g : m_DeviceGeometry) tri_geometry_destroy(g);
    m_DeviceGeometry.clear();
    m_DeviceGeometryGeneration.clear();
    DropFonts();
    DropPoseSets();
}

void Renderer::DropFonts() {  // only while no context that was given one can still render with it
    for (auto& it : m_Fonts) tri_font_destroy(it.second);
    m_Fonts.clear();
}

void Renderer::SubmitText(uint32_t viewportId, const glm::vec2& position, const glm::vec4& color, const std::string& text) {
    if (text.empty()) return;
    if (!m_TextRenderer.IsLoaded() && !m_TextFontTried) {  // TextRenderer::LoadDefaultFont (TextRenderer.cpp:261-284)
        m_TextFontTried = true;
        const std::string path = m_AssetsDirectory + "/Fonts/JetBrainsMono-Regular.ttf";
        if (!m_TextRenderer.LoadFontFile(path, 32.0f))
            LogError("TextRenderer could not load the default font", path.c_str());
    }
    m_TextRenderer.QueueText(viewportId, position, color, text);  // (ignored without a font)
}

bool Renderer::SetTextFont(const std::string& path, float pixelHeight) {
    m_TextFontTried = true;  // an embedder that names a font does not get the default behind its back
    FinishFrame();           // no frame in flight samples the atlas that is about to go
    if (!m_TextRenderer.LoadFontFile(path, pixelHeight)) return false;  // (the previous font stays)
    auto clear = [](ViewportContext& vc) {  // every later frame sets its text anew, with the new atlas
        if (vc.m_Group) tri_group_set_text(vc.m_Group, nullptr, nullptr, 0);
        else if (vc.m_Ctx) tri_set_text(vc.m_Ctx, nullptr, nullptr, 0);
    };
    for (auto& it : m_Viewports) clear(it.second);
    for (auto& it : m_RingTargets)
        for (ViewportContext& vc : it.second) clear(vc);
    DropFonts();
    m_FontsVersion = m_TextRenderer.GetFontVersion();
    m_TextRenderer.BeginFrame();  // quads of the old glyph table are not drawn with the new atlas
    return true;
}

// The viewport's queued text onto this frame's target (count 0 when nothing is queued): called for every target
// before its tri_render, so ring targets (SetFramesInFlight > 1), which are separate contexts, each carry the text
// of the frame they render.
bool Renderer::SetTargetText(ViewportContext& vc, uint32_t viewportId) {
    m_TextQuads.clear();
    m_TextRenderer.LayoutViewport(viewportId, m_TextQuads);
    if (IsTemporalUpscalingEnabled(viewportId) && &vc != &m_LegacyTarget && vc.m_Info.Size.x > 0.0f && vc.m_Info.Size.y > 0.0f) {
        // the context is smaller than the viewport the quads were laid out for: drawn there, enlarged with the frame
        const float sx = (float)vc.m_Width / (float)(uint32_t)vc.m_Info.Size.x, sy = (float)vc.m_Height / (float)(uint32_t)vc.m_Info.Size.y;
        for (tri_text_quad& q : m_TextQuads) {
            q.x0 *= sx;
            q.x1 *= sx;
            q.y0 *= sy;
            q.y1 *= sy;
        }
    }
    if (m_TextQuads.empty()) {
        const int rc = vc.m_Group ? tri_group_set_text(vc.m_Group, nullptr, nullptr, 0) : tri_set_text(vc.m_Ctx, nullptr, nullptr, 0);
        return rc == TRI_OK;
    }
    if (m_FontsVersion != m_TextRenderer.GetFontVersion()) {
        DropFonts();  // (SetTextFont has waited for the frames and cleared the targets' text)
        m_FontsVersion = m_TextRenderer.GetFontVersion();
    }
    auto fontOn = [&](int32_t device) -> tri_font* {
        auto it = m_Fonts.find(device);
        if (it != m_Fonts.end()) return it->second;
        tri_font* f = nullptr;
        if (tri_font_create(device, m_TextRenderer.AtlasPixels().data(), TextRenderer::s_AtlasSize, TextRenderer::s_AtlasSize,
                            &f) != TRI_OK) {
            LogError("text atlas", tri_last_error());
            return nullptr;
        }
        m_Fonts.emplace(device, f);
        return f;
    };
    int rc;
    if (vc.m_Group) {
        std::vector<tri_font*> fonts;  // one per distinct device
        std::vector<int32_t> seen;
        for (int32_t d : m_Devices) {
            if (std::find(seen.begin(), seen.end(), d) != seen.end()) continue;
            seen.push_back(d);
            tri_font* f = fontOn(d);
            if (!f) return false;
            fonts.push_back(f);
        }
        rc = tri_group_set_text(vc.m_Group, fonts.data(), m_TextQuads.data(), (uint32_t)m_TextQuads.size());
    } else {
        tri_image img{};
        if (tri_get_output(vc.m_Ctx, &img) != TRI_OK) return false;
        tri_font* f = fontOn(img.device);
        if (!f) return false;
        rc = tri_set_text(vc.m_Ctx, f, m_TextQuads.data(), (uint32_t)m_TextQuads.size());
    }
    if (rc != TRI_OK) LogError("text overlay", tri_last_error());
    return rc == TRI_OK;
}

void Renderer::Shutdown() {
    StopRecording();  // the frames in flight reach the file, which is finalised
    m_FrameGenerator.Shutdown();  // (waits for a job in flight)
    m_AiFromDevice = false;
    DestroyViewportTargets();
    m_FrameDatasetRecorder.Flush();  // every queued sample is on disk
    m_PendingFrameReadback.clear();
    m_Viewports.clear();
    if (m_Initialised) m_Shutdown = true;
    m_Initialised = false;
}

void Renderer::SetFramesInFlight(uint32_t n) {
    n = std::min<uint32_t>(std::max<uint32_t>(n, 1u), 4u);
    if (n == m_FramesInFlight) return;
    FinishFrame();
    DestroyViewportTargets();  // rebuilt by the next DrawFrame's PrepareViewport
    m_FramesInFlight = n;
}

// Target `index` of a viewport (0: its m_Viewports entry; 1 .. n-1: the ring's), carrying the viewport's info.
Renderer::ViewportContext& Renderer::TargetOf(uint32_t viewportId, ViewportContext& primary, uint32_t index) {
    if (index == 0) return primary;
    std::vector<ViewportContext>& ring = m_RingTargets[viewportId];
    if (ring.size() < m_FramesInFlight - 1) ring.resize(m_FramesInFlight - 1);  // (sized once per SetFramesInFlight)
    ViewportContext& t = ring[index - 1];
    t.m_Info = primary.m_Info;
    return t;
}

const Renderer::ViewportContext* Renderer::LatestTarget(uint32_t viewportId) const {
    auto it = m_Viewports.find(viewportId);
    if (it == m_Viewports.end()) return nullptr;
    auto li = m_LatestTarget.find(viewportId);
    if (li == m_LatestTarget.end() || li->second == 0) return &it->second;
    auto ri = m_RingTargets.find(viewportId);
    if (ri == m_RingTargets.end() || ri->second.size() < li->second) return &it->second;
    return &ri->second[li->second - 1];
}

bool Renderer::SetDeviceCount(uint32_t count, const std::vector<int32_t>& devices) {
    std::vector<int32_t> devs;
    if (count > 1) {
        if (!devices.empty() && devices.size() != count) {
            LogError("SetDeviceCount", "device list length differs from the count");
            return false;
        }
        for (uint32_t i = 0; i < count; ++i) {
            const int32_t d = devices.empty() ? (int32_t)i : devices[i];
            if (d < 0) {
                LogError("SetDeviceCount", "negative device ordinal");
                return false;
            }
            devs.push_back(d);
        }
    }
    if (devs == m_Devices) return true;
    if (m_Recording) {  // the recorded frames in flight are written before their targets go
        if (devs.size() > 1) {
            LogError("SetDeviceCount", "multi-device viewports are not recorded: the recording was finalised");
            StopRecording();
        } else {
            FinishFrame();
        }
    }
    if (m_AiReadback && devs.size() > 1) {
        LogError("SetDeviceCount", "multi-device viewports have no AI readback: it was turned off");
        SetAiReadbackEnabled(false);
    }
    if (devs.size() > 1 && m_FrameGenerator.IsInitialised()) {  // ... and with it no generator
        LogError("SetDeviceCount", "multi-device viewports have no frame generator: the model was unloaded");
        m_FrameGenerator.Shutdown();
        if (m_AiFromDevice) SubmitAiInterpolation(nullptr, 0, 0, 0);
    }
    if (m_SelectionOutline && devs.size() > 1) {
        LogError("SetDeviceCount", "multi-device viewports draw no selection outline: it was turned off");
        m_SelectionOutline = false;
    }
    if (devs.size() > 1) {
        bool any = false;
        for (auto& it : m_MotionViewports) any |= it.second;
        if (any) LogError("SetDeviceCount", "multi-device viewports write no motion vectors: the output was turned off");
        m_MotionViewports.clear();
        m_MotionHistory.clear();
        any = false;
        for (auto& it : m_Reprojection) any |= it.second.m_Enabled;
        if (any) LogError("SetDeviceCount", "multi-device viewports have no history reprojection: it was turned off");
        DropObjects(m_Reprojection, tri_history_destroy);
        m_Reprojection.clear();
        any = false;
        for (auto& it : m_Taa) any |= it.second.m_Enabled;
        if (any) LogError("SetDeviceCount", "multi-device viewports have no temporal anti-aliasing: it was turned off");
        DropObjects(m_Taa, tri_taa_destroy);
        m_Taa.clear();
        any = false;
        for (auto& it : m_Upscale) any |= it.second.m_Enabled;
        if (any) LogError("SetDeviceCount", "multi-device viewports have no temporal upscaling: it was turned off");
        DropObjects(m_Upscale, tri_upscale_destroy);
        m_Upscale.clear();
    }
    DestroyViewportTargets();  // rebuilt by the next DrawFrame's PrepareViewport
    m_Devices = devs;
    return true;
}

// Multi-device viewports: one copy of the concatenated buffers per distinct device and generation,
// bound by every viewport's group (tri_group_bind_geometry picks each band's device copy).
bool Renderer::UploadSharedGeometry(std::vector<tri_geometry*>& out) {
    std::vector<int32_t> udev;
    for (int32_t d : m_Devices)
        if (std::find(udev.begin(), udev.end(), d) == udev.end()) udev.push_back(d);
    if (m_DeviceGeometry.size() != udev.size()) {
        for (tri_geometry* g : m_DeviceGeometry) tri_geometry_destroy(g);
        m_DeviceGeometry.assign(udev.size(), nullptr);
        m_DeviceGeometryGeneration.assign(udev.size(), 0);
    }
    const std::vector<tri_mesh_range> ranges = GetMeshRanges();
    for (size_t u = 0; u < udev.size(); ++u) {
        if (!m_DeviceGeometry[u] && tri_geometry_create(udev[u], &m_DeviceGeometry[u]) != TRI_OK) {
            LogError("UploadMeshFromCache", tri_last_error());
            m_DeviceGeometry[u] = nullptr;
            return false;
        }
        if (m_DeviceGeometryGeneration[u] != m_GeometryGeneration) {
            if (tri_geometry_upload(m_DeviceGeometry[u], m_VertexBuffer.data(), m_VertexBuffer.size(), m_IndexBuffer.data(),
                                    m_IndexBuffer.size(), ranges.data(), (uint32_t)ranges.size()) != TRI_OK) {
                LogError("UploadMeshFromCache", tri_last_error());
                return false;
            }
            m_DeviceGeometryGeneration[u] = m_GeometryGeneration;
            ++m_GeometryUploads;
        }
    }
    out = m_DeviceGeometry;
    return true;
}

// Renderer.cpp:3818-3927: the discovered cubemap (KTX, Default/ directory, loose px/nx/... PNG faces),
// else the solid 0x808080 fallback.
void Renderer::CreateSkyboxCubemap() {
    std::string source;
    Loader::CubemapTextureData data = Loader::DiscoverDefaultSkybox(m_AssetsDirectory, source);
    if (!data.IsValid()) {
        data = Loader::CubemapTextureData::CreateSolidColor(0x808080u);
        source = "solid 0x808080";
    }
    m_SkyboxCubemap = std::move(data);
    m_SkyboxSource = source;
    ++m_SkyboxGeneration;
}

void Renderer::SetAssetsDirectory(const std::string& directory) {
    m_AssetsDirectory = directory;
    if (m_Initialised) CreateSkyboxCubemap();
}

bool Renderer::SetSkyboxCubemap(const Loader::CubemapTextureData& cubemap) {
    if (!cubemap.IsValid()) {
        LogError("SetSkyboxCubemap", "cubemap needs 6 square faces of one of the three formats and their whole mip chain");
        return false;
    }
    m_SkyboxCubemap = cubemap;
    m_SkyboxSource = "SetSkyboxCubemap";
    ++m_SkyboxGeneration;
    return true;
}

// ---- geometry ---------------------------------------------------------------------------------
void Renderer::UploadMesh(const std::vector<Geometry::Mesh>& meshes, const std::vector<Geometry::Material>& materials,
                          const std::vector<std::string>& textures) {
    m_GeometryCache = meshes;
    m_Materials = materials;
    for (size_t& p : m_PrimitiveMeshIndices) p = kInvalidMeshIndex;
    ResolveMaterialTextureSlots(textures, 0, m_Materials.size());
    UploadMeshFromCache();
}

void Renderer::AppendMeshes(std::vector<Geometry::Mesh> meshes, std::vector<Geometry::Material> materials,
                            std::vector<std::string> textures) {
    if (meshes.empty()) return;
    const size_t oldMaterials = m_Materials.size();
    for (Geometry::Mesh& m : meshes) {
        if (m.MaterialIndex >= 0) m.MaterialIndex += static_cast<int32_t>(oldMaterials);
        m_GeometryCache.emplace_back(std::move(m));
    }
    const size_t offset = m_Materials.size();
    for (Geometry::Material& m : materials) m_Materials.emplace_back(std::move(m));
    ResolveMaterialTextureSlots(textures, offset, materials.size());
    UploadMeshFromCache();
}

size_t Renderer::GetOrCreatePrimitiveMeshIndex(MeshComponent::PrimitiveType type) {
    if (type == MeshComponent::PrimitiveType::None) return kInvalidMeshIndex;
    const size_t slot = static_cast<size_t>(type) - 1;
    if (slot >= 3) return kInvalidMeshIndex;
    const size_t existing = m_PrimitiveMeshIndices[slot];
    if (existing != kInvalidMeshIndex && existing < m_GeometryCache.size()) return existing;
    const size_t index = CreatePrimitiveMeshInCache(type);
    if (index == kInvalidMeshIndex) return index;
    if (!m_IsUploadingMeshes) UploadMeshFromCache();
    return index;
}

size_t Renderer::CreatePrimitiveMeshInCache(MeshComponent::PrimitiveType type) {
    const size_t slot = static_cast<size_t>(type) - 1;
    if (type == MeshComponent::PrimitiveType::None || slot >= 3) return kInvalidMeshIndex;
    const size_t existing = m_PrimitiveMeshIndices[slot];
    if (existing != kInvalidMeshIndex && existing < m_GeometryCache.size()) return existing;
    Geometry::Mesh mesh = type == MeshComponent::PrimitiveType::Cube     ? BuildPrimitiveCubeMesh()
                          : type == MeshComponent::PrimitiveType::Sphere ? BuildPrimitiveSphereMesh()
                                                                         : BuildPrimitiveQuadMesh();
    Geometry::Material material{};  // primitives: metallic 0, roughness 1 (Renderer.cpp:1900-1906)
    material.BaseColorFactor = {1.0f, 1.0f, 1.0f, 1.0f};
    material.MetallicFactor = 0.0f;
    material.RoughnessFactor = 1.0f;
    material.BaseColorTextureSlot = 0;
    mesh.MaterialIndex = static_cast<int32_t>(m_Materials.size());
    m_Materials.push_back(material);
    m_GeometryCache.push_back(std::move(mesh));
    m_PrimitiveMeshIndices[slot] = m_GeometryCache.size() - 1;
    ++m_MaterialGeneration;
    return m_GeometryCache.size() - 1;
}

void Renderer::EnsurePrimitiveMeshesInCache() {
    if (!m_Registry) return;
    for (ECS::Entity e : m_Registry->GetEntities()) {
        if (!m_Registry->HasComponent<MeshComponent>(e)) continue;
        MeshComponent& c = m_Registry->GetComponent<MeshComponent>(e);
        if (c.m_Primitive == MeshComponent::PrimitiveType::None) continue;
        if (c.m_MeshIndex != kInvalidMeshIndex && c.m_MeshIndex < m_GeometryCache.size()) continue;
        const size_t index = CreatePrimitiveMeshInCache(c.m_Primitive);
        if (index != kInvalidMeshIndex) c.m_MeshIndex = index;
    }
}

void Renderer::UploadMeshFromCache() {  // Renderer.cpp:1965-2116
    m_IsUploadingMeshes = true;
    EnsurePrimitiveMeshesInCache();
    m_VertexBuffer.clear();
    m_IndexBuffer.clear();
    m_MeshDrawInfo.clear();
    m_MeshBoundsMin.clear();
    m_MeshBoundsMax.clear();
    uint32_t firstIndex = 0;
    int32_t baseVertex = 0;
    for (const Geometry::Mesh& mesh : m_GeometryCache) {
        const size_t v0 = m_VertexBuffer.size();
        m_VertexBuffer.resize(v0 + mesh.Vertices.size());
        std::memcpy(m_VertexBuffer.data() + v0, mesh.Vertices.data(), mesh.Vertices.size() * sizeof(Vertex));
        m_IndexBuffer.insert(m_IndexBuffer.end(), mesh.Indices.begin(), mesh.Indices.end());  // mesh-local
        MeshDrawInfo info;
        info.m_FirstIndex = firstIndex;
        info.m_IndexCount = static_cast<uint32_t>(mesh.Indices.size());
        info.m_BaseVertex = baseVertex;
        info.m_MaterialIndex = mesh.MaterialIndex;
        m_MeshDrawInfo.push_back(info);
        glm::vec3 lo{INFINITY}, hi{-INFINITY};  // box of the referenced vertices (shadow frustum fit)
        for (uint32_t idx : mesh.Indices) {
            if (idx >= mesh.Vertices.size()) continue;
            const glm::vec3& p = mesh.Vertices[idx].Position;
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], p[a]);
                hi[a] = std::max(hi[a], p[a]);
            }
        }
        m_MeshBoundsMin.push_back(lo);
        m_MeshBoundsMax.push_back(hi);
        firstIndex += info.m_IndexCount;
        baseVertex += static_cast<int32_t>(mesh.Vertices.size());
    }
    if (m_HasSpriteGeometry) {  // after every cached mesh, outside m_MeshDrawInfo (no MeshComponent reaches it)
        const Geometry::Mesh quad = BuildSpriteQuadMesh();
        const size_t v0 = m_VertexBuffer.size();
        m_VertexBuffer.resize(v0 + quad.Vertices.size());
        std::memcpy(m_VertexBuffer.data() + v0, quad.Vertices.data(), quad.Vertices.size() * sizeof(Vertex));
        m_IndexBuffer.insert(m_IndexBuffer.end(), quad.Indices.begin(), quad.Indices.end());
        m_SpriteDrawInfo.m_FirstIndex = firstIndex;
        m_SpriteDrawInfo.m_IndexCount = static_cast<uint32_t>(quad.Indices.size());
        m_SpriteDrawInfo.m_BaseVertex = baseVertex;
        m_SpriteDrawInfo.m_MaterialIndex = -1;
    }
    m_MeshDrawCommands.clear();
    if (m_Registry) {
        for (ECS::Entity e : m_Registry->GetEntities()) {
            if (!m_Registry->HasComponent<MeshComponent>(e)) continue;
            MeshComponent& c = m_Registry->GetComponent<MeshComponent>(e);
            if (c.m_MeshIndex >= m_MeshDrawInfo.size()) continue;
            const MeshDrawInfo& d = m_MeshDrawInfo[c.m_MeshIndex];
            c.m_FirstIndex = d.m_FirstIndex;
            c.m_IndexCount = d.m_IndexCount;
            c.m_BaseVertex = d.m_BaseVertex;
            c.m_MaterialIndex = d.m_MaterialIndex;
        }
    }
    m_ModelCount = m_GeometryCache.size();
    m_TriangleCount = firstIndex / 3;  // the cached meshes' triangles (the sprite quad is not a model)
    ++m_GeometryGeneration;
    ++m_MaterialGeneration;
    m_IsUploadingMeshes = false;
}

// ---- textures ---------------------------------------------------------------------------------
void Renderer::UploadTexture(const std::string& texturePath, const Loader::TextureData& texture) {
    const std::string key = NormalizeTexturePath(texturePath);
    if (texture.Width <= 0 || texture.Height <= 0 ||
        texture.Pixels.size() < (size_t)texture.Width * texture.Height * 4) {
        LogError("UploadTexture", "texture has no RGBA8 pixel data; using the default slot");
        m_TextureSlotLookup[key] = 0u;
        return;
    }
    auto it = m_TextureSlotLookup.find(key);
    uint32_t slot;
    if (it != m_TextureSlotLookup.end() && it->second != 0) {
        slot = it->second;
    } else {
        if (m_TextureSlots.size() >= TRI_MAX_TEXTURE_SLOTS) {
            LogError("UploadTexture", "all 256 texture slots are in use; using the default slot");
            m_TextureSlotLookup[key] = 0u;
            return;
        }
        slot = static_cast<uint32_t>(m_TextureSlots.size());
        m_TextureSlots.emplace_back();
        m_TextureSlotLookup[key] = slot;
    }
    m_TextureSlots[slot].m_SourcePath = key;
    m_TextureSlots[slot].m_Data = texture;
    ++m_TextureGeneration;
}

int32_t Renderer::ResolveTextureSlot(const std::string& texturePath) {
    const std::string key = NormalizeTexturePath(texturePath);
    if (key.empty()) return 0;
    auto it = m_TextureSlotLookup.find(key);
    if (it != m_TextureSlotLookup.end()) return static_cast<int32_t>(it->second);
    // Load on first use (ResolveTextureSlot -> TextureLoader::Load, Renderer.cpp:3700-3745). Formats
    // stb would decode but that are not restated here (PNG, JPEG) fail like a failed load in the
    // reference: the default slot (:3740-3745).
    const Loader::TextureData data = Loader::TextureLoader::Load(key);
    if (data.Width > 0) {
        UploadTexture(key, data);
        it = m_TextureSlotLookup.find(key);
        if (it != m_TextureSlotLookup.end()) return static_cast<int32_t>(it->second);
    }
    LogError("ResolveTextureSlot", (key + " could not be loaded; using the default slot").c_str());
    m_TextureSlotLookup.emplace(key, 0u);
    return 0;
}

void Renderer::ResolveMaterialTextureSlots(const std::vector<std::string>& textures, size_t offset, size_t count) {
    if (m_Materials.empty()) return;
    const size_t safeOffset = std::min(offset, m_Materials.size());
    const size_t n = std::min(count, m_Materials.size() - safeOffset);
    for (size_t i = 0; i < n; ++i) {
        Geometry::Material& m = m_Materials[safeOffset + i];
        m.BaseColorTextureSlot = 0;
        if (m.BaseColorTextureIndex < 0 || (size_t)m.BaseColorTextureIndex >= textures.size()) continue;
        const std::string key = NormalizeTexturePath(textures[m.BaseColorTextureIndex]);
        if (key.empty()) continue;
        m.BaseColorTextureSlot = ResolveTextureSlot(key);
    }
    ++m_MaterialGeneration;
}

// ---- frame preparation --------------------------------------------------------------------------
void Renderer::GatherMeshDraws() {  // Renderer.cpp:2910-2994
    m_MeshDrawCommands.clear();
    if (!m_Registry) return;
    for (ECS::Entity e : m_Registry->GetEntities()) {
        if (!m_Registry->HasComponent<MeshComponent>(e)) continue;
        MeshComponent& c = m_Registry->GetComponent<MeshComponent>(e);
        if (!c.m_Visible) continue;
        if (c.m_Primitive != MeshComponent::PrimitiveType::None && c.m_MeshIndex == kInvalidMeshIndex) {
            c.m_MeshIndex = GetOrCreatePrimitiveMeshIndex(c.m_Primitive);
            if (c.m_MeshIndex == kInvalidMeshIndex) continue;
        }
        if (c.m_MeshIndex >= m_MeshDrawInfo.size()) continue;
        if (m_MeshDrawInfo[c.m_MeshIndex].m_IndexCount == 0) continue;
        MeshDrawCommand cmd;
        if (m_Registry->HasComponent<Transform>(e)) cmd.m_ModelMatrix = ComposeTransform(m_Registry->GetComponent<Transform>(e));
        if (m_Registry->HasComponent<TextureComponent>(e)) {
            TextureComponent& t = m_Registry->GetComponent<TextureComponent>(e);
            if (t.m_IsDirty || t.m_TextureSlot < 0) {
                t.m_TextureSlot = ResolveTextureSlot(t.m_TexturePath);
                t.m_IsDirty = false;
            }
            cmd.m_TextureComponent = &t;
        }
        if (m_Registry->HasComponent<AnimationComponent>(e))
            cmd.m_AnimationComponent = &m_Registry->GetComponent<AnimationComponent>(e);
        cmd.m_Component = &c;
        cmd.m_Entity = e;
        m_MeshDrawCommands.push_back(cmd);
    }
}

void Renderer::GatherSpriteDraws() {  // Renderer.cpp:2996-3042
    m_SpriteDrawList.clear();
    if (!m_Registry) return;
    for (ECS::Entity e : m_Registry->GetEntities()) {
        if (!m_Registry->HasComponent<Transform>(e) || !m_Registry->HasComponent<SpriteComponent>(e)) continue;
        SpriteComponent& sprite = m_Registry->GetComponent<SpriteComponent>(e);
        if (!sprite.m_Visible) continue;
        TextureComponent* tex = nullptr;
        if (m_Registry->HasComponent<TextureComponent>(e)) {
            tex = &m_Registry->GetComponent<TextureComponent>(e);
            if (tex->m_IsDirty || tex->m_TextureSlot < 0) {
                tex->m_TextureSlot = ResolveTextureSlot(tex->m_TexturePath);
                tex->m_IsDirty = false;
            }
        }
        SpriteDrawCommand cmd;
        cmd.m_ModelMatrix = ComposeTransform(m_Registry->GetComponent<Transform>(e));
        cmd.m_Component = &sprite;
        cmd.m_TextureComponent = tex;
        cmd.m_Entity = e;
        m_SpriteDrawList.push_back(cmd);
    }
}

void Renderer::GatherDraws() {
    GatherMeshDraws();
    GatherSpriteDraws();
    if (!m_SpriteDrawList.empty() && !m_HasSpriteGeometry) {
        // first sprite: the quad joins the device geometry (the reference built its own buffer at Init);
        // the upload clears the mesh commands, which are gathered again (no texture slot changes)
        m_HasSpriteGeometry = true;
        UploadMeshFromCache();
        GatherMeshDraws();
    }
}

// Renderer.cpp:3168-3245: each animated draw gets a slice [offset, offset + count) of one palette
// (count clamped to s_MaxBonesPerSkeleton); draws without a palette keep offset 0 / count 0.
// With device poses on, the draws the device poses (SetDevicePoseEnabled) take slices behind that palette instead:
// m_PoseDraws, submitted by SubmitPoses.
void Renderer::PrepareBonePaletteBuffer() {
    m_BonePalette.clear();
    m_PoseDraws.clear();
    std::vector<MeshDrawCommand*> posed;
    uint32_t total = 0;
    for (MeshDrawCommand& cmd : m_MeshDrawCommands) {
        cmd.m_BoneOffset = 0;
        cmd.m_BoneCount = 0;
        if (cmd.m_AnimationComponent && PosesOnDevice(*cmd.m_AnimationComponent)) {
            posed.push_back(&cmd);
            continue;
        }
        if (!cmd.m_AnimationComponent || cmd.m_AnimationComponent->m_BoneMatrices.empty()) continue;
        const auto& src = cmd.m_AnimationComponent->m_BoneMatrices;
        const uint32_t n = (uint32_t)std::min<size_t>(src.size(), s_MaxBonesPerSkeleton);
        cmd.m_BoneOffset = total;
        cmd.m_BoneCount = n;
        total += n;
        for (uint32_t b = 0; b < n; ++b) {
            float m[16];
            CopyMat(src[b], m);
            m_BonePalette.insert(m_BonePalette.end(), m, m + 16);
        }
    }
    for (MeshDrawCommand* cmd : posed) {  // behind the uploaded prefix, back to back
        const AnimationComponent& a = *cmd->m_AnimationComponent;
        const size_t bones = Animation::AnimationAssetService::Get().GetSkeleton(a.m_SkeletonAssetHandle)->m_Bones.size();
        cmd->m_BoneOffset = total;
        cmd->m_BoneCount = (uint32_t)std::min<size_t>(bones, s_MaxBonesPerSkeleton);
        m_PoseDraws.push_back({a.m_SkeletonAssetHandle, a.m_AnimationAssetHandle, a.m_CurrentClipIndex, a.m_CurrentTime, total,
                               a.m_StateMachine ? &a.m_StateMachine->GetProgram() : nullptr});
        total += cmd->m_BoneCount;
    }
}

bool Renderer::PosesOnDevice(const AnimationComponent& a) const {
    if (!m_DevicePose || a.m_SkeletonAssetHandle == Animation::AnimationAssetService::s_InvalidHandle) return false;
    // a state machine: the program its last Advance emitted must be one the device takes and must have been emitted
    // against this component's assets; otherwise the CPU system evaluates it and its matrices join the uploaded prefix
    if (a.m_StateMachine && (!a.m_StateMachine->GetProgram().FitsDevice() ||
                             a.m_StateMachine->GetSkeletonHandle() != a.m_SkeletonAssetHandle ||
                             a.m_StateMachine->GetAnimationLibraryHandle() != a.m_AnimationAssetHandle))
        return false;
    const auto& service = Animation::AnimationAssetService::Get();
    if (m_PoseCompatibleGeneration != service.GetGeneration()) {  // something was registered: look again
        m_PoseCompatible.clear();
        m_PoseCompatibleGeneration = service.GetGeneration();
    }
    const auto key = std::make_pair(a.m_SkeletonAssetHandle, a.m_AnimationAssetHandle);
    auto known = m_PoseCompatible.find(key);
    if (known == m_PoseCompatible.end()) {
        const Animation::Skeleton* sk = service.GetSkeleton(key.first);
        known = m_PoseCompatible.emplace(key, sk && Animation::DevicePoseCompatible(*sk, service.GetAnimationClips(key.second))).first;
    }
    return known->second;
}

void Renderer::DropPoseSets() {  // only while no context can still pose from them
    for (auto& it : m_PoseSets) tri_animset_destroy(it.second.m_Set);
    m_PoseSets.clear();
}

// The (skeleton asset, animation asset) pair on a device, added to that device's set at its first use: the decomposed
// defaults, and every clip with its channels resolved against the skeleton (a channel without a bone is left out).
Renderer::PoseAssetOnDevice* Renderer::PoseAssetOn(int32_t device, size_t skeleton, size_t animation) {
    if (m_PoseSets.empty()) m_PoseSetsGeneration = Animation::AnimationAssetService::Get().GetGeneration();
    PoseDeviceSet& ds = m_PoseSets[device];
    if (!ds.m_Set && tri_animset_create(device, &ds.m_Set) != TRI_OK) return nullptr;
    const auto key = std::make_pair(skeleton, animation);
    auto have = ds.m_Assets.find(key);
    if (have != ds.m_Assets.end()) return &have->second;
    const auto& service = Animation::AnimationAssetService::Get();
    const Animation::Skeleton* sk = service.GetSkeleton(skeleton);
    if (!sk) return nullptr;
    std::vector<tri_pose_bone> bones(sk->m_Bones.size());
    for (size_t b = 0; b < bones.size(); ++b) {
        const Animation::Bone& src = sk->m_Bones[b];
        const Animation::TransformDecomposition d = Animation::DecomposeBindTransform(src.m_LocalBindTransform);
        tri_pose_bone& o = bones[b];
        std::memset(&o, 0, sizeof o);
        o.parent = src.m_ParentIndex;
        o.translation[0] = d.m_Translation.x; o.translation[1] = d.m_Translation.y; o.translation[2] = d.m_Translation.z;
        o.rotation[0] = d.m_Rotation.w; o.rotation[1] = d.m_Rotation.x; o.rotation[2] = d.m_Rotation.y; o.rotation[3] = d.m_Rotation.z;
        o.scale[0] = d.m_Scale.x; o.scale[1] = d.m_Scale.y; o.scale[2] = d.m_Scale.z;
        CopyMat(src.m_InverseBindMatrix, o.inverse_bind);
    }
    PoseAssetOnDevice out;
    if (tri_animset_add_skeleton(ds.m_Set, bones.data(), (uint32_t)bones.size(), sk->m_RootBoneIndex, &out.m_Skeleton) != TRI_OK)
        return nullptr;
    if (const std::vector<Animation::AnimationClip>* clips = service.GetAnimationClips(animation)) {
        for (const Animation::AnimationClip& clip : *clips) {
            std::vector<tri_pose_channel> channels;
            std::vector<float> vt, vv, qt, qv;
            auto vec = [&](const std::vector<Animation::VectorKeyframe>& keys, uint32_t& first, uint32_t& count) {
                first = (uint32_t)vt.size();
                count = (uint32_t)keys.size();
                for (const auto& k : keys) {
                    vt.push_back(k.m_TimeSeconds);
                    vv.insert(vv.end(), {k.m_Value.x, k.m_Value.y, k.m_Value.z});
                }
            };
            for (const Animation::TransformChannel& ch : clip.m_Channels) {
                const int bone = Animation::ResolveChannelBoneIndex(ch, *sk, clip.m_Name);
                if (bone < 0 || (size_t)bone >= bones.size()) continue;
                tri_pose_channel o{};
                o.bone = (uint32_t)bone;
                vec(ch.m_TranslationKeys, o.translation_first, o.translation_count);
                vec(ch.m_ScaleKeys, o.scale_first, o.scale_count);
                o.rotation_first = (uint32_t)qt.size();
                o.rotation_count = (uint32_t)ch.m_RotationKeys.size();
                for (const auto& k : ch.m_RotationKeys) {
                    qt.push_back(k.m_TimeSeconds);
                    qv.insert(qv.end(), {k.m_Value.w, k.m_Value.x, k.m_Value.y, k.m_Value.z});
                }
                channels.push_back(o);
            }
            uint32_t index = 0;
            if (tri_animset_add_clip(ds.m_Set, out.m_Skeleton, channels.data(), (uint32_t)channels.size(), vt.data(), vv.data(),
                                     (uint32_t)vt.size(), qt.data(), qv.data(), (uint32_t)qt.size(), clip.m_DurationSeconds,
                                     &index) != TRI_OK)
                return nullptr;
            out.m_Clips.push_back(index);
        }
    }
    return &ds.m_Assets.emplace(key, std::move(out)).first->second;
}

// This frame's posed draws onto a target: one tri_pose_palette (every band of a group) behind the uploaded prefix.
bool Renderer::SubmitPoses(ViewportContext& vc) {
    const Target t{vc.m_Ctx, vc.m_Group};
    std::vector<int32_t> devices;
    if (vc.m_Group) {
        for (int32_t d : m_Devices)
            if (std::find(devices.begin(), devices.end(), d) == devices.end()) devices.push_back(d);
    } else {
        tri_image img{};
        if (tri_get_output(vc.m_Ctx, &img) != TRI_OK) return false;
        devices.push_back(img.device);
    }
    // one program among the draws: every posed draw goes through tri_pose_graph, the plain clips as [CLIP] programs
    for (const PoseDraw& p : m_PoseDraws)
        if (p.m_Program) return SubmitPoseGraph(vc, devices);
    std::vector<tri_animset*> sets;
    m_PoseInstances.clear();
    for (size_t di = 0; di < devices.size(); ++di) {
        for (size_t i = 0; i < m_PoseDraws.size(); ++i) {
            const PoseDraw& p = m_PoseDraws[i];
            const PoseAssetOnDevice* on = PoseAssetOn(devices[di], p.m_Skeleton, p.m_Animation);
            if (!on) return false;
            const uint32_t clip = p.m_Clip < on->m_Clips.size() ? on->m_Clips[p.m_Clip] : TRI_POSE_BIND;
            const tri_pose_instance inst{on->m_Skeleton, clip, p.m_Time, p.m_Offset};
            if (di == 0) m_PoseInstances.push_back(inst);
            else if (std::memcmp(&m_PoseInstances[i], &inst, sizeof inst) != 0) {  // the sets were filled in one order
                LogError("device poses", "the devices' sets disagree");
                return false;
            }
        }
        if (!m_PoseDraws.empty()) sets.push_back(m_PoseSets[devices[di]].m_Set);
    }
    if (t.Pose(sets.data(), m_PoseInstances.data(), (uint32_t)m_PoseInstances.size()) != TRI_OK) return false;
    vc.m_HasPosedSuffix = !m_PoseInstances.empty();
    return true;
}

bool Renderer::SubmitPoseGraph(ViewportContext& vc, const std::vector<int32_t>& devices) {
    const Target t{vc.m_Ctx, vc.m_Group};
    std::vector<tri_animset*> sets;
    std::vector<tri_pose_graph_instance> instances;
    std::vector<tri_pose_op> ops;
    std::vector<float> weights;
    for (size_t di = 0; di < devices.size(); ++di) {
        instances.clear();
        ops.clear();
        for (const PoseDraw& p : m_PoseDraws) {
            PoseAssetOnDevice* on = PoseAssetOn(devices[di], p.m_Skeleton, p.m_Animation);
            if (!on) return false;
            const uint32_t first = (uint32_t)ops.size();
            if (!p.m_Program) {
                if (p.m_Clip < on->m_Clips.size()) ops.push_back(tri_pose_op{TRI_POSE_OP_CLIP, on->m_Clips[p.m_Clip], p.m_Time, 0u});
                else ops.push_back(tri_pose_op{TRI_POSE_OP_REST, 0u, 0.0f, 0u});
            } else {
                const size_t bones = Animation::AnimationAssetService::Get().GetSkeleton(p.m_Skeleton)->m_Bones.size();
                for (const Animation::PoseOp& op : p.m_Program->m_Ops) {
                    tri_pose_op o{op.m_Op, op.m_A, op.m_F, 0u};
                    if (op.m_Op == Animation::PoseOp::Clip) {
                        if (op.m_A >= on->m_Clips.size()) return false;
                        o.a = on->m_Clips[op.m_A];
                    } else if ((op.m_Op == Animation::PoseOp::Blend || op.m_Op == Animation::PoseOp::Add) &&
                               op.m_A != Animation::PoseOp::s_NoMask) {
                        if (op.m_A >= p.m_Program->m_Masks.size()) return false;
                        // by content, at its first use on this device: new weights are a new mask
                        weights = p.m_Program->m_Masks[op.m_A].m_BoneWeights;
                        weights.resize(bones, 1.0f);
                        auto have = on->m_Masks.find(weights);
                        if (have == on->m_Masks.end()) {
                            uint32_t index = 0;
                            if (tri_animset_add_mask(m_PoseSets[devices[di]].m_Set, on->m_Skeleton, weights.data(), (uint32_t)weights.size(),
                                                     &index) != TRI_OK)
                                return false;
                            have = on->m_Masks.emplace(weights, index).first;
                        }
                        o.a = have->second;
                    }
                    ops.push_back(o);
                }
            }
            instances.push_back(tri_pose_graph_instance{on->m_Skeleton, first, (uint32_t)ops.size() - first, p.m_Offset});
        }
        if (di == 0) {
            m_PoseGraphInstances = instances;
            m_PoseOps = ops;
        } else if (instances.size() != m_PoseGraphInstances.size() || ops.size() != m_PoseOps.size() ||
                   std::memcmp(instances.data(), m_PoseGraphInstances.data(), instances.size() * sizeof instances[0]) != 0 ||
                   std::memcmp(ops.data(), m_PoseOps.data(), ops.size() * sizeof ops[0]) != 0) {  // the sets were filled in one order
            LogError("device poses", "the devices' sets disagree");
            return false;
        }
        sets.push_back(m_PoseSets[devices[di]].m_Set);
    }
    if (t.PoseGraph(sets.data(), m_PoseGraphInstances.data(), (uint32_t)m_PoseGraphInstances.size(), m_PoseOps.data(),
                    (uint32_t)m_PoseOps.size()) != TRI_OK)
        return false;
    vc.m_HasPosedSuffix = true;
    return true;
}

void Renderer::BuildDrawList(std::vector<tri_draw>& out, std::vector<ECS::Entity>* entities) const {  // Renderer.cpp:5110-5151
    out.clear();
    if (entities) entities->clear();  // the draw index -> entity table of this list (entity ids)
    for (const MeshDrawCommand& cmd : m_MeshDrawCommands) {
        if (!cmd.m_Component || cmd.m_Component->m_MeshIndex >= m_MeshDrawInfo.size()) continue;
        const MeshDrawInfo& info = m_MeshDrawInfo[cmd.m_Component->m_MeshIndex];
        if (info.m_IndexCount == 0) continue;
        tri_draw d;
        std::memset(&d, 0, sizeof d);
        d.mesh_index = static_cast<uint32_t>(cmd.m_Component->m_MeshIndex);
        tri_push_constant& pc = d.pc;  // RenderablePushConstant defaults (RenderData.h:16-29)
        CopyMat(cmd.m_ModelMatrix, pc.model);
        pc.tint[0] = pc.tint[1] = pc.tint[2] = pc.tint[3] = 1.0f;
        pc.texture_scale[0] = pc.texture_scale[1] = 1.0f;
        pc.tiling_factor = 1.0f;
        int32_t slot = 0;
        if (cmd.m_TextureComponent && cmd.m_TextureComponent->m_TextureSlot >= 0)
            slot = cmd.m_TextureComponent->m_TextureSlot;
        else if (info.m_MaterialIndex >= 0 && (size_t)info.m_MaterialIndex < m_Materials.size())
            slot = m_Materials[info.m_MaterialIndex].BaseColorTextureSlot;
        pc.texture_slot = slot;
        pc.material_index = info.m_MaterialIndex;
        pc.bone_offset = static_cast<int32_t>(cmd.m_BoneOffset);  // :5145-5146
        pc.bone_count = static_cast<int32_t>(cmd.m_BoneCount);
        out.push_back(d);
        if (entities) entities->push_back(cmd.m_Entity);
    }
    if (!m_HasSpriteGeometry) return;
    for (const SpriteDrawCommand& cmd : m_SpriteDrawList) {  // DrawSprites, Renderer.cpp:3044-3089
        if (!cmd.m_Component) continue;
        const SpriteComponent& sp = *cmd.m_Component;
        tri_draw d;
        std::memset(&d, 0, sizeof d);
        d.mesh_index = static_cast<uint32_t>(m_MeshDrawInfo.size());  // the sprite quad's range
        tri_push_constant& pc = d.pc;
        CopyMat(cmd.m_ModelMatrix, pc.model);
        pc.tint[0] = sp.m_TintColor.x; pc.tint[1] = sp.m_TintColor.y;
        pc.tint[2] = sp.m_TintColor.z; pc.tint[3] = sp.m_TintColor.w;
        pc.texture_scale[0] = sp.m_UVScale.x; pc.texture_scale[1] = sp.m_UVScale.y;
        pc.texture_offset[0] = sp.m_UVOffset.x; pc.texture_offset[1] = sp.m_UVOffset.y;
        pc.tiling_factor = sp.m_TilingFactor;
        pc.use_material_override = sp.m_UseMaterialOverride ? 1 : 0;
        pc.sort_bias = sp.m_SortOffset;
        pc.texture_slot = (cmd.m_TextureComponent && cmd.m_TextureComponent->m_TextureSlot >= 0)
                              ? cmd.m_TextureComponent->m_TextureSlot : 0;
        pc.material_index = -1;  // RenderablePushConstant default (RenderData.h:25)
        out.push_back(d);
        if (entities) entities->push_back(cmd.m_Entity);
    }
}

void Renderer::UpdateUniformBuffer(const Camera* camera, tri_global_ubo& g) const {  // Renderer.cpp:5822-5925
    std::memset(&g, 0, sizeof g);
    if (camera) {
        CopyMat(camera->GetViewMatrix(), g.view);
        CopyMat(camera->GetProjectionMatrix(), g.projection);
        const glm::vec3 p = camera->GetPosition();
        g.camera_position[0] = p.x; g.camera_position[1] = p.y; g.camera_position[2] = p.z;
    } else {
        CopyMat(glm::mat4(1.0f), g.view);
        CopyMat(glm::mat4(1.0f), g.projection);
    }
    g.camera_position[3] = 1.0f;
    g.ambient_color_intensity[0] = m_AmbientColor.x;
    g.ambient_color_intensity[1] = m_AmbientColor.y;
    g.ambient_color_intensity[2] = m_AmbientColor.z;
    g.ambient_color_intensity[3] = m_AmbientIntensity;
    glm::vec3 dir = glm::normalize(glm::vec3{-0.5f, -1.0f, -0.3f});  // s_DefaultDirectional* (Renderer.h:464-466)
    glm::vec3 color{1.0f, 0.98f, 0.92f};
    float intensity = 5.0f;
    uint32_t ndir = 0, npt = 0;
    if (m_Registry) {
        for (ECS::Entity e : m_Registry->GetEntities()) {
            if (!m_Registry->HasComponent<LightComponent>(e)) continue;
            const LightComponent& L = m_Registry->GetComponent<LightComponent>(e);
            if (!L.m_Enabled) continue;
            if (L.m_Type == LightComponent::Type::Directional) {
                if (ndir == 0) {
                    if (glm::dot(L.m_Direction, L.m_Direction) > 0.0001f) dir = glm::normalize(L.m_Direction);
                    color = L.m_Color;
                    intensity = std::max(L.m_Intensity, 0.0f);
                }
                ++ndir;
                continue;
            }
            if (L.m_Type == LightComponent::Type::Point) {
                if (npt >= TRI_MAX_POINT_LIGHTS) continue;
                glm::vec3 pos{0.0f};
                if (m_Registry->HasComponent<Transform>(e)) pos = m_Registry->GetComponent<Transform>(e).Position;
                tri_point_light& pl = g.point_lights[npt++];
                pl.position_range[0] = pos.x; pl.position_range[1] = pos.y; pl.position_range[2] = pos.z;
                pl.position_range[3] = std::max(L.m_Range, 0.0f);
                pl.color_intensity[0] = L.m_Color.x; pl.color_intensity[1] = L.m_Color.y;
                pl.color_intensity[2] = L.m_Color.z; pl.color_intensity[3] = std::max(L.m_Intensity, 0.0f);
            }
        }
    }
    const bool fallback = (ndir == 0 && npt == 0);
    g.directional_light_direction[0] = dir.x; g.directional_light_direction[1] = dir.y;
    g.directional_light_direction[2] = dir.z; g.directional_light_direction[3] = 0.0f;
    g.directional_light_color[0] = color.x; g.directional_light_color[1] = color.y;
    g.directional_light_color[2] = color.z; g.directional_light_color[3] = intensity;
    g.light_counts[0] = (ndir > 0 || fallback) ? 1u : 0u;
    g.light_counts[1] = npt;
    // AiBlendConfig (Renderer.cpp:5916-5925): (strength, 1 / width, 1 / height, 1) while an AI frame is held, else 0
    if (m_AiWidth && m_AiHeight) {
        g.ai_blend_config[0] = m_AiBlendStrength;
        g.ai_blend_config[1] = 1.0f / (float)std::max<uint32_t>(m_AiWidth, 1);
        g.ai_blend_config[2] = 1.0f / (float)std::max<uint32_t>(m_AiHeight, 1);
        g.ai_blend_config[3] = 1.0f;
    } else {
        std::memset(g.ai_blend_config, 0, sizeof g.ai_blend_config);
    }
}

bool Renderer::SubmitAiInterpolation(const float* pixels, uint32_t width, uint32_t height, uint32_t channels) {
    ++m_AiGeneration;
    m_AiFromDevice = false;
    if (!pixels || width == 0 || height == 0 || channels == 0) {  // no frame: the texture is not ready, no blend
        m_AiFrame.clear();
        m_AiWidth = m_AiHeight = 0;
        return true;
    }
    // UploadAiInterpolationToGpu's packing (Renderer.cpp:1572-1590)
    const size_t n = (size_t)width * height;
    m_AiFrame.resize(n * 4);
    for (size_t p = 0; p < n; ++p)
        for (uint32_t ch = 0; ch < 4; ++ch) {
            float v = 0.0f;
            if (ch < channels) v = pixels[p * channels + ch];
            else if (ch == 3) v = 1.0f;  // opaque when the network omits alpha
            v = std::min(std::max(v, 0.0f), 1.0f);
            m_AiFrame[p * 4 + ch] = (uint8_t)std::round(v * 255.0f);
        }
    m_AiWidth = width;
    m_AiHeight = height;
    return true;
}

bool Renderer::BuildShadowConfig(tri_shadow_config& out) {
    std::memset(&out, 0, sizeof out);
    if (!m_Registry || m_ShadowMapSize == 0) return false;
    const LightComponent* sun = nullptr;  // the directional light UpdateUniformBuffer uses (first enabled)
    for (ECS::Entity e : m_Registry->GetEntities()) {
        if (!m_Registry->HasComponent<LightComponent>(e)) continue;
        const LightComponent& L = m_Registry->GetComponent<LightComponent>(e);
        if (L.m_Enabled && L.m_Type == LightComponent::Type::Directional) {
            sun = &L;
            break;
        }
    }
    if (!sun || !sun->m_ShadowCaster) return false;
    glm::vec3 lo{INFINITY}, hi{-INFINITY};  // world box of the drawn meshes
    for (const MeshDrawCommand& cmd : m_MeshDrawCommands) {
        if (!cmd.m_Component || cmd.m_Component->m_MeshIndex >= m_MeshBoundsMin.size()) continue;
        const glm::vec3 a = m_MeshBoundsMin[cmd.m_Component->m_MeshIndex], b = m_MeshBoundsMax[cmd.m_Component->m_MeshIndex];
        if (a.x > b.x) continue;
        for (int k = 0; k < 8; ++k) {
            const glm::vec4 c{(k & 1) ? b.x : a.x, (k & 2) ? b.y : a.y, (k & 4) ? b.z : a.z, 1.0f};
            const glm::vec4 w = cmd.m_ModelMatrix * c;
            for (int ax = 0; ax < 3; ++ax) {
                lo[ax] = std::min(lo[ax], w[ax]);
                hi[ax] = std::max(hi[ax], w[ax]);
            }
        }
    }
    for (const SpriteDrawCommand& cmd : m_SpriteDrawList) {  // sprites cast too: their quad's corners
        if (!m_HasSpriteGeometry) break;
        for (int k = 0; k < 4; ++k) {
            const glm::vec4 c{(k & 1) ? 0.5f : -0.5f, (k & 2) ? 0.5f : -0.5f, 0.0f, 1.0f};
            const glm::vec4 w = cmd.m_ModelMatrix * c;
            for (int ax = 0; ax < 3; ++ax) {
                lo[ax] = std::min(lo[ax], w[ax]);
                hi[ax] = std::max(hi[ax], w[ax]);
            }
        }
    }
    if (lo.x > hi.x) return false;
    glm::vec3 dir{-0.5f, -1.0f, -0.3f};
    if (glm::dot(sun->m_Direction, sun->m_Direction) > 0.0001f) dir = sun->m_Direction;
    const float d[3] = {dir.x, dir.y, dir.z}, mn[3] = {lo.x, lo.y, lo.z}, mx[3] = {hi.x, hi.y, hi.z};
    if (tri_shadow_fit_ortho(d, mn, mx, out.light_view_proj) != TRI_OK) return false;
    out.size = m_ShadowMapSize;
    out.depth_bias = 0.001f;
    out.slope_bias = 2.0f;
    return true;
}

const Camera* Renderer::GetActiveCamera(const ViewportContext& context) const {  // Renderer.cpp:4545-4574
    const uint32_t id = context.m_Info.ViewportID;
    if (id == 1u) return m_EditorCamera;
    if (id == 2u) return (m_RuntimeCameraReady && m_RuntimeCamera) ? m_RuntimeCamera : m_EditorCamera;
    if (m_EditorCamera) return m_EditorCamera;
    return (m_RuntimeCameraReady && m_RuntimeCamera) ? m_RuntimeCamera : nullptr;
}

const Camera* Renderer::GetActiveCamera() const {
    if (m_EditorCamera) return m_EditorCamera;
    return (m_RuntimeCameraReady && m_RuntimeCamera) ? m_RuntimeCamera : nullptr;
}

void Renderer::SetViewport(uint32_t viewportId, const ViewportInfo& info) {
    ViewportContext& ctx = m_Viewports[viewportId];
    ctx.m_Info = info;
    ctx.m_Info.ViewportID = viewportId;
    // the recorded viewport keeps the recording extent (every FRAME record has the session's size); a SetViewport
    // after the recording ends sizes it again
    if (m_Recording && viewportId == m_RecordingViewportId)
        ctx.m_Info.Size = glm::vec2((float)m_RecordingWidth, (float)m_RecordingHeight);
    m_LastViewport = ctx.m_Info;
    m_ActiveViewportId = viewportId;  // Renderer.cpp:2753-2754
}

ViewportInfo Renderer::GetViewport() const { return m_LastViewport; }

glm::mat4 Renderer::GetViewportViewMatrix(uint32_t id) const {
    auto it = m_Viewports.find(id);
    const Camera* cam = it != m_Viewports.end() ? GetActiveCamera(it->second) : GetActiveCamera();
    return cam ? cam->GetViewMatrix() : glm::mat4(1.0f);
}

glm::mat4 Renderer::GetViewportProjectionMatrix(uint32_t id) const {
    auto it = m_Viewports.find(id);
    const Camera* cam = it != m_Viewports.end() ? GetActiveCamera(it->second) : GetActiveCamera();
    return cam ? cam->GetProjectionMatrix() : glm::mat4(1.0f);
}

std::vector<tri_mesh_range> Renderer::GetMeshRanges() const {
    std::vector<tri_mesh_range> ranges(m_MeshDrawInfo.size());
    for (size_t i = 0; i < ranges.size(); ++i)
        ranges[i] = {m_MeshDrawInfo[i].m_FirstIndex, m_MeshDrawInfo[i].m_IndexCount, m_MeshDrawInfo[i].m_BaseVertex,
                     m_MeshDrawInfo[i].m_MaterialIndex};
    if (m_HasSpriteGeometry)
        ranges.push_back({m_SpriteDrawInfo.m_FirstIndex, m_SpriteDrawInfo.m_IndexCount, m_SpriteDrawInfo.m_BaseVertex,
                          m_SpriteDrawInfo.m_MaterialIndex});
    return ranges;
}

bool Renderer::PrepareViewport(ViewportContext& vc) {
    uint32_t w = (uint32_t)std::max(vc.m_Info.Size.x, 0.0f), h = (uint32_t)std::max(vc.m_Info.Size.y, 0.0f);
    if (w == 0 || h == 0) return false;
    RenderExtent(vc, w, h);  // (smaller than the viewport while temporal upscaling is on for it)
    const bool multi = m_Devices.size() > 1;
    if ((vc.m_Ctx || vc.m_Group) && (vc.m_Width != w || vc.m_Height != h)) {  // CreateOrResizeOffscreenResources
        tri_destroy(vc.m_Ctx);
        tri_group_destroy(vc.m_Group);
        vc.m_Ctx = nullptr;
        vc.m_Group = nullptr;
        vc.m_HasImage = false;
    }
    if (!vc.m_Ctx && !vc.m_Group) {
        int rc;
        if (multi) {  // row bands on m_Devices, assembled on the first band's device
            if (h < m_Devices.size()) return false;
            tri_group_config gc{w, h, (uint32_t)m_Devices.size(), 0u, m_Devices.data(), m_RasterFlags, 0u};
            rc = tri_group_create(&gc, &vc.m_Group);
        } else {
            tri_config cfg{w, h, 0, 0, -1, m_RasterFlags};
            rc = tri_create(&cfg, &vc.m_Ctx);
        }
        if (rc != TRI_OK) {
            LogError("viewport target", tri_last_error());
            vc.m_Ctx = nullptr;
            vc.m_Group = nullptr;
            return false;
        }
        vc.m_Width = w;
        vc.m_Height = h;
        vc.m_GeometryGeneration = vc.m_TextureGeneration = vc.m_MaterialGeneration = vc.m_SkyboxGeneration = 0;
        vc.m_AiGeneration = 0;
        vc.m_Shadow = tri_shadow_config{};  // a fresh context starts without the pre-pass and bones
        vc.m_BonePalette.clear();
        vc.m_HasPosedSuffix = false;
        vc.m_IdOutput = vc.m_OutlineSet = false;  // ... and without the id output and the outline (SetTargetIds)
        vc.m_DrawEntities.clear();
        vc.m_MotionOutput = false;  // ... and without the motion output (SetTargetMotion)
    }
    const Target t{vc.m_Ctx, vc.m_Group};
    if (vc.m_GeometryGeneration != m_GeometryGeneration && multi) {
        std::vector<tri_geometry*> geos;
        if (!UploadSharedGeometry(geos)) return false;
        if (tri_group_bind_geometry(vc.m_Group, (uint32_t)geos.size(), geos.data()) != TRI_OK) {
            LogError("UploadMeshFromCache", tri_last_error());
            return false;
        }
        vc.m_GeometryGeneration = m_GeometryGeneration;
    }
    if (vc.m_GeometryGeneration != m_GeometryGeneration) {
        // one device copy of the concatenated buffers per generation, bound by every viewport
        if (!m_SharedGeometry && tri_geometry_create(-1, &m_SharedGeometry) != TRI_OK) {
            LogError("UploadMeshFromCache", tri_last_error());
            return false;
        }
        if (m_SharedGeometryGeneration != m_GeometryGeneration) {
            const std::vector<tri_mesh_range> ranges = GetMeshRanges();
            if (tri_geometry_upload(m_SharedGeometry, m_VertexBuffer.data(), m_VertexBuffer.size(), m_IndexBuffer.data(),
                                    m_IndexBuffer.size(), ranges.data(), (uint32_t)ranges.size()) != TRI_OK) {
                LogError("UploadMeshFromCache", tri_last_error());
                return false;
            }
            m_SharedGeometryGeneration = m_GeometryGeneration;
            ++m_GeometryUploads;
        }
        if (tri_bind_geometry(vc.m_Ctx, m_SharedGeometry) != TRI_OK) {
            LogError("UploadMeshFromCache", tri_last_error());
            return false;
        }
        vc.m_GeometryGeneration = m_GeometryGeneration;
    }
    if (vc.m_MaterialGeneration != m_MaterialGeneration) {  // BuildMaterialPayload (Renderer.cpp:5927-5951)
        std::vector<tri_material_record> recs;
        for (const Geometry::Material& m : m_Materials)
            recs.push_back({{m.BaseColorFactor.x, m.BaseColorFactor.y, m.BaseColorFactor.z, m.BaseColorFactor.w},
                            {m.MetallicFactor, m.RoughnessFactor, 1.0f, 0.0f}});
        if (t.Materials(recs.data(), (uint32_t)recs.size()) != TRI_OK) {
            LogError("material buffer", tri_last_error());
            return false;
        }
        vc.m_MaterialGeneration = m_MaterialGeneration;
    }
    if (vc.m_SkyboxGeneration != m_SkyboxGeneration) {
        const bool ok = m_SkyboxCubemap.IsValid();
        // format, size and the whole mip chain as loaded (CreateSkyboxCubemap, Renderer.cpp:3965-4097)
        tri_skybox_desc desc{};
        desc.format = (uint32_t)m_SkyboxCubemap.m_Format;
        desc.size = m_SkyboxCubemap.m_Width;
        desc.mip_count = m_SkyboxCubemap.m_MipCount;
        desc.texels = m_SkyboxCubemap.m_PixelData.data();
        desc.bytes = ok ? m_SkyboxCubemap.ChainBytes() : 0;
        if (t.Skybox(ok ? &desc : nullptr) != TRI_OK) {
            LogError("skybox cubemap", tri_last_error());
            return false;
        }
        vc.m_SkyboxGeneration = m_SkyboxGeneration;
    }
    vc.m_AiFrameDeferred = false;
    if (vc.m_AiGeneration != m_AiGeneration && m_AiFromDevice && m_AiWidth && vc.m_Ctx) {
        // a target that was not there when the output was consumed (new, resized): the tensor is still the generator's.
        // While the next job is rewriting it, the frame path does not wait: this target renders without the blend and
        // ConsumeAiOutput packs the next output into it. A generator that has lost the tensor with no job in flight (a
        // failed submit, a device error) ends the device blend for every target, as SubmitAiInterpolation(nullptr) does.
        if (m_FrameGenerator.HasJobInFlight()) {
            vc.m_AiFrameDeferred = true;
        } else if (!UploadAiFrameFromDevice(vc)) {
            LogError("AI frame generator", "the generated frame is gone: the blend is off until the next output");
            SubmitAiInterpolation(nullptr, 0, 0, 0);
        }
    }
    if (vc.m_AiGeneration != m_AiGeneration && !vc.m_AiFrameDeferred) {  // the AI frame texture (UploadAiInterpolationToGpu)
        if (t.AiFrame(m_AiWidth ? m_AiFrame.data() : nullptr, m_AiWidth, m_AiHeight) != TRI_OK) {
            LogError("AI frame texture", tri_last_error());
            return false;
        }
        vc.m_AiGeneration = m_AiGeneration;
    }
    if (vc.m_TextureGeneration != m_TextureGeneration) {
        for (size_t s = 0; s < m_TextureSlots.size(); ++s) {
            const Loader::TextureData& tex = m_TextureSlots[s].m_Data;
            if (t.Texture((uint32_t)s, tex.Pixels.data(), (uint32_t)tex.Width, (uint32_t)tex.Height) != TRI_OK) {
                LogError("texture slot", tri_last_error());
                return false;
            }
        }
        vc.m_TextureGeneration = m_TextureGeneration;
    }
    return true;
}

// The uniform block as one target gets it: without the blend while the target's texture waits for the generator's next
// output (PrepareViewport), or when an earlier pass of this frame found the generated frame gone.
tri_global_ubo Renderer::TargetUniforms(const ViewportContext& vc, const tri_global_ubo& ubo) const {
    tri_global_ubo out = ubo;
    if (vc.m_AiFrameDeferred || !HasAiFrame()) std::memset(out.ai_blend_config, 0, sizeof out.ai_blend_config);
    return out;
}

bool Renderer::BuildFrameInputs(uint32_t viewportId, tri_global_ubo& ubo, std::vector<tri_draw>& draws) {
    auto it = m_Viewports.find(viewportId);
    // viewport id 0 without a registered viewport 0: the legacy present pass when no viewport renders
    if (it == m_Viewports.end() && (viewportId != 0 || !m_Viewports.empty())) return false;
    GatherDraws();
    PrepareBonePaletteBuffer();
    UpdateUniformBuffer(it != m_Viewports.end() ? GetActiveCamera(it->second) : GetActiveCamera(), ubo);
    BuildDrawList(draws);
    return true;
}

bool Renderer::SubmitTarget(ViewportContext& vc, const tri_global_ubo& ubo, const std::vector<tri_draw>& draws,
                            const tri_shadow_config& shadow, bool shadowOn) {
    const Target t{vc.m_Ctx, vc.m_Group};
    if (std::memcmp(&vc.m_Shadow, &shadow, sizeof shadow) != 0) {  // pre-pass on / off / refitted
        if (t.Shadow(shadowOn ? &shadow : nullptr) != TRI_OK) {
            LogError("shadow map", tri_last_error());
            return false;
        }
        vc.m_Shadow = shadow;
    }
    if (vc.m_BonePalette != m_BonePalette) {  // the bone SSBO (binding 4) of this frame
        if (t.Bones(m_BonePalette.data(), (uint32_t)(m_BonePalette.size() / 16)) != TRI_OK) {
            LogError("bone palette", tri_last_error());
            return false;
        }
        vc.m_BonePalette = m_BonePalette;
        vc.m_HasPosedSuffix = false;  // (an upload drops the posed suffix)
        ++m_BonePaletteUploads;
    }
    if ((!m_PoseDraws.empty() || vc.m_HasPosedSuffix) && !SubmitPoses(vc)) {
        LogError("device poses", tri_last_error());
        return false;
    }
    const float clear[4] = {m_ClearColor.x, m_ClearColor.y, m_ClearColor.z, m_ClearColor.w};
    if (t.Frame(&ubo, clear) != TRI_OK || t.Draws(draws.data(), (uint32_t)draws.size()) != TRI_OK ||
        t.Render() != TRI_OK) {
        LogError("DrawFrame", tri_last_error());
        return false;
    }
    vc.m_HasImage = t.Output(&vc.m_Image) == TRI_OK;
    return true;
}

void Renderer::DrawFrame() {  // Renderer.cpp:733-837
    const auto t0 = std::chrono::steady_clock::now();
    if (!m_Initialised || m_Shutdown) return;
    // the fence (Renderer.cpp:752-772): the reference waits for the previous frame; with n frames in flight, for
    // frame k - n + 1, whose targets this frame is about to reuse
    const uint32_t inflight = m_Devices.size() > 1 ? 1u : m_FramesInFlight;
    while (m_Pending.size() >= inflight) FinishOldestFrame();
    const uint32_t tix = (uint32_t)(m_FrameCount++ % inflight);
    // the device tensor handed out by GetFrameReadbackDeviceTensor was valid until here: its slot serves again (an
    // unconsumed pending tensor moves from the slot's pinned buffer into host memory first)
    ReleaseHeldReadbackSlot(true);
    if (!m_PoseSets.empty() && m_PoseSetsGeneration != Animation::AnimationAssetService::Get().GetGeneration()) {
        FinishFrame();   // an asset was registered or replaced since the devices' sets were filled: no frame in flight
        DropPoseSets();  // may still pose from them, and they are filled again from what the service holds now
    }
    GatherDraws();
    PrepareBonePaletteBuffer();
    std::vector<tri_draw> draws;
    std::vector<ECS::Entity> drawEntities;
    BuildDrawList(draws, &drawEntities);
    tri_shadow_config shadow;
    const bool shadowOn = BuildShadowConfig(shadow);
    std::vector<ViewportContext*> submitted;
    tri_global_ubo lastUbo{};
    // RecordCommandBuffer's per-viewport render passes: the other viewports first, the primary one last
    // (Renderer.cpp:5208-5221), so the uniform block left bound is the primary viewport's
    ViewportContext* activeTarget = nullptr;
    ViewportContext* recorded = nullptr;
    ViewportContext* grabbed = nullptr;
    auto pass = [&](uint32_t id, ViewportContext& primary) {
        ViewportContext& vc = TargetOf(id, primary, tix);  // this frame's target of the viewport
        if (!PrepareViewport(vc)) return;
        tri_global_ubo ubo;
        UpdateUniformBuffer(GetActiveCamera(vc), ubo);
        if (!SetTargetText(vc, id)) LogError("DrawFrame", "the text overlay of this frame is missing");
        if (!SetTargetIds(vc, id, draws, drawEntities)) LogError("DrawFrame", "the entity ids of this frame are missing");
        // temporal anti-aliasing: the frame is rendered under this frame's jitter, the motion history keeps the
        // unjittered block and hands the previous projection on under the same jitter
        float jitter[2] = {0.0f, 0.0f};
        // (temporal upscaling, exclusive with it on a viewport: the same contract over the smaller render extent)
        const bool jittered = BeginTaaFrame(vc, id, jitter) || BeginUpscaleFrame(vc, id, jitter);
        if (!SetTargetMotion(vc, id, ubo, draws, drawEntities, jittered ? jitter : nullptr))
            LogError("DrawFrame", "the motion vectors of this frame are missing");
        tri_global_ubo shown = ubo;
        if (jittered && tri_taa_jitter_projection(ubo.projection, jitter[0], jitter[1], vc.m_Width, vc.m_Height, shown.projection) != TRI_OK)
            LogError("temporal anti-aliasing", tri_last_error());
        if (!SubmitTarget(vc, TargetUniforms(vc, shown), draws, shadow, shadowOn)) return;
        if (!ResolveTarget(vc, id, false)) LogError("DrawFrame", "the temporal anti-aliasing of this frame is missing");
        if (!UpscaleTarget(vc, id, false)) LogError("DrawFrame", "the temporal upscaling of this frame is missing");
        if (!ReprojectTarget(vc, id, false)) LogError("DrawFrame", "the history reprojection of this frame is missing");
        // recording: convert this frame on the device, behind its pass, into the slot of this frame in flight
        if (m_Recording && id == m_RecordingViewportId && CaptureRecordedFrame(vc, tix)) recorded = &vc;
        // AI readback: the active viewport's tensor, likewise, when the readback throttle has elapsed (ResolvePending-
        // Readback's interval, Renderer.cpp:1111-1140) and the viewport has the present extent (:5301-5337)
        // (the viewport's size: under temporal upscaling the context is smaller, and the tensor is its raw frame)
        const uint32_t viewW = (uint32_t)std::max(vc.m_Info.Size.x, 0.0f), viewH = (uint32_t)std::max(vc.m_Info.Size.y, 0.0f);
        if (m_AiReadback && id == m_ActiveViewportId && vc.m_Ctx &&
            !(m_PresentWidth && m_PresentHeight && (m_PresentWidth != viewW || m_PresentHeight != viewH))) {
            const auto now = std::chrono::steady_clock::now();
            if (now >= m_NextAiReadbackTime && CaptureReadbackFrame(vc, tix)) {
                m_NextAiReadbackTime = now + m_AiReadbackInterval;
                grabbed = &vc;
            }
        }
        lastUbo = ubo;
        submitted.push_back(&vc);
        m_LatestTarget[id] = tix;
        if (id == m_ActiveViewportId) activeTarget = &vc;
    };
    for (auto& it : m_Viewports)
        if (it.first != m_ActiveViewportId) pass(it.first, it.second);
    auto active = m_Viewports.find(m_ActiveViewportId);
    if (active != m_Viewports.end()) pass(active->first, active->second);
    const bool primaryActive = activeTarget != nullptr;
    // Legacy direct-to-swapchain path (Renderer.cpp:5233, :5498-5590): without a rendered primary viewport
    // the skybox, the meshes and the sprites go straight into the present image at the swapchain extent,
    // cleared to the clear colour, with the uniform block last recorded: the null-camera update
    // (GetActiveCamera()) when no viewport rendered (:5223-5226), else the last viewport pass's.
    // the queue lasts one frame (TextRenderer::BeginFrame): text for ids that rendered no pass is dropped
    m_TextRenderer.BeginFrame();
    ViewportContext* legacy = nullptr;
    if (!primaryActive && m_PresentWidth && m_PresentHeight) {
        m_LegacyTarget.m_Info.Size = glm::vec2((float)m_PresentWidth, (float)m_PresentHeight);
        m_LegacyTarget.m_Info.ViewportID = 0;
        if (PrepareViewport(m_LegacyTarget)) {
            tri_global_ubo ubo = lastUbo;
            if (submitted.empty()) UpdateUniformBuffer(GetActiveCamera(), ubo);
            if (SubmitTarget(m_LegacyTarget, TargetUniforms(m_LegacyTarget, ubo), draws, shadow, shadowOn)) {
                legacy = &m_LegacyTarget;
                submitted.push_back(legacy);
            }
        }
    }
    // Primary viewport -> swapchain image, VK_FILTER_LINEAR (Renderer.cpp:5346-5361), stream-ordered behind its pass.
    PendingFrame pf;
    pf.m_Targets = submitted;
    pf.m_Legacy = legacy;
    pf.m_Recorded = recorded;
    pf.m_RecordSlot = tix;
    pf.m_Grabbed = grabbed;
    pf.m_GrabGeneration = m_GrabGeneration;
    if (primaryActive && m_PresentWidth && m_PresentHeight) {
        if (PresentBlit(*activeTarget, m_PresentWidth, m_PresentHeight) == TRI_OK) {
            pf.m_Blit = activeTarget;
            pf.m_BlitWidth = m_PresentWidth;
            pf.m_BlitHeight = m_PresentHeight;
        } else {
            LogError("present blit", tri_last_error());
        }
    }
    m_Pending.push_back(std::move(pf));
    // no wait here: the next DrawFrame (or a reader) fences this frame, as the reference fences the previous
    // frame's timeline value at the start of DrawFrame (Renderer.cpp:752-772)
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    RecordFrameTiming(ms);
}

void Renderer::FinishFrame() {  // every frame in flight
    while (!m_Pending.empty()) FinishOldestFrame();
}

void Renderer::FinishOldestFrame() {  // the frame fence (Renderer.cpp:744-772)
    if (m_Pending.empty()) return;
    PendingFrame p = std::move(m_Pending.front());
    m_Pending.pop_front();
    // this frame's present replaces the previous one (none if it failed)
    m_PresentSource = nullptr;
    m_PresentGroup = nullptr;
    m_PresentLegacy = false;
    m_PresentedWidth = m_PresentedHeight = 0;
    // A frame that outgrew the bin/clip queues has grown them inside tri_synchronize and is re-rendered (and its
    // present blit redone), so a presented frame is always complete.
    for (ViewportContext* vc : p.m_Targets) {
        const Target t{vc->m_Ctx, vc->m_Group};
        int rc = t.Sync();
        bool rerendered = false;
        for (int retry = 0; rc == TRI_E_OVERFLOW && retry < 3; ++retry) {
            rc = t.Render();
            if (rc == TRI_OK) rc = t.Sync();
            rerendered = true;
        }
        if (rc != TRI_OK) LogError("frame fence", tri_last_error());
        if (rc == TRI_OK && rerendered) {  // the passes behind the first render read an incomplete frame
            RedoTemporal(m_Taa, *vc, &Renderer::ResolveTarget, tri_taa_reset, "temporal anti-aliasing");
            RedoTemporal(m_Upscale, *vc, &Renderer::UpscaleTarget, tri_upscale_reset, "temporal upscaling");
            RedoTemporal(m_Reprojection, *vc, &Renderer::ReprojectTarget, tri_history_reset, "history reprojection");
        }
        if (rc == TRI_OK) vc->m_HasImage = t.Output(&vc->m_Image) == TRI_OK;  // a re-render moves a group's buffer
        if (vc == p.m_Legacy && rc == TRI_OK) {
            m_PresentSource = vc->m_Ctx;
            m_PresentGroup = vc->m_Group;
            m_PresentLegacy = true;
            m_PresentedWidth = (uint32_t)vc->m_Info.Size.x;  // the target PrepareViewport sized
            m_PresentedHeight = (uint32_t)vc->m_Info.Size.y;
        }
        if (vc == p.m_Recorded && m_Recorder) {  // this frame's FRAME record, in submission order
            // a re-rendered frame was captured incomplete: convert it again (as the present blit is redone below)
            bool ok = rc == TRI_OK;
            if (ok && rerendered)
                ok = tri_recorder_release(m_Recorder, p.m_RecordSlot) == TRI_OK && CaptureRecordedFrame(*vc, p.m_RecordSlot);
            const uint8_t* product = nullptr;
            uint64_t bytes = 0;
            if (ok && tri_recorder_wait_ex(m_Recorder, p.m_RecordSlot, &product, &bytes) != TRI_OK) {
                LogError("recording", tri_last_error());
                ok = false;
            }
            if (ok && !(m_RecordingJpeg ? m_VideoEncoder.SubmitJpeg(product, bytes, m_RecordingWidth, m_RecordingHeight)
                                        : m_VideoEncoder.SubmitPlanes(product, m_RecordingWidth, m_RecordingHeight)))
                LogError("recording", "the encoder refused a frame");
            if (tri_recorder_release(m_Recorder, p.m_RecordSlot) != TRI_OK) LogError("recording", tri_last_error());
        }
        if (vc == p.m_Grabbed && m_Grab && p.m_GrabGeneration == m_GrabGeneration)
            ResolveReadbackFrame(*vc, p.m_RecordSlot, rc == TRI_OK, rerendered);
        if (vc == p.m_Blit && rc != TRI_OK) p.m_Blit = nullptr;
        if (vc == p.m_Blit && rerendered) {  // (the first wait covered the blit behind the pass: same stream)
            if (PresentBlit(*vc, p.m_BlitWidth, p.m_BlitHeight) != TRI_OK || t.Sync() != TRI_OK) {
                LogError("present blit", tri_last_error());
                p.m_Blit = nullptr;
            }
        }
    }
    if (p.m_Blit) {
        m_PresentSource = p.m_Blit->m_Ctx;
        m_PresentGroup = p.m_Blit->m_Group;
        m_PresentedWidth = p.m_BlitWidth;  // the blit's destination extent
        m_PresentedHeight = p.m_BlitHeight;
    }
    ProcessAiFrame();  // (Renderer.cpp:789: after the readback has resolved)
}

// Renderer.cpp:6171-6284. The session starts before anything is resized, so a refused start changes nothing.
bool Renderer::SetViewportRecordingEnabled(bool enabled, uint32_t viewportId, uint32_t width, uint32_t height,
                                           const std::string& outputPath) {
    StopRecording();  // disabling, or a restart: the running file gets its frames in flight and is finalised
    if (!enabled) return true;
    if (m_Devices.size() > 1) {
        LogError("viewport recording", "multi-device viewports (SetDeviceCount > 1) are not recorded");
        return false;
    }
    if (IsTemporalUpscalingEnabled(viewportId)) {  // (its context has the render extent, a session one fixed extent)
        LogError("viewport recording", "the viewport has temporal upscaling on (SetTemporalUpscalingEnabled): not recorded");
        return false;
    }
    const uint32_t w = width + (width & 1u), h = height + (height & 1u);  // even planes, as the reference rounds
    if (w != width || h != height) {
        char msg[128];
        std::snprintf(msg, sizeof msg, "extent %ux%u adjusted to %ux%u (even dimensions)", width, height, w, h);
        LogError("viewport recording", msg);
    }
    if (w > TRI_MAX_DIM || h > TRI_MAX_DIM) {
        LogError("viewport recording", "extent beyond the framebuffer limit");
        return false;
    }
    m_VideoEncoder.SetQuality(m_RecordingQuality);
    if (!m_VideoEncoder.BeginSession(outputPath, w, h, 1) || !m_VideoEncoder.IsSessionActive()) {
        LogError("viewport recording", "the video encoder did not start a session");
        return false;
    }
    FinishFrame();  // the recorded viewport's targets are about to be resized
    m_Recording = true;
    m_RecordingViewportId = viewportId;
    m_RecordingWidth = w;
    m_RecordingHeight = h;
    m_RecordingPath = outputPath;
    m_RecordingJpeg = outputPath.size() >= 4 && std::tolower((unsigned char)outputPath[outputPath.size() - 3]) == 'm' &&
                      std::tolower((unsigned char)outputPath[outputPath.size() - 2]) == 'k' &&
                      std::tolower((unsigned char)outputPath[outputPath.size() - 1]) == 'v' &&
                      outputPath[outputPath.size() - 4] == '.';  // (the encoder accepted the name: .y4m or .mkv)
    auto it = m_Viewports.find(viewportId);  // (a viewport registered later is pinned by SetViewport)
    if (it != m_Viewports.end()) it->second.m_Info.Size = glm::vec2((float)w, (float)h);
    tri_recorder_destroy(m_Recorder);  // a recorder of the previous extent
    m_Recorder = nullptr;
    return true;
}

void Renderer::StopRecording() {
    if (!m_Recording) return;
    FinishFrame();
    m_Recording = false;
    if (m_VideoEncoder.IsSessionActive() && !m_VideoEncoder.EndSession())
        LogError("viewport recording", ("could not finalise " + m_RecordingPath).c_str());
    tri_recorder_destroy(m_Recorder);
    m_Recorder = nullptr;
}

// The recorded viewport's frame -> recorder slot `slot` (asynchronous). The recorder is made here, once the target
// exists: one slot per frame in flight, on the target's device.
bool Renderer::CaptureRecordedFrame(ViewportContext& vc, uint32_t slot) {
    if (!vc.m_Ctx || !vc.m_HasImage) return false;  // (multi-device viewports are refused when recording starts)
    if (vc.m_Width != m_RecordingWidth || vc.m_Height != m_RecordingHeight) {
        LogError("recording", "the viewport target does not have the recording extent");
        return false;
    }
    if (!m_Recorder) {  // (SetFramesInFlight drops it with the targets, so its slots always match)
        const tri_record_params params{m_RecordingJpeg ? TRI_RECORD_JPEG420 : TRI_RECORD_YUV444, m_VideoEncoder.GetQuality(),
                                       m_VideoEncoder.GetRestartInterval(), 0};
        if (tri_recorder_create_ex(vc.m_Image.device, m_RecordingWidth, m_RecordingHeight, m_FramesInFlight, &params,
                                   &m_Recorder) != TRI_OK) {
            LogError("recording", tri_last_error());
            return false;
        }
    }
    if (tri_recorder_capture(m_Recorder, slot, vc.m_Ctx) != TRI_OK) {
        LogError("recording", tri_last_error());
        return false;
    }
    return true;
}

// ---- AI readback and dataset capture ---------------------------------------------------------------------------

namespace {

// ParseTensorShapeNhwc + BuildCanonicalNhwcShape (Renderer.cpp:269-327): {1, H, W, C} of a rank-3 (HWC) or rank-4
// (NHWC) shape, a dimension <= 0 (dynamic) replaced by the fallback.
bool CanonicalNhwcShape(const int64_t* shape, size_t rank, uint32_t fallbackWidth, uint32_t fallbackHeight,
                        uint32_t fallbackChannels, int64_t (&out)[4]) {
    if (!shape || (rank != 3 && rank != 4)) return false;
    const int64_t* hwc = shape + (rank == 4 ? 1 : 0);
    auto resolve = [](int64_t v, int64_t fallback) { return std::max<int64_t>(v <= 0 ? fallback : v, 0); };
    out[0] = 1;
    out[1] = resolve(hwc[0], (int64_t)fallbackHeight);
    out[2] = resolve(hwc[1], (int64_t)fallbackWidth);
    out[3] = resolve(hwc[2], (int64_t)fallbackChannels);
    return true;
}

}  // namespace

// Renderer.cpp:358-415, in its order: scale, swap, clamp.
void Renderer::NormaliseAndReorderAiOutput(std::vector<float>& data, int64_t channels) {
    if (data.empty()) return;
    if (channels <= 0) {
        LogError("AI output", "invalid channel count");
        return;
    }
    const size_t ch = (size_t)channels;
    if (data.size() % ch != 0) {
        LogError("AI output", "the element count is no multiple of the channel count");
        return;
    }
    const auto mm = std::minmax_element(data.begin(), data.end());
    const float lo = *mm.first, hi = *mm.second;
    constexpr float kTolerance = 1.0e-3f;
    if (hi > 1.0f + kTolerance || lo < -kTolerance) {
        const float scale = 1.0f / 255.0f;
        for (float& v : data) v *= scale;
    }
    if (ch >= 3)
        for (size_t p = 0; p < data.size(); p += ch) std::swap(data[p], data[p + 2]);
    for (float& v : data) v = std::min(std::max(v, 0.0f), 1.0f);
}

bool Renderer::SetAiReadbackEnabled(bool enabled) {
    if (enabled && m_Devices.size() > 1) {
        LogError("AI readback", "multi-device viewports (SetDeviceCount > 1) have no AI readback");
        return false;
    }
    if (enabled == m_AiReadback) return true;
    if (!enabled) {  // the captures in flight are dropped with the grab
        FinishFrame();
        DropGrab();
        m_PendingFrameReadback.clear();
    }
    m_AiReadback = enabled;
    return true;
}

void Renderer::SetAiThrottleIntervals(uint32_t readbackMs, uint32_t inferenceMs) {
    m_AiReadbackInterval = std::chrono::milliseconds(readbackMs);
    m_AiInferenceInterval = std::chrono::milliseconds(inferenceMs);
    m_NextAiReadbackTime = m_NextAiInferenceTime = std::chrono::steady_clock::time_point{};  // both elapse at once
}

void Renderer::DropGrab() {
    ReleaseHeldReadbackSlot(true);
    tri_framegrab_destroy(m_Grab);  // (waits for its captures)
    m_Grab = nullptr;
    ++m_GrabGeneration;
}

// The slot that holds the latest resolved tensor goes back to the grab. While it was held, the pending readback lived
// in its pinned buffer (no copy unless it is needed): `keepPending` copies an unconsumed one into m_PendingFrameReadback.
void Renderer::ReleaseHeldReadbackSlot(bool keepPending) {
    if (m_PendingInSlot && keepPending && m_GrabHostTensor)
        m_PendingFrameReadback.assign(m_GrabHostTensor, m_GrabHostTensor + FrameReadbackCount());
    m_PendingInSlot = false;
    if (m_Grab && m_GrabHeldSlot >= 0 && tri_framegrab_release(m_Grab, (uint32_t)m_GrabHeldSlot) != TRI_OK)
        LogError("AI readback", tri_last_error());
    m_GrabHeldSlot = -1;
    m_GrabDeviceTensor = nullptr;
    m_GrabHostTensor = nullptr;
    m_GrabHeldCtx = nullptr;
}

// The active viewport's frame -> grab slot `slot` (asynchronous). The grab is made here, once the target exists: one
// slot per frame in flight, on the target's device, with pinned host copies; a target of another extent (the viewport
// was resized) gets a new grab.
bool Renderer::CaptureReadbackFrame(ViewportContext& vc, uint32_t slot) {
    if (!vc.m_Ctx || !vc.m_HasImage) return false;
    if (m_Grab && (m_GrabWidth != vc.m_Width || m_GrabHeight != vc.m_Height)) DropGrab();
    if (!m_Grab) {  // (SetFramesInFlight drops it with the targets, so its slots always match)
        if (tri_framegrab_create(vc.m_Image.device, vc.m_Width, vc.m_Height, m_FramesInFlight, TRI_GRAB_HOST_COPY,
                                 &m_Grab) != TRI_OK) {
            LogError("AI readback", tri_last_error());
            m_Grab = nullptr;
            return false;
        }
        m_GrabWidth = vc.m_Width;
        m_GrabDevice = vc.m_Image.device;
        m_GrabHeight = vc.m_Height;
    }
    if (tri_framegrab_capture(m_Grab, slot, vc.m_Ctx) != TRI_OK) {
        LogError("AI readback", tri_last_error());
        return false;
    }
    return true;
}

// After the frame's fence: the slot's floats become the pending readback (a newer frame replaces an unconsumed one),
// and the slot stays busy until the next DrawFrame, so that its device tensor can be handed out and its pinned buffer
// can serve TryAcquireRenderedFrame without a copy in between.
void Renderer::ResolveReadbackFrame(ViewportContext& vc, uint32_t slot, bool ok, bool rerendered) {
    // a re-rendered frame was captured incomplete: convert it again
    if (ok && rerendered) ok = tri_framegrab_release(m_Grab, slot) == TRI_OK && CaptureReadbackFrame(vc, slot);
    const float* host = nullptr;
    const float* device = nullptr;
    if (ok && tri_framegrab_wait(m_Grab, slot, &host, &device) != TRI_OK) {
        LogError("AI readback", tri_last_error());
        ok = false;
    }
    if (!ok) {  // the tensor pending so far stays
        if (tri_framegrab_release(m_Grab, slot) != TRI_OK) LogError("AI readback", tri_last_error());
        return;
    }
    ReleaseHeldReadbackSlot(false);  // (an older frame's slot: this frame replaces what it held)
    m_PendingFrameReadback.clear();
    m_FrameReadbackWidth = m_GrabWidth;
    m_FrameReadbackHeight = m_GrabHeight;
    m_GrabHeldSlot = (int32_t)slot;
    m_GrabDeviceTensor = device;
    m_GrabHostTensor = host;
    m_GrabHeldCtx = vc.m_Ctx;
    m_PendingInSlot = true;
}

bool Renderer::TryAcquireRenderedFrame(std::vector<float>& out) {
    if (!m_PendingInSlot && m_PendingFrameReadback.empty()) {
        AiInferenceThrottleElapsed();  // (the reference arms the throttle before it looks for a frame, :933-943)
        return false;
    }
    out.resize(FrameReadbackCount());  // (a vector the caller reuses is not allocated again)
    return TryAcquireRenderedFrame(out.data(), out.size());
}

bool Renderer::AiInferenceThrottleElapsed() {  // Renderer.cpp:933-940
    const auto now = std::chrono::steady_clock::now();
    if (now < m_NextAiInferenceTime) return false;
    m_NextAiInferenceTime = now + m_AiInferenceInterval;
    return true;
}

bool Renderer::TryAcquireRenderedFrame(float* out, size_t capacity) {
    const size_t n = FrameReadbackCount();
    const bool pending = m_PendingInSlot || !m_PendingFrameReadback.empty();
    if (pending && (!out || capacity < n)) return false;  // (it stays pending, and the throttle is not armed)
    if (!AiInferenceThrottleElapsed() || !pending) return false;
    std::memcpy(out, m_PendingInSlot ? m_GrabHostTensor : m_PendingFrameReadback.data(), n * sizeof(float));
    m_PendingInSlot = false;
    m_PendingFrameReadback.clear();
    if (m_FrameDatasetCaptureEnabled) {  // the exact tensor the generator gets (:973-977)
        const int64_t shape[4] = {1, (int64_t)m_FrameReadbackHeight, (int64_t)m_FrameReadbackWidth,
                                  (int64_t)s_FrameReadbackChannelCount};
        m_FrameDatasetRecorder.RecordInputFrame(out, n, m_FrameReadbackWidth, m_FrameReadbackHeight,
                                                s_FrameReadbackChannelCount, shape, 4);
    }
    return true;
}

bool Renderer::GetFrameReadbackDeviceTensor(const float** device, uint32_t& width, uint32_t& height) {
    FinishFrame();  // (on demand, as the other readers: the latest frame's capture is resolved)
    if (!device || !m_Grab || m_GrabHeldSlot < 0 || !m_GrabDeviceTensor) return false;
    *device = m_GrabDeviceTensor;
    width = m_GrabWidth;
    height = m_GrabHeight;
    return true;
}

bool Renderer::SubmitAiOutput(const float* data, size_t count, const int64_t* shape, size_t rank) {
    int64_t canonical[4];
    if (!CanonicalNhwcShape(shape, rank, m_FrameReadbackWidth, m_FrameReadbackHeight, s_FrameReadbackChannelCount, canonical)) {
        LogError("AI output", "the tensor must be channels-last: [height, width, channels] or [1, height, width, channels]");
        return false;
    }
    if (!data || count == 0) return false;  // (TryConsumeOutput's empty output, Renderer.cpp:915)
    std::vector<float> output(data, data + count);
    NormaliseAndReorderAiOutput(output, canonical[3]);
    if (m_FrameDatasetCaptureEnabled) m_FrameDatasetRecorder.RecordAiOutput(output.data(), output.size(), canonical, 4);
    if ((uint64_t)canonical[1] * (uint64_t)canonical[2] * (uint64_t)canonical[3] != (uint64_t)count ||
        canonical[1] > (int64_t)UINT32_MAX || canonical[2] > (int64_t)UINT32_MAX || canonical[3] > (int64_t)UINT32_MAX) {
        LogError("AI output", "the element count does not match the shape: the blend frame is unchanged");
        return false;
    }
    return SubmitAiInterpolation(output.data(), (uint32_t)canonical[2], (uint32_t)canonical[1], (uint32_t)canonical[3]);
}

// Renderer.cpp:1743-1782, with the container's extension.
std::string Renderer::ResolveAiModelPath() const {
    namespace fs = std::filesystem;
    std::error_code ec;
    const char* env = std::getenv("TRIDENT_AI_MODEL");
    if (env && *env) {
        const fs::path candidate{env};
        if (fs::exists(candidate, ec)) return fs::absolute(candidate, ec).string();
        LogError("TRIDENT_AI_MODEL names a file that does not exist; trying the default search paths", env);
    }
    const fs::path cwd = fs::current_path(ec);
    if (ec) return {};
    for (const fs::path& root : {cwd, cwd.parent_path(), cwd.parent_path().parent_path()}) {
        if (root.empty()) continue;
        const fs::path candidate = root / "Assets" / "AI" / "frame_generator.trifgen";
        if (fs::exists(candidate, ec)) return fs::absolute(candidate, ec).string();
    }
    return {};
}

bool Renderer::TryInitialiseAiModel() {  // Renderer.cpp:1077-1108
    const std::string path = ResolveAiModelPath();
    if (path.empty()) {
        if (!m_AiModelMissingWarningIssued) {
            LogError("AI frame generator", "no model found: rendering continues without AI augmentation until one is provided");
            m_AiModelMissingWarningIssued = true;
            m_AiModelInitialiseWarningIssued = false;
        }
        return false;
    }
    if (LoadAiModel(path)) {
        m_AiModelMissingWarningIssued = m_AiModelInitialiseWarningIssued = false;
        return true;
    }
    if (!m_AiModelInitialiseWarningIssued) {
        LogError("AI frame generator failed to initialise; frames skip AI processing until a valid model is supplied",
                 (path + ": " + m_FrameGenerator.GetLastError()).c_str());
        m_AiModelInitialiseWarningIssued = true;
    }
    return false;
}

bool Renderer::LoadAiModel(const std::string& path) {
    if (m_Devices.size() > 1) {
        LogError("AI frame generator", "multi-device viewports (SetDeviceCount > 1) have no frame generator");
        return false;
    }
    // a file that is refused leaves the running model, its job in flight and its output alone; one that is accepted
    // waits for that job and drops it with the old generator (FrameGenerator::Initialise)
    if (!m_FrameGenerator.Initialise(path)) return false;
    if (m_AiFromDevice) SubmitAiInterpolation(nullptr, 0, 0, 0);  // the old model's tensor went with it
    m_AiShapeWarningIssued = false;
    return SetAiReadbackEnabled(true);  // l_ReadbackRequired (Renderer.cpp:787)
}

void Renderer::RefreshAiDebugStats() {
    m_AiDebugStats.m_ModelInitialised = m_FrameGenerator.IsInitialised();
    m_AiDebugStats.m_BlendStrength = m_AiBlendStrength;
    m_AiDebugStats.m_TextureReady = HasAiFrame();
    m_AiDebugStats.m_TextureExtent.width = m_AiWidth;
    m_AiDebugStats.m_TextureExtent.height = m_AiHeight;
    m_AiDebugStats.m_PendingJobCount = m_FrameGenerator.GetPendingJobCount();
    m_AiDebugStats.m_CompletedInferenceCount = m_FrameGenerator.GetCompletedInferenceCount();
    m_AiDebugStats.m_LastInferenceMilliseconds = m_FrameGenerator.GetLastInferenceMilliseconds();
    m_AiDebugStats.m_AverageInferenceMilliseconds = m_FrameGenerator.GetAverageInferenceMilliseconds();
}

template <typename F>
void Renderer::ForEachTarget(F&& f) {
    for (auto& it : m_Viewports) f(it.second);
    for (auto& it : m_RingTargets)
        for (ViewportContext& vc : it.second) f(vc);
    f(m_LegacyTarget);
}

bool Renderer::UploadAiFrameFromDevice(ViewportContext& vc) {
    const float* tensor = nullptr;
    uint32_t w = 0, h = 0;
    if (!vc.m_Ctx || !m_FrameGenerator.GetOutputDevice(&tensor, w, h)) return false;
    if (tri_upload_ai_frame_device(vc.m_Ctx, tensor, w, h, 3, m_FrameGenerator.GetHandle()) != TRI_OK) return false;
    vc.m_AiGeneration = m_AiGeneration;
    return true;
}

// A finished output becomes the blend frame: packed on the device into every single-device target there is, on the
// target's own stream behind the frames it has queued (a target made later fetches it in PrepareViewport).
void Renderer::ConsumeAiOutput() {
    const float* tensor = nullptr;
    uint32_t w = 0, h = 0;
    if (!m_FrameGenerator.GetOutputDevice(&tensor, w, h)) return;
    ++m_AiGeneration;
    m_AiFrame.clear();
    m_AiWidth = w;
    m_AiHeight = h;
    m_AiFromDevice = true;
    ForEachTarget([&](ViewportContext& vc) {
        if (vc.m_Ctx && !UploadAiFrameFromDevice(vc)) LogError("AI frame texture", tri_last_error());
    });
    if (m_FrameDatasetCaptureEnabled) {  // the normalised tensor, as SubmitAiOutput records it (Renderer.cpp:917-924)
        std::vector<float> output;
        if (m_FrameGenerator.ReadOutput(output)) {
            NormaliseAndReorderAiOutput(output, 3);
            const int64_t shape[4] = {1, (int64_t)h, (int64_t)w, 3};
            m_FrameDatasetRecorder.RecordAiOutput(output.data(), output.size(), shape, 4);
        } else {
            LogError("AI output", tri_last_error());
        }
    }
    RefreshAiDebugStats();
}

void Renderer::ProcessAiFrame() {  // Renderer.cpp:839-982
    if (!m_FrameGenerator.IsInitialised()) {
        m_AiDebugStats.m_ModelInitialised = false;
        m_AiDebugStats.m_BlendStrength = m_AiBlendStrength;
        m_AiDebugStats.m_TextureReady = HasAiFrame();
        m_AiDebugStats.m_TextureExtent.width = m_AiWidth;
        m_AiDebugStats.m_TextureExtent.height = m_AiHeight;
        const auto now = std::chrono::steady_clock::now();
        if (now >= m_AiNextModelSearchTime) {  // a model dropped on disk starts the AI path without a restart
            TryInitialiseAiModel();
            m_AiNextModelSearchTime = now + s_AiModelSearchInterval;
        }
        if (!m_FrameGenerator.IsInitialised()) {
            m_AiDebugStats.m_PendingJobCount = 0;
            m_AiDebugStats.m_CompletedInferenceCount = 0;
            m_AiDebugStats.m_LastInferenceMilliseconds = m_AiDebugStats.m_AverageInferenceMilliseconds = 0.0;
        } else {
            RefreshAiDebugStats();
        }
        return;
    }
    // (1) a finished output first, so that the blend reacts at once
    if (m_FrameGenerator.TryConsumeOutput()) ConsumeAiOutput();
    RefreshAiDebugStats();
    // (2) one job at a time: while one is in flight the held tensor stays pending and the throttle is not armed
    if (m_FrameGenerator.HasJobInFlight()) return;
    if (!AiInferenceThrottleElapsed()) return;
    if (!m_PendingInSlot || !m_GrabDeviceTensor || !m_GrabHeldCtx) return;  // no fresh tensor: the last output stays
    m_PendingInSlot = false;  // acquired (TryAcquireRenderedFrame, :943)
    const size_t expected = (size_t)m_FrameReadbackWidth * m_FrameReadbackHeight * m_FrameGenerator.GetInputChannels();
    if (FrameReadbackCount() != expected) {  // :957-963
        if (!m_AiShapeWarningIssued) {
            const std::string msg = "the frame has " + std::to_string(FrameReadbackCount()) + " elements, the model expects " +
                                    std::to_string(expected) + ": inference is skipped";
            LogError("AI frame generator", msg.c_str());
            m_AiShapeWarningIssued = true;
        }
        return;
    }
    void* stream = nullptr;
    if (tri_get_stream(m_GrabHeldCtx, &stream) != TRI_OK) return;
    // (3) the tensor where the grab made it; the copy is ordered on the stream that made it, so the slot may serve again
    if (!m_FrameGenerator.ProcessFrame(m_GrabDevice, m_GrabDeviceTensor, m_FrameReadbackWidth, m_FrameReadbackHeight,
                                       s_FrameReadbackChannelCount, stream)) {
        if (!m_AiShapeWarningIssued) {
            LogError("AI frame generator rejected the frame; the previous output stays", m_FrameGenerator.GetLastError().c_str());
            m_AiShapeWarningIssued = true;
        }
        RefreshAiDebugStats();
        return;
    }
    if (m_FrameDatasetCaptureEnabled && m_GrabHostTensor) {  // the exact tensor the generator got (:973-977)
        const int64_t shape[4] = {1, (int64_t)m_FrameReadbackHeight, (int64_t)m_FrameReadbackWidth,
                                  (int64_t)s_FrameReadbackChannelCount};
        m_FrameDatasetRecorder.RecordInputFrame(m_GrabHostTensor, FrameReadbackCount(), m_FrameReadbackWidth,
                                                m_FrameReadbackHeight, s_FrameReadbackChannelCount, shape, 4);
    }
    RefreshAiDebugStats();
}

bool Renderer::FinishAiInference(uint32_t timeoutMs) {
    if (!m_FrameGenerator.HasJobInFlight()) return true;
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeoutMs);
    for (;;) {
        if (m_FrameGenerator.TryConsumeOutput()) {
            ConsumeAiOutput();
            return true;
        }
        if (!m_FrameGenerator.HasJobInFlight()) {  // a device error lost the job
            RefreshAiDebugStats();
            return false;
        }
        if (std::chrono::steady_clock::now() >= deadline) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

bool Renderer::ReadAiBlendFrame(std::vector<uint8_t>& rgba, uint32_t& width, uint32_t& height) {
    FinishFrame();
    const ViewportContext* vc = LatestTarget(m_ActiveViewportId);
    if (!vc || !vc->m_Ctx || !HasAiFrame() || vc->m_AiGeneration != m_AiGeneration) return false;
    rgba.resize((size_t)m_AiWidth * m_AiHeight * 4);
    if (tri_read_ai_frame(vc->m_Ctx, rgba.data()) != TRI_OK) {
        LogError("AI frame texture", tri_last_error());
        return false;
    }
    width = m_AiWidth;
    height = m_AiHeight;
    return true;
}

void Renderer::SetFrameDatasetCaptureEnabled(bool enabled) {
    m_FrameDatasetCaptureEnabled = enabled;
    SyncFrameDatasetRecorder();
}

void Renderer::SetFrameDatasetCaptureDirectory(const std::string& directory) {
    m_FrameDatasetCaptureDirectory = directory.empty() ? DefaultDatasetDirectory() : directory;
    SyncFrameDatasetRecorder();
}

void Renderer::SetFrameDatasetCaptureInterval(uint32_t interval) {
    m_FrameDatasetCaptureInterval = std::max<uint32_t>(1u, interval);
    m_FrameDatasetRecorder.SetSampleInterval(m_FrameDatasetCaptureInterval);
}

void Renderer::SyncFrameDatasetRecorder() {  // Renderer.cpp:6393-6398
    m_FrameDatasetRecorder.SetCaptureDirectory(m_FrameDatasetCaptureDirectory);
    m_FrameDatasetRecorder.SetSampleInterval(m_FrameDatasetCaptureInterval);
    m_FrameDatasetRecorder.EnableCapture(m_FrameDatasetCaptureEnabled);
}

void Renderer::RecordFrameTiming(double ms) {  // Renderer.cpp:6286-6343
    if (m_PerformanceHistory.empty()) return;
    FrameTimingSample s;
    s.FrameMilliseconds = ms;
    s.FramesPerSecond = ms > 0.0 ? 1000.0 / ms : 0.0;
    s.CaptureTime = std::chrono::system_clock::now();
    m_PerformanceHistory[m_PerformanceHistoryNextIndex] = s;
    m_PerformanceHistoryNextIndex = (m_PerformanceHistoryNextIndex + 1) % m_PerformanceHistory.size();
    m_PerformanceSampleCount = std::min(m_PerformanceSampleCount + 1, m_PerformanceHistory.size());
    FrameTimingStats st;
    st.MinimumMilliseconds = std::numeric_limits<double>::max();
    st.MinimumFPS = std::numeric_limits<double>::max();
    double sumMs = 0.0, sumFps = 0.0;
    for (size_t i = 0; i < m_PerformanceSampleCount; ++i) {
        const FrameTimingSample& x = m_PerformanceHistory[i];
        st.MinimumMilliseconds = std::min(st.MinimumMilliseconds, x.FrameMilliseconds);
        st.MaximumMilliseconds = std::max(st.MaximumMilliseconds, x.FrameMilliseconds);
        st.MinimumFPS = std::min(st.MinimumFPS, x.FramesPerSecond);
        st.MaximumFPS = std::max(st.MaximumFPS, x.FramesPerSecond);
        sumMs += x.FrameMilliseconds;
        sumFps += x.FramesPerSecond;
    }
    st.AverageMilliseconds = sumMs / (double)m_PerformanceSampleCount;
    st.AverageFPS = sumFps / (double)m_PerformanceSampleCount;
    m_PerformanceStats = st;
}

// ---- entity ids ---------------------------------------------------------------------------------------------------
void Renderer::SetEntityIdOutputEnabled(uint32_t viewportId, bool enabled) { m_IdOutputViewports[viewportId] = enabled; }

void Renderer::SetSelectionOutline(bool enabled, const glm::vec4& colour, uint32_t widthPx) {
    if (enabled && m_Devices.size() > 1) {
        LogError("selection outline", "multi-device viewports (SetDeviceCount > 1) draw no outline: a band's halo lies in another band");
        m_SelectionOutline = false;
        return;
    }
    if (enabled && (widthPx < 1 || widthPx > 8)) {
        LogError("selection outline", "the width must be 1..8 pixels");
        return;
    }
    m_SelectionOutline = enabled;
    if (enabled) {
        m_OutlineColour = colour;
        m_OutlineWidth = widthPx;
    }
}

// The id output follows SetEntityIdOutputEnabled or the outline's need of it; the outline is the selected entity's
// draws of this frame's list. Both are context state that stays set, so only changes are sent (ring targets are
// separate contexts: each is brought up to date when its turn comes).
bool Renderer::SetTargetIds(ViewportContext& vc, uint32_t viewportId, const std::vector<tri_draw>& draws,
                            const std::vector<ECS::Entity>& entities) {
    const Target t{vc.m_Ctx, vc.m_Group};
    std::vector<uint32_t> selected;
    const bool outline = m_SelectionOutline && vc.m_Ctx && m_SelectedEntity != kNoEntity;
    if (outline)
        for (uint32_t d = 0; d < entities.size(); ++d)
            if (entities[d] == m_SelectedEntity) selected.push_back(d);
    auto want = m_IdOutputViewports.find(viewportId);
    const bool ids = (want != m_IdOutputViewports.end() && want->second) || !selected.empty() ||
                     (vc.m_Ctx && WantsMotion(viewportId));  // (the motion pass reads the ids)
    bool ok = true;
    if (ids != vc.m_IdOutput) {
        if (t.IdOutput(ids) != TRI_OK) {
            LogError("entity ids", tri_last_error());
            ok = false;
        } else {
            vc.m_IdOutput = ids;
            if (!ids) vc.m_OutlineSet = false;  // (switching the output off removes the context's outline)
        }
    }
    vc.m_DrawEntities = vc.m_IdOutput ? entities : std::vector<ECS::Entity>();
    if (!vc.m_Ctx) return ok;
    if (selected.empty() || !vc.m_IdOutput) {
        if (vc.m_OutlineSet && tri_set_outline(vc.m_Ctx, nullptr) != TRI_OK) ok = false;
        vc.m_OutlineSet = false;
        return ok;
    }
    const glm::vec4 &a = vc.m_OutlineColour, &b = m_OutlineColour;
    if (vc.m_OutlineSet && vc.m_OutlineDraws == selected && a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w &&
        vc.m_OutlineWidth == m_OutlineWidth)
        return ok;
    // (tri_set_outline checks the indices against the context's current draw list: this frame's goes in first;
    // SubmitTarget's own tri_set_draws of the same list then changes nothing)
    tri_outline o{};
    o.draws = selected.data();
    o.draw_count = (uint32_t)selected.size();
    o.rgba[0] = m_OutlineColour.x; o.rgba[1] = m_OutlineColour.y; o.rgba[2] = m_OutlineColour.z; o.rgba[3] = m_OutlineColour.w;
    o.width_px = m_OutlineWidth;
    if (tri_set_draws(vc.m_Ctx, draws.data(), (uint32_t)draws.size()) != TRI_OK || tri_set_outline(vc.m_Ctx, &o) != TRI_OK) {
        LogError("selection outline", tri_last_error());
        return false;
    }
    vc.m_OutlineSet = true;
    vc.m_OutlineDraws = selected;
    vc.m_OutlineColour = m_OutlineColour;
    vc.m_OutlineWidth = m_OutlineWidth;
    return ok;
}

const Renderer::ViewportContext* Renderer::IdTarget(uint32_t viewportId) {
    FinishFrame();
    const ViewportContext* vc = LatestTarget(viewportId);
    if (!vc || (!vc->m_Ctx && !vc->m_Group) || !vc->m_IdOutput) return nullptr;
    return vc;
}

// A viewport pixel as a pixel of the target's frame: the same unless temporal upscaling renders the viewport smaller, then
// the render pixel that holds the viewport pixel's centre (the upscale rule's unjittered sample). Negative stays negative.
void Renderer::ToFramePixel(const ViewportContext& vc, int32_t& x, int32_t& y) const {
    if (&vc == &m_LegacyTarget || !IsTemporalUpscalingEnabled(vc.m_Info.ViewportID)) return;
    const int64_t vw = (int64_t)std::max(vc.m_Info.Size.x, 0.0f), vh = (int64_t)std::max(vc.m_Info.Size.y, 0.0f);
    if (vw <= 0 || vh <= 0) return;
    if (x >= 0) x = (int32_t)std::min<int64_t>((2 * (int64_t)x + 1) * vc.m_Width / (2 * vw), 0x7FFFFFFF);
    if (y >= 0) y = (int32_t)std::min<int64_t>((2 * (int64_t)y + 1) * vc.m_Height / (2 * vh), 0x7FFFFFFF);
}

bool Renderer::PickEntity(uint32_t viewportId, int32_t x, int32_t y, ECS::Entity& out, float* depth01) {
    const ViewportContext* vc = IdTarget(viewportId);
    if (vc) ToFramePixel(*vc, x, y);
    if (!vc || x < 0 || y < 0 || x >= (int32_t)vc->m_Width || y >= (int32_t)vc->m_Height) return false;
    tri_pick_result r{};
    if (Target{vc->m_Ctx, vc->m_Group}.Pick(x, y, &r) != TRI_OK) {
        LogError("entity pick", tri_last_error());
        return false;
    }
    if (r.id == 0 || r.id > vc->m_DrawEntities.size()) return false;
    out = vc->m_DrawEntities[r.id - 1];
    if (depth01) {
        float z = 1.0f;
        if (r.has_depth) std::memcpy(&z, &r.depth_bits, 4);
        *depth01 = z;
    }
    return true;
}

std::vector<ECS::Entity> Renderer::PickEntitiesInRect(uint32_t viewportId, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    std::vector<ECS::Entity> found;
    const ViewportContext* vc = IdTarget(viewportId);
    if (!vc || x1 < x0 || y1 < y0) return found;
    ToFramePixel(*vc, x0, y0);
    ToFramePixel(*vc, x1, y1);
    const uint32_t n = (uint32_t)vc->m_DrawEntities.size();
    std::vector<uint32_t> bits((n + 31u) / 32u + 1u, 0u);
    if (vc->m_Ctx) {
        if (tri_pick_rect(vc->m_Ctx, x0, y0, x1, y1, bits.data(), (uint32_t)bits.size(), nullptr) != TRI_OK) {
            LogError("entity pick", tri_last_error());
            return found;
        }
    } else {  // a multi-device viewport: from the bands' ids on the host
        std::vector<uint32_t> ids((size_t)vc->m_Width * vc->m_Height);
        if (tri_group_read_ids(vc->m_Group, ids.data()) != TRI_OK) {
            LogError("entity pick", tri_last_error());
            return found;
        }
        for (int32_t y = std::max(y0, 0); y <= std::min(y1, (int32_t)vc->m_Height - 1); ++y)
            for (int32_t x = std::max(x0, 0); x <= std::min(x1, (int32_t)vc->m_Width - 1); ++x) {
                const uint32_t id = ids[(size_t)y * vc->m_Width + x];
                if (id && id <= n) bits[(id - 1) / 32] |= 1u << ((id - 1) & 31u);
            }
    }
    for (uint32_t d = 0; d < n; ++d)  // draw order; an entity with several draws (none today) is named once
        if ((bits[d / 32] >> (d & 31u)) & 1u)
            if (std::find(found.begin(), found.end(), vc->m_DrawEntities[d]) == found.end()) found.push_back(vc->m_DrawEntities[d]);
    return found;
}

bool Renderer::ReadViewportEntityIds(uint32_t viewportId, std::vector<uint32_t>& out, uint32_t background) {
    const ViewportContext* vc = IdTarget(viewportId);
    if (!vc) return false;
    out.resize((size_t)vc->m_Width * vc->m_Height);
    if (Target{vc->m_Ctx, vc->m_Group}.ReadIds(out.data()) != TRI_OK) {
        LogError("entity ids", tri_last_error());
        return false;
    }
    for (uint32_t& v : out) v = (v == 0 || v > vc->m_DrawEntities.size()) ? background : vc->m_DrawEntities[v - 1];
    return true;
}

// ---- motion vectors -----------------------------------------------------------------------------------------------
void Renderer::SetMotionVectorOutputEnabled(uint32_t viewportId, bool enabled) {
    if (enabled && m_Devices.size() > 1) {
        LogError("motion vectors", "multi-device viewports (SetDeviceCount > 1) write no motion vectors");
        return;
    }
    m_MotionViewports[viewportId] = enabled;
}

bool Renderer::IsMotionVectorOutputEnabled(uint32_t viewportId) const {
    auto it = m_MotionViewports.find(viewportId);
    return it != m_MotionViewports.end() && it->second;
}

// The output is context state that stays set, so only changes are sent (ring targets are separate contexts: each is
// brought up to date when its turn comes). The history is the viewport's, whichever target rendered its last frame.
bool Renderer::SetTargetMotion(ViewportContext& vc, uint32_t viewportId, const tri_global_ubo& ubo,
                               const std::vector<tri_draw>& draws, const std::vector<ECS::Entity>& entities, const float* jitter) {
    const bool want = vc.m_Ctx && vc.m_IdOutput && WantsMotion(viewportId);
    if (vc.m_Ctx && want != vc.m_MotionOutput) {
        if (tri_set_motion_output(vc.m_Ctx, want ? 1 : 0) != TRI_OK || (want && tri_get_motion_output(vc.m_Ctx, &vc.m_MotionImage) != TRI_OK)) {
            LogError("motion vectors", tri_last_error());
            m_MotionHistory.erase(viewportId);
            return false;
        }
        vc.m_MotionOutput = want;
    }
    if (!want) {
        m_MotionHistory.erase(viewportId);  // the first frame after the output is switched on has no history
        return !WantsMotion(viewportId);
    }
    MotionHistory& h = m_MotionHistory[viewportId];
    const uint32_t n = (uint32_t)std::min(draws.size(), entities.size());
    int rc;
    if (h.m_Valid && h.m_Width == vc.m_Width && h.m_Height == vc.m_Height) {
        tri_motion_history mh{};
        std::memcpy(mh.prev_view, h.m_View, sizeof mh.prev_view);
        std::memcpy(mh.prev_projection, h.m_Projection, sizeof mh.prev_projection);
        // under temporal anti-aliasing: the previous unjittered projection under the CURRENT jitter
        if (jitter && tri_taa_jitter_projection(h.m_Projection, jitter[0], jitter[1], vc.m_Width, vc.m_Height, mh.prev_projection) != TRI_OK)
            LogError("temporal anti-aliasing", tri_last_error());
        std::vector<float> prev((size_t)n * 16);
        for (uint32_t d = 0; d < n; ++d) {  // an entity the last frame did not draw keeps its current model
            auto it = h.m_Models.find(entities[d]);
            std::memcpy(&prev[(size_t)d * 16], it != h.m_Models.end() ? it->second.data() : draws[d].pc.model, 64);
        }
        mh.prev_models = n ? prev.data() : nullptr;
        mh.draw_count = n;
        rc = tri_set_motion_history(vc.m_Ctx, &mh);
    } else {
        rc = tri_set_motion_history(vc.m_Ctx, nullptr);
    }
    if (rc != TRI_OK) LogError("motion vectors", tri_last_error());
    h.m_Valid = true;
    h.m_Width = vc.m_Width;
    h.m_Height = vc.m_Height;
    std::memcpy(h.m_View, ubo.view, sizeof h.m_View);
    std::memcpy(h.m_Projection, ubo.projection, sizeof h.m_Projection);
    h.m_Models.clear();
    for (uint32_t d = 0; d < n; ++d) std::memcpy(h.m_Models[entities[d]].data(), draws[d].pc.model, 64);
    return rc == TRI_OK;
}

const Renderer::ViewportContext* Renderer::MotionTarget(uint32_t viewportId) {
    FinishFrame();
    const ViewportContext* vc = LatestTarget(viewportId);
    if (!vc || !vc->m_Ctx || !vc->m_MotionOutput) return nullptr;
    return vc;
}

bool Renderer::ReadViewportMotionVectors(uint32_t viewportId, std::vector<float>& out) {
    const ViewportContext* vc = MotionTarget(viewportId);
    if (!vc) return false;
    out.resize((size_t)vc->m_Width * vc->m_Height * 2);
    if (tri_read_motion(vc->m_Ctx, out.data()) != TRI_OK) {
        LogError("motion vectors", tri_last_error());
        return false;
    }
    return true;
}

void* Renderer::GetViewportMotionTexture(uint32_t viewportId) {
    const ViewportContext* vc = MotionTarget(viewportId);
    return vc ? const_cast<tri_image*>(&vc->m_MotionImage) : nullptr;
}

// ---- history reprojection -------------------------------------------------------------------------------------------
void Renderer::SetHistoryReprojectionEnabled(uint32_t viewportId, bool enabled, float depthTolerance) {
    if (enabled && m_Devices.size() > 1) {
        LogError("history reprojection", "multi-device viewports (SetDeviceCount > 1) have no history reprojection");
        return;
    }
    if (enabled && !(depthTolerance >= 0.0f && std::isfinite(depthTolerance))) {
        LogError("history reprojection", "the depth tolerance is negative or not finite");
        return;
    }
    Reprojection& st = m_Reprojection[viewportId];
    // the first frame after the switch goes on has no history (frames rendered meanwhile were not stored)
    if (enabled && !st.m_Enabled && st.m_Object && tri_history_reset(st.m_Object) != TRI_OK)
        LogError("history reprojection", tri_last_error());
    if (!enabled) st.m_LastTarget = nullptr;  // the readers answer for reprojected frames only
    st.m_Enabled = enabled;
    st.m_DepthTolerance = depthTolerance;
}

bool Renderer::IsHistoryReprojectionEnabled(uint32_t viewportId) const {
    auto it = m_Reprojection.find(viewportId);
    return it != m_Reprojection.end() && it->second.m_Enabled;
}

// ---- what the three temporal passes' records share (Renderer.h) ---------------------------------------------------------
// The target's frame overflowed a queue and was rendered again. When its pass was the object's last, a redo pass reads
// the same previous frame and stores the complete one. With several frames in flight a later frame has already been
// built from the incomplete one: nothing can mend that frame, and the object is reset so that nothing builds on it.
template <typename Map, typename Reset>
void Renderer::RedoTemporal(Map& records, ViewportContext& vc, bool (Renderer::*pass)(ViewportContext&, uint32_t, bool),
                            Reset reset, const char* what) {
    auto it = records.find(vc.m_Info.ViewportID);
    if (it == records.end() || !it->second.m_Enabled || !it->second.m_Object || &vc == &m_LegacyTarget) return;
    if (it->second.m_LastTarget == &vc) {
        if ((this->*pass)(vc, vc.m_Info.ViewportID, true)) {
            if (tri_synchronize(vc.m_Ctx) != TRI_OK) LogError(what, tri_last_error());
        }
    } else if (reset(it->second.m_Object) != TRI_OK) {
        LogError(what, tri_last_error());
    }
}

template <typename Map>
typename Map::mapped_type* Renderer::TemporalOutput(Map& records, uint32_t viewportId) {
    FinishFrame();
    auto it = records.find(viewportId);
    if (it == records.end() || !it->second.m_Object || !it->second.m_LastTarget) return nullptr;
    if (it->second.m_LastTarget != LatestTarget(viewportId)) return nullptr;  // the latest frame did not go through the pass
    return &it->second;
}

template <typename Map>
auto Renderer::ResolvedBy(Map& records, const ViewportContext& vc) -> decltype(records.begin()->second.m_Object) {
    auto it = records.find(vc.m_Info.ViewportID);
    if (it != records.end() && it->second.m_Enabled && it->second.m_Object && it->second.m_LastTarget == &vc && vc.m_Ctx &&
        &vc != &m_LegacyTarget)
        return it->second.m_Object;
    return nullptr;
}

// One tri_history per viewport, whichever of its targets renders the frame: ring targets are separate contexts and the
// object orders its passes across their streams itself.
bool Renderer::ReprojectTarget(ViewportContext& vc, uint32_t viewportId, bool redo) {
    auto it = m_Reprojection.find(viewportId);
    if (it == m_Reprojection.end() || !it->second.m_Enabled) return true;
    Reprojection& st = it->second;
    st.m_LastTarget = nullptr;
    if (!vc.m_Ctx || !vc.m_MotionOutput) return false;
    if (!EnsureObject(st.m_Object, st.m_Width == vc.m_Width && st.m_Height == vc.m_Height, vc.m_Ctx, tri_history_destroy,
                      [&](int32_t device, tri_history** out) { return tri_history_create(device, vc.m_Width, vc.m_Height, out); },
                      "history reprojection"))
        return false;
    st.m_Width = vc.m_Width;
    st.m_Height = vc.m_Height;
    tri_reproject_params params{};
    params.depth_tolerance = st.m_DepthTolerance;
    params.flags = redo ? TRI_HISTORY_REDO : 0u;
    if (tri_history_reproject(st.m_Object, vc.m_Ctx, &params) != TRI_OK ||
        tri_history_get_output(st.m_Object, &st.m_Colour, &st.m_Mask) != TRI_OK) {
        LogError("history reprojection", tri_last_error());
        return false;
    }
    st.m_LastTarget = &vc;
    return true;
}

bool Renderer::ReadViewportReprojection(uint32_t viewportId, std::vector<uint8_t>& bgra, std::vector<uint8_t>& mask) {
    Reprojection* st = TemporalOutput(m_Reprojection, viewportId);
    if (!st) return false;
    bgra.resize((size_t)st->m_Width * st->m_Height * 4);
    mask.resize((size_t)st->m_Width * st->m_Height);
    if (tri_history_read(st->m_Object, bgra.data(), mask.data()) != TRI_OK) {
        LogError("history reprojection", tri_last_error());
        return false;
    }
    return true;
}

void* Renderer::GetViewportReprojectedTexture(uint32_t viewportId) {
    Reprojection* st = TemporalOutput(m_Reprojection, viewportId);
    return st ? &st->m_Colour : nullptr;
}

void* Renderer::GetViewportDisocclusionTexture(uint32_t viewportId) {
    Reprojection* st = TemporalOutput(m_Reprojection, viewportId);
    return st ? &st->m_Mask : nullptr;
}

// ---- temporal anti-aliasing -----------------------------------------------------------------------------------------
void Renderer::SetTemporalAntiAliasingEnabled(uint32_t viewportId, bool enabled, float alpha, uint32_t period, bool rejectIds) {
    if (enabled && m_Devices.size() > 1) {
        LogError("temporal anti-aliasing", "multi-device viewports (SetDeviceCount > 1) have no temporal anti-aliasing");
        return;
    }
    if (enabled && !(alpha > 0.0f && alpha <= 1.0f)) {
        LogError("temporal anti-aliasing", "alpha lies outside (0, 1]");
        return;
    }
    if (enabled && period > 64) {
        LogError("temporal anti-aliasing", "the jitter period is above 64");
        return;
    }
    if (enabled && IsTemporalUpscalingEnabled(viewportId)) {
        LogError("temporal anti-aliasing", "the viewport has temporal upscaling on (SetTemporalUpscalingEnabled)");
        return;
    }
    Taa& st = m_Taa[viewportId];
    if (enabled && !st.m_Enabled) {  // switching on: frames rendered meanwhile were not accumulated
        if (st.m_Object && tri_taa_reset(st.m_Object) != TRI_OK) LogError("temporal anti-aliasing", tri_last_error());
        st.m_FrameIndex = 0;
    }
    if (!enabled) st.m_LastTarget = nullptr;  // the readers and the present answer for resolved frames only
    st.m_Enabled = enabled;
    st.m_Alpha = alpha;
    st.m_Period = period;
    st.m_RejectIds = rejectIds;
}

bool Renderer::IsTemporalAntiAliasingEnabled(uint32_t viewportId) const {
    auto it = m_Taa.find(viewportId);
    return it != m_Taa.end() && it->second.m_Enabled;
}

bool Renderer::BeginTaaFrame(const ViewportContext& vc, uint32_t viewportId, float jitter[2]) {
    auto it = m_Taa.find(viewportId);
    if (it == m_Taa.end() || !it->second.m_Enabled || !vc.m_Ctx) return false;
    Taa& st = it->second;
    if (st.m_Width != vc.m_Width || st.m_Height != vc.m_Height) {  // the first frame, or a resize: the count restarts
        st.m_FrameIndex = 0;
        st.m_Width = vc.m_Width;
        st.m_Height = vc.m_Height;
    }
    if (tri_taa_jitter(st.m_FrameIndex, st.m_Period, jitter) != TRI_OK) {
        LogError("temporal anti-aliasing", tri_last_error());
        return false;
    }
    ++st.m_FrameIndex;
    return true;
}

// One tri_taa per viewport, whichever of its targets renders the frame, like the history reprojection's object.
bool Renderer::ResolveTarget(ViewportContext& vc, uint32_t viewportId, bool redo) {
    auto it = m_Taa.find(viewportId);
    if (it == m_Taa.end() || !it->second.m_Enabled) return true;
    Taa& st = it->second;
    st.m_LastTarget = nullptr;
    if (!vc.m_Ctx || !vc.m_MotionOutput) return false;
    if (!EnsureObject(st.m_Object, st.m_ObjectWidth == vc.m_Width && st.m_ObjectHeight == vc.m_Height, vc.m_Ctx, tri_taa_destroy,
                      [&](int32_t device, tri_taa** out) { return tri_taa_create(device, vc.m_Width, vc.m_Height, out); },
                      "temporal anti-aliasing"))
        return false;
    st.m_ObjectWidth = vc.m_Width;
    st.m_ObjectHeight = vc.m_Height;
    tri_taa_params params{};
    params.alpha = st.m_Alpha;
    params.flags = (redo ? TRI_TAA_REDO : 0u) | (st.m_RejectIds ? TRI_TAA_REJECT_ID : 0u);
    if (tri_taa_resolve(st.m_Object, vc.m_Ctx, &params) != TRI_OK ||
        tri_taa_get_output(st.m_Object, &st.m_Resolved, nullptr, nullptr) != TRI_OK) {
        LogError("temporal anti-aliasing", tri_last_error());
        return false;
    }
    st.m_LastTarget = &vc;
    return true;
}

int Renderer::PresentBlit(ViewportContext& vc, uint32_t width, uint32_t height) {
    if (tri_taa* taa = ResolvedBy(m_Taa, vc)) return tri_taa_blit_linear(taa, vc.m_Ctx, nullptr, width, height);
    if (tri_upscale* up = ResolvedBy(m_Upscale, vc)) return tri_upscale_blit_linear(up, vc.m_Ctx, nullptr, width, height);
    return Target{vc.m_Ctx, vc.m_Group}.Blit(width, height);
}

// ---- temporal upscaling ---------------------------------------------------------------------------------------------
namespace {
uint32_t ScaledExtent(uint32_t size, float scale) { return std::max(1u, (uint32_t)((float)size * scale + 0.5f)); }
}  // namespace

bool Renderer::SetTemporalUpscalingEnabled(uint32_t viewportId, bool enabled, float renderScale, float alpha, bool rejectIds) {
    if (enabled && m_Devices.size() > 1) {
        LogError("temporal upscaling", "multi-device viewports (SetDeviceCount > 1) have no temporal upscaling");
        return false;
    }
    if (enabled && !(alpha > 0.0f && alpha <= 1.0f)) {
        LogError("temporal upscaling", "alpha lies outside (0, 1]");
        return false;
    }
    if (enabled && !(renderScale >= 1.0f / 3.0f && renderScale <= 1.0f)) {
        LogError("temporal upscaling", "the render scale lies outside [1/3, 1]");
        return false;
    }
    if (enabled && IsTemporalAntiAliasingEnabled(viewportId)) {
        LogError("temporal upscaling", "the viewport has temporal anti-aliasing on (SetTemporalAntiAliasingEnabled)");
        return false;
    }
    if (enabled && m_Recording && viewportId == m_RecordingViewportId) {  // (the session's extent is the viewport's size)
        LogError("temporal upscaling", "the viewport is being recorded (SetViewportRecordingEnabled)");
        return false;
    }
    auto vp = m_Viewports.find(viewportId);
    if (enabled && vp != m_Viewports.end()) {  // the extent rule, for the size the viewport has now
        const uint32_t w = (uint32_t)std::max(vp->second.m_Info.Size.x, 0.0f), h = (uint32_t)std::max(vp->second.m_Info.Size.y, 0.0f);
        uint32_t period = 0;
        if (w && h && tri_upscale_jitter_period(ScaledExtent(w, renderScale), ScaledExtent(h, renderScale), w, h, &period) != TRI_OK) {
            LogError("temporal upscaling", tri_last_error());
            return false;
        }
    }
    Upscale& st = m_Upscale[viewportId];
    if (enabled && (!st.m_Enabled || st.m_Scale != renderScale)) {  // switching on, or another scale: no history
        if (st.m_Object && tri_upscale_reset(st.m_Object) != TRI_OK) LogError("temporal upscaling", tri_last_error());
        st.m_FrameIndex = 0;
    }
    if (!enabled) st.m_LastTarget = nullptr;  // the readers and the present answer for upscaled frames only
    st.m_Enabled = enabled;
    if (enabled) {
        st.m_Scale = renderScale;
        st.m_Alpha = alpha;
        st.m_RejectIds = rejectIds;
    }
    return true;
}

bool Renderer::IsTemporalUpscalingEnabled(uint32_t viewportId) const {
    auto it = m_Upscale.find(viewportId);
    return it != m_Upscale.end() && it->second.m_Enabled;
}

void Renderer::RenderExtent(const ViewportContext& vc, uint32_t& width, uint32_t& height) const {
    if (&vc == &m_LegacyTarget) return;
    auto it = m_Upscale.find(vc.m_Info.ViewportID);
    if (it == m_Upscale.end() || !it->second.m_Enabled) return;
    width = ScaledExtent(width, it->second.m_Scale);
    height = ScaledExtent(height, it->second.m_Scale);
}

bool Renderer::BeginUpscaleFrame(const ViewportContext& vc, uint32_t viewportId, float jitter[2]) {
    auto it = m_Upscale.find(viewportId);
    if (it == m_Upscale.end() || !it->second.m_Enabled || !vc.m_Ctx || &vc == &m_LegacyTarget) return false;
    Upscale& st = it->second;
    st.m_Jitter[0] = st.m_Jitter[1] = 0.0f;
    if (st.m_Width != vc.m_Width || st.m_Height != vc.m_Height) {  // the first frame, a resize or another scale
        st.m_FrameIndex = 0;
        st.m_Width = vc.m_Width;
        st.m_Height = vc.m_Height;
    }
    const uint32_t ow = (uint32_t)std::max(vc.m_Info.Size.x, 0.0f), oh = (uint32_t)std::max(vc.m_Info.Size.y, 0.0f);
    uint32_t period = 0;
    if (tri_upscale_jitter_period(vc.m_Width, vc.m_Height, ow, oh, &period) != TRI_OK ||
        tri_taa_jitter(st.m_FrameIndex, period, jitter) != TRI_OK) {
        LogError("temporal upscaling", tri_last_error());
        jitter[0] = jitter[1] = 0.0f;
        return false;
    }
    st.m_Jitter[0] = jitter[0];
    st.m_Jitter[1] = jitter[1];
    ++st.m_FrameIndex;
    return true;
}

// One tri_upscale per viewport, whichever of its targets renders the frame, like temporal anti-aliasing's object.
bool Renderer::UpscaleTarget(ViewportContext& vc, uint32_t viewportId, bool redo) {
    auto it = m_Upscale.find(viewportId);
    if (it == m_Upscale.end() || !it->second.m_Enabled || &vc == &m_LegacyTarget) return true;
    Upscale& st = it->second;
    st.m_LastTarget = nullptr;
    if (!vc.m_Ctx || !vc.m_MotionOutput) return false;
    const uint32_t ow = (uint32_t)std::max(vc.m_Info.Size.x, 0.0f), oh = (uint32_t)std::max(vc.m_Info.Size.y, 0.0f);
    const bool matches = st.m_RenderWidth == vc.m_Width && st.m_RenderHeight == vc.m_Height && st.m_OutWidth == ow && st.m_OutHeight == oh;
    if (!EnsureObject(st.m_Object, matches, vc.m_Ctx, tri_upscale_destroy,  // (another scale is another extent)
                      [&](int32_t device, tri_upscale** out) { return tri_upscale_create(device, vc.m_Width, vc.m_Height, ow, oh, out); },
                      "temporal upscaling"))
        return false;
    st.m_RenderWidth = vc.m_Width;
    st.m_RenderHeight = vc.m_Height;
    st.m_OutWidth = ow;
    st.m_OutHeight = oh;
    tri_upscale_params params{};
    params.alpha = st.m_Alpha;
    params.jitter[0] = st.m_Jitter[0];
    params.jitter[1] = st.m_Jitter[1];
    params.flags = (redo ? TRI_UPSCALE_REDO : 0u) | (st.m_RejectIds ? TRI_UPSCALE_REJECT_ID : 0u);
    if (tri_upscale_resolve(st.m_Object, vc.m_Ctx, &params) != TRI_OK ||
        tri_upscale_get_output(st.m_Object, &st.m_Resolved, nullptr, nullptr) != TRI_OK) {
        LogError("temporal upscaling", tri_last_error());
        return false;
    }
    st.m_LastTarget = &vc;
    return true;
}

bool Renderer::ReadViewportUpscaledPixels(uint32_t viewportId, std::vector<uint8_t>& rgba, uint32_t* width, uint32_t* height) {
    Upscale* st = TemporalOutput(m_Upscale, viewportId);
    if (!st) return false;
    std::vector<uint8_t> bgra((size_t)st->m_OutWidth * st->m_OutHeight * 4);
    if (tri_upscale_read(st->m_Object, bgra.data(), nullptr, nullptr) != TRI_OK) {
        LogError("temporal upscaling", tri_last_error());
        return false;
    }
    BgraToRgba(bgra, rgba);
    if (width) *width = st->m_OutWidth;
    if (height) *height = st->m_OutHeight;
    return true;
}

bool Renderer::ReadViewportUpscaleMask(uint32_t viewportId, std::vector<uint8_t>& mask) {
    Upscale* st = TemporalOutput(m_Upscale, viewportId);
    if (!st) return false;
    mask.resize((size_t)st->m_OutWidth * st->m_OutHeight);
    if (tri_upscale_read(st->m_Object, nullptr, nullptr, mask.data()) != TRI_OK) {
        LogError("temporal upscaling", tri_last_error());
        return false;
    }
    return true;
}

void* Renderer::GetViewportUpscaledTexture(uint32_t viewportId) {
    Upscale* st = TemporalOutput(m_Upscale, viewportId);
    return st ? &st->m_Resolved : nullptr;
}

bool Renderer::ReadViewportResolvedPixels(uint32_t viewportId, std::vector<uint8_t>& rgba) {
    Taa* st = TemporalOutput(m_Taa, viewportId);
    if (!st) return false;
    std::vector<uint8_t> bgra((size_t)st->m_ObjectWidth * st->m_ObjectHeight * 4);
    if (tri_taa_read(st->m_Object, bgra.data(), nullptr, nullptr) != TRI_OK) {
        LogError("temporal anti-aliasing", tri_last_error());
        return false;
    }
    BgraToRgba(bgra, rgba);
    return true;
}

bool Renderer::ReadViewportTaaMask(uint32_t viewportId, std::vector<uint8_t>& mask) {
    Taa* st = TemporalOutput(m_Taa, viewportId);
    if (!st) return false;
    mask.resize((size_t)st->m_ObjectWidth * st->m_ObjectHeight);
    if (tri_taa_read(st->m_Object, nullptr, nullptr, mask.data()) != TRI_OK) {
        LogError("temporal anti-aliasing", tri_last_error());
        return false;
    }
    return true;
}

void* Renderer::GetViewportResolvedTexture(uint32_t viewportId) {
    Taa* st = TemporalOutput(m_Taa, viewportId);
    return st ? &st->m_Resolved : nullptr;
}

void* Renderer::GetViewportTexture(uint32_t viewportId) const {
    const_cast<Renderer*>(this)->FinishFrame();  // the handle's contents are a completed frame
    const ViewportContext* vc = LatestTarget(viewportId);  // the latest frame's target (frames in flight)
    if (!vc || (!vc->m_Ctx && !vc->m_Group) || !vc->m_HasImage) return nullptr;
    return const_cast<tri_image*>(&vc->m_Image);
}

bool Renderer::ReadViewportPixels(uint32_t viewportId, std::vector<uint8_t>& rgba, std::vector<float>* depth) {
    FinishFrame();
    const ViewportContext* latest = LatestTarget(viewportId);  // the latest frame's target (frames in flight)
    if (!latest || (!latest->m_Ctx && !latest->m_Group)) return false;
    const ViewportContext& vc = *latest;
    std::vector<uint8_t> bgra((size_t)vc.m_Width * vc.m_Height * 4);
    std::vector<uint32_t> dbits;
    if (depth) dbits.resize((size_t)vc.m_Width * vc.m_Height);
    if (Target{vc.m_Ctx, vc.m_Group}.Readback(bgra.data(), depth ? dbits.data() : nullptr) != TRI_OK) {
        LogError("readback", tri_last_error());
        return false;
    }
    BgraToRgba(bgra, rgba);
    if (depth) {
        depth->resize(dbits.size());
        std::memcpy(depth->data(), dbits.data(), dbits.size() * 4);
    }
    return true;
}

bool Renderer::ReadPresentPixels(std::vector<uint8_t>& rgba, uint32_t& width, uint32_t& height) {
    FinishFrame();
    if (!m_PresentSource && !m_PresentGroup) return false;
    // sized from the extent the present was produced at, not the current SetPresentExtent (a resize between
    // DrawFrame and this read would otherwise under-size the buffer the readback fills)
    std::vector<uint8_t> bgra((size_t)m_PresentedWidth * m_PresentedHeight * 4);
    const Target t{m_PresentSource, m_PresentGroup};
    if ((m_PresentLegacy ? t.Readback(bgra.data(), nullptr) : t.ReadPresent(bgra.data())) != TRI_OK) {
        LogError("present readback", tri_last_error());
        return false;
    }
    BgraToRgba(bgra, rgba);
    width = m_PresentedWidth;
    height = m_PresentedHeight;
    return true;
}

}  // namespace Trident
