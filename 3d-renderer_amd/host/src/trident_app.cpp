// trident_app.cpp — flat C driver over Trident::Renderer (see host/include/trident_app.h).
// Entity set-up follows Forge's ApplicationLayer: a primitive spawned with Transform +
// MeshComponent (ApplicationLayer.cpp:677-718), lights as LightComponent entities.
#include "trident_app.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "trident/Renderer.h"
#include "trident/SceneFile.h"
#include "trident/ModelLoader.h"
#include "trident/Animation.h"
#include "trident/AnimationSystem.h"
#include "trident/AnimationStateMachine.h"

#include <algorithm>
#include <array>

using namespace Trident;

struct trident_app {
    Renderer renderer;
    ECS::Registry registry;
    EditorCamera editor;
    RuntimeCamera runtime;
    ECS::AnimationSystem animation{&renderer};
};

namespace {

glm::vec3 V3(const float* p, glm::vec3 dflt) { return p ? glm::vec3{p[0], p[1], p[2]} : dflt; }

template <typename F>
int Guard(trident_app* app, F&& f) {
    if (!app) return TRI_E_INVALID;
    try {
        return f();
    } catch (const std::exception&) {
        return TRI_E_INVALID;
    }
}

template <typename F>
int GuardDataset(trident_dataset* dataset, F&& f) {
    if (!dataset) return TRI_E_INVALID;
    try {
        f();
        return TRI_OK;
    } catch (const std::exception&) {
        return TRI_E_INVALID;
    }
}

}  // namespace

extern "C" {

int trident_app_create(uint32_t raster_flags, trident_app** out) {
    if (!out) return TRI_E_INVALID;
    *out = nullptr;
    try {
        auto* app = new trident_app();
        app->renderer.Init();
        app->renderer.SetRasterFlags(raster_flags);
        app->renderer.SetActiveRegistry(&app->registry);
        app->renderer.SetEditorCamera(&app->editor);
        app->renderer.SetRuntimeCamera(&app->runtime);
        *out = app;
        return TRI_OK;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

void trident_app_destroy(trident_app* app) {
    if (!app) return;
    app->renderer.Shutdown();
    delete app;
}

int trident_app_append_mesh(trident_app* app, const tri_vertex* vertices, uint32_t vertex_count,
                            const uint32_t* indices, uint32_t index_count, const float base_color[4], float metallic,
                            float roughness, const char* texture_path, uint32_t* mesh_index) {
    return Guard(app, [&] {
        if ((!vertices && vertex_count) || (!indices && index_count) || index_count % 3) return TRI_E_INVALID;
        Geometry::Mesh mesh;
        mesh.Vertices.resize(vertex_count);
        if (vertex_count) std::memcpy(static_cast<void*>(mesh.Vertices.data()), vertices, (size_t)vertex_count * sizeof(Vertex));
        mesh.Indices.assign(indices, indices + index_count);
        mesh.MaterialIndex = 0;  // local to this append; AppendMeshes offsets it
        Geometry::Material mat;
        if (base_color) mat.BaseColorFactor = {base_color[0], base_color[1], base_color[2], base_color[3]};
        mat.MetallicFactor = metallic;
        mat.RoughnessFactor = roughness;
        std::vector<std::string> textures;
        if (texture_path && *texture_path) {
            textures.emplace_back(texture_path);
            mat.BaseColorTextureIndex = 0;
        }
        const size_t before = app->renderer.GetModelCount();
        app->renderer.AppendMeshes({mesh}, {mat}, textures);
        if (mesh_index) *mesh_index = static_cast<uint32_t>(before);
        return TRI_OK;
    });
}

int trident_app_upload_texture(trident_app* app, const char* path, const uint8_t* rgba, uint32_t width,
                               uint32_t height) {
    return Guard(app, [&] {
        if (!path || !rgba || !width || !height) return TRI_E_INVALID;
        Loader::TextureData t;
        t.Width = (int)width;
        t.Height = (int)height;
        t.Pixels.assign(rgba, rgba + (size_t)width * height * 4);
        app->renderer.UploadTexture(path, t);
        return TRI_OK;
    });
}

int trident_app_add_mesh_entity(trident_app* app, int primitive, uint32_t mesh_index, const float position[3],
                                const float rotation_deg[3], const float scale[3], uint32_t* entity) {
    return Guard(app, [&] {
        if (primitive < 0 || primitive > 3) return TRI_E_INVALID;
        const ECS::Entity e = app->registry.CreateEntity();
        Transform& t = app->registry.AddComponent<Transform>(e);
        t.Position = V3(position, glm::vec3{0.0f});
        t.Rotation = V3(rotation_deg, glm::vec3{0.0f});
        t.Scale = V3(scale, glm::vec3{1.0f});
        MeshComponent& m = app->registry.AddComponent<MeshComponent>(e);
        m.m_Primitive = static_cast<MeshComponent::PrimitiveType>(primitive);
        if (primitive == 0) m.m_MeshIndex = mesh_index;
        if (entity) *entity = e;
        return TRI_OK;
    });
}

int trident_app_add_sprite_entity(trident_app* app, const float position[3], const float rotation_deg[3],
                                  const float scale[3], const float tint[4], const float uv_scale[2],
                                  const float uv_offset[2], float tiling, uint32_t* entity) {
    return Guard(app, [&] {
        const ECS::Entity e = app->registry.CreateEntity();
        Transform& t = app->registry.AddComponent<Transform>(e);
        t.Position = V3(position, glm::vec3{0.0f});
        t.Rotation = V3(rotation_deg, glm::vec3{0.0f});
        t.Scale = V3(scale, glm::vec3{1.0f});
        SpriteComponent& sp = app->registry.AddComponent<SpriteComponent>(e);
        if (tint) sp.m_TintColor = {tint[0], tint[1], tint[2], tint[3]};
        if (uv_scale) sp.m_UVScale = {uv_scale[0], uv_scale[1]};
        if (uv_offset) sp.m_UVOffset = {uv_offset[0], uv_offset[1]};
        sp.m_TilingFactor = tiling;
        if (entity) *entity = e;
        return TRI_OK;
    });
}

int trident_app_set_sprite_visible(trident_app* app, uint32_t entity, int visible) {
    return Guard(app, [&] {
        if (!app->registry.HasComponent<SpriteComponent>(entity)) return TRI_E_INVALID;
        app->registry.GetComponent<SpriteComponent>(entity).m_Visible = visible != 0;
        return TRI_OK;
    });
}

int trident_app_entity_sprite(trident_app* app, uint32_t entity, float out[10]) {
    return Guard(app, [&] {
        if (!app->registry.HasComponent<SpriteComponent>(entity)) return TRI_E_INVALID;
        const SpriteComponent& sp = app->registry.GetComponent<SpriteComponent>(entity);
        const float v[10] = {sp.m_TintColor.x, sp.m_TintColor.y, sp.m_TintColor.z, sp.m_TintColor.w, sp.m_UVScale.x,
                             sp.m_UVScale.y, sp.m_UVOffset.x, sp.m_UVOffset.y, sp.m_TilingFactor,
                             sp.m_Visible ? 1.0f : 0.0f};
        std::memcpy(out, v, sizeof v);
        return TRI_OK;
    });
}

int trident_app_set_entity_texture(trident_app* app, uint32_t entity, const char* texture_path) {
    return Guard(app, [&] {
        TextureComponent& t = app->registry.AddComponent<TextureComponent>(entity);
        t.m_TexturePath = texture_path ? texture_path : "";
        t.m_TextureSlot = -1;
        t.m_IsDirty = true;
        return TRI_OK;
    });
}

int trident_app_set_entity_transform(trident_app* app, uint32_t entity, const float position[3],
                                     const float rotation_deg[3], const float scale[3]) {
    return Guard(app, [&] {
        if (!app->registry.HasComponent<Transform>(entity)) return TRI_E_INVALID;
        Transform& t = app->registry.GetComponent<Transform>(entity);
        t.Position = V3(position, t.Position);
        t.Rotation = V3(rotation_deg, t.Rotation);
        t.Scale = V3(scale, t.Scale);
        return TRI_OK;
    });
}

int trident_app_set_entity_visible(trident_app* app, uint32_t entity, int visible) {
    return Guard(app, [&] {
        if (!app->registry.HasComponent<MeshComponent>(entity)) return TRI_E_INVALID;
        app->registry.GetComponent<MeshComponent>(entity).m_Visible = visible != 0;
        return TRI_OK;
    });
}

namespace {
void CopySource(const std::string& src, char* out, uint32_t cap) {
    if (!out || cap == 0) return;
    const size_t n = std::min<size_t>(src.size(), cap - 1);
    std::memcpy(out, src.data(), n);
    out[n] = 0;
}
}  // namespace

int trident_app_set_light_shadow_caster(trident_app* app, uint32_t entity, int caster) {
    return Guard(app, [&] {
        if (!app->registry.HasComponent<LightComponent>(entity)) return TRI_E_INVALID;
        app->registry.GetComponent<LightComponent>(entity).m_ShadowCaster = caster != 0;
        return TRI_OK;
    });
}

int trident_app_set_shadow_map_size(trident_app* app, uint32_t size) {
    return Guard(app, [&] {
        if (size > TRI_MAX_DIM) return TRI_E_INVALID;
        app->renderer.SetShadowMapSize(size);
        return TRI_OK;
    });
}

int trident_app_set_device_count(trident_app* app, uint32_t count, const int32_t* devices) {
    return Guard(app, [&] {
        std::vector<int32_t> devs;
        if (devices && count > 1) devs.assign(devices, devices + count);
        return app->renderer.SetDeviceCount(count, devs) ? TRI_OK : TRI_E_INVALID;
    });
}

int trident_app_shadow_config(trident_app* app, tri_shadow_config* out, int* enabled) {
    return Guard(app, [&] {
        if (!out || !enabled) return TRI_E_INVALID;
        tri_global_ubo ubo;
        std::vector<tri_draw> draws;  // GatherMeshDraws for the current registry state
        app->renderer.BuildFrameInputs(app->renderer.GetActiveViewportId(), ubo, draws);
        *enabled = app->renderer.BuildShadowConfig(*out) ? 1 : 0;
        return TRI_OK;
    });
}

int trident_app_viewport_texture(trident_app* app, uint32_t viewport_id, tri_image* out) {
    return Guard(app, [&] {
        if (!out) return TRI_E_INVALID;
        const void* h = app->renderer.GetViewportTexture(viewport_id);
        if (!h) return TRI_E_STATE;
        *out = *static_cast<const tri_image*>(h);
        return TRI_OK;
    });
}

int trident_app_geometry_uploads(trident_app* app, uint64_t* count) {
    return Guard(app, [&] {
        if (!count) return TRI_E_INVALID;
        *count = app->renderer.GetGeometryUploadCount();
        return TRI_OK;
    });
}

int trident_app_set_assets_dir(trident_app* app, const char* directory, char* source, uint32_t source_cap) {
    return Guard(app, [&] {
        if (!directory) return TRI_E_INVALID;
        app->renderer.SetAssetsDirectory(directory);
        CopySource(app->renderer.GetSkyboxSource(), source, source_cap);
        return TRI_OK;
    });
}

int trident_load_image(const char* path, int flip, uint8_t* rgba, uint64_t capacity, uint32_t* width, uint32_t* height) {
    if (!path || !width || !height) return TRI_E_INVALID;
    try {
        Loader::TextureData t;
        if (flip) {
            t = Loader::TextureLoader::Load(path);
        } else {
            std::array<std::string, 6> one;
            one.fill(path);
            const Loader::CubemapTextureData c = Loader::SkyboxTextureLoader::LoadFromFaces(one);
            if (c.m_Width) {
                t.Width = (int)c.m_Width;
                t.Height = (int)c.m_Height;
                t.Pixels.assign(c.m_PixelData.begin(), c.m_PixelData.begin() + (size_t)c.m_Width * c.m_Height * 4);
            }
        }
        if (t.Width <= 0) return TRI_E_INVALID;
        *width = (uint32_t)t.Width;
        *height = (uint32_t)t.Height;
        if (!rgba) return TRI_OK;
        if (capacity < t.Pixels.size()) return TRI_E_OVERFLOW;
        std::memcpy(rgba, t.Pixels.data(), t.Pixels.size());
        return TRI_OK;
    } catch (...) {
        return TRI_E_INVALID;
    }
}

int trident_load_default_skybox(const char* assets_dir, uint8_t* faces, uint64_t capacity, uint32_t* size, char* source,
                                uint32_t source_cap) {
    if (!assets_dir || !size) return TRI_E_INVALID;
    try {
        std::string src;
        const Loader::CubemapTextureData c = Loader::DiscoverDefaultSkybox(assets_dir, src);
        CopySource(src, source, source_cap);
        *size = c.IsValid() ? c.m_Width : 0;
        if (!faces || !c.IsValid()) return TRI_OK;
        if (c.m_Format != Loader::CubemapFormat::Rgba8Srgb || c.m_MipCount != 1) return TRI_E_UNSUPPORTED;
        if (capacity < c.m_PixelData.size()) return TRI_E_OVERFLOW;
        std::memcpy(faces, c.m_PixelData.data(), c.m_PixelData.size());
        return TRI_OK;
    } catch (...) {
        return TRI_E_INVALID;
    }
}

static int ReturnCubemap(const Loader::CubemapTextureData& c, trident_cubemap_info* info, uint8_t* texels, uint64_t capacity) {
    *info = trident_cubemap_info{};
    if (!c.IsValid()) return TRI_OK;
    info->format = (uint32_t)c.m_Format;
    info->size = c.m_Width;
    info->mip_count = c.m_MipCount;
    info->bytes_per_pixel = c.m_BytesPerPixel;
    info->is_hdr = c.m_IsHdr ? 1u : 0u;
    info->region_levels = (uint32_t)c.m_FaceRegions.size();
    info->bytes = c.ChainBytes();
    if (!texels) return TRI_OK;
    if (capacity < info->bytes) return TRI_E_OVERFLOW;
    std::memcpy(texels, c.m_PixelData.data(), (size_t)info->bytes);
    return TRI_OK;
}

int trident_load_default_skybox_ex(const char* assets_dir, trident_cubemap_info* info, uint8_t* texels, uint64_t capacity,
                                   char* source, uint32_t source_cap) {
    if (!assets_dir || !info) return TRI_E_INVALID;
    try {
        std::string src;
        const Loader::CubemapTextureData c = Loader::DiscoverDefaultSkybox(assets_dir, src);
        CopySource(src, source, source_cap);
        return ReturnCubemap(c, info, texels, capacity);
    } catch (...) {
        return TRI_E_INVALID;
    }
}

int trident_load_skybox(const char* path, int kind, trident_cubemap_info* info, uint8_t* texels, uint64_t capacity) {
    if (!path || !info || kind < 0 || kind > 1) return TRI_E_INVALID;
    try {
        return ReturnCubemap(kind == 0 ? Loader::SkyboxTextureLoader::LoadFromKtx(path)
                                       : Loader::SkyboxTextureLoader::LoadFromDirectory(path),
                             info, texels, capacity);
    } catch (...) {
        return TRI_E_INVALID;
    }
}

int trident_float_to_half(const float* values, uint16_t* halves, uint32_t count) {
    if (count && (!values || !halves)) return TRI_E_INVALID;
    for (uint32_t i = 0; i < count; ++i) halves[i] = Loader::FloatToHalf(values[i]);
    return TRI_OK;
}

int trident_app_set_entity_bones(trident_app* app, uint32_t entity, const float* matrices, uint32_t count) {
    return Guard(app, [&] {
        if (count && !matrices) return TRI_E_INVALID;
        AnimationComponent& a = app->registry.HasComponent<AnimationComponent>(entity)
                                    ? app->registry.GetComponent<AnimationComponent>(entity)
                                    : app->registry.AddComponent<AnimationComponent>(entity);
        a.m_BoneMatrices.resize(count);
        for (uint32_t b = 0; b < count; ++b)
            for (int c = 0; c < 4; ++c)
                for (int r = 0; r < 4; ++r) a.m_BoneMatrices[b][c][r] = matrices[16 * b + 4 * c + r];
        return TRI_OK;
    });
}

int trident_app_set_entities_bones(trident_app* app, const uint32_t* entities, uint32_t entity_count,
                                   const float* matrices, uint32_t matrices_per_entity) {
    return Guard(app, [&] {
        if (entity_count && (!entities || (matrices_per_entity && !matrices))) return TRI_E_INVALID;
        for (uint32_t i = 0; i < entity_count; ++i) {
            const int rc = trident_app_set_entity_bones(app, entities[i], matrices + 16ull * matrices_per_entity * i, matrices_per_entity);
            if (rc != TRI_OK) return rc;
        }
        return TRI_OK;
    });
}

int trident_app_add_light(trident_app* app, int type, const float position[3], const float direction[3],
                          const float color[3], float intensity, float range, int enabled, uint32_t* entity) {
    return Guard(app, [&] {
        if (type != TRIDENT_LIGHT_DIRECTIONAL && type != TRIDENT_LIGHT_POINT) return TRI_E_INVALID;
        const ECS::Entity e = app->registry.CreateEntity();
        Transform& t = app->registry.AddComponent<Transform>(e);
        t.Position = V3(position, glm::vec3{0.0f});
        LightComponent& l = app->registry.AddComponent<LightComponent>(e);
        l.m_Type = static_cast<LightComponent::Type>(type);
        l.m_Direction = V3(direction, l.m_Direction);
        l.m_Color = V3(color, l.m_Color);
        l.m_Intensity = intensity;
        l.m_Range = range;
        l.m_Enabled = enabled != 0;
        if (entity) *entity = e;
        return TRI_OK;
    });
}

int trident_app_set_camera(trident_app* app, int which, const float position[3], const float rotation_deg[3],
                           float fov_deg, float near_clip, float far_clip, int ready) {
    return Guard(app, [&] {
        if (which != 0 && which != 1) return TRI_E_INVALID;
        Camera& cam = which == 0 ? static_cast<Camera&>(app->editor) : static_cast<Camera&>(app->runtime);
        cam.SetPosition(V3(position, cam.GetPosition()));
        cam.SetRotation(V3(rotation_deg, cam.GetRotation()));
        cam.SetFieldOfView(fov_deg);
        cam.SetClipPlanes(near_clip, far_clip);
        if (which == 1) app->renderer.SetRuntimeCameraReady(ready != 0);
        return TRI_OK;
    });
}

int trident_app_set_viewport(trident_app* app, uint32_t viewport_id, uint32_t width, uint32_t height) {
    return Guard(app, [&] {
        if (width > TRI_MAX_DIM || height > TRI_MAX_DIM) return TRI_E_INVALID;
        ViewportInfo info;
        info.Size = {(float)width, (float)height};
        app->renderer.SetViewport(viewport_id, info);
        // The viewport panel resizes the camera that renders into it (ApplicationLayer.cpp:253-290).
        if (width && height) {
            glm::vec2 s{(float)width, (float)height};
            if (app->renderer.IsViewportRecording() && app->renderer.GetRecordingViewportId() == viewport_id) {
                uint32_t rw = 0, rh = 0;  // the recorded viewport keeps the recording extent, and so does its camera
                app->renderer.GetRecordingExtent(rw, rh);
                s = glm::vec2{(float)rw, (float)rh};
            }
            if (viewport_id == 2u) app->runtime.SetViewportSize(s);
            else app->editor.SetViewportSize(s);
        }
        return TRI_OK;
    });
}

int trident_app_set_clear_color(trident_app* app, const float rgba[4]) {
    return Guard(app, [&] {
        if (!rgba) return TRI_E_INVALID;
        app->renderer.SetClearColor({rgba[0], rgba[1], rgba[2], rgba[3]});
        return TRI_OK;
    });
}

int trident_app_set_skybox(trident_app* app, const uint8_t* faces, uint32_t size) {
    return Guard(app, [&] {
        if (!faces || !size) return TRI_E_INVALID;
        Loader::CubemapTextureData d;
        d.m_Width = d.m_Height = size;
        d.m_PixelData.assign(faces, faces + 6ull * size * size * 4);
        return app->renderer.SetSkyboxCubemap(d) ? TRI_OK : TRI_E_INVALID;
    });
}

int trident_app_import_model(trident_app* app, const char* path, uint32_t* entities, uint32_t capacity,
                             uint32_t* count) {
    return Guard(app, [&] {
        if (!path) return TRI_E_INVALID;
        std::vector<ECS::Entity> spawned;
        const bool ok = ImportModel(app->renderer, app->registry, path, &spawned);
        if (count) *count = (uint32_t)spawned.size();
        for (size_t i = 0; entities && i < spawned.size() && i < capacity; ++i) entities[i] = spawned[i];
        return ok ? TRI_OK : TRI_E_INVALID;
    });
}

int trident_app_save_scene(trident_app* app, const char* path, const char* scene_name) {
    return Guard(app, [&] {
        if (!path) return TRI_E_INVALID;
        Scene scene(app->registry, &app->renderer, scene_name ? scene_name : "Untitled");
        scene.Save(path);
        return TRI_OK;
    });
}

int trident_app_load_scene(trident_app* app, const char* path, uint32_t* entity_count) {
    return Guard(app, [&] {
        if (!path) return TRI_E_INVALID;
        Scene scene(app->registry, &app->renderer);
        if (!scene.Load(path)) return TRI_E_INVALID;
        if (entity_count) *entity_count = (uint32_t)scene.GetLoadedEntityCount();
        return TRI_OK;
    });
}

int trident_app_use_scene_camera(trident_app* app) {
    return Guard(app, [&] {
        ECS::Entity chosen = 0;
        bool found = false;
        for (ECS::Entity e : app->registry.GetEntities()) {
            if (!app->registry.HasComponent<CameraComponent>(e)) continue;
            if (!found || app->registry.GetComponent<CameraComponent>(e).m_Primary) {
                const bool primary = app->registry.GetComponent<CameraComponent>(e).m_Primary;
                if (!found || primary) chosen = e;
                found = true;
                if (primary) break;
            }
        }
        if (!found) return TRI_E_INVALID;
        const CameraComponent& c = app->registry.GetComponent<CameraComponent>(chosen);
        RuntimeCamera& cam = app->runtime;
        if (app->registry.HasComponent<Transform>(chosen)) {
            const Transform& t = app->registry.GetComponent<Transform>(chosen);
            cam.SetPosition(t.Position);
            cam.SetRotation(t.Rotation);
        }
        cam.SetProjectionType(c.m_ProjectionType);
        cam.SetFieldOfView(c.m_FieldOfView);
        cam.SetOrthographicSize(c.m_OrthographicSize);
        cam.SetClipPlanes(c.m_NearClip, c.m_FarClip);
        app->renderer.SetRuntimeCameraReady(true);
        return TRI_OK;
    });
}

int trident_app_entity_transform(trident_app* app, uint32_t entity, float out[9]) {
    return Guard(app, [&] {
        if (!out || !app->registry.HasComponent<Transform>(entity)) return TRI_E_INVALID;
        const Transform& t = app->registry.GetComponent<Transform>(entity);
        const float v[9] = {t.Position.x, t.Position.y, t.Position.z, t.Rotation.x, t.Rotation.y,
                            t.Rotation.z, t.Scale.x, t.Scale.y, t.Scale.z};
        std::memcpy(out, v, sizeof v);
        return TRI_OK;
    });
}

int trident_app_entity_mesh(trident_app* app, uint32_t entity, uint64_t out[3]) {
    return Guard(app, [&] {
        if (!out || !app->registry.HasComponent<MeshComponent>(entity)) return TRI_E_INVALID;
        const MeshComponent& m = app->registry.GetComponent<MeshComponent>(entity);
        out[0] = (uint64_t)m.m_MeshIndex;
        out[1] = (uint64_t)m.m_Primitive;
        out[2] = (uint64_t)m.m_SourceMeshIndex;
        return TRI_OK;
    });
}

int trident_app_entity_count(trident_app* app, uint32_t* count) {
    return Guard(app, [&] {
        if (!count) return TRI_E_INVALID;
        *count = (uint32_t)app->registry.GetEntities().size();
        return TRI_OK;
    });
}

int trident_app_set_present_extent(trident_app* app, uint32_t width, uint32_t height) {
    return Guard(app, [&] {
        if (width > TRI_MAX_DIM || height > TRI_MAX_DIM) return TRI_E_INVALID;
        app->renderer.SetPresentExtent(width, height);
        return TRI_OK;
    });
}

int trident_app_set_ai_blend_strength(trident_app* app, float strength) {
    return Guard(app, [&] {
        app->renderer.SetAiBlendStrength(strength);
        return TRI_OK;
    });
}

int trident_app_submit_ai_frame(trident_app* app, const float* pixels, uint32_t width, uint32_t height, uint32_t channels) {
    return Guard(app, [&] {
        if (width > TRI_MAX_DIM || height > TRI_MAX_DIM || channels > 4) return TRI_E_INVALID;
        return app->renderer.SubmitAiInterpolation(pixels, width, height, channels) ? TRI_OK : TRI_E_INVALID;
    });
}

int trident_app_read_present(trident_app* app, uint8_t* rgba, uint32_t width, uint32_t height) {
    return Guard(app, [&] {
        if (!rgba) return TRI_E_INVALID;
        std::vector<uint8_t> px;
        uint32_t w = 0, h = 0;
        if (!app->renderer.ReadPresentPixels(px, w, h)) return TRI_E_STATE;
        if (w != width || h != height) return TRI_E_INVALID;
        std::memcpy(rgba, px.data(), px.size());
        return TRI_OK;
    });
}

int trident_app_draw_frame(trident_app* app) {
    return Guard(app, [&] {
        app->renderer.DrawFrame();
        return TRI_OK;
    });
}

int trident_app_set_frames_in_flight(trident_app* app, uint32_t n) {
    return Guard(app, [&] {
        if (n == 0 || n > 4) return TRI_E_INVALID;
        app->renderer.SetFramesInFlight(n);
        return TRI_OK;
    });
}

int trident_app_set_recording(trident_app* app, int enabled, uint32_t viewport_id, uint32_t width, uint32_t height,
                              const char* path, uint32_t out_extent[2]) {
    return Guard(app, [&] {
        if (enabled && !path) return TRI_E_INVALID;
        const bool ok = app->renderer.SetViewportRecordingEnabled(enabled != 0, viewport_id, width, height, path ? path : "");
        if (out_extent) app->renderer.GetRecordingExtent(out_extent[0], out_extent[1]);
        if (ok && enabled) {  // the panel now shows the recording extent: its camera follows (as set_viewport does)
            uint32_t rw = 0, rh = 0;
            app->renderer.GetRecordingExtent(rw, rh);
            const glm::vec2 s{(float)rw, (float)rh};
            if (viewport_id == 2u) app->runtime.SetViewportSize(s);
            else app->editor.SetViewportSize(s);
        }
        return ok ? TRI_OK : TRI_E_STATE;
    });
}

int trident_app_set_recording_quality(trident_app* app, int quality, int* out_quality) {
    return Guard(app, [&] {
        app->renderer.SetRecordingQuality(quality);
        if (out_quality) *out_quality = app->renderer.GetRecordingQuality();
        return TRI_OK;
    });
}

int trident_app_recording_state(trident_app* app, int* recording, uint64_t* frames) {
    return Guard(app, [&] {
        if (recording) *recording = app->renderer.IsViewportRecording() ? 1 : 0;
        if (frames) *frames = app->renderer.GetRecordedFrameCount();
        return TRI_OK;
    });
}

int trident_app_set_entity_id_output(trident_app* app, uint32_t viewport_id, int enabled) {
    return Guard(app, [&] {
        app->renderer.SetEntityIdOutputEnabled(viewport_id, enabled != 0);
        return TRI_OK;
    });
}

int trident_app_pick_entity(trident_app* app, uint32_t viewport_id, int32_t x, int32_t y, int* hit, uint32_t* entity,
                            float* depth01) {
    return Guard(app, [&] {
        if (!hit || !entity) return TRI_E_INVALID;
        ECS::Entity e = Renderer::kNoEntity;
        *hit = app->renderer.PickEntity(viewport_id, x, y, e, depth01) ? 1 : 0;
        *entity = e;
        return TRI_OK;
    });
}

int trident_app_pick_entities_in_rect(trident_app* app, uint32_t viewport_id, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                                      uint32_t* entities, uint32_t capacity, uint32_t* count) {
    return Guard(app, [&] {
        if (!count || (capacity && !entities)) return TRI_E_INVALID;
        const std::vector<ECS::Entity> found = app->renderer.PickEntitiesInRect(viewport_id, x0, y0, x1, y1);
        *count = (uint32_t)found.size();
        for (uint32_t i = 0; i < capacity && i < found.size(); ++i) entities[i] = found[i];
        return TRI_OK;
    });
}

int trident_app_read_entity_ids(trident_app* app, uint32_t viewport_id, uint32_t* entities, uint64_t capacity,
                                uint32_t background) {
    return Guard(app, [&] {
        if (!entities) return TRI_E_INVALID;
        std::vector<uint32_t> ids;
        if (!app->renderer.ReadViewportEntityIds(viewport_id, ids, background)) return TRI_E_STATE;
        if (ids.size() > capacity) return TRI_E_INVALID;
        std::memcpy(entities, ids.data(), ids.size() * sizeof(uint32_t));
        return TRI_OK;
    });
}

int trident_app_set_selected_entity(trident_app* app, uint32_t entity) {
    return Guard(app, [&] {
        app->renderer.SetSelectedEntity(entity);
        return TRI_OK;
    });
}

int trident_app_set_selection_outline(trident_app* app, int enabled, const float rgba[4], uint32_t width_px) {
    return Guard(app, [&] {
        if (enabled && !rgba) return TRI_E_INVALID;
        if (enabled) app->renderer.SetSelectionOutline(true, glm::vec4(rgba[0], rgba[1], rgba[2], rgba[3]), width_px);
        else app->renderer.SetSelectionOutline(false);
        const bool refused = enabled && (!app->renderer.IsSelectionOutlineEnabled() || width_px < 1 || width_px > 8);
        return refused ? TRI_E_STATE : TRI_OK;
    });
}

int trident_app_set_motion_vector_output(trident_app* app, uint32_t viewport_id, int enabled) {
    return Guard(app, [&] {
        app->renderer.SetMotionVectorOutputEnabled(viewport_id, enabled != 0);
        return app->renderer.IsMotionVectorOutputEnabled(viewport_id) == (enabled != 0) ? TRI_OK : TRI_E_STATE;
    });
}

int trident_app_read_motion_vectors(trident_app* app, uint32_t viewport_id, float* xy, uint64_t capacity) {
    return Guard(app, [&] {
        if (!xy) return TRI_E_INVALID;
        std::vector<float> m;
        if (!app->renderer.ReadViewportMotionVectors(viewport_id, m)) return TRI_E_STATE;
        if (m.size() > capacity) return TRI_E_INVALID;
        std::memcpy(xy, m.data(), m.size() * sizeof(float));
        return TRI_OK;
    });
}

int trident_app_motion_texture(trident_app* app, uint32_t viewport_id, tri_image* out) {
    return Guard(app, [&] {
        if (!out) return TRI_E_INVALID;
        const void* h = app->renderer.GetViewportMotionTexture(viewport_id);
        if (!h) return TRI_E_STATE;
        *out = *static_cast<const tri_image*>(h);
        return TRI_OK;
    });
}

int trident_app_set_history_reprojection(trident_app* app, uint32_t viewport_id, int enabled, float depth_tolerance) {
    return Guard(app, [&] {
        app->renderer.SetHistoryReprojectionEnabled(viewport_id, enabled != 0, depth_tolerance);
        return app->renderer.IsHistoryReprojectionEnabled(viewport_id) == (enabled != 0) ? TRI_OK : TRI_E_STATE;
    });
}

int trident_app_read_reprojection(trident_app* app, uint32_t viewport_id, uint8_t* bgra, uint8_t* mask, uint64_t capacity) {
    return Guard(app, [&] {
        if (!bgra || !mask) return TRI_E_INVALID;
        std::vector<uint8_t> c, m;
        if (!app->renderer.ReadViewportReprojection(viewport_id, c, m)) return TRI_E_STATE;
        if (m.size() > capacity) return TRI_E_INVALID;
        std::memcpy(bgra, c.data(), c.size());
        std::memcpy(mask, m.data(), m.size());
        return TRI_OK;
    });
}

int trident_app_reprojection_textures(trident_app* app, uint32_t viewport_id, tri_image* colour, tri_image* mask) {
    return Guard(app, [&] {
        if (!colour || !mask) return TRI_E_INVALID;
        const void* c = app->renderer.GetViewportReprojectedTexture(viewport_id);
        const void* m = app->renderer.GetViewportDisocclusionTexture(viewport_id);
        if (!c || !m) return TRI_E_STATE;
        *colour = *static_cast<const tri_image*>(c);
        *mask = *static_cast<const tri_image*>(m);
        return TRI_OK;
    });
}

int trident_app_set_temporal_anti_aliasing(trident_app* app, uint32_t viewport_id, int enabled, float alpha, uint32_t period,
                                           int reject_ids) {
    return Guard(app, [&] {
        app->renderer.SetTemporalAntiAliasingEnabled(viewport_id, enabled != 0, alpha, period, reject_ids != 0);
        // (a refused request leaves the switch as it was: on, perhaps, with its earlier values)
        if (enabled && (!(alpha > 0.0f && alpha <= 1.0f) || period > 64)) return TRI_E_STATE;
        return app->renderer.IsTemporalAntiAliasingEnabled(viewport_id) == (enabled != 0) ? TRI_OK : TRI_E_STATE;
    });
}

int trident_app_is_temporal_anti_aliasing(trident_app* app, uint32_t viewport_id, int* enabled) {
    return Guard(app, [&] {
        if (!enabled) return TRI_E_INVALID;
        *enabled = app->renderer.IsTemporalAntiAliasingEnabled(viewport_id) ? 1 : 0;
        return TRI_OK;
    });
}

int trident_app_read_resolved(trident_app* app, uint32_t viewport_id, uint8_t* rgba, uint8_t* mask, uint64_t capacity) {
    return Guard(app, [&] {
        std::vector<uint8_t> c, m;
        if (rgba) {
            if (!app->renderer.ReadViewportResolvedPixels(viewport_id, c)) return TRI_E_STATE;
            if (c.size() / 4 > capacity) return TRI_E_INVALID;
            std::memcpy(rgba, c.data(), c.size());
        }
        if (mask) {
            if (!app->renderer.ReadViewportTaaMask(viewport_id, m)) return TRI_E_STATE;
            if (m.size() > capacity) return TRI_E_INVALID;
            std::memcpy(mask, m.data(), m.size());
        }
        return TRI_OK;
    });
}

int trident_app_resolved_texture(trident_app* app, uint32_t viewport_id, tri_image* out) {
    return Guard(app, [&] {
        if (!out) return TRI_E_INVALID;
        const void* c = app->renderer.GetViewportResolvedTexture(viewport_id);
        if (!c) return TRI_E_STATE;
        *out = *static_cast<const tri_image*>(c);
        return TRI_OK;
    });
}

int trident_app_set_temporal_upscaling(trident_app* app, uint32_t viewport_id, int enabled, float render_scale, float alpha,
                                       int reject_ids) {
    return Guard(app, [&] {
        // (a refused request leaves the switch as it was: on, perhaps, with its earlier values)
        return app->renderer.SetTemporalUpscalingEnabled(viewport_id, enabled != 0, render_scale, alpha, reject_ids != 0) ? TRI_OK
                                                                                                                         : TRI_E_STATE;
    });
}

int trident_app_is_temporal_upscaling(trident_app* app, uint32_t viewport_id, int* enabled) {
    return Guard(app, [&] {
        if (!enabled) return TRI_E_INVALID;
        *enabled = app->renderer.IsTemporalUpscalingEnabled(viewport_id) ? 1 : 0;
        return TRI_OK;
    });
}

int trident_app_read_upscaled(trident_app* app, uint32_t viewport_id, uint8_t* rgba, uint8_t* mask, uint64_t capacity) {
    return Guard(app, [&] {
        std::vector<uint8_t> c, m;
        if (rgba) {
            if (!app->renderer.ReadViewportUpscaledPixels(viewport_id, c)) return TRI_E_STATE;
            if (c.size() / 4 > capacity) return TRI_E_INVALID;
            std::memcpy(rgba, c.data(), c.size());
        }
        if (mask) {
            if (!app->renderer.ReadViewportUpscaleMask(viewport_id, m)) return TRI_E_STATE;
            if (m.size() > capacity) return TRI_E_INVALID;
            std::memcpy(mask, m.data(), m.size());
        }
        return TRI_OK;
    });
}

int trident_app_upscaled_texture(trident_app* app, uint32_t viewport_id, tri_image* out) {
    return Guard(app, [&] {
        if (!out) return TRI_E_INVALID;
        const void* c = app->renderer.GetViewportUpscaledTexture(viewport_id);
        if (!c) return TRI_E_STATE;
        *out = *static_cast<const tri_image*>(c);
        return TRI_OK;
    });
}

struct trident_font {
    TextRenderer text;
};

int trident_app_submit_text(trident_app* app, uint32_t viewport_id, const float position[2], const float color[4],
                            const char* text, uint32_t bytes) {
    return Guard(app, [&] {
        if (!position || !color || (bytes && !text)) return TRI_E_INVALID;
        app->renderer.SubmitText(viewport_id, glm::vec2(position[0], position[1]),
                                 glm::vec4(color[0], color[1], color[2], color[3]), std::string(text ? text : "", bytes));
        return TRI_OK;
    });
}

int trident_app_set_font(trident_app* app, const char* path, float pixel_height) {
    return Guard(app, [&] {
        if (!path) return TRI_E_INVALID;
        return app->renderer.SetTextFont(path, pixel_height) ? TRI_OK : TRI_E_STATE;
    });
}

int trident_font_create(trident_font** out) {
    if (!out) return TRI_E_INVALID;
    *out = nullptr;
    try {
        *out = new trident_font();
        return TRI_OK;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

void trident_font_destroy(trident_font* font) { delete font; }

int trident_font_load(trident_font* font, const char* path, float pixel_height) {
    if (!font || !path) return TRI_E_INVALID;
    try {
        return font->text.LoadFontFile(path, pixel_height) ? TRI_OK : TRI_E_STATE;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

int trident_font_load_memory(trident_font* font, const uint8_t* data, uint64_t size, float pixel_height) {
    if (!font || !data) return TRI_E_INVALID;
    try {
        return font->text.LoadFontMemory(data, (size_t)size, pixel_height) ? TRI_OK : TRI_E_STATE;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

int trident_font_atlas(trident_font* font, uint8_t* out, uint64_t capacity, uint32_t* width, uint32_t* height) {
    if (!font) return TRI_E_INVALID;
    if (!font->text.IsLoaded()) return TRI_E_STATE;
    if (width) *width = TextRenderer::s_AtlasSize;
    if (height) *height = TextRenderer::s_AtlasSize;
    if (!out) return TRI_OK;
    const std::vector<uint8_t>& a = font->text.AtlasPixels();
    if (capacity < a.size()) return TRI_E_INVALID;
    std::memcpy(out, a.data(), a.size());
    return TRI_OK;
}

int trident_font_glyph(trident_font* font, uint32_t codepoint, float out[9]) {
    if (!font || !out) return TRI_E_INVALID;
    if (!font->text.IsLoaded()) return TRI_E_STATE;
    const TextRenderer::Glyph& g = font->text.ResolveGlyph((char32_t)codepoint);
    const float v[9] = {g.m_Offset.x, g.m_Offset.y, g.m_Size.x, g.m_Size.y, g.m_UVMin.x, g.m_UVMin.y,
                        g.m_UVMax.x, g.m_UVMax.y, g.m_Advance};
    std::memcpy(out, v, sizeof v);
    return TRI_OK;
}

int trident_font_metrics(trident_font* font, float out[3]) {
    if (!font || !out) return TRI_E_INVALID;
    if (!font->text.IsLoaded()) return TRI_E_STATE;
    out[0] = font->text.GetLineAdvance();
    out[1] = font->text.GetScale();
    out[2] = font->text.GetFontPixelHeight();
    return TRI_OK;
}

int trident_font_layout(trident_font* font, const float position[2], const float color[4], const char* text,
                        uint32_t bytes, tri_text_quad* out, uint32_t capacity, uint32_t* count) {
    if (!font || !position || !color || !count || (bytes && !text)) return TRI_E_INVALID;
    if (!font->text.IsLoaded()) return TRI_E_STATE;
    try {
        std::vector<tri_text_quad> quads;
        font->text.LayoutText(glm::vec2(position[0], position[1]), glm::vec4(color[0], color[1], color[2], color[3]),
                              std::string_view(text ? text : "", bytes), quads);
        *count = (uint32_t)quads.size();
        if (quads.size() > capacity || (!quads.empty() && !out)) return TRI_E_INVALID;
        if (!quads.empty()) std::memcpy(out, quads.data(), quads.size() * sizeof(tri_text_quad));
        return TRI_OK;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

struct trident_video {
    VideoEncoder encoder;
};

int trident_video_create(trident_video** out) {
    if (!out) return TRI_E_INVALID;
    *out = nullptr;
    try {
        *out = new trident_video();
        return TRI_OK;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

void trident_video_destroy(trident_video* video) { delete video; }

int trident_video_begin(trident_video* video, const char* path, uint32_t width, uint32_t height, uint32_t fps) {
    if (!video || !path) return TRI_E_INVALID;
    try {
        return video->encoder.BeginSession(path, width, height, fps) ? TRI_OK : TRI_E_STATE;
    } catch (const std::exception&) {
        return TRI_E_INVALID;
    }
}

int trident_video_submit_rgba(trident_video* video, const uint8_t* rgba, uint64_t bytes, uint32_t width, uint32_t height) {
    if (!video) return TRI_E_INVALID;
    try {
        VideoEncoder::RecordedFrame frame;
        if (rgba && bytes) frame.m_Pixels.assign(rgba, rgba + bytes);
        frame.m_Width = width;
        frame.m_Height = height;
        return video->encoder.SubmitFrame(frame) ? TRI_OK : TRI_E_STATE;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

int trident_video_submit_planes(trident_video* video, const uint8_t* yuv, uint32_t width, uint32_t height) {
    if (!video) return TRI_E_INVALID;
    return video->encoder.SubmitPlanes(yuv, width, height) ? TRI_OK : TRI_E_STATE;
}

int trident_video_submit_jpeg(trident_video* video, const uint8_t* jpeg, uint64_t bytes, uint32_t width, uint32_t height) {
    if (!video) return TRI_E_INVALID;
    try {
        return video->encoder.SubmitJpeg(jpeg, bytes, width, height) ? TRI_OK : TRI_E_STATE;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

int trident_video_set_quality(trident_video* video, uint32_t quality) {
    if (!video) return TRI_E_INVALID;
    return video->encoder.SetQuality(quality) ? TRI_OK : TRI_E_INVALID;
}

int trident_video_set_restart_interval(trident_video* video, uint32_t restart_mcus) {
    if (!video) return TRI_E_INVALID;
    return video->encoder.SetRestartInterval(restart_mcus) ? TRI_OK : TRI_E_INVALID;
}

int trident_video_end(trident_video* video) {
    if (!video) return TRI_E_INVALID;
    return video->encoder.EndSession() ? TRI_OK : TRI_E_STATE;
}

int trident_video_state(trident_video* video, int* active, uint64_t* frames) {
    if (!video) return TRI_E_INVALID;
    if (active) *active = video->encoder.IsSessionActive() ? 1 : 0;
    if (frames) *frames = video->encoder.GetFrameCount();
    return TRI_OK;
}

int trident_video_convert_rgba(const uint8_t* rgba, uint64_t pixels, uint8_t* yuv) {
    if (pixels && (!rgba || !yuv)) return TRI_E_INVALID;
    VideoEncoder::ConvertRgbaToYuv444(rgba, pixels, yuv);
    return TRI_OK;
}

int trident_app_set_dataset_capture(trident_app* app, int enabled, const char* directory, uint32_t interval) {
    return Guard(app, [&] {
        if (directory) app->renderer.SetFrameDatasetCaptureDirectory(directory);
        if (interval) app->renderer.SetFrameDatasetCaptureInterval(interval);
        app->renderer.SetFrameDatasetCaptureEnabled(enabled != 0);
        return TRI_OK;
    });
}

int trident_app_dataset_capture_state(trident_app* app, int* enabled, uint32_t* interval, char* directory, uint32_t capacity) {
    return Guard(app, [&] {
        if (enabled) *enabled = app->renderer.IsFrameDatasetCaptureEnabled() ? 1 : 0;
        if (interval) *interval = app->renderer.GetFrameDatasetCaptureInterval();
        if (directory) {
            const std::string& d = app->renderer.GetFrameDatasetCaptureDirectory();
            if (d.size() + 1 > capacity) return TRI_E_INVALID;
            std::memcpy(directory, d.c_str(), d.size() + 1);
        }
        return TRI_OK;
    });
}

int trident_app_set_ai_readback(trident_app* app, int enabled, uint32_t readback_ms, uint32_t inference_ms) {
    return Guard(app, [&] {
        app->renderer.SetAiThrottleIntervals(readback_ms, inference_ms);
        return app->renderer.SetAiReadbackEnabled(enabled != 0) ? TRI_OK : TRI_E_STATE;
    });
}

int trident_app_ai_readback_state(trident_app* app, int* enabled) {
    return Guard(app, [&] {
        if (enabled) *enabled = app->renderer.IsAiReadbackEnabled() ? 1 : 0;
        return TRI_OK;
    });
}

int trident_app_acquire_frame(trident_app* app, float* out, uint64_t capacity, uint32_t* width, uint32_t* height, int* got) {
    return Guard(app, [&] {
        if (!got) return TRI_E_INVALID;
        *got = 0;
        uint32_t w = 0, h = 0;
        app->renderer.GetFrameReadbackExtent(w, h);
        if (width) *width = w;
        if (height) *height = h;
        // (checked before the acquisition: a tensor that does not fit stays pending)
        if (!out || capacity < (uint64_t)w * h * 4u) return w && h ? TRI_E_INVALID : TRI_OK;
        *got = app->renderer.TryAcquireRenderedFrame(out, (size_t)capacity) ? 1 : 0;
        return TRI_OK;
    });
}

int trident_app_readback_device_tensor(trident_app* app, const float** device, uint32_t* width, uint32_t* height, int* got) {
    return Guard(app, [&] {
        if (!device || !got) return TRI_E_INVALID;
        uint32_t w = 0, h = 0;
        *device = nullptr;
        *got = app->renderer.GetFrameReadbackDeviceTensor(device, w, h) ? 1 : 0;
        if (width) *width = w;
        if (height) *height = h;
        return TRI_OK;
    });
}

int trident_app_submit_ai_output(trident_app* app, const float* data, uint64_t count, const int64_t* shape, uint32_t rank) {
    return Guard(app, [&] { return app->renderer.SubmitAiOutput(data, (size_t)count, shape, rank) ? TRI_OK : TRI_E_STATE; });
}

int trident_app_load_ai_model(trident_app* app, const char* path, char* message, uint32_t capacity) {
    return Guard(app, [&] {
        if (message && capacity) message[0] = '\0';
        if (!path) return TRI_E_INVALID;
        const bool multi = app->renderer.GetDeviceCount() > 1;  // refused before the file is looked at
        if (app->renderer.LoadAiModel(path)) return TRI_OK;
        if (multi) return TRI_E_STATE;
        const std::string& err = app->renderer.GetAiModelError();
        if (message && capacity) {
            const size_t n = std::min<size_t>(err.size(), capacity - 1);
            std::memcpy(message, err.data(), n);
            message[n] = '\0';
        }
        return TRI_E_INVALID;
    });
}

int trident_app_resolve_ai_model_path(trident_app* app, char* path, uint32_t capacity, int* found) {
    return Guard(app, [&] {
        const std::string p = app->renderer.ResolveAiModelPath();
        if (found) *found = p.empty() ? 0 : 1;
        if (path && capacity) path[0] = '\0';
        if (p.empty() || !path) return TRI_OK;
        if (p.size() + 1 > capacity) return TRI_E_INVALID;
        std::memcpy(path, p.c_str(), p.size() + 1);
        return TRI_OK;
    });
}

int trident_app_try_initialise_ai_model(trident_app* app, int* initialised) {
    return Guard(app, [&] {
        const bool ok = app->renderer.TryInitialiseAiModel();
        if (initialised) *initialised = ok ? 1 : 0;
        return TRI_OK;
    });
}

int trident_app_ai_debug_stats(trident_app* app, trident_ai_debug_stats* out) {
    return Guard(app, [&] {
        if (!out) return TRI_E_INVALID;
        const Renderer::AiDebugStats s = app->renderer.GetAiDebugStats();
        out->model_initialised = s.m_ModelInitialised ? 1 : 0;
        out->pending_job_count = (uint32_t)s.m_PendingJobCount;
        out->completed_inference_count = s.m_CompletedInferenceCount;
        out->last_inference_ms = s.m_LastInferenceMilliseconds;
        out->average_inference_ms = s.m_AverageInferenceMilliseconds;
        out->texture_ready = s.m_TextureReady ? 1 : 0;
        out->blend_strength = s.m_BlendStrength;
        out->texture_width = s.m_TextureExtent.width;
        out->texture_height = s.m_TextureExtent.height;
        out->reserved_metric = s.m_ReservedMetric;
        return TRI_OK;
    });
}

int trident_app_ai_model_info(trident_app* app, int* initialised, int64_t input_shape[4], int64_t output_shape[4]) {
    return Guard(app, [&] {
        const AI::FrameGenerator& g = app->renderer.GetFrameGenerator();
        if (initialised) *initialised = g.IsInitialised() ? 1 : 0;
        const std::vector<int64_t> in = g.GetPrimaryInputShape(), out = g.GetPrimaryOutputShape();
        for (size_t i = 0; i < 4; ++i) {
            if (input_shape) input_shape[i] = i < in.size() ? in[i] : 0;
            if (output_shape) output_shape[i] = i < out.size() ? out[i] : 0;
        }
        return TRI_OK;
    });
}

int trident_app_finish_ai_inference(trident_app* app, uint32_t timeout_ms, int* finished) {
    return Guard(app, [&] {
        const bool ok = app->renderer.FinishAiInference(timeout_ms);
        if (finished) *finished = ok ? 1 : 0;
        return TRI_OK;
    });
}

int trident_app_read_ai_blend_frame(trident_app* app, uint8_t* rgba, uint64_t capacity, uint32_t* width, uint32_t* height) {
    return Guard(app, [&] {
        std::vector<uint8_t> px;
        uint32_t w = 0, h = 0;
        if (!app->renderer.ReadAiBlendFrame(px, w, h)) return TRI_E_STATE;
        if (width) *width = w;
        if (height) *height = h;
        if (!rgba || capacity < px.size()) return TRI_E_INVALID;
        std::memcpy(rgba, px.data(), px.size());
        return TRI_OK;
    });
}

int trident_ai_normalise_output(float* data, uint64_t count, int64_t channels) {
    if (count && !data) return TRI_E_INVALID;
    try {
        std::vector<float> v(data, data + count);
        Renderer::NormaliseAndReorderAiOutput(v, channels);
        if (count) std::memcpy(data, v.data(), count * sizeof(float));
        return TRI_OK;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

struct trident_dataset {
    FrameDatasetRecorder recorder;
};

int trident_dataset_create(trident_dataset** out) {
    if (!out) return TRI_E_INVALID;
    *out = nullptr;
    try {
        *out = new trident_dataset();
        return TRI_OK;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

void trident_dataset_destroy(trident_dataset* dataset) { delete dataset; }

int trident_dataset_set_directory(trident_dataset* dataset, const char* directory) {
    return GuardDataset(dataset, [&] { dataset->recorder.SetCaptureDirectory(directory ? directory : ""); });
}

int trident_dataset_set_interval(trident_dataset* dataset, uint32_t interval) {
    return GuardDataset(dataset, [&] { dataset->recorder.SetSampleInterval(interval); });
}

int trident_dataset_enable(trident_dataset* dataset, int enabled) {
    return GuardDataset(dataset, [&] { dataset->recorder.EnableCapture(enabled != 0); });
}

int trident_dataset_reset(trident_dataset* dataset) {
    return GuardDataset(dataset, [&] { dataset->recorder.Reset(); });
}

int trident_dataset_record_input(trident_dataset* dataset, const float* data, uint64_t count, uint32_t width, uint32_t height,
                                 uint32_t channels, const int64_t* shape, uint32_t rank) {
    return GuardDataset(dataset, [&] {
        dataset->recorder.RecordInputFrame(data, (size_t)count, width, height, channels, shape, rank);
    });
}

int trident_dataset_record_output(trident_dataset* dataset, const float* data, uint64_t count, const int64_t* shape,
                                  uint32_t rank) {
    return GuardDataset(dataset, [&] { dataset->recorder.RecordAiOutput(data, (size_t)count, shape, rank); });
}

int trident_dataset_flush(trident_dataset* dataset) {
    return GuardDataset(dataset, [&] { dataset->recorder.Flush(); });
}

int trident_dataset_state(trident_dataset* dataset, int* enabled, uint32_t* interval, uint64_t* next_index, uint64_t* pending) {
    if (!dataset) return TRI_E_INVALID;
    if (enabled) *enabled = dataset->recorder.IsCaptureEnabled() ? 1 : 0;
    if (interval) *interval = dataset->recorder.GetSampleInterval();
    if (next_index) *next_index = dataset->recorder.GetNextSampleIndex();
    if (pending) *pending = dataset->recorder.GetPendingSampleCount();
    return TRI_OK;
}

int trident_dataset_write_npy(const char* path, const float* data, uint64_t count, const int64_t* shape, uint32_t rank) {
    if (!path) return TRI_E_INVALID;
    try {
        return FrameDatasetRecorder::WriteNpyFile(path, data, (size_t)count, shape, rank) ? TRI_OK : TRI_E_STATE;
    } catch (const std::exception&) {
        return TRI_E_INVALID;
    }
}

int trident_app_finish_frame(trident_app* app) {
    return Guard(app, [&] {
        app->renderer.FinishFrame();
        return TRI_OK;
    });
}

int trident_app_read_pixels(trident_app* app, uint32_t viewport_id, uint8_t* rgba, float* depth) {
    return Guard(app, [&] {
        if (!rgba) return TRI_E_INVALID;
        std::vector<uint8_t> px;
        std::vector<float> d;
        if (!app->renderer.ReadViewportPixels(viewport_id, px, depth ? &d : nullptr)) return TRI_E_STATE;
        std::memcpy(rgba, px.data(), px.size());
        if (depth) std::memcpy(depth, d.data(), d.size() * sizeof(float));
        return TRI_OK;
    });
}

int trident_app_frame_inputs(trident_app* app, uint32_t viewport_id, tri_global_ubo* ubo, tri_draw* draws,
                             uint32_t capacity, uint32_t* draw_count) {
    return Guard(app, [&] {
        if (!ubo || !draw_count) return TRI_E_INVALID;
        std::vector<tri_draw> list;
        if (!app->renderer.BuildFrameInputs(viewport_id, *ubo, list)) return TRI_E_STATE;
        *draw_count = (uint32_t)list.size();
        if (list.size() > capacity || (!draws && !list.empty())) return list.size() > capacity ? TRI_E_OVERFLOW : TRI_E_INVALID;
        if (!list.empty()) std::memcpy(draws, list.data(), list.size() * sizeof(tri_draw));
        return TRI_OK;
    });
}

int trident_app_geometry(trident_app* app, const tri_vertex** vertices, size_t* vertex_count,
                         const uint32_t** indices, size_t* index_count, tri_mesh_range* ranges, uint32_t capacity,
                         uint32_t* range_count) {
    return Guard(app, [&] {
        if (!vertices || !vertex_count || !indices || !index_count || !range_count) return TRI_E_INVALID;
        *vertices = app->renderer.GetVertexBuffer().data();
        *vertex_count = app->renderer.GetVertexBuffer().size();
        *indices = app->renderer.GetIndexBuffer().data();
        *index_count = app->renderer.GetIndexBuffer().size();
        const std::vector<tri_mesh_range> r = app->renderer.GetMeshRanges();
        *range_count = (uint32_t)r.size();
        if (r.size() > capacity) return TRI_E_OVERFLOW;
        if (!r.empty() && ranges) std::memcpy(ranges, r.data(), r.size() * sizeof(tri_mesh_range));
        return TRI_OK;
    });
}

int trident_app_materials(trident_app* app, tri_material_record* out, uint32_t capacity, uint32_t* count) {
    return Guard(app, [&] {
        if (!count) return TRI_E_INVALID;
        const auto& mats = app->renderer.GetMaterials();
        *count = (uint32_t)mats.size();
        if (mats.size() > capacity) return TRI_E_OVERFLOW;
        for (size_t i = 0; i < mats.size() && out; ++i)
            out[i] = {{mats[i].BaseColorFactor.x, mats[i].BaseColorFactor.y, mats[i].BaseColorFactor.z,
                       mats[i].BaseColorFactor.w},
                      {mats[i].MetallicFactor, mats[i].RoughnessFactor, 1.0f, 0.0f}};
        return TRI_OK;
    });
}

int trident_app_frame_timing(trident_app* app, double out[7]) {
    return Guard(app, [&] {
        if (!out) return TRI_E_INVALID;
        const FrameTimingStats& s = app->renderer.GetFrameTimingStats();
        out[0] = s.MinimumMilliseconds;
        out[1] = s.MaximumMilliseconds;
        out[2] = s.AverageMilliseconds;
        out[3] = s.MinimumFPS;
        out[4] = s.MaximumFPS;
        out[5] = s.AverageFPS;
        out[6] = (double)app->renderer.GetFrameTimingHistoryCount();
        return TRI_OK;
    });
}

}  // extern "C"

namespace {

glm::mat4 Mat4From(const float* m) {
    glm::mat4 r(1.0f);
    for (int c = 0; c < 4; ++c)
        for (int k = 0; k < 4; ++k) r[c][k] = m[4 * c + k];
    return r;
}

size_t AnimHandle(uint64_t handle) {
    return handle == UINT64_MAX ? Animation::AnimationAssetService::s_InvalidHandle : (size_t)handle;
}

size_t AnimClip(uint32_t clip) { return clip == UINT32_MAX ? Animation::AnimationAssetService::s_InvalidHandle : (size_t)clip; }

// trident_sm_* / trident_node_*: machines and not yet attached blend-tree nodes by id
std::unordered_map<uint64_t, std::shared_ptr<Animation::AnimationStateMachine>> g_machines;
std::unordered_map<uint64_t, std::unique_ptr<Animation::AnimationBlendNode>> g_nodes;
uint64_t g_next_graph_id = 1;

Animation::AnimationStateMachine* Machine(uint64_t id) {
    auto found = g_machines.find(id);
    return found == g_machines.end() ? nullptr : found->second.get();
}

// Takes the node out of the table: 0 is "no node"; an unknown id sets *ok to false.
std::unique_ptr<Animation::AnimationBlendNode> TakeNode(uint64_t id, bool* ok) {
    if (!id) return nullptr;
    auto found = g_nodes.find(id);
    if (found == g_nodes.end()) {
        *ok = false;
        return nullptr;
    }
    std::unique_ptr<Animation::AnimationBlendNode> node = std::move(found->second);
    g_nodes.erase(found);
    return node;
}

uint64_t KeepNode(std::unique_ptr<Animation::AnimationBlendNode> node) {
    const uint64_t id = g_next_graph_id++;
    g_nodes[id] = std::move(node);
    return id;
}

int CopyName(const std::string& name, char* out, uint32_t capacity) {
    if (!out) return TRI_OK;
    if (capacity < name.size() + 1) return TRI_E_INVALID;
    std::memcpy(out, name.c_str(), name.size() + 1);
    return TRI_OK;
}

template <typename F>
int GuardAnim(F&& f) {
    try {
        return f();
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

}  // namespace

extern "C" {

int trident_app_set_entity_animation(trident_app* app, uint32_t entity, const char* skeleton_asset_id,
                                     const char* animation_asset_id, const char* clip, float time, float speed,
                                     int looping, int playing) {
    return Guard(app, [&] {
        AnimationComponent& a = app->registry.HasComponent<AnimationComponent>(entity)
                                    ? app->registry.GetComponent<AnimationComponent>(entity)
                                    : app->registry.AddComponent<AnimationComponent>(entity);
        a.m_SkeletonAssetId = skeleton_asset_id ? skeleton_asset_id : "";
        a.m_AnimationAssetId = animation_asset_id ? animation_asset_id : "";
        a.m_CurrentClip = clip ? clip : "";
        a.m_CurrentTime = time;
        a.m_PlaybackSpeed = speed;
        a.m_IsLooping = looping != 0;
        a.m_IsPlaying = playing != 0;
        return TRI_OK;
    });
}

int trident_app_set_entity_state_machine(trident_app* app, uint32_t entity, uint64_t machine) {
    return Guard(app, [&] {
        if (!app->registry.HasComponent<AnimationComponent>(entity)) return TRI_E_INVALID;
        AnimationComponent& a = app->registry.GetComponent<AnimationComponent>(entity);
        if (!machine) {
            a.m_StateMachine.reset();
            return TRI_OK;
        }
        auto found = g_machines.find(machine);
        if (found == g_machines.end()) return TRI_E_INVALID;
        a.m_StateMachine = found->second;  // shared: the id keeps driving its parameters
        return TRI_OK;
    });
}

int trident_app_update_animation(trident_app* app, float dt) {
    return Guard(app, [&] {
        app->animation.Update(app->registry, dt);
        return TRI_OK;
    });
}

int trident_app_initialise_pose(trident_app* app, uint32_t entity) {
    return Guard(app, [&] {
        if (!app->registry.HasComponent<AnimationComponent>(entity)) return TRI_E_INVALID;
        ECS::AnimationSystem::InitialisePose(app->registry.GetComponent<AnimationComponent>(entity));
        return TRI_OK;
    });
}

int trident_app_entity_pose(trident_app* app, uint32_t entity, float* out, uint32_t capacity, uint32_t* count) {
    return Guard(app, [&] {
        if (!count || !app->registry.HasComponent<AnimationComponent>(entity)) return TRI_E_INVALID;
        AnimationComponent& a = app->registry.GetComponent<AnimationComponent>(entity);
        if (app->renderer.PosesOnDevice(a)) ECS::AnimationSystem::EvaluatePose(a);
        *count = (uint32_t)a.m_BoneMatrices.size();
        if (!out) return TRI_OK;
        if (capacity < *count) return TRI_E_INVALID;
        for (size_t b = 0; b < a.m_BoneMatrices.size(); ++b)
            for (int c = 0; c < 4; ++c)
                for (int k = 0; k < 4; ++k) out[16 * b + 4 * c + k] = a.m_BoneMatrices[b][c][k];
        return TRI_OK;
    });
}

int trident_app_entity_animation_state(trident_app* app, uint32_t entity, float* time, int* playing, uint64_t handles[3]) {
    return Guard(app, [&] {
        if (!time || !playing || !handles || !app->registry.HasComponent<AnimationComponent>(entity)) return TRI_E_INVALID;
        const AnimationComponent& a = app->registry.GetComponent<AnimationComponent>(entity);
        *time = a.m_CurrentTime;
        *playing = a.m_IsPlaying ? 1 : 0;
        const size_t h[3] = {a.m_SkeletonAssetHandle, a.m_AnimationAssetHandle, a.m_CurrentClipIndex};
        for (int i = 0; i < 3; ++i) handles[i] = h[i] == Animation::AnimationAssetService::s_InvalidHandle ? UINT64_MAX : (uint64_t)h[i];
        return TRI_OK;
    });
}

int trident_app_set_device_pose(trident_app* app, int enabled) {
    return Guard(app, [&] {
        app->renderer.SetDevicePoseEnabled(enabled != 0);
        return TRI_OK;
    });
}

int trident_app_bone_palette_uploads(trident_app* app, uint64_t* count) {
    return Guard(app, [&] {
        if (!count) return TRI_E_INVALID;
        *count = app->renderer.GetBonePaletteUploadCount();
        return TRI_OK;
    });
}

int trident_anim_decompose(const float local_bind[16], float out[10]) {
    if (!local_bind || !out) return TRI_E_INVALID;
    const Animation::TransformDecomposition d = Animation::DecomposeBindTransform(Mat4From(local_bind));
    const float v[10] = {d.m_Translation.x, d.m_Translation.y, d.m_Translation.z, d.m_Rotation.w, d.m_Rotation.x,
                         d.m_Rotation.y, d.m_Rotation.z, d.m_Scale.x, d.m_Scale.y, d.m_Scale.z};
    std::memcpy(out, v, sizeof v);
    return TRI_OK;
}

int trident_anim_register(const char* asset_id, uint32_t bone_count, const int32_t* parents, const float* local_binds,
                          const float* inverse_binds, const char* const* source_names, int32_t root_index,
                          uint64_t* handle) {
    if (!asset_id || !handle || (bone_count && (!parents || !local_binds || !inverse_binds))) return TRI_E_INVALID;
    return GuardAnim([&] {
        Animation::Skeleton sk;
        sk.m_Bones.resize(bone_count);
        for (uint32_t b = 0; b < bone_count; ++b) {
            Animation::Bone& bone = sk.m_Bones[b];
            bone.m_SourceName = source_names && source_names[b] ? source_names[b] : "Bone" + std::to_string(b);
            bone.m_ParentIndex = parents[b];
            bone.m_LocalBindTransform = Mat4From(local_binds + 16 * (size_t)b);
            bone.m_InverseBindMatrix = Mat4From(inverse_binds + 16 * (size_t)b);
        }
        sk.m_RootBoneIndex = root_index;
        Animation::FinaliseSkeleton(sk);
        const size_t h = Animation::AnimationAssetService::Get().RegisterRuntimeAsset(asset_id, std::move(sk), {});
        if (h == Animation::AnimationAssetService::s_InvalidHandle) return TRI_E_INVALID;
        *handle = (uint64_t)h;
        return TRI_OK;
    });
}

int trident_anim_add_clip(uint64_t handle, const char* name, float duration, const tri_pose_channel* channels,
                          const int32_t* stored_bones, const char* const* source_names, uint32_t channel_count,
                          const float* vec_times, const float* vec_values, uint32_t vec_count, const float* quat_times,
                          const float* quat_values, uint32_t quat_count, uint32_t* clip_index) {
    if (!name || !clip_index || (channel_count && !channels) || (vec_count && (!vec_times || !vec_values)) ||
        (quat_count && (!quat_times || !quat_values)))
        return TRI_E_INVALID;
    return GuardAnim([&] {
        auto& service = Animation::AnimationAssetService::Get();
        const Animation::Skeleton* sk = service.GetSkeleton(AnimHandle(handle));
        const std::vector<Animation::AnimationClip>* have = service.GetAnimationClips(AnimHandle(handle));
        if (!sk || !have) return TRI_E_INVALID;
        Animation::AnimationClip clip;
        clip.m_Name = name;
        clip.m_DurationSeconds = duration;
        clip.m_TicksPerSecond = 1000.0f;
        auto vec_keys = [&](uint32_t first, uint32_t count, std::vector<Animation::VectorKeyframe>& out) {
            if ((uint64_t)first + count > vec_count) return false;
            for (uint32_t i = first; i < first + count; ++i)
                out.push_back({vec_times[i], glm::vec3(vec_values[3 * (size_t)i], vec_values[3 * (size_t)i + 1], vec_values[3 * (size_t)i + 2])});
            return true;
        };
        for (uint32_t c = 0; c < channel_count; ++c) {
            Animation::TransformChannel ch;
            ch.m_BoneIndex = stored_bones ? stored_bones[c] : (int)channels[c].bone;
            if (source_names && source_names[c]) ch.m_SourceBoneName = source_names[c];
            if (!vec_keys(channels[c].translation_first, channels[c].translation_count, ch.m_TranslationKeys) ||
                !vec_keys(channels[c].scale_first, channels[c].scale_count, ch.m_ScaleKeys) ||
                (uint64_t)channels[c].rotation_first + channels[c].rotation_count > quat_count)
                return TRI_E_INVALID;
            for (uint32_t i = channels[c].rotation_first; i < channels[c].rotation_first + channels[c].rotation_count; ++i)
                ch.m_RotationKeys.push_back({quat_times[i], glm::quat(quat_values[4 * (size_t)i], quat_values[4 * (size_t)i + 1],
                                                                      quat_values[4 * (size_t)i + 2], quat_values[4 * (size_t)i + 3])});
            clip.m_Channels.push_back(std::move(ch));
        }
        // re-register the asset under its id with the clip appended (the handle stays)
        std::string id;
        Animation::Skeleton skeleton = *sk;
        std::vector<Animation::AnimationClip> clips = *have;
        clips.push_back(std::move(clip));
        *clip_index = (uint32_t)clips.size() - 1;
        if (!service.AssetId(AnimHandle(handle), id)) return TRI_E_INVALID;
        return service.RegisterRuntimeAsset(id, std::move(skeleton), std::move(clips)) == AnimHandle(handle) ? TRI_OK : TRI_E_STATE;
    });
}

int trident_anim_load(const char* path, uint64_t* handle) {
    if (!path || !handle) return TRI_E_INVALID;
    return GuardAnim([&] {
        const size_t h = Animation::AnimationAssetService::Get().AcquireSkeleton(path);
        if (h == Animation::AnimationAssetService::s_InvalidHandle) return TRI_E_INVALID;
        *handle = (uint64_t)h;
        return TRI_OK;
    });
}

int trident_anim_describe(uint64_t handle, char* out, uint64_t capacity, uint64_t* needed) {
    if (!needed) return TRI_E_INVALID;
    return GuardAnim([&] {
        auto& service = Animation::AnimationAssetService::Get();
        const Animation::Skeleton* sk = service.GetSkeleton(AnimHandle(handle));
        const std::vector<Animation::AnimationClip>* clips = service.GetAnimationClips(AnimHandle(handle));
        if (!sk || !clips) return TRI_E_INVALID;
        std::string j;
        auto num = [&](float v) {
            char buf[40];
            if (std::isfinite(v)) std::snprintf(buf, sizeof buf, "%.9g", (double)v);
            else std::snprintf(buf, sizeof buf, "null");
            j += buf;
        };
        auto str = [&](const std::string& v) {
            j += '"';
            for (char c : v) {
                if (c == '"' || c == '\\') j += '\\';
                j += (unsigned char)c < 0x20 ? '?' : c;
            }
            j += '"';
        };
        auto mat = [&](const glm::mat4& m) {
            j += '[';
            for (int k = 0; k < 16; ++k) {
                if (k) j += ',';
                num(m[k / 4][k % 4]);
            }
            j += ']';
        };
        j += "{\"root\":" + std::to_string(sk->m_RootBoneIndex) + ",\"bones\":[";
        for (size_t b = 0; b < sk->m_Bones.size(); ++b) {
            const Animation::Bone& bone = sk->m_Bones[b];
            j += b ? ",{\"name\":" : "{\"name\":";
            str(bone.m_Name);
            j += ",\"source\":";
            str(bone.m_SourceName);
            j += ",\"parent\":" + std::to_string(bone.m_ParentIndex) + ",\"children\":[";
            for (size_t c = 0; c < bone.m_Children.size(); ++c) j += (c ? "," : "") + std::to_string(bone.m_Children[c]);
            j += "],\"local\":";
            mat(bone.m_LocalBindTransform);
            j += ",\"inverse\":";
            mat(bone.m_InverseBindMatrix);
            j += '}';
        }
        j += "],\"clips\":[";
        for (size_t c = 0; c < clips->size(); ++c) {
            const Animation::AnimationClip& clip = (*clips)[c];
            j += c ? ",{\"name\":" : "{\"name\":";
            str(clip.m_Name);
            j += ",\"duration\":";
            num(clip.m_DurationSeconds);
            j += ",\"ticks\":";
            num(clip.m_TicksPerSecond);
            j += ",\"channels\":[";
            for (size_t h = 0; h < clip.m_Channels.size(); ++h) {
                const Animation::TransformChannel& ch = clip.m_Channels[h];
                j += h ? ",{\"bone\":" : "{\"bone\":";
                j += std::to_string(ch.m_BoneIndex) + ",\"source\":";
                str(ch.m_SourceBoneName);
                auto vec = [&](const char* key, const std::vector<Animation::VectorKeyframe>& keys) {
                    j += std::string(",\"") + key + "\":[";
                    for (size_t k = 0; k < keys.size(); ++k) {
                        j += k ? ",[" : "[";
                        num(keys[k].m_TimeSeconds); j += ','; num(keys[k].m_Value.x); j += ','; num(keys[k].m_Value.y); j += ',';
                        num(keys[k].m_Value.z); j += ']';
                    }
                    j += ']';
                };
                vec("t", ch.m_TranslationKeys);
                j += ",\"r\":[";
                for (size_t k = 0; k < ch.m_RotationKeys.size(); ++k) {
                    const Animation::QuaternionKeyframe& q = ch.m_RotationKeys[k];
                    j += k ? ",[" : "[";
                    num(q.m_TimeSeconds); j += ','; num(q.m_Value.w); j += ','; num(q.m_Value.x); j += ','; num(q.m_Value.y); j += ',';
                    num(q.m_Value.z); j += ']';
                }
                j += ']';
                vec("s", ch.m_ScaleKeys);
                j += '}';
            }
            j += "]}";
        }
        j += "]}";
        *needed = j.size() + 1;
        if (!out) return TRI_OK;
        if (capacity < j.size() + 1) return TRI_E_INVALID;
        std::memcpy(out, j.c_str(), j.size() + 1);
        return TRI_OK;
    });
}

int trident_anim_clip_index(uint64_t handle, const char* name, uint32_t* clip_index) {
    if (!name || !clip_index) return TRI_E_INVALID;
    return GuardAnim([&] {
        const size_t i = Animation::AnimationAssetService::Get().ResolveClipIndex(AnimHandle(handle), name);
        if (i == Animation::AnimationAssetService::s_InvalidHandle) return TRI_E_INVALID;
        *clip_index = (uint32_t)i;
        return TRI_OK;
    });
}

int trident_anim_resolve_channels(uint64_t handle, uint32_t clip_index, int32_t* bones, uint32_t capacity, uint32_t* count) {
    if (!count) return TRI_E_INVALID;
    return GuardAnim([&] {
        auto& service = Animation::AnimationAssetService::Get();
        const Animation::Skeleton* sk = service.GetSkeleton(AnimHandle(handle));
        const Animation::AnimationClip* clip = service.GetClip(AnimHandle(handle), AnimClip(clip_index));
        if (!sk || !clip) return TRI_E_INVALID;
        *count = (uint32_t)clip->m_Channels.size();
        if (!bones || capacity < *count) return bones ? TRI_E_INVALID : TRI_OK;
        for (uint32_t c = 0; c < *count; ++c) bones[c] = Animation::ResolveChannelBoneIndex(clip->m_Channels[c], *sk, clip->m_Name);
        return TRI_OK;
    });
}

int trident_anim_evaluate(uint64_t handle, uint32_t clip_index, float time, float* out, uint32_t capacity, uint32_t* count) {
    if (!count) return TRI_E_INVALID;
    return GuardAnim([&] {
        Animation::AnimationPlayer player(Animation::AnimationAssetService::Get());
        player.SetSkeletonHandle(AnimHandle(handle));
        player.SetAnimationHandle(AnimHandle(handle));
        player.SetClipIndex(AnimClip(clip_index));
        player.EvaluateAt(time);
        std::vector<glm::mat4> pose;
        player.CopyPoseTo(pose);
        *count = (uint32_t)pose.size();
        if (!out) return TRI_OK;
        if (capacity < pose.size()) return TRI_E_INVALID;
        for (size_t b = 0; b < pose.size(); ++b)
            for (int c = 0; c < 4; ++c)
                for (int k = 0; k < 4; ++k) out[16 * b + 4 * c + k] = pose[b][c][k];
        return TRI_OK;
    });
}

int trident_anim_eval_program(uint64_t handle, const tri_pose_op* ops, uint32_t op_count, const float* mask_weights,
                              const uint32_t* mask_counts, uint32_t mask_count, float* out, uint32_t capacity,
                              uint32_t* count) {
    if (!count || (op_count && !ops) || (mask_count && !mask_counts)) return TRI_E_INVALID;
    return GuardAnim([&] {
        auto& service = Animation::AnimationAssetService::Get();
        const Animation::Skeleton* sk = service.GetSkeleton(AnimHandle(handle));
        if (!sk) return TRI_E_INVALID;
        Animation::PoseProgram program;
        for (uint32_t i = 0; i < op_count; ++i) {
            Animation::PoseOp op;
            op.m_Op = ops[i].op;
            op.m_A = ops[i].a;
            op.m_F = ops[i].f;
            program.m_Ops.push_back(op);
        }
        size_t at = 0;
        for (uint32_t m = 0; m < mask_count; ++m) {
            if (mask_counts[m] && !mask_weights) return TRI_E_INVALID;
            Animation::AnimationMask mask;
            mask.m_BoneWeights.assign(mask_weights + at, mask_weights + at + mask_counts[m]);
            at += mask_counts[m];
            program.m_Masks.push_back(std::move(mask));
        }
        Animation::AnimationPose pose;
        if (!Animation::EvaluatePoseProgram(*sk, service.GetAnimationClips(AnimHandle(handle)), program, pose)) return TRI_E_INVALID;
        const std::vector<glm::mat4> mats = Animation::AnimationPoseUtilities::ComposeSkinningMatrices(*sk, pose);
        *count = (uint32_t)mats.size();
        if (!out) return TRI_OK;
        if (capacity < mats.size()) return TRI_E_INVALID;
        for (size_t b = 0; b < mats.size(); ++b)
            for (int c = 0; c < 4; ++c)
                for (int k = 0; k < 4; ++k) out[16 * b + 4 * c + k] = mats[b][c][k];
        return TRI_OK;
    });
}

int trident_node_clip(uint32_t clip_index, int looping, float speed, const char* speed_parameter, uint64_t* out) {
    if (!out) return TRI_E_INVALID;
    return GuardAnim([&] {
        auto node = std::make_unique<Animation::ClipNode>(AnimClip(clip_index), looping != 0, speed);
        if (speed_parameter) node->SetSpeedParameter(speed_parameter);
        *out = KeepNode(std::move(node));
        return TRI_OK;
    });
}

int trident_node_blend(uint64_t first, uint64_t second, float weight, const char* weight_parameter, uint64_t* out) {
    if (!out) return TRI_E_INVALID;
    return GuardAnim([&] {
        if ((first && !g_nodes.count(first)) || (second && !g_nodes.count(second)) || (first && first == second)) return TRI_E_INVALID;
        bool ok = true;
        auto a = TakeNode(first, &ok);
        auto b = TakeNode(second, &ok);
        auto node = std::make_unique<Animation::BlendNode>(std::move(a), std::move(b), weight);
        if (weight_parameter) node->SetWeightParameter(weight_parameter);
        *out = KeepNode(std::move(node));
        return TRI_OK;
    });
}

int trident_node_blend_space(const uint32_t* clip_indices, const float* positions, uint32_t count, float parameter_default,
                             const char* parameter, uint64_t* out) {
    if (!out || (count && (!clip_indices || !positions))) return TRI_E_INVALID;
    return GuardAnim([&] {
        std::vector<Animation::BlendSpace1DNode::Sample> samples(count);
        for (uint32_t i = 0; i < count; ++i) {
            samples[i].m_ClipIndex = AnimClip(clip_indices[i]);
            samples[i].m_Position = positions[i];
        }
        auto node = std::make_unique<Animation::BlendSpace1DNode>(std::move(samples), parameter_default);
        if (parameter) node->SetParameterName(parameter);
        *out = KeepNode(std::move(node));
        return TRI_OK;
    });
}

int trident_node_destroy(uint64_t node) { return g_nodes.erase(node) ? TRI_OK : TRI_E_INVALID; }

int trident_sm_create(uint64_t skeleton_handle, uint64_t library_handle, uint64_t* out) {
    if (!out) return TRI_E_INVALID;
    return GuardAnim([&] {
        auto machine = std::make_shared<Animation::AnimationStateMachine>(Animation::AnimationAssetService::Get());
        machine->SetSkeletonHandle(AnimHandle(skeleton_handle));
        machine->SetAnimationLibraryHandle(AnimHandle(library_handle));
        *out = g_next_graph_id++;
        g_machines[*out] = std::move(machine);
        return TRI_OK;
    });
}

int trident_sm_destroy(uint64_t machine) { return g_machines.erase(machine) ? TRI_OK : TRI_E_INVALID; }

int trident_sm_set_handles(uint64_t machine, uint64_t skeleton_handle, uint64_t library_handle) {
    return GuardAnim([&] {
        Animation::AnimationStateMachine* m = Machine(machine);
        if (!m) return TRI_E_INVALID;
        m->SetSkeletonHandle(AnimHandle(skeleton_handle));
        m->SetAnimationLibraryHandle(AnimHandle(library_handle));
        return TRI_OK;
    });
}

int trident_sm_parameter(uint64_t machine, const char* name, int type, float value, int add) {
    if (!name) return TRI_E_INVALID;
    return GuardAnim([&] {
        Animation::AnimationStateMachine* m = Machine(machine);
        if (!m) return TRI_E_INVALID;
        switch (type) {
            case TRIDENT_SM_FLOAT: add ? m->AddFloatParameter(name, value) : m->SetFloatParameter(name, value); break;
            case TRIDENT_SM_BOOL: add ? m->AddBoolParameter(name, value != 0.0f) : m->SetBoolParameter(name, value != 0.0f); break;
            case TRIDENT_SM_INTEGER: add ? m->AddIntegerParameter(name, (int)value) : m->SetIntegerParameter(name, (int)value); break;
            case TRIDENT_SM_TRIGGER:
                if (add) m->AddTriggerParameter(name);
                else if (value != 0.0f) m->FireTrigger(name);
                else m->ResetTrigger(name);
                break;
            default: return TRI_E_INVALID;
        }
        return TRI_OK;
    });
}

int trident_sm_get_parameter(uint64_t machine, const char* name, int* type, float* as_float, int* trigger_set) {
    if (!name) return TRI_E_INVALID;
    return GuardAnim([&] {
        Animation::AnimationStateMachine* m = Machine(machine);
        const Animation::AnimationParameter* p = m ? m->FindParameter(name) : nullptr;
        if (!p) return TRI_E_INVALID;
        if (type) *type = (int)p->m_Type;
        if (as_float) *as_float = p->AsFloat(0.0f);
        if (trigger_set) *trigger_set = p->m_TriggerValue ? 1 : 0;
        return TRI_OK;
    });
}

int trident_sm_add_layer(uint64_t machine, const char* name, float weight, int additive, uint32_t* out_layer) {
    if (!out_layer) return TRI_E_INVALID;
    return GuardAnim([&] {
        Animation::AnimationStateMachine* m = Machine(machine);
        if (!m) return TRI_E_INVALID;
        *out_layer = (uint32_t)m->AddLayer(name ? name : "", weight, additive != 0);
        return TRI_OK;
    });
}

int trident_sm_set_layer_mask(uint64_t machine, uint32_t layer, const float* weights, uint32_t count) {
    if (count && !weights) return TRI_E_INVALID;
    return GuardAnim([&] {
        Animation::AnimationStateMachine* m = Machine(machine);
        if (!m) return TRI_E_INVALID;
        Animation::AnimationMask mask;
        mask.m_BoneWeights.assign(weights, weights + count);
        m->SetLayerMask(layer, std::move(mask));
        return TRI_OK;
    });
}

int trident_sm_set_layer_weight(uint64_t machine, uint32_t layer, float weight) {
    Animation::AnimationStateMachine* m = Machine(machine);
    if (!m) return TRI_E_INVALID;
    m->SetLayerWeight(layer, weight);
    return TRI_OK;
}

int trident_sm_set_layer_entry(uint64_t machine, uint32_t layer, const char* state) {
    return GuardAnim([&] {
        Animation::AnimationStateMachine* m = Machine(machine);
        if (!m || !state) return TRI_E_INVALID;
        m->SetLayerEntryState(layer, state);
        return TRI_OK;
    });
}

int trident_sm_add_state(uint64_t machine, uint32_t layer, const char* name, uint64_t root_node) {
    return GuardAnim([&] {
        Animation::AnimationStateMachine* m = Machine(machine);
        if (!m || !name || layer >= m->GetLayerCount() || (root_node && !g_nodes.count(root_node))) return TRI_E_INVALID;
        bool ok = true;
        m->AddState(layer, name, TakeNode(root_node, &ok));
        return TRI_OK;
    });
}

int trident_sm_add_transition(uint64_t machine, uint32_t layer, const char* from_state, const char* target_state,
                              int has_exit_time, float exit_time, float fade_duration,
                              const trident_sm_condition* conditions, uint32_t condition_count) {
    if (!from_state || !target_state || (condition_count && !conditions)) return TRI_E_INVALID;
    try {
        Animation::AnimationStateMachine* m = Machine(machine);
        if (!m || layer >= m->GetLayerCount()) return TRI_E_INVALID;
        Animation::AnimationTransition t;
        t.m_TargetState = target_state;
        t.m_HasExitTime = has_exit_time != 0;
        t.m_ExitTimeSeconds = exit_time;
        t.m_FadeDurationSeconds = fade_duration;
        for (uint32_t i = 0; i < condition_count; ++i) {
            const trident_sm_condition& c = conditions[i];
            if (!c.parameter || c.comparison < 0 || c.comparison > TRIDENT_SM_TRIGGERED) return TRI_E_INVALID;
            Animation::AnimationTransitionCondition cond;
            cond.m_ParameterName = c.parameter;
            cond.m_Comparison = (Animation::AnimationConditionComparison)c.comparison;
            cond.m_FloatValue = c.float_value;
            cond.m_IntValue = c.int_value;
            cond.m_BoolValue = c.bool_value != 0;
            t.m_Conditions.push_back(std::move(cond));
        }
        m->AddTransition(layer, from_state, t);
        return TRI_OK;
    } catch (const std::runtime_error&) {  // AddTransition from a state the layer does not have
        return TRI_E_STATE;
    } catch (const std::exception&) {
        return TRI_E_OOM;
    }
}

int trident_sm_update(uint64_t machine, float dt) {
    return GuardAnim([&] {
        Animation::AnimationStateMachine* m = Machine(machine);
        if (!m) return TRI_E_INVALID;
        m->Update(dt);
        return TRI_OK;
    });
}

int trident_sm_pose(uint64_t machine, float* out, uint32_t capacity, uint32_t* count) {
    if (!count) return TRI_E_INVALID;
    return GuardAnim([&] {
        Animation::AnimationStateMachine* m = Machine(machine);
        if (!m) return TRI_E_INVALID;
        std::vector<glm::mat4> pose;
        m->CopyPose(pose);
        *count = (uint32_t)pose.size();
        if (!out) return TRI_OK;
        if (capacity < pose.size()) return TRI_E_INVALID;
        for (size_t b = 0; b < pose.size(); ++b)
            for (int c = 0; c < 4; ++c)
                for (int k = 0; k < 4; ++k) out[16 * b + 4 * c + k] = pose[b][c][k];
        return TRI_OK;
    });
}

int trident_sm_program(uint64_t machine, tri_pose_op* ops, uint32_t capacity, uint32_t* count, uint32_t* mask_count) {
    if (!count) return TRI_E_INVALID;
    Animation::AnimationStateMachine* m = Machine(machine);
    if (!m) return TRI_E_INVALID;
    const Animation::PoseProgram& program = m->GetProgram();
    *count = (uint32_t)program.m_Ops.size();
    if (mask_count) *mask_count = (uint32_t)program.m_Masks.size();
    if (!ops) return TRI_OK;
    if (capacity < program.m_Ops.size()) return TRI_E_INVALID;
    for (size_t i = 0; i < program.m_Ops.size(); ++i) ops[i] = tri_pose_op{program.m_Ops[i].m_Op, program.m_Ops[i].m_A, program.m_Ops[i].m_F, 0u};
    return TRI_OK;
}

int trident_sm_program_mask(uint64_t machine, uint32_t mask, float* weights, uint32_t capacity, uint32_t* count) {
    if (!count) return TRI_E_INVALID;
    Animation::AnimationStateMachine* m = Machine(machine);
    if (!m || mask >= m->GetProgram().m_Masks.size()) return TRI_E_INVALID;
    const std::vector<float>& w = m->GetProgram().m_Masks[mask].m_BoneWeights;
    *count = (uint32_t)w.size();
    if (!weights) return TRI_OK;
    if (capacity < w.size()) return TRI_E_INVALID;
    std::copy(w.begin(), w.end(), weights);
    return TRI_OK;
}

int trident_sm_layer_state(uint64_t machine, uint32_t layer, char* current, char* next, uint32_t name_capacity,
                           float* time_in_state, float* transition_elapsed, float* transition_duration) {
    Animation::AnimationStateMachine* m = Machine(machine);
    const Animation::AnimationLayer* l = m ? m->GetLayer(layer) : nullptr;
    if (!l) return TRI_E_INVALID;
    if (CopyName(l->m_CurrentState ? l->m_CurrentState->m_Name : std::string(), current, name_capacity)) return TRI_E_INVALID;
    if (CopyName(l->m_NextState ? l->m_NextState->m_Name : std::string(), next, name_capacity)) return TRI_E_INVALID;
    if (time_in_state) *time_in_state = l->m_TimeInState;
    if (transition_elapsed) *transition_elapsed = l->m_TransitionElapsed;
    if (transition_duration) *transition_duration = l->m_TransitionDuration;
    return TRI_OK;
}

int trident_anim_advance(uint64_t handle, uint32_t clip_index, float time, float speed, int looping, int playing, float dt,
                         float* out_time, int* out_playing) {
    if (!out_time || !out_playing) return TRI_E_INVALID;
    return GuardAnim([&] {
        Animation::AnimationPlayer player(Animation::AnimationAssetService::Get());
        player.SetSkeletonHandle(AnimHandle(handle));
        player.SetAnimationHandle(AnimHandle(handle));
        player.SetClipIndex(AnimClip(clip_index));
        player.SetCurrentTime(time);
        player.SetPlaybackSpeed(speed);
        player.SetLooping(looping != 0);
        player.SetIsPlaying(playing != 0);
        player.Update(dt);
        *out_time = player.GetCurrentTime();
        *out_playing = player.IsPlaying() ? 1 : 0;
        return TRI_OK;
    });
}

}  // extern "C"
