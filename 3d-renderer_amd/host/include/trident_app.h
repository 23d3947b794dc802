/* trident_app.h — a flat C driver over the C++ Trident::Renderer shim (host/include/trident/ headers).
 *
 * It plays the part of Trident-Forge's ApplicationLayer (Trident-Forge/src/Layer/ApplicationLayer.cpp)
 * for tests and tools that are not C++: it owns one ECS::Registry, an EditorCamera and a
 * RuntimeCamera, and forwards to RenderCommand. Everything below the shim is the drop-in C-ABI in
 * include/tri_raster.h. All functions return TRI_OK or a negative TRI_E_* code.
 */
#ifndef TRIDENT_APP_H
#define TRIDENT_APP_H

#include <stddef.h>
#include <stdint.h>

#include "../../../include/tri_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trident_app trident_app;

/* primitive: 0 none, 1 cube, 2 sphere, 3 quad (MeshComponent::PrimitiveType) */
enum { TRIDENT_PRIMITIVE_NONE = 0, TRIDENT_PRIMITIVE_CUBE = 1, TRIDENT_PRIMITIVE_SPHERE = 2, TRIDENT_PRIMITIVE_QUAD = 3 };
enum { TRIDENT_LIGHT_DIRECTIONAL = 0, TRIDENT_LIGHT_POINT = 1 };

int trident_app_create(uint32_t raster_flags, trident_app** out);
void trident_app_destroy(trident_app* app);

/* Renderer::AppendMeshes with one mesh + one material; returns the mesh index in *mesh_index. */
int trident_app_append_mesh(trident_app* app, const tri_vertex* vertices, uint32_t vertex_count,
                            const uint32_t* indices, uint32_t index_count, const float base_color[4],
                            float metallic, float roughness, const char* texture_path, uint32_t* mesh_index);
int trident_app_upload_texture(trident_app* app, const char* path, const uint8_t* rgba, uint32_t width,
                               uint32_t height);

/* Entity with Transform + MeshComponent (primitive, or mesh_index when primitive == 0). */
int trident_app_add_mesh_entity(trident_app* app, int primitive, uint32_t mesh_index, const float position[3],
                                const float rotation_deg[3], const float scale[3], uint32_t* entity);
int trident_app_set_entity_texture(trident_app* app, uint32_t entity, const char* texture_path);
/* Entity with Transform + SpriteComponent (tint, UV scale / offset, tiling; NULL = the component's
 * defaults); drawn after the meshes (GatherSpriteDraws / DrawSprites, Renderer.cpp:2996-3089). A texture
 * goes on with trident_app_set_entity_texture. */
int trident_app_add_sprite_entity(trident_app* app, const float position[3], const float rotation_deg[3],
                                  const float scale[3], const float tint[4], const float uv_scale[2],
                                  const float uv_offset[2], float tiling, uint32_t* entity);
int trident_app_set_sprite_visible(trident_app* app, uint32_t entity, int visible);
/* SpriteComponent of an entity: tint[4], uv_scale[2], uv_offset[2], tiling, visible. */
int trident_app_entity_sprite(trident_app* app, uint32_t entity, float out[10]);
int trident_app_set_entity_transform(trident_app* app, uint32_t entity, const float position[3],
                                     const float rotation_deg[3], const float scale[3]);
int trident_app_set_entity_visible(trident_app* app, uint32_t entity, int visible);
/* AnimationComponent::m_BoneMatrices of an entity (count column-major mat4s; 0 clears the palette):
 * the draw skins with them (PrepareBonePaletteBuffer, Renderer.cpp:3168-3245). */
int trident_app_set_entity_bones(trident_app* app, uint32_t entity, const float* matrices, uint32_t count);
/* The same for entity_count entities in one call: entity i takes matrices[i * matrices_per_entity ...]. */
int trident_app_set_entities_bones(trident_app* app, const uint32_t* entities, uint32_t entity_count,
                                   const float* matrices, uint32_t matrices_per_entity);
int trident_app_add_light(trident_app* app, int type, const float position[3], const float direction[3],
                          const float color[3], float intensity, float range, int enabled, uint32_t* entity);

/* LightComponent::m_ShadowCaster of a light entity (LightComponent.h:33): a shadow-casting first
 * directional light turns on the shadow-map pre-pass (Renderer::SetShadowMapSize, default 2048). */
int trident_app_set_light_shadow_caster(trident_app* app, uint32_t entity, int caster);
int trident_app_set_shadow_map_size(trident_app* app, uint32_t size);
/* Renderer::SetDeviceCount: with count > 1 every viewport renders as `count` row bands on `devices`
 * (NULL = 0 .. count-1; ordinals may repeat) assembled on the first band's device (tri_group). */
int trident_app_set_device_count(trident_app* app, uint32_t count, const int32_t* devices);
/* The pre-pass configuration DrawFrame would use now (*enabled = 0 when there is none). */
int trident_app_shadow_config(trident_app* app, tri_shadow_config* out, int* enabled);

/* which: 0 editor, 1 runtime. Runtime camera readiness follows `ready`. */
int trident_app_set_camera(trident_app* app, int which, const float position[3], const float rotation_deg[3],
                           float fov_deg, float near_clip, float far_clip, int ready);
int trident_app_set_viewport(trident_app* app, uint32_t viewport_id, uint32_t width, uint32_t height);
int trident_app_set_clear_color(trident_app* app, const float rgba[4]);
/* Renderer::SetSkyboxCubemap: faces [6][size][size] RGBA8 sRGB (+X,-X,+Y,-Y,+Z,-Z). */
int trident_app_set_skybox(trident_app* app, const uint8_t* faces, uint32_t size);

/* Renderer::SetAssetsDirectory: the directory whose Skyboxes/ CreateSkyboxCubemap searches
 * (Renderer.cpp:3830-3927); re-runs the discovery. *source (nullable, source_cap bytes) names the result. */
int trident_app_set_assets_dir(trident_app* app, const char* directory, char* source, uint32_t source_cap);

/* The loaders on their own (no app): TextureLoader::Load (flip = 1: stb's flip-on-load for 2D textures)
 * or one cube face (flip = 0). rgba = NULL queries the size; else capacity must hold width*height*4. */
int trident_load_image(const char* path, int flip, uint8_t* rgba, uint64_t capacity, uint32_t* width,
                       uint32_t* height);
/* DiscoverDefaultSkybox(assets_dir): faces [6][size][size] RGBA8 (+X,-X,+Y,-Y,+Z,-Z); faces = NULL
 * queries *size; *size = 0 when nothing valid was found. */
int trident_load_default_skybox(const char* assets_dir, uint8_t* faces, uint64_t capacity, uint32_t* size,
                                char* source, uint32_t source_cap);

/* The same discovery for every cubemap it can return (KTX 1 files, EXR faces, mip chains): *info describes the result
 * (size 0: nothing valid was found), texels = NULL queries it; else capacity must hold info->bytes, the chain as
 * tri_upload_skybox_ex takes it. trident_load_default_skybox itself is TRI_E_UNSUPPORTED for a cubemap that is not
 * one level of RGBA8 sRGB when it is asked for the faces. */
typedef struct {
    uint32_t format;          /* TRI_SKY_FMT_* */
    uint32_t size;            /* level 0 face edge */
    uint32_t mip_count;
    uint32_t bytes_per_pixel;
    uint32_t is_hdr;
    uint32_t region_levels;   /* levels with recorded face regions (m_FaceRegions.size()) */
    uint64_t bytes;           /* the whole chain */
} trident_cubemap_info;
int trident_load_default_skybox_ex(const char* assets_dir, trident_cubemap_info* info, uint8_t* texels, uint64_t capacity,
                                   char* source, uint32_t source_cap);
/* SkyboxTextureLoader::LoadFromKtx (kind 0: path is the file) or LoadFromDirectory (kind 1: path is the directory). */
int trident_load_skybox(const char* path, int kind, trident_cubemap_info* info, uint8_t* texels, uint64_t capacity);
/* Loader::FloatToHalf over count values. */
int trident_float_to_half(const float* values, uint16_t* halves, uint32_t count);

/* Model import as Forge's drop handler (ModelLoader: .obj/.mtl, .gltf, .glb): entities per mesh
 * instance. Up to `capacity` spawned entity ids go to `entities`; *count gets how many were spawned. */
int trident_app_import_model(trident_app* app, const char* path, uint32_t* entities, uint32_t capacity,
                             uint32_t* count);
/* `.trident` scene files (Scene::Save / Scene::Load, ECS/Scene.cpp:80-151). Load replaces every
 * entity and rebuilds imported geometry from the SourceAsset paths; *entity_count may be null. */
int trident_app_save_scene(trident_app* app, const char* path, const char* scene_name);
int trident_app_load_scene(trident_app* app, const char* path, uint32_t* entity_count);
/* The runtime camera follows the scene's primary CameraComponent entity (the first camera entity
 * when none is primary): Transform position / rotation, projection, field of view, clip planes. */
int trident_app_use_scene_camera(trident_app* app);
/* Component inspection for tests: Transform (9 floats) and MeshComponent {mesh_index, primitive,
 * source mesh index} of an entity; TRI_E_INVALID when absent. */
int trident_app_entity_transform(trident_app* app, uint32_t entity, float out[9]);
int trident_app_entity_mesh(trident_app* app, uint32_t entity, uint64_t out[3]);
int trident_app_entity_count(trident_app* app, uint32_t* count);

/* Renderer::SetPresentExtent: DrawFrame then blits the active (last SetViewport) viewport onto a
 * width x height present image (VK_FILTER_LINEAR); 0 x 0 disables. */
int trident_app_set_present_extent(trident_app* app, uint32_t width, uint32_t height);
/* Renderer::SetAiBlendStrength / SubmitAiInterpolation (Default.frag's AI frame blend): width * height * channels
 * floats in [0, 1] (NULL or a zero extent drops the frame). */
int trident_app_set_ai_blend_strength(trident_app* app, float strength);
int trident_app_submit_ai_frame(trident_app* app, const float* pixels, uint32_t width, uint32_t height, uint32_t channels);
int trident_app_read_present(trident_app* app, uint8_t* rgba, uint32_t width, uint32_t height);

int trident_app_draw_frame(trident_app* app);
/* Renderer::FinishFrame: wait for the frame the last draw_frame submitted (the next draw_frame does it first). */
int trident_app_finish_frame(trident_app* app);
/* Renderer::SetFramesInFlight (1..4; 1 = the reference's pacing). */
int trident_app_set_frames_in_flight(trident_app* app, uint32_t n);
/* Renderer::SetViewportRecordingEnabled: record viewport `viewport_id` to the .y4m file `path` at width x height
 * (odd values rounded up to even; out_extent, nullable, gets the recording extent). TRI_E_STATE when the renderer
 * refuses (an FFmpeg container or another extension, a zero extent, SetDeviceCount > 1): recording is then off.
 * While recording, the viewport's camera is sized to the recording extent (as the panel that shows the target would
 * size it), so the frames are those of a viewport of that extent. enabled = 0 finalises the file (path may be NULL). */
int trident_app_set_recording(trident_app* app, int enabled, uint32_t viewport_id, uint32_t width, uint32_t height,
                              const char* path, uint32_t out_extent[2]);
/* Renderer::SetRecordingQuality / GetRecordingQuality: the JPEG quality of .mkv recordings (a `path` ending in .mkv
 * records Motion-JPEG in Matroska, encoded on the device), from the next session; clamped to 1..100, default 90.
 * out_quality, nullable, gets the value in force. */
int trident_app_set_recording_quality(trident_app* app, int quality, int* out_quality);
/* Renderer::IsViewportRecording / GetRecordedFrameCount (FRAME records of the current or last session). */
int trident_app_recording_state(trident_app* app, int* recording, uint64_t* frames);

/* Trident::VideoEncoder on its own (no app, no device). begin / submit / end return TRI_OK where the encoder
 * returns true and TRI_E_STATE where it returns false. submit_rgba: `bytes` bytes of RGBA8 rows, converted on the
 * host; submit_planes: 3 * width * height bytes converted already (Y, U, V planes). */
typedef struct trident_video trident_video;
int trident_video_create(trident_video** out);
void trident_video_destroy(trident_video* video);
int trident_video_begin(trident_video* video, const char* path, uint32_t width, uint32_t height, uint32_t fps);
int trident_video_submit_rgba(trident_video* video, const uint8_t* rgba, uint64_t bytes, uint32_t width,
                              uint32_t height);
int trident_video_submit_planes(trident_video* video, const uint8_t* yuv, uint32_t width, uint32_t height);
/* An .mkv session (Matroska, V_MJPEG): submit_rgba encodes the frame as a baseline JPEG on the host; submit_jpeg
 * takes a complete JPEG of the session's extent, encoded already (tri_recorder_wait_ex). set_quality (1..100, default
 * 90) and set_restart_interval (MCUs, 1..65535; 0 = the default) are sticky; TRI_E_INVALID outside the range. */
int trident_video_submit_jpeg(trident_video* video, const uint8_t* jpeg, uint64_t bytes, uint32_t width, uint32_t height);
int trident_video_set_quality(trident_video* video, uint32_t quality);
int trident_video_set_restart_interval(trident_video* video, uint32_t restart_mcus);
int trident_video_end(trident_video* video);
int trident_video_state(trident_video* video, int* active, uint64_t* frames);
/* VideoEncoder::ConvertRgbaToYuv444 alone: `pixels` RGBA8 pixels -> 3 * pixels bytes, planar (alpha ignored). */
int trident_video_convert_rgba(const uint8_t* rgba, uint64_t pixels, uint8_t* yuv);

/* ---- AI readback and dataset capture ---- */
/* Renderer::SetFrameDatasetCaptureDirectory (when `directory` is not NULL; "" = the default directory), ...Interval
 * (when interval != 0) and ...Enabled, in this order. Disabling writes every queued sample before it returns. */
int trident_app_set_dataset_capture(trident_app* app, int enabled, const char* directory, uint32_t interval);
/* The getters: IsFrameDatasetCaptureEnabled, GetFrameDatasetCaptureInterval, and the directory copied into
 * `directory` (capacity bytes with the terminator; TRI_E_INVALID when it does not fit). Every pointer is nullable. */
int trident_app_dataset_capture_state(trident_app* app, int* enabled, uint32_t* interval, char* directory,
                                      uint32_t capacity);
/* Renderer::SetAiThrottleIntervals(readback_ms, inference_ms) (0 disables a throttle), then SetAiReadbackEnabled.
 * TRI_E_STATE when the renderer refuses (SetDeviceCount > 1). */
int trident_app_set_ai_readback(trident_app* app, int enabled, uint32_t readback_ms, uint32_t inference_ms);
/* Renderer::IsAiReadbackEnabled. */
int trident_app_ai_readback_state(trident_app* app, int* enabled);
/* Renderer::TryAcquireRenderedFrame: *got = 1 and width * height * 4 floats in `out` (R, G, B, A per pixel) when a
 * tensor was pending and the inference throttle has elapsed, else *got = 0. TRI_E_INVALID, with the tensor left
 * pending, when `capacity` (in floats) is too small. width and height (nullable) always get
 * Renderer::GetFrameReadbackExtent, the extent to size `out` for (0 x 0 before the first resolved frame). */
int trident_app_acquire_frame(trident_app* app, float* out, uint64_t capacity, uint32_t* width, uint32_t* height, int* got);
/* Renderer::GetFrameReadbackDeviceTensor: the latest tensor on the device (*got = 0 before one was resolved), valid
 * until the next draw_frame. Waits for the frames in flight. */
int trident_app_readback_device_tensor(trident_app* app, const float** device, uint32_t* width, uint32_t* height, int* got);
/* Renderer::SubmitAiOutput: TRI_OK where it returns true, TRI_E_STATE where it returns false. */
int trident_app_submit_ai_output(trident_app* app, const float* data, uint64_t count, const int64_t* shape, uint32_t rank);
/* ---- the frame generator on the device (Renderer::LoadAiModel, ProcessAiFrame, GetAiDebugStats) ---- */
/* Renderer::LoadAiModel(path): TRI_OK, or TRI_E_INVALID with Renderer::GetAiModelError() (which names the damaged
 * tensor) copied into `message` (nullable; capacity bytes with the terminator, truncated to fit); TRI_E_STATE while
 * SetDeviceCount > 1. No device is needed: the device generator is made for the first frame's extent. */
int trident_app_load_ai_model(trident_app* app, const char* path, char* message, uint32_t capacity);
/* Renderer::ResolveAiModelPath: *found = 1 and the path in `path` (TRI_E_INVALID when it does not fit), else 0. */
int trident_app_resolve_ai_model_path(trident_app* app, char* path, uint32_t capacity, int* found);
/* Renderer::TryInitialiseAiModel: the search, then LoadAiModel on what it found. */
int trident_app_try_initialise_ai_model(trident_app* app, int* initialised);
/* Renderer::GetAiDebugStats (Renderer.h:99-110): the snapshot the last ProcessAiFrame / FinishAiInference took. */
typedef struct trident_ai_debug_stats {
    int32_t model_initialised;
    uint32_t pending_job_count;
    uint64_t completed_inference_count;
    double last_inference_ms;
    double average_inference_ms;
    int32_t texture_ready;
    float blend_strength;
    uint32_t texture_width;
    uint32_t texture_height;
    double reserved_metric;
} trident_ai_debug_stats;
int trident_app_ai_debug_stats(trident_app* app, trident_ai_debug_stats* out);
/* AI::FrameGenerator::IsInitialised, GetPrimaryInputShape and GetPrimaryOutputShape ([1, H, W, C]; H and W are -1
 * until the first frame fixes them; all 0 without a model). Every pointer is nullable. */
int trident_app_ai_model_info(trident_app* app, int* initialised, int64_t input_shape[4], int64_t output_shape[4]);
/* Renderer::FinishAiInference(timeout_ms): *finished = 0 when the deadline passed first. */
int trident_app_finish_ai_inference(trident_app* app, uint32_t timeout_ms, int* finished);
/* Renderer::ReadAiBlendFrame: the active viewport's blend frame as the device holds it, width * height * 4 bytes
 * (R, G, B, A) into `rgba` (capacity in bytes; TRI_E_INVALID when too small). TRI_E_STATE without a blend frame. */
int trident_app_read_ai_blend_frame(trident_app* app, uint8_t* rgba, uint64_t capacity, uint32_t* width, uint32_t* height);
/* Renderer::NormaliseAndReorderAiOutput alone, in place (no app, no device). */
int trident_ai_normalise_output(float* data, uint64_t count, int64_t channels);

/* Trident::FrameDatasetRecorder on its own (no app, no device). record_input / record_output forward to
 * RecordInputFrame (rank 0: the default shape) / RecordAiOutput; enable(0) and flush return once the queued files are
 * written. state: the next sample index and the inputs still waiting for an output. */
typedef struct trident_dataset trident_dataset;
int trident_dataset_create(trident_dataset** out);
void trident_dataset_destroy(trident_dataset* dataset);
int trident_dataset_set_directory(trident_dataset* dataset, const char* directory);
int trident_dataset_set_interval(trident_dataset* dataset, uint32_t interval);
int trident_dataset_enable(trident_dataset* dataset, int enabled);
int trident_dataset_reset(trident_dataset* dataset);
int trident_dataset_record_input(trident_dataset* dataset, const float* data, uint64_t count, uint32_t width,
                                 uint32_t height, uint32_t channels, const int64_t* shape, uint32_t rank);
int trident_dataset_record_output(trident_dataset* dataset, const float* data, uint64_t count, const int64_t* shape,
                                  uint32_t rank);
int trident_dataset_flush(trident_dataset* dataset);
int trident_dataset_state(trident_dataset* dataset, int* enabled, uint32_t* interval, uint64_t* next_index,
                          uint64_t* pending);
/* FrameDatasetRecorder::WriteNpyFile alone: TRI_OK, or TRI_E_STATE where it refuses (no file is written then). */
int trident_dataset_write_npy(const char* path, const float* data, uint64_t count, const int64_t* shape, uint32_t rank);

/* ---- entity ids: picking, rectangle selection, the entity image, the selection outline ---- */
/* Renderer::SetEntityIdOutputEnabled: from the viewport's next draw_frame on. */
int trident_app_set_entity_id_output(trident_app* app, uint32_t viewport_id, int enabled);
/* Renderer::PickEntity on the viewport's latest frame (fences): *hit 1 with the entity and its depth in [0, 1]
 * (depth01 nullable), 0 on background, outside the viewport or without ids. */
int trident_app_pick_entity(trident_app* app, uint32_t viewport_id, int32_t x, int32_t y, int* hit, uint32_t* entity,
                            float* depth01);
/* Renderer::PickEntitiesInRect: *count distinct entities in draw order, the first min(capacity, *count) written. */
int trident_app_pick_entities_in_rect(trident_app* app, uint32_t viewport_id, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                                      uint32_t* entities, uint32_t capacity, uint32_t* count);
/* Renderer::ReadViewportEntityIds: width * height entities (`background` where none); TRI_E_STATE where it returns
 * false, TRI_E_INVALID when capacity (in pixels) is short. */
int trident_app_read_entity_ids(trident_app* app, uint32_t viewport_id, uint32_t* entities, uint64_t capacity,
                                uint32_t background);
/* Renderer::SetSelectedEntity (0xFFFFFFFF: none) and Renderer::SetSelectionOutline; the latter is TRI_E_STATE where
 * the renderer refuses (SetDeviceCount > 1, a width outside 1..8): the outline is then as it was, or off. */
int trident_app_set_selected_entity(trident_app* app, uint32_t entity);
int trident_app_set_selection_outline(trident_app* app, int enabled, const float rgba[4], uint32_t width_px);

/* ---- motion vectors ---- */
/* Renderer::SetMotionVectorOutputEnabled: from the viewport's next draw_frame on; TRI_E_STATE where the renderer
 * refuses (SetDeviceCount > 1). */
int trident_app_set_motion_vector_output(trident_app* app, uint32_t viewport_id, int enabled);
/* Renderer::ReadViewportMotionVectors: width * height * 2 floats; TRI_E_STATE where it returns false, TRI_E_INVALID
 * when capacity (in floats) is short. */
int trident_app_read_motion_vectors(trident_app* app, uint32_t viewport_id, float* xy, uint64_t capacity);
/* Renderer::GetViewportMotionTexture: copies the motion image's handle (TRI_E_STATE where it returns null). */
int trident_app_motion_texture(trident_app* app, uint32_t viewport_id, tri_image* out);

/* ---- history reprojection ---- */
/* Renderer::SetHistoryReprojectionEnabled: from the viewport's next draw_frame on; TRI_E_STATE where the renderer
 * refuses (SetDeviceCount > 1, a negative or non-finite tolerance). */
int trident_app_set_history_reprojection(trident_app* app, uint32_t viewport_id, int enabled, float depth_tolerance);
/* Renderer::ReadViewportReprojection: width * height * 4 bytes of warped colour (B G R A) and width * height mask
 * bytes; TRI_E_STATE where it returns false, TRI_E_INVALID when capacity (in pixels) is short. */
int trident_app_read_reprojection(trident_app* app, uint32_t viewport_id, uint8_t* bgra, uint8_t* mask, uint64_t capacity);
/* Renderer::GetViewportReprojectedTexture / GetViewportDisocclusionTexture: copies the two handles (TRI_E_STATE where
 * they return null). */
int trident_app_reprojection_textures(trident_app* app, uint32_t viewport_id, tri_image* colour, tri_image* mask);

/* ---- temporal anti-aliasing ---- */
/* Renderer::SetTemporalAntiAliasingEnabled: from the viewport's next draw_frame on; TRI_E_STATE where the renderer
 * refuses (SetDeviceCount > 1, an alpha outside (0, 1], a period above 64). */
int trident_app_set_temporal_anti_aliasing(trident_app* app, uint32_t viewport_id, int enabled, float alpha, uint32_t period,
                                           int reject_ids);
/* Renderer::IsTemporalAntiAliasingEnabled into *enabled. */
int trident_app_is_temporal_anti_aliasing(trident_app* app, uint32_t viewport_id, int* enabled);
/* Renderer::ReadViewportResolvedPixels (width * height * 4 bytes, R G B A) and ReadViewportTaaMask (width * height
 * bytes); either pointer may be NULL. TRI_E_STATE where they return false, TRI_E_INVALID when capacity (in pixels) is
 * short. */
int trident_app_read_resolved(trident_app* app, uint32_t viewport_id, uint8_t* rgba, uint8_t* mask, uint64_t capacity);
/* Renderer::GetViewportResolvedTexture: copies the handle (TRI_E_STATE where it returns null). */
int trident_app_resolved_texture(trident_app* app, uint32_t viewport_id, tri_image* out);
/* Renderer::SetTemporalUpscalingEnabled: from the viewport's next draw_frame on; TRI_E_STATE where the renderer refuses
 * (SetDeviceCount > 1, a render scale outside [1/3, 1] or against the extent rule, an alpha outside (0, 1], temporal
 * anti-aliasing on for the viewport). */
int trident_app_set_temporal_upscaling(trident_app* app, uint32_t viewport_id, int enabled, float render_scale, float alpha,
                                       int reject_ids);
/* Renderer::IsTemporalUpscalingEnabled into *enabled. */
int trident_app_is_temporal_upscaling(trident_app* app, uint32_t viewport_id, int* enabled);
/* Renderer::ReadViewportUpscaledPixels (width * height * 4 bytes, R G B A, at the viewport's full size) and
 * ReadViewportUpscaleMask (width * height bytes); either pointer may be NULL. TRI_E_STATE where they return false,
 * TRI_E_INVALID when capacity (in pixels) is short. */
int trident_app_read_upscaled(trident_app* app, uint32_t viewport_id, uint8_t* rgba, uint8_t* mask, uint64_t capacity);
/* Renderer::GetViewportUpscaledTexture: copies the handle (TRI_E_STATE where it returns null). */
int trident_app_upscaled_texture(trident_app* app, uint32_t viewport_id, tri_image* out);

/* ---- text overlay ---- */
/* Renderer::SubmitText: `bytes` bytes of UTF-8 (no terminator needed) at `position` (viewport pixels) in `color`
 * (RGBA) for the viewport's next draw_frame. */
int trident_app_submit_text(trident_app* app, uint32_t viewport_id, const float position[2], const float color[4],
                            const char* text, uint32_t bytes);
/* Renderer::SetTextFont: TRI_OK, or TRI_E_STATE where it returns false (the previous font stays). */
int trident_app_set_font(trident_app* app, const char* path, float pixel_height);
/* Trident::TextRenderer on its own (no app, no device): load a TrueType file (TRI_E_STATE where LoadFontFile returns
 * false), then read what it baked. atlas: out = NULL queries the extent, else capacity must hold width * height
 * coverage bytes. glyph: ResolveGlyph(codepoint) as offset.xy, size.xy, uv_min.xy, uv_max.xy, advance.
 * metrics: line advance, scale (pixels per font unit), pixel height. layout: one string at `position` into at most
 * `capacity` quads; *count gets how many the string needs (TRI_E_INVALID, nothing written, when capacity is short). */
typedef struct trident_font trident_font;
int trident_font_create(trident_font** out);
void trident_font_destroy(trident_font* font);
int trident_font_load(trident_font* font, const char* path, float pixel_height);
int trident_font_load_memory(trident_font* font, const uint8_t* data, uint64_t size, float pixel_height);
int trident_font_atlas(trident_font* font, uint8_t* out, uint64_t capacity, uint32_t* width, uint32_t* height);
int trident_font_glyph(trident_font* font, uint32_t codepoint, float out[9]);
int trident_font_metrics(trident_font* font, float out[3]);
int trident_font_layout(trident_font* font, const float position[2], const float color[4], const char* text,
                        uint32_t bytes, tri_text_quad* out, uint32_t capacity, uint32_t* count);

/* ---- skeletal animation on the CPU (host/include/trident/Animation.h): no app, no GPU ----------------------
 * The asset service (Animation::AnimationAssetService::Get()) and the float32 player, over flat arrays. Matrices are
 * column-major, quaternions w, x, y, z. */
/* Animation::DecomposeBindTransform: out = translation[3], rotation[4], scale[3] — the defaults a tri_pose_bone takes. */
int trident_anim_decompose(const float local_bind[16], float out[10]);
/* RegisterRuntimeAsset with a skeleton and no clips (an id registered before keeps its handle and is replaced).
 * parents: negative = none; source_names: nullable, and a NULL entry names bone i "Bone<i>"; root_index is
 * m_RootBoneIndex as given (negative: unset). bone_count 0 registers an empty skeleton. */
int trident_anim_register(const char* asset_id, uint32_t bone_count, const int32_t* parents, const float* local_binds,
                          const float* inverse_binds, const char* const* source_names, int32_t root_index,
                          uint64_t* handle);
/* Append a clip to the asset. channels[i].bone and the key ranges are tri_pose_channel's; stored_bones (nullable)
 * overrides the stored index per channel (it may be stale or negative); source_names (nullable, entries nullable) are
 * the channels' m_SourceBoneName. *clip_index receives the clip's index. */
int trident_anim_add_clip(uint64_t handle, const char* name, float duration, const tri_pose_channel* channels,
                          const int32_t* stored_bones, const char* const* source_names, uint32_t channel_count,
                          const float* vec_times, const float* vec_values, uint32_t vec_count, const float* quat_times,
                          const float* quat_values, uint32_t quat_count, uint32_t* clip_index);
/* AnimationAssetService::AcquireSkeleton(path): the asset of a model file (.gltf / .glb), loaded once per path;
 * TRI_E_INVALID when the file yields neither bones nor clips. */
int trident_anim_load(const char* path, uint64_t* handle);
/* The asset as JSON text, for tests: {"root", "bones": [{"name", "source", "parent", "children", "local", "inverse"}],
 * "clips": [{"name", "duration", "ticks", "channels": [{"bone", "source", "t", "r", "s"}]}]} with keys as
 * [time, x, y, z] / [time, w, x, y, z] and floats printed with 9 significant digits. *needed gets the byte count
 * (with the terminator); out is written when capacity allows. */
int trident_anim_describe(uint64_t handle, char* out, uint64_t capacity, uint64_t* needed);
/* ResolveClipIndex: TRI_E_INVALID when the asset has no clip of that name. */
int trident_anim_clip_index(uint64_t handle, const char* name, uint32_t* clip_index);
/* ResolveChannelBoneIndex of every channel of a clip (-1: skipped), as the player applies them. */
int trident_anim_resolve_channels(uint64_t handle, uint32_t clip_index, int32_t* bones, uint32_t capacity,
                                  uint32_t* count);
/* A fresh AnimationPlayer on (handle, handle, clip_index) evaluated at `time` (EvaluateAt + CopyPoseTo): *count
 * matrices, written to out when capacity allows. clip_index UINT32_MAX = no clip (the bind pose); an unknown handle
 * gives the fallback pose, one identity. */
int trident_anim_evaluate(uint64_t handle, uint32_t clip_index, float time, float* out, uint32_t capacity,
                          uint32_t* count);
/* Animation::EvaluatePoseProgram + ComposeSkinningMatrices on the asset: the float32 CPU meaning of a pose program
 * (include/tri_raster.h). A CLIP's `a` indexes the asset's clips; a BLEND / ADD's `a` indexes the masks given here
 * (mask m holds mask_counts[m] weights, concatenated in mask_weights) or is TRI_POSE_NO_MASK. No limit on length or
 * depth. TRI_E_INVALID: an unknown handle, a program that breaks the stack discipline, an unknown op, clip or mask. */
int trident_anim_eval_program(uint64_t handle, const tri_pose_op* ops, uint32_t op_count, const float* mask_weights,
                              const uint32_t* mask_counts, uint32_t mask_count, float* out, uint32_t capacity,
                              uint32_t* count);
/* ---- animation state machines and blend trees (host/include/trident/AnimationStateMachine.h), no GPU ----
 * Machines and nodes are named by ids (never 0). A node id is consumed when the node becomes a child of a blend node
 * or the root of a state; node id 0 stands for "no node". */
enum { TRIDENT_SM_FLOAT = 0, TRIDENT_SM_BOOL = 1, TRIDENT_SM_INTEGER = 2, TRIDENT_SM_TRIGGER = 3 };
enum { TRIDENT_SM_EQUALS = 0, TRIDENT_SM_NOT_EQUALS, TRIDENT_SM_GREATER, TRIDENT_SM_LESS, TRIDENT_SM_GREATER_EQUAL,
       TRIDENT_SM_LESS_EQUAL, TRIDENT_SM_TRIGGERED };
typedef struct trident_sm_condition {
    const char* parameter;
    int32_t comparison; /* TRIDENT_SM_EQUALS .. TRIDENT_SM_TRIGGERED */
    float float_value;
    int32_t int_value;
    int32_t bool_value;
} trident_sm_condition;
/* ClipNode (clip_index UINT32_MAX: no clip), BlendNode, BlendSpace1DNode; the parameter names may be NULL. */
int trident_node_clip(uint32_t clip_index, int looping, float speed, const char* speed_parameter, uint64_t* out_node);
int trident_node_blend(uint64_t first, uint64_t second, float weight, const char* weight_parameter, uint64_t* out_node);
int trident_node_blend_space(const uint32_t* clip_indices, const float* positions, uint32_t count, float parameter_default,
                             const char* parameter, uint64_t* out_node);
int trident_node_destroy(uint64_t node);
/* An AnimationStateMachine on the asset service with its two handles set (UINT64_MAX: invalid). */
int trident_sm_create(uint64_t skeleton_handle, uint64_t library_handle, uint64_t* out_machine);
int trident_sm_destroy(uint64_t machine);
int trident_sm_set_handles(uint64_t machine, uint64_t skeleton_handle, uint64_t library_handle);
/* add != 0: Add*Parameter(name, value); add == 0: Set*Parameter, and for a trigger FireTrigger (value != 0) or
 * ResetTrigger (value == 0). Bool: value != 0; Integer: (int)value. */
int trident_sm_parameter(uint64_t machine, const char* name, int type, float value, int add);
/* TRI_E_INVALID for a parameter the machine does not have. */
int trident_sm_get_parameter(uint64_t machine, const char* name, int* type, float* as_float, int* trigger_set);
int trident_sm_add_layer(uint64_t machine, const char* name, float weight, int additive, uint32_t* out_layer);
int trident_sm_set_layer_mask(uint64_t machine, uint32_t layer, const float* weights, uint32_t count);
int trident_sm_set_layer_weight(uint64_t machine, uint32_t layer, float weight);
int trident_sm_set_layer_entry(uint64_t machine, uint32_t layer, const char* state);
int trident_sm_add_state(uint64_t machine, uint32_t layer, const char* name, uint64_t root_node);
/* TRI_E_STATE: from_state is not a state of the layer (AddTransition's std::runtime_error). */
int trident_sm_add_transition(uint64_t machine, uint32_t layer, const char* from_state, const char* target_state,
                              int has_exit_time, float exit_time, float fade_duration,
                              const trident_sm_condition* conditions, uint32_t condition_count);
/* AnimationStateMachine::Update / CopyPose. */
int trident_sm_update(uint64_t machine, float dt);
int trident_sm_pose(uint64_t machine, float* out, uint32_t capacity, uint32_t* count);
/* The pose program the last update emitted (a CLIP's `a`: the library's clip index; a BLEND / ADD's `a`: a mask of
 * this program, read with trident_sm_program_mask, or TRI_POSE_NO_MASK). */
int trident_sm_program(uint64_t machine, tri_pose_op* ops, uint32_t capacity, uint32_t* count, uint32_t* mask_count);
int trident_sm_program_mask(uint64_t machine, uint32_t mask, float* weights, uint32_t capacity, uint32_t* count);
/* A layer's runtime state: the names of its current and next state ("" for none; either may be NULL) and its timers. */
int trident_sm_layer_state(uint64_t machine, uint32_t layer, char* current, char* next, uint32_t name_capacity,
                           float* time_in_state, float* transition_elapsed, float* transition_duration);
/* AnimationPlayer::Update on a player set to (time, speed, looping, playing): the time and play state after dt. */
int trident_anim_advance(uint64_t handle, uint32_t clip_index, float time, float speed, int looping, int playing,
                         float dt, float* out_time, int* out_playing);

/* ---- animated entities (ECS::AnimationSystem, host/include/trident/AnimationSystem.h) ---- */
/* The playback fields of an entity's AnimationComponent (added when absent): asset ids as registered with
 * trident_anim_register (NULL = empty), the clip name, time, speed, looping, playing. */
int trident_app_set_entity_animation(trident_app* app, uint32_t entity, const char* skeleton_asset_id,
                                     const char* animation_asset_id, const char* clip, float time, float speed,
                                     int looping, int playing);
/* AnimationComponent::m_StateMachine of an entity that has the component: the machine of trident_sm_create (shared
 * with its id, which keeps setting its parameters), or 0 to remove it. */
int trident_app_set_entity_state_machine(trident_app* app, uint32_t entity, uint64_t machine);
/* AnimationSystem::Update(registry, dt): poses into m_BoneMatrices, or time only in device mode. */
int trident_app_update_animation(trident_app* app, float dt);
/* AnimationSystem::InitialisePose of the entity's component. */
int trident_app_initialise_pose(trident_app* app, uint32_t entity);
/* The entity's pose: its m_BoneMatrices; for a component the device poses, evaluated on the CPU at its current time on demand.
 * *count matrices, written to out when capacity allows. */
int trident_app_entity_pose(trident_app* app, uint32_t entity, float* out, uint32_t capacity, uint32_t* count);
/* m_CurrentTime, m_IsPlaying and the cached {skeleton handle, animation handle, clip index} (UINT64_MAX: invalid). */
int trident_app_entity_animation_state(trident_app* app, uint32_t entity, float* time, int* playing, uint64_t handles[3]);
/* Renderer::SetDevicePoseEnabled (the app's animation system follows its renderer). */
int trident_app_set_device_pose(trident_app* app, int enabled);
/* Renderer::GetBonePaletteUploadCount. */
int trident_app_bone_palette_uploads(trident_app* app, uint64_t* count);

/* Renderer::GetViewportTexture: copies the viewport's image handle (TRI_E_STATE before its first frame). */
int trident_app_viewport_texture(trident_app* app, uint32_t viewport_id, tri_image* out);
/* Renderer::GetGeometryUploadCount. */
int trident_app_geometry_uploads(trident_app* app, uint64_t* count);
int trident_app_read_pixels(trident_app* app, uint32_t viewport_id, uint8_t* rgba, float* depth /* nullable */);

/* Frame inputs DrawFrame would submit for a viewport (host-only). */
int trident_app_frame_inputs(trident_app* app, uint32_t viewport_id, tri_global_ubo* ubo, tri_draw* draws,
                             uint32_t capacity, uint32_t* draw_count);
/* The concatenated geometry (pointers stay valid until the next mesh change). */
int trident_app_geometry(trident_app* app, const tri_vertex** vertices, size_t* vertex_count,
                         const uint32_t** indices, size_t* index_count, tri_mesh_range* ranges, uint32_t capacity,
                         uint32_t* range_count);
int trident_app_materials(trident_app* app, tri_material_record* out, uint32_t capacity, uint32_t* count);
/* Renderer::GetFrameTimingStats: min/max/avg ms, min/max/avg fps, sample count. */
int trident_app_frame_timing(trident_app* app, double out[7]);

#ifdef __cplusplus
}
#endif

#endif /* TRIDENT_APP_H */
