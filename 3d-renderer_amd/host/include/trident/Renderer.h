// Renderer.h — Trident::Renderer, the reference's renderer API (Trident/src/Renderer/Renderer.h:77-598)
// for the draw path, backed by the HIP software rasterizer through the C-ABI (include/tri_raster.h)
// instead of Vulkan. Same names, argument meaning and error behaviour (no exceptions on the frame
// path; failures are logged and the frame is skipped, Renderer.cpp:779-824). Vulkan-typed getters
// become opaque device pointers (GetViewportTexture).
#pragma once

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../../include/tri_raster.h"
#include "Camera.h"
#include "Scene.h"
#include "AnimationStateMachine.h"
#include "FrameDatasetRecorder.h"
#include "FrameGenerator.h"
#include "VideoEncoder.h"
#include "TextRenderer.h"

namespace Trident {

struct ViewportInfo {
    uint32_t ViewportID = 0;
    glm::vec2 Position{0.0f};
    glm::vec2 Size{0.0f};
};

struct FrameTimingSample {
    double FrameMilliseconds = 0.0;
    double FramesPerSecond = 0.0;
    std::chrono::system_clock::time_point CaptureTime{};
};

struct FrameTimingStats {  // Renderer.h:472-479
    double MinimumMilliseconds = 0.0;
    double MaximumMilliseconds = 0.0;
    double AverageMilliseconds = 0.0;
    double MinimumFPS = 0.0;
    double MaximumFPS = 0.0;
    double AverageFPS = 0.0;  // mean of per-frame 1000/ms (Renderer.cpp:6335-6342)
};

class Renderer {
public:
    Renderer();
    ~Renderer();

    void Init();
    void Shutdown();
    void DrawFrame();

    void UploadMesh(const std::vector<Geometry::Mesh>& meshes, const std::vector<Geometry::Material>& materials,
                    const std::vector<std::string>& textures);
    void AppendMeshes(std::vector<Geometry::Mesh> meshes, std::vector<Geometry::Material> materials,
                      std::vector<std::string> textures);
    void UploadTexture(const std::string& texturePath, const Loader::TextureData& texture);
    void SetEditorCamera(Camera* camera) { m_EditorCamera = camera; }
    void SetRuntimeCamera(Camera* camera) { m_RuntimeCamera = camera; }
    void SetRuntimeCameraReady(bool ready) { m_RuntimeCameraReady = ready; }
    void SetActiveRegistry(ECS::Registry* registry) { m_Registry = registry; }
    bool HasRuntimeCamera() const { return m_RuntimeCamera != nullptr && m_RuntimeCameraReady; }

    int32_t ResolveTextureSlot(const std::string& texturePath);
    size_t GetOrCreatePrimitiveMeshIndex(MeshComponent::PrimitiveType primitiveType);

    void SetClearColor(const glm::vec4& color) { m_ClearColor = color; }
    // The AI frame blend of Default.frag (:182-191). SetAiBlendStrength clamps to [0, 1] (Renderer.cpp:2533-2538,
    // default 0.35, Renderer.h:508). SubmitAiInterpolation takes a generated frame the way UploadAiInterpolationToGpu
    // does (Renderer.cpp:1560-1700): width * height * channels floats, each clamped to [0, 1] and rounded to a UNORM8
    // byte, alpha 1 when the frame has fewer than four channels; every viewport then blends with it (UpdateUniformBuffer
    // packs AiBlendConfig = (strength, 1 / width, 1 / height, 1) while a frame is held, :5916-5921). nullptr or an
    // empty frame drops it (the blend is off again). The frame generator (ONNX Runtime) itself stays outside.
    void SetAiBlendStrength(float blendStrength) { m_AiBlendStrength = std::min(std::max(blendStrength, 0.0f), 1.0f); }
    float GetAiBlendStrength() const { return m_AiBlendStrength; }
    bool SubmitAiInterpolation(const float* pixels, uint32_t width, uint32_t height, uint32_t channels);
    bool HasAiFrame() const { return m_AiWidth != 0 && m_AiHeight != 0; }
    // Replaces the skybox cubemap (CreateSkyboxCubemap, Renderer.cpp:3818-4110). Init installs the
    // reference's fallback, a solid 0x808080 cubemap (:3925-3926). An invalid cubemap is rejected
    // and logged; returns false in that case.
    bool SetSkyboxCubemap(const Loader::CubemapTextureData& cubemap);
    // Where CreateSkyboxCubemap looks for Skyboxes/ (the reference: "Assets", next to the executable,
    // Renderer.cpp:3830). Changing it re-runs the discovery; GetSkyboxSource names what was loaded
    // ("PNG fallback", "Default directory", ... or "solid 0x808080").
    void SetAssetsDirectory(const std::string& directory);
    // Text overlay (Renderer::SubmitText, Renderer.h:229, Renderer.cpp:6065-6079 -> TextRenderer::QueueText): queues
    // `text` for the viewport's next DrawFrame, drawn inside its pass after the sprites (the library's text pass,
    // tri_set_text) and therefore part of everything that takes the target afterwards: the pixels, the present blit,
    // a recorded frame, the AI tensor. The queue is cleared every DrawFrame; empty text is ignored; text for a viewport
    // id that does not render this frame is dropped, and the legacy present path draws none (the reference records
    // text for viewport contexts only). The first SubmitText loads <assets directory>/Fonts/JetBrainsMono-Regular.ttf
    // at 32 px unless SetTextFont named a font; without a font an error is logged once and text is absent.
    void SubmitText(uint32_t viewportId, const glm::vec2& position, const glm::vec4& color, const std::string& text);
    // Names the font file and pixel height instead of the default; false (the previous font stays) when it cannot
    // be loaded. Waits for the frames in flight.
    bool SetTextFont(const std::string& path, float pixelHeight);
    const std::string& GetSkyboxSource() const { return m_SkyboxSource; }
    glm::vec4 GetClearColor() const { return m_ClearColor; }

    size_t GetModelCount() const { return m_ModelCount; }
    size_t GetTriangleCount() const { return m_TriangleCount; }
    const FrameTimingStats& GetFrameTimingStats() const { return m_PerformanceStats; }
    size_t GetFrameTimingHistoryCount() const { return m_PerformanceSampleCount; }

    void SetViewport(uint32_t viewportId, const ViewportInfo& info);  // also makes it the active viewport
    // Swapchain extent stand-in (Swapchain.cpp): when set, DrawFrame ends by blitting the active
    // viewport onto a present image of this size with linear filtering (Renderer.cpp:5346-5361). With no
    // active viewport rendered this frame (none registered, or the active one has no target), it renders
    // the skybox, meshes and sprites straight into the present image at this extent instead — the legacy
    // direct-to-swapchain path (Renderer.cpp:5233, :5498-5590), camera from GetActiveCamera().
    void SetPresentExtent(uint32_t width, uint32_t height) { m_PresentWidth = width; m_PresentHeight = height; }
    // The last presented image (RGBA8 rows, BGRA reordered) and its size; false before a present.
    bool ReadPresentPixels(std::vector<uint8_t>& rgba, uint32_t& width, uint32_t& height);
    // Wait for the frame the last DrawFrame submitted (its viewport passes and present blit), re-rendering a pass
    // that outgrew the internal queues. DrawFrame itself calls it first, for the previous frame — the reference waits
    // for the previous frame's timeline value at the start of DrawFrame (Renderer.cpp:752-772) — so the caller's host
    // work between frames overlaps the GPU. The readers (ReadViewportPixels, ReadPresentPixels, GetViewportTexture)
    // call it on demand.
    void FinishFrame();
    // Frames in flight (1..4; default 1, the reference's pacing: DrawFrame waits for the previous frame's timeline
    // value). With n > 1 every single-device viewport keeps n render targets and frame k renders into target k mod n,
    // so DrawFrame waits only for frame k - n + 1 and the next frames' vertex and set-up work overlaps this frame's
    // raster (the C-ABI bench's contexts in flight, through the engine API). GetViewportTexture / ReadViewportPixels
    // return the latest frame's target. Multi-device viewports (SetDeviceCount > 1) keep 1 (tri_group double-buffers
    // its own frame). Changing it waits for every frame in flight and rebuilds the targets at the next DrawFrame.
    void SetFramesInFlight(uint32_t n);
    uint32_t GetFramesInFlight() const { return m_FramesInFlight; }
    // Viewport recording (Renderer.h:205-220, Renderer.cpp:6171-6284; width and height replace the VkExtent2D).
    // Enabling rounds an odd width or height up to the next even value (with a warning), starts a Y4M session at
    // that extent with fps 1 (the header reads F1:1, as the reference's) and pins the viewport's target to it: while
    // recording, SetViewport of that id keeps the recording extent (the reference guards the layout's resize the
    // same way, Renderer.cpp:2813-2818). A start the encoder refuses (an FFmpeg container, another extension, a
    // zero extent), or a request while SetDeviceCount > 1, leaves recording off, resizes nothing and returns false.
    // Enabling while already recording finalises the running file first. Disabling finishes the frames in flight,
    // finalises the file and always returns true; so do Shutdown and a SetDeviceCount above 1.
    // While recording, every DrawFrame that renders the recorded viewport writes exactly one FRAME record holding
    // that frame's pixels, in submission order (the reference delivers its readback one frame late): the frame is
    // converted on the device behind its render pass (tri_recorder_capture) and written when its fence is waited for.
    bool SetViewportRecordingEnabled(bool enabled, uint32_t viewportId, uint32_t width, uint32_t height,
                                     const std::string& outputPath);
    bool IsViewportRecording() const { return m_Recording; }
    // An outputPath ending in .mkv (any case) records Motion-JPEG in Matroska instead: each frame is encoded on the
    // device (tri_recorder_create_ex, TRI_RECORD_JPEG420) behind its pass and reaches the file as one SimpleBlock
    // through VideoEncoder::SubmitJpeg; every rule above holds unchanged, "FRAME record" read as "block". The quality
    // (1..100, default 90; values outside are clamped) applies from the next session.
    void SetRecordingQuality(int quality) { m_RecordingQuality = quality < 1 ? 1u : (quality > 100 ? 100u : (uint32_t)quality); }
    int GetRecordingQuality() const { return (int)m_RecordingQuality; }
    uint32_t GetRecordingViewportId() const { return m_RecordingViewportId; }  // meaningful while recording
    void GetRecordingExtent(uint32_t& width, uint32_t& height) const { width = m_RecordingWidth; height = m_RecordingHeight; }
    uint64_t GetRecordedFrameCount() const { return m_VideoEncoder.GetFrameCount(); }  // of the current or last session
    // Frame readback for AI consumers (SetReadbackEnabled / ResolvePendingReadback / TryAcquireRenderedFrame,
    // Renderer.cpp:984-995, :1111-1389). SetAiReadbackEnabled stands in for m_FrameGenerator.IsInitialised() in the
    // reference's l_ReadbackRequired (:787) for a generator that lives outside the library and says so here (the
    // generator inside, LoadAiModel below, turns it on itself). While enabled,
    // a DrawFrame that renders the active viewport on one device converts it on the device, behind its pass, into a
    // channels-last RGBA float tensor (tri_framegrab, one slot per frame in flight; each value float(byte) *
    // (1.0f / 255.0f)), provided the readback throttle has elapsed at submission; when a present extent is set and
    // differs from the viewport's, nothing is captured (the reference skips the copy, :5301-5337). The frame's fence
    // resolves the capture (again after an overflow re-render, as recording does): its floats become the pending
    // readback, a newer frame replacing an unconsumed one. Refused (false) while SetDeviceCount > 1, which also turns
    // it off. Independent of viewport recording.
    bool SetAiReadbackEnabled(bool enabled);
    bool IsAiReadbackEnabled() const { return m_AiReadback; }
    // The readback and inference throttles in milliseconds (Renderer.h:522-523: 66 and 66); 0 disables one.
    void SetAiThrottleIntervals(uint32_t readbackMs, uint32_t inferenceMs);
    // The pending tensor, once: true moves it into `out` (width * height * 4 floats) and clears it (:984-995). Subject
    // to the inference throttle (:933-940): false until it has elapsed since the last acquisition. When dataset
    // capture is on, the tensor is recorded as the input sample with shape {1, H, W, 4} (:973-977). Public here
    // because the generator is outside.
    bool TryAcquireRenderedFrame(std::vector<float>& out);
    // The same into the caller's memory (`capacity` floats; too few: false, and the tensor stays pending). Until the
    // next DrawFrame the pending tensor still lies in the grab's pinned buffer, so this is its only host copy.
    bool TryAcquireRenderedFrame(float* out, size_t capacity);
    void GetFrameReadbackExtent(uint32_t& width, uint32_t& height) const { width = m_FrameReadbackWidth; height = m_FrameReadbackHeight; }
    // The latest resolved tensor where it was made, for a consumer on the same device: valid until the next
    // DrawFrame. false before the first resolved frame.
    bool GetFrameReadbackDeviceTensor(const float** device, uint32_t& width, uint32_t& height);
    // The generator's output (ProcessAiFrame, Renderer.cpp:913-931): `shape` must have rank 3 (HWC) or 4 (NHWC), else
    // false and nothing changes. Dimensions <= 0 fall back to the readback extent and channel count. The data is
    // normalised as NormaliseAndReorderAiOutput does (:358-415: scaled by 1/255 when max > 1 + 1e-3 or min < -1e-3,
    // channels 0 and 2 swapped when there are at least 3, clamped to [0, 1]), recorded as the oldest pending
    // sample's output when dataset capture is on, and handed to SubmitAiInterpolation at the canonical shape.
    bool SubmitAiOutput(const float* data, size_t count, const int64_t* shape, size_t rank);
    // The normalisation alone, in place, on whole pixels of `channels` floats (unchanged, with a log line, for a
    // channel count <= 0 or one that does not divide the element count).
    static void NormaliseAndReorderAiOutput(std::vector<float>& data, int64_t channels);
    // The frame generator on the device (Renderer::ProcessAiFrame, Renderer.cpp:839-982; TryInitialiseAiModel /
    // ResolveAiModelPath, :1077-1108, :1743-1782). ResolveAiModelPath tries TRIDENT_AI_MODEL, then
    // Assets/AI/frame_generator.trifgen under the working directory and its two parents (the reference's search with
    // the container's extension for .onnx); "" when nothing is found. While no model is initialised the search is
    // retried once a second from ProcessAiFrame. LoadAiModel names a container explicitly: false (GetAiModelError()
    // says why, and names the tensor) for a missing or damaged file, and while SetDeviceCount > 1. An initialised
    // generator turns the AI readback on, as m_FrameGenerator.IsInitialised() does in the reference (:787).
    //
    // ProcessAiFrame runs where a frame's fence resolves its capture (DrawFrame's fence, FinishFrame), in the
    // reference's order: (1) a finished output is packed on the device into the blend frame of every viewport target
    // (HasAiFrame and AiBlendConfig then behave as after SubmitAiInterpolation) and, only with dataset capture on, copied
    // to the host, normalised and recorded; (2) when the inference throttle has elapsed, no job is in flight and a
    // fresh tensor is held, its element count is checked against the model's input (a 6-channel model, or an extent
    // that is no multiple of 4, warns once and skips, :957-963) and (3) the held device tensor is submitted, its host
    // copy recorded as the sample's input when capture is on. The manual path (TryAcquireRenderedFrame, SubmitAiOutput,
    // SubmitAiInterpolation) stays as it is; a tensor either path consumed is gone for the other.
    struct AiDebugStats {  // Renderer.h:99-110
        bool m_ModelInitialised = false;
        size_t m_PendingJobCount = 0;
        uint64_t m_CompletedInferenceCount = 0;
        double m_LastInferenceMilliseconds = 0.0;
        double m_AverageInferenceMilliseconds = 0.0;
        bool m_TextureReady = false;
        float m_BlendStrength = 0.0f;
        struct Extent { uint32_t width = 0, height = 0; } m_TextureExtent;
        double m_ReservedMetric = 0.0;
    };
    std::string ResolveAiModelPath() const;
    bool TryInitialiseAiModel();
    bool LoadAiModel(const std::string& path);
    const std::string& GetAiModelError() const { return m_FrameGenerator.GetLastError(); }
    const AI::FrameGenerator& GetFrameGenerator() const { return m_FrameGenerator; }
    // The snapshot ProcessAiFrame and FinishAiInference last took (all zeros before the first).
    AiDebugStats GetAiDebugStats() const { return m_AiDebugStats; }
    // Polls until the job in flight has finished and consumes it as ProcessAiFrame's step (1) does; true at once without
    // a job. false when timeoutMs expires first (the job stays in flight).
    bool FinishAiInference(uint32_t timeoutMs = 5000);
    // The blend frame of the active viewport's latest target as the device holds it: width * height R8G8B8A8 texels.
    bool ReadAiBlendFrame(std::vector<uint8_t>& rgba, uint32_t& width, uint32_t& height);
    // Frame dataset capture (Renderer.cpp:2498-2525, :6393-6400). Init honours TRIDENT_DATASET_CAPTURE_ENABLE (any
    // non-empty value) and TRIDENT_DATASET_CAPTURE_DIR (:551-576). Disabling and Shutdown write what is queued.
    void SetFrameDatasetCaptureEnabled(bool enabled);
    void SetFrameDatasetCaptureDirectory(const std::string& directory);  // empty: current_path()/DatasetCapture
    void SetFrameDatasetCaptureInterval(uint32_t interval);              // at least 1
    bool IsFrameDatasetCaptureEnabled() const { return m_FrameDatasetCaptureEnabled; }
    const std::string& GetFrameDatasetCaptureDirectory() const { return m_FrameDatasetCaptureDirectory; }
    uint32_t GetFrameDatasetCaptureInterval() const { return m_FrameDatasetCaptureInterval; }
    uint32_t GetActiveViewportId() const { return m_ActiveViewportId; }
    ViewportInfo GetViewport() const;
    // Vulkan returned a VkDescriptorSet for ImGui (Renderer.h:235); here: an opaque handle, a pointer to
    // the viewport's tri_image (device pointer, size, pitch, B8G8R8A8_UNORM, device ordinal) that an ImGui
    // HIP/GL-interop backend can display. nullptr before the viewport's first frame; valid until its next
    // resize or Shutdown.
    void* GetViewportTexture(uint32_t viewportId) const;
    // Shadow-map pre-pass (BASELINE config 5): the reference reserves LightComponent::m_ShadowCaster
    // (LightComponent.h:33) without rendering shadows; here, when the directional light UpdateUniformBuffer
    // picks (the first enabled one) is a shadow caster, every viewport renders a size x size map fitted
    // to the visible draws' world box (tri_shadow_fit_ortho) first. 0 disables the pass entirely.
    void SetShadowMapSize(uint32_t size) { m_ShadowMapSize = size; }
    // The pre-pass configuration DrawFrame uses this frame (false: no shadow-casting sun).
    bool BuildShadowConfig(tri_shadow_config& out);
    // How many times the concatenated geometry went to the device: once per UploadMeshFromCache
    // generation, shared by every viewport (the reference binds one vertex/index buffer for all).
    uint64_t GetGeometryUploadCount() const { return m_GeometryUploads; }
    const Camera* GetActiveCamera() const;
    glm::mat4 GetViewportViewMatrix(uint32_t viewportId) const;
    glm::mat4 GetViewportProjectionMatrix(uint32_t viewportId) const;

    std::vector<Geometry::Material>& GetMaterials() { return m_Materials; }
    const std::vector<Geometry::Material>& GetMaterials() const { return m_Materials; }

    // Entity ids (tri_set_id_output and its readers): which entity a pixel of a viewport shows, for clicks in a viewport
    // panel, rectangle selection, segmentation masks beside the colour tensor, and the selection outline.
    // SetSelectedEntity has the reference's name and meaning (Renderer.cpp:6053: it stores the entity); kNoEntity
    // selects nothing. Every frame keeps, per target, the draw index -> entity table of the draw list it submitted
    // (mesh commands, then sprites), so the readers answer for the latest finished frame of the viewport: they fence
    // like ReadViewportPixels, and each ring target (SetFramesInFlight) carries its own id image and table.
    static constexpr ECS::Entity kNoEntity = 0xFFFFFFFFu;
    void SetSelectedEntity(ECS::Entity entity) { m_SelectedEntity = entity; }
    ECS::Entity GetSelectedEntity() const { return m_SelectedEntity; }
    // From the viewport's next DrawFrame on, its frames carry ids (off: they stop, unless the outline needs them).
    void SetEntityIdOutputEnabled(uint32_t viewportId, bool enabled);
    // The entity at pixel (x, y) of the viewport's latest frame and, optionally, its depth in [0, 1]. false on
    // background, outside the viewport, for a viewport that does not exist or whose latest frame carries no ids.
    bool PickEntity(uint32_t viewportId, int32_t x, int32_t y, ECS::Entity& out, float* depth01 = nullptr);
    // The distinct entities with a pixel inside the inclusive rectangle (clamped to the viewport), in draw order.
    std::vector<ECS::Entity> PickEntitiesInRect(uint32_t viewportId, int32_t x0, int32_t y0, int32_t x1, int32_t y1);
    // The entity of every pixel (width * height, rows top to bottom), `background` where there is none.
    bool ReadViewportEntityIds(uint32_t viewportId, std::vector<uint32_t>& out, uint32_t background = 0xFFFFFFFFu);
    // Outlines every draw of the selected entity in every single-device viewport that renders it (tri_set_outline: an
    // outer outline of the visible silhouette, widthPx in 1..8, under the text), and turns the id output on for those
    // viewports. Refused with a log line (the outline stays off) while SetDeviceCount > 1, which also turns it off:
    // a band's halo lies in another band.
    void SetSelectionOutline(bool enabled, const glm::vec4& colour = glm::vec4(1.0f, 0.6f, 0.0f, 1.0f), uint32_t widthPx = 2);
    bool IsSelectionOutlineEnabled() const { return m_SelectionOutline; }

    // Motion vectors (tri_set_motion_output and its readers): per pixel of a viewport, where the surface it shows lay
    // one frame ago, minus the pixel, in pixels (x right, y down) — for frame interpolation and extrapolation, temporal
    // reprojection and training data. From the viewport's next DrawFrame on its frames carry motion; the request also
    // turns the viewport's id output on (the pass reads the ids), as the outline does. History is kept per VIEWPORT,
    // not per ring target: the view and projection of the viewport's last rendered frame and an entity -> model map
    // of that frame's draws, so frame k's history is frame k - 1's whatever SetFramesInFlight is. A viewport's first
    // frame with the output on, and the first after a resize, have no history: their motion is all zero. An entity
    // without an entry (new, just made visible, a sprite's first frame) takes its current model as the previous one:
    // camera motion only. Skinned draws get the rigid motion of their model matrix; per-bone motion is not computed.
    // Refused with a log line while SetDeviceCount > 1, which also turns the output off.
    void SetMotionVectorOutputEnabled(uint32_t viewportId, bool enabled);
    bool IsMotionVectorOutputEnabled(uint32_t viewportId) const;
    // width * height * 2 floats (x then y, rows top to bottom) of the viewport's latest frame (fences); false for a
    // viewport that does not exist or whose latest frame carries no motion.
    bool ReadViewportMotionVectors(uint32_t viewportId, std::vector<float>& out);
    // An opaque pointer to the tri_image of the motion image (R32G32_SFLOAT, pitch width * 8), valid like
    // GetViewportTexture's; null where ReadViewportMotionVectors returns false.
    void* GetViewportMotionTexture(uint32_t viewportId);

    // History reprojection (tri_history): behind each of the viewport's frames, the previous frame's colour fetched
    // where the pixel's motion vector points, and a mask byte per pixel that says where that fetch is not valid
    // (TRI_REPROJECT_*: no history, no projection, outside the frame, another entity, beyond depthTolerance in depth;
    // 0: valid) — what temporal accumulation, frame extrapolation and a warped baseline for the frame generator start
    // from. The request turns the viewport's id and motion outputs on, as motion turns ids on. One history per
    // VIEWPORT, not per ring target: frame k is warped from frame k - 1 whatever SetFramesInFlight is. No history
    // (mask 1 everywhere, the current colour): the viewport's first frame, the first after a resize, the first after
    // the switch goes on. The colour is the frame's as the viewport shows it, text and outline included. A frame
    // re-rendered after a queue overflow is reprojected again; with several frames in flight the frame after it had
    // already read it, so the history is reset instead. Refused with a log line while SetDeviceCount > 1 (which also
    // turns it off), and for a negative or non-finite tolerance.
    void SetHistoryReprojectionEnabled(uint32_t viewportId, bool enabled, float depthTolerance = 0.0f);
    bool IsHistoryReprojectionEnabled(uint32_t viewportId) const;
    // width * height * 4 bytes (B G R A) and width * height mask bytes of the viewport's latest frame (fences); false
    // for a viewport that does not exist or whose latest frame was not reprojected.
    bool ReadViewportReprojection(uint32_t viewportId, std::vector<uint8_t>& bgra, std::vector<uint8_t>& mask);
    // Opaque pointers to the tri_image of the warped colour (B8G8R8A8_UNORM) and of the mask (R8_UINT, pitch width),
    // valid until the viewport is resized or the switch goes off; null where ReadViewportReprojection returns false.
    void* GetViewportReprojectedTexture(uint32_t viewportId);
    void* GetViewportDisocclusionTexture(uint32_t viewportId);

    // Temporal anti-aliasing (tri_taa): while it is on, each DrawFrame of the viewport renders with its projection
    // moved inside the pixel — tri_taa_jitter(frameIndex, period), frameIndex counting the viewport's frames from 0
    // since the switch went on or the last resize — and resolves the frame over the viewport's accumulated, clamped
    // history (weight alpha for the current frame; rejectIds: the 3 x 3 entity test). The request turns the viewport's
    // id and motion outputs on; the motion history keeps the UNJITTERED projection and is handed on under the current
    // jitter, so still geometry maps to itself and nothing blurs. One tri_taa per VIEWPORT, not per ring target; a
    // resize makes a new one, switching on resets it. Behind the viewport's tri_render and before the history
    // reprojection. A frame re-rendered after a queue overflow is resolved again (redo); with several frames in
    // flight the history is reset instead, as for the history reprojection. While it is on for the active viewport,
    // the present blit and ReadPresentPixels show the RESOLVED image. GetViewportTexture, ReadViewportPixels, the
    // recording, the AI tensor and the dataset samples keep taking the context's raw, jittered frame. Refused with a
    // log line while SetDeviceCount > 1 (which also turns it off), for an alpha outside (0, 1] and for a period
    // above 64.
    void SetTemporalAntiAliasingEnabled(uint32_t viewportId, bool enabled, float alpha = 0.1f, uint32_t period = 8,
                                        bool rejectIds = true);
    bool IsTemporalAntiAliasingEnabled(uint32_t viewportId) const;
    // width * height * 4 bytes, R G B A like ReadViewportPixels, of the viewport's latest resolved frame (fences); false
    // for a viewport that does not exist or whose latest frame was not resolved.
    bool ReadViewportResolvedPixels(uint32_t viewportId, std::vector<uint8_t>& rgba);
    // width * height mask bytes (TRI_TAA_*) of the same frame.
    bool ReadViewportTaaMask(uint32_t viewportId, std::vector<uint8_t>& mask);
    // Opaque pointer to the tri_image of the resolved colour (B8G8R8A8_UNORM), valid until the viewport is resized or
    // the switch goes off; null where ReadViewportResolvedPixels returns false.
    void* GetViewportResolvedTexture(uint32_t viewportId);

    // Temporal upscaling (tri_upscale): while it is on, the viewport's context is made at
    // max(1, (uint32_t)(size * renderScale + 0.5f)) per axis, each DrawFrame renders it under
    // tri_taa_jitter(frameIndex, tri_upscale_jitter_period(...)) over that RENDER extent (the motion history keeps the
    // unjittered projection, as for temporal anti-aliasing) and resolves it over a history kept at the viewport's full
    // size (weight alpha for a sample on a pixel's centre; rejectIds: the 3 x 3 entity test). The request turns the id
    // and motion outputs on. One tri_upscale per VIEWPORT; a resize or another scale makes a new one and restarts the
    // frame index; redo and reset as for temporal anti-aliasing. While it is on for the active viewport, the present
    // blit and ReadPresentPixels show the UPSCALED image. ReadViewportPixels, GetViewportTexture, the id and motion
    // readers, the AI tensor (TryAcquireRenderedFrame, GetFrameReadbackDeviceTensor; GetFrameReadbackExtent says its
    // extent) and the dataset samples made from it keep the raw frame AT THE RENDER EXTENT; the readback's present-extent
    // condition compares the viewport's size. PickEntity and PickEntitiesInRect keep taking viewport pixels. Text and the
    // selection outline are drawn at the render extent (text positions scaled to it) and enlarged with the frame.
    // A viewport is NOT recorded while it is upscaled: a recording session has one fixed extent, the viewport's size, so
    // the request is refused on a viewport that is being recorded, and SetViewportRecordingEnabled is refused for a
    // viewport that has it on.
    // Refused with a log line, the switch staying as it was: a renderScale outside [1/3, 1] or one whose render extent
    // breaks tri_upscale_create's extent rule for the viewport's size, an alpha outside (0, 1], a viewport with
    // temporal anti-aliasing on (and SetTemporalAntiAliasingEnabled is refused while this is on), SetDeviceCount > 1
    // (which also turns it off). Returns whether the request was taken.
    bool SetTemporalUpscalingEnabled(uint32_t viewportId, bool enabled, float renderScale = 0.5f, float alpha = 0.1f,
                                     bool rejectIds = true);
    bool IsTemporalUpscalingEnabled(uint32_t viewportId) const;
    // The viewport's full size: width * height * 4 bytes, R G B A, of its latest upscaled frame (fences); false for a
    // viewport that does not exist or whose latest frame was not upscaled. width / height (may be null) get the extent.
    bool ReadViewportUpscaledPixels(uint32_t viewportId, std::vector<uint8_t>& rgba, uint32_t* width = nullptr,
                                    uint32_t* height = nullptr);
    // width * height mask bytes (TRI_UPSCALE_*) of the same frame.
    bool ReadViewportUpscaleMask(uint32_t viewportId, std::vector<uint8_t>& mask);
    // Opaque pointer to the tri_image of the upscaled colour (B8G8R8A8_UNORM), valid until the viewport is resized, the
    // scale changes or the switch goes off; null where ReadViewportUpscaledPixels returns false.
    void* GetViewportUpscaledTexture(uint32_t viewportId);

    // Frame readback (ResolvePendingReadback, Renderer.cpp:1299-1389): RGBA8 rows of the viewport
    // (BGRA reordered to RGBA), optionally the D32 depth.
    bool ReadViewportPixels(uint32_t viewportId, std::vector<uint8_t>& rgba, std::vector<float>* depth = nullptr);
    // The exact uniform block + draw list DrawFrame submits for a viewport (GatherMeshDraws +
    // UpdateUniformBuffer + the push-constant loop): host-only, used to test frame preparation. Id 0 with
    // no viewport registered: the legacy present pass's inputs (GetActiveCamera()).
    bool BuildFrameInputs(uint32_t viewportId, tri_global_ubo& ubo, std::vector<tri_draw>& draws);
    // Rasterizer flags (TRI_FLAG_*) used for viewports created from now on.
    void SetRasterFlags(uint32_t flags) { m_RasterFlags = flags; }
    // Multi-device viewports (SURVEY 8(b) tri_config.device_count, 8(e)): with count > 1 every viewport
    // renders as a tri_group of `count` row bands on `devices` (default 0 .. count-1; an ordinal may
    // repeat), the frame assembled on the first band's device over RCCL; count <= 1 is one context per
    // viewport (the default). Existing viewport targets are rebuilt at the next DrawFrame. The geometry
    // goes to each distinct device once per generation and is shared by every viewport there. Returns
    // false (and changes nothing) for an invalid device list.
    bool SetDeviceCount(uint32_t count, const std::vector<int32_t>& devices = {});
    uint32_t GetDeviceCount() const { return (uint32_t)std::max<size_t>(m_Devices.size(), 1); }
    // Device poses (default off): the one switch. When on, a draw whose AnimationComponent has a valid skeleton handle,
    // and whose asset the device path takes (Animation::DevicePoseCompatible), is posed by tri_pose_palette at the
    // component's clip and time (no valid clip: the bind pose) behind the uploaded palette; its m_BoneMatrices are not
    // read, and an ECS::AnimationSystem made with this renderer only advances its time. Every other animated draw goes
    // through the uploaded prefix as before. Assets reach a device once, at their first use there; after any
    // registration with the asset service (AnimationAssetService::GetGeneration) they are looked at and sent again.
    void SetDevicePoseEnabled(bool enabled) { m_DevicePose = enabled; }
    // Whether this renderer poses the component's draw on the device (false while device poses are off).
    bool PosesOnDevice(const AnimationComponent& component) const;
    bool IsDevicePoseEnabled() const { return m_DevicePose; }
    // Host uploads of a bone palette (tri_upload_bone_palette calls) since Init.
    uint64_t GetBonePaletteUploadCount() const { return m_BonePaletteUploads; }
    bool IsShutdown() const { return m_Shutdown; }
    // The concatenated buffers UploadMeshFromCache builds (the device copy of these is what
    // tri_upload_geometry receives).
    const std::vector<tri_vertex>& GetVertexBuffer() const { return m_VertexBuffer; }
    const std::vector<uint32_t>& GetIndexBuffer() const { return m_IndexBuffer; }
    std::vector<tri_mesh_range> GetMeshRanges() const;

private:
    struct MeshDrawInfo {  // Renderer.h:293-299
        uint32_t m_FirstIndex = 0;
        uint32_t m_IndexCount = 0;
        int32_t m_BaseVertex = 0;
        int32_t m_MaterialIndex = -1;
    };
    struct MeshDrawCommand {
        glm::mat4 m_ModelMatrix{1.0f};
        const MeshComponent* m_Component = nullptr;
        const TextureComponent* m_TextureComponent = nullptr;
        const AnimationComponent* m_AnimationComponent = nullptr;
        uint32_t m_BoneOffset = 0;
        uint32_t m_BoneCount = 0;
        ECS::Entity m_Entity = 0;
    };
    struct SpriteDrawCommand {  // Renderer.h SpriteDrawCommand: one visible SpriteComponent per frame
        glm::mat4 m_ModelMatrix{1.0f};
        const SpriteComponent* m_Component = nullptr;
        const TextureComponent* m_TextureComponent = nullptr;
        ECS::Entity m_Entity = 0;
    };
    struct ViewportContext {
        ViewportInfo m_Info{};
        tri_ctx* m_Ctx = nullptr;      // one-device viewport
        tri_group* m_Group = nullptr;  // multi-device viewport (SetDeviceCount > 1)
        uint32_t m_Width = 0, m_Height = 0;
        uint64_t m_GeometryGeneration = 0, m_TextureGeneration = 0, m_MaterialGeneration = 0, m_SkyboxGeneration = 0;
        uint64_t m_AiGeneration = 0;
        // the generator's tensor is being rewritten by the job in flight, so this target (new or resized since the
        // output was consumed) renders without the blend until the next output is packed into it
        bool m_AiFrameDeferred = false;
        std::vector<float> m_BonePalette;  // the palette last uploaded to this viewport's context
        bool m_HasPosedSuffix = false;     // the last tri_pose_palette on this context had instances
        tri_shadow_config m_Shadow{};      // the pre-pass configuration last set on this context
        tri_image m_Image{};               // GetViewportTexture's handle (after the first frame)
        bool m_HasImage = false;
        // entity ids: the context's id output is on; the outline last set on it (draws and style) so that an unchanged
        // one is not set again; the entity of each draw of the frame last submitted to this target
        bool m_IdOutput = false, m_OutlineSet = false;
        std::vector<uint32_t> m_OutlineDraws;
        glm::vec4 m_OutlineColour{0.0f};
        uint32_t m_OutlineWidth = 0;
        std::vector<ECS::Entity> m_DrawEntities;
        // motion vectors: the context's motion output is on; its image
        bool m_MotionOutput = false;
        tri_image m_MotionImage{};
    };

    void CreateSkyboxCubemap();
    void UploadMeshFromCache();
    void EnsurePrimitiveMeshesInCache();
    size_t CreatePrimitiveMeshInCache(MeshComponent::PrimitiveType primitiveType);
    void ResolveMaterialTextureSlots(const std::vector<std::string>& textures, size_t offset, size_t count);
    void GatherMeshDraws();
    void GatherSpriteDraws();
    void GatherDraws();  // GatherMeshDraws + GatherSpriteDraws (adds the sprite quad to the geometry once)
    void PrepareBonePaletteBuffer();
    void UpdateUniformBuffer(const Camera* camera, tri_global_ubo& out) const;
    void BuildDrawList(std::vector<tri_draw>& out, std::vector<ECS::Entity>* entities = nullptr) const;
    // before the target's tri_render: the id output and the outline this frame wants on it
    bool SetTargetIds(ViewportContext& target, uint32_t viewportId, const std::vector<tri_draw>& draws,
                      const std::vector<ECS::Entity>& entities);
    const ViewportContext* IdTarget(uint32_t viewportId);  // fenced; null unless the latest frame carries ids
    // before the target's tri_render, after SetTargetIds: the motion output this frame wants on it, the viewport's
    // history as the context's, and this frame's camera and models as the history of the viewport's next frame
    // (ubo: the UNJITTERED block; jitter: null, or this frame's sub-pixel offset, under which the stored previous
    // projection is handed to the context — the temporal anti-aliasing's contract)
    bool SetTargetMotion(ViewportContext& target, uint32_t viewportId, const tri_global_ubo& ubo,
                         const std::vector<tri_draw>& draws, const std::vector<ECS::Entity>& entities,
                         const float* jitter = nullptr);
    const ViewportContext* MotionTarget(uint32_t viewportId);  // fenced; null unless the latest frame carries motion
    // the motion output a viewport's frames carry: asked for itself, by the history reprojection, or by the
    // temporal anti-aliasing
    bool WantsMotion(uint32_t viewportId) const {
        return IsMotionVectorOutputEnabled(viewportId) || IsHistoryReprojectionEnabled(viewportId) ||
               IsTemporalAntiAliasingEnabled(viewportId) || IsTemporalUpscalingEnabled(viewportId);
    }
    struct Upscale;
    // the extent a viewport's context is made at: its size, scaled while temporal upscaling is on for it
    void RenderExtent(const ViewportContext& target, uint32_t& width, uint32_t& height) const;
    // a viewport pixel (PickEntity, PickEntitiesInRect) as a pixel of the target's frame
    void ToFramePixel(const ViewportContext& target, int32_t& x, int32_t& y) const;
    // before the target's tri_render: this frame's jitter of the viewport (false: the switch is off, no jitter)
    bool BeginUpscaleFrame(const ViewportContext& target, uint32_t viewportId, float jitter[2]);
    // behind the target's tri_render: the frame resolved over the viewport's full-size history
    bool UpscaleTarget(ViewportContext& target, uint32_t viewportId, bool redo);
    struct Taa;
    // before the target's tri_render: this frame's jitter of the viewport (false: the switch is off, no jitter)
    bool BeginTaaFrame(const ViewportContext& target, uint32_t viewportId, float jitter[2]);
    // behind the target's tri_render: the frame resolved over the viewport's history (redo: it was rendered again)
    bool ResolveTarget(ViewportContext& target, uint32_t viewportId, bool redo);
    // the presentation blit of a target: its viewport's resolved image while that frame was resolved, else its colour
    int PresentBlit(ViewportContext& target, uint32_t width, uint32_t height);
    struct Reprojection;
    // behind the target's tri_render: the viewport's history warped by this frame (redo: the frame was rendered again)
    bool ReprojectTarget(ViewportContext& target, uint32_t viewportId, bool redo);
    // What the three passes above share, over m_Reprojection, m_Taa or m_Upscale (Renderer.cpp):
    // FinishOldestFrame re-rendered the target's frame: `pass` again as a redo when it was the object's last, else `reset`
    template <typename Map, typename Reset>
    void RedoTemporal(Map& records, ViewportContext& target, bool (Renderer::*pass)(ViewportContext&, uint32_t, bool),
                      Reset reset, const char* what);
    // fenced; the viewport's record, or null unless the latest frame went through its pass
    template <typename Map>
    typename Map::mapped_type* TemporalOutput(Map& records, uint32_t viewportId);
    // the viewport's object while the target's frame is the one it resolved last, else null (PresentBlit)
    template <typename Map>
    auto ResolvedBy(Map& records, const ViewportContext& target) -> decltype(records.begin()->second.m_Object);
    const Camera* GetActiveCamera(const ViewportContext& context) const;
    bool PrepareViewport(ViewportContext& context);
    // One viewport pass: pre-pass / palette / UBO / draws, then tri_render (asynchronous); false on error.
    bool SubmitTarget(ViewportContext& context, const tri_global_ubo& ubo, const std::vector<tri_draw>& draws,
                      const tri_shadow_config& shadow, bool shadowOn);
    void RecordFrameTiming(double milliseconds);

    Camera* m_EditorCamera = nullptr;
    Camera* m_RuntimeCamera = nullptr;
    bool m_RuntimeCameraReady = false;
    ECS::Registry* m_Registry = nullptr;

    std::vector<Geometry::Mesh> m_GeometryCache;
    std::vector<Geometry::Material> m_Materials;
    std::vector<MeshDrawInfo> m_MeshDrawInfo;
    std::vector<MeshDrawCommand> m_MeshDrawCommands;
    std::vector<SpriteDrawCommand> m_SpriteDrawList;
    // The sprite quad (BuildSpriteGeometry, Renderer.cpp:2853-2890): the reference keeps it in its own
    // vertex/index buffer; here it is one more mesh range after the cached meshes, appended to the
    // device geometry the first time a sprite is drawn (mesh index m_MeshDrawInfo.size()).
    bool m_HasSpriteGeometry = false;
    MeshDrawInfo m_SpriteDrawInfo{};
    static constexpr uint32_t s_MaxBonesPerSkeleton = 128;  // Renderer.h:291
    std::vector<float> m_BonePalette;  // PrepareBonePaletteBuffer's scratch: per-draw palettes, back to back
    // device poses: this frame's posed draws (PrepareBonePaletteBuffer), and per device the set with what it holds
    struct PoseDraw {
        size_t m_Skeleton, m_Animation, m_Clip;  // asset handles and the clip index
        float m_Time;
        uint32_t m_Offset;
        const Animation::PoseProgram* m_Program;  // a state machine's program of this update, or null: the clip at m_Time
    };
    struct PoseAssetOnDevice {
        uint32_t m_Skeleton = 0;
        std::vector<uint32_t> m_Clips;
        std::map<std::vector<float>, uint32_t> m_Masks;  // masks on the device by content (padded to the bone count)
    };
    struct PoseDeviceSet {
        tri_animset* m_Set = nullptr;
        std::map<std::pair<size_t, size_t>, PoseAssetOnDevice> m_Assets;  // by (skeleton handle, animation handle)
    };
    bool m_DevicePose = false;
    uint64_t m_BonePaletteUploads = 0;
    std::vector<PoseDraw> m_PoseDraws;
    mutable std::map<std::pair<size_t, size_t>, bool> m_PoseCompatible;  // DevicePoseCompatible per (skeleton, animation)
    mutable uint64_t m_PoseCompatibleGeneration = 0;  // the asset service's generation the cache was filled under
    uint64_t m_PoseSetsGeneration = 0;                // ... and the one the devices' sets were filled under
    std::map<int32_t, PoseDeviceSet> m_PoseSets;
    std::vector<tri_pose_instance> m_PoseInstances;
    std::vector<tri_pose_graph_instance> m_PoseGraphInstances;  // a frame with at least one program: every posed draw
    std::vector<tri_pose_op> m_PoseOps;
    bool SubmitPoses(ViewportContext& context);
    PoseAssetOnDevice* PoseAssetOn(int32_t device, size_t skeleton, size_t animation);
    bool SubmitPoseGraph(ViewportContext& context, const std::vector<int32_t>& devices);
    void DropPoseSets();
    size_t m_PrimitiveMeshIndices[3] = {SIZE_MAX, SIZE_MAX, SIZE_MAX};
    bool m_IsUploadingMeshes = false;
    tri_geometry* m_SharedGeometry = nullptr;  // the device copy every viewport context binds
    uint64_t m_SharedGeometryGeneration = 0;
    std::vector<int32_t> m_Devices;                 // SetDeviceCount's bands (empty: one context per viewport)
    std::vector<tri_geometry*> m_DeviceGeometry;    // multi-device: one shared copy per distinct device
    std::vector<uint64_t> m_DeviceGeometryGeneration;
    bool UploadSharedGeometry(std::vector<tri_geometry*>& out);
    void DestroyViewportTargets();
    uint64_t m_GeometryUploads = 0;
    std::vector<glm::vec3> m_MeshBoundsMin, m_MeshBoundsMax;  // object-space box per cached mesh
    uint32_t m_ShadowMapSize = 2048;
    std::vector<tri_vertex> m_VertexBuffer;
    std::vector<uint32_t> m_IndexBuffer;
    uint64_t m_GeometryGeneration = 1, m_TextureGeneration = 1, m_MaterialGeneration = 1;
    Loader::CubemapTextureData m_SkyboxCubemap;
    std::string m_AssetsDirectory = "Assets";
    std::string m_SkyboxSource;
    uint64_t m_SkyboxGeneration = 1;
    std::vector<uint8_t> m_AiFrame;  // the AI frame's R8G8B8A8_UNORM bytes (SubmitAiInterpolation)
    uint32_t m_AiWidth = 0, m_AiHeight = 0;
    float m_AiBlendStrength = 0.35f;
    uint64_t m_AiGeneration = 1;

    struct TextureSlot {
        std::string m_SourcePath;
        Loader::TextureData m_Data;
    };
    std::vector<TextureSlot> m_TextureSlots;
    std::unordered_map<std::string, uint32_t> m_TextureSlotLookup;

    ECS::Entity m_SelectedEntity = kNoEntity;
    std::map<uint32_t, bool> m_IdOutputViewports;  // SetEntityIdOutputEnabled, by viewport id
    bool m_SelectionOutline = false;
    glm::vec4 m_OutlineColour{1.0f, 0.6f, 0.0f, 1.0f};
    uint32_t m_OutlineWidth = 2;
    struct MotionHistory {  // a viewport's last rendered frame
        bool m_Valid = false;
        uint32_t m_Width = 0, m_Height = 0;
        float m_View[16] = {}, m_Projection[16] = {};
        std::unordered_map<ECS::Entity, std::array<float, 16>> m_Models;
    };
    std::map<uint32_t, bool> m_MotionViewports;  // SetMotionVectorOutputEnabled, by viewport id
    std::map<uint32_t, MotionHistory> m_MotionHistory;
    struct TemporalRecord {  // what a viewport's history reprojection, anti-aliasing and upscaling records share
        bool m_Enabled = false;
        const ViewportContext* m_LastTarget = nullptr;  // the target whose frame the last pass read
        uint32_t m_FrameIndex = 0;  // the jittered passes: the viewport's frames since the switch went on or the extent changed
    };
    struct Reprojection : TemporalRecord {  // SetHistoryReprojectionEnabled, by viewport id
        float m_DepthTolerance = 0.0f;
        tri_history* m_Object = nullptr;  // made at the viewport's first reprojected frame, again after a resize
        uint32_t m_Width = 0, m_Height = 0;
        tri_image m_Colour{}, m_Mask{};
    };
    std::map<uint32_t, Reprojection> m_Reprojection;
    struct Taa : TemporalRecord {  // SetTemporalAntiAliasingEnabled, by viewport id
        float m_Alpha = 0.1f;
        uint32_t m_Period = 8;
        bool m_RejectIds = true;
        tri_taa* m_Object = nullptr;  // made at the viewport's first resolved frame, again after a resize
        uint32_t m_ObjectWidth = 0, m_ObjectHeight = 0;
        uint32_t m_Width = 0, m_Height = 0;  // the extent m_FrameIndex counts frames of
        tri_image m_Resolved{};
    };
    std::map<uint32_t, Taa> m_Taa;
    struct Upscale : TemporalRecord {  // SetTemporalUpscalingEnabled, by viewport id
        float m_Scale = 0.5f, m_Alpha = 0.1f;
        bool m_RejectIds = true;
        tri_upscale* m_Object = nullptr;  // made at the viewport's first upscaled frame, again after a resize or a scale change
        uint32_t m_RenderWidth = 0, m_RenderHeight = 0, m_OutWidth = 0, m_OutHeight = 0;  // the object's extents
        uint32_t m_Width = 0, m_Height = 0;  // the render extent m_FrameIndex counts frames of (a scale change changes it)
        float m_Jitter[2] = {0.0f, 0.0f};    // of the frame being rendered (BeginUpscaleFrame)
        tri_image m_Resolved{};
    };
    std::map<uint32_t, Upscale> m_Upscale;
    std::map<uint32_t, ViewportContext> m_Viewports;
    ViewportInfo m_LastViewport{};
    uint32_t m_ActiveViewportId = 0;
    uint32_t m_PresentWidth = 0, m_PresentHeight = 0;
    tri_ctx* m_PresentSource = nullptr;    // viewport context the last present was blitted from
    tri_group* m_PresentGroup = nullptr;   // ... or multi-device viewport
    ViewportContext m_LegacyTarget;        // the legacy path's present-extent target (no active viewport)
    bool m_PresentLegacy = false;          // the last present was rendered directly (legacy path), not blitted
    // the extent the last present was produced at (SetPresentExtent may change before ReadPresentPixels)
    uint32_t m_PresentedWidth = 0, m_PresentedHeight = 0;
    uint32_t m_RasterFlags = 0;
    struct PendingFrame {  // what a DrawFrame submitted and no fence has waited for yet
        std::vector<ViewportContext*> m_Targets;
        ViewportContext* m_Legacy = nullptr;  // the legacy present target among them
        ViewportContext* m_Blit = nullptr;    // the primary viewport target whose present blit was enqueued
        uint32_t m_BlitWidth = 0, m_BlitHeight = 0;
        ViewportContext* m_Recorded = nullptr;  // the recorded viewport's target, captured into m_RecordSlot
        uint32_t m_RecordSlot = 0;
        ViewportContext* m_Grabbed = nullptr;  // the active viewport's target, captured into the grab's m_RecordSlot
        uint64_t m_GrabGeneration = 0;         // ... of this grab (a rebuilt grab holds nothing of this frame)
    };
    std::deque<PendingFrame> m_Pending;  // oldest first; at most m_FramesInFlight
    void FinishOldestFrame();
    // frames in flight: viewport id -> its targets 1 .. n-1 (target 0 is the m_Viewports entry), and the target of its
    // latest frame
    uint32_t m_FramesInFlight = 1;
    uint64_t m_FrameCount = 0;
    std::map<uint32_t, std::vector<ViewportContext>> m_RingTargets;
    std::map<uint32_t, uint32_t> m_LatestTarget;
    ViewportContext& TargetOf(uint32_t viewportId, ViewportContext& primary, uint32_t index);
    const ViewportContext* LatestTarget(uint32_t viewportId) const;

    // viewport recording: the session, the recorded viewport and its pinned extent, and the device-side recorder
    // (one slot per frame in flight; created by the first recorded DrawFrame, dropped with the viewport targets)
    bool m_Recording = false;
    uint32_t m_RecordingViewportId = 0;
    uint32_t m_RecordingWidth = 0, m_RecordingHeight = 0;
    std::string m_RecordingPath;
    VideoEncoder m_VideoEncoder;
    tri_recorder* m_Recorder = nullptr;
    bool m_RecordingJpeg = false;  // the session is an .mkv: the recorder makes JPEGs
    uint32_t m_RecordingQuality = 90;

    // text overlay: the font and the frame's queue, and one device atlas per device (made by the first DrawFrame
    // with text, dropped with the viewport targets and when the font changes)
    TextRenderer m_TextRenderer;
    bool m_TextFontTried = false;  // the default font was looked for (and logged if missing)
    std::map<int32_t, tri_font*> m_Fonts;
    uint64_t m_FontsVersion = 0;  // TextRenderer::GetFontVersion the atlases were made from
    std::vector<tri_text_quad> m_TextQuads;
    void DropFonts();
    bool SetTargetText(ViewportContext& target, uint32_t viewportId);  // before the target's tri_render
    bool CaptureRecordedFrame(ViewportContext& target, uint32_t slot);
    void StopRecording();  // finish the frames in flight, finalise the file

    // AI readback: the device-side grab (made by the first captured DrawFrame, dropped with the viewport targets and
    // when the active viewport's extent changes), the throttles and the pending tensor
    bool m_AiReadback = false;
    tri_framegrab* m_Grab = nullptr;
    uint32_t m_GrabWidth = 0, m_GrabHeight = 0;
    uint64_t m_GrabGeneration = 0;
    int32_t m_GrabHeldSlot = -1;  // the slot whose device tensor GetFrameReadbackDeviceTensor hands out
    const float* m_GrabDeviceTensor = nullptr;
    const float* m_GrabHostTensor = nullptr;  // the held slot's pinned buffer
    bool m_PendingInSlot = false;             // the pending readback is m_GrabHostTensor (else m_PendingFrameReadback)
    size_t FrameReadbackCount() const { return (size_t)m_FrameReadbackWidth * m_FrameReadbackHeight * s_FrameReadbackChannelCount; }
    void ReleaseHeldReadbackSlot(bool keepPending);
    bool AiInferenceThrottleElapsed();
    std::chrono::milliseconds m_AiReadbackInterval{66}, m_AiInferenceInterval{66};
    std::chrono::steady_clock::time_point m_NextAiReadbackTime{}, m_NextAiInferenceTime{};
    std::vector<float> m_PendingFrameReadback;
    uint32_t m_FrameReadbackWidth = 0, m_FrameReadbackHeight = 0;
    static constexpr uint32_t s_FrameReadbackChannelCount = 4;
    bool CaptureReadbackFrame(ViewportContext& target, uint32_t slot);
    void ResolveReadbackFrame(ViewportContext& target, uint32_t slot, bool ok, bool rerendered);
    void DropGrab();
    // the generator on the device
    AI::FrameGenerator m_FrameGenerator;
    AiDebugStats m_AiDebugStats{};
    bool m_AiFromDevice = false;  // the blend frame is the generator's output tensor (packed per target), not m_AiFrame
    tri_ctx* m_GrabHeldCtx = nullptr;  // the context whose stream made the held tensor
    int32_t m_GrabDevice = -1;         // the grab's device
    static constexpr std::chrono::milliseconds s_AiModelSearchInterval{1000};
    std::chrono::steady_clock::time_point m_AiNextModelSearchTime{};
    bool m_AiModelMissingWarningIssued = false, m_AiModelInitialiseWarningIssued = false, m_AiShapeWarningIssued = false;
    void ProcessAiFrame();
    void RefreshAiDebugStats();
    void ConsumeAiOutput();  // after TryConsumeOutput: pack into every target, record the sample's output
    bool UploadAiFrameFromDevice(ViewportContext& target);
    tri_global_ubo TargetUniforms(const ViewportContext& target, const tri_global_ubo& ubo) const;
    template <typename F> void ForEachTarget(F&& f);
    // dataset capture
    FrameDatasetRecorder m_FrameDatasetRecorder;
    bool m_FrameDatasetCaptureEnabled = false;
    std::string m_FrameDatasetCaptureDirectory;
    uint32_t m_FrameDatasetCaptureInterval = 1;
    void SyncFrameDatasetRecorder();

    glm::vec3 m_AmbientColor{0.03f};
    float m_AmbientIntensity = 1.0f;
    glm::vec4 m_ClearColor{0.005f, 0.005f, 0.005f, 1.0f};
    size_t m_ModelCount = 0;
    size_t m_TriangleCount = 0;

    static constexpr size_t s_PerformanceHistorySize = 240;
    std::vector<FrameTimingSample> m_PerformanceHistory;
    size_t m_PerformanceHistoryNextIndex = 0;
    size_t m_PerformanceSampleCount = 0;
    FrameTimingStats m_PerformanceStats{};
    bool m_Initialised = false;
    bool m_Shutdown = false;
};

}  // namespace Trident
