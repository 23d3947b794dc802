// RenderCommand.h — the static facade Trident-Forge drives the renderer through
// (Trident/src/Renderer/RenderCommand.h:11-84), restricted to the draw path. Each call forwards to
// the process-wide renderer (Startup::GetRenderer(), Application/Startup.h:38) — here
// RenderCommand::GetRenderer(). Text / gizmo entry points are outside the path.
#pragma once

#include <string>
#include <vector>

#include "Renderer.h"

namespace Trident {

class RenderCommand {
public:
    static Renderer& GetRenderer();  // stands in for Startup::GetRenderer()

    static void Init() { GetRenderer().Init(); }
    static void Shutdown() { GetRenderer().Shutdown(); }
    static void DrawFrame() { GetRenderer().DrawFrame(); }
    static void SetViewport(uint32_t viewportId, const ViewportInfo& info) { GetRenderer().SetViewport(viewportId, info); }
    static void SetClearColor(const glm::vec4& color) { GetRenderer().SetClearColor(color); }
    static void AppendMeshes(std::vector<Geometry::Mesh> meshes, std::vector<Geometry::Material> materials,
                             std::vector<std::string> textures) {
        GetRenderer().AppendMeshes(std::move(meshes), std::move(materials), std::move(textures));
    }
    static void UploadMesh(const std::vector<Geometry::Mesh>& meshes, const std::vector<Geometry::Material>& materials,
                           const std::vector<std::string>& textures) {
        GetRenderer().UploadMesh(meshes, materials, textures);
    }
    static void SetEditorCamera(Camera* camera) { GetRenderer().SetEditorCamera(camera); }
    static void SetRuntimeCamera(Camera* camera) { GetRenderer().SetRuntimeCamera(camera); }
    static void SetRuntimeCameraReady(bool ready) { GetRenderer().SetRuntimeCameraReady(ready); }
    static void SetActiveRegistry(ECS::Registry* registry) { GetRenderer().SetActiveRegistry(registry); }
    static bool HasRuntimeCamera() { return GetRenderer().HasRuntimeCamera(); }
    static ViewportInfo GetViewport() { return GetRenderer().GetViewport(); }
    static void* GetViewportTexture(uint32_t viewportId) { return GetRenderer().GetViewportTexture(viewportId); }
    static glm::mat4 GetViewportViewMatrix(uint32_t id) { return GetRenderer().GetViewportViewMatrix(id); }
    static glm::mat4 GetViewportProjectionMatrix(uint32_t id) { return GetRenderer().GetViewportProjectionMatrix(id); }
    static glm::vec4 GetClearColor() { return GetRenderer().GetClearColor(); }
    // Text overlay (RenderCommand::SubmitText)
    static void SubmitText(uint32_t viewportId, const glm::vec2& position, const glm::vec4& color, const std::string& text) {
        GetRenderer().SubmitText(viewportId, position, color, text);
    }
    // Entity ids: picking, rectangle selection, the per-pixel entity image and the selection outline
    static void SetSelectedEntity(ECS::Entity entity) { GetRenderer().SetSelectedEntity(entity); }
    static void SetEntityIdOutputEnabled(uint32_t viewportId, bool enabled) { GetRenderer().SetEntityIdOutputEnabled(viewportId, enabled); }
    static bool PickEntity(uint32_t viewportId, int32_t x, int32_t y, ECS::Entity& out, float* depth01 = nullptr) {
        return GetRenderer().PickEntity(viewportId, x, y, out, depth01);
    }
    static std::vector<ECS::Entity> PickEntitiesInRect(uint32_t viewportId, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
        return GetRenderer().PickEntitiesInRect(viewportId, x0, y0, x1, y1);
    }
    static bool ReadViewportEntityIds(uint32_t viewportId, std::vector<uint32_t>& out, uint32_t background = 0xFFFFFFFFu) {
        return GetRenderer().ReadViewportEntityIds(viewportId, out, background);
    }
    static void SetSelectionOutline(bool enabled, const glm::vec4& colour = glm::vec4(1.0f, 0.6f, 0.0f, 1.0f), uint32_t widthPx = 2) {
        GetRenderer().SetSelectionOutline(enabled, colour, widthPx);
    }
    // Motion vectors: the per-pixel screen-space motion image of a viewport
    static void SetMotionVectorOutputEnabled(uint32_t viewportId, bool enabled) { GetRenderer().SetMotionVectorOutputEnabled(viewportId, enabled); }
    static bool ReadViewportMotionVectors(uint32_t viewportId, std::vector<float>& out) { return GetRenderer().ReadViewportMotionVectors(viewportId, out); }
    static void* GetViewportMotionTexture(uint32_t viewportId) { return GetRenderer().GetViewportMotionTexture(viewportId); }
    // History reprojection: the viewport's previous frame warped by motion, and its disocclusion mask
    static void SetHistoryReprojectionEnabled(uint32_t viewportId, bool enabled, float depthTolerance = 0.0f) {
        GetRenderer().SetHistoryReprojectionEnabled(viewportId, enabled, depthTolerance);
    }
    static bool ReadViewportReprojection(uint32_t viewportId, std::vector<uint8_t>& bgra, std::vector<uint8_t>& mask) {
        return GetRenderer().ReadViewportReprojection(viewportId, bgra, mask);
    }
    static void* GetViewportReprojectedTexture(uint32_t viewportId) { return GetRenderer().GetViewportReprojectedTexture(viewportId); }
    static void* GetViewportDisocclusionTexture(uint32_t viewportId) { return GetRenderer().GetViewportDisocclusionTexture(viewportId); }
    // Temporal anti-aliasing: jittered frames resolved over the viewport's clamped, accumulated history
    static void SetTemporalAntiAliasingEnabled(uint32_t viewportId, bool enabled, float alpha = 0.1f, uint32_t period = 8,
                                               bool rejectIds = true) {
        GetRenderer().SetTemporalAntiAliasingEnabled(viewportId, enabled, alpha, period, rejectIds);
    }
    static bool IsTemporalAntiAliasingEnabled(uint32_t viewportId) { return GetRenderer().IsTemporalAntiAliasingEnabled(viewportId); }
    static bool ReadViewportResolvedPixels(uint32_t viewportId, std::vector<uint8_t>& rgba) {
        return GetRenderer().ReadViewportResolvedPixels(viewportId, rgba);
    }
    static bool ReadViewportTaaMask(uint32_t viewportId, std::vector<uint8_t>& mask) { return GetRenderer().ReadViewportTaaMask(viewportId, mask); }
    static void* GetViewportResolvedTexture(uint32_t viewportId) { return GetRenderer().GetViewportResolvedTexture(viewportId); }
    static bool SetTemporalUpscalingEnabled(uint32_t viewportId, bool enabled, float renderScale = 0.5f, float alpha = 0.1f,
                                            bool rejectIds = true) {
        return GetRenderer().SetTemporalUpscalingEnabled(viewportId, enabled, renderScale, alpha, rejectIds);
    }
    static bool IsTemporalUpscalingEnabled(uint32_t viewportId) { return GetRenderer().IsTemporalUpscalingEnabled(viewportId); }
    static bool ReadViewportUpscaledPixels(uint32_t viewportId, std::vector<uint8_t>& rgba, uint32_t* width = nullptr,
                                           uint32_t* height = nullptr) {
        return GetRenderer().ReadViewportUpscaledPixels(viewportId, rgba, width, height);
    }
    static bool ReadViewportUpscaleMask(uint32_t viewportId, std::vector<uint8_t>& mask) {
        return GetRenderer().ReadViewportUpscaleMask(viewportId, mask);
    }
    static void* GetViewportUpscaledTexture(uint32_t viewportId) { return GetRenderer().GetViewportUpscaledTexture(viewportId); }
    static FrameTimingStats GetFrameTimingStats() { return GetRenderer().GetFrameTimingStats(); }
    static size_t GetModelCount() { return GetRenderer().GetModelCount(); }
    static int32_t ResolveTextureSlot(const std::string& texturePath) { return GetRenderer().ResolveTextureSlot(texturePath); }
    // Viewport recording (RenderCommand.h: SetViewportRecordingEnabled / IsViewportRecording)
    static bool SetViewportRecordingEnabled(bool enabled, uint32_t viewportId, uint32_t width, uint32_t height,
                                            const std::string& outputPath) {
        return GetRenderer().SetViewportRecordingEnabled(enabled, viewportId, width, height, outputPath);
    }
    static bool IsViewportRecording() { return GetRenderer().IsViewportRecording(); }
    static void SetRecordingQuality(int quality) { GetRenderer().SetRecordingQuality(quality); }
    static int GetRecordingQuality() { return GetRenderer().GetRecordingQuality(); }
    static void GetRecordingExtent(uint32_t& width, uint32_t& height) { GetRenderer().GetRecordingExtent(width, height); }
    static uint64_t GetRecordedFrameCount() { return GetRenderer().GetRecordedFrameCount(); }
    // Dataset capture (RenderCommand.h:69-77)
    static void SetFrameDatasetCaptureEnabled(bool enabled) { GetRenderer().SetFrameDatasetCaptureEnabled(enabled); }
    static bool IsFrameDatasetCaptureEnabled() { return GetRenderer().IsFrameDatasetCaptureEnabled(); }
    static void SetFrameDatasetCaptureDirectory(const std::string& directory) {
        GetRenderer().SetFrameDatasetCaptureDirectory(directory);
    }
    static std::string GetFrameDatasetCaptureDirectory() { return GetRenderer().GetFrameDatasetCaptureDirectory(); }
    static void SetFrameDatasetCaptureInterval(uint32_t interval) { GetRenderer().SetFrameDatasetCaptureInterval(interval); }
    static uint32_t GetFrameDatasetCaptureInterval() { return GetRenderer().GetFrameDatasetCaptureInterval(); }
    // The AI loop's ends, for a frame generator outside the library
    static bool SetAiReadbackEnabled(bool enabled) { return GetRenderer().SetAiReadbackEnabled(enabled); }
    static bool IsAiReadbackEnabled() { return GetRenderer().IsAiReadbackEnabled(); }
    static void SetAiThrottleIntervals(uint32_t readbackMs, uint32_t inferenceMs) {
        GetRenderer().SetAiThrottleIntervals(readbackMs, inferenceMs);
    }
    static bool TryAcquireRenderedFrame(std::vector<float>& out) { return GetRenderer().TryAcquireRenderedFrame(out); }
    static bool SubmitAiOutput(const float* data, size_t count, const int64_t* shape, size_t rank) {
        return GetRenderer().SubmitAiOutput(data, count, shape, rank);
    }
    // The frame generator on the device (Renderer::LoadAiModel, GetAiDebugStats, RenderCommand.h's AI debug panel)
    static bool LoadAiModel(const std::string& path) { return GetRenderer().LoadAiModel(path); }
    static Renderer::AiDebugStats GetAiDebugStats() { return GetRenderer().GetAiDebugStats(); }
    static bool FinishAiInference(uint32_t timeoutMs = 5000) { return GetRenderer().FinishAiInference(timeoutMs); }
    // Poses evaluated on the device (opt-in; Renderer::SetDevicePoseEnabled)
    static void SetDevicePoseEnabled(bool enabled) { GetRenderer().SetDevicePoseEnabled(enabled); }
    static bool IsDevicePoseEnabled() { return GetRenderer().IsDevicePoseEnabled(); }
    static size_t GetOrCreatePrimitiveMeshIndex(MeshComponent::PrimitiveType primitiveType) {
        return GetRenderer().GetOrCreatePrimitiveMeshIndex(primitiveType);
    }
};

}  // namespace Trident
