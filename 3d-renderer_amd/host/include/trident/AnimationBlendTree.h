// AnimationBlendTree.h — Trident's blend-tree nodes (Animation/AnimationBlendTree.h) restated. The class and method
// names are the reference's. A node here does not blend poses itself: its Advance moves its own time forward and
// appends what its pose is to a pose program (Animation.h, include/tri_raster.h "A pose program"), which the CPU
// interpreter and the device kernel both evaluate. Evaluate, the reference's entry point, is Advance followed by the
// CPU interpreter.
#pragma once

#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "Animation.h"

namespace Trident {
namespace Animation {

struct AnimationParameter;
struct AnimationGraphContext {
    AnimationAssetService& m_AssetService;
    size_t m_SkeletonHandle = AnimationAssetService::s_InvalidHandle;
    size_t m_AnimationHandle = AnimationAssetService::s_InvalidHandle;
    const std::unordered_map<std::string, AnimationParameter>* m_Parameters = nullptr;
};

class AnimationBlendNode {
public:
    virtual ~AnimationBlendNode() = default;

    virtual void Reset() {}
    // Advance by deltaSeconds and append the node's pose to the program: true when exactly one pose was pushed, false
    // when the node's pose is the empty pose (nothing appended). An empty pose makes every blend with it a no-op
    // (BlendPose runs over min(sizes) bones), which the callers fold away.
    virtual bool Advance(const AnimationGraphContext& context, float deltaSeconds, PoseProgram& program) = 0;
    AnimationPose Evaluate(const AnimationGraphContext& context, float deltaSeconds);
};

class ClipNode : public AnimationBlendNode {
public:
    ClipNode(size_t clipIndex, bool isLooping, float playbackSpeed)
        : m_ClipIndex(clipIndex), m_IsLooping(isLooping), m_PlaybackSpeed(playbackSpeed) {}

    void SetSpeedParameter(const std::string& parameterName) { m_SpeedParameter = parameterName; }
    float GetCurrentTime() const { return m_CurrentTime; }

    void Reset() override { m_CurrentTime = 0.0f; }
    // time += delta * speed, then fmod-wrapped into [0, duration) (looping) or clamped to [0, duration]; a clip whose
    // duration is <= 0 does neither. A missing clip gives the rest pose and no time advance; a missing skeleton the
    // empty pose.
    bool Advance(const AnimationGraphContext& context, float deltaSeconds, PoseProgram& program) override;

private:
    float ResolveSpeed(const AnimationGraphContext& context) const;

    size_t m_ClipIndex = AnimationAssetService::s_InvalidHandle;
    bool m_IsLooping = true;
    float m_PlaybackSpeed = 1.0f;
    float m_CurrentTime = 0.0f;
    std::string m_SpeedParameter{};
};

class BlendNode : public AnimationBlendNode {
public:
    BlendNode(std::unique_ptr<AnimationBlendNode> first, std::unique_ptr<AnimationBlendNode> second, float weight)
        : m_First(std::move(first)), m_Second(std::move(second)), m_Weight(weight) {}

    void SetWeightParameter(const std::string& parameterName) { m_WeightParameter = parameterName; }

    void Reset() override;
    // Both children advance on every update. Without a first child the result is the empty pose; without a second it
    // is the first child's pose.
    bool Advance(const AnimationGraphContext& context, float deltaSeconds, PoseProgram& program) override;

private:
    float ResolveWeight(const AnimationGraphContext& context) const;

    std::unique_ptr<AnimationBlendNode> m_First;
    std::unique_ptr<AnimationBlendNode> m_Second;
    float m_Weight = 0.5f;
    std::string m_WeightParameter{};
};

class BlendSpace1DNode : public AnimationBlendNode {
public:
    struct Sample {
        size_t m_ClipIndex = AnimationAssetService::s_InvalidHandle;
        float m_Position = 0.0f;
    };

    // The samples are sorted by position with a stable sort: samples at equal positions keep the order they were given
    // in (the reference's std::sort leaves it unspecified).
    BlendSpace1DNode(std::vector<Sample> samples, float parameterDefault);

    void SetParameterName(const std::string& parameterName) { m_ParameterName = parameterName; }
    float GetCurrentTime() const { return m_CurrentTime; }

    void Reset() override { m_CurrentTime = 0.0f; }
    // The time only ever grows by deltaSeconds (never wrapped). The first neighbouring pair whose positions bracket the
    // parameter is blended, otherwise the first and last samples; T = clamp((p - left) / max(right - left, eps), 0, 1).
    bool Advance(const AnimationGraphContext& context, float deltaSeconds, PoseProgram& program) override;

private:
    float ResolveParameter(const AnimationGraphContext& context) const;

    std::vector<Sample> m_Samples{};
    float m_ParameterValue = 0.0f;
    float m_CurrentTime = 0.0f;
    std::string m_ParameterName{};
};

}  // namespace Animation
}  // namespace Trident
