// AnimationStateMachine.h — Trident's animation state machine (Animation/AnimationStateMachine.h) restated: parameters,
// conditions, transitions, states, layers and the machine, with the reference's names and sequencing
// (AnimationStateMachine.cpp:242-504). One update is two steps: Advance moves all host state (times, transitions,
// triggers) and emits the update's pose program; Update then evaluates that program with the float32 interpreter of
// Animation.h. The device path hands the same program to tri_pose_graph, so what an update means is stated once.
#pragma once

#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "AnimationBlendTree.h"

namespace Trident {
namespace Animation {

enum class AnimationParameterType { Float, Bool, Integer, Trigger };

struct AnimationParameter {
    AnimationParameterType m_Type = AnimationParameterType::Float;
    float m_FloatValue = 0.0f;
    bool m_BoolValue = false;
    int m_IntValue = 0;
    bool m_TriggerValue = false;

    float AsFloat(float defaultValue) const;  // Integer: cast; Bool / Trigger: 1 or 0
    bool AsBool(bool defaultValue) const;     // Float: > 0; Integer: != 0
    int AsInt(int defaultValue) const;        // Float: truncated
    bool ConsumeTrigger();                    // whether it was set; cleared. false for another type
    void ResetTrigger();
};

enum class AnimationConditionComparison { Equals, NotEquals, GreaterThan, LessThan, GreaterOrEqual, LessOrEqual, Triggered };

struct AnimationTransitionCondition {
    std::string m_ParameterName;
    AnimationConditionComparison m_Comparison = AnimationConditionComparison::Equals;
    float m_FloatValue = 0.0f;
    int m_IntValue = 0;
    bool m_BoolValue = false;
};

struct AnimationTransition {
    std::string m_TargetState;
    bool m_HasExitTime = false;
    float m_ExitTimeSeconds = 0.0f;
    float m_FadeDurationSeconds = 0.2f;
    std::vector<AnimationTransitionCondition> m_Conditions{};
};

struct AnimationState {
    explicit AnimationState(std::string name, std::unique_ptr<AnimationBlendNode> rootNode)
        : m_Name(std::move(name)), m_RootNode(std::move(rootNode)) {}

    std::string m_Name;
    std::unique_ptr<AnimationBlendNode> m_RootNode;
    std::vector<AnimationTransition> m_Transitions{};
};

struct AnimationLayer {
    AnimationLayer() = default;
    AnimationLayer(const AnimationLayer&) = delete;
    AnimationLayer& operator=(const AnimationLayer&) = delete;
    AnimationLayer(AnimationLayer&&) noexcept = default;
    AnimationLayer& operator=(AnimationLayer&&) noexcept = default;

    std::string m_Name;
    float m_Weight = 1.0f;
    bool m_IsAdditive = false;
    AnimationMask m_Mask{};
    std::unordered_map<std::string, std::unique_ptr<AnimationState>> m_States{};
    std::string m_EntryState;
    AnimationState* m_CurrentState = nullptr;
    AnimationState* m_NextState = nullptr;
    float m_TimeInState = 0.0f;
    float m_TransitionElapsed = 0.0f;
    float m_TransitionDuration = 0.0f;
};

class AnimationStateMachine {
public:
    explicit AnimationStateMachine(AnimationAssetService& assetService) : m_AssetService(&assetService) {}

    void SetSkeletonHandle(size_t skeletonHandle);
    void SetAnimationLibraryHandle(size_t animationLibraryHandle) { m_AnimationLibraryHandle = animationLibraryHandle; }
    size_t GetSkeletonHandle() const { return m_SkeletonHandle; }
    size_t GetAnimationLibraryHandle() const { return m_AnimationLibraryHandle; }

    void AddFloatParameter(const std::string& name, float defaultValue);
    void AddBoolParameter(const std::string& name, bool defaultValue);
    void AddIntegerParameter(const std::string& name, int defaultValue);
    void AddTriggerParameter(const std::string& name);

    void SetFloatParameter(const std::string& name, float value) { AddFloatParameter(name, value); }
    void SetBoolParameter(const std::string& name, bool value) { AddBoolParameter(name, value); }
    void SetIntegerParameter(const std::string& name, int value) { AddIntegerParameter(name, value); }
    void FireTrigger(const std::string& name);
    void ResetTrigger(const std::string& name);
    const AnimationParameter* FindParameter(const std::string& name) const;

    size_t AddLayer(const std::string& name, float weight, bool isAdditive);
    void SetLayerMask(size_t layerIndex, AnimationMask mask);
    void SetLayerWeight(size_t layerIndex, float weight);
    void SetLayerEntryState(size_t layerIndex, const std::string& stateName);
    size_t GetLayerCount() const { return m_Layers.size(); }
    const AnimationLayer* GetLayer(size_t layerIndex) const { return layerIndex < m_Layers.size() ? &m_Layers[layerIndex] : nullptr; }

    // std::out_of_range for a layer that does not exist; AddTransition from an unknown state is std::runtime_error.
    AnimationState& AddState(size_t layerIndex, const std::string& stateName, std::unique_ptr<AnimationBlendNode> rootNode);
    AnimationTransition& AddTransition(size_t layerIndex, const std::string& fromState, const AnimationTransition& transition);

    // Advance + Evaluate. Without a skeleton behind the handle nothing changes.
    void Update(float deltaSeconds);
    // The CPU half of Update: the program of the last Advance through the float32 interpreter, into CopyPose's matrices.
    void Evaluate();
    // The host half of Update: false (no change) without a skeleton; otherwise every layer advanced in order and the
    // update's program in GetProgram(). The program starts with REST (the final pose) and appends per layer its pose
    // and its BLEND / ADD with the layer's weight and mask (a mask whose weights are all 1.0 is emitted as no mask:
    // the arithmetic is the same); a layer whose pose is empty contributes nothing.
    bool Advance(float deltaSeconds);
    const PoseProgram& GetProgram() const { return m_Program; }
    void CopyPose(std::vector<glm::mat4>& outMatrices) const { outMatrices = m_SkinningMatrices; }

private:
    AnimationState* FindState(AnimationLayer& layer, const std::string& stateName) const;
    void EnsureRestPose();
    void UpdateLayer(AnimationLayer& layer, float deltaSeconds, const Skeleton& skeleton);
    bool EvaluateTransitionConditions(const AnimationTransition& transition);

    AnimationAssetService* m_AssetService = nullptr;
    size_t m_SkeletonHandle = AnimationAssetService::s_InvalidHandle;
    size_t m_AnimationLibraryHandle = AnimationAssetService::s_InvalidHandle;

    std::unordered_map<std::string, AnimationParameter> m_Parameters{};
    std::vector<AnimationLayer> m_Layers{};

    size_t m_RestBones = 0;  // the bone count the rest matrices were built for
    PoseProgram m_Program{};
    std::vector<glm::mat4> m_SkinningMatrices{};
};

}  // namespace Animation
}  // namespace Trident
