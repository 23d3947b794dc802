// AnimationStateMachine.cpp — the blend-tree nodes and the state machine (see AnimationBlendTree.h and
// AnimationStateMachine.h). Everything here is host state and sequencing; the pose arithmetic is the program
// interpreter's (Animation.cpp) or the device's (csrc/pose_eval.hip).
#include "trident/AnimationStateMachine.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <stdexcept>

namespace Trident {
namespace Animation {

namespace {

const AnimationParameter* Lookup(const AnimationGraphContext& context, const std::string& name) {
    if (name.empty() || !context.m_Parameters) return nullptr;
    auto found = context.m_Parameters->find(name);
    return found == context.m_Parameters->end() ? nullptr : &found->second;
}

void Push(PoseProgram& program, uint32_t op, uint32_t a, float f) {
    PoseOp o;
    o.m_Op = op;
    o.m_A = a;
    o.m_F = f;
    program.m_Ops.push_back(o);
}

}  // namespace

AnimationPose AnimationBlendNode::Evaluate(const AnimationGraphContext& context, float deltaSeconds) {
    PoseProgram program;
    AnimationPose pose;
    if (!Advance(context, deltaSeconds, program)) return pose;  // the empty pose
    const Skeleton* skeleton = context.m_AssetService.GetSkeleton(context.m_SkeletonHandle);
    if (skeleton) EvaluatePoseProgram(*skeleton, context.m_AssetService.GetAnimationClips(context.m_AnimationHandle), program, pose);
    return pose;
}

// ---- ClipNode (AnimationBlendTree.cpp:38-88) ----
float ClipNode::ResolveSpeed(const AnimationGraphContext& context) const {
    const AnimationParameter* p = Lookup(context, m_SpeedParameter);
    return p ? p->AsFloat(m_PlaybackSpeed) : m_PlaybackSpeed;
}

bool ClipNode::Advance(const AnimationGraphContext& context, float deltaSeconds, PoseProgram& program) {
    if (!context.m_AssetService.GetSkeleton(context.m_SkeletonHandle)) return false;
    const AnimationClip* clip = context.m_AssetService.GetClip(context.m_AnimationHandle, m_ClipIndex);
    if (!clip) {
        Push(program, PoseOp::Rest, 0, 0.0f);
        return true;
    }
    m_CurrentTime += deltaSeconds * ResolveSpeed(context);
    const float duration = clip->m_DurationSeconds;
    if (duration > 0.0f) {
        if (m_IsLooping) {
            const float mod = std::fmod(m_CurrentTime, duration);
            m_CurrentTime = mod < 0.0f ? duration + mod : mod;
        } else {
            m_CurrentTime = m_CurrentTime < 0.0f ? 0.0f : (duration < m_CurrentTime ? duration : m_CurrentTime);
        }
    }
    Push(program, PoseOp::Clip, (uint32_t)m_ClipIndex, m_CurrentTime);
    return true;
}

// ---- BlendNode (:113-145) ----
void BlendNode::Reset() {
    if (m_First) m_First->Reset();
    if (m_Second) m_Second->Reset();
}

float BlendNode::ResolveWeight(const AnimationGraphContext& context) const {
    const AnimationParameter* p = Lookup(context, m_WeightParameter);
    return glm::clamp(p ? p->AsFloat(m_Weight) : m_Weight, 0.0f, 1.0f);
}

bool BlendNode::Advance(const AnimationGraphContext& context, float deltaSeconds, PoseProgram& program) {
    const bool base = m_First && m_First->Advance(context, deltaSeconds, program);
    if (m_Second) {
        const size_t mark = program.m_Ops.size();
        const bool target = m_Second->Advance(context, deltaSeconds, program);  // advances whatever becomes of its pose
        if (base && target) Push(program, PoseOp::Blend, PoseOp::s_NoMask, ResolveWeight(context));
        else program.m_Ops.resize(mark);  // a blend with an empty pose on either side changes nothing
    }
    return base;
}

// ---- BlendSpace1DNode (:147-229) ----
BlendSpace1DNode::BlendSpace1DNode(std::vector<Sample> samples, float parameterDefault)
    : m_Samples(std::move(samples)), m_ParameterValue(parameterDefault) {
    std::stable_sort(m_Samples.begin(), m_Samples.end(), [](const Sample& a, const Sample& b) { return a.m_Position < b.m_Position; });
}

float BlendSpace1DNode::ResolveParameter(const AnimationGraphContext& context) const {
    const AnimationParameter* p = Lookup(context, m_ParameterName);
    return p ? p->AsFloat(m_ParameterValue) : m_ParameterValue;
}

bool BlendSpace1DNode::Advance(const AnimationGraphContext& context, float deltaSeconds, PoseProgram& program) {
    if (!context.m_AssetService.GetSkeleton(context.m_SkeletonHandle) || m_Samples.empty()) return false;
    m_CurrentTime += deltaSeconds;  // never wrapped
    const float parameter = ResolveParameter(context);
    const Sample* left = &m_Samples.front();
    const Sample* right = &m_Samples.back();
    for (size_t i = 0; i + 1 < m_Samples.size(); ++i)
        if (parameter >= m_Samples[i].m_Position && parameter <= m_Samples[i + 1].m_Position) {
            left = &m_Samples[i];
            right = &m_Samples[i + 1];
            break;
        }
    if (!context.m_AssetService.GetClip(context.m_AnimationHandle, left->m_ClipIndex) ||
        !context.m_AssetService.GetClip(context.m_AnimationHandle, right->m_ClipIndex)) {
        Push(program, PoseOp::Rest, 0, 0.0f);
        return true;
    }
    const float delta = right->m_Position - left->m_Position;
    const float denominator = delta < FLT_EPSILON ? FLT_EPSILON : delta;  // std::max(delta, eps)
    const float T = glm::clamp((parameter - left->m_Position) / denominator, 0.0f, 1.0f);
    Push(program, PoseOp::Clip, (uint32_t)left->m_ClipIndex, m_CurrentTime);
    Push(program, PoseOp::Clip, (uint32_t)right->m_ClipIndex, m_CurrentTime);
    Push(program, PoseOp::Blend, PoseOp::s_NoMask, T);
    return true;
}

// ---- AnimationParameter (AnimationStateMachine.cpp:23-93) ----
float AnimationParameter::AsFloat(float defaultValue) const {
    switch (m_Type) {
        case AnimationParameterType::Float: return m_FloatValue;
        case AnimationParameterType::Integer: return static_cast<float>(m_IntValue);
        case AnimationParameterType::Bool: return m_BoolValue ? 1.0f : 0.0f;
        case AnimationParameterType::Trigger: return m_TriggerValue ? 1.0f : 0.0f;
    }
    return defaultValue;
}

bool AnimationParameter::AsBool(bool defaultValue) const {
    switch (m_Type) {
        case AnimationParameterType::Bool: return m_BoolValue;
        case AnimationParameterType::Float: return m_FloatValue > 0.0f;
        case AnimationParameterType::Integer: return m_IntValue != 0;
        case AnimationParameterType::Trigger: return m_TriggerValue;
    }
    return defaultValue;
}

int AnimationParameter::AsInt(int defaultValue) const {
    switch (m_Type) {
        case AnimationParameterType::Integer: return m_IntValue;
        case AnimationParameterType::Float: return static_cast<int>(m_FloatValue);
        case AnimationParameterType::Bool: return m_BoolValue ? 1 : 0;
        case AnimationParameterType::Trigger: return m_TriggerValue ? 1 : 0;
    }
    return defaultValue;
}

bool AnimationParameter::ConsumeTrigger() {
    if (m_Type != AnimationParameterType::Trigger) return false;
    const bool was = m_TriggerValue;
    m_TriggerValue = false;
    return was;
}

void AnimationParameter::ResetTrigger() {
    if (m_Type == AnimationParameterType::Trigger) m_TriggerValue = false;
}

// ---- AnimationStateMachine ----
void AnimationStateMachine::SetSkeletonHandle(size_t skeletonHandle) {
    m_SkeletonHandle = skeletonHandle;
    EnsureRestPose();
}

void AnimationStateMachine::AddFloatParameter(const std::string& name, float value) {
    AnimationParameter& p = m_Parameters[name];
    p.m_Type = AnimationParameterType::Float;
    p.m_FloatValue = value;
}

void AnimationStateMachine::AddBoolParameter(const std::string& name, bool value) {
    AnimationParameter& p = m_Parameters[name];
    p.m_Type = AnimationParameterType::Bool;
    p.m_BoolValue = value;
}

void AnimationStateMachine::AddIntegerParameter(const std::string& name, int value) {
    AnimationParameter& p = m_Parameters[name];
    p.m_Type = AnimationParameterType::Integer;
    p.m_IntValue = value;
}

void AnimationStateMachine::AddTriggerParameter(const std::string& name) {
    AnimationParameter& p = m_Parameters[name];
    p.m_Type = AnimationParameterType::Trigger;
    p.m_TriggerValue = false;
}

void AnimationStateMachine::FireTrigger(const std::string& name) {
    AnimationParameter& p = m_Parameters[name];
    p.m_Type = AnimationParameterType::Trigger;
    p.m_TriggerValue = true;
}

void AnimationStateMachine::ResetTrigger(const std::string& name) {
    auto found = m_Parameters.find(name);
    if (found != m_Parameters.end()) found->second.ResetTrigger();
}

const AnimationParameter* AnimationStateMachine::FindParameter(const std::string& name) const {
    auto found = m_Parameters.find(name);
    return found == m_Parameters.end() ? nullptr : &found->second;
}

size_t AnimationStateMachine::AddLayer(const std::string& name, float weight, bool isAdditive) {
    AnimationLayer layer;
    layer.m_Name = name;
    layer.m_Weight = weight;
    layer.m_IsAdditive = isAdditive;
    layer.m_Mask.Resize(m_RestBones);
    m_Layers.push_back(std::move(layer));
    return m_Layers.size() - 1;
}

void AnimationStateMachine::SetLayerMask(size_t layerIndex, AnimationMask mask) {
    if (layerIndex < m_Layers.size()) m_Layers[layerIndex].m_Mask = std::move(mask);
}

void AnimationStateMachine::SetLayerWeight(size_t layerIndex, float weight) {
    if (layerIndex < m_Layers.size()) m_Layers[layerIndex].m_Weight = weight;
}

void AnimationStateMachine::SetLayerEntryState(size_t layerIndex, const std::string& stateName) {
    if (layerIndex < m_Layers.size()) m_Layers[layerIndex].m_EntryState = stateName;
}

AnimationState& AnimationStateMachine::AddState(size_t layerIndex, const std::string& stateName, std::unique_ptr<AnimationBlendNode> rootNode) {
    AnimationLayer& layer = m_Layers.at(layerIndex);
    std::unique_ptr<AnimationState>& slot = layer.m_States[stateName];
    // a state of the same name is replaced: a layer must not keep pointing at the one that goes away
    if (slot && layer.m_CurrentState == slot.get()) layer.m_CurrentState = nullptr;
    if (slot && layer.m_NextState == slot.get()) layer.m_NextState = nullptr;
    slot = std::make_unique<AnimationState>(stateName, std::move(rootNode));
    return *slot;
}

AnimationTransition& AnimationStateMachine::AddTransition(size_t layerIndex, const std::string& fromState, const AnimationTransition& transition) {
    AnimationState* state = FindState(m_Layers.at(layerIndex), fromState);
    if (!state) throw std::runtime_error("AnimationStateMachine::AddTransition - state not found");
    state->m_Transitions.push_back(transition);
    return state->m_Transitions.back();
}

AnimationState* AnimationStateMachine::FindState(AnimationLayer& layer, const std::string& stateName) const {
    auto found = layer.m_States.find(stateName);
    return found == layer.m_States.end() ? nullptr : found->second.get();
}

void AnimationStateMachine::EnsureRestPose() {
    const Skeleton* skeleton = m_AssetService ? m_AssetService->GetSkeleton(m_SkeletonHandle) : nullptr;
    if (!skeleton || m_RestBones == skeleton->m_Bones.size()) return;
    m_RestBones = skeleton->m_Bones.size();
    m_SkinningMatrices = AnimationPoseUtilities::ComposeSkinningMatrices(*skeleton, AnimationPoseUtilities::BuildRestPose(*skeleton));
}

void AnimationStateMachine::Update(float deltaSeconds) {
    if (Advance(deltaSeconds)) Evaluate();
}

void AnimationStateMachine::Evaluate() {
    const Skeleton* skeleton = m_AssetService ? m_AssetService->GetSkeleton(m_SkeletonHandle) : nullptr;
    if (!skeleton) return;
    AnimationPose pose;
    if (EvaluatePoseProgram(*skeleton, m_AssetService->GetAnimationClips(m_AnimationLibraryHandle), m_Program, pose))
        m_SkinningMatrices = AnimationPoseUtilities::ComposeSkinningMatrices(*skeleton, pose);
}

bool AnimationStateMachine::Advance(float deltaSeconds) {
    const Skeleton* skeleton = m_AssetService ? m_AssetService->GetSkeleton(m_SkeletonHandle) : nullptr;
    if (!skeleton) return false;
    EnsureRestPose();
    m_Program.m_Ops.clear();
    m_Program.m_Masks.clear();
    Push(m_Program, PoseOp::Rest, 0, 0.0f);  // the final pose starts at the rest pose

    const AnimationGraphContext context{*m_AssetService, m_SkeletonHandle, m_AnimationLibraryHandle, &m_Parameters};
    for (AnimationLayer& layer : m_Layers) {
        UpdateLayer(layer, deltaSeconds, *skeleton);
        const size_t mark = m_Program.m_Ops.size();
        bool pose = true;  // whether the layer's pose is on the program's stack (false: the empty pose)
        if (layer.m_CurrentState && layer.m_CurrentState->m_RootNode) pose = layer.m_CurrentState->m_RootNode->Advance(context, deltaSeconds, m_Program);
        else Push(m_Program, PoseOp::Rest, 0, 0.0f);
        if (layer.m_NextState && layer.m_TransitionDuration > 0.0f && layer.m_NextState->m_RootNode) {
            const size_t target_mark = m_Program.m_Ops.size();
            const bool target = layer.m_NextState->m_RootNode->Advance(context, deltaSeconds, m_Program);
            const float T = glm::clamp(layer.m_TransitionElapsed / layer.m_TransitionDuration, 0.0f, 1.0f);
            if (pose && target) Push(m_Program, PoseOp::Blend, PoseOp::s_NoMask, T);
            else m_Program.m_Ops.resize(target_mark);
        }
        if (!pose) {  // an empty layer pose: the layer's blend runs over no bones
            m_Program.m_Ops.resize(mark);
            continue;
        }
        uint32_t mask = PoseOp::s_NoMask;
        const std::vector<float>& w = layer.m_Mask.m_BoneWeights;
        if (std::any_of(w.begin(), w.end(), [](float x) { return !(x == 1.0f); })) {
            mask = (uint32_t)m_Program.m_Masks.size();
            m_Program.m_Masks.push_back(layer.m_Mask);
        }
        Push(m_Program, layer.m_IsAdditive ? PoseOp::Add : PoseOp::Blend, mask, layer.m_Weight);
    }
    return true;
}

// AnimationStateMachine.cpp:330-407, in its order
void AnimationStateMachine::UpdateLayer(AnimationLayer& layer, float deltaSeconds, const Skeleton& skeleton) {
    if (!layer.m_CurrentState) {
        layer.m_CurrentState = FindState(layer, layer.m_EntryState);
        if (layer.m_CurrentState) {
            if (layer.m_CurrentState->m_RootNode) layer.m_CurrentState->m_RootNode->Reset();
            layer.m_TimeInState = 0.0f;
        }
    }
    if (!layer.m_CurrentState) return;

    layer.m_TimeInState += deltaSeconds;

    if (layer.m_NextState) {
        layer.m_TransitionElapsed += deltaSeconds;
        if (layer.m_TransitionDuration <= 0.0f || layer.m_TransitionElapsed >= layer.m_TransitionDuration) {
            layer.m_CurrentState = layer.m_NextState;
            layer.m_NextState = nullptr;
            layer.m_TransitionElapsed = 0.0f;
            layer.m_TransitionDuration = 0.0f;
            layer.m_TimeInState = 0.0f;
        }
    }

    const std::vector<AnimationTransition>& transitions = layer.m_CurrentState->m_Transitions;
    for (size_t i = 0; i < transitions.size() && !layer.m_NextState; ++i) {
        const AnimationTransition& transition = transitions[i];
        if (transition.m_HasExitTime && layer.m_TimeInState < transition.m_ExitTimeSeconds) continue;
        if (!EvaluateTransitionConditions(transition)) continue;
        AnimationState* target = FindState(layer, transition.m_TargetState);
        if (!target) continue;
        if (target->m_RootNode) target->m_RootNode->Reset();
        layer.m_NextState = target;
        layer.m_TransitionDuration = transition.m_FadeDurationSeconds;
        layer.m_TransitionElapsed = 0.0f;
        if (layer.m_TransitionDuration <= 0.0f) {  // snap
            layer.m_CurrentState = layer.m_NextState;
            layer.m_NextState = nullptr;
            layer.m_TimeInState = 0.0f;
            // as in the reference the scan goes on over the transitions of the state just left (`transitions` is still
            // that state's list), so a later one of them may start a fade out of the new state in the same update
        }
    }

    layer.m_Mask.Resize(skeleton.m_Bones.size());
}

// :409-504. A Triggered condition consumes the trigger when it is reached, whatever the conditions after it say.
bool AnimationStateMachine::EvaluateTransitionConditions(const AnimationTransition& transition) {
    for (const AnimationTransitionCondition& c : transition.m_Conditions) {
        auto found = m_Parameters.find(c.m_ParameterName);
        if (found == m_Parameters.end()) return false;
        AnimationParameter& p = found->second;
        bool holds = false;
        switch (c.m_Comparison) {
            case AnimationConditionComparison::Equals:
            case AnimationConditionComparison::NotEquals: {
                const bool wantEqual = c.m_Comparison == AnimationConditionComparison::Equals;
                if (p.m_Type == AnimationParameterType::Bool) holds = (p.AsBool(false) == c.m_BoolValue) == wantEqual;
                else if (p.m_Type == AnimationParameterType::Integer) holds = (p.AsInt(0) == c.m_IntValue) == wantEqual;
                else {  // floats within eps are equal; a NaN difference passes both comparisons, as in the reference
                    const float d = std::fabs(p.AsFloat(0.0f) - c.m_FloatValue);
                    holds = wantEqual ? !(d > FLT_EPSILON) : !(d <= FLT_EPSILON);
                }
                break;
            }
            case AnimationConditionComparison::GreaterThan: holds = p.AsFloat(0.0f) > c.m_FloatValue; break;
            case AnimationConditionComparison::LessThan: holds = p.AsFloat(0.0f) < c.m_FloatValue; break;
            case AnimationConditionComparison::GreaterOrEqual: holds = p.AsFloat(0.0f) >= c.m_FloatValue; break;
            case AnimationConditionComparison::LessOrEqual: holds = p.AsFloat(0.0f) <= c.m_FloatValue; break;
            case AnimationConditionComparison::Triggered: holds = p.ConsumeTrigger(); break;
        }
        if (!holds) return false;
    }
    return true;
}

}  // namespace Animation
}  // namespace Trident
