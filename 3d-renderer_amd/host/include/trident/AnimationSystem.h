// AnimationSystem.h — ECS::AnimationSystem (ECS/AnimationSystem.h, ECS/Components/AnimationSystem.cpp:23-164): every
// entity with an AnimationComponent and a MeshComponent has its cached handles refreshed, its clip time advanced and,
// unless poses are evaluated on the device, its m_BoneMatrices written by the CPU player. A component with an
// m_StateMachine is driven by it instead (:77-86, :126-137): the machine takes the component's handles, updates by the
// frame's delta (0 while m_IsPlaying is false) and its pose becomes m_BoneMatrices. With a renderer that poses on the
// device (Renderer::PosesOnDevice) the machine is only advanced: the renderer submits the program the update emitted.
#pragma once

#include "Animation.h"
#include "AnimationStateMachine.h"
#include "Scene.h"

namespace Trident {

class Renderer;

namespace ECS {

class AnimationSystem {
public:
    // renderer: whose Renderer::SetDevicePoseEnabled decides what Update evaluates (Forge passes
    // &RenderCommand::GetRenderer()); without one every pose is evaluated on the CPU.
    explicit AnimationSystem(const Renderer* renderer = nullptr)
        : m_Player(Animation::AnimationAssetService::Get()), m_Renderer(renderer) {}

    // Every entity with an AnimationComponent and a MeshComponent: handles refreshed, time and play state advanced,
    // and the pose written to m_BoneMatrices — except for the components the renderer poses on the device
    // (Renderer::PosesOnDevice), whose m_BoneMatrices are left alone.
    void Update(Registry& registry, float deltaTime);
    // Re-resolve the handles whose id string changed (or that are still invalid); an empty id clears its handle.
    static void RefreshCachedHandles(AnimationComponent& component, Animation::AnimationAssetService& service);
    // The pose at time 0 of the component's clip into m_BoneMatrices (the bind pose without a clip).
    static void InitialisePose(AnimationComponent& component);
    // The pose at the component's current time into m_BoneMatrices: what Update leaves there on the CPU path, on demand
    // for host code that reads the matrices while the renderer poses on the device.
    static void EvaluatePose(AnimationComponent& component);

private:
    void UpdateComponent(AnimationComponent& component, float deltaTime);

    Animation::AnimationPlayer m_Player;
    const Renderer* m_Renderer = nullptr;
};

}  // namespace ECS
}  // namespace Trident
