// AnimationSystem.cpp — see AnimationSystem.h.
#include "trident/AnimationSystem.h"
#include "trident/Renderer.h"

#include <functional>

namespace Trident {
namespace ECS {

namespace {

constexpr size_t kInvalid = Animation::AnimationAssetService::s_InvalidHandle;

void Configure(Animation::AnimationPlayer& player, const AnimationComponent& c) {
    player.SetSkeletonHandle(c.m_SkeletonAssetHandle);
    player.SetAnimationHandle(c.m_AnimationAssetHandle);
    player.SetClipIndex(c.m_CurrentClipIndex);
    player.SetPlaybackSpeed(c.m_PlaybackSpeed);
    player.SetLooping(c.m_IsLooping);
}

}  // namespace

void AnimationSystem::RefreshCachedHandles(AnimationComponent& c, Animation::AnimationAssetService& service) {
    const std::hash<std::string> hash;
    if (c.m_SkeletonAssetId.empty()) {
        c.m_SkeletonAssetHandle = kInvalid;
        c.m_SkeletonAssetHash = 0;
    } else if (const size_t h = hash(c.m_SkeletonAssetId); c.m_SkeletonAssetHandle == kInvalid || h != c.m_SkeletonAssetHash) {
        c.m_SkeletonAssetHash = h;
        c.m_SkeletonAssetHandle = service.AcquireSkeleton(c.m_SkeletonAssetId);
    }
    if (c.m_AnimationAssetId.empty()) {
        c.m_AnimationAssetHandle = kInvalid;
        c.m_AnimationAssetHash = 0;
        c.m_CurrentClipIndex = kInvalid;
    } else if (const size_t h = hash(c.m_AnimationAssetId); c.m_AnimationAssetHandle == kInvalid || h != c.m_AnimationAssetHash) {
        c.m_AnimationAssetHash = h;
        c.m_AnimationAssetHandle = service.AcquireAnimationLibrary(c.m_AnimationAssetId);
        c.m_CurrentClipIndex = kInvalid;
        c.m_CurrentClipHash = 0;  // the clip name is looked up again in the new library
    }
    if (c.m_CurrentClip.empty() || c.m_AnimationAssetHandle == kInvalid) {
        c.m_CurrentClipIndex = kInvalid;
        c.m_CurrentClipHash = 0;
    } else if (const size_t h = hash(c.m_CurrentClip); h != c.m_CurrentClipHash) {
        c.m_CurrentClipHash = h;
        c.m_CurrentClipIndex = service.ResolveClipIndex(c.m_AnimationAssetHandle, c.m_CurrentClip);
    }
}

void AnimationSystem::InitialisePose(AnimationComponent& c) {
    c.m_BoneMatrices.clear();
    Animation::AnimationAssetService& service = Animation::AnimationAssetService::Get();
    RefreshCachedHandles(c, service);
    if (c.m_StateMachine) {
        c.m_StateMachine->SetSkeletonHandle(c.m_SkeletonAssetHandle);
        c.m_StateMachine->SetAnimationLibraryHandle(c.m_AnimationAssetHandle);
        c.m_StateMachine->Update(0.0f);
        c.m_StateMachine->CopyPose(c.m_BoneMatrices);
        return;
    }
    Animation::AnimationPlayer player(service);
    Configure(player, c);
    player.SetIsPlaying(true);
    player.EvaluateAt(0.0f);
    player.CopyPoseTo(c.m_BoneMatrices);
}

void AnimationSystem::EvaluatePose(AnimationComponent& c) {
    Animation::AnimationAssetService& service = Animation::AnimationAssetService::Get();
    RefreshCachedHandles(c, service);
    if (c.m_StateMachine) {  // at the machine's current state: its last program, nothing advanced
        c.m_StateMachine->Evaluate();
        c.m_StateMachine->CopyPose(c.m_BoneMatrices);
        return;
    }
    Animation::AnimationPlayer player(service);
    Configure(player, c);
    player.EvaluateAt(c.m_CurrentTime);
    player.CopyPoseTo(c.m_BoneMatrices);
}

void AnimationSystem::Update(Registry& registry, float deltaTime) {
    for (Entity e : registry.GetEntities()) {
        if (!registry.HasComponent<AnimationComponent>(e) || !registry.HasComponent<MeshComponent>(e)) continue;
        UpdateComponent(registry.GetComponent<AnimationComponent>(e), deltaTime);
    }
}

void AnimationSystem::UpdateComponent(AnimationComponent& c, float deltaTime) {
    RefreshCachedHandles(c, Animation::AnimationAssetService::Get());
    if (c.m_StateMachine) {
        c.m_StateMachine->SetSkeletonHandle(c.m_SkeletonAssetHandle);
        c.m_StateMachine->SetAnimationLibraryHandle(c.m_AnimationAssetHandle);
        if (!c.m_StateMachine->Advance(c.m_IsPlaying ? deltaTime : 0.0f)) return;
        if (m_Renderer && m_Renderer->PosesOnDevice(c)) return;  // the device evaluates this update's program
        c.m_StateMachine->Evaluate();
        c.m_StateMachine->CopyPose(c.m_BoneMatrices);
        return;
    }
    Configure(m_Player, c);
    m_Player.SetIsPlaying(c.m_IsPlaying);
    m_Player.SetCurrentTime(c.m_CurrentTime);
    const bool evaluate = !(m_Renderer && m_Renderer->PosesOnDevice(c));  // the device evaluates what it takes
    if (!evaluate) {  // time and play state only
        m_Player.AdvanceTime(deltaTime);
    } else if (c.m_IsPlaying) {
        m_Player.Update(deltaTime);
    } else {
        m_Player.EvaluateAt(c.m_CurrentTime);  // a paused preview keeps its sample time
    }
    c.m_CurrentTime = m_Player.GetCurrentTime();
    c.m_IsPlaying = m_Player.IsPlaying();
    if (evaluate) m_Player.CopyPoseTo(c.m_BoneMatrices);
}

}  // namespace ECS
}  // namespace Trident
