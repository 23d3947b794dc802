// Animation.h — Trident's skeletal animation data, asset service and player (Animation/AnimationData.h,
// AnimationAssetService.h, AnimationPlayer.h, AnimationRemap.h), restated on glm_subset.h. The field and method names
// are the reference's: they are the interface. The pose rules the player evaluates are stated once in
// include/tri_raster.h ("skeletal poses evaluated on the device"); this is their float32 CPU restatement, with the
// operation order of the device kernel (the shim builds with -ffp-contract=off).
// Also here: the pose-space types (Animation/AnimationPose.h) and the pose programs both pose evaluators interpret.
#pragma once

#include <cstddef>
#include <cstdint>
#include <limits>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "glm_subset.h"

namespace Trident {
namespace Animation {

struct VectorKeyframe {
    float m_TimeSeconds = 0.0f;
    glm::vec3 m_Value{0.0f};
};

struct QuaternionKeyframe {
    float m_TimeSeconds = 0.0f;
    glm::quat m_Value{1.0f, 0.0f, 0.0f, 0.0f};
};

struct TransformChannel {
    int m_BoneIndex = -1;
    std::string m_SourceBoneName;
    std::vector<VectorKeyframe> m_TranslationKeys{};
    std::vector<QuaternionKeyframe> m_RotationKeys{};
    std::vector<VectorKeyframe> m_ScaleKeys{};
};

struct AnimationClip {
    std::string m_Name;
    float m_DurationSeconds = 0.0f;
    float m_TicksPerSecond = 0.0f;
    std::vector<TransformChannel> m_Channels{};
};

struct Bone {
    std::string m_Name;        // trimmed, "mixamorig:" removed
    std::string m_SourceName;  // as authored
    int m_ParentIndex = -1;
    std::vector<int> m_Children{};
    glm::mat4 m_LocalBindTransform{1.0f};
    glm::mat4 m_InverseBindMatrix{1.0f};
};

struct Skeleton {
    int m_RootBoneIndex = -1;
    std::vector<Bone> m_Bones{};
    std::unordered_map<std::string, int> m_NameToIndex{};
    std::unordered_map<std::string, int> m_SourceNameToIndex{};
};

// A bone's defaults: the decomposition of its local bind transform (AnimationPlayer.cpp:343-390). The device path
// receives exactly these floats (tri_pose_bone), so both float32 evaluations start from the same bits.
struct TransformDecomposition {
    glm::vec3 m_Translation{0.0f};
    glm::quat m_Rotation{1.0f, 0.0f, 0.0f, 0.0f};
    glm::vec3 m_Scale{1.0f};
};
TransformDecomposition DecomposeBindTransform(const glm::mat4& localBind);

// A bone name trimmed of white space, with a leading "mixamorig:" removed (AnimationRemap.cpp:16-40).
std::string NormaliseBoneName(std::string name);
// The bone a channel drives (AnimationRemap.cpp:43-91): the stored index when it is in range and either no name is
// stored or the bone's names agree with it; otherwise the source-name table; otherwise the normalised name in the
// normalised-name table; otherwise -1, with one warning on stderr.
int ResolveChannelBoneIndex(const TransformChannel& channel, const Skeleton& skeleton, const std::string& clipName);
// Child lists and both name tables from the bones' parents and names: what a skeleton built from flat arrays still
// lacks. m_RootBoneIndex stays as it is (unset: the traversal starts at every parentless bone).
void FinaliseSkeleton(Skeleton& skeleton);

// Whether the device path (tri_animset_add_skeleton / tri_animset_add_clip, include/tri_raster.h) takes this skeleton
// with these clips: 1..256 bones, parents in range, no parent cycle the traversal would reach, key times finite and
// non-decreasing, durations finite. What it refuses is evaluated on the CPU.
bool DevicePoseCompatible(const Skeleton& skeleton, const std::vector<AnimationClip>* clips);

class AnimationAssetService {
public:
    static constexpr size_t s_InvalidHandle = std::numeric_limits<size_t>::max();

    static AnimationAssetService& Get();

    // A new handle, or the id's existing one with its contents replaced; s_InvalidHandle for an empty id. Channels
    // without a source name take their bone's. The bones' m_Children are rebuilt from their m_ParentIndex: the
    // reference walks whatever child lists it is given; here the parents are the one statement of the hierarchy.
    size_t RegisterRuntimeAsset(const std::string& assetId, Skeleton skeleton, std::vector<AnimationClip> clips);
    // The handle of the id: a registered runtime asset, else the model file of that name, loaded through
    // Loader::ModelLoader once per id. s_InvalidHandle for an empty id or a file without bones and clips (one warning
    // per id).
    size_t AcquireSkeleton(const std::string& skeletonAssetId);
    size_t AcquireAnimationLibrary(const std::string& animationAssetId);
    size_t FindAsset(const std::string& assetId) const;
    bool AssetId(size_t handle, std::string& outAssetId) const;
    // Counts the registrations (RegisterRuntimeAsset, loads included): who caches what an asset holds compares it.
    uint64_t GetGeneration() const { return m_Generation; }
    size_t ResolveClipIndex(size_t animationHandle, const std::string& clipName) const;
    const Skeleton* GetSkeleton(size_t skeletonHandle) const;
    const std::vector<AnimationClip>* GetAnimationClips(size_t animationHandle) const;
    const AnimationClip* GetClip(size_t animationHandle, size_t clipIndex) const;

private:
    struct AssetRecord {
        std::string m_AssetId;
        Skeleton m_Skeleton;
        std::vector<AnimationClip> m_Clips;
        std::unordered_map<std::string, size_t> m_ClipLookup;
    };
    std::unordered_map<size_t, AssetRecord> m_Assets;
    std::unordered_map<std::string, size_t> m_IdToHandle;
    size_t m_NextHandle = 1;
    uint64_t m_Generation = 0;
    std::set<std::string> m_MissingIds;
    size_t LoadAssetIfNeeded(const std::string& assetId);
};

class AnimationPlayer {
public:
    explicit AnimationPlayer(AnimationAssetService& assetService) : m_AssetService(&assetService) {}

    void SetSkeletonHandle(size_t skeletonHandle) { m_SkeletonHandle = skeletonHandle; }
    void SetAnimationHandle(size_t animationHandle) { m_AnimationHandle = animationHandle; }
    void SetClipIndex(size_t clipIndex) { m_ClipIndex = clipIndex; }
    void SetPlaybackSpeed(float playbackSpeed) { m_PlaybackSpeed = playbackSpeed; }
    void SetLooping(bool isLooping) { m_IsLooping = isLooping; }
    void SetIsPlaying(bool isPlaying) { m_IsPlaying = isPlaying; }
    void SetCurrentTime(float timeSeconds) { m_CurrentTimeSeconds = timeSeconds; }

    // Advance by deltaSeconds * speed, wrap (looping) or clamp and stop (not looping) at either end of the clip, then
    // evaluate; a paused player re-evaluates at its current time (AnimationPlayer.cpp:57-102).
    void Update(float deltaSeconds);
    void EvaluateAt(float sampleTimeSeconds);
    // Update's time advance alone, no pose: what remains on the host when poses are evaluated on the device.
    void AdvanceTime(float deltaSeconds);

    float GetCurrentTime() const { return m_CurrentTimeSeconds; }
    bool IsPlaying() const { return m_IsPlaying; }
    float GetClipDuration() const;
    void CopyPoseTo(std::vector<glm::mat4>& outMatrices) const { outMatrices = m_PoseMatrices; }

private:
    void EvaluatePose(float sampleTimeSeconds);

    AnimationAssetService* m_AssetService = nullptr;
    size_t m_SkeletonHandle = AnimationAssetService::s_InvalidHandle;
    size_t m_AnimationHandle = AnimationAssetService::s_InvalidHandle;
    size_t m_ClipIndex = AnimationAssetService::s_InvalidHandle;
    float m_CurrentTimeSeconds = 0.0f;
    float m_PlaybackSpeed = 1.0f;
    bool m_IsLooping = true;
    bool m_IsPlaying = true;
    std::vector<glm::mat4> m_PoseMatrices{};
};

// ---- pose space (Animation/AnimationPose.h) ----
// A pose as decomposed TRS values per bone, masks of per-bone weights, and the arithmetic on them. The rules are
// include/tri_raster.h's ("Pose space"); this is their float32 restatement in the device kernel's operation order
// (k_pose_graph, csrc/pose_eval.hip): where neither side evaluates sin / acos the two agree bit for bit.
struct AnimationPose {
    void Resize(size_t boneCount);  // new bones: translation 0, rotation identity, scale 1

    std::vector<glm::vec3> m_Translations{};
    std::vector<glm::quat> m_Rotations{};
    std::vector<glm::vec3> m_Scales{};
};

struct AnimationMask {
    void Resize(size_t boneCount);             // pads with 1.0, truncates
    float GetWeight(size_t boneIndex) const;   // 1.0 beyond the weights

    std::vector<float> m_BoneWeights{};
};

namespace AnimationPoseUtilities {
AnimationPose BuildRestPose(const Skeleton& skeleton);
AnimationPose SampleClipPose(const Skeleton& skeleton, const AnimationClip& clip, float sampleTimeSeconds);
// Both run over min(sizes) bones: an empty pose on either side leaves the base as it is.
void BlendPose(AnimationPose& basePose, const AnimationPose& targetPose, float blendWeight, const AnimationMask* mask);
void AdditivePose(AnimationPose& basePose, const AnimationPose& additivePose, float additiveWeight, const AnimationMask* mask);
// One matrix per bone. A pose shorter than the skeleton is completed with the rest pose's values; a parent cycle the
// traversal would reach gives identities (the reference would not return).
std::vector<glm::mat4> ComposeSkinningMatrices(const Skeleton& skeleton, const AnimationPose& pose);
}  // namespace AnimationPoseUtilities

// ---- pose programs ----
// What one update of an animation graph means, as the postfix program of include/tri_raster.h (tri_pose_op): the
// state machine emits it, EvaluatePoseProgram is its CPU meaning and tri_pose_graph its device meaning. m_A of a Clip
// indexes the animation library's clips, m_A of a Blend / Add indexes m_Masks (or is s_NoMask).
struct PoseOp {
    enum Kind : uint32_t { Rest = 0, Clip = 1, Blend = 2, Add = 3 };
    static constexpr uint32_t s_NoMask = 0xFFFFFFFFu;
    uint32_t m_Op = Rest;
    uint32_t m_A = 0;
    float m_F = 0.0f;
};

struct PoseProgram {
    static constexpr size_t s_MaxOps = 64;   // TRI_POSE_MAX_OPS
    static constexpr size_t s_MaxStack = 8;  // TRI_POSE_STACK
    std::vector<PoseOp> m_Ops{};
    std::vector<AnimationMask> m_Masks{};

    // The stack discipline alone (never below two entries for a Blend / Add, one entry at the end, known ops).
    bool WellFormed() const;
    // WellFormed within the device's two limits.
    bool FitsDevice() const;
};

// The program's final pose; false (outPose untouched) for a program that is not WellFormed or names a clip or mask
// that does not exist. No limit on depth or length here.
bool EvaluatePoseProgram(const Skeleton& skeleton, const std::vector<AnimationClip>* clips, const PoseProgram& program,
                         AnimationPose& outPose);

}  // namespace Animation
}  // namespace Trident
