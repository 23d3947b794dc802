// Animation.cpp — the asset service and the CPU player (see Animation.h). The pose rules are include/tri_raster.h's
// ("skeletal poses evaluated on the device"); every float operation below is written in the order stated there, which
// is also the device kernel's (csrc/pose_eval.hip): where neither side calls sin / acos the two agree bit for bit.
#include "trident/Animation.h"
#include "trident/ModelLoader.h"

#include <algorithm>
#include <cctype>
#include <cfloat>
#include <cmath>
#include <cstdio>

namespace Trident {
namespace Animation {

namespace {

constexpr float kEps = FLT_EPSILON;

float Clamp01(float x) {
    const float lo = x < 0.0f ? 0.0f : x;  // glm::max(x, 0)
    return 1.0f < lo ? 1.0f : lo;          // glm::min(.., 1)
}

float QuatDot(const glm::quat& a, const glm::quat& b) { return (a.w * b.w + a.x * b.x) + (a.y * b.y + a.z * b.z); }

// glm::slerp
glm::quat Slerp(const glm::quat& a, const glm::quat& b, float T) {
    glm::quat z = b;
    float c = QuatDot(a, b);
    if (c < 0.0f) {
        z = glm::quat(-b.w, -b.x, -b.y, -b.z);
        c = -c;
    }
    if (c > 1.0f - kEps) {
        const float u = 1.0f - T;
        return glm::quat(a.w * u + z.w * T, a.x * u + z.x * T, a.y * u + z.y * T, a.z * u + z.z * T);
    }
    const float A = std::acos(c);
    const float s0 = std::sin((1.0f - T) * A), s1 = std::sin(T * A), s2 = std::sin(A);
    return glm::quat((s0 * a.w + s1 * z.w) / s2, (s0 * a.x + s1 * z.x) / s2, (s0 * a.y + s1 * z.y) / s2,
                     (s0 * a.z + s1 * z.z) / s2);
}

// glm::quat_cast of the 3x3 matrix with columns c0, c1, c2
glm::quat QuatCast(const glm::vec3& c0, const glm::vec3& c1, const glm::vec3& c2) {
    const float fourX = c0.x - c1.y - c2.z, fourY = c1.y - c0.x - c2.z, fourZ = c2.z - c0.x - c1.y;
    const float fourW = c0.x + c1.y + c2.z;
    int biggest = 0;
    float four = fourW;
    if (fourX > four) { four = fourX; biggest = 1; }
    if (fourY > four) { four = fourY; biggest = 2; }
    if (fourZ > four) { four = fourZ; biggest = 3; }
    const float val = std::sqrt(four + 1.0f) * 0.5f;
    const float mult = 0.25f / val;
    switch (biggest) {
        case 0: return glm::quat(val, (c1.z - c2.y) * mult, (c2.x - c0.z) * mult, (c0.y - c1.x) * mult);
        case 1: return glm::quat((c1.z - c2.y) * mult, val, (c0.y + c1.x) * mult, (c2.x + c0.z) * mult);
        case 2: return glm::quat((c2.x - c0.z) * mult, (c0.y + c1.x) * mult, val, (c1.z + c2.y) * mult);
        default: return glm::quat((c0.y - c1.x) * mult, (c2.x + c0.z) * mult, (c1.z + c2.y) * mult, val);
    }
}

// The key pair around t for a track of at least two keys with t > its first time: the first i with
// t < time[i + 1], and the interpolation factor. False when there is none (t at or past the last key, or NaN).
template <typename Key>
bool FindKeys(const std::vector<Key>& keys, float t, size_t& i, float& T) {
    for (i = 0; i + 1 < keys.size(); ++i) {
        if (t < keys[i + 1].m_TimeSeconds) {
            const float a = keys[i].m_TimeSeconds, d = keys[i + 1].m_TimeSeconds - a;
            T = Clamp01(d > kEps ? (t - a) / d : 0.0f);
            return true;
        }
    }
    return false;
}

glm::vec3 SampleVectorKeys(const std::vector<VectorKeyframe>& keys, float t, const glm::vec3& def) {
    if (keys.empty()) return def;
    if (keys.size() == 1 || t <= keys.front().m_TimeSeconds) return keys.front().m_Value;
    size_t i;
    float T;
    if (!FindKeys(keys, t, i, T)) return keys.back().m_Value;
    const glm::vec3 &a = keys[i].m_Value, &b = keys[i + 1].m_Value;
    const float u = 1.0f - T;
    return glm::vec3(a.x * u + b.x * T, a.y * u + b.y * T, a.z * u + b.z * T);
}

glm::quat SampleQuaternionKeys(const std::vector<QuaternionKeyframe>& keys, float t, const glm::quat& def) {
    if (keys.empty()) return def;
    if (keys.size() == 1 || t <= keys.front().m_TimeSeconds) return glm::normalize(keys.front().m_Value);
    size_t i;
    float T;
    if (!FindKeys(keys, t, i, T)) return glm::normalize(keys.back().m_Value);
    return glm::normalize(Slerp(keys[i].m_Value, keys[i + 1].m_Value, T));
}

// translate * toMat4(normalize(q)) * scale in the rules' closed form
glm::mat4 LocalMatrix(const glm::vec3& t, const glm::quat& r, const glm::vec3& s) {
    const glm::mat4 R = glm::mat4_cast(glm::normalize(r));
    glm::mat4 m(1.0f);
    m[0] = glm::vec4(R[0].x * s.x, R[0].y * s.x, R[0].z * s.x, 0.0f);
    m[1] = glm::vec4(R[1].x * s.y, R[1].y * s.y, R[1].z * s.y, 0.0f);
    m[2] = glm::vec4(R[2].x * s.z, R[2].y * s.z, R[2].z * s.z, 0.0f);
    m[3] = glm::vec4(t.x, t.y, t.z, 1.0f);
    return m;
}

bool IsIdentity(const glm::mat4& m) {
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r)
            if (!(m[c][r] == (c == r ? 1.0f : 0.0f))) return false;
    return true;
}

void FillMissingChannelNames(const Skeleton& skeleton, std::vector<AnimationClip>& clips) {
    for (AnimationClip& clip : clips)
        for (TransformChannel& ch : clip.m_Channels) {
            if (!ch.m_SourceBoneName.empty() || ch.m_BoneIndex < 0 || (size_t)ch.m_BoneIndex >= skeleton.m_Bones.size())
                continue;
            const Bone& bone = skeleton.m_Bones[(size_t)ch.m_BoneIndex];
            ch.m_SourceBoneName = bone.m_SourceName.empty() ? bone.m_Name : bone.m_SourceName;
        }
}

}  // namespace

TransformDecomposition DecomposeBindTransform(const glm::mat4& m) {
    TransformDecomposition out;
    out.m_Translation = glm::vec3(m[3].x, m[3].y, m[3].z);
    glm::vec3 col[3];
    for (int j = 0; j < 3; ++j) {
        col[j] = glm::vec3(m[j].x, m[j].y, m[j].z);
        const float len = glm::length(col[j]);
        out.m_Scale[j] = len;
        if (len > kEps) col[j] = glm::vec3(col[j].x / len, col[j].y / len, col[j].z / len);
    }
    out.m_Rotation = glm::normalize(QuatCast(col[0], col[1], col[2]));
    return out;
}

std::string NormaliseBoneName(std::string name) {
    auto space = [](unsigned char ch) { return std::isspace(ch) != 0; };
    size_t b = 0, e = name.size();
    while (b < e && space((unsigned char)name[b])) ++b;
    while (e > b && space((unsigned char)name[e - 1])) --e;
    name = name.substr(b, e - b);
    static const std::string prefix = "mixamorig:";
    if (name.size() > prefix.size() && name.compare(0, prefix.size(), prefix) == 0) name.erase(0, prefix.size());
    return name;
}

int ResolveChannelBoneIndex(const TransformChannel& channel, const Skeleton& skeleton, const std::string& clipName) {
    const int n = (int)skeleton.m_Bones.size();
    const std::string& source = channel.m_SourceBoneName;
    const int stored = channel.m_BoneIndex;
    if (stored >= 0 && stored < n) {
        const Bone& bone = skeleton.m_Bones[(size_t)stored];
        if (source.empty() || bone.m_SourceName == source || bone.m_Name == source) return stored;
    }
    int found = -1;
    if (!source.empty()) {
        auto it = skeleton.m_SourceNameToIndex.find(source);
        if (it != skeleton.m_SourceNameToIndex.end()) found = it->second;
        else {
            it = skeleton.m_NameToIndex.find(NormaliseBoneName(source));
            if (it != skeleton.m_NameToIndex.end()) found = it->second;
        }
    }
    if (found < 0 || found >= n) {
        std::fprintf(stderr, "[Trident] Animation: clip '%s': no bone for the channel targeting '%s' (stored index %d)\n",
                     clipName.empty() ? "<unnamed>" : clipName.c_str(), source.c_str(), stored);
        return -1;
    }
    return found;
}

void FinaliseSkeleton(Skeleton& skeleton) {
    const int n = (int)skeleton.m_Bones.size();
    skeleton.m_NameToIndex.clear();
    skeleton.m_SourceNameToIndex.clear();
    for (Bone& bone : skeleton.m_Bones) bone.m_Children.clear();
    for (int b = 0; b < n; ++b) {
        Bone& bone = skeleton.m_Bones[(size_t)b];
        if (bone.m_Name.empty()) bone.m_Name = NormaliseBoneName(bone.m_SourceName);
        skeleton.m_NameToIndex.emplace(bone.m_Name, b);
        skeleton.m_SourceNameToIndex.emplace(bone.m_SourceName, b);
        if (bone.m_ParentIndex >= 0 && bone.m_ParentIndex < n) skeleton.m_Bones[(size_t)bone.m_ParentIndex].m_Children.push_back(b);
    }
}

bool DevicePoseCompatible(const Skeleton& skeleton, const std::vector<AnimationClip>* clips) {
    const size_t n = skeleton.m_Bones.size();
    if (n < 1 || n > 256) return false;
    for (const Bone& bone : skeleton.m_Bones)
        if (bone.m_ParentIndex >= (int)n) return false;
    std::vector<char> seen(n, 0);
    std::vector<size_t> queue;
    auto start = [&](size_t b) { seen[b] = 1; queue.push_back(b); };
    if (skeleton.m_RootBoneIndex >= 0 && (size_t)skeleton.m_RootBoneIndex < n) start((size_t)skeleton.m_RootBoneIndex);
    else {
        for (size_t b = 0; b < n; ++b)
            if (skeleton.m_Bones[b].m_ParentIndex < 0) start(b);
        if (queue.empty()) start(0);
    }
    for (size_t q = 0; q < queue.size(); ++q)
        for (size_t c = 0; c < n; ++c) {
            if (skeleton.m_Bones[c].m_ParentIndex != (int)queue[q]) continue;
            if (seen[c]) return false;
            seen[c] = 1;
            queue.push_back(c);
        }
    auto ordered = [](const auto& keys) {
        for (size_t i = 0; i < keys.size(); ++i) {
            if (!std::isfinite(keys[i].m_TimeSeconds)) return false;
            if (i && keys[i].m_TimeSeconds < keys[i - 1].m_TimeSeconds) return false;
        }
        return true;
    };
    if (clips)
        for (const AnimationClip& clip : *clips) {
            if (!std::isfinite(clip.m_DurationSeconds)) return false;
            for (const TransformChannel& ch : clip.m_Channels)
                if (!ordered(ch.m_TranslationKeys) || !ordered(ch.m_RotationKeys) || !ordered(ch.m_ScaleKeys)) return false;
        }
    return true;
}

AnimationAssetService& AnimationAssetService::Get() {
    static AnimationAssetService instance;
    return instance;
}

size_t AnimationAssetService::RegisterRuntimeAsset(const std::string& assetId, Skeleton skeleton, std::vector<AnimationClip> clips) {
    if (assetId.empty()) return s_InvalidHandle;
    m_MissingIds.erase(assetId);
    ++m_Generation;
    FillMissingChannelNames(skeleton, clips);
    // the parents are the one statement of the hierarchy (as in tri_pose_bone): child lists that came with the skeleton
    // are replaced by the ones the parents imply, so the traversal along either is the same
    for (Bone& bone : skeleton.m_Bones) bone.m_Children.clear();
    for (size_t b = 0; b < skeleton.m_Bones.size(); ++b) {
        const int parent = skeleton.m_Bones[b].m_ParentIndex;
        if (parent >= 0 && (size_t)parent < skeleton.m_Bones.size()) skeleton.m_Bones[(size_t)parent].m_Children.push_back((int)b);
    }
    size_t handle;
    auto known = m_IdToHandle.find(assetId);
    if (known != m_IdToHandle.end()) handle = known->second;
    else {
        handle = m_NextHandle++;
        m_IdToHandle[assetId] = handle;
    }
    AssetRecord& rec = m_Assets[handle];
    rec.m_AssetId = assetId;
    rec.m_Skeleton = std::move(skeleton);
    rec.m_Clips = std::move(clips);
    rec.m_ClipLookup.clear();
    for (size_t i = 0; i < rec.m_Clips.size(); ++i) rec.m_ClipLookup.emplace(rec.m_Clips[i].m_Name, i);  // first of a name wins
    return handle;
}

// The handle of an id: what RegisterRuntimeAsset put there, else the model file of that name loaded through
// Loader::ModelLoader once (a file that yields neither bones nor clips is remembered as missing and warned about once).
size_t AnimationAssetService::LoadAssetIfNeeded(const std::string& assetId) {
    if (assetId.empty()) return s_InvalidHandle;
    const size_t known = FindAsset(assetId);
    if (known != s_InvalidHandle) return known;
    if (m_MissingIds.count(assetId)) return s_InvalidHandle;
    Loader::ModelData model = Loader::ModelLoader::Load(assetId);
    if (model.m_Skeleton.m_Bones.empty() && model.m_AnimationClips.empty()) {
        m_MissingIds.insert(assetId);
        std::fprintf(stderr, "[Trident] Animation: asset '%s' could not be loaded; identity pose\n", assetId.c_str());
        return s_InvalidHandle;
    }
    return RegisterRuntimeAsset(assetId, std::move(model.m_Skeleton), std::move(model.m_AnimationClips));
}

size_t AnimationAssetService::AcquireSkeleton(const std::string& skeletonAssetId) { return LoadAssetIfNeeded(skeletonAssetId); }

size_t AnimationAssetService::AcquireAnimationLibrary(const std::string& animationAssetId) { return LoadAssetIfNeeded(animationAssetId); }

size_t AnimationAssetService::FindAsset(const std::string& assetId) const {
    auto it = m_IdToHandle.find(assetId);
    return it == m_IdToHandle.end() ? s_InvalidHandle : it->second;
}

bool AnimationAssetService::AssetId(size_t handle, std::string& outAssetId) const {
    auto rec = m_Assets.find(handle);
    if (handle == s_InvalidHandle || rec == m_Assets.end()) return false;
    outAssetId = rec->second.m_AssetId;
    return true;
}

size_t AnimationAssetService::ResolveClipIndex(size_t animationHandle, const std::string& clipName) const {
    if (animationHandle == s_InvalidHandle || clipName.empty()) return s_InvalidHandle;
    auto rec = m_Assets.find(animationHandle);
    if (rec == m_Assets.end()) return s_InvalidHandle;
    auto clip = rec->second.m_ClipLookup.find(clipName);
    if (clip == rec->second.m_ClipLookup.end()) {
        std::fprintf(stderr, "[Trident] Animation: asset '%s' has no clip '%s'\n", rec->second.m_AssetId.c_str(), clipName.c_str());
        return s_InvalidHandle;
    }
    return clip->second;
}

const Skeleton* AnimationAssetService::GetSkeleton(size_t skeletonHandle) const {
    auto rec = m_Assets.find(skeletonHandle);
    return skeletonHandle == s_InvalidHandle || rec == m_Assets.end() ? nullptr : &rec->second.m_Skeleton;
}

const std::vector<AnimationClip>* AnimationAssetService::GetAnimationClips(size_t animationHandle) const {
    auto rec = m_Assets.find(animationHandle);
    return animationHandle == s_InvalidHandle || rec == m_Assets.end() ? nullptr : &rec->second.m_Clips;
}

const AnimationClip* AnimationAssetService::GetClip(size_t animationHandle, size_t clipIndex) const {
    const std::vector<AnimationClip>* clips = GetAnimationClips(animationHandle);
    if (!clips || clipIndex == s_InvalidHandle || clipIndex >= clips->size()) return nullptr;
    return &(*clips)[clipIndex];
}

float AnimationPlayer::GetClipDuration() const {
    const AnimationClip* clip = m_AssetService ? m_AssetService->GetClip(m_AnimationHandle, m_ClipIndex) : nullptr;
    return clip ? clip->m_DurationSeconds : 0.0f;
}

void AnimationPlayer::Update(float deltaSeconds) {
    AdvanceTime(deltaSeconds);
    EvaluatePose(m_CurrentTimeSeconds);  // paused players refresh too
}

void AnimationPlayer::AdvanceTime(float deltaSeconds) {
    if (m_IsPlaying) {
        m_CurrentTimeSeconds += deltaSeconds * m_PlaybackSpeed;
        const float duration = GetClipDuration();
        if (duration > 0.0f && (m_CurrentTimeSeconds > duration || m_CurrentTimeSeconds < 0.0f)) {
            if (m_IsLooping) {
                const float mod = std::fmod(m_CurrentTimeSeconds, duration);
                m_CurrentTimeSeconds = mod < 0.0f ? duration + mod : mod;
            } else {
                m_CurrentTimeSeconds = m_CurrentTimeSeconds < 0.0f ? 0.0f : duration;
                m_IsPlaying = false;
            }
        }
    }
}

void AnimationPlayer::EvaluateAt(float sampleTimeSeconds) {
    m_CurrentTimeSeconds = sampleTimeSeconds;
    EvaluatePose(sampleTimeSeconds);
}

namespace {

// A clip's channels applied in order to per-bone values that hold the defaults.
void SampleChannels(const Skeleton& skeleton, const AnimationClip& clip, float t, std::vector<TransformDecomposition>& value) {
    const size_t n = value.size();
    for (const TransformChannel& ch : clip.m_Channels) {
        const int bone = ResolveChannelBoneIndex(ch, skeleton, clip.m_Name);
        if (bone < 0 || (size_t)bone >= n) continue;
        TransformDecomposition& v = value[(size_t)bone];
        v.m_Translation = SampleVectorKeys(ch.m_TranslationKeys, t, v.m_Translation);
        v.m_Rotation = SampleQuaternionKeys(ch.m_RotationKeys, t, v.m_Rotation);
        v.m_Scale = SampleVectorKeys(ch.m_ScaleKeys, t, v.m_Scale);
    }
}

// Local matrices, the traversal along the parents (a bone's children are the bones that name it as their parent), the
// two fix-ups and global * inverse_bind. False for a cycle the reference would walk for ever.
bool ComposeValues(const Skeleton& skeleton, const std::vector<TransformDecomposition>& value, std::vector<glm::mat4>& out) {
    const size_t n = skeleton.m_Bones.size();
    std::vector<glm::mat4> local(n), global(n);
    for (size_t b = 0; b < n; ++b) local[b] = LocalMatrix(value[b].m_Translation, value[b].m_Rotation, value[b].m_Scale);

    std::vector<char> reached(n, 0);
    std::vector<size_t> queue;
    queue.reserve(n);
    const glm::mat4 identity(1.0f);
    auto start = [&](size_t b) {
        reached[b] = 1;
        global[b] = identity * local[b];
        queue.push_back(b);
    };
    if (skeleton.m_RootBoneIndex >= 0 && (size_t)skeleton.m_RootBoneIndex < n) start((size_t)skeleton.m_RootBoneIndex);
    else {
        for (size_t b = 0; b < n; ++b)
            if (skeleton.m_Bones[b].m_ParentIndex < 0) start(b);
        if (queue.empty()) start(0);
    }
    for (size_t q = 0; q < queue.size(); ++q) {
        const size_t b = queue[q];
        for (size_t c = 0; c < n; ++c) {
            if (skeleton.m_Bones[c].m_ParentIndex != (int)b) continue;
            if (reached[c]) {  // a cycle the reference would walk for ever: refused
                std::fprintf(stderr, "[Trident] Animation: the skeleton's parents form a cycle; identity pose\n");
                return false;
            }
            reached[c] = 1;
            global[c] = global[b] * local[c];
            queue.push_back(c);
        }
    }
    out.resize(n);
    for (size_t b = 0; b < n; ++b) {
        if (!reached[b] || IsIdentity(global[b])) global[b] = local[b];
        out[b] = global[b] * skeleton.m_Bones[b].m_InverseBindMatrix;
    }
    return true;
}

// glm's quaternion product, each line left to right
glm::quat QuatMul(const glm::quat& p, const glm::quat& q) {
    return glm::quat(((p.w * q.w - p.x * q.x) - p.y * q.y) - p.z * q.z, ((p.w * q.x + p.x * q.w) + p.y * q.z) - p.z * q.y,
                     ((p.w * q.y + p.y * q.w) + p.z * q.x) - p.x * q.z, ((p.w * q.z + p.z * q.w) + p.x * q.y) - p.y * q.x);
}

glm::vec3 Mix3(const glm::vec3& a, const glm::vec3& b, float F) {
    const float u = 1.0f - F;
    return glm::vec3(a.x * u + b.x * F, a.y * u + b.y * F, a.z * u + b.z * F);
}

}  // namespace

void AnimationPlayer::EvaluatePose(float t) {
    const Skeleton* skeleton = m_AssetService ? m_AssetService->GetSkeleton(m_SkeletonHandle) : nullptr;
    auto fallback = [&]() {  // identities, as many as the last pose had (at least one)
        m_PoseMatrices.assign(std::max<size_t>(m_PoseMatrices.size(), 1), glm::mat4(1.0f));
    };
    if (!skeleton || skeleton->m_Bones.empty()) return fallback();
    const AnimationClip* clip = m_AssetService->GetClip(m_AnimationHandle, m_ClipIndex);
    const size_t n = skeleton->m_Bones.size();

    std::vector<TransformDecomposition> value(n);
    for (size_t b = 0; b < n; ++b) value[b] = DecomposeBindTransform(skeleton->m_Bones[b].m_LocalBindTransform);
    if (clip) SampleChannels(*skeleton, *clip, t, value);
    std::vector<glm::mat4> pose;
    if (!ComposeValues(*skeleton, value, pose)) return fallback();
    m_PoseMatrices = std::move(pose);
}

// ---- pose space ----
void AnimationPose::Resize(size_t boneCount) {
    m_Translations.resize(boneCount, glm::vec3(0.0f));
    m_Rotations.resize(boneCount, glm::quat(1.0f, 0.0f, 0.0f, 0.0f));
    m_Scales.resize(boneCount, glm::vec3(1.0f));
}

void AnimationMask::Resize(size_t boneCount) { m_BoneWeights.resize(boneCount, 1.0f); }

float AnimationMask::GetWeight(size_t boneIndex) const {
    return boneIndex >= m_BoneWeights.size() ? 1.0f : m_BoneWeights[boneIndex];
}

namespace {

AnimationPose PoseOfValues(const std::vector<TransformDecomposition>& value) {
    AnimationPose pose;
    pose.Resize(value.size());
    for (size_t b = 0; b < value.size(); ++b) {
        pose.m_Translations[b] = value[b].m_Translation;
        pose.m_Rotations[b] = value[b].m_Rotation;
        pose.m_Scales[b] = value[b].m_Scale;
    }
    return pose;
}

std::vector<TransformDecomposition> RestValues(const Skeleton& skeleton) {
    std::vector<TransformDecomposition> value(skeleton.m_Bones.size());
    for (size_t b = 0; b < value.size(); ++b) value[b] = DecomposeBindTransform(skeleton.m_Bones[b].m_LocalBindTransform);
    return value;
}

}  // namespace

AnimationPose AnimationPoseUtilities::BuildRestPose(const Skeleton& skeleton) { return PoseOfValues(RestValues(skeleton)); }

AnimationPose AnimationPoseUtilities::SampleClipPose(const Skeleton& skeleton, const AnimationClip& clip, float sampleTimeSeconds) {
    std::vector<TransformDecomposition> value = RestValues(skeleton);
    SampleChannels(skeleton, clip, sampleTimeSeconds, value);
    return PoseOfValues(value);
}

void AnimationPoseUtilities::BlendPose(AnimationPose& base, const AnimationPose& target, float blendWeight, const AnimationMask* mask) {
    const float W = Clamp01(blendWeight);
    const size_t count = std::min(base.m_Translations.size(), target.m_Translations.size());
    for (size_t b = 0; b < count; ++b) {
        const float m = mask ? mask->GetWeight(b) : 1.0f;
        const float F = Clamp01(W * m);
        base.m_Translations[b] = Mix3(base.m_Translations[b], target.m_Translations[b], F);
        base.m_Scales[b] = Mix3(base.m_Scales[b], target.m_Scales[b], F);
        base.m_Rotations[b] = glm::normalize(Slerp(base.m_Rotations[b], target.m_Rotations[b], F));
    }
}

void AnimationPoseUtilities::AdditivePose(AnimationPose& base, const AnimationPose& add, float additiveWeight, const AnimationMask* mask) {
    const size_t count = std::min(base.m_Translations.size(), add.m_Translations.size());
    for (size_t b = 0; b < count; ++b) {
        const float m = mask ? mask->GetWeight(b) : 1.0f;
        const float F = additiveWeight * m;
        const glm::vec3 &T = base.m_Translations[b], &S = base.m_Scales[b], &aT = add.m_Translations[b], &aS = add.m_Scales[b];
        base.m_Translations[b] = glm::vec3(T.x + aT.x * F, T.y + aT.y * F, T.z + aT.z * F);
        base.m_Scales[b] = glm::vec3(S.x + aS.x * F, S.y + aS.y * F, S.z + aS.z * F);
        const glm::quat target = QuatMul(base.m_Rotations[b], glm::normalize(add.m_Rotations[b]));
        base.m_Rotations[b] = glm::normalize(Slerp(base.m_Rotations[b], target, F));
    }
}

std::vector<glm::mat4> AnimationPoseUtilities::ComposeSkinningMatrices(const Skeleton& skeleton, const AnimationPose& pose) {
    std::vector<TransformDecomposition> value = RestValues(skeleton);
    const size_t have = std::min({value.size(), pose.m_Translations.size(), pose.m_Rotations.size(), pose.m_Scales.size()});
    for (size_t b = 0; b < have; ++b) {
        value[b].m_Translation = pose.m_Translations[b];
        value[b].m_Rotation = pose.m_Rotations[b];
        value[b].m_Scale = pose.m_Scales[b];
    }
    std::vector<glm::mat4> out;
    if (!ComposeValues(skeleton, value, out)) out.assign(skeleton.m_Bones.size(), glm::mat4(1.0f));
    return out;
}

// ---- pose programs ----
bool PoseProgram::WellFormed() const {
    size_t depth = 0;
    for (const PoseOp& op : m_Ops) {
        if (op.m_Op == PoseOp::Rest || op.m_Op == PoseOp::Clip) ++depth;
        else if (op.m_Op == PoseOp::Blend || op.m_Op == PoseOp::Add) {
            if (depth < 2) return false;
            --depth;
        } else return false;
    }
    return depth == 1;
}

bool PoseProgram::FitsDevice() const {
    if (m_Ops.size() > s_MaxOps || !WellFormed()) return false;
    size_t depth = 0;
    for (const PoseOp& op : m_Ops) {
        if (op.m_Op == PoseOp::Rest || op.m_Op == PoseOp::Clip) {
            if (++depth > s_MaxStack) return false;
        } else --depth;
    }
    return true;
}

bool EvaluatePoseProgram(const Skeleton& skeleton, const std::vector<AnimationClip>* clips, const PoseProgram& program,
                         AnimationPose& outPose) {
    if (!program.WellFormed()) return false;
    for (const PoseOp& op : program.m_Ops) {
        if (op.m_Op == PoseOp::Clip && (!clips || op.m_A >= clips->size())) return false;
        if ((op.m_Op == PoseOp::Blend || op.m_Op == PoseOp::Add) && op.m_A != PoseOp::s_NoMask && op.m_A >= program.m_Masks.size())
            return false;
    }
    const AnimationPose rest = AnimationPoseUtilities::BuildRestPose(skeleton);
    std::vector<AnimationPose> stack;
    for (const PoseOp& op : program.m_Ops) {
        if (op.m_Op == PoseOp::Rest) stack.push_back(rest);
        else if (op.m_Op == PoseOp::Clip) stack.push_back(AnimationPoseUtilities::SampleClipPose(skeleton, (*clips)[op.m_A], op.m_F));
        else {
            const AnimationPose top = std::move(stack.back());
            stack.pop_back();
            const AnimationMask* mask = op.m_A == PoseOp::s_NoMask ? nullptr : &program.m_Masks[op.m_A];
            if (op.m_Op == PoseOp::Blend) AnimationPoseUtilities::BlendPose(stack.back(), top, op.m_F, mask);
            else AnimationPoseUtilities::AdditivePose(stack.back(), top, op.m_F, mask);
        }
    }
    outPose = std::move(stack.back());
    return true;
}

}  // namespace Animation
}  // namespace Trident
