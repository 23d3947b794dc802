// anim_check.cpp — the glTF skin / animation reader over the fixture rig (argv[1]: tests/golden/anim/rig.gltf) and
// damaged copies of it (truncated buffers and files, joint indices beyond the skin, accessor counts that disagree, a
// node cycle, corrupted payload bytes), and the asset service, the channel resolution and the CPU player over a good
// rig and damaged ones (a parent cycle, parents and channel bones out of range, NaN and decreasing key times,
// zero-length quaternions, a 300-bone skeleton, an empty one), built with the address and undefined-behaviour
// sanitizers (`make anim-check`):
// nothing may crash or read out of bounds, every pose is finite or the stated fallback, and what the device path
// would refuse is reported as such. CPU only; never loaded into Python.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <sstream>

#include "trident/Animation.h"
#include "trident/ModelLoader.h"

using namespace Trident::Animation;

namespace {

int g_failures = 0;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                               \
        }                                                                               \
    } while (0)

glm::mat4 Translation(float x, float y, float z) { return glm::translate(glm::mat4(1.0f), glm::vec3(x, y, z)); }

Skeleton Chain(size_t n) {
    Skeleton sk;
    sk.m_Bones.resize(n);
    for (size_t b = 0; b < n; ++b) {
        sk.m_Bones[b].m_SourceName = (b == 1 ? "mixamorig:" : "") + std::string("Bone") + std::to_string(b);
        sk.m_Bones[b].m_ParentIndex = (int)b - 1;
        sk.m_Bones[b].m_LocalBindTransform = Translation(0.0f, 0.01f, 0.0f);
    }
    FinaliseSkeleton(sk);
    return sk;
}

AnimationClip Clip(const std::string& name, int bone, const std::string& source, std::vector<float> times) {
    AnimationClip clip;
    clip.m_Name = name;
    clip.m_DurationSeconds = 1.0f;
    TransformChannel ch;
    ch.m_BoneIndex = bone;
    ch.m_SourceBoneName = source;
    for (size_t i = 0; i < times.size(); ++i) {
        ch.m_TranslationKeys.push_back({times[i], glm::vec3((float)i, 0.0f, 0.0f)});
        ch.m_RotationKeys.push_back({times[i], i % 2 ? glm::quat(0.0f, 0.0f, 0.0f, 0.0f) : glm::quat(0.5f, 0.5f, -0.5f, 0.5f)});
        ch.m_ScaleKeys.push_back({times[i], glm::vec3(1.0f)});
    }
    clip.m_Channels.push_back(ch);
    return clip;
}

bool Finite(const std::vector<glm::mat4>& pose) {
    for (const glm::mat4& m : pose)
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 4; ++r)
                if (!std::isfinite(m[c][r])) return false;
    return true;
}

bool AllIdentity(const std::vector<glm::mat4>& pose) {
    for (const glm::mat4& m : pose)
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 4; ++r)
                if (m[c][r] != (c == r ? 1.0f : 0.0f)) return false;
    return true;
}

// every clip of the asset at a spread of times (NaN and infinities included); returns the last pose
std::vector<glm::mat4> Play(size_t handle, size_t clips, bool expectFinite) {
    AnimationAssetService& service = AnimationAssetService::Get();
    AnimationPlayer player(service);
    player.SetSkeletonHandle(handle);
    player.SetAnimationHandle(handle);
    std::vector<glm::mat4> pose;
    const float inf = std::numeric_limits<float>::infinity();
    for (size_t c = 0; c <= clips; ++c) {  // (one past the end: no clip, the bind pose)
        player.SetClipIndex(c);
        for (float t : {-1.0f, 0.0f, 0.25f, 0.5f, 0.75f, 1.0f, 2.0f, inf, -inf, std::nanf("")}) {
            player.EvaluateAt(t);
            player.CopyPoseTo(pose);
            CHECK(!pose.empty());
            if (expectFinite) CHECK(Finite(pose));
        }
        player.SetCurrentTime(0.9f);
        player.SetPlaybackSpeed(-3.0f);
        player.Update(0.5f);
        CHECK(std::isfinite(player.GetCurrentTime()));
    }
    return pose;
}

// One copy of the fixture with `text` as its content: loaded, and played when it yields an asset. Returns the bones.
size_t LoadVariant(const std::filesystem::path& dir, const std::string& name, const std::string& text) {
    const std::filesystem::path file = dir / (name + ".gltf");
    std::ofstream(file, std::ios::binary) << text;
    Trident::Loader::ModelData model = Trident::Loader::ModelLoader::Load(file.string());
    const size_t bones = model.m_Skeleton.m_Bones.size(), clips = model.m_AnimationClips.size();
    for (const auto& mesh : model.m_Meshes)
        for (const Vertex& v : mesh.Vertices)
            for (int k = 0; k < 4; ++k) CHECK((&v.m_BoneIndices.x)[k] >= 0 && (size_t)(&v.m_BoneIndices.x)[k] < std::max<size_t>(bones, 1));
    if (bones || clips) {
        const size_t h = AnimationAssetService::Get().RegisterRuntimeAsset("check:" + name, std::move(model.m_Skeleton),
                                                                            std::move(model.m_AnimationClips));
        Play(h, clips, false);
    }
    return bones;
}

void CheckGltf(const std::string& rigPath) {
    std::ifstream in(rigPath, std::ios::binary);
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string good = ss.str();
    CHECK(!good.empty());
    const std::filesystem::path dir = std::filesystem::temp_directory_path() / ("anim_check_" + std::to_string((long)std::rand()));
    std::filesystem::create_directories(dir);
    CHECK(LoadVariant(dir, "good", good) == 7);
    const size_t payload = good.find("base64,") + 7, payloadEnd = good.find('"', payload);
    CHECK(payload != std::string::npos + 7 && payloadEnd != std::string::npos);
    int variant = 0;
    auto name = [&]() { return "v" + std::to_string(variant++); };
    // a truncated buffer, a truncated file
    CHECK(LoadVariant(dir, name(), good.substr(0, payload + (payloadEnd - payload) / 2) + good.substr(payloadEnd)) == 0);
    CHECK(LoadVariant(dir, name(), good.substr(0, good.size() / 2)) == 0);
    // every accessor count, one at a time: larger than its data, zero, one short
    for (size_t at = good.find("\"count\":"); at != std::string::npos; at = good.find("\"count\":", at + 1)) {
        const size_t digits = at + 8;
        size_t end = digits;
        while (end < good.size() && std::isdigit((unsigned char)good[end])) ++end;
        const long n = std::atol(good.substr(digits, end - digits).c_str());
        for (long other : {n + 7, 0L, n - 1, 100000000L})
            if (other >= 0) LoadVariant(dir, name(), good.substr(0, digits) + std::to_string(other) + good.substr(end));
    }
    // a joint that is no node, a joint index beyond the skin (every payload byte position in turn gets all ones in a
    // sample of places: joints, weights, key times and matrices become huge or NaN), a node that is its own ancestor
    size_t joints = good.find("\"joints\":[");
    CHECK(joints != std::string::npos);
    CHECK(LoadVariant(dir, name(), good.substr(0, joints + 10) + "500," + good.substr(joints + 10)) == 0);
    for (size_t at = payload; at + 4 < payloadEnd; at += 37) {
        std::string bad = good;
        bad[at] = bad[at + 1] = bad[at + 2] = bad[at + 3] = '/';
        LoadVariant(dir, name(), bad);
    }
    const size_t kids = good.find("\"children\":[");
    CHECK(kids != std::string::npos);
    LoadVariant(dir, name(), good.substr(0, kids + 12) + "0,4," + good.substr(kids + 12));
    std::filesystem::remove_all(dir);
}

}  // namespace

int main(int argc, char** argv) {
    AnimationAssetService& service = AnimationAssetService::Get();
    if (argc > 1) CheckGltf(argv[1]);
    else {
        std::fprintf(stderr, "usage: anim_check <rig.gltf>\n");
        return 2;
    }

    {  // a good rig: by index, by source name, by stripped prefix, and a channel that maps to nothing
        Skeleton sk = Chain(5);
        std::vector<AnimationClip> clips = {Clip("index", 2, "", {0.0f, 0.5f, 0.5f, 1.0f}), Clip("source", 0, "Bone3", {0.0f, 1.0f}),
                                            Clip("prefix", 9, "Bone1", {0.25f}), Clip("stale", 7, "Tail", {0.0f, 1.0f})};
        CHECK(DevicePoseCompatible(sk, &clips));
        CHECK(ResolveChannelBoneIndex(clips[0].m_Channels[0], sk, "index") == 2);
        CHECK(ResolveChannelBoneIndex(clips[1].m_Channels[0], sk, "source") == 3);
        CHECK(ResolveChannelBoneIndex(clips[2].m_Channels[0], sk, "prefix") == 1);
        CHECK(ResolveChannelBoneIndex(clips[3].m_Channels[0], sk, "stale") == -1);
        const size_t h = service.RegisterRuntimeAsset("check:good", sk, clips);
        CHECK(h != AnimationAssetService::s_InvalidHandle);
        CHECK(service.ResolveClipIndex(h, "prefix") == 2 && service.ResolveClipIndex(h, "absent") == AnimationAssetService::s_InvalidHandle);
        CHECK(Play(h, clips.size(), true).size() == 5);
    }
    {  // a parent cycle the traversal reaches: refused, the fallback pose
        Skeleton sk = Chain(4);
        sk.m_Bones[0].m_ParentIndex = 3;
        sk.m_RootBoneIndex = 0;
        FinaliseSkeleton(sk);
        CHECK(!DevicePoseCompatible(sk, nullptr));
        const size_t h = service.RegisterRuntimeAsset("check:cycle", sk, {});
        CHECK(AllIdentity(Play(h, 0, true)));
    }
    {  // parents and a root out of range, a channel bone far out of range
        Skeleton sk = Chain(3);
        sk.m_Bones[1].m_ParentIndex = 99;
        sk.m_Bones[2].m_ParentIndex = -7;
        sk.m_RootBoneIndex = 1000;
        FinaliseSkeleton(sk);
        std::vector<AnimationClip> clips = {Clip("far", 1 << 30, "", {0.0f, 1.0f}), Clip("negative", -5, "", {0.0f, 1.0f})};
        CHECK(!DevicePoseCompatible(sk, &clips));
        const size_t h = service.RegisterRuntimeAsset("check:range", sk, clips);
        CHECK(Play(h, clips.size(), true).size() == 3);
    }
    {  // NaN, infinite and decreasing key times: the CPU plays them (the linear scan), the device path refuses them
        Skeleton sk = Chain(2);
        const float inf = std::numeric_limits<float>::infinity();
        std::vector<AnimationClip> clips = {Clip("nan", 0, "", {0.0f, std::nanf(""), 1.0f}), Clip("back", 1, "", {0.5f, 0.25f, 0.75f}),
                                            Clip("inf", 1, "", {-inf, 0.0f, inf})};
        for (const AnimationClip& clip : clips) {
            std::vector<AnimationClip> one = {clip};
            CHECK(!DevicePoseCompatible(sk, &one));
        }
        const size_t h = service.RegisterRuntimeAsset("check:times", sk, clips);
        CHECK(Play(h, clips.size(), false).size() == 2);  // (infinite key times give non-finite weights: no crash is the check)
    }
    {  // zero-length quaternions everywhere, a zero bind matrix
        Skeleton sk = Chain(2);
        sk.m_Bones[1].m_LocalBindTransform = glm::mat4(0.0f);
        AnimationClip clip = Clip("zero", 0, "", {0.0f, 0.5f, 1.0f});
        for (QuaternionKeyframe& k : clip.m_Channels[0].m_RotationKeys) k.m_Value = glm::quat(0.0f, 0.0f, 0.0f, 0.0f);
        const size_t h = service.RegisterRuntimeAsset("check:zero", sk, {clip});
        CHECK(Play(h, 1, true).size() == 2);
    }
    {  // 300 bones: beyond the device limit, fine on the CPU
        Skeleton sk = Chain(300);
        CHECK(!DevicePoseCompatible(sk, nullptr));
        CHECK(DevicePoseCompatible(Chain(256), nullptr));
        const size_t h = service.RegisterRuntimeAsset("check:300", sk, {Clip("c", 299, "", {0.0f, 1.0f})});
        CHECK(Play(h, 1, true).size() == 300);
    }
    {  // nothing there: the fallback pose, one identity
        const size_t h = service.RegisterRuntimeAsset("check:empty", Skeleton{}, {});
        CHECK(!DevicePoseCompatible(Skeleton{}, nullptr));
        const std::vector<glm::mat4> pose = Play(h, 0, true);
        CHECK(pose.size() == 1 && AllIdentity(pose));
        CHECK(service.RegisterRuntimeAsset("", Skeleton{}, {}) == AnimationAssetService::s_InvalidHandle);
        CHECK(Play(AnimationAssetService::s_InvalidHandle, 0, true).size() == 1);
    }
    if (g_failures) {
        std::fprintf(stderr, "anim_check: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("anim_check ok\n");
    return 0;
}
