// anim_graph_check — the animation state machine, the blend-tree nodes and the CPU pose-program interpreter driven over
// degenerate input under the address and undefined-behaviour sanitizers (make anim-graph-check). Host only: it links
// Animation.cpp and AnimationStateMachine.cpp and nothing of the renderer.
#include <cmath>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <vector>

#include "trident/AnimationStateMachine.h"

using namespace Trident::Animation;

namespace {

int g_failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                  \
        }                                                                  \
    } while (0)

Skeleton MakeSkeleton(int bones) {
    Skeleton sk;
    for (int b = 0; b < bones; ++b) {
        Bone bone;
        bone.m_SourceName = "bone" + std::to_string(b);
        bone.m_ParentIndex = b - 1;
        bone.m_LocalBindTransform = glm::translate(glm::mat4(1.0f), glm::vec3(0.0f, 0.1f * (float)b, 0.0f));
        sk.m_Bones.push_back(bone);
    }
    FinaliseSkeleton(sk);
    return sk;
}

AnimationClip MakeClip(const char* name, float duration, int bone) {
    AnimationClip clip;
    clip.m_Name = name;
    clip.m_DurationSeconds = duration;
    TransformChannel ch;
    ch.m_BoneIndex = bone;
    ch.m_TranslationKeys = {{0.0f, glm::vec3(0.0f)}, {1.0f, glm::vec3(1.0f, 2.0f, 3.0f)}};
    ch.m_RotationKeys = {{0.0f, glm::quat(1.0f, 0.0f, 0.0f, 0.0f)}, {1.0f, glm::quat(0.0f, 1.0f, 0.0f, 0.0f)}};
    clip.m_Channels.push_back(ch);
    return clip;
}

bool Finite(const std::vector<glm::mat4>& m) {
    for (const glm::mat4& x : m)
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 4; ++r)
                if (!std::isfinite(x[c][r])) return false;
    return true;
}

PoseOp Op(uint32_t op, uint32_t a, float f) {
    PoseOp o;
    o.m_Op = op;
    o.m_A = a;
    o.m_F = f;
    return o;
}

}  // namespace

int main() {
    AnimationAssetService& service = AnimationAssetService::Get();
    const size_t asset = service.RegisterRuntimeAsset("check:rig", MakeSkeleton(5), {MakeClip("a", 1.0f, 1), MakeClip("b", 0.0f, 4),
                                                                                   MakeClip("c", 2.0f, 77)});
    const Skeleton* sk = service.GetSkeleton(asset);
    CHECK(sk && sk->m_Bones.size() == 5);
    std::vector<glm::mat4> pose;

    {  // no layers; a layer without an entry state; an entry state that does not exist
        AnimationStateMachine sm(service);
        sm.SetSkeletonHandle(asset);
        sm.SetAnimationLibraryHandle(asset);
        sm.Update(0.1f);
        sm.CopyPose(pose);
        CHECK(pose.size() == 5 && sm.GetProgram().m_Ops.size() == 1);
        const size_t layer = sm.AddLayer("empty", 1.0f, false);
        sm.Update(0.1f);
        sm.SetLayerEntryState(layer, "nowhere");
        sm.Update(0.1f);
        sm.SetLayerEntryState(99, "x");
        sm.SetLayerWeight(99, 1.0f);
        sm.SetLayerMask(99, AnimationMask{});
        CHECK(sm.GetProgram().m_Ops.size() == 3 && sm.GetLayer(layer)->m_CurrentState == nullptr);
        bool threw = false;
        try {
            sm.AddTransition(layer, "nowhere", AnimationTransition{});
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try {
            sm.AddState(7, "x", nullptr);
        } catch (const std::out_of_range&) {
            threw = true;
        }
        CHECK(threw);
    }

    {  // transitions to a missing state, blend nodes without children, an empty blend space, states without a root
        AnimationStateMachine sm(service);
        sm.SetSkeletonHandle(asset);
        sm.SetAnimationLibraryHandle(asset);
        const size_t layer = sm.AddLayer("base", 1.0f, false);
        sm.AddState(layer, "bare", std::make_unique<BlendNode>(nullptr, nullptr, 0.5f));
        sm.AddState(layer, "half", std::make_unique<BlendNode>(nullptr, std::make_unique<ClipNode>(0, true, 1.0f), 0.5f));
        sm.AddState(layer, "space", std::make_unique<BlendSpace1DNode>(std::vector<BlendSpace1DNode::Sample>{}, 0.0f));
        sm.AddState(layer, "rootless", nullptr);
        sm.AddState(layer, "missing", std::make_unique<ClipNode>(1234, false, -3.0f));
        sm.SetLayerEntryState(layer, "bare");
        sm.AddTriggerParameter("next");
        AnimationTransition t;
        t.m_Conditions.push_back({"next", AnimationConditionComparison::Triggered, 0.0f, 0, false});
        const char* chain[] = {"bare", "nowhere", "half", "space", "rootless", "missing", "bare"};
        for (int i = 0; i + 1 < 7; ++i) {
            if (std::string(chain[i]) == "nowhere") continue;
            t.m_TargetState = chain[i + 1];
            t.m_FadeDurationSeconds = i % 2 ? 0.0f : 0.05f;
            sm.AddTransition(layer, chain[i], t);
            if (std::string(chain[i + 1]) == "nowhere") {  // a second way out of the state whose first leads nowhere
                t.m_TargetState = chain[i + 2];
                sm.AddTransition(layer, chain[i], t);
            }
        }
        for (int i = 0; i < 40; ++i) {
            if (i % 3 == 0) sm.FireTrigger("next");
            sm.Update(0.02f);
            sm.CopyPose(pose);
            CHECK(pose.size() == 5 && Finite(pose));
            CHECK(sm.GetProgram().WellFormed());
        }
        sm.AddState(layer, "bare", nullptr);  // replacing the state a layer may be in
        sm.Update(0.02f);
        sm.Update(NAN);
        sm.Update(-1.0e30f);
    }

    {  // masks longer and shorter than the skeleton, a skeleton handle that becomes invalid between updates
        AnimationStateMachine sm(service);
        sm.SetSkeletonHandle(asset);
        sm.SetAnimationLibraryHandle(asset);
        const size_t layer = sm.AddLayer("base", 0.5f, true);
        sm.AddState(layer, "a", std::make_unique<ClipNode>(0, true, 1.0f));
        sm.SetLayerEntryState(layer, "a");
        AnimationMask longer, shorter;
        longer.m_BoneWeights.assign(40, 0.5f);
        shorter.m_BoneWeights.assign(2, 0.25f);
        sm.SetLayerMask(layer, longer);
        sm.Update(0.1f);
        CHECK(sm.GetProgram().m_Masks.size() == 1 && sm.GetProgram().m_Masks[0].m_BoneWeights.size() == 5);
        sm.SetLayerMask(layer, shorter);
        sm.Update(0.1f);
        CHECK(sm.GetProgram().m_Masks[0].m_BoneWeights.size() == 5 && sm.GetProgram().m_Masks[0].m_BoneWeights[4] == 1.0f);
        sm.CopyPose(pose);
        const std::vector<glm::mat4> before = pose;
        sm.SetSkeletonHandle(asset + 1000);  // no such asset
        sm.Update(0.1f);
        sm.Evaluate();
        sm.CopyPose(pose);
        CHECK(pose.size() == before.size());
        sm.SetSkeletonHandle(service.RegisterRuntimeAsset("check:small", MakeSkeleton(2), {}));  // another bone count, no clips
        sm.Update(0.1f);
        sm.CopyPose(pose);
        CHECK(pose.size() == 2 && Finite(pose));
        sm.SetSkeletonHandle(asset);
        sm.Update(0.1f);
        sm.CopyPose(pose);
        CHECK(pose.size() == 5);
    }

    {  // the interpreter: programs at both limits, beyond them, and malformed ones
        const std::vector<AnimationClip>* clips = service.GetAnimationClips(asset);
        PoseProgram p;
        AnimationPose out;
        AnimationMask shorter, longer;
        shorter.m_BoneWeights = {0.0f};
        longer.m_BoneWeights.assign(300, 2.0f);
        p.m_Masks = {shorter, longer};
        for (size_t i = 0; i < PoseProgram::s_MaxStack; ++i) p.m_Ops.push_back(Op(PoseOp::Clip, (uint32_t)(i % 3), 0.3f * (float)i));
        for (size_t i = 0; i + 1 < PoseProgram::s_MaxStack; ++i) p.m_Ops.push_back(Op(i % 2 ? PoseOp::Add : PoseOp::Blend, (uint32_t)(i % 2), 0.5f));
        CHECK(p.FitsDevice() && EvaluatePoseProgram(*sk, clips, p, out) && out.m_Translations.size() == 5);
        CHECK(Finite(AnimationPoseUtilities::ComposeSkinningMatrices(*sk, out)));
        p.m_Ops.insert(p.m_Ops.begin(), Op(PoseOp::Rest, 0, 0.0f));  // depth 9
        p.m_Ops.push_back(Op(PoseOp::Blend, PoseOp::s_NoMask, 2.0f));
        CHECK(p.WellFormed() && !p.FitsDevice() && EvaluatePoseProgram(*sk, clips, p, out));
        PoseProgram longest;
        longest.m_Ops.push_back(Op(PoseOp::Rest, 0, 0.0f));
        while (longest.m_Ops.size() + 2 <= PoseProgram::s_MaxOps) {
            longest.m_Ops.push_back(Op(PoseOp::Clip, 1, -5.0f));
            longest.m_Ops.push_back(Op(PoseOp::Add, PoseOp::s_NoMask, -0.25f));
        }
        CHECK(longest.m_Ops.size() == 63 && longest.FitsDevice() && EvaluatePoseProgram(*sk, clips, longest, out));
        longest.m_Ops.push_back(Op(PoseOp::Clip, 1, 0.0f));
        longest.m_Ops.push_back(Op(PoseOp::Blend, PoseOp::s_NoMask, NAN));
        CHECK(longest.WellFormed() && !longest.FitsDevice() && EvaluatePoseProgram(*sk, clips, longest, out));
        AnimationPoseUtilities::ComposeSkinningMatrices(*sk, out);
        for (const std::vector<PoseOp>& bad : {std::vector<PoseOp>{}, {Op(PoseOp::Blend, 0, 0.5f)}, {Op(PoseOp::Rest, 0, 0), Op(PoseOp::Rest, 0, 0)},
                                               {Op(9, 0, 0)}, {Op(PoseOp::Clip, 3, 0)},
                                               {Op(PoseOp::Rest, 0, 0), Op(PoseOp::Rest, 0, 0), Op(PoseOp::Add, 2, 1.0f)}}) {
            PoseProgram q;
            q.m_Ops = bad;
            q.m_Masks = p.m_Masks;
            CHECK(!EvaluatePoseProgram(*sk, clips, q, out));
        }
        PoseProgram noclips;
        noclips.m_Ops = {Op(PoseOp::Clip, 0, 0.0f)};
        CHECK(!EvaluatePoseProgram(*sk, nullptr, noclips, out));
        // poses of other sizes than the skeleton
        AnimationPose empty, big;
        big.Resize(9);
        AnimationPoseUtilities::BlendPose(out, empty, 0.5f, &shorter);
        AnimationPoseUtilities::AdditivePose(out, big, 0.5f, &longer);
        AnimationPoseUtilities::BlendPose(empty, out, 0.5f, nullptr);
        CHECK(AnimationPoseUtilities::ComposeSkinningMatrices(*sk, empty).size() == 5);
        CHECK(AnimationPoseUtilities::ComposeSkinningMatrices(*sk, big).size() == 5);
    }

    if (g_failures) {
        std::fprintf(stderr, "anim_graph_check: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("anim_graph_check: ok\n");
    return 0;
}
