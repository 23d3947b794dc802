// pose_eval.hip — skeletal poses evaluated on the device: the tri_animset store, k_pose and k_pose_graph (the pose rules
// are stated in include/tri_raster.h, "skeletal poses evaluated on the device"; this file restates them for the GPU).
// k_pose_graph (further down) puts a pose program per instance in front of k_pose's phases 2 and 3.
//
// k_pose: one 64-lane workgroup per instance, lanes striding over the skeleton's bones.
//   phase 1  per bone: the three tracks sampled (an upper-bound search over the track's key times, one dword a probe;
//            values are 16-B records), the local matrix into LDS
//   phase 2  the traversal's levels in order: every bone of a level multiplies its parent's global (LDS) by its local,
//            a barrier between levels (a workgroup is one wave: the barrier costs no wait on other waves)
//   phase 3  the two fix-ups and global * inverse_bind per bone, back into LDS; then the first min(bones, 128) matrices
//            leave as 16-B stores, consecutive lanes on consecutive addresses
// Every input was validated on the host when it was added (tri_animset_add_*) or posed (tri_pose_check): the kernel has
// no bounds branch for bad input. Built under the default HIPFLAGS: -ffp-contract=off, IEEE division and square root,
// sinf / acosf as the device library gives them.
#include "capi_util.h"
#include "raster_launch.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kPoseThreads = 64;
// floats between two matrices in LDS: 16 + one 16-B access width, so that lanes reading one column of consecutive
// bones with 16-B reads do not all start on the same banks
constexpr int kPoseLdsStride = 20;

struct PoseBoneDev {
    float4 t;  // translation xyz
    float4 r;  // rotation: x = w, y = x, z = y, w = z
    float4 s;  // scale xyz
    float ib[16];
    int32_t eval_parent;  // the traversal's parent: -1 for a start bone (identity), else the bone's parent
    uint32_t unreached;   // 1: the traversal does not reach the bone (global = local)
    uint32_t pad[2];
};
static_assert(sizeof(PoseBoneDev) == 128, "PoseBoneDev layout");

struct PoseSkelDev {
    uint32_t bone_first, bone_count;
    uint32_t order_first;  // into `order`: the reached bones sorted by depth
    uint32_t level_first;  // into `levels`: level_count + 1 offsets into this skeleton's order
    uint32_t level_count;
    uint32_t pad[3];
};

struct PoseClipDev {
    uint32_t skeleton;
    uint32_t track_first;  // into `tracks`: 3 per bone {translation, rotation, scale}, {first key, key count}
    float duration;
    uint32_t pad;
};

struct PoseQuat {
    float w, x, y, z;
};

__device__ __forceinline__ float pose_clamp01(float x) {
    const float lo = x < 0.0f ? 0.0f : x;
    return 1.0f < lo ? 1.0f : lo;
}

__device__ __forceinline__ float pose_qdot(const PoseQuat& a, const PoseQuat& b) {
    return (a.w * b.w + a.x * b.x) + (a.y * b.y + a.z * b.z);
}

__device__ __forceinline__ PoseQuat pose_qnormalize(const PoseQuat& q) {
    const float len = sqrtf(pose_qdot(q, q));
    if (len <= 0.0f) return {1.0f, 0.0f, 0.0f, 0.0f};
    const float o = 1.0f / len;
    return {q.w * o, q.x * o, q.y * o, q.z * o};
}

__device__ __forceinline__ PoseQuat pose_slerp(const PoseQuat& a, const PoseQuat& b, float T) {
    PoseQuat z = b;
    float c = pose_qdot(a, b);
    if (c < 0.0f) {
        z = {-b.w, -b.x, -b.y, -b.z};
        c = -c;
    }
    if (c > 1.0f - FLT_EPSILON) {
        const float u = 1.0f - T;
        return {a.w * u + z.w * T, a.x * u + z.x * T, a.y * u + z.y * T, a.z * u + z.z * T};
    }
    const float A = acosf(c);
    const float s0 = sinf((1.0f - T) * A), s1 = sinf(T * A), s2 = sinf(A);
    return {(s0 * a.w + s1 * z.w) / s2, (s0 * a.x + s1 * z.x) / s2, (s0 * a.y + s1 * z.y) / s2,
            (s0 * a.z + s1 * z.z) / s2};
}

// The key pair of a track with count >= 2 at a time t > time[0]: the first i with t < time[i + 1] (an upper-bound
// search: times are non-decreasing) and the interpolation factor; false when t is at or past the last key (or NaN).
__device__ __forceinline__ bool pose_find(const float* __restrict__ times, uint32_t count, float t, uint32_t& i, float& T) {
    uint32_t lo = 1, hi = count;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (times[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    if (lo == count) return false;
    i = lo - 1;
    const float a = times[i], d = times[lo] - a;
    T = pose_clamp01(d > FLT_EPSILON ? (t - a) / d : 0.0f);
    return true;
}

__device__ __forceinline__ float4 pose_sample_vec(const float* __restrict__ times, const float4* __restrict__ vals,
                                                  uint2 track, float t, float4 def) {
    if (track.y == 0) return def;
    times += track.x;
    vals += track.x;
    if (track.y == 1 || t <= times[0]) return vals[0];
    uint32_t i;
    float T;
    if (!pose_find(times, track.y, t, i, T)) return vals[track.y - 1];
    const float4 a = vals[i], b = vals[i + 1];
    const float u = 1.0f - T;
    return make_float4(a.x * u + b.x * T, a.y * u + b.y * T, a.z * u + b.z * T, 0.0f);
}

__device__ __forceinline__ PoseQuat pose_load_quat(const float4* __restrict__ p) {
    const float4 v = *p;
    return {v.x, v.y, v.z, v.w};
}

__device__ __forceinline__ PoseQuat pose_sample_quat(const float* __restrict__ times, const float4* __restrict__ vals,
                                                     uint2 track, float t, PoseQuat def) {
    if (track.y == 0) return def;
    times += track.x;
    vals += track.x;
    if (track.y == 1 || t <= times[0]) return pose_qnormalize(pose_load_quat(vals));
    uint32_t i;
    float T;
    if (!pose_find(times, track.y, t, i, T)) return pose_qnormalize(pose_load_quat(vals + track.y - 1));
    return pose_qnormalize(pose_slerp(pose_load_quat(vals + i), pose_load_quat(vals + i + 1), T));
}

// r = a * b, glm's order: column j = ((a0*b[j].x + a1*b[j].y) + a2*b[j].z) + a3*b[j].w
__device__ __forceinline__ void pose_mul(const float* a, const float* b, float* r) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            r[4 * j + i] = ((a[i] * b[4 * j] + a[4 + i] * b[4 * j + 1]) + a[8 + i] * b[4 * j + 2]) + a[12 + i] * b[4 * j + 3];
}

__device__ __forceinline__ void pose_lds_load(const float* s, float* m) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(s + 4 * j);
        m[4 * j] = v.x; m[4 * j + 1] = v.y; m[4 * j + 2] = v.z; m[4 * j + 3] = v.w;
    }
}

__device__ __forceinline__ void pose_lds_store(float* s, const float* m) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        *reinterpret_cast<float4*>(s + 4 * j) = make_float4(m[4 * j], m[4 * j + 1], m[4 * j + 2], m[4 * j + 3]);
}

// The local matrix of a bone's {T, R, S}: translate * toMat4(normalize(R)) * scale in the rules' closed form.
__device__ __forceinline__ void pose_local_matrix(const float4& T, const PoseQuat& R, const float4& S, float* m) {
    const PoseQuat q = pose_qnormalize(R);
    const float qxx = q.x * q.x, qyy = q.y * q.y, qzz = q.z * q.z;
    const float qxz = q.x * q.z, qxy = q.x * q.y, qyz = q.y * q.z;
    const float qwx = q.w * q.x, qwy = q.w * q.y, qwz = q.w * q.z;
    m[0] = (1.0f - 2.0f * (qyy + qzz)) * S.x; m[1] = (2.0f * (qxy + qwz)) * S.x; m[2] = (2.0f * (qxz - qwy)) * S.x;
    m[3] = 0.0f;
    m[4] = (2.0f * (qxy - qwz)) * S.y; m[5] = (1.0f - 2.0f * (qxx + qzz)) * S.y; m[6] = (2.0f * (qyz + qwx)) * S.y;
    m[7] = 0.0f;
    m[8] = (2.0f * (qxz + qwy)) * S.z; m[9] = (2.0f * (qyz - qwx)) * S.z; m[10] = (1.0f - 2.0f * (qxx + qyy)) * S.z;
    m[11] = 0.0f;
    m[12] = T.x; m[13] = T.y; m[14] = T.z; m[15] = 1.0f;
}

// Phases 2 and 3 and the store, for a workgroup whose local matrices are in s_local (a barrier behind them).
__device__ __forceinline__ void pose_hierarchy_store(float* s_local, float* s_global, const PoseSkelDev& sk,
                                                     const PoseBoneDev* sb, const uint32_t* order,
                                                     const uint32_t* levels, float* palette, uint32_t palette_offset) {
    const uint32_t nb = sk.bone_count;
    const uint32_t* __restrict__ so = order + sk.order_first;
    const uint32_t* __restrict__ sl = levels + sk.level_first;
    for (uint32_t l = 0; l < sk.level_count; ++l) {
        const uint32_t end = sl[l + 1];
        for (uint32_t k = sl[l] + threadIdx.x; k < end; k += kPoseThreads) {
            const uint32_t b = so[k];
            const int32_t parent = sb[b].eval_parent;
            float P[16] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
            float L[16], G[16];
            if (parent >= 0) pose_lds_load(s_global + parent * kPoseLdsStride, P);
            pose_lds_load(s_local + b * kPoseLdsStride, L);
            pose_mul(P, L, G);
            pose_lds_store(s_global + b * kPoseLdsStride, G);
        }
        __syncthreads();
    }

    for (uint32_t b = threadIdx.x; b < nb; b += kPoseThreads) {
        float L[16], G[16], M[16];
        pose_lds_load(s_local + b * kPoseLdsStride, L);
        bool use_local = sb[b].unreached != 0;
        if (!use_local) {
            pose_lds_load(s_global + b * kPoseLdsStride, G);
            bool ident = true;
#pragma unroll
            for (int i = 0; i < 16; ++i) ident = ident && G[i] == ((i % 5) == 0 ? 1.0f : 0.0f);
            use_local = ident;
        }
        if (use_local) {
#pragma unroll
            for (int i = 0; i < 16; ++i) G[i] = L[i];
        }
        pose_mul(G, sb[b].ib, M);
        pose_lds_store(s_local + b * kPoseLdsStride, M);  // the bone's own slot: no other lane reads it in this phase
    }
    __syncthreads();

    const uint32_t nout = nb < TRI_POSE_PALETTE_BONES ? nb : TRI_POSE_PALETTE_BONES;
    float4* __restrict__ out = reinterpret_cast<float4*>(palette) + 4ull * palette_offset;
    for (uint32_t k = threadIdx.x; k < 4 * nout; k += kPoseThreads)
        out[k] = *reinterpret_cast<const float4*>(s_local + (k >> 2) * kPoseLdsStride + 4 * (k & 3));
}

__global__ __launch_bounds__(kPoseThreads) void k_pose(
    const tri_pose_instance* __restrict__ instances, const PoseSkelDev* __restrict__ skels,
    const PoseClipDev* __restrict__ clips, const PoseBoneDev* __restrict__ bones, const uint2* __restrict__ tracks,
    const float* __restrict__ vtimes, const float4* __restrict__ vvals, const float* __restrict__ qtimes,
    const float4* __restrict__ qvals, const uint32_t* __restrict__ order, const uint32_t* __restrict__ levels,
    float* __restrict__ palette, uint32_t lds_bones) {
    extern __shared__ float4 s_pose[];  // lds_bones local matrices, then lds_bones globals (16-B aligned rows)
    float* s_local = reinterpret_cast<float*>(s_pose);
    float* s_global = s_local + (size_t)lds_bones * kPoseLdsStride;

    const tri_pose_instance inst = instances[blockIdx.x];
    const PoseSkelDev sk = skels[inst.skeleton];
    const uint32_t nb = sk.bone_count;
    const PoseBoneDev* __restrict__ sb = bones + sk.bone_first;
    const bool has_clip = inst.clip != TRI_POSE_BIND;
    const uint2* __restrict__ tr = has_clip ? tracks + clips[inst.clip].track_first : nullptr;
    const float t = inst.time;

    for (uint32_t b = threadIdx.x; b < nb; b += kPoseThreads) {
        float4 T = sb[b].t, S = sb[b].s;
        const float4 r = sb[b].r;
        PoseQuat R{r.x, r.y, r.z, r.w};
        if (has_clip) {
            T = pose_sample_vec(vtimes, vvals, tr[3 * b], t, T);
            R = pose_sample_quat(qtimes, qvals, tr[3 * b + 1], t, R);
            S = pose_sample_vec(vtimes, vvals, tr[3 * b + 2], t, S);
        }
        float m[16];
        pose_local_matrix(T, R, S, m);
        pose_lds_store(s_local + b * kPoseLdsStride, m);
    }
    __syncthreads();
    pose_hierarchy_store(s_local, s_global, sk, sb, order, levels, palette, inst.palette_offset);
}

// ---- k_pose_graph: a pose program per instance in front of the same phases 2 and 3 --------------------------------
// Phase 1 runs the instance's program for each of the lane's bones (b = lane, lane + 64, ...). The program is uniform
// across the workgroup: every lane executes the same op at the same time (the op records are read through scalar
// loads: their address depends on blockIdx and the loop counter alone), and only the track searches diverge. The top
// of the pose stack stays in registers; the TRI_POSE_STACK - 1 entries below it live in LDS, component-major, one
// dword per lane per row ((entry * 10 + component) * 64 + lane: consecutive lanes on consecutive banks, conflict-free
// for the 32-bit accesses used). They occupy the s_global half, idle until phase 2 (7 * 10 * 64 * 4 = 17920 B, under
// the 20 KiB of the 256-bone size group; the smaller groups size that half for it). No pose state is indexed
// dynamically in registers: nothing goes to scratch.
constexpr int kPoseStackRows = 10;  // T xyz, R wxyz, S xyz
constexpr int kPoseStackFloats = (TRI_POSE_STACK - 1) * kPoseStackRows * kPoseThreads;

struct PoseTRS {
    float4 T;
    PoseQuat R;
    float4 S;
};

__device__ __forceinline__ void pose_stack_store(float* s, const PoseTRS& p) {
    s[0 * kPoseThreads] = p.T.x; s[1 * kPoseThreads] = p.T.y; s[2 * kPoseThreads] = p.T.z;
    s[3 * kPoseThreads] = p.R.w; s[4 * kPoseThreads] = p.R.x; s[5 * kPoseThreads] = p.R.y; s[6 * kPoseThreads] = p.R.z;
    s[7 * kPoseThreads] = p.S.x; s[8 * kPoseThreads] = p.S.y; s[9 * kPoseThreads] = p.S.z;
}

__device__ __forceinline__ PoseTRS pose_stack_load(const float* s) {
    PoseTRS p;
    p.T = make_float4(s[0 * kPoseThreads], s[1 * kPoseThreads], s[2 * kPoseThreads], 0.0f);
    p.R = {s[3 * kPoseThreads], s[4 * kPoseThreads], s[5 * kPoseThreads], s[6 * kPoseThreads]};
    p.S = make_float4(s[7 * kPoseThreads], s[8 * kPoseThreads], s[9 * kPoseThreads], 0.0f);
    return p;
}

__device__ __forceinline__ float4 pose_mix3(const float4& a, const float4& b, float F) {
    const float u = 1.0f - F;
    return make_float4(a.x * u + b.x * F, a.y * u + b.y * F, a.z * u + b.z * F, 0.0f);
}

// glm's quaternion product, each line left to right
__device__ __forceinline__ PoseQuat pose_qmul(const PoseQuat& p, const PoseQuat& q) {
    return {((p.w * q.w - p.x * q.x) - p.y * q.y) - p.z * q.z, ((p.w * q.x + p.x * q.w) + p.y * q.z) - p.z * q.y,
            ((p.w * q.y + p.y * q.w) + p.z * q.x) - p.x * q.z, ((p.w * q.z + p.z * q.w) + p.x * q.y) - p.y * q.x};
}

__global__ __launch_bounds__(kPoseThreads) void k_pose_graph(
    const tri_pose_graph_instance* __restrict__ instances, const tri_pose_op* __restrict__ ops,
    const PoseSkelDev* __restrict__ skels, const PoseClipDev* __restrict__ clips, const PoseBoneDev* __restrict__ bones,
    const uint2* __restrict__ tracks, const float* __restrict__ vtimes, const float4* __restrict__ vvals,
    const float* __restrict__ qtimes, const float4* __restrict__ qvals, const uint32_t* __restrict__ order,
    const uint32_t* __restrict__ levels, const uint32_t* __restrict__ mask_first, const float* __restrict__ mask_weights,
    float* __restrict__ palette, uint32_t lds_bones) {
    extern __shared__ float4 s_pose[];  // lds_bones local matrices, then the larger of lds_bones globals and the stack
    float* s_local = reinterpret_cast<float*>(s_pose);
    float* s_global = s_local + (size_t)lds_bones * kPoseLdsStride;
    float* s_stack = s_global + threadIdx.x;

    const tri_pose_graph_instance inst = instances[blockIdx.x];
    const PoseSkelDev sk = skels[inst.skeleton];
    const uint32_t nb = sk.bone_count;
    const PoseBoneDev* __restrict__ sb = bones + sk.bone_first;
    const tri_pose_op* __restrict__ prog = ops + inst.op_first;

    // whole 64-bone rounds: a lane past the last bone runs the program on the last bone and stores nothing, so that
    // the op loop runs with every lane of the wave
    for (uint32_t base = 0; base < nb; base += kPoseThreads) {
        const uint32_t lane_bone = base + threadIdx.x;
        const uint32_t b = lane_bone < nb ? lane_bone : nb - 1;
        const float4 rr = sb[b].r;
        const PoseTRS rest{sb[b].t, PoseQuat{rr.x, rr.y, rr.z, rr.w}, sb[b].s};
        PoseTRS top = rest;
        uint32_t depth = 0;  // entries on the stack, the top included
        for (uint32_t i = 0; i < inst.op_count; ++i) {
            const tri_pose_op op = prog[i];
            if (op.op == TRI_POSE_OP_REST || op.op == TRI_POSE_OP_CLIP) {
                if (depth) pose_stack_store(s_stack + (depth - 1) * (kPoseStackRows * kPoseThreads), top);
                ++depth;
                top = rest;
                if (op.op == TRI_POSE_OP_CLIP) {
                    const uint2* __restrict__ tr = tracks + clips[op.a].track_first + 3 * b;
                    top.T = pose_sample_vec(vtimes, vvals, tr[0], op.f, rest.T);
                    top.R = pose_sample_quat(qtimes, qvals, tr[1], op.f, rest.R);
                    top.S = pose_sample_vec(vtimes, vvals, tr[2], op.f, rest.S);
                }
            } else {
                --depth;
                const PoseTRS base_pose = pose_stack_load(s_stack + (depth - 1) * (kPoseStackRows * kPoseThreads));
                const float m = op.a == TRI_POSE_NO_MASK ? 1.0f : mask_weights[mask_first[op.a] + b];
                if (op.op == TRI_POSE_OP_BLEND) {
                    const float F = pose_clamp01(pose_clamp01(op.f) * m);
                    top.T = pose_mix3(base_pose.T, top.T, F);
                    top.S = pose_mix3(base_pose.S, top.S, F);
                    top.R = pose_qnormalize(pose_slerp(base_pose.R, top.R, F));
                } else {
                    const float F = op.f * m;
                    top.T = make_float4(base_pose.T.x + top.T.x * F, base_pose.T.y + top.T.y * F,
                                        base_pose.T.z + top.T.z * F, 0.0f);
                    top.S = make_float4(base_pose.S.x + top.S.x * F, base_pose.S.y + top.S.y * F,
                                        base_pose.S.z + top.S.z * F, 0.0f);
                    const PoseQuat target = pose_qmul(base_pose.R, pose_qnormalize(top.R));
                    top.R = pose_qnormalize(pose_slerp(base_pose.R, target, F));
                }
            }
        }
        if (lane_bone < nb) {
            float m[16];
            pose_local_matrix(top.T, top.R, top.S, m);
            pose_lds_store(s_local + b * kPoseLdsStride, m);
        }
    }
    __syncthreads();  // the stack is dead from here: phase 2 writes the globals over it
    pose_hierarchy_store(s_local, s_global, sk, sb, order, levels, palette, inst.palette_offset);
}

// A host vector's device image: grown by doubling, the appended tail copied by sync().
struct DevArray {
    void* d = nullptr;
    size_t cap = 0, synced = 0;  // bytes
    hipError_t sync(const void* host, size_t bytes) {
        if (bytes > cap) {
            void* nd = nullptr;
            const size_t ncap = std::max<size_t>(std::max<size_t>(2 * cap, bytes), 256);
            hipError_t e = hipMalloc(&nd, ncap);
            if (e != hipSuccess) return e;
            if (d) (void)hipFree(d);
            d = nd;
            cap = ncap;
            synced = 0;
        }
        if (bytes > synced) {
            hipError_t e = hipMemcpy(static_cast<char*>(d) + synced, static_cast<const char*>(host) + synced, bytes - synced,
                                     hipMemcpyHostToDevice);
            if (e != hipSuccess) return e;
            synced = bytes;
        }
        return hipSuccess;
    }
};

}  // namespace

struct tri_animset {
    int device = 0;
    std::vector<PoseSkelDev> skels;
    std::vector<PoseClipDev> clips;
    std::vector<PoseBoneDev> bones;
    std::vector<uint2> tracks;
    std::vector<float> vtimes, qtimes;
    std::vector<float4> vvals, qvals;
    std::vector<uint32_t> order, levels;
    std::vector<uint32_t> mask_skeleton, mask_first;  // per mask: its skeleton, its first weight in mask_weights
    std::vector<float> mask_weights;                  // per mask, one weight per bone of its skeleton
    DevArray d_skels, d_clips, d_bones, d_tracks, d_vtimes, d_qtimes, d_vvals, d_qvals, d_order, d_levels, d_mask_first,
        d_mask_weights;
};

namespace {

// Bring the device images up to the host vectors. Kernels of earlier tri_pose_palette calls may still read an image
// that has to move: the device is drained first, and the copies complete before the call returns.
int animset_upload(tri_animset* s, const char* who) {
    hipError_t e = hipSetDevice(s->device);
    if (e != hipSuccess) return tri_hip_fail(e, who);
    if ((e = hipDeviceSynchronize()) != hipSuccess) return tri_hip_fail(e, who);
#define POSE_SYNC(arr, vec) \
    if ((e = s->arr.sync(s->vec.data(), s->vec.size() * sizeof(s->vec[0]))) != hipSuccess) return tri_hip_fail(e, who)
    POSE_SYNC(d_skels, skels); POSE_SYNC(d_clips, clips); POSE_SYNC(d_bones, bones); POSE_SYNC(d_tracks, tracks);
    POSE_SYNC(d_vtimes, vtimes); POSE_SYNC(d_qtimes, qtimes); POSE_SYNC(d_vvals, vvals); POSE_SYNC(d_qvals, qvals);
    POSE_SYNC(d_order, order); POSE_SYNC(d_levels, levels);
    POSE_SYNC(d_mask_first, mask_first); POSE_SYNC(d_mask_weights, mask_weights);
#undef POSE_SYNC
    if ((e = hipDeviceSynchronize()) != hipSuccess) return tri_hip_fail(e, who);
    return TRI_OK;
}

bool times_ok(const float* t, uint32_t first, uint32_t count) {
    for (uint32_t i = 0; i < count; ++i) {
        if (!std::isfinite(t[first + i])) return false;
        if (i && t[first + i] < t[first + i - 1]) return false;
    }
    return true;
}

}  // namespace

int tri_internal_animset_device(const tri_animset* s) { return s->device; }

int tri_pose_check(const tri_animset* s, const tri_pose_instance* inst, uint32_t count, uint32_t prefix,
                   uint32_t* extent, TriPoseScratch& scratch) {
    *extent = prefix;
    if (count > TRI_POSE_MAX_INSTANCES) return tri_internal_fail(TRI_E_INVALID, "tri_pose_palette: too many instances");
    scratch.spans.resize(count);
    scratch.bones.resize(count);
    for (uint32_t i = 0; i < count; ++i) {
        const tri_pose_instance& p = inst[i];
        if (p.skeleton >= s->skels.size()) return tri_internal_fail(TRI_E_INVALID, "tri_pose_palette: unknown skeleton");
        if (p.clip != TRI_POSE_BIND && (p.clip >= s->clips.size() || s->clips[p.clip].skeleton != p.skeleton))
            return tri_internal_fail(TRI_E_INVALID, "tri_pose_palette: unknown clip, or a clip of another skeleton");
        const uint32_t nb = s->skels[p.skeleton].bone_count;
        const uint32_t n = std::min<uint32_t>(nb, TRI_POSE_PALETTE_BONES);
        if (p.palette_offset < prefix) return tri_internal_fail(TRI_E_INVALID, "tri_pose_palette: an instance inside the uploaded prefix");
        if (p.palette_offset > TRI_POSE_MAX_PALETTE - n) return tri_internal_fail(TRI_E_INVALID, "tri_pose_palette: palette offset too large");
        scratch.spans[i] = {p.palette_offset, n};
        scratch.bones[i] = nb;
        *extent = std::max(*extent, p.palette_offset + n);
    }
    std::sort(scratch.spans.begin(), scratch.spans.end());
    for (uint32_t i = 1; i < count; ++i)
        if (scratch.spans[i - 1].first + scratch.spans[i - 1].second > scratch.spans[i].first)
            return tri_internal_fail(TRI_E_INVALID, "tri_pose_palette: two instances overlap");
    return TRI_OK;
}

int tri_pose_graph_check(const tri_animset* s, const tri_pose_graph_instance* inst, uint32_t count,
                         const tri_pose_op* ops, uint32_t op_count, uint32_t prefix, uint32_t* extent,
                         TriPoseScratch& scratch) {
    if (op_count > TRI_POSE_MAX_INSTANCES * TRI_POSE_MAX_OPS) return tri_internal_fail(TRI_E_INVALID, "tri_pose_graph: too many ops");
    // the palette side is tri_pose_check's: the same records with no clip
    scratch.plain.resize(count);
    for (uint32_t i = 0; i < count; ++i) scratch.plain[i] = {inst[i].skeleton, TRI_POSE_BIND, 0.0f, inst[i].palette_offset};
    if (const int rc = tri_pose_check(s, scratch.plain.data(), count, prefix, extent, scratch)) return rc;
    for (uint32_t i = 0; i < count; ++i) {
        const tri_pose_graph_instance& p = inst[i];
        if ((uint64_t)p.op_first + p.op_count > op_count) return tri_internal_fail(TRI_E_INVALID, "tri_pose_graph: an op range outside the ops");
        if (p.op_count < 1 || p.op_count > TRI_POSE_MAX_OPS) return tri_internal_fail(TRI_E_INVALID, "tri_pose_graph: a program without ops or with more than TRI_POSE_MAX_OPS");
        uint32_t depth = 0;
        for (uint32_t k = 0; k < p.op_count; ++k) {
            const tri_pose_op& op = ops[p.op_first + k];
            switch (op.op) {
                case TRI_POSE_OP_CLIP:
                    if (op.a >= s->clips.size() || s->clips[op.a].skeleton != p.skeleton)
                        return tri_internal_fail(TRI_E_INVALID, "tri_pose_graph: unknown clip, or a clip of another skeleton");
                    [[fallthrough]];
                case TRI_POSE_OP_REST:
                    if (++depth > TRI_POSE_STACK) return tri_internal_fail(TRI_E_INVALID, "tri_pose_graph: a program deeper than TRI_POSE_STACK");
                    break;
                case TRI_POSE_OP_BLEND:
                case TRI_POSE_OP_ADD:
                    if (op.a != TRI_POSE_NO_MASK && (op.a >= s->mask_first.size() || s->mask_skeleton[op.a] != p.skeleton))
                        return tri_internal_fail(TRI_E_INVALID, "tri_pose_graph: unknown mask, or a mask of another skeleton");
                    if (depth < 2) return tri_internal_fail(TRI_E_INVALID, "tri_pose_graph: a program pops an empty stack");
                    --depth;
                    break;
                default:
                    return tri_internal_fail(TRI_E_INVALID, "tri_pose_graph: unknown op");
            }
        }
        if (depth != 1) return tri_internal_fail(TRI_E_INVALID, "tri_pose_graph: a program does not end with one pose");
    }
    return TRI_OK;
}

hipError_t tri_launch_pose_graph(const tri_animset* s, const tri_pose_graph_instance* d_inst, const tri_pose_op* d_ops,
                                 uint32_t count, uint32_t max_bones, float* palette, hipStream_t stream) {
    if (!count) return hipSuccess;
    if (max_bones < 1) max_bones = 1;
    // the local matrices, then whichever is larger of the globals and the pose stack: at most 40 KiB (256 bones)
    const size_t second = std::max<size_t>((size_t)max_bones * kPoseLdsStride, kPoseStackFloats);
    const size_t lds = ((size_t)max_bones * kPoseLdsStride + second) * sizeof(float);
    hipLaunchKernelGGL(k_pose_graph, dim3(count), dim3(kPoseThreads), lds, stream, d_inst, d_ops,
                       static_cast<const PoseSkelDev*>(s->d_skels.d), static_cast<const PoseClipDev*>(s->d_clips.d),
                       static_cast<const PoseBoneDev*>(s->d_bones.d), static_cast<const uint2*>(s->d_tracks.d),
                       static_cast<const float*>(s->d_vtimes.d), static_cast<const float4*>(s->d_vvals.d),
                       static_cast<const float*>(s->d_qtimes.d), static_cast<const float4*>(s->d_qvals.d),
                       static_cast<const uint32_t*>(s->d_order.d), static_cast<const uint32_t*>(s->d_levels.d),
                       static_cast<const uint32_t*>(s->d_mask_first.d), static_cast<const float*>(s->d_mask_weights.d),
                       palette, max_bones);
    return hipGetLastError();
}

hipError_t tri_launch_pose(const tri_animset* s, const tri_pose_instance* d_inst, uint32_t count, uint32_t max_bones,
                           float* palette, hipStream_t stream) {
    if (!count) return hipSuccess;
    if (max_bones < 1) max_bones = 1;
    const size_t lds = 2ull * max_bones * kPoseLdsStride * sizeof(float);  // at most 40 KiB (256 bones)
    hipLaunchKernelGGL(k_pose, dim3(count), dim3(kPoseThreads), lds, stream, d_inst,
                       static_cast<const PoseSkelDev*>(s->d_skels.d), static_cast<const PoseClipDev*>(s->d_clips.d),
                       static_cast<const PoseBoneDev*>(s->d_bones.d), static_cast<const uint2*>(s->d_tracks.d),
                       static_cast<const float*>(s->d_vtimes.d), static_cast<const float4*>(s->d_vvals.d),
                       static_cast<const float*>(s->d_qtimes.d), static_cast<const float4*>(s->d_qvals.d),
                       static_cast<const uint32_t*>(s->d_order.d), static_cast<const uint32_t*>(s->d_levels.d), palette,
                       max_bones);
    return hipGetLastError();
}

extern "C" {

int tri_animset_create(int32_t device, tri_animset** out) {
    if (!out) return tri_internal_fail(TRI_E_INVALID, "tri_animset_create: null argument");
    *out = nullptr;
    int dev = 0;
    if (const int rc = tri_resolve_device(device, "tri_animset_create", &dev)) return rc;
    tri_animset* s = new tri_animset();
    s->device = dev;
    *out = s;
    return TRI_OK;
}

int tri_animset_destroy(tri_animset* s) {
    if (!s) return TRI_OK;
    (void)hipSetDevice(s->device);
    for (DevArray* a : {&s->d_skels, &s->d_clips, &s->d_bones, &s->d_tracks, &s->d_vtimes, &s->d_qtimes, &s->d_vvals,
                        &s->d_qvals, &s->d_order, &s->d_levels, &s->d_mask_first, &s->d_mask_weights})
        if (a->d) (void)hipFree(a->d);
    delete s;
    return TRI_OK;
}

int tri_animset_add_skeleton(tri_animset* s, const tri_pose_bone* in, uint32_t n, int32_t root, uint32_t* out) {
    if (!s || !in || !out) return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_skeleton: null argument");
    if (n < 1 || n > TRI_POSE_MAX_BONES) return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_skeleton: bone count outside 1..TRI_POSE_MAX_BONES");
    for (uint32_t b = 0; b < n; ++b)
        if (in[b].parent >= (int32_t)n) return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_skeleton: a parent index beyond the bones");
    // the traversal (AnimationPlayer.cpp:209-266), breadth first: depth, the parent used, what it never reaches
    std::vector<int32_t> eval_parent(n, -1);
    std::vector<uint8_t> seen(n, 0);
    std::vector<uint32_t> queue, depth(n, 0);
    queue.reserve(n);
    auto start = [&](uint32_t b) { seen[b] = 1; queue.push_back(b); };
    if (root >= 0 && (uint32_t)root < n) start((uint32_t)root);
    else {
        for (uint32_t b = 0; b < n; ++b)
            if (in[b].parent < 0) start(b);
        if (queue.empty()) start(0);
    }
    for (size_t q = 0; q < queue.size(); ++q) {
        const uint32_t b = queue[q];
        for (uint32_t c = 0; c < n; ++c) {
            if (in[c].parent != (int32_t)b) continue;
            if (seen[c]) return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_skeleton: the parents form a cycle the traversal would reach");
            seen[c] = 1;
            eval_parent[c] = (int32_t)b;
            depth[c] = depth[b] + 1;
            queue.push_back(c);
        }
    }
    if (s->skels.size() >= (1u << 20) || s->bones.size() + n > (1u << 28)) return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_skeleton: the set is full");

    PoseSkelDev sk{};
    sk.bone_first = (uint32_t)s->bones.size();
    sk.bone_count = n;
    sk.order_first = (uint32_t)s->order.size();
    sk.level_first = (uint32_t)s->levels.size();
    sk.level_count = depth[queue.back()] + 1;  // breadth first: the queue is sorted by depth
    for (uint32_t b = 0; b < n; ++b) {
        PoseBoneDev d{};
        d.t = make_float4(in[b].translation[0], in[b].translation[1], in[b].translation[2], 0.0f);
        d.r = make_float4(in[b].rotation[0], in[b].rotation[1], in[b].rotation[2], in[b].rotation[3]);
        d.s = make_float4(in[b].scale[0], in[b].scale[1], in[b].scale[2], 0.0f);
        std::memcpy(d.ib, in[b].inverse_bind, sizeof d.ib);
        d.eval_parent = eval_parent[b];
        d.unreached = seen[b] ? 0u : 1u;
        s->bones.push_back(d);
    }
    uint32_t level = 0;
    s->levels.push_back(0);
    for (size_t q = 0; q < queue.size(); ++q) {
        for (; level < depth[queue[q]]; ++level) s->levels.push_back((uint32_t)q);
        s->order.push_back(queue[q]);
    }
    s->levels.push_back((uint32_t)queue.size());
    s->skels.push_back(sk);
    const int rc = animset_upload(s, "tri_animset_add_skeleton");
    if (rc) return rc;
    *out = (uint32_t)s->skels.size() - 1;
    return TRI_OK;
}

int tri_animset_add_clip(tri_animset* s, uint32_t skeleton, const tri_pose_channel* ch, uint32_t nch, const float* vt,
                         const float* vv, uint32_t nv, const float* qt, const float* qv, uint32_t nq, float duration,
                         uint32_t* out) {
    if (!s || !out || (nch && !ch) || (nv && (!vt || !vv)) || (nq && (!qt || !qv)))
        return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_clip: null argument");
    if (skeleton >= s->skels.size()) return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_clip: unknown skeleton");
    if (!std::isfinite(duration)) return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_clip: duration not finite");
    const uint32_t nb = s->skels[skeleton].bone_count;
    if (s->vtimes.size() + (size_t)nv > (1u << 30) || s->qtimes.size() + (size_t)nq > (1u << 30) ||
        s->tracks.size() + 3ull * nb > (1u << 30))
        return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_clip: the set is full");
    const uint32_t vbase = (uint32_t)s->vtimes.size(), qbase = (uint32_t)s->qtimes.size();
    std::vector<uint2> tracks(3 * (size_t)nb, make_uint2(0, 0));
    for (uint32_t c = 0; c < nch; ++c) {
        if (ch[c].bone >= nb) return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_clip: a channel's bone beyond the skeleton");
        const uint32_t first[3] = {ch[c].translation_first, ch[c].rotation_first, ch[c].scale_first};
        const uint32_t count[3] = {ch[c].translation_count, ch[c].rotation_count, ch[c].scale_count};
        for (int k = 0; k < 3; ++k) {
            if (!count[k]) continue;  // a track without keys leaves the bone's value
            const bool quat = k == 1;
            if ((uint64_t)first[k] + count[k] > (quat ? nq : nv))
                return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_clip: a key range outside the key arrays");
            if (!times_ok(quat ? qt : vt, first[k], count[k]))
                return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_clip: key times not finite or decreasing");
            tracks[3 * (size_t)ch[c].bone + k] = make_uint2((quat ? qbase : vbase) + first[k], count[k]);  // the last channel wins
        }
    }
    PoseClipDev cl{};
    cl.skeleton = skeleton;
    cl.track_first = (uint32_t)s->tracks.size();
    cl.duration = duration;
    s->tracks.insert(s->tracks.end(), tracks.begin(), tracks.end());
    for (uint32_t i = 0; i < nv; ++i) {
        s->vtimes.push_back(vt[i]);
        s->vvals.push_back(make_float4(vv[3 * (size_t)i], vv[3 * (size_t)i + 1], vv[3 * (size_t)i + 2], 0.0f));
    }
    for (uint32_t i = 0; i < nq; ++i) {
        s->qtimes.push_back(qt[i]);
        s->qvals.push_back(make_float4(qv[4 * (size_t)i], qv[4 * (size_t)i + 1], qv[4 * (size_t)i + 2], qv[4 * (size_t)i + 3]));
    }
    s->clips.push_back(cl);
    const int rc = animset_upload(s, "tri_animset_add_clip");
    if (rc) return rc;
    *out = (uint32_t)s->clips.size() - 1;
    return TRI_OK;
}

int tri_animset_add_mask(tri_animset* s, uint32_t skeleton, const float* weights, uint32_t count, uint32_t* out) {
    if (!s || !out || (count && !weights)) return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_mask: null argument");
    if (skeleton >= s->skels.size()) return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_mask: unknown skeleton");
    const uint32_t nb = s->skels[skeleton].bone_count;
    if (s->mask_first.size() >= (1u << 24) || s->mask_weights.size() + (size_t)nb > (1u << 30))
        return tri_internal_fail(TRI_E_INVALID, "tri_animset_add_mask: the set is full");
    s->mask_skeleton.push_back(skeleton);
    s->mask_first.push_back((uint32_t)s->mask_weights.size());
    for (uint32_t b = 0; b < nb; ++b) s->mask_weights.push_back(b < count ? weights[b] : 1.0f);  // AnimationMask::GetWeight
    const int rc = animset_upload(s, "tri_animset_add_mask");
    if (rc) return rc;
    *out = (uint32_t)s->mask_first.size() - 1;
    return TRI_OK;
}

}  // extern "C"
