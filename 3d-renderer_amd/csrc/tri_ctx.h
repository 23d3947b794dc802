// tri_ctx.h — the context, geometry and font objects behind the C-ABI handles, and the owning holders their members
// are made of. Internal to the units that implement the entry points over a context (tri_raster_capi.hip: lifecycle,
// frame and readback; tri_geometry.hip: geometry; tri_resources.hip: every other upload; tri_ids.hip: the entity-id
// entry points; tri_motion.hip: the motion-vector entry points) and to the objects that read a context's frame and keep
// state of their own between frames (tri_temporal.h: their shared core; tri_history.hip, tri_taa.hip, tri_upscale.hip);
// the other units keep to the accessors of capi_util.h.
//
// Ownership: a DevBuf, PinBuf, Event or Staged member frees what it holds when its object is deleted (with the
// object's device current), so a new buffer needs no line in tri_destroy. Raw pointers in these structs are borrowed:
// d_color / d_depth (the context's own targets, or the caller's through tri_bind_output) and geom.
#pragma once

#include "capi_util.h"
#include "frame_select.h"
#include "raster_launch.h"

#include <cstdarg>
#include <cstdio>
#include <utility>
#include <vector>

// Record a formatted message for tri_last_error (returns `code`).
inline int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return tri_internal_fail(code, buf);
}

// Whether a 16-B vector access may start at p (the choice between a kernel's vector and scalar variants).
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Device memory: count elements of T. grow() frees and allocates (the contents are not kept).
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int grow(size_t need) {
        if (need <= cap && p) return TRI_OK;
        if (p) TRI_HIP_TRY(hipFree(p));
        p = nullptr;
        cap = std::max<size_t>(need, 1);
        TRI_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), cap * sizeof(T)));
        return TRI_OK;
    }
    // Free the memory now (nothing queued may still use it); the buffer is empty again.
    int release() {
        T* q = p;
        p = nullptr;
        cap = 0;
        if (q) TRI_HIP_TRY(hipFree(q));
        return TRI_OK;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

// Pinned host memory, likewise.
template <typename T>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    int grow(size_t need) {
        if (need <= cap && p) return TRI_OK;
        if (p) TRI_HIP_TRY(hipHostFree(p));
        p = nullptr;
        cap = std::max<size_t>(need, 1);
        TRI_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p), cap * sizeof(T), hipHostMallocDefault));
        return TRI_OK;
    }
    operator T*() const { return p; }
};

// An event, created at its first use.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    int ensure(unsigned flags) {
        if (!e) TRI_HIP_TRY(hipEventCreateWithFlags(&e, flags));
        return TRI_OK;
    }
};

// Upload staging: a pinned buffer, a device twin where the copy's destination is the stage's own, and the event
// behind the last copy out of the pinned buffer (or the last kernel that read the twin). The pinned bytes are
// rewritten only after that event, so the caller may overwrite its arrays as soon as a call returns and no call waits
// for the stream.
struct Staged {
    PinBuf<char> h;
    DevBuf<char> d;
    Event fence;
    bool busy = false;
    // wait for the last commit; room for `bytes`, regrown to `room` bytes (>= bytes) when there is less
    int acquire(size_t bytes, size_t room, bool twin) {
        if (busy) TRI_HIP_TRY(hipEventSynchronize(fence.e));
        busy = false;
        if (bytes <= h.cap && h.p) return TRI_OK;
        if (const int rc = h.grow(room)) return rc;
        return twin ? d.grow(room) : TRI_OK;  // (hipFree waits for the device: nothing still reads the old twin)
    }
    int commit(hipStream_t stream) {
        if (const int rc = fence.ensure(hipEventDisableTiming)) return rc;
        TRI_HIP_TRY(hipEventRecord(fence.e, stream));
        busy = true;
        return TRI_OK;
    }
};

struct TimingSet {
    Event ev[kStageCount + 1];
    bool shadow = false;  // the frame ran the shadow pre-pass (ev[kStageShadow] was recorded)
    Event id[2];          // round k_id_raster, made at the first timed frame with the id pass
    bool has_id = false;  // ... and recorded on this frame
    Event motion[2];          // round k_motion, likewise
    bool has_motion = false;
};

// Geometry (UploadMeshFromCache, Renderer.cpp:1965-2116): one concatenated vertex buffer, one index
// buffer, the per-mesh ranges and the cluster-culling tables (fsel::GeomInfo). A context owns one; a tri_geometry made
// with tri_geometry_create is the same object shared by several contexts of one device (the editor's
// Scene and Game viewports read one vertex/index buffer, as the reference's do).
struct tri_geometry : fsel::GeomInfo {
    int device = 0;
    bool shared = false;
    uint64_t version = 0;  // bumped by every upload (contexts re-resolve their draws)
    DevBuf<TriVsIn> d_vin;
    DevBuf<float> d_pos;   // 3 floats per vertex (k_vertex's stream with vary_obj)
    DevBuf<float> d_attr;  // 9 floats per vertex {pos, normal, colour} (k_raster's, vary_obj)
    DevBuf<TriVsSkin> d_skin;
    bool has_skin_data = false;
    DevBuf<uint32_t> d_idx;
    DevBuf<TriCluster> d_clusters;
    DevBuf<TriCluster> d_vbox;  // per vertex block: union box of its clusters
    bool geometry_set = false;
};

// One A8 coverage atlas on one device (tri_font_create).
struct tri_font {
    int device = 0;
    DevBuf<uint8_t> d_alpha;
    uint32_t w = 0, h = 0;
};

struct tri_ctx {
    tri_config cfg{};
    int device = 0;
    int32_t W = 0, H = 0, y0 = 0, y1 = 0, nbx = 0, nby = 0, nbins = 0;
    int cu_count = 256;  // compute units of the device (k_setup's grid sizing)
    uint32_t last_path = 0;  // tri_frame_stats.path of the last frame built
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    tri_geometry own_geom;
    tri_geometry* geom = &own_geom;  // own_geom, or a shared tri_geometry (tri_bind_geometry)
    uint64_t geom_seen = 0;          // geom->version the resolved draws were built against

    tri_material_record mat0{{1, 1, 1, 1}, {1, 1, 1, 0}};

    // texture slots; slot 0 = default 1x1 white
    DevBuf<uint32_t> d_tex[TRI_MAX_TEXTURE_SLOTS];
    uint32_t tex_w[TRI_MAX_TEXTURE_SLOTS] = {}, tex_h[TRI_MAX_TEXTURE_SLOTS] = {};
    uint32_t tex_solid[TRI_MAX_TEXTURE_SLOTS] = {};  // texel of a 1x1 slot (RGBA8)
    int16_t tex_alpha[TRI_MAX_TEXTURE_SLOTS] = {};    // the alpha byte every texel of the slot has, or -1
    TriTexDesc texdesc[TRI_MAX_TEXTURE_SLOTS] = {};  // per-slot descriptors, aliases resolved
    bool tex_dirty = true;
    bool need_lut = false;  // fsel::slots_need_lut(texdesc), kept with the table
    DevBuf<float> d_lut;

    DevBuf<float> d_bones;  // (pose_reserve_palette grows it keeping the uploaded prefix: the one buffer not grown by grow())
    DevBuf<uint32_t> d_sky;
    DevBuf<uint32_t> d_ai;  // the AI blend's RGBA8 UNORM frame (tri_upload_ai_frame)
    Event ai_packed;  // behind tri_upload_ai_frame_device's kernel: the generator's next job waits for it
    uint32_t ai_w = 0, ai_h = 0;
    uint32_t sky_size = 0;
    // tri_upload_skybox_ex: a cubemap k_sky_fill draws (another format, a mip chain, or TRI_SKYBOX_PREFILL)
    bool sky_prefill = false;
    uint32_t sky_format = TRI_SKY_FMT_RGBA8_SRGB, sky_mips = 1;
    bool sky_uniform = false;  // every texel of the cubemap equal (e.g. the solid fallback)
    uint32_t sky_uniform_bgra = 0;
    uint32_t nbones = 0;         // the palette's extent: the uploaded prefix and the posed suffix behind it
    uint32_t nbones_prefix = 0;  // what tri_upload_bone_palette put there
    // tri_pose_palette's and tri_pose_graph's records (16 B each; a graph call's instances, then its operations): a ring
    // of stages with device twins, each fenced behind the pose kernels that read it
    Staged pose_ring[4];
    uint32_t pose_next = 0;
    TriPoseScratch pose_scratch;  // tri_pose_check's, kept between calls

    // per frame
    tri_global_ubo ubo{};
    float pv[16] = {};
    uint32_t clear_bgra = 0;
    bool frame_set = false;
    std::vector<tri_draw> draws;
    bool draws_dirty = true;

    // resolved draws (fsel::resolve_draws) and their device copies, uploaded through draw_stage
    fsel::DrawResolution res;
    DevBuf<TriDrawDev> d_draws;
    DevBuf<TriDrawShade> d_draw_shade;
    DevBuf<uint32_t> d_vbase, d_pbase, d_cbase, d_cvis;
    Staged draw_stage;
    PinBuf<TriCounters> h_ctr;  // the frame's counters, copied on the stream by tri_synchronize

    // work buffers
    DevBuf<float4> d_clip;
    DevBuf<TriSnap> d_snap;
    DevBuf<uint8_t> d_oc;
    int32_t bin_log2 = 6;
    DevBuf<float4> d_vary;
    DevBuf<TriRec> d_recs;
    DevBuf<uint32_t> d_clip_slot;
    DevBuf<uint4> d_prim_vs;
    DevBuf<uint2> d_setup_stats;
    uint32_t last_nchunks = 0;
    DevBuf<uint32_t> d_bin_count, d_bin_list;
    DevBuf<TriCounters> d_ctr;
    uint32_t ovf_rec_cap = 1u << 16, ovf_vert_cap = 1u << 17;
    uint32_t bin_cap = 0;

    // shadow-map pre-pass (tri_set_shadow)
    tri_shadow_config shadow{};
    DevBuf<float4> d_lpos;
    DevBuf<TriSnap> d_lsnap;
    DevBuf<uint32_t> d_sbin_count, d_sbin_list, d_shadow;
    uint32_t s_nbx = 0, s_nbins = 0, s_bin_cap = 0;
    bool shadow_rendered = false;  // a frame with the current map size has been enqueued

    // text overlay (tri_set_text): the caller's quads, what tri_text_build made of them for this context's rows, and
    // its device image (text_stage's twin), uploaded at the next tri_render
    tri_font* text_font = nullptr;
    std::vector<tri_text_quad> text_quads;
    TriTextPlan text_plan;
    bool text_dirty = false;
    Staged text_stage;

    // entity ids (tri_set_id_output, tri_set_outline; tri_ids.hip): the id image of the context's rows, whether the
    // last tri_render wrote it, the outline's draws as the caller gave them and their per-draw flags on the device
    // (sel_stage's twin, rebuilt when the outline or the draw count changes), tri_pick_rect's bitmap
    bool id_on = false, ids_rendered = false;
    DevBuf<uint32_t> d_ids;
    bool outline_on = false, sel_dirty = false;
    std::vector<uint32_t> outline_draws;
    float outline_rgba[4] = {};
    uint32_t outline_width = 0, sel_ndraws = 0;
    Staged sel_stage;
    DevBuf<uint32_t> d_pick_bits;
    PinBuf<uint32_t> h_pick;

    // motion vectors (tri_set_motion_output, tri_set_motion_history; tri_motion.hip): the motion image of the context's
    // rows, whether the last tri_render wrote it, the caller's history (copied; its prev_models points into
    // motion_prev_models or is null) and the reprojection table's staging
    bool motion_on = false, motion_rendered = false, motion_has_history = false;
    DevBuf<float> d_motion;
    tri_motion_history motion_history{};
    std::vector<float> motion_prev_models;
    std::vector<float> motion_table;
    Staged motion_stage;

    DevBuf<uint32_t> d_color_own;
    DevBuf<float> d_depth_own;
    DevBuf<uint32_t> d_present;  // tri_blit_linear's owned target
    uint32_t present_w = 0, present_h = 0;
    uint32_t* d_color = nullptr;
    float* d_depth = nullptr;

    // the frame's arguments: built here by tri_render, passed by value to the frame's first kernel, which
    // publishes them to d_args for the later kernels (raster_launch.h)
    TriLaunchArgs args{};
    DevBuf<TriLaunchArgs> d_args;
    bool launched = false;  // a frame was enqueued (tri_set_stream orders the next one behind it)
#ifdef TRI_DIAG_FRONT
    uint32_t diag_frames = 0;  // diagnostics build: frames rendered (the first one runs the whole plan)
#endif

    bool timing = false;
    uint32_t timing_period = 1, timing_counter = 0;  // time every timing_period-th frame
    std::vector<TimingSet> pending;
    std::vector<TimingSet> free_sets;
    tri_timing acc{};
    double acc_id_ms = 0.0;     // tri_get_id_timing: the id pass's own stamps over the timed frames that ran it
    uint64_t acc_id_frames = 0;
    double acc_motion_ms = 0.0;  // tri_get_motion_timing, likewise
    uint64_t acc_motion_frames = 0;
};

// tri_render's outline pass (tri_ids.hip): the per-draw flags to the device when they changed, then k_id_outline on
// the context's stream.
int tri_ids_outline_pass(tri_ctx* c);
// tri_render's motion pass (tri_motion.hip): checks the stored history against the frame's draws, builds and stages the
// reprojection table on the context's stream and fills k_motion's arguments; *pass says which kernel the plan takes.
int tri_motion_prepare(tri_ctx* c, TriMotionArgs* args, TriMotionPass* pass);
// Switch the motion output off and free its image (tri_set_id_output(0) takes it along); the stream is idle.
int tri_motion_release(tri_ctx* c);

inline int make_current(tri_ctx* c) {
    TRI_HIP_TRY(hipSetDevice(c->device));
    return TRI_OK;
}

// Replace a buffer's contents from host memory between frames: the context's stream drained (no queued frame still
// reads what grow() frees), a blocking copy, and the null stream drained: the context's stream is non-blocking, so
// null-stream work is not ordered with it and must be complete before the next frame can read the buffer.
template <typename T>
int upload_blocking(tri_ctx* c, DevBuf<T>& buf, size_t count, const void* src, size_t bytes) {
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    if (const int rc = buf.grow(count)) return rc;
    if (bytes) TRI_HIP_TRY(hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice));
    TRI_HIP_TRY(hipStreamSynchronize(nullptr));
    return TRI_OK;
}
