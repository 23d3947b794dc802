// raster_launch.h — host-side launchers for the gfx950 kernels (the frame plan: raster_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <vector>
#include "raster_common.h"

// Tunables (numeric; -D overrides them for A/B builds), read by the kernels and by the host's launch geometry.
// k_setup occupancy target (waves per SIMD); with 4 waves per workgroup, also its workgroups per CU
#ifndef TRI_SETUP_WAVES
#define TRI_SETUP_WAVES 6
#endif
#ifndef TRI_SETUP_WGS_PER_CU
#define TRI_SETUP_WGS_PER_CU TRI_SETUP_WAVES
#endif
// (the host's other set-up tunables, TRI_SETUP_WGS_PER_CU_OVERLAP and TRI_SETUP_BAND_CHUNKS, which no kernel reads,
// are with the rule that uses them: frame_select.h)

// Device pointers in the global address space (device compilation only; the host sees plain pointers of the same
// size). The later kernels of a frame read these pointers from the device copy of their arguments, not from
// kernel-argument memory, so without the qualifier the compiler cannot tell them from LDS pointers: every access
// became a flat instruction, which counts against the LDS wait counter too (a wait for an LDS result then also
// waits for every outstanding memory load).
// (Only in the kernels' translation units, TRI_KERNEL_TU: host code elsewhere fills the struct with plain pointers,
// and the device pass of a host-only file still type-checks those assignments.)
#if defined(__HIP_DEVICE_COMPILE__) && defined(TRI_KERNEL_TU)
#define TRI_G __attribute__((address_space(1)))
#else
#define TRI_G
#endif

struct TriDeviceBuffers {
    TRI_G const TriVsIn* vin;
    TRI_G const float* vpos;           // 12 B per vertex: the positions alone (k_vertex's only input with vary_obj)
    TRI_G const float* vattr;          // 36 B per vertex {pos, normal, colour}: the fragment stage's records with vary_obj
    TRI_G const TriVsSkin* vskin;      // may be null when no draw skins
    TRI_G const float* bones;
    uint64_t vertex_count;
    TRI_G const uint32_t* indices;
    TRI_G const TriDrawDev* draws;
    TRI_G const TriDrawShade* draw_shade;
    TRI_G const uint32_t* draw_vbase;  // ndraws+1
    TRI_G const uint32_t* draw_pbase;  // ndraws+1
    TRI_G const uint32_t* sky;         // 6 * sky_size^2 RGBA8 sRGB texels (+X,-X,+Y,-Y,+Z,-Z)
    TRI_G const float* srgb_lut;       // 256 sRGB -> linear (host, double) + 256 alpha b/255
    TRI_G float4* clip;                // nslots (read only when a primitive is clipped)
    TRI_G TriSnap* snap;               // nslots: {X, Y as exact floats, 1/w, z}
    TRI_G uint8_t* oc;                 // nslots outcodes
    TRI_G float4* vary;                // 3 * (nslots + ovf_vert_cap)
    TRI_G TriRec* recs;                // ovf_rec_cap clipped sub-triangles
    TRI_G uint32_t* clip_slot;         // nprims: first sub-triangle record of a clipped primitive
    TRI_G uint4* prim_vs;              // nprims: {vertex slot 0, 1, 2, draw | TRI_PRIM_CLIPPED} of every
                                 // primitive k_setup passed on (visible or clipped)
    TRI_G uint32_t* bin_count;         // nbins entry counters (zero between frames: k_raster re-zeroes)
    TRI_G uint32_t* bin_list;          // nbins * bin_cap record ids (fixed-capacity queue per bin)
    TRI_G TriCounters* counters;
    TRI_G uint2* setup_stats;          // nchunks {triangles set up, bin entries} per k_setup workgroup
    TRI_G uint32_t* color;             // band rows * W
    TRI_G float* depth;                // band rows * W (may be null)
    // cluster culling (only when TriFrameParams::cull_on)
    TRI_G const TriCluster* clusters;  // all meshes' clusters
    TRI_G const TriCluster* vbox;      // per mesh vertex block: the union box of the clusters referencing it
    TRI_G const uint32_t* draw_cbase;  // ndraws+1: first (draw, cluster) pair of each draw
    TRI_G uint32_t* cvis;              // ncl_total visibility flags, written by k_vertex each frame
    // shadow-map pre-pass (only when TriFrameParams::shadow_on)
    TRI_G float4* lpos;                // nslots + ovf_vert_cap: light-NDC position per vertex slot (xyz, 0)
    TRI_G TriSnap* lsnap;              // nslots: the light-NDC position snapped to the map ({X | outcode << 24, Y, 1, z})
    TRI_G uint32_t* sbin_count;        // s_nbins shadow-map bin counters (zeroed by k_shadow_raster)
    TRI_G uint32_t* sbin_list;         // s_nbins * s_bin_cap primitive ids
    TRI_G uint32_t* shadow_map;        // s_size * s_size float32 depth bits
    TRI_G const uint32_t* ai_frame;    // the AI blend's RGBA8 UNORM frame (only when TriFrameParams::ai_on)
};

// One frame's arguments (DESIGN.md §2 "launch cost"). The frame's first kernel (k_vertex, k_vertex_band or
// k_reset) takes them by value — kernel-argument memory, which its many short waves read fastest — and its
// workgroup 0 publishes them to a device copy that every later kernel of the frame reads through a 16-B
// pointer argument (k_setup, k_shadow_raster, k_raster: one kernarg block of 1.8 KB per frame instead of one
// per launch). Stream order makes the copy complete before k_setup starts and keeps the next frame's copy
// behind this frame's raster.
struct TriLaunchArgs {
    TriFrameParams fp;
    TriDeviceBuffers b;
};
static_assert(sizeof(TriLaunchArgs) % 16 == 0, "TriLaunchArgs moves in 16-B pieces");

// The kernels of one frame in launch order (which instantiation, grid, block) — computed on the host from the
// frame's parameters; the same plan is launched directly or as a cached HIP graph.
struct TriKernelLaunch {
    const void* func;  // the first launch takes (TriLaunchArgs by value, TriLaunchArgs* copy); the others the copy
    dim3 grid, block;
    int stage;  // TriStage stamped before this launch when timing (-1: none)
};
struct TriFramePlan {
    uint32_t n = 0;
    TriKernelLaunch k[6];
};
// The id pass's own arguments (id_pass.hip), by value behind the frame's published arguments: the frame's
// TriLaunchArgs stay as they are, so no other kernel of the frame sees the pass.
struct TriIdArgs {
    TRI_G uint32_t* ids;  // W x (y1 - y0) draw ids of the context's rows
};
constexpr int kStageId = -1;  // the id pass's launch: none of tri_timing's stamps (its layout is fixed); two of its own
// id_pass: with the context's id output on, k_id_raster between the set-up (and the shadow map's raster) and the
// frame's raster kernel, which re-zeroes the bin counts the pass reads; off, the plan is launch for launch the same.
// The motion pass's own arguments (motion_pass.hip), by value and alone: k_motion reads nothing of the frame's
// TriLaunchArgs.
struct TriMotionArgs {
    TRI_G const uint32_t* ids;   // W x rows draw ids (the id pass's image)
    TRI_G const float* depth;    // W x rows, the frame's depth target
    TRI_G float* motion;         // W x rows x 2
    TRI_G const float* table;    // (ndraws + 1) x 16: row-major R_k (motion_math.h)
    uint32_t W, npix;            // the frame's width; W x rows pixels
    uint32_t y0;                 // the context's first row in the frame
    uint32_t ndraws;
    float sx, sy, hw, hh;        // 2 / W, 2 / H, W / 2, H / 2 (float32, from the host)
};
constexpr int kStageMotion = -2;  // the motion pass's launch: like kStageId, two stamps of its own
enum TriMotionPass { kMotionOff = 0, kMotionVec4, kMotionScalar };
// motion: with the context's motion output on, k_motion behind the frame's raster kernel, whose depth it reads; four
// pixels per lane (kMotionVec4) when every image starts on a 16-B boundary, else one. Off, the plan is launch for
// launch the same.
void tri_plan_frame(const TriFrameParams& fp, TriFramePlan& plan, bool id_pass = false, TriMotionPass motion = kMotionOff);
// k_motion and its grid over W x rows pixels (motion_pass.hip)
const void* tri_motion_kernel(bool vec4);
dim3 tri_motion_grid(uint32_t npix, bool vec4);
// The history reprojection pass's arguments (history_pass.hip), by value and alone: k_reproject is no part of a frame's
// plan; tri_history_reproject enqueues it behind the frame. Every image is W x H, whole frames only.
struct TriReprojectArgs {
    TRI_G const uint32_t* colour;       // the frame just rendered: B8G8R8A8, ids, depth
    TRI_G const uint32_t* ids;
    TRI_G const float* depth;
    TRI_G const float* table;           // (ndraws + 1) x 16: the motion table the frame staged
    TRI_G const uint32_t* prev_colour;  // the stored previous frame (not read when has_prev is 0)
    TRI_G const uint32_t* prev_ids;
    TRI_G const float* prev_depth;
    TRI_G uint32_t* next_colour;        // the other set: the frame just rendered, stored for the next call
    TRI_G uint32_t* next_ids;
    TRI_G float* next_depth;
    TRI_G uint32_t* warped;             // B8G8R8A8
    TRI_G uint8_t* mask;                // one byte per pixel (4-B aligned)
    uint32_t W, H, npix, ndraws;
    float sx, sy, hw, hh;               // 2 / W, 2 / H, W / 2, H / 2 (float32, from the host)
    float tolerance;
    uint32_t has_prev;
};
// k_reproject over the frame on `stream`: four pixels per lane (vec4) when every image starts on a 16-B boundary, else one.
hipError_t tri_launch_reproject(const TriReprojectArgs& args, bool vec4, hipStream_t stream);
// The temporal anti-aliasing pass's arguments (taa_pass.hip), by value and alone like k_reproject's: tri_taa_resolve
// enqueues k_taa_resolve behind the frame. Every image is W x H, whole frames only. The context's planes are read four
// bytes at a time and may start anywhere; the object's own come from hipMalloc.
struct TriTaaArgs {
    TRI_G const uint32_t* colour;    // the frame just rendered: B8G8R8A8, ids, depth
    TRI_G const uint32_t* ids;
    TRI_G const float* depth;
    TRI_G const float* table;        // (ndraws + 1) x 16: the motion table the frame staged
    TRI_G const uint2* prev_acc;     // the stored history (not read when has_prev is 0): 4 x uint16 per pixel, and ids
    TRI_G const uint32_t* prev_ids;
    TRI_G uint2* next_acc;           // the other set
    TRI_G uint32_t* next_ids;
    TRI_G uint32_t* resolved;        // B8G8R8A8
    TRI_G uint8_t* mask;             // one byte per pixel
    uint32_t W, H, ndraws;
    float sx, sy, hw, hh;            // 2 / W, 2 / H, W / 2, H / 2 (float32, from the host)
    float alpha;
    uint32_t has_prev, reject_id;
};
hipError_t tri_launch_taa_resolve(const TriTaaArgs& args, hipStream_t stream);
// The temporal upscaling pass's arguments (upscale_pass.hip), by value and alone like k_taa_resolve's: tri_upscale_resolve
// enqueues k_upscale_resolve behind the frame. The context's planes and the previous ids are Wr x Hr, the object's
// accumulated colour, resolved image and mask Wo x Ho; whole frames only. The context's planes are read four bytes at a
// time and may start anywhere; the object's own come from hipMalloc. The frame's ids reach the written set through a
// copy on the same stream, not through the kernel.
struct TriUpscaleArgs {
    TRI_G const uint32_t* colour;    // the frame just rendered, Wr x Hr: B8G8R8A8, ids, depth
    TRI_G const uint32_t* ids;
    TRI_G const float* depth;
    TRI_G const float* table;        // (ndraws + 1) x 16: the motion table the frame staged
    TRI_G const uint2* prev_acc;     // the stored history (not read when has_prev is 0): Wo x Ho, 4 x uint16 per pixel
    TRI_G const uint32_t* prev_ids;  // ... and the ids it was accumulated under, Wr x Hr
    TRI_G uint2* next_acc;           // the other set, Wo x Ho
    TRI_G uint32_t* resolved;        // B8G8R8A8, Wo x Ho
    TRI_G uint8_t* mask;             // one byte per output pixel
    uint32_t Wr, Hr, Wo, Ho, ndraws;
    float rx, ry, ox, oy;            // Wr / Wo, Hr / Ho, Wo / Wr, Ho / Hr (float32, from the host)
    float sx, sy, hw, hh;            // 2 / Wo, 2 / Ho, Wo / 2, Ho / 2
    float alpha, jx, jy;
    uint32_t has_prev, reject_id;
};
hipError_t tri_launch_upscale_resolve(const TriUpscaleArgs& args, hipStream_t stream);
// k_id_raster at the frame's bin size (id_pass.hip)
const void* tri_id_raster_kernel(const TriFrameParams& fp);
#ifdef TRI_DIAG_FRONT
void tri_diag_front_plan(TriFramePlan& plan);  // diagnostics build only (raster_kernels.hip)
#endif
// k_raster_plain's instantiation for a frame without the shadow pre-pass (raster_plain.hip)
const void* tri_raster_plain_kernel(const TriFrameParams& fp);
// The frame kind that instantiation takes: the frame's TRI_KIND_* switches (include/tri_raster.h) when a kernel with
// them as compile-time constants is built for its bin size, -1 for the generic instantiation (raster_plain.hip)
int tri_raster_kind(const TriFrameParams& fp);
// The frame's first kernel (vertex_stage.hip): k_vertex, k_vertex_band (row bands with cluster culling) or k_reset
// (a frame without vertex work)
enum TriFrontKernel { kFrontVertex = 0, kFrontBand, kFrontReset };
const void* tri_vertex_stage_kernel(TriFrontKernel k);

// Event stamps of one frame, in launch order: vertex, setup (+ clip, + the shadow map binning), shadow-map
// raster (only with the pre-pass), raster, end.
enum TriStage { kStageVertex = 0, kStageShadow, kStageSetup, kStageRaster, kStageCount };

// One frame = 3 dependent launches on `stream` (k_vertex, k_setup with in-wave clipping, k_raster), 4 with the
// shadow pre-pass (k_shadow_raster after k_setup<shadow>); `events` (may be null) gets kStageCount + 1 stamps
// (the kStageShadow stamp only when the pre-pass runs).
// `id`: the id pass's arguments when the plan holds its launch (kStageId); `id_events` (may be null): two stamps of the
// pass's own, in front of and behind that launch. `motion`, `motion_events`: the same for the motion pass (kStageMotion).
hipError_t tri_run_plan(const TriFramePlan& plan, const TriLaunchArgs& args, TriLaunchArgs* d_args,
                        hipStream_t stream, hipEvent_t* events, const TriIdArgs* id = nullptr,
                        hipEvent_t* id_events = nullptr, const TriMotionArgs* motion = nullptr,
                        hipEvent_t* motion_events = nullptr);

// The id pass's other kernels (id_pass.hip; include/tri_raster.h "entity ids"). ids: W x rows.
// k_id_collect: ORs bit id - 1 of `bits` (nwords words, cleared by the caller) for every id >= 1 inside columns
// [x0, x0 + w) of local rows [row0, row0 + h).
hipError_t tri_launch_id_collect(const uint32_t* ids, int32_t W, int32_t x0, int32_t row0, int32_t w, int32_t h,
                                 uint32_t* bits, uint32_t nwords, hipStream_t stream);
// k_id_outline: composites rgba over the outline pixels of the draws flagged in sel (ndraws words), width r in 1..8.
hipError_t tri_launch_id_outline(const uint32_t* ids, const uint32_t* sel, uint32_t ndraws, uint32_t* color, int32_t W,
                                 int32_t rows, int32_t r, const float rgba[4], hipStream_t stream);

// k_sky_fill (sky_fill.hip): the skybox pass ahead of a TRI_SKY_PREFILLED frame's raster kernel. By value: the pass
// runs in front of the frame's first kernel, which publishes the frame's own arguments.
struct TriSkyFillArgs {
    int32_t W, H, y0, y1;          // the frame and the context's rows
    uint32_t clear_bgra;
    uint32_t mode;                 // TRI_SKY_RAY or TRI_SKY_PERSP
    uint32_t format, size, mips;   // TRI_SKY_FMT_*, the level 0 face edge, the level count
    uint32_t pad;
    float ip[16], R[9], pw[4], far[16];  // TriFrameParams::sky_ip, sky_R, sky_pw, sky_far
    uint32_t level_texel[16];      // each level's first texel (level-major, then face, then rows)
    TRI_G const uint32_t* texels;
    TRI_G const float* lut;        // TriDeviceBuffers::srgb_lut
    TRI_G uint32_t* color;         // the context's first row
};
hipError_t tri_launch_sky_fill(const TriSkyFillArgs& args, hipStream_t stream);

// Presentation blit (tri_blit_linear): src W x H B8G8R8A8 -> dst dw x dh, linear, clamp-to-edge.
hipError_t tri_launch_blit(const uint32_t* src, int32_t w, int32_t h, uint32_t* dst, int32_t dw, int32_t dh,
                           const float* unorm_lut, hipStream_t stream);

// The band codec (band_codec.hip): B8G8R8A8 <-> 3-byte BGR with a known alpha. The sender's status reaches the
// display with the band (tri_xfer): pack_bgr24 also ORs its alpha flag into `trailer` (a word after the packed pixels,
// zero at allocation, sticky like the flags), which unpack_bgr24 ORs into the display's `flags`; a dbp slot carries
// its own alpha mark (header word 1) and overflow (its payload count), which unpack ORs into `flags` (both nullable).
hipError_t tri_launch_pack_bgr24(const uint32_t* src, uint8_t* dst, uint64_t n, uint32_t alpha, uint32_t* flag,
                                 hipStream_t stream, uint32_t* trailer = nullptr);
hipError_t tri_launch_unpack_bgr24(const uint8_t* src, uint32_t* dst, uint64_t n, uint32_t alpha, hipStream_t stream,
                                   const uint32_t* trailer = nullptr, uint32_t* flags = nullptr);
hipError_t tri_launch_dbp_pack(const uint32_t* src, uint64_t n, uint32_t alpha, uint8_t* dst, uint32_t slot_bytes,
                               uint32_t* flags, hipStream_t stream);
hipError_t tri_launch_dbp_unpack(const uint8_t* src, uint64_t n, uint32_t alpha, uint32_t slot_bytes, uint32_t* dst,
                                 hipStream_t stream);
uint64_t tri_dbp_stream_bytes(uint64_t pixels, uint32_t slot_bytes);
hipError_t tri_launch_dbp_unpack_bands(const uint8_t* const* src, uint32_t* const* dst, const uint64_t* n, uint32_t count,
                                       uint32_t alpha, uint32_t slot_bytes, hipStream_t stream, uint32_t* flags = nullptr);

// Recording (record_yuv.hip): src width x height B8G8R8A8 (4-B aligned, pitch_bytes a multiple of 4 and at least
// width * 4) -> dst 3 * width * height bytes at any alignment: the Y, U and V planes of the reference's fp64
// conversion (VideoEncoder.cpp:716-736), byte for byte.
hipError_t tri_launch_bgra_to_yuv444(const void* src, uint32_t width, uint32_t height, uint32_t pitch_bytes, uint8_t* dst,
                                     hipStream_t stream);
// JPEG recording (jpeg_encode.hip): the same source -> a baseline JPEG behind the header that `out` already holds, by
// csrc/jpeg_math.h's rule. Every pointer is device memory sized by jpeg::make_layout / jpeg::max_bytes for the extent
// and `restart` (>= 1): tables one jpeg::Tables, coef mcus * 384 int16 (16-B aligned), scratch intervals *
// segment_bytes, counts and offsets one dword per interval, size_word one dword (the stream's size, SOI to EOI).
struct tri_jpeg_job {
    const void* src;
    uint32_t pitch_bytes, width, height;
    uint32_t restart, segment_bytes, header_bytes;
    const void* tables;
    int16_t* coef;
    uint8_t* scratch;
    uint32_t *counts, *offsets;
    uint8_t* out;
    uint32_t* size_word;
};
hipError_t tri_launch_jpeg_encode(const tri_jpeg_job& job, hipStream_t stream);
// The AI input tensor (frame_tensor.hip): the same source -> dst width * height * 4 floats (4-B aligned; 16-B aligned
// for the 16-B store path), R, G, B, A per pixel, each (float)byte * (1.0f / 255.0f) (Renderer.cpp:1111-1389).
hipError_t tri_launch_bgra_to_rgba_f32(const void* src, uint32_t width, uint32_t height, uint32_t pitch_bytes, float* dst,
                                       hipStream_t stream);

// The frame generator (nn_conv.hip, frame_generator.hip; include/tri_raster.h "the frame generator").
// One checked layer on the current device: every pointer device memory, res1 / res2 may be null.
hipError_t tri_launch_nn_conv(const tri_nn_conv_desc& desc, const float* in, const float* packed_weights,
                              const float* scale, const float* shift, const float* res1, const float* res2, float* out,
                              hipStream_t stream);
// k_ai_pack: pixels x channels (1..4) floats -> pixels R8G8B8A8 dwords (tri_upload_ai_frame_device's rules).
hipError_t tri_launch_ai_pack(const float* src, uint64_t pixels, uint32_t channels, uint32_t* dst, hipStream_t stream);
int tri_internal_framegen_device(const tri_framegen* gen);
// Recorded on the generator's stream behind its last submitted job (null before the first).
hipEvent_t tri_internal_framegen_done(const tri_framegen* gen);
// The generator's stream waits for `read`, recorded behind a reader of its output on another stream.
hipError_t tri_internal_framegen_reader(tri_framegen* gen, hipEvent_t read);

// The text overlay (text_overlay.hip; include/tri_raster.h "text overlay"). A wave of k_text_overlay scans its
// bin's quad references TRI_TEXT_SCAN_CHUNK at a time (one per lane) and walks the ballot of the hits in order: the
// ballot is the per-round list, TRI_TEXT_LIST_CAP entries; a strip under more quads takes more rounds. Screen bins are
// TRI_TEXT_BIN x TRI_TEXT_BIN pixels. (Mirrored in python/trident_raster/abi.py; the tests size themselves from them.)
#define TRI_TEXT_SCAN_CHUNK 64
#define TRI_TEXT_LIST_CAP 64
#define TRI_TEXT_BIN 32
// One quad as the kernel reads it: snapped corners (mirroring resolved: X0 < X1, Y0 < Y1), u, v at (X0, Y0) and their
// span to (X1, Y1), the colour.
struct TriTextQuadDev {
    int32_t X0, Y0, X1, Y1;
    float u0, du, v0, dv;
    float rgba[4];
};
static_assert(sizeof(TriTextQuadDev) == 48, "TriTextQuadDev layout");
// What tri_text_build derives from a context's quads (host only): `blob` is the device image — nquads TriTextQuadDev,
// at off_refs nrefs uint4 {quad, x0 | x1 << 16, y0 | y1 << 16, 0} (inclusive pixel boxes) filed per bin in
// submission order, at off_rows nbx * nby uint2 {first, end} reference ranges — and the launch's bin box.
struct TriTextPlan {
    std::vector<uint8_t> blob;
    size_t off_refs = 0, off_rows = 0;
    uint32_t nquads = 0, nrefs = 0;
    uint32_t bx0 = 0, by0 = 0, nbx = 0, nby = 0;
};
bool tri_text_quads_finite(const tri_text_quad* quads, uint32_t count);
// rows [y0, y1) of a frame W wide: quads that cover no pixel centre there are dropped (nquads 0: nothing to launch)
void tri_text_build(const tri_text_quad* quads, uint32_t count, int32_t W, int32_t y0, int32_t y1, TriTextPlan& plan);
// color: the context's first row; d_blob: plan.blob on the device (16-B aligned)
hipError_t tri_launch_text(uint32_t* color, int32_t W, int32_t y0, int32_t y1, const TriTextPlan& plan,
                           const uint8_t* d_blob, const uint8_t* atlas, uint32_t aw, uint32_t ah, hipStream_t stream);

// Device pose evaluation (pose_eval.hip; include/tri_raster.h "skeletal poses evaluated on the device").
int tri_internal_animset_device(const tri_animset* set);
// The host-side check of a tri_pose_palette call against a palette whose uploaded prefix holds `prefix` matrices:
// TRI_OK with the end of the posed suffix (*extent, in matrices; `prefix` for no instances), or TRI_E_INVALID with the
// message recorded. scratch is the caller's to keep between calls (no allocation per frame once it has grown); on
// success scratch.bones[i] is instance i's bone count.
struct TriPoseScratch {
    std::vector<std::pair<uint32_t, uint32_t>> spans;  // {first matrix, matrices}, sorted for the overlap test
    std::vector<uint32_t> bones;
    std::vector<tri_pose_instance> plain;  // tri_pose_graph_check's: its instances as tri_pose_check takes them
};
int tri_pose_check(const tri_animset* set, const tri_pose_instance* instances, uint32_t count, uint32_t prefix,
                   uint32_t* extent, TriPoseScratch& scratch);
// d_instances: checked records on the set's device, none of a skeleton with more than lds_bones bones (the workgroups'
// LDS is sized by it); palette: at least *extent matrices.
hipError_t tri_launch_pose(const tri_animset* set, const tri_pose_instance* d_instances, uint32_t count,
                           uint32_t lds_bones, float* palette, hipStream_t stream);
// The same for a tri_pose_graph call: tri_pose_check on the instances' skeletons and palette slices, then every
// program's op range, stack discipline, limits, ops, clips and masks. Every index k_pose_graph uses is checked here.
int tri_pose_graph_check(const tri_animset* set, const tri_pose_graph_instance* instances, uint32_t count,
                         const tri_pose_op* ops, uint32_t op_count, uint32_t prefix, uint32_t* extent,
                         TriPoseScratch& scratch);
// d_instances as for tri_launch_pose; d_ops: the operations their op_first index, on the same device.
hipError_t tri_launch_pose_graph(const tri_animset* set, const tri_pose_graph_instance* d_instances,
                                 const tri_pose_op* d_ops, uint32_t count, uint32_t lds_bones, float* palette,
                                 hipStream_t stream);
// The matrices of a context's uploaded palette prefix.
uint32_t tri_internal_pose_prefix(tri_ctx* ctx);
