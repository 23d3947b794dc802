/*
 * tri_raster.h — C-ABI drop-in boundary for the MI355X (gfx950) HIP software rasterizer that
 * replaces Trident's Vulkan graphics-pipeline stage (the work recorded by
 * Renderer::RecordCommandBuffer, Trident/src/Renderer/Renderer.cpp:4890-5636, and executed by the
 * driver with Default.vert / Default.frag).
 *
 * Plain C: no torch, no HIP types in the signatures. Device memory, streams and events are owned by
 * the context; callers pass host pointers (copied) except in tri_bind_output / tri_set_stream, which
 * take opaque device pointers / a hipStream_t as void*.
 *
 * Every entry point returns an int status (TRI_OK == 0, negative on error) and records a message
 * readable through tri_last_error() — mirroring the reference's "bool + TR_CORE_* log, no exceptions
 * on the frame path" convention (Renderer.cpp:779-824). One host thread per context; not thread-safe
 * (Application.cpp:82-134 is a single render thread).
 *
 * Which reference interface each entry point replaces is noted next to it. The C++
 * Trident::Renderer-compatible shim (3d-renderer_amd/host/) calls these; INTEGRATION.md shows the
 * binding a Trident maintainer would add.
 */
#ifndef TRI_RASTER_H
#define TRI_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRI_RASTER_ABI_VERSION 2 /* 2: tri_geometry, tri_image, shadow pre-pass, tri_group fences */

/* ---- status codes ---------------------------------------------------------------------- */
#define TRI_OK 0
#define TRI_E_INVALID (-1)     /* bad argument (null, out of range, size mismatch)              */
#define TRI_E_HIP (-2)         /* HIP runtime error (no device, launch failure, ...)            */
#define TRI_E_OOM (-3)         /* device allocation failed                                      */
#define TRI_E_OVERFLOW (-4)    /* a frame overflowed an internal bin/clip buffer; buffers were   *
                                * grown, re-render the frame                                    */
#define TRI_E_UNSUPPORTED (-5) /* combination outside the path (AI blend + shadow pre-pass)     */
#define TRI_E_STATE (-6)       /* call order violated (e.g. render before geometry upload)      */
#define TRI_E_TIMEOUT (-7)     /* a multi-GPU exchange missed its deadline (communicators aborted) */

/* ---- limits mirrored from the reference ----------------------------------------------- */
#define TRI_MAX_POINT_LIGHTS 8   /* kMaxPointLights, UniformBuffer.h:7                           */
#define TRI_MAX_TEXTURE_SLOTS 256 /* Pipeline.h:18 (sampler2D BaseColorSamplers[256])            */
#define TRI_MAX_BONE_INFLUENCES 4 /* Vertex::MaxBoneInfluences, Vertex.h:11                      */
#define TRI_MAX_DIM 8192          /* framebuffer width/height limit (guard-band fixed point)    */

/* ---- GPU ABI structs: byte-identical to the reference's --------------------------------- */

/* Vertex (Trident/src/Renderer/Vertex.h:9-78): glm without SIMD alignment => 100-byte stride.
 * Offsets: Position 0, Normal 12, Tangent 24, Bitangent 36, Color 48, TexCoord 60,
 * BoneIndices 68, BoneWeights 84. */
typedef struct tri_vertex {
    float position[3];
    float normal[3];
    float tangent[3];
    float bitangent[3];
    float color[3];
    float texcoord[2];
    int32_t bone_indices[4];
    float bone_weights[4];
} tri_vertex;

/* MeshDrawInfo (Renderer.h:293-299): one per uploaded mesh; indices are mesh-local and
 * base_vertex is added at draw time (Renderer.cpp:2032-2038, :2062-2077). */
typedef struct tri_mesh_range {
    uint32_t first_index;
    uint32_t index_count;
    int32_t base_vertex;
    int32_t material_index;
} tri_mesh_range;

/* RenderablePushConstant (Trident/src/Renderer/RenderData.h:14-30), 128 bytes. */
typedef struct tri_push_constant {
    float model[16]; /* column-major glm::mat4 */
    float tint[4];
    float texture_scale[2];
    float texture_offset[2];
    float tiling_factor;
    int32_t texture_slot;
    int32_t use_material_override;
    float sort_bias;
    int32_t material_index;
    int32_t padding0;
    int32_t bone_offset;
    int32_t bone_count;
} tri_push_constant;

/* One vkCmdDrawIndexed(IndexCount, 1, FirstIndex, BaseVertex, 0) + its push constant
 * (Renderer.cpp:5110-5151). mesh_index selects a tri_mesh_range. */
typedef struct tri_draw {
    uint32_t mesh_index;
    uint32_t reserved[3];
    tri_push_constant pc;
} tri_draw;

/* PointLightUniform (UniformBuffer.h:10-14). */
typedef struct tri_point_light {
    float position_range[4];  /* xyz = world position, w = radius */
    float color_intensity[4]; /* rgb = colour, w = intensity      */
} tri_point_light;

/* GlobalUniformBuffer (UniformBuffer.h:17-28), 480 bytes std140, as written by
 * Renderer::UpdateUniformBuffer (Renderer.cpp:5822-6051). */
typedef struct tri_global_ubo {
    float view[16];
    float projection[16];
    float camera_position[4];
    float ambient_color_intensity[4];
    float directional_light_direction[4];
    float directional_light_color[4];
    uint32_t light_counts[4];
    float ai_blend_config[4];
    tri_point_light point_lights[TRI_MAX_POINT_LIGHTS];
} tri_global_ubo;

/* MaterialUniformBuffer (UniformBuffer.h:31-35). Only record 0 is read by Default.frag:58-62. */
typedef struct tri_material_record {
    float base_color_factor[4];
    float material_factors[4]; /* x metallic, y roughness, z ambient strength, w reserved */
} tri_material_record;

/* Context configuration. The viewport is always the full width x height framebuffer
 * (Renderer.cpp:5062-5069: x=y=0, minDepth 0, maxDepth 1). band_y0/band_y1 select the row band
 * this context rasterizes (multi-GPU screen partition); 0/0 means all rows. */
typedef struct tri_config {
    uint32_t width;
    uint32_t height;
    uint32_t band_y0;
    uint32_t band_y1;
    int32_t device; /* HIP device ordinal; -1 = current device */
    uint32_t flags; /* TRI_FLAG_* */
} tri_config;

#define TRI_FLAG_NO_DEPTH_OUTPUT 0x1u /* skip the depth write (reference storeOp DONT_CARE) */
#define TRI_FLAG_EXACT_SHADING 0x2u   /* Default.frag with IEEE div/sqrt/powf in the oracle's order *
                                       * (default: hardware rcp/rsq/exp/log; both within 1 LSB)     */
#define TRI_FLAG_CLUSTER_CULL 0x4u    /* cull 512-triangle clusters by their projected boxes on whole *
                                       * frames too (row-band contexts always do); output unchanged  */

/* Per-stage accumulated device time (HIP events on the context stream) and last-frame counters. */
typedef struct tri_timing {
    uint64_t frames;        /* frames timed since the last reset                  */
    double ms_vertex;       /* vs_transform (+ per-vertex divide / viewport / snap) */
    double ms_setup;        /* tri_setup_bin (setup + cull + per-bin queues)       */
    double ms_shadow;       /* shadow-map depth raster (0 without the pre-pass; its set-up/binning  *
                             * shares the set-up pass and is in ms_setup, as is clipping)             */
    double ms_raster;       /* tile_raster_shade (coverage + early-Z + PBR + store) */
    double ms_frame;        /* first kernel start to last kernel end              */
    double reserved;
} tri_timing;

typedef struct tri_frame_stats {
    uint64_t triangles_in;      /* primitives submitted                            */
    uint64_t triangles_setup;   /* primitives surviving clip/cull/snap             */
    uint64_t triangles_clipped; /* primitives that went through geometric clipping */
    uint64_t bin_entries;       /* (triangle, bin) pairs                           */
    uint64_t vertices_shaded;   /* vertex-shader invocations                       */
    uint32_t bins_x, bins_y, bin_size;
    uint32_t path;              /* TRI_PATH_* bits: the fragment path the last frame took (diagnostics) */
} tri_frame_stats;

/* tri_frame_stats.path bits */
#define TRI_PATH_ONE_DRAW   0x1u  /* one draw over a 1x1 texture slot: the single-draw solid instantiation */
#define TRI_PATH_VARY_OBJ   0x2u  /* object-space varyings (no per-frame varying writes)                   */
#define TRI_PATH_OBJ_XFORM  0x4u  /* ... carried through a non-identity model / normal matrix per pixel     */
#define TRI_PATH_OBJ_UCOL   0x8u  /* ... one vertex colour for the whole geometry                           */
#define TRI_PATH_SHADOW    0x10u  /* the shadow-map pre-pass ran                                            */
#define TRI_PATH_OBJ48     0x20u  /* object-space varyings outside the single-draw solid instantiation      */
#define TRI_PATH_IDX_ROUTE 0x40u  /* several draws: vertex slots from the index buffer, no per-primitive record */
#define TRI_PATH_EXACT     0x80u  /* the exact instantiation shaded it: TRI_FLAG_EXACT_SHADING, or uvs beyond 8192 texels */
#define TRI_PATH_KIND     0x100u  /* a frame-kind instantiation shaded it: the frame-uniform switches below are      *
                                   * compile-time constants of its kernel, which is named by                         *
                                   * (path >> TRI_PATH_KIND_SHIFT) & TRI_KIND_MASK; clear: the generic instantiation */
#define TRI_PATH_KIND_SHIFT 16
/* the switches of a frame kind (single-draw solid frames with object-space varyings only) */
#define TRI_KIND_XFORM   0x1u  /* TRI_PATH_OBJ_XFORM                                              */
#define TRI_KIND_UCOL    0x2u  /* TRI_PATH_OBJ_UCOL: no colour gathers                            */
#define TRI_KIND_SUN     0x4u  /* a directional light                                             */
#define TRI_KIND_DEPTH   0x8u  /* the frame has a depth target (no TRI_FLAG_NO_DEPTH_OUTPUT)      */
#define TRI_KIND_SKYQ   0x10u  /* background pixels queue for the skybox pass (a non-uniform sky) */
#define TRI_KIND_LIGHTS 0x20u  /* at least one point light                                        */
#define TRI_KIND_MASK   0x3Fu

/* Shadow-map pre-pass (BASELINE.json config 5). The reference reserves the switch
 * (LightComponent::m_ShadowCaster, Trident/src/ECS/Components/LightComponent.h:33) but renders no shadow
 * map, so this pass is defined here and restated by the oracle:
 *   - every frame, before the main pass, the draws' triangles are rasterised depth-only into a
 *     size x size D32 map by the orthographic light transform `light_view_proj` (column-major, affine:
 *     its last row must be exactly 0,0,0,1): texel (i, j) covers light NDC x in [2i/size - 1, 2(i+1)/size - 1),
 *     y likewise; the main pass's raster rules (8-bit snap, top-left fill, plane depth), no culling,
 *     depth clamp instead of near/far clipping, a slope-scaled depth bias (Vulkan depthBiasSlopeFactor
 *     semantics: + slope_bias * the triangle's largest depth change per texel, before the clamp),
 *     LEQUAL (the map keeps the minimum depth, clear 1.0);
 *     triangles reaching beyond the guard band (|x|, |y| > 2*16000/size - 1 in light NDC) cast nothing;
 *   - in Default.frag the directional light's radiance is scaled by the fraction of a 2x2 bilinear
 *     depth compare (zref - depth_bias <= map) that passes, zref being the fragment's light-space depth;
 *     fragments outside the map are lit. Point lights and ambient are unchanged. */
typedef struct tri_shadow_config {
    uint32_t size;              /* map edge in texels (e.g. 2048); 0 disables the pre-pass         */
    uint32_t flags;             /* reserved, 0                                                      */
    float depth_bias;           /* light-NDC depth subtracted before the compare (e.g. 0.002)       */
    float slope_bias;           /* depthBiasSlopeFactor of the depth pass: each caster's depth is   *
                                 * raised by slope_bias * max(|dz/dx|, |dz/dy|) per texel (e.g. 2) */
    float light_view_proj[16];  /* column-major light ortho * light view                            */
} tri_shadow_config;

typedef struct tri_ctx tri_ctx;

/* ---- lifetime ---------------------------------------------------------------------------- */
/* Renderer::Init (Renderer.h:115, Renderer.cpp:587-648): allocates the colour/depth targets and
 * the default 1x1 white texture in slot 0 (Renderer.cpp:3404-3436). */
int tri_create(const tri_config* config, tri_ctx** out_ctx);
/* Renderer::Shutdown (Renderer.h:116). Null is accepted. */
int tri_destroy(tri_ctx* ctx);
/* Use an external hipStream_t (passed as void*) for every launch/copy; NULL = the context's own. */
int tri_set_stream(tri_ctx* ctx, void* hip_stream);
const char* tri_last_error(void);
int tri_abi_version(void);

/* ---- data upload (copies) ---------------------------------------------------------------- */
/* Renderer::UploadMesh / AppendMeshes -> UploadMeshFromCache (Renderer.h:120-121,
 * Renderer.cpp:1965-2116): one concatenated vertex buffer, one uint32 mesh-local index buffer and
 * one MeshDrawInfo per mesh. Replaces the whole geometry set. */
int tri_upload_geometry(tri_ctx* ctx, const tri_vertex* vertices, uint64_t vertex_count,
                        const uint32_t* indices, uint64_t index_count,
                        const tri_mesh_range* meshes, uint32_t mesh_count);
/* Shared geometry (the reference binds ONE vertex and index buffer for every viewport,
 * Renderer.cpp:1965-2116, :5095-5108): a tri_geometry holds the uploaded meshes on one device and any
 * number of contexts on that device reference it through tri_bind_geometry (NULL returns a context to
 * its own geometry, which tri_upload_geometry fills). Uploading to a shared geometry waits for the
 * device to go idle; contexts pick the new meshes up at their next tri_render. */
typedef struct tri_geometry tri_geometry;
int tri_geometry_create(int32_t device /* -1 = current */, tri_geometry** out_geometry);
int tri_geometry_upload(tri_geometry* geometry, const tri_vertex* vertices, uint64_t vertex_count,
                        const uint32_t* indices, uint64_t index_count, const tri_mesh_range* meshes,
                        uint32_t mesh_count);
int tri_geometry_destroy(tri_geometry* geometry); /* after every context using it is unbound/destroyed */
int tri_bind_geometry(tri_ctx* ctx, tri_geometry* geometry);

/* Material buffer payload (BuildMaterialPayload, Renderer.cpp:5927-5951). count 0 => the default
 * record {1,1,1,1},{1,1,1,0} (Renderer.cpp:5941-5943). */
int tri_upload_materials(tri_ctx* ctx, const tri_material_record* records, uint32_t count);
/* Texture slot upload (PopulateTextureSlot, Renderer.cpp:3469-3620): R8G8B8A8_SRGB texels,
 * row-major, rows already flipped by the loader (TextureLoader.cpp:290-304). slot < 256. */
int tri_upload_texture(tri_ctx* ctx, uint32_t slot, const uint8_t* rgba8_srgb, uint32_t width,
                       uint32_t height);
/* Bone palette SSBO (binding 4, PrepareBonePaletteBuffer Renderer.cpp:3168-3245):
 * column-major mat4s. */
int tri_upload_bone_palette(tri_ctx* ctx, const float* matrices, uint32_t matrix_count);

/* ---- skeletal poses evaluated on the device ------------------------------------------------------
 * The pose rules (Animation::AnimationPlayer::EvaluatePose, AnimationPlayer.cpp:141-341), stated once. The device
 * kernel (csrc/pose_eval.hip), the shim's CPU player (host/src/Animation.cpp) and the float64 restatement of the tests
 * (tests/anim_ref.py) each implement exactly this; the two float32 ones use the same IEEE operations in the same
 * order (no contraction), so they agree bit for bit wherever no library call (sin, acos) is evaluated.
 *
 * Quaternions are {w, x, y, z}; matrices are column-major glm::mat4. eps = FLT_EPSILON.
 *   dot(a, b)       = (a.w*b.w + a.x*b.x) + (a.y*b.y + a.z*b.z)
 *   normalize(q)    = len = sqrt(dot(q, q)); {1,0,0,0} when len <= 0, else q * (1 / len)
 *   clamp(x, 0, 1)  = min(max(x, 0), 1) with max(a,b) = a < b ? b : a and min(a,b) = b < a ? b : a
 *   mix(a, b, T)    = a*(1 - T) + b*T, per component
 *   slerp(a, b, T)  = c = dot(a, b); when c < 0: b = -b, c = -c; when c > 1 - eps: mix(a, b, T) per component;
 *                     otherwise A = acos(c) and (sin((1 - T)*A)*a + sin(T*A)*b) / sin(A) per component
 *   toMat4(q)       = glm::mat4_cast: column 0 = {1 - 2(yy + zz), 2(xy + wz), 2(xz - wy)}, column 1 =
 *                     {2(xy - wz), 1 - 2(xx + zz), 2(yz + wx)}, column 2 = {2(xz + wy), 2(yz - wx), 1 - 2(xx + yy)}
 *   A * B           = column j of the product is ((A0*B[j].x + A1*B[j].y) + A2*B[j].z) + A3*B[j].w
 *
 * Per-bone defaults: the decomposition of the bone's local bind transform (DecomposeBindTransform, :343-390):
 * translation = column 3; scale = the lengths of columns 0..2 (length(v) = sqrt((x*x + y*y) + z*z)); rotation =
 * normalize(quat_cast(columns / scale)), a column left undivided when its length is <= eps. The host computes this
 * once per skeleton: the library takes the decomposed defaults (tri_pose_bone), never the matrix.
 *
 * Channels: a clip's channels apply in order, and each track (translation, rotation, scale) of a channel that has at
 * least one key replaces the bone's current value, so per (bone, track) the last channel with keys wins;
 * tri_animset_add_clip resolves that. The caller resolves channel -> bone (ResolveChannelBoneIndex) and leaves out
 * the channels it cannot map.
 *
 * Sampling a track at time t (:287-341): no keys: the default. One key, or t <= time[0]: key 0. Otherwise the first i
 * with t < time[i+1]: d = time[i+1] - time[i], T = clamp(d > eps ? (t - time[i]) / d : 0, 0, 1), and the value is
 * mix(key[i], key[i+1], T) for vectors, normalize(slerp(key[i], key[i+1], T)) for quaternions. Otherwise the last
 * key. A quaternion taken from a single key or an end point is normalize(key). Key times are non-decreasing (for
 * those the reference's linear scan is an upper-bound search, which is what the kernel does); a track with
 * decreasing or non-finite times is refused.
 *
 * Local matrix: translate * toMat4(normalize(q)) * scale, evaluated as: column j (j < 3) = column j of
 * toMat4(normalize(q)) times scale[j] with w = 0, column 3 = {translation, 1}. For finite inputs glm's two products
 * give the same floats (every other term is an exact zero); only the sign of a zero entry can differ.
 *
 * Hierarchy (:209-277): the traversal starts at the root index when it is a bone, otherwise at every bone without
 * a parent, otherwise at bone 0; a start bone's global is identity * local (through the product above); a child's is
 * parent_global * local. A bone the traversal does not reach takes global = local (the reference leaves it at its
 * previous evaluation's value, which is local only on the first one: here it is always the fresh local). A reached
 * bone whose global equals the identity in all 16 entries takes local too (:270-273).
 * The traversal follows the parents (a bone's children are the bones that name it as their parent; the shim rebuilds
 * Bone::m_Children from the parents when an asset is registered, where the reference walks the child lists as given).
 * pose = global * inverse_bind. A parent graph with a cycle reachable from the start set, which the reference would
 * walk for ever, is refused when the skeleton is added.
 *
 * Time advance (AnimationPlayer::Update, :57-102) is the caller's: an instance carries the final sample time.
 *
 * Pose space (Animation::AnimationPoseUtilities, AnimationPose.cpp:153-225). A pose is, per bone, a translation, a
 * rotation quaternion and a scale; everything below is per bone: bone b of a result depends on bone b of its inputs
 * alone. Implemented three times like the rules above: k_pose_graph (csrc/pose_eval.hip), the shim's float32
 * interpreter (host/src/Animation.cpp, EvaluatePoseProgram) and float64 numpy (tests/anim_graph_ref.py).
 *   Rest pose (BuildRestPose): the bone's decomposed defaults, as tri_pose_bone carries them.
 *   Clip pose (SampleClipPose, :171-196): the rest pose with every track that has keys sampled at the time by the
 *     track rules above (SampleVectorKeys / SampleQuaternionKeys of AnimationPose.cpp:40-94 are the player's: the
 *     same branches, the same clamp, normalize on every sampled quaternion). The value the player holds before the
 *     local matrix's normalize: a default rotation is taken as stored.
 *   blend(base, target, weight, mask) (BlendPose, :198-211): W = clamp(weight, 0, 1); per bone F = clamp(W * m, 0, 1)
 *     with m the bone's mask weight, 1.0 without a mask (the product and the second clamp are evaluated then too);
 *     T = mix(base.T, target.T, F), S = mix(base.S, target.S, F), R = normalize(slerp(base.R, target.R, F)).
 *   additive(base, add, weight, mask) (AdditivePose, :213-225): F = weight * m, not clamped; per component
 *     T = base.T + add.T * F and S = base.S + add.S * F (an additive pose that holds rest scales adds them: the
 *     reference's behaviour, kept); R = normalize(slerp(base.R, base.R * normalize(add.R), F)), slerp taking F as it
 *     is, also outside [0, 1]. p * q is glm's quaternion product, each line left to right:
 *       w = p.w*q.w - p.x*q.x - p.y*q.y - p.z*q.z      x = p.w*q.x + p.x*q.w + p.y*q.z - p.z*q.y
 *       y = p.w*q.y + p.y*q.w + p.z*q.x - p.x*q.z      z = p.w*q.z + p.z*q.w + p.x*q.y - p.y*q.x
 *   A mask holds one weight per bone; a bone beyond its weights weighs 1.0 (AnimationMask::GetWeight).
 *   Compose (ComposeSkinningMatrices, :227-310): the local matrix of {T, R, S} by the closed form above (with its
 *     normalize(R)), then the hierarchy and global * inverse_bind as above. That function starts every evaluation
 *     from identity globals, so a bone the traversal does not reach takes its fresh local matrix (identity == global
 *     sends it there): the rule already chosen above. The traversal follows the parents.
 *
 * A pose program is a postfix sequence of tri_pose_op over a stack of poses, evaluated per bone:
 *   TRI_POSE_OP_REST   push the rest pose
 *   TRI_POSE_OP_CLIP   push the clip pose of clip `a` at time `f`
 *   TRI_POSE_OP_BLEND  pop target; top = blend(top, target, f, mask a or TRI_POSE_NO_MASK)
 *   TRI_POSE_OP_ADD    pop add;    top = additive(top, add, f, mask a or TRI_POSE_NO_MASK)
 * A valid program has 1..TRI_POSE_MAX_OPS operations, never pops below one entry for a BLEND / ADD (two are needed),
 * never holds more than TRI_POSE_STACK entries and ends with exactly one, which is composed into the palette. */
#define TRI_POSE_MAX_BONES 256      /* bones of one skeleton (ancestors beyond the palette slice still count)      */
#define TRI_POSE_PALETTE_BONES 128  /* an instance writes its first min(bones, 128) matrices                      *
                                     * (PrepareBonePaletteBuffer's clamp, Renderer.cpp:3168-3245)                 */
#define TRI_POSE_BIND 0xFFFFFFFFu   /* tri_pose_instance.clip: no clip, every bone at its defaults                */
#define TRI_POSE_MAX_INSTANCES 65536u
#define TRI_POSE_MAX_PALETTE (1u << 24) /* matrices a palette may hold                                            */
#define TRI_POSE_STACK 8            /* poses a program may hold at once                                           */
#define TRI_POSE_MAX_OPS 64         /* operations of one program                                                  */
#define TRI_POSE_NO_MASK 0xFFFFFFFFu /* tri_pose_op.a of a BLEND / ADD: every bone weighs 1.0                     */
#define TRI_POSE_OP_REST 0u
#define TRI_POSE_OP_CLIP 1u
#define TRI_POSE_OP_BLEND 2u
#define TRI_POSE_OP_ADD 3u

/* One bone: its parent (negative: none), the decomposed defaults and the inverse bind matrix. */
typedef struct tri_pose_bone {
    int32_t parent;
    uint32_t reserved[3];
    float translation[4]; /* xyz; w ignored */
    float rotation[4];    /* w, x, y, z     */
    float scale[4];       /* xyz; w ignored */
    float inverse_bind[16];
} tri_pose_bone;

/* One TransformChannel with its bone resolved: key ranges {first, count} into the clip's vector keys (translation,
 * scale) and quaternion keys (rotation). */
typedef struct tri_pose_channel {
    uint32_t bone;
    uint32_t translation_first, translation_count;
    uint32_t rotation_first, rotation_count;
    uint32_t scale_first, scale_count;
    uint32_t reserved;
} tri_pose_channel;

typedef struct tri_pose_instance {
    uint32_t skeleton;       /* from tri_animset_add_skeleton                                  */
    uint32_t clip;           /* from tri_animset_add_clip for that skeleton, or TRI_POSE_BIND  */
    float time;              /* sample time in seconds                                         */
    uint32_t palette_offset; /* first matrix of the instance's slice in the context's palette  */
} tri_pose_instance;

/* One operation of a pose program (above). */
typedef struct tri_pose_op {
    uint32_t op;       /* TRI_POSE_OP_*                                                              */
    uint32_t a;        /* CLIP: the clip; BLEND / ADD: the mask or TRI_POSE_NO_MASK; REST: ignored  */
    float f;           /* CLIP: the sample time in seconds; BLEND / ADD: the weight; REST: ignored  */
    uint32_t reserved;
} tri_pose_op;

/* One instance of tri_pose_graph: its program is ops[op_first .. op_first + op_count). */
typedef struct tri_pose_graph_instance {
    uint32_t skeleton;       /* from tri_animset_add_skeleton                                  */
    uint32_t op_first;
    uint32_t op_count;
    uint32_t palette_offset; /* first matrix of the instance's slice in the context's palette  */
} tri_pose_graph_instance;

/* A device-resident, append-only store of skeletons and clips on one device (-1: the current one). Adding validates
 * on the host, derives the traversal's level order and completes its upload before it returns; a destroy only after
 * every context that posed from the set is synchronised. Without a HIP device tri_animset_create is TRI_E_HIP. */
typedef struct tri_animset tri_animset;
int tri_animset_create(int32_t device, tri_animset** out);
int tri_animset_destroy(tri_animset* set);
/* TRI_E_INVALID: bone_count outside 1..TRI_POSE_MAX_BONES, a parent >= bone_count, a cycle reachable from the
 * traversal's start set. root_index outside 0..bone_count-1 means "no root". */
int tri_animset_add_skeleton(tri_animset* set, const tri_pose_bone* bones, uint32_t bone_count, int32_t root_index,
                             uint32_t* out_skeleton);
/* vector keys: vec_times[i], vec_values[3*i..]; quaternion keys: quat_times[i], quat_values[4*i..] = w, x, y, z.
 * TRI_E_INVALID: an unknown skeleton, a channel bone >= its bone count, a key range outside the arrays, key times
 * of a range not finite or decreasing, a duration that is not finite. */
int tri_animset_add_clip(tri_animset* set, uint32_t skeleton, const tri_pose_channel* channels, uint32_t channel_count,
                         const float* vec_times, const float* vec_values, uint32_t vec_count,
                         const float* quat_times, const float* quat_values, uint32_t quat_count, float duration,
                         uint32_t* out_clip);
/* Per-bone mask weights for a skeleton, append-only and uploaded like a clip. weight_count may differ from the bone
 * count: bones beyond it weigh 1.0, weights beyond the bones are dropped (weights may be NULL when it is 0).
 * TRI_E_INVALID: an unknown skeleton. */
int tri_animset_add_mask(tri_animset* set, uint32_t skeleton, const float* weights, uint32_t weight_count,
                         uint32_t* out_mask);

/* Evaluate `count` instances on the context's stream (k_pose), each writing its min(bones, TRI_POSE_PALETTE_BONES)
 * matrices at palette_offset of the context's bone palette. The palette is then the uploaded prefix (what the last
 * tri_upload_bone_palette put there; that call drops any posed suffix) followed by the posed suffix, which every
 * tri_pose_palette replaces; count 0 drops it. Matrices of the suffix that no instance covers are unspecified.
 * Stream-ordered like tri_render: no host synchronisation while the palette's capacity suffices (the records travel
 * through a pinned ring and may be overwritten when the call returns); growing the palette synchronises and keeps
 * the prefix. TRI_E_INVALID, before anything is enqueued: an instance below the prefix or beyond
 * TRI_POSE_MAX_PALETTE, two instances that overlap, an unknown skeleton or clip, a clip of another skeleton, a set
 * on another device, count above TRI_POSE_MAX_INSTANCES. */
int tri_pose_palette(tri_ctx* ctx, tri_animset* set, const tri_pose_instance* instances, uint32_t count);
/* tri_pose_palette with a pose program per instance (k_pose_graph): the same palette contract (the call replaces the
 * posed suffix, never writes the uploaded prefix, count 0 drops the suffix), the same stream order (instances and
 * operations travel through a pinned ring; both arrays may be overwritten when the call returns). Programs of several
 * instances may share or overlap ranges of `ops`. TRI_E_INVALID, before anything is enqueued: whatever
 * tri_pose_palette refuses, an op range outside `ops`, an invalid program (see the rules above), an unknown op, a
 * clip or mask that is unknown or belongs to another skeleton. */
int tri_pose_graph(tri_ctx* ctx, tri_animset* set, const tri_pose_graph_instance* instances, uint32_t count,
                   const tri_pose_op* ops, uint32_t op_count);
/* Blocking read of the palette's first matrix_count matrices (at most its current extent), for tests and tools. */
int tri_read_bone_palette(tri_ctx* ctx, float* out_matrices, uint32_t matrix_count);

/* Skybox cubemap (CreateSkyboxCubemap, Renderer.cpp:3818-4110; LoadFromFaces TextureLoader.cpp:
 * 334-830): 6 faces in Vulkan layer order +X,-X,+Y,-Y,+Z,-Z, each size x size RGBA8 sRGB texels, rows
 * top to bottom, one mip. The skybox pass (Skybox.cpp:13-79, Skybox.vert/.frag, cull FRONT, depth
 * LEQUAL without writes) then gives every uncovered pixel its sky colour instead of the clear colour.
 * faces = NULL or size = 0 removes the skybox. */
int tri_upload_skybox(tri_ctx* ctx, const uint8_t* faces_rgba8_srgb, uint32_t size);

/* The other cubemaps CreateSkyboxCubemap uploads (Renderer.cpp:3965-4097): R8G8B8A8_UNORM (no sRGB decode),
 * R16G16B16A16_SFLOAT, and a mip chain sampled with mipmapMode LINEAR, minLod 0, maxLod = mip_count.
 * texels: level-major, then face (+X,-X,+Y,-Y,+Z,-Z), then rows top to bottom; level l is max(1, size >> l) square; a
 * texel is 4 bytes (the two 8-bit formats) or 8 bytes (four binary16 values); alpha is ignored (Skybox.frag writes 1).
 * bytes must be the chain's exact size. A one-level TRI_SKY_FMT_RGBA8_SRGB cubemap without TRI_SKYBOX_PREFILL is
 * tri_upload_skybox itself. Every other cubemap is drawn by a pass of its own ahead of the frame's raster kernel
 * (k_sky_fill): per level the filtering of tri_upload_skybox (major-axis face, LINEAR, taps across edges from the
 * adjacent face, a corner tap the mean of the three texels meeting there); the level of detail by Vulkan's rules from
 * fine quad differences of the normalised direction (quads at even frame coordinates; a neighbour the sky does not
 * cover gives a zero derivative), the cube map derivative transformation on the pixel's own face,
 * lambda = clamp(log2 rho_max, 0, mip_count), d = min(lambda, mip_count - 1), a linear blend of levels floor(d) and
 * floor(d) + 1; clamp(c, 0, 1) is stored (no tone mapping). TRI_SKYBOX_PREFILL takes that pass for a one-level sRGB
 * cubemap too. texels = NULL removes the skybox. TRI_E_INVALID: a byte count that is not the chain's, a size of 0
 * or above 16384, more than floor(log2(size)) + 1 levels or none, an unknown format or flag. */
#define TRI_SKY_FMT_RGBA8_SRGB 0u
#define TRI_SKY_FMT_RGBA8_UNORM 1u
#define TRI_SKY_FMT_RGBA16F 2u
#define TRI_SKYBOX_PREFILL 0x1u
typedef struct {
    uint32_t format;    /* TRI_SKY_FMT_* */
    uint32_t size;      /* level 0 face edge */
    uint32_t mip_count; /* 1 .. floor(log2(size)) + 1 */
    uint32_t flags;     /* TRI_SKYBOX_PREFILL */
    const void* texels;
    uint64_t bytes;
} tri_skybox_desc;
int tri_upload_skybox_ex(tri_ctx* ctx, const tri_skybox_desc* desc);

/* Default.frag's AI frame-generation blend (Default.frag:182-191). The texture is what UploadAiInterpolationToGpu
 * (Renderer.cpp:1560-1700) fills and EnsureAiTextureResources (:1390-1500) creates: width x height R8G8B8A8_UNORM
 * texels (no sRGB decode), rows top to bottom, sampled LINEAR with CLAMP_TO_EDGE at level 0. A frame whose UBO has
 * AiBlendConfig.w > 0 and w' = clamp(AiBlendConfig.x, 0, 1) > 0 (UpdateUniformBuffer packs (strength, 1 / width,
 * 1 / height, 1) while the texture is ready, Renderer.cpp:5916-5925) replaces every mesh fragment's output c by
 * mix(c, texture(ai, gl_FragCoord.xy * AiBlendConfig.yz), w') before the UNORM store; the skybox pass does not
 * blend. rgba8 = NULL or a zero extent removes the texture (DestroyAiResources). Rendering a blending frame
 * without a texture is TRI_E_STATE; with the shadow pre-pass (not part of the reference) TRI_E_UNSUPPORTED. */
int tri_upload_ai_frame(tri_ctx* ctx, const uint8_t* rgba8_unorm, uint32_t width, uint32_t height);

/* Shadow-map pre-pass for the directional light (see tri_shadow_config). NULL or size 0 disables it
 * (the default: C1-C3 frames are exactly the reference's). size <= TRI_MAX_DIM. */
int tri_set_shadow(tri_ctx* ctx, const tri_shadow_config* config);
/* Host-only helper (no device): the orthographic light transform the shim fits for a shadow-casting
 * directional light travelling along `light_dir` (the UBO's DirectionalLightDirection) over the world
 * box [aabb_min, aabb_max]: glm::lookAtRH from 2 * radius behind the box centre, then glm::orthoRH_ZO
 * over the box corners in light view space (1% margin), so every corner lands inside the map. */
int tri_shadow_fit_ortho(const float light_dir[3], const float aabb_min[3], const float aabb_max[3],
                         float out_light_view_proj[16]);
/* Synchronous copy of the last rendered shadow map: size*size float32 depth bits, row j = light NDC y
 * increasing. TRI_E_STATE when no shadow pass is configured. */
int tri_read_shadow_map(tri_ctx* ctx, uint32_t* depth_bits);

/* ---- per frame --------------------------------------------------------------------------- */
/* UpdateUniformBuffer's vkCmdUpdateBuffer (Renderer.cpp:5958) + the colour clear value
 * (Renderer.cpp:5037-5050, SetClearColor Renderer.h:187). */
int tri_set_frame(tri_ctx* ctx, const tri_global_ubo* ubo, const float clear_rgba[4]);
/* The per-draw loop of RecordCommandBuffer (Renderer.cpp:5110-5151): draws in submission order. */
int tri_set_draws(tri_ctx* ctx, const tri_draw* draws, uint32_t draw_count);
/* Render into caller-owned device buffers (e.g. torch tensors for an RCCL all-gather):
 * colour = band_rows * width uint32 BGRA8 texels, depth = band_rows * width float32. NULL resets
 * to the context's own buffers. */
int tri_bind_output(tri_ctx* ctx, void* device_bgra8, void* device_depth);
/* Enqueue one frame on the context stream (asynchronous: vkQueueSubmit, Renderer.cpp:5679). */
int tri_render(tri_ctx* ctx);
/* Wait for the stream; reports TRI_E_OVERFLOW if a queued frame overflowed an internal buffer. */
int tri_synchronize(tri_ctx* ctx);
/* Frame readback (Renderer.cpp:5297-5338, :1299-1389): synchronous copy of the band, tightly packed
 * BGRA8 (width*4 bytes per row) and float32 depth bits. Either pointer may be NULL. */
int tri_readback(tri_ctx* ctx, uint8_t* bgra8, uint32_t* depth_bits);

/* The context's colour target as an opaque image handle: what Renderer::GetViewportTexture returns
 * instead of a VkDescriptorSet (Renderer.h:235; Forge shows it with ImGui::Image, GameViewportPanel.cpp:66,
 * SceneViewportPanel.cpp:139). Rows top to bottom, B8G8R8A8_UNORM; valid until the context is destroyed,
 * its output is rebound or its size changes; contents are those of the last completed tri_render. */
#define TRI_FORMAT_B8G8R8A8_UNORM 44u /* the VkFormat value of the reference's offscreen target */
typedef struct tri_image {
    void* device_ptr;     /* device memory on `device`                   */
    uint32_t width;
    uint32_t height;      /* rows of the context (its band)              */
    uint32_t pitch_bytes; /* bytes from one row to the next              */
    uint32_t format;      /* TRI_FORMAT_B8G8R8A8_UNORM                   */
    int32_t device;       /* HIP device ordinal                          */
    uint32_t reserved;
} tri_image;
int tri_get_output(tri_ctx* ctx, tri_image* out);

/* Presentation blit (Renderer.cpp:5346-5361: vkCmdBlitImage of the primary viewport's offscreen
 * target onto the swapchain image, VK_FILTER_LINEAR). Scales this context's B8G8R8A8 target to
 * width x height: each destination texel centre maps to the source by the extent ratio, the source
 * is filtered bilinearly on UNORM values with clamp-to-edge taps, and the result is rounded to UNORM8.
 * `dst` is a device pointer to width*height*4 bytes, or NULL for a context-owned present image that
 * tri_read_present copies out. Stream-ordered after the context's last tri_render. Whole frames only
 * (a row-band context returns TRI_E_STATE). */
int tri_blit_linear(tri_ctx* ctx, void* dst, uint32_t width, uint32_t height);
/* Synchronous copy of the context-owned present image of the last tri_blit_linear(ctx, NULL, w, h):
 * w*h*4 bytes of BGRA8. */
int tri_read_present(tri_ctx* ctx, uint8_t* bgra8);

/* ---- lossless 3-byte band transfer (multi-GPU assembly) ----------------------------
 * Replaces nothing in the reference (it has no multi-GPU path); it serves tri_group's and the bench's
 * gather onto the display GPU, whose inbound xGMI bytes bound the N = 8 frame rate.
 * tri_frame_alpha: the alpha byte EVERY pixel of the next tri_render of ctx will have, proven from the
 * context's state (material record 0, each draw's tint and texture slot, the clear colour, the skybox),
 * or -1 when it cannot be proven uniform. A band of such a frame can travel as 3 bytes per pixel. */
int tri_frame_alpha(tri_ctx* ctx, int32_t* alpha);
/* B8G8R8A8 (4 B/pixel, device pointer, 4-B aligned) <-> B, G, R bytes (3 B/pixel, device pointer),
 * stream-ordered on hip_stream (NULL = the null stream). pack: every alpha byte that differs from `alpha`
 * sets *flag (a device uint32, may be NULL) to nonzero — the transfer would not be lossless; unpack writes
 * `alpha` into every pixel. */
int tri_pack_bgr24(const void* bgra8, void* bgr8, uint64_t pixels, uint32_t alpha, uint32_t* flag, void* hip_stream);
int tri_unpack_bgr24(const void* bgr8, void* bgra8, uint64_t pixels, uint32_t alpha, void* hip_stream);
/* The delta bit-plane band format (lossless): the band as a 1-D pixel stream in slots of
 * TRI_DBP_SLOT_PIXELS pixels, each slot_bytes long (a multiple of 16, at least TRI_DBP_MIN_SLOT; TRI_DBP_MAX_SLOT
 * never overflows). Per 64-pixel block and channel, the bit width of the zigzag-mapped pixel-to-pixel differences and
 * that many 64-bit bit planes; alpha is dropped and restored as `alpha` (proven uniform, tri_frame_alpha).
 * tri_dbp_pack: flags[0] |= 1 when a pixel's alpha differs, |= 2 when a slot needed more than slot_bytes (that slot is
 * not decodable: grow slot_bytes and send again); flags[1] = max(flags[1], the largest slot's bytes) — the size the
 * next frames need. Both stream-ordered on hip_stream; stream buffers 16-B aligned, pixel buffers 4-B aligned.
 * tri_dbp_bytes: the stream's size for `pixels` pixels. */
#define TRI_DBP_SLOT_PIXELS 4096u
#define TRI_DBP_MIN_SLOT 176u
#define TRI_DBP_MAX_SLOT 12448u
int tri_dbp_pack(const void* bgra8, uint64_t pixels, uint32_t alpha, void* stream_out, uint32_t slot_bytes,
                 uint32_t* flags, void* hip_stream);
int tri_dbp_unpack(const void* stream_in, uint64_t pixels, uint32_t alpha, uint32_t slot_bytes, void* bgra8,
                   void* hip_stream);
uint64_t tri_dbp_bytes(uint64_t pixels, uint32_t slot_bytes);
/* tri_dbp_unpack of `count` (<= TRI_DBP_MAX_BANDS) streams with one slot size in one launch (the display device's
 * remote bands: a workgroup per slot of any of them); same alignment rules, bands of 0 pixels are skipped. */
#define TRI_DBP_MAX_BANDS 16u
int tri_dbp_unpack_bands(const void* const* streams_in, void* const* bgra8, const uint64_t* pixels, uint32_t count,
                         uint32_t alpha, uint32_t slot_bytes, void* hip_stream);

/* ---- viewport recording (Renderer::SetViewportRecordingEnabled / SubmitViewportFrame, Renderer.h:205-220) ----
 * The reference reads the frame back and converts it on the host (VideoEncoder::ConvertRgbaToYuv444,
 * VideoEncoder.cpp:716-736); here the conversion runs on the device behind the frame and the planes come back
 * through pinned memory while the next frames render.
 * tri_convert_yuv444: B8G8R8A8 (device pointer, 4-B aligned, rows pitch_bytes apart: a multiple of 4, at least
 * width * 4) -> 3 * width * height bytes at any alignment (device pointer): the Y plane, then U, then V, each
 * width * height bytes, rows top to bottom — one Y4M C444 FRAME payload. Per pixel, in IEEE double and this order:
 *   Y = 0.299 R + 0.587 G + 0.114 B,  U = -0.169 R - 0.331 G + 0.5 B + 128,  V = 0.5 R - 0.419 G - 0.081 B + 128,
 * clamped to [0, 255] and truncated (grey 128 gives Y = 127); alpha is ignored. Stream-ordered on hip_stream
 * (NULL = the null stream). Bytes beyond `width` in a pitched row are not read. */
int tri_convert_yuv444(const void* device_bgra8, uint32_t width, uint32_t height, uint32_t pitch_bytes,
                       void* device_yuv, void* hip_stream);
/* A recorder owns `slots` (1..8) device YUV buffers of one extent, as many pinned host buffers, a copy stream and
 * per-slot events, on one device (-1 = current). Each slot is idle or busy:
 *   tri_recorder_capture  (idle -> busy, asynchronous) on the context's stream, behind its last tri_render,
 *                         converts the colour target tri_bind_output currently binds into the slot, then copies it
 *                         to the slot's pinned buffer on the recorder's stream. TRI_E_STATE: a busy slot, a
 *                         row-band context (as tri_blit_linear); TRI_E_INVALID: a context of another extent or
 *                         on another device, a slot out of range.
 *   tri_recorder_wait     waits for the slot's copy and returns the pinned planes (tri_convert_yuv444's layout),
 *                         valid until the release. TRI_E_STATE for an idle slot.
 *   tri_recorder_release  (busy -> idle) first waits for a capture that has not finished, so the slot's next
 *                         capture cannot race the copy; releasing an idle slot is TRI_OK.
 * A frame that tri_synchronize reports as TRI_E_OVERFLOW was captured incomplete: release the slot and capture
 * again after the re-render. One host thread per recorder. Multi-device frames (tri_group) are out of scope: a
 * recorder captures single contexts only. tri_recorder_destroy waits for the captures in flight; NULL is TRI_OK. */
typedef struct tri_recorder tri_recorder;
int tri_recorder_create(int32_t device, uint32_t width, uint32_t height, uint32_t slots, tri_recorder** out);
int tri_recorder_destroy(tri_recorder* recorder);
int tri_recorder_capture(tri_recorder* recorder, uint32_t slot, tri_ctx* ctx);
int tri_recorder_wait(tri_recorder* recorder, uint32_t slot, const uint8_t** yuv);
int tri_recorder_release(tri_recorder* recorder, uint32_t slot);

/* ---- JPEG recording: the frame as a baseline JPEG, encoded on the device (Matroska V_MJPEG payloads) ----
 * A recorder created with TRI_RECORD_JPEG420 turns a frame into a complete JFIF stream instead of YUV planes: SOF0,
 * 8 bit, Y sampled 2 x 2 and Cb, Cr 1 x 1 (16 x 16 MCUs, extents padded by edge replication), JFIF full-range
 * BT.601, the T.81 Annex K quantisers scaled by `quality` (1..100, the IJG rule) and the Annex K Huffman tables, with
 * restart intervals of `restart_mcus` MCUs (1..65535; 0 = the library's default) that the device encodes in
 * parallel. The rule is integer arithmetic throughout (csrc/jpeg_math.h): the bytes are the same from the device and
 * from the host encoder. Three stages run on the capturing stream: pixels to quantised coefficients, one restart
 * interval per wave to stuffed bytes, and the gather of the intervals and their RSTn behind the header. Every
 * buffer is sized from the worst case (tri_jpeg_max_bytes), so no frame can overflow one.
 *   tri_recorder_create_ex     `params` NULL, or format TRI_RECORD_YUV444, is tri_recorder_create. TRI_E_INVALID: an
 *                              unknown format or flag bit, a quality or restart interval out of range.
 *   tri_recorder_capture       as above, for either format.
 *   tri_recorder_capture_image the same capture from any device image of the recorder's extent (B8G8R8A8, 4-B
 *                              aligned, rows pitch_bytes apart), ordered on hip_stream (NULL = the null stream); the
 *                              image must stay unchanged until the slot's wait returns. TRI_E_INVALID: a null image,
 *                              a pitch below 4 * width or not a multiple of 4.
 *   tri_recorder_wait_ex       waits for the slot and returns its product in pinned memory, valid until the release:
 *                              a JPEG recorder's stream, SOI to EOI, and its size (only the stream's own bytes,
 *                              rounded up to 256, cross the bus); a YUV444 recorder's planes with bytes = 3 w h.
 *   tri_recorder_wait          on a JPEG recorder is TRI_E_STATE.
 * tri_jpeg_header writes the stream's bytes before the first entropy-coded byte (SOI .. SOS; they depend only on the
 * extent, 1..65535 each, and the parameters) into `out`; tri_jpeg_max_bytes is the size no stream of that extent
 * and those parameters exceeds (0 with an error recorded for bad arguments). Both are host only and need no device. */
#define TRI_RECORD_YUV444 0u
#define TRI_RECORD_JPEG420 1u
typedef struct tri_record_params {
    uint32_t format;       /* TRI_RECORD_* */
    uint32_t quality;      /* JPEG: 1..100 */
    uint32_t restart_mcus; /* JPEG: 1..65535 MCUs per restart interval, 0 = default */
    uint32_t flags;        /* 0 */
} tri_record_params;
int tri_recorder_create_ex(int32_t device, uint32_t width, uint32_t height, uint32_t slots,
                           const tri_record_params* params, tri_recorder** out);
int tri_recorder_capture_image(tri_recorder* recorder, uint32_t slot, const void* device_bgra, uint32_t pitch_bytes,
                               void* hip_stream);
int tri_recorder_wait_ex(tri_recorder* recorder, uint32_t slot, const uint8_t** data, uint64_t* bytes);
int tri_jpeg_header(uint32_t width, uint32_t height, const tri_record_params* params, uint8_t* out, uint32_t capacity,
                    uint32_t* bytes);
uint64_t tri_jpeg_max_bytes(uint32_t width, uint32_t height, const tri_record_params* params);

/* ---- frame tensors for AI consumers (Renderer::SetReadbackEnabled / ResolvePendingReadback /
 * TryAcquireRenderedFrame, Renderer.cpp:984-995, :1111-1389) ----
 * The reference reads the primary viewport back and builds the frame generator's input on the host; here the
 * conversion runs on the device behind the frame, and the tensor can stay there for a consumer on the same device.
 * tri_convert_rgba_f32: B8G8R8A8 (device pointer, 4-B aligned, rows pitch_bytes apart: a multiple of 4, at least
 * width * 4) -> width * height * 4 floats, tightly packed, at a 4-B aligned device pointer (16-B aligned is faster):
 * channels-last, R, G, B, A per pixel (memory bytes 2, 1, 0, 3 of the source pixel), rows top to bottom. Every value
 * is exactly (float)byte * (1.0f / 255.0f): one float32 multiply by the constant 0x3B808081, not a division
 * (255 gives exactly 1.0f). Stream-ordered on hip_stream (NULL = the null stream). Bytes beyond `width` in a pitched
 * row are not read. Errors as tri_convert_yuv444, plus TRI_E_INVALID for an output that is not 4-B aligned. */
int tri_convert_rgba_f32(const void* device_bgra8, uint32_t width, uint32_t height, uint32_t pitch_bytes,
                         void* device_f32, void* hip_stream);
/* A grab is the tensor counterpart of tri_recorder, with the same slot protocol and error codes. It owns `slots`
 * (1..8) device tensors of one extent and per-slot events on one device (-1 = current); with TRI_GRAB_HOST_COPY it
 * also owns as many pinned host buffers and a copy stream (without the flag nothing ever crosses PCIe). Other flag
 * bits are TRI_E_INVALID.
 *   tri_framegrab_capture  (idle -> busy, asynchronous) on the context's stream, behind its last tri_render,
 *                          converts the colour target tri_bind_output currently binds into the slot's device tensor
 *                          (tri_convert_rgba_f32's layout and arithmetic); with TRI_GRAB_HOST_COPY it then copies
 *                          the tensor to the slot's pinned buffer on the grab's stream, behind an event.
 *                          TRI_E_STATE: a busy slot, a row-band context; TRI_E_INVALID: a context of another extent
 *                          or on another device, a slot out of range.
 *   tri_framegrab_wait     either out-pointer may be NULL (not both). `device` waits for the conversion and returns
 *                          the device tensor; `host` waits for the copy and returns the pinned tensor. Both stay
 *                          valid until the release. TRI_E_STATE for an idle slot, and for `host` on a grab created
 *                          without TRI_GRAB_HOST_COPY.
 *   tri_framegrab_release  (busy -> idle) first waits for a capture that has not finished, so the slot's next
 *                          capture cannot race the conversion or the copy; releasing an idle slot is TRI_OK.
 * A frame that tri_synchronize reports as TRI_E_OVERFLOW was captured incomplete: release the slot and capture
 * again after the re-render. One host thread per grab; single contexts only (no tri_group).
 * tri_framegrab_destroy waits for the captures in flight; NULL is TRI_OK. */
#define TRI_GRAB_HOST_COPY 1u
typedef struct tri_framegrab tri_framegrab;
int tri_framegrab_create(int32_t device, uint32_t width, uint32_t height, uint32_t slots, uint32_t flags,
                         tri_framegrab** out);
int tri_framegrab_destroy(tri_framegrab* grab);
int tri_framegrab_capture(tri_framegrab* grab, uint32_t slot, tri_ctx* ctx);
int tri_framegrab_wait(tri_framegrab* grab, uint32_t slot, const float** host, const float** device);
int tri_framegrab_release(tri_framegrab* grab, uint32_t slot);

/* ---- the frame generator (AI::FrameGenerator's InterpolationUNet, Renderer::ProcessAiFrame, Renderer.cpp:839-982) ----
 * The reference runs the network in an ONNX Runtime session on the host side of a readback. Here its 20 convolutions
 * are HIP kernels on the f32-input matrix cores, float32 throughout, on channels-last ([H, W, C]) device tensors.
 *
 * tri_nn_conv is one layer: an implicit GEMM (M = the output pixels of a spatial tile, N = output channels,
 * K = taps x input channels) with the epilogue
 *     y = act(acc * scale[c] + shift[c] + res1) + res2
 * where res1 and res2 (output-shaped tensors) may be NULL. A bias is scale 1, shift = bias; an eval-mode BatchNorm is
 * scale = gamma / sqrt(var + 1e-5), shift = beta - mean * scale.
 *   TRI_NN_CONV3X3   3 x 3, padding 1, stride 1 or 2: the output is ceil(H / stride) x ceil(W / stride).
 *   TRI_NN_CONVT4X4  torch's ConvTranspose2d(kernel 4, stride 2, padding 1): the output is 2H x 2W; stride must be 2.
 * packed_weights is what tri_nn_pack_weights (host only, no device) makes of torch's layout — Conv2d
 * [Cout][Cin][3][3], ConvTranspose2d [Cin][Cout][4][4] — the same number of floats: [ky][kx][ci][co], and for the
 * transposed convolution [output parity y][x][tap a][b][ci][co] with ky = 1 - py + 2a, kx = 1 - px + 2b (no flip).
 * Every pointer of tri_nn_conv is device memory of the current device, 4-B aligned; the launch is stream-ordered on
 * hip_stream (NULL = the null stream). TRI_E_INVALID: a null or misaligned pointer, an unknown op, stride or
 * activation, an extent outside 1..TRI_MAX_DIM, channels outside 1..TRI_NN_MAX_CHANNELS. */
#define TRI_NN_CONV3X3 0u
#define TRI_NN_CONVT4X4 1u
#define TRI_NN_ACT_NONE 0u
#define TRI_NN_ACT_RELU 1u
#define TRI_NN_ACT_SIGMOID 2u
#define TRI_NN_MAX_CHANNELS 1024
typedef struct tri_nn_conv_desc {
    uint32_t op;           /* TRI_NN_CONV3X3 / TRI_NN_CONVT4X4 */
    uint32_t stride;       /* 1 or 2 (the transposed convolution: 2) */
    uint32_t in_height;
    uint32_t in_width;
    uint32_t in_channels;
    uint32_t out_channels;
    uint32_t activation;   /* TRI_NN_ACT_* */
    uint32_t reserved;     /* 0 */
} tri_nn_conv_desc;
int tri_nn_pack_weights(const tri_nn_conv_desc* desc, const float* torch_weights, float* packed_weights);
int tri_nn_conv(const tri_nn_conv_desc* desc, const void* input, const void* packed_weights, const void* scale,
                const void* shift, const void* res1, const void* res2, void* output, void* hip_stream);

/* A generator owns the network's weights and every activation for one frozen extent on one device (-1 = current),
 * and a stream of its own at the device's lowest priority (the job runs behind the frames: their kernels do not queue
 * behind its workgroups). `weights` is a weights container (tools/export_frame_generator.py writes it from
 * a checkpoint) in host memory. width and height are multiples of 4 within 4..TRI_MAX_DIM (two stride-2 levels with
 * additive skips); the container's input channels are 1..8; the output is [height][width][3].
 *   tri_framegen_submit   copies device_input_nhwc ([height][width][input channels] floats on the generator's device)
 *                         into the generator's own buffer on producer_stream (NULL = the null stream), so later work on
 *                         that stream may reuse the source, then runs the 20 layers on the generator's stream behind an
 *                         event. One job at a time: TRI_E_STATE while a job is in flight, which it is from the submit
 *                         until tri_framegen_poll reports it done or tri_framegen_wait returns.
 *   tri_framegen_poll     never blocks. *done = 1 once per job, when it has finished; 0 otherwise (also before any
 *                         submit).
 *   tri_framegen_wait     blocks until the job in flight has finished. TRI_E_STATE when nothing was ever submitted.
 *                         A device error in poll or wait (TRI_E_HIP) loses the job: the generator's stream is drained,
 *                         there is no output, and the next submit is accepted.
 *   tri_framegen_output   the device tensor of the last finished job; TRI_E_STATE before one has finished or while a
 *   tri_framegen_read_output   job is in flight (the layers are writing it). read_output copies it to the host.
 *   tri_framegen_last_ms  device time of the last finished job, between events around its 20 launches.
 * TRI_E_INVALID: a bad extent, a damaged container (the message names the tensor); TRI_E_OOM: an allocation failed.
 * tri_framegen_destroy waits for a job in flight; NULL is TRI_OK. One host thread per generator. */
typedef struct tri_framegen tri_framegen;
int tri_framegen_create(int32_t device, const void* weights, uint64_t bytes, uint32_t width, uint32_t height,
                        tri_framegen** out);
int tri_framegen_destroy(tri_framegen* gen);
int tri_framegen_info(const tri_framegen* gen, uint32_t* input_channels, uint32_t* width, uint32_t* height);
int tri_framegen_submit(tri_framegen* gen, const void* device_input_nhwc, void* producer_stream);
int tri_framegen_poll(tri_framegen* gen, int32_t* done);
int tri_framegen_wait(tri_framegen* gen);
int tri_framegen_output(tri_framegen* gen, const float** device_hw3);
int tri_framegen_read_output(tri_framegen* gen, float* host_hw3);
int tri_framegen_last_ms(tri_framegen* gen, float* ms);

/* tri_upload_ai_frame for a tensor that is already on the context's device: [height][width][channels] floats in
 * [0, 1], channels 1..4. A kernel on the context's stream (behind the frames already queued, which still sample the
 * previous texture) packs it into the R8G8B8A8 blend frame by the rules of the host path
 * (NormaliseAndReorderAiOutput + UploadAiInterpolationToGpu's packing, Renderer.cpp:358-415, :1572-1590), bit for bit:
 * channels 0 and 2 swapped when there are at least 3, clamp to [0, 1], round(v * 255.0f) half away from zero, alpha
 * 255 (and the other missing channels 0) when absent. The host path's 1/255 rescale of tensors beyond [0, 1] is not
 * applied. With `behind` non-NULL the context's stream first waits for that generator's last submitted job (the
 * tensor is usually its output), and the generator's next job waits for this kernel before it overwrites the tensor.
 * tri_read_ai_frame copies the blend frame (width * height * 4 bytes) to the host after the context's stream has
 * drained; TRI_E_STATE without one. */
int tri_upload_ai_frame_device(tri_ctx* ctx, const void* device_nhwc, uint32_t width, uint32_t height,
                               uint32_t channels, tri_framegen* behind);
int tri_read_ai_frame(tri_ctx* ctx, uint8_t* rgba8);
/* The stream the context currently enqueues on (its own, or tri_set_stream's) as a hipStream_t: what a producer hands
 * to tri_framegen_submit so that the copy of a tensor the context made is ordered with the context's later frames. */
int tri_get_stream(tri_ctx* ctx, void** hip_stream);

/* ---- text overlay (Renderer::SubmitText -> TextRenderer::QueueText / RecordViewport, Text.vert / Text.frag) ----
 * The reference draws queued text inside the viewport's render pass, after the sprites: one textured quad per glyph
 * (6 vertices of TextVertex), cull NONE, no depth test or write, blend SRC_ALPHA / ONE_MINUS_SRC_ALPHA for colour and
 * ONE / ONE_MINUS_SRC_ALPHA for alpha. Here tri_render appends the same pass on the context's stream whenever quads
 * are set, so everything that takes the colour target after the frame (tri_readback, tri_blit_linear,
 * tri_recorder_capture, tri_framegrab_capture, tri_xfer_frame, the group's assembly) sees the overlay. The pass,
 * exactly (float32 unless stated):
 *   - each corner snaps as X = (int32_t)rintf(x * 256.0f) (the main pass's 8-bit snap), after x * 256.0f is pinned to
 *     [-2^29, 2^29] (2^21 pixels, 256 times TRI_MAX_DIM: the differences of snapped values then fit int32; a quad
 *     reaching further is drawn as if it ended there, tx and ty included); a quad with x1 < x0 (y1 < y0) is drawn
 *     mirrored: its corners swap together with their u (v);
 *   - pixel (px, py) is covered iff X0 <= px * 256 + 128 < X1 and Y0 <= py * 256 + 128 < Y1 (the top-left rule of the
 *     quad's two triangles; a zero-area quad covers nothing);
 *   - tx = (float)(px * 256 + 128 - X0) / (float)(X1 - X0), u = u0 + tx * (u1 - u0), v likewise;
 *   - alpha = the atlas (byte / 255.0f) sampled LINEAR, CLAMP_TO_EDGE, level 0 at (u, v) (x = u * width - 0.5);
 *   - src = clamp((r, g, b, a) * alpha, 0, 1); out.rgb = src.rgb * src.a + dst.rgb * (1 - src.a),
 *     out.a = src.a + dst.a * (1 - src.a): the colour is multiplied by alpha twice, as the reference's is;
 *   - quads blend in submission order, and after every quad the pixel is rounded to B8G8R8A8_UNORM
 *     (clamp, * 255 + 0.5, truncate); the next quad reads byte / 255.0f. Pixels no quad covers are not written;
 *     depth is neither read nor written.
 * A tri_font is the atlas's alpha plane on one device (the reference uploads RGBA with RGB = 255 and samples .a only,
 * TextRenderer.cpp:374-379): width, height in 1..TRI_MAX_DIM, rows top to bottom. device -1 = the current device.
 * tri_font_destroy only after every context that uses the font dropped it (tri_set_text with another font, NULL or
 * count 0, or tri_destroy); NULL is TRI_OK.
 * The pass runs behind the frame's last timing stamp: tri_timing (ms_frame and the stages) does not include it. */
typedef struct tri_font tri_font;
int tri_font_create(int32_t device, const uint8_t* alpha, uint32_t width, uint32_t height, tri_font** out);
int tri_font_destroy(tri_font* font);

/* One glyph quad (TextRenderer::RecordViewport's 6 vertices, TextRenderer.cpp:144-193). */
typedef struct tri_text_quad {
    float x0, y0, x1, y1; /* viewport pixels, full-frame coordinates, y down          */
    float u0, v0, u1, v1; /* normalised atlas coordinates at (x0, y0) / (x1, y1)      */
    float rgba[4];        /* TextVertex::m_Color                                       */
} tri_text_quad;
#define TRI_MAX_TEXT_QUADS 65536u

/* The quads every following tri_render of ctx composites over its frame, until the next tri_set_text. The array is
 * copied (free on return; safe with frames in flight). count == 0 or font == NULL removes the overlay. A row-band
 * context takes the same full-frame coordinates and composites its own rows only (also under tri_bind_output).
 * While quads are set, tri_frame_alpha reports -1 (text changes the alpha channel). TRI_E_INVALID — the previous
 * text stays — for null quads with a non-zero count, a count above TRI_MAX_TEXT_QUADS, a non-finite coordinate, a
 * font on another device. */
int tri_set_text(tri_ctx* ctx, tri_font* font, const tri_text_quad* quads, uint32_t count);

/* ---- entity ids: per-pixel draw ids, picking, selection outlines ---------------------------- */
/* With the id output on, every tri_render also writes, per pixel of the context's rows, which draw owns the pixel:
 * 0 for background (clear colour, skybox, text), else 1 + the index, in the array passed to tri_set_draws, of the draw
 * whose fragment won the depth test (LESS_OR_EQUAL in primitive order: among coincident fragments the last draw wins,
 * as in the colour target). A skipped draw (bad mesh index) keeps its index and owns no pixel. The pass is a kernel
 * of its own (k_id_raster) between the frame's set-up and its raster kernel: it re-resolves visibility from the same
 * bin queues with the same depth keys and shades nothing; colour and depth are bit-identical with the output on or
 * off. tri_timing's layout and meaning are unchanged: a timed frame stamps the pass with two events of its own, its
 * time is taken out of the stage it runs in (ms_setup, or ms_shadow with the pre-pass) and reported by
 * tri_get_id_timing; ms_frame contains it. A frame that reports TRI_E_OVERFLOW has invalid ids like its colour;
 * re-render it.
 * The readers synchronise (as tri_readback, TRI_E_OVERFLOW included) and answer for the last tri_render; TRI_E_STATE
 * with the output off or before a frame was rendered with it on. Coordinates are full-frame pixels, y down. */
#define TRI_FORMAT_R32_UINT 98u /* VK_FORMAT_R32_UINT: tri_image.format of the id image */
/* Allocates (enable != 0) or frees width x rows uint32. Switching it off also removes the outline. */
int tri_set_id_output(tri_ctx* ctx, int enable);
/* width x rows ids, tightly packed. */
int tri_read_ids(tri_ctx* ctx, uint32_t* ids);
/* The id image in device memory (pitch width * 4, TRI_FORMAT_R32_UINT): contents are those of the last completed
 * tri_render, valid until the next one or until the output is switched off. */
int tri_get_id_output(tri_ctx* ctx, tri_image* out);
typedef struct tri_pick_result {
    uint32_t id;         /* 0 = background, else the caller's draw index + 1       */
    uint32_t depth_bits; /* the pixel's float32 depth bits (0 without has_depth)   */
    uint32_t has_depth;  /* 0 under TRI_FLAG_NO_DEPTH_OUTPUT                       */
    uint32_t reserved;
} tri_pick_result;
/* One pixel (copies 4 + 4 bytes, not the buffers). TRI_E_INVALID outside the context's rows. */
int tri_pick(tri_ctx* ctx, int32_t x, int32_t y, tri_pick_result* out);
/* The distinct draws inside the inclusive rectangle (x0, y0)-(x1, y1), clamped to the context's rows: bit d of
 * draw_bits (word d / 32, bit d % 32) is set iff some pixel there has id d + 1; *distinct (may be NULL) is their
 * number. word_count >= ceil(draw_count / 32) of the last rendered draw list, else TRI_E_INVALID, as for reversed
 * corners; a rectangle that misses the rows reports none. Gathered on the device (k_id_collect). */
int tri_pick_rect(tri_ctx* ctx, int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint32_t* draw_bits, uint32_t word_count,
                  uint32_t* distinct);
/* The selection outline: after the frame's raster kernel and before the text pass, tri_render composites `rgba` over
 * every outline pixel. With S(p) = 1 iff id(p) >= 1 and draw id(p) - 1 is in `draws`, pixel p is an outline pixel iff
 * S(p) = 0 and some pixel q of the context's rows with max(|dx|, |dy|) <= width_px has S(q) = 1 (an outer outline of
 * the visible silhouette). The composite is the text pass's blend at coverage 1: src = clamp(rgba, 0, 1),
 * out.rgb = src.rgb * src.a + dst.rgb * (1 - src.a), out.a = src.a + dst.a * (1 - src.a), rounded to UNORM8
 * (alpha 1 stores the colour's bytes exactly); every other pixel is untouched. */
typedef struct tri_outline {
    const uint32_t* draws; /* indices into the tri_set_draws array (copied)     */
    uint32_t draw_count;   /* 0: nothing selected, nothing drawn                 */
    float rgba[4];
    uint32_t width_px;     /* 1..8                                               */
    uint32_t reserved;
} tri_outline;
/* Stays set until the next call, like tri_set_text; NULL removes it. Needs the id output (TRI_E_STATE without it).
 * TRI_E_INVALID: width_px outside 1..8, a non-finite colour, a draw index >= the current draw count (indices that a
 * later, shorter draw list leaves dangling select nothing). TRI_E_UNSUPPORTED on a context that renders a row band:
 * the outline's halo lies in other bands. */
int tri_set_outline(tri_ctx* ctx, const tri_outline* outline);
/* The id pass's own event timing over the frames tri_set_timing timed since it was last set: *ms_id the summed
 * milliseconds of k_id_raster, *frames how many timed frames ran it (synchronizes, like tri_get_timing). */
int tri_get_id_timing(tri_ctx* ctx, double* ms_id, uint64_t* frames);

/* ---- motion vectors: per-pixel screen-space motion from ids and depth ------------------------ */
/* With the motion output on (it needs the id output), every tri_render also writes two float32 per pixel of the
 * context's rows: m(p) = prev(p) - p in pixels, where the surface point visible at pixel p lay one frame ago (x right,
 * y down). k_motion, a streaming kernel of its own after the frame's raster kernel, reads the pixel's id and depth and
 * one 4 x 4 reprojection matrix per draw; no other kernel of the frame changes, and colour, depth and ids are
 * bit-identical with the output on or off. With R the matrix of the pixel's draw (row id(p) of the table
 * tri_motion_matrices builds; row 0 for the background) and W x H the frame, in float32 and in exactly this order:
 *     fx = (float)x + 0.5f             fy = (float)y + 0.5f            (y: the full-frame row)
 *     xn = fx * sx - 1.0f              yn = fy * sy - 1.0f             sx = 2.0f / (float)W, sy = 2.0f / (float)H
 *     z  = id(p) ? depth(p) : 1.0f
 *     q_i = ((R[i][0] * xn + R[i][1] * yn) + R[i][2] * z) + R[i][3]    for i = 0, 1, 3
 *     q_3 > 0.0f:  iw = 1.0f / q_3,  m.x = (q_0 * iw - xn) * (0.5f * W),  m.y = (q_1 * iw - yn) * (0.5f * H)
 *     otherwise (NaN, or the point lay behind the previous camera) m = (0, 0); a pair with a non-finite component is
 *     stored as (0, 0).
 * No multiply-add is contracted and the divide is correctly rounded, so a float32 restatement gives the same bits.
 * Skinned draws get the rigid motion of their model matrix. A frame that reports TRI_E_OVERFLOW has invalid motion
 * like its colour; re-render it. tri_timing's layout and meaning are unchanged: a timed frame stamps the pass with two
 * events of its own, its time is taken out of ms_raster and reported by tri_get_motion_timing; ms_frame contains it. */
#define TRI_FORMAT_R32G32_SFLOAT 103u /* VK_FORMAT_R32G32_SFLOAT: tri_image.format of the motion image */
typedef struct tri_motion_history {
    float prev_view[16];        /* as tri_global_ubo.view / .projection, of the previous frame            */
    float prev_projection[16];
    const float* prev_models;   /* draw_count x 16 floats: the model each draw of the CURRENT tri_set_draws *
                                 * array had in the previous frame; NULL: every draw keeps its current one  */
    uint32_t draw_count;        /* with prev_models: must equal the draw count at tri_render                */
    uint32_t reserved;
} tri_motion_history;
/* Allocates (enable != 0) or frees width x rows x 2 floats. TRI_E_STATE without the id output (switching that off
 * also switches this off); TRI_E_UNSUPPORTED on a context created with TRI_FLAG_NO_DEPTH_OUTPUT. Row-band contexts
 * are supported: the pass has no halo. */
int tri_set_motion_output(tri_ctx* ctx, int enable);
/* The previous frame's camera and models, copied; stays until replaced. NULL: no history, all motion zero.
 * TRI_E_INVALID for prev_models with a draw_count of 0. tri_render reports TRI_E_STATE while the motion output is on
 * and a stored prev_models count differs from the frame's draw count. */
int tri_set_motion_history(tri_ctx* ctx, const tri_motion_history* history);
/* width x rows x 2 floats, tightly packed, x then y. Synchronises and reports TRI_E_OVERFLOW like tri_read_ids;
 * TRI_E_STATE with the output off or before a frame was rendered with it on. */
int tri_read_motion(tri_ctx* ctx, float* xy);
/* The motion image in device memory (pitch width * 8, TRI_FORMAT_R32G32_SFLOAT), valid like tri_get_id_output's. */
int tri_get_motion_output(tri_ctx* ctx, tri_image* out);
/* As tri_get_id_timing, for k_motion. */
int tri_get_motion_timing(tri_ctx* ctx, double* ms_motion, uint64_t* frames);
/* The reprojection table tri_render stages for k_motion, (draw_count + 1) x 16 floats: out[16 k + 4 i + j] = R_k[i][j],
 * R_0 for the background and R_{d+1} for draws[d]. With P, V the uniform block's projection and view, M_d the first
 * 64 bytes of the draw's push constant and primes for the history's values,
 *     R_{d+1} = (P' V' M'_d) inverse(P V M_d),        R_0 = (P' V'_0) inverse(P V_0),
 * V_0 being V with its translation column replaced by (0, 0, 0, 1) (the background lies at infinity; the kernel
 * applies R_0 at z = 1). Computed in float64 and rounded once. A row is the exact identity when the current and the
 * previous matrices are bitwise equal, when P V M_d is singular or non-finite, when the row would hold a non-finite
 * entry, and — every row — when history is NULL. Host only: no device, no context. TRI_E_INVALID for a null ubo or
 * out, null draws with draw_count > 0, prev_models with a count of 0 or one that differs from draw_count. */
int tri_motion_matrices(const tri_global_ubo* ubo, const tri_draw* draws, uint32_t draw_count,
                        const tri_motion_history* history, float* out);

/* ---- history reprojection: the last frame warped by motion, with a disocclusion mask ---------- */
/* A tri_history keeps the previous frame of one view — colour, ids and depth — outside any context, so it survives
 * frames in flight that are separate contexts as well as a single context that overwrites itself. After a tri_render
 * with the motion output on, tri_history_reproject enqueues k_reproject on the context's stream: per pixel it fetches
 * the previous frame's colour where the motion vector points, says in a mask byte where that fetch is not valid, and
 * stores the frame just rendered as the next call's previous frame. No kernel of the frame changes; the context's
 * colour, depth, ids and motion are bit-identical with and without the pass.
 * The rule, for pixel p = (x, y) with current id i, depth d and colour c (4 bytes, B G R A), R the row of the motion
 * table tri_render staged for i, I', D', C' the stored previous frame and W x H the frame; float32, no multiply-add
 * contracted, in exactly this order:
 *     fx, fy, xn, yn, z, q_0, q_1, q_3, iw, m.x, m.y   exactly as under "motion vectors" (m is what k_motion stores)
 *     q_2  = ((R[2][0] * xn + R[2][1] * yn) + R[2][2] * z) + R[2][3]
 *     proj = q_3 > 0.0f and m.x, m.y finite before their zeroing
 *     u = fx + m.x       v = fy + m.y                   the previous position, pixel centres at + 0.5
 *     inside = proj && u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H
 *     xi = (int)floorf(u)    yi = (int)floorf(v)        only when inside
 *     i' = I'[yi][xi]        d' = i' ? D'[yi][xi] : 1.0f          zp = q_2 * iw
 * The mask byte (at most one bit is set):
 *     TRI_REPROJECT_NO_HISTORY  the object holds no previous frame; the mask is then exactly 1 on every pixel
 *     TRI_REPROJECT_NO_PROJ     !proj
 *     TRI_REPROJECT_OUTSIDE     proj && !inside
 *     TRI_REPROJECT_ID          inside && i' != i
 *     TRI_REPROJECT_DEPTH       inside && i' == i && i != 0 && depth_tolerance > 0 && !(fabsf(zp - d') <= depth_tolerance)
 * The warped colour where the mask is 0: with su = u - 0.5f, sv = v - 0.5f, x0 = floorf(su), y0 = floorf(sv),
 * fu = su - x0, fv = sv - y0 and the taps (x0, y0) (x0+1, y0) (x0, y0+1) (x0+1, y0+1) of C', each coordinate clamped
 * to the frame, per channel as float:  t = c00 * (1.0f - fu) + c10 * fu,  b = c01 * (1.0f - fu) + c11 * fu,
 * r = t * (1.0f - fv) + b * fv,  out = min((int)(r + 0.5f), 255). Where the mask is not 0 it is c, unchanged. A tap is
 * taken whatever id it has.
 * The colour is read as the context holds it when the call is enqueued: after the selection outline and the text
 * overlay. A caller who wants clean history leaves them off that frame. One host thread per object. */
#define TRI_FORMAT_R8_UINT 13u /* VK_FORMAT_R8_UINT: tri_image.format of the mask image */
#define TRI_REPROJECT_NO_HISTORY 1u
#define TRI_REPROJECT_NO_PROJ 2u
#define TRI_REPROJECT_OUTSIDE 4u
#define TRI_REPROJECT_ID 8u
#define TRI_REPROJECT_DEPTH 16u
#define TRI_HISTORY_REDO 1u /* tri_reproject_params.flags: the frame of the last call, rendered again */
typedef struct tri_history tri_history;
typedef struct tri_reproject_params {
    float depth_tolerance; /* >= 0 and finite, in depth-buffer units; 0: no depth test */
    uint32_t flags;        /* 0 or TRI_HISTORY_REDO */
    uint32_t reserved[2];
} tri_reproject_params;
/* Two sets of {colour, ids, depth} (12 B per pixel each), the warped colour (4 B), the mask (1 B) and the object's
 * events, on one device (-1 = current). TRI_E_INVALID for a zero extent or more than 2^31 pixels, before any device
 * is touched. tri_history_destroy waits for the last pass; NULL is TRI_OK. */
int tri_history_create(int32_t device, uint32_t width, uint32_t height, tri_history** out);
int tri_history_destroy(tri_history* history);
/* Asynchronous, on the context's stream behind the tri_render whose frame it reads (and behind the object's previous
 * pass, which may have run on another context's stream). The sets swap at the start of the NEXT call: that call reads
 * what this one stored — unless it carries TRI_HISTORY_REDO, which reads the same previous set again and overwrites
 * what this call stored (for a frame re-rendered after TRI_E_OVERFLOW). On an object that has not been reprojected
 * since its creation or tri_history_reset, a redo is a plain call.
 * TRI_E_INVALID: a null argument, a context on another device or of another extent, a negative or non-finite
 * tolerance, unknown flag bits. TRI_E_UNSUPPORTED: a row-band context (the fetch leaves the band). TRI_E_STATE: the
 * context's motion output is off, or no frame has been rendered with it. Every check comes before the device is made
 * current. While a timed frame is wanted of the context (tri_set_timing), the pass is stamped by two events of the
 * object's own whenever the previous stamps have been collected. */
int tri_history_reproject(tri_history* history, tri_ctx* ctx, const tri_reproject_params* params);
/* Forget the stored frame: the next call reports TRI_REPROJECT_NO_HISTORY everywhere (and a redo is a plain call). */
int tri_history_reset(tri_history* history);
/* The last pass's warped colour (width x height x 4 bytes, B G R A) and mask (width x height bytes), tightly packed;
 * either pointer may be NULL. Waits for the pass. TRI_E_STATE before the first pass. */
int tri_history_read(tri_history* history, uint8_t* bgra8, uint8_t* mask);
/* The two images in device memory: the colour as the context's (TRI_FORMAT_B8G8R8A8_UNORM, pitch width * 4), the mask
 * as TRI_FORMAT_R8_UINT with pitch width. Either pointer may be NULL. Valid until the object is destroyed; contents
 * are those of the last completed pass. TRI_E_STATE before the first pass. */
int tri_history_get_output(tri_history* history, tri_image* colour, tri_image* mask);
/* The summed milliseconds of the stamped passes and their number (waits for the last stamped pass). tri_timing is
 * untouched: the pass runs behind the frame's last stamp. */
int tri_history_get_timing(tri_history* history, double* ms, uint64_t* passes);

/* ---- temporal anti-aliasing: jittered frames resolved over clamped, accumulated history -------- */
/* The raster samples a pixel once, at its centre. A caller who moves that sample inside the pixel from frame to frame
 * (tri_taa_jitter, tri_taa_jitter_projection) and accumulates the frames gets the pixel's area instead. A tri_taa keeps
 * the accumulated colour of one view — 16-bit UNORM, so that a weight of 0.1 still moves it by one step — and the ids
 * it was accumulated under, twice, outside any context like a tri_history. After a tri_render with the motion output
 * on, tri_taa_resolve enqueues k_taa_resolve on the context's stream: per pixel it fetches the accumulated history where
 * the motion table says the surface lay, clamps it to the range of the current frame's 3 x 3 neighbourhood (stale
 * history cannot ghost), mixes the current colour in with weight alpha, and stores the sum as the next history and,
 * rounded to 8 bits, as the resolved image. No kernel of the frame changes; the context's colour, depth, ids and motion
 * are bit-identical with and without the pass.
 * The rule, for pixel p = (x, y) with current colour c (4 bytes, B G R A), id i and depth d, R the row of the motion
 * table tri_render staged for i, A' the previous accumulated colour (four uint16 per pixel, B G R A), I' the previous
 * ids and W x H the frame; integers and float32, no multiply-add contracted, in exactly this order:
 *     u, v, proj, inside, xi, yi and the four taps with fu, fv      exactly as under "history reprojection"
 *     TRI_TAA_NO_HISTORY  the object holds no previous frame; the mask is then exactly 1 on every pixel
 *     TRI_TAA_NO_PROJ     !proj                      TRI_TAA_OUTSIDE     proj && !inside
 *     TRI_TAA_ID          with TRI_TAA_REJECT_ID, inside, and none of I'[clamp(yi + dy, 0, H - 1)][clamp(xi + dx, 0, W - 1)],
 *                         dx, dy in {-1, 0, 1}, equals i. (A 3 x 3 test on purpose: under jitter a silhouette moves by up
 *                         to half a pixel between frames, and a nearest-pixel test would reject exactly the pixels that
 *                         need accumulating. There is no depth test: a slope's depth changes under jitter.)
 *     lo, hi = per channel, as bytes, the min and max of c over (clamp(x + dx, 0, W - 1), clamp(y + dy, 0, H - 1))
 *     cur16 = (float)(c_ch * 257)     lo16 = (float)(lo * 257)     hi16 = (float)(hi * 257)
 *     valid = (mask & 15) == 0
 *     valid:    t = c00 * (1.0f - fu) + c10 * fu,  b = c01 * (1.0f - fu) + c11 * fu,  h = t * (1.0f - fv) + b * fv
 *               over the taps of A' (not rounded);  hc = fminf(fmaxf(h, lo16), hi16)
 *               TRI_TAA_CLAMPED iff hc != h in any channel
 *               r = hc * (1.0f - alpha) + cur16 * alpha;  s = min((int)(r + 0.5f), 65535)
 *               out8 = min((int)((float)s * (1.0f / 257.0f) + 0.5f), 255)
 *     invalid:  s = c_ch * 257,  out8 = c_ch       (the history restarts from the current frame)
 *     stored:   A[p] = s, I[p] = i, resolved[p] = out8 (B8G8R8A8), mask[p]
 * All four channels follow the same rule. The colour is read as the context holds it when the call is enqueued: after
 * the selection outline and the text overlay. One host thread per object.
 *
 * The jitter contract. Frame n is rendered with tri_taa_jitter_projection(P_n, j_n) in the uniform block, and
 * tri_set_motion_history is given the previous view with tri_taa_jitter_projection(P_{n-1}, j_n) as prev_projection:
 * the previous UNJITTERED projection under the CURRENT jitter. The staged table then maps a pixel to the place its
 * surface had in the unjittered history plus j_n — where the accumulated history, which is registered to the
 * unjittered frame, must be sampled. For a still camera and scene the two matrices are bitwise equal, the row is the
 * exact identity, the history tap is the pixel itself and nothing blurs. */
#define TRI_FORMAT_R16G16B16A16_UNORM 91u /* VK_FORMAT_R16G16B16A16_UNORM: tri_image.format of the accumulated colour */
#define TRI_TAA_NO_HISTORY 1u
#define TRI_TAA_NO_PROJ 2u
#define TRI_TAA_OUTSIDE 4u
#define TRI_TAA_ID 8u
#define TRI_TAA_CLAMPED 32u
#define TRI_TAA_REDO 1u      /* tri_taa_params.flags: the frame of the last call, rendered again */
#define TRI_TAA_REJECT_ID 2u /* ... the 3 x 3 id test */
typedef struct tri_taa tri_taa;
typedef struct tri_taa_params {
    float alpha;    /* the current frame's weight, 0 < alpha <= 1 (1: the resolved image is the current frame) */
    uint32_t flags; /* TRI_TAA_REDO | TRI_TAA_REJECT_ID */
    uint32_t reserved[2];
} tri_taa_params;
/* The sub-pixel offset of frame `index`, in pixels: with k = index % period + 1,
 * xy = (radical_inverse_2(k) - 0.5, radical_inverse_3(k) - 0.5), computed in double and rounded once (the Halton
 * sequence, centred). period == 0 gives (0, 0). Host only. TRI_E_INVALID for a null xy or a period above 64. */
int tri_taa_jitter(uint32_t index, uint32_t period, float xy[2]);
/* proj with every projected point moved by exactly (+jx, +jy) pixels of a width x height frame (x right, y down, the
 * pixel convention of "motion vectors"), perspective and orthographic alike: with dx = 2 jx / width, dy = 2 jy / height
 * in double, out[4c + 0] = proj[4c + 0] + dx * proj[4c + 3] and out[4c + 1] = proj[4c + 1] + dy * proj[4c + 3] for every
 * column c, rounded once; rows 2 and 3 are copied bitwise, so depth is untouched. out may be proj. Host only.
 * TRI_E_INVALID for a null pointer or a zero extent. */
int tri_taa_jitter_projection(const float proj[16], float jx, float jy, uint32_t width, uint32_t height, float out[16]);
/* Two sets of {accumulated colour 8 B, ids 4 B} per pixel, the resolved image (4 B), the mask (1 B) and the object's
 * events, on one device (-1 = current). TRI_E_INVALID for a zero extent or more than 2^31 pixels, before any device is
 * touched. tri_taa_destroy waits for the last pass; NULL is TRI_OK. */
int tri_taa_create(int32_t device, uint32_t width, uint32_t height, tri_taa** out);
int tri_taa_destroy(tri_taa* taa);
/* Asynchronous, on the context's stream behind the tri_render whose frame it reads (and behind the object's previous
 * pass, which may have run on another context's stream). The sets swap and TRI_TAA_REDO works as tri_history_reproject's
 * do. TRI_E_INVALID: a null argument, a context on another device or of another extent, an alpha outside (0, 1] or not
 * finite, unknown flag bits. TRI_E_UNSUPPORTED: a row-band context. TRI_E_STATE: the context's motion output is off, or
 * no frame has been rendered with it. Every check comes before the device is made current. Stamped like
 * tri_history_reproject while a timed frame is wanted of the context. */
int tri_taa_resolve(tri_taa* taa, tri_ctx* ctx, const tri_taa_params* params);
/* Forget the accumulated frame: the next call reports TRI_TAA_NO_HISTORY everywhere (and a redo is a plain call). */
int tri_taa_reset(tri_taa* taa);
/* The last pass's resolved image (width x height x 4 bytes, B G R A), accumulated colour (width x height x 4 uint16,
 * B G R A) and mask (width x height bytes), tightly packed; any pointer may be NULL. Waits for the pass. TRI_E_STATE
 * before the first pass. */
int tri_taa_read(tri_taa* taa, uint8_t* bgra8, uint16_t* rgba16, uint8_t* mask);
/* The three images in device memory: the resolved colour (TRI_FORMAT_B8G8R8A8_UNORM, pitch width * 4), the accumulated
 * colour the last pass wrote (TRI_FORMAT_R16G16B16A16_UNORM, pitch width * 8; it changes sets from pass to pass, so ask
 * after each), the mask (TRI_FORMAT_R8_UINT, pitch width). Any pointer may be NULL. TRI_E_STATE before the first pass. */
int tri_taa_get_output(tri_taa* taa, tri_image* colour8, tri_image* colour16, tri_image* mask);
/* As tri_history_get_timing. */
int tri_taa_get_timing(tri_taa* taa, double* ms, uint64_t* passes);
/* tri_blit_linear's rule over the resolved image instead of the context's colour: the presentation blit into dst
 * (width x height B8G8R8A8; NULL: the context's present image, read by tri_read_present), on the context's stream
 * behind the object's last pass. TRI_E_INVALID: a null object or context, a bad destination extent, another device or
 * extent; TRI_E_STATE: a row-band context, or no pass has run. */
int tri_taa_blit_linear(tri_taa* taa, tri_ctx* ctx, void* dst, uint32_t width, uint32_t height);

/* ---- temporal upscaling: jittered low-resolution frames resolved at the display extent ---------- */
/* The jitter that removes staircases also places each frame's samples at new sub-pixel positions of a finer grid. A
 * tri_upscale keeps the accumulated colour of one view at an OUTPUT extent Wo x Ho (16-bit UNORM, as a tri_taa) and the
 * ids of the last frame at the RENDER extent Wr x Hr (the context's), twice, outside any context. After a tri_render with
 * the motion output on, tri_upscale_resolve enqueues k_upscale_resolve on the context's stream: one output pixel per
 * lane takes the render pixel whose jittered sample lies nearest, weighs it by the sample's distance from the output
 * pixel's centre, and accumulates it over the clamped history fetched at the output extent. No kernel of the frame
 * changes; the context's colour, depth, ids and motion are bit-identical with and without the pass.
 * The host computes, each as one float32 division, rx = (float)Wr / (float)Wo, ry = (float)Hr / (float)Ho,
 * ox = (float)Wo / (float)Wr, oy = (float)Ho / (float)Hr; (jx, jy) is the frame's jitter in render pixels. The rule for
 * output pixel (X, Y), integers and float32, no multiply-add contracted, in exactly this order:
 *     px = ((float)X + 0.5f) * rx                      py likewise with Y, ry
 *     xr = clamp((int)floorf(px + jx), 0, Wr - 1)      yr likewise: the render pixel whose jittered sample lies nearest
 *     c, i, d = colour, id, depth of render pixel (xr, yr);  R = the staged motion table's row for i
 *     dx = (((float)xr + 0.5f) - jx) * ox - ((float)X + 0.5f)      dy likewise: the sample minus the output centre, output px
 *     k  = fmaxf(0.0f, 1.0f - fabsf(dx)) * fmaxf(0.0f, 1.0f - fabsf(dy))       a = alpha * k
 *     TRI_UPSCALE_NO_HISTORY  the object holds no previous frame; the mask is then exactly 1 on every pixel
 *     u, v, proj, inside, the nearest previous pixel `at` and the four taps with fu, fv: exactly as under "history
 *     reprojection", for pixel (X, Y) of a Wo x Ho frame with id i and depth d
 *     TRI_UPSCALE_NO_PROJ     !proj                    TRI_UPSCALE_OUTSIDE     proj && !inside
 *     TRI_UPSCALE_ID          with TRI_UPSCALE_REJECT_ID, inside, and with xi = at % Wo, yi = at / Wo,
 *                             xq = min((int)(((float)xi + 0.5f) * rx), Wr - 1), yq likewise, none of the previous ids
 *                             I'[clamp(yq + dy, 0, Hr - 1)][clamp(xq + dx, 0, Wr - 1)], dx, dy in {-1, 0, 1}, equals i
 *     lo, hi = per channel, as bytes, the min and max of the render frame's colour over the clamped 3 x 3 round (xr, yr)
 *     valid = (mask & 15) == 0
 *     valid:    "temporal anti-aliasing"'s blend of the four taps of A' (Wo x Ho), its clamp to lo, hi
 *               (TRI_UPSCALE_CLAMPED) and its mix r = hc * (1.0f - a) + cur16 * a, s and out8 as there;
 *               TRI_UPSCALE_NO_SAMPLE in addition iff k == 0.0f: the frame added nothing to this pixel
 *     invalid:  s = c_ch * 257,  out8 = c_ch       (the history restarts from the nearest sample, whatever k is)
 *     stored:   A[Y][X] = s, resolved[Y][X] = out8 (B8G8R8A8), mask[Y][X] at the output extent;
 *               I[y][x] = ids[y][x] for every render pixel
 * At Wo == Wr and Ho == Hr this is not tri_taa's rule: the weight is alpha (1 - |jx|)(1 - |jy|).
 *
 * The jitter contract is tri_taa's, with tri_taa_jitter_projection taking the RENDER extent: frame n is rendered with
 * jitter(P_n, j_n), tri_set_motion_history gets jitter(P_{n-1}, j_n). A still scene gives identity rows, and each output
 * pixel's tap is then the pixel itself. */
#define TRI_UPSCALE_NO_HISTORY 1u
#define TRI_UPSCALE_NO_PROJ 2u
#define TRI_UPSCALE_OUTSIDE 4u
#define TRI_UPSCALE_ID 8u
#define TRI_UPSCALE_CLAMPED 32u
#define TRI_UPSCALE_NO_SAMPLE 64u
#define TRI_UPSCALE_REDO 1u      /* tri_upscale_params.flags: the frame of the last call, rendered again */
#define TRI_UPSCALE_REJECT_ID 2u /* ... the 3 x 3 id test */
typedef struct tri_upscale tri_upscale;
typedef struct tri_upscale_params {
    float alpha;     /* the current frame's weight at a sample on the pixel's centre, 0 < alpha <= 1 */
    float jitter[2]; /* the jitter the frame was rendered under, in render pixels, |j| <= 0.5 */
    uint32_t flags;  /* TRI_UPSCALE_REDO | TRI_UPSCALE_REJECT_ID */
} tri_upscale_params;
/* Two sets of {accumulated colour 8 B per output pixel, ids 4 B per render pixel}, the resolved image (4 B) and the mask
 * (1 B) at the output extent and the object's events, on one device (-1 = current). TRI_E_INVALID, before any device is
 * touched: a zero extent, more than 2^31 pixels, a side above 2^30, or an output extent outside render_w <= out_w <= 3 render_w,
 * render_h <= out_h <= 3 render_h. tri_upscale_destroy waits for the last pass; NULL is TRI_OK. */
int tri_upscale_create(int32_t device, uint32_t render_w, uint32_t render_h, uint32_t out_w, uint32_t out_h, tri_upscale** out);
int tri_upscale_destroy(tri_upscale* up);
/* Asynchronous, on the context's stream behind the tri_render whose frame it reads (and behind the object's previous
 * pass, which may have run on another context's stream); the frame's ids are copied into the written set on the same
 * stream. The sets swap and TRI_UPSCALE_REDO works as tri_history_reproject's do. TRI_E_INVALID: a null argument, a
 * context on another device or whose extent is not the render extent, an alpha outside (0, 1], a jitter that is not
 * finite or beyond half a pixel, unknown flag bits. TRI_E_UNSUPPORTED: a row-band context. TRI_E_STATE: the context's
 * motion output is off, or no frame has been rendered with it. Every check comes before the device is made current. */
int tri_upscale_resolve(tri_upscale* up, tri_ctx* ctx, const tri_upscale_params* params);
/* Forget the accumulated frame: the next call reports TRI_UPSCALE_NO_HISTORY everywhere (and a redo is a plain call). */
int tri_upscale_reset(tri_upscale* up);
/* The last pass's resolved image (out_w x out_h x 4 bytes, B G R A), accumulated colour (x 4 uint16) and mask (bytes),
 * tightly packed; any pointer may be NULL. Waits for the pass. TRI_E_STATE before the first pass. */
int tri_upscale_read(tri_upscale* up, uint8_t* bgra8, uint16_t* rgba16, uint8_t* mask);
/* The last pass's stored ids (render_w x render_h uint32). Waits for the pass. TRI_E_STATE before the first pass. */
int tri_upscale_read_ids(tri_upscale* up, uint32_t* ids);
/* The three images in device memory, all at the output extent, in tri_taa_get_output's formats; colour16 is the set the
 * last pass wrote. Any pointer may be NULL. TRI_E_STATE before the first pass. */
int tri_upscale_get_output(tri_upscale* up, tri_image* colour8, tri_image* colour16, tri_image* mask);
/* As tri_history_get_timing; the interval covers the kernel and the id copy. */
int tri_upscale_get_timing(tri_upscale* up, double* ms, uint64_t* passes);
/* As tri_taa_blit_linear, over the object's resolved image. */
int tri_upscale_blit_linear(tri_upscale* up, tri_ctx* ctx, void* dst, uint32_t width, uint32_t height);
/* min(64, ceil(8 (out_w / render_w) (out_h / render_h))) in double: eight samples per output pixel's area (8 at 1 x, 18 at
 * 1.5 x, 32 at 2 x, 64 at 3 x). Host only. TRI_E_INVALID for a null period or extents tri_upscale_create refuses. */
int tri_upscale_jitter_period(uint32_t render_w, uint32_t render_h, uint32_t out_w, uint32_t out_h, uint32_t* period);

/* ---- one rank's band exchange (process per GPU) --------------------------------------------- */
/* A process-per-GPU caller (bench.py at N > 1) renders one row band per rank and assembles the frame on the
 * display rank. tri_xfer drives that exchange natively over RCCL communicators of its own: one call per frame
 * renders the band on the context's stream, then on the same stream packs and sends it (a sender) or receives and
 * decodes every remote band into the frame (the display rank) — no per-operation host bookkeeping in the
 * caller (torch.distributed's point-to-point calls cost ≈ 20 µs of host time each). Bootstrap, once per
 * communicator: rank 0 calls tri_xfer_unique_id and the caller broadcasts the TRI_XFER_ID_BYTES bytes (e.g. over
 * torch.distributed); every rank then calls tri_xfer_comm_create (collective). Communicators serve any number of
 * exchanges used one at a time. */
#define TRI_XFER_ID_BYTES 128u
typedef struct tri_xfer_comm tri_xfer_comm;
typedef struct tri_xfer tri_xfer;
typedef struct tri_xfer_config {
    uint32_t width;           /* pixels per row                                                          */
    const uint32_t* band_y;   /* world + 1 row boundaries: rank r renders rows [band_y[r], band_y[r + 1]);
                                 every band has rows except the display's, which may be empty: the
                                 display then renders nothing and only assembles (ctx NULL every frame) */
    uint32_t display;         /* the rank that assembles the frame                                       */
    uint32_t format;          /* TRI_GROUP_FMT_*: the bands' transfer format                             */
    uint32_t slot_bytes;      /* TRI_GROUP_FMT_DBP: the slot size every rank agreed                      */
    uint32_t alpha;           /* packed formats: the proven alpha (tri_frame_alpha)                      */
    uint32_t nbuf;            /* buffer slots (tri_xfer_bind_slot)                                       */
} tri_xfer_config;
int tri_xfer_unique_id(uint8_t* id_out);
int tri_xfer_comm_create(const uint8_t* id, uint32_t world, uint32_t rank, int32_t device, tri_xfer_comm** out);
int tri_xfer_comm_destroy(tri_xfer_comm* comm);
/* comms: one communicator per slot in flight (slot s uses comms[s % comm_count]; each created with the same world,
 * rank and device), so that each one's operations stay on one stream (the slot's context stream). With fewer
 * communicators than slots (e.g. a second ncclCommInitRank failed), a communicator shared by several slots has its
 * operations fenced across their streams by an event (correct, ≈ 2 µs of host time per frame more). */
int tri_xfer_create(tri_xfer_comm* const* comms, uint32_t comm_count, const tri_xfer_config* config, tri_xfer** out);
int tri_xfer_destroy(tri_xfer* xfer);
/* Slot `slot`'s pixel buffer (device, 4-B aligned, caller-owned): this rank's band (a sender) or the whole
 * width × height frame (the display rank, which renders its own band in place at its row offset). */
int tri_xfer_bind_slot(tri_xfer* xfer, uint32_t slot, void* bgra8);
/* One frame into slot `slot`: if ctx is not NULL, bind it to the slot (and `depth`, may be NULL), apply the frame
 * state when given (ubo / draws not NULL: tri_set_frame / tri_set_draws) and tri_render; then, if `exchange`, the
 * band's transfer, on the same stream (the context's; ctx NULL: the slot's last stream, or a stream of the slot's
 * own if it never rendered, so an assemble-only display's slots overlap as render streams do). A slot reused on its
 * stream is ordered behind its previous transfer by stream order; a slot that changes stream is fenced. Every rank
 * must make the same sequence of exchanging calls per slot (the transfers match in order per communicator). */
int tri_xfer_frame(tri_xfer* xfer, uint32_t slot, tri_ctx* ctx, void* depth, const tri_global_ubo* ubo,
                   const float clear_rgba[4], const tri_draw* draws, uint32_t draw_count, uint32_t exchange);
/* Wait for every slot's stream, at most the exchange's timeout (tri_xfer_set_timeout, default 60000 ms; 0 = none):
 * TRI_E_TIMEOUT when it expires, TRI_E_HIP when a communicator reports an asynchronous error — both abort the
 * exchange's communicators (ncclCommAbort; later exchanging frames on them fail with TRI_E_STATE), so the caller can
 * exit instead of hanging the job. Then TRI_E_STATE if a packed band's alpha differed, TRI_E_OVERFLOW if a band
 * outgrew the agreed dbp slot (both lossy). On the display rank these report the senders' bands too: the status
 * travels with each packed band and the decode ORs it in. */
int tri_xfer_synchronize(tri_xfer* xfer);
/* The bounded wait alone (TRI_E_TIMEOUT / TRI_E_HIP as above), without reading the status flags. */
int tri_xfer_wait(tri_xfer* xfer);
int tri_xfer_set_timeout(tri_xfer* xfer, uint32_t timeout_ms);
/* The number of communicators the exchange runs on (comm_count at tri_xfer_create). */
int tri_xfer_comm_count(tri_xfer* xfer, uint32_t* count);
/* Bytes this rank sends and receives per frame; max_slot_bytes (may be NULL; synchronising): the largest dbp slot
 * this rank's packs needed. */
int tri_xfer_info(tri_xfer* xfer, uint64_t* sent_bytes, uint64_t* received_bytes, uint32_t* max_slot_bytes);
/* Loopback transport (tests only; replaces nothing in the reference): `world` tri_xfer exchanges of one process on
 * one device stand in for `world` ranks (RCCL refuses two ranks on one GPU). tri_xfer_comm_create_loopback is
 * tri_xfer_comm_create's counterpart: the k-th communicator each rank creates on a hub forms channel k. Sends become
 * a device copy into the display's receive buffer, ordered by events as ncclSend / ncclRecv order them; every other
 * step of the exchange runs as on N GPUs. Drive the ranks frame by frame, every sender before the display. */
typedef struct tri_xfer_loopback tri_xfer_loopback;
int tri_xfer_loopback_create(uint32_t world, tri_xfer_loopback** out);
int tri_xfer_loopback_destroy(tri_xfer_loopback* hub);
int tri_xfer_comm_create_loopback(tri_xfer_loopback* hub, uint32_t rank, int32_t device, tri_xfer_comm** out);

/* ---- measurement -------------------------------------------------------------------------- */
/* enable = N > 0: HIP events around every stage of every N-th frame (1 = all frames; sampling keeps
 * the event overhead out of throughput runs); 0 = off. Also resets the accumulators. */
int tri_set_timing(tri_ctx* ctx, int enable);
int tri_get_timing(tri_ctx* ctx, tri_timing* out); /* synchronizes                      */
int tri_get_frame_stats(tri_ctx* ctx, tri_frame_stats* out); /* synchronizes           */

/* ---- multi-device frames (SURVEY 8(b) tri_config.device_count; 8(e) screen partition) ---------
 * A tri_group renders one frame on N contexts, context r owning rows [r*H/N, (r+1)*H/N) (sort-first:
 * geometry and uniforms replicated, every context culls clusters to its rows), and assembles the B8G8R8A8
 * frame on the display context's device: bands on that device render straight into the frame, bands
 * on other devices are gathered with RCCL grouped ncclSend / ncclRecv over xGMI (one communicator per
 * distinct device, ncclCommInitAll). One host thread drives the whole group, as Renderer::DrawFrame
 * does (the engine's single render thread, Application.cpp:82-134).
 * The geometry is held once per distinct device (one tri_geometry bound by every band context there).
 * The assembled frame is double-buffered: frame k lands in buffer k % 2, and frame k + 2 overwrites it
 * only after the consumer's fence on frame k (tri_group_present), when one was set — the reference keeps
 * one framebuffer per swapchain image and waits on that image's fence (Renderer.cpp:744-772). */
typedef struct tri_group tri_group;
typedef struct tri_group_config {
    uint32_t width;
    uint32_t height;
    uint32_t device_count;  /* N >= 1 bands                                                       */
    uint32_t display;       /* index of the band whose device holds the assembled frame            */
    const int32_t* devices; /* N HIP ordinals, NULL = 0..N-1; an ordinal may repeat (bands sharing  *
                             * a device are assembled without copies)                               */
    uint32_t flags;         /* TRI_FLAG_* for every band context                                    */
    uint32_t group_flags;   /* TRI_GROUP_* (0 = defaults)                                           */
} tri_group_config;
/* Bands travel to the display device as 4-byte pixels even when tri_frame_alpha proves a uniform alpha
 * (default: the delta bit-plane format then, TRI_GROUP_FMT_DBP below — lossless, restored on arrival). */
#define TRI_GROUP_NO_PACK 0x1u
/* Bands on the display device render into band buffers and travel like remote bands (a device-local copy
 * instead of RCCL): the remote path's buffers, fences and codec on a single GPU (tests, diagnostics). */
#define TRI_GROUP_STAGE_BANDS 0x2u
/* With a proven uniform alpha, bands travel as their B, G, R bytes (3 per pixel) instead of the delta bit-plane
 * format. */
#define TRI_GROUP_PACK_BGR24 0x4u
/* Band transfer formats (tri_group_transfer_format). */
#define TRI_GROUP_FMT_BGRA32 0u /* 4 bytes per pixel                                                  */
#define TRI_GROUP_FMT_BGR24 1u  /* 3 bytes per pixel, the proven alpha restored on arrival           */
/* the delta bit-plane format (tri_dbp_pack): fixed slots of slot_bytes per 4096 pixels, sized at every
 * tri_group_synchronize from the largest slot the frames since the previous one needed (+ 1/16); the first frame
 * uses TRI_DBP_MAX_SLOT, which always fits. A frame with a slot that outgrew its size is reported by
 * tri_group_synchronize as TRI_E_OVERFLOW (its slot is then refitted: render the frame again). */
#define TRI_GROUP_FMT_DBP 2u

int tri_group_create(const tri_group_config* config, tri_group** out_group);
int tri_group_destroy(tri_group* group);
/* The band context of index `band` (uploads, cameras, shadows, timing, readback of its own band). */
int tri_group_context(tri_group* group, uint32_t band, tri_ctx** out_ctx);
/* Broadcasts of the per-context uploads / frame inputs to every band (same semantics as the tri_* calls). */
int tri_group_upload_geometry(tri_group* group, const tri_vertex* vertices, uint64_t vertex_count,
                              const uint32_t* indices, uint64_t index_count, const tri_mesh_range* meshes,
                              uint32_t mesh_count);
int tri_group_upload_materials(tri_group* group, const tri_material_record* records, uint32_t count);
int tri_group_upload_texture(tri_group* group, uint32_t slot, const uint8_t* rgba8_srgb, uint32_t width,
                             uint32_t height);
int tri_group_upload_bone_palette(tri_group* group, const float* matrices, uint32_t matrix_count);
int tri_group_upload_skybox(tri_group* group, const uint8_t* faces_rgba8_srgb, uint32_t size);
int tri_group_upload_skybox_ex(tri_group* group, const tri_skybox_desc* desc);
int tri_group_upload_ai_frame(tri_group* group, const uint8_t* rgba8_unorm, uint32_t width, uint32_t height);
int tri_group_set_shadow(tri_group* group, const tri_shadow_config* config);
int tri_group_set_frame(tri_group* group, const tri_global_ubo* ubo, const float clear_rgba[4]);
int tri_group_set_draws(tri_group* group, const tri_draw* draws, uint32_t draw_count);
/* tri_set_text on every band with the same full-frame quads (each band composites its own rows). fonts: one atlas per
 * distinct device of the group, in any order (as tri_group_bind_geometry's objects: a band takes the one on its
 * device; TRI_E_INVALID — no band changed — if a band's device has none). fonts == NULL or count == 0 removes the
 * overlay. */
int tri_group_set_text(tri_group* group, tri_font* const* fonts, const tri_text_quad* quads, uint32_t count);
/* tri_pose_palette on every band with the same instances. sets: one tri_animset per distinct device of the group, in
 * any order, each holding the same skeletons and clips under the same indices (TRI_E_INVALID — nothing enqueued — if
 * a band's device has none, or any band refuses the instances; a HIP failure on a later band leaves the earlier ones
 * posed). count == 0 drops every band's posed suffix. */
int tri_group_pose_palette(tri_group* group, tri_animset* const* sets, const tri_pose_instance* instances,
                           uint32_t count);
/* tri_pose_graph on every band with the same instances and operations, under tri_group_pose_palette's terms: the
 * sets also hold the same masks under the same indices, and every band's check passes before any band enqueues. */
int tri_group_pose_graph(tri_group* group, tri_animset* const* sets, const tri_pose_graph_instance* instances,
                         uint32_t count, const tri_pose_op* ops, uint32_t op_count);
/* Enqueue every band, then the assembly onto the display device (asynchronous). */
int tri_group_render(tri_group* group);
/* Wait for every band and the assembly; TRI_E_OVERFLOW as tri_synchronize (re-render the frame). */
int tri_group_synchronize(tri_group* group);
/* The assembled frame (width*height BGRA8, from the display device) and, optionally, the depth of
 * every band (width*height float32 bits). Synchronous. */
int tri_group_readback(tri_group* group, uint8_t* bgra8, uint32_t* depth_bits);
/* The assembled frame in device memory: its pointer on the display device and that device's ordinal
 * (the buffer of the most recent tri_group_render; complete once its assembly has run). */
int tri_group_frame(tri_group* group, void** device_bgra8, int32_t* device);
/* The same buffer as a tri_image (GetViewportTexture's handle for a multi-device viewport). */
int tri_group_get_output(tri_group* group, tri_image* out);
/* Consumer fence ("frame k presented"): the caller is done reading the most recent frame once the work
 * already enqueued on hip_stream (a stream on the display device) has run; NULL = once the frame's own
 * assembly (and any tri_group_blit_linear of it) has run on the group's assembly stream, i.e. the caller
 * reads nothing further on other streams. Frame k + 2, which reuses that buffer, waits for this point on
 * the device before any band or receive writes it. Without a fence the next-but-one frame overwrites the
 * buffer unconditionally (a caller that reads with tri_group_readback, which synchronises, needs none);
 * a tri_group_blit_linear of frame k is always waited for (it reads the buffer on the assembly stream). */
int tri_group_present(tri_group* group, void* hip_stream);
/* Binds caller-owned geometry objects: for every band, the one of `geometries` on the band's device
 * (TRI_E_INVALID if a band's device has none). count 0 returns the bands to the group's own per-device
 * copies, which tri_group_upload_geometry fills. The objects must outlive the binding. */
int tri_group_bind_geometry(tri_group* group, uint32_t count, tri_geometry* const* geometries);
/* tri_blit_linear / tri_read_present over the assembled frame (the presentation blit of a multi-device
 * viewport, on the display device, stream-ordered after the frame's assembly; frame k + 2's bands and
 * receives wait for the blit of frame k). A blit into a caller-supplied dst does not touch the group's
 * own present target: tri_group_read_present then fails with TRI_E_STATE until a blit with dst = NULL. */
int tri_group_blit_linear(tri_group* group, void* dst, uint32_t width, uint32_t height);
int tri_group_read_present(tri_group* group, uint8_t* bgra8);
/* The most recent frame's band transfer: bytes per pixel on the links (4, 3, or for the delta bit-plane format
 * its stream bytes per pixel rounded up) and the bytes the display device received over RCCL (exact). */
int tri_group_transfer_info(tri_group* group, uint32_t* bytes_per_pixel, uint64_t* inbound_bytes);
/* The most recent frame's transfer format (TRI_GROUP_FMT_*) and, for TRI_GROUP_FMT_DBP, its slot size in bytes
 * per 4096 pixels (0 otherwise); before any frame, the format and slot the next frame would use with packing. */
int tri_group_transfer_format(tri_group* group, uint32_t* format, uint32_t* slot_bytes);
/* Entity ids over a group: the id output of every band context; the whole frame's ids (width * height), copied band
 * by band from each band's device (no RCCL: the ids never travel to the display device); one pixel from the band that
 * holds it. Outlines are single-context only (tri_set_outline). */
int tri_group_set_id_output(tri_group* group, int enable);
int tri_group_read_ids(tri_group* group, uint32_t* ids);
int tri_group_pick(tri_group* group, int32_t x, int32_t y, tri_pick_result* out);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(tri_vertex) == 100, "Vertex stride must match Trident's 100-byte Vertex");
static_assert(sizeof(tri_push_constant) == 128, "RenderablePushConstant is 128 bytes");
static_assert(sizeof(tri_draw) == 144, "tri_draw layout");
static_assert(sizeof(tri_global_ubo) == 480, "GlobalUniformBuffer is 480 bytes");
static_assert(sizeof(tri_material_record) == 32, "MaterialUniformBuffer is 32 bytes");
static_assert(sizeof(tri_shadow_config) == 80, "tri_shadow_config layout");
static_assert(sizeof(tri_group_config) == 32, "tri_group_config layout");
static_assert(sizeof(tri_image) == 32, "tri_image layout");
static_assert(sizeof(tri_text_quad) == 48, "tri_text_quad layout");
static_assert(sizeof(tri_pick_result) == 16, "tri_pick_result layout");
static_assert(sizeof(tri_outline) == 40, "tri_outline layout");
static_assert(sizeof(tri_motion_history) == 144, "tri_motion_history layout");
static_assert(sizeof(tri_record_params) == 16, "tri_record_params layout");
static_assert(sizeof(tri_reproject_params) == 16, "tri_reproject_params layout");
static_assert(sizeof(tri_taa_params) == 16, "tri_taa_params layout");
static_assert(sizeof(tri_upscale_params) == 16, "tri_upscale_params layout");
static_assert(sizeof(tri_pose_bone) == 128, "tri_pose_bone layout");
static_assert(sizeof(tri_pose_channel) == 32, "tri_pose_channel layout");
static_assert(sizeof(tri_pose_instance) == 16, "tri_pose_instance layout");
static_assert(sizeof(tri_pose_op) == 16, "tri_pose_op layout");
static_assert(sizeof(tri_pose_graph_instance) == 16, "tri_pose_graph_instance layout");
#endif

#endif /* TRI_RASTER_H */
