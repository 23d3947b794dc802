// tri_resources.hip — the resource entry points of the C-ABI (include/tri_raster.h): what a context's frames read
// besides geometry. Materials and texture slots (Renderer.cpp:3404-3656), the skybox, the AI frame, the shadow
// pre-pass's configuration, fonts and the text overlay's quads, the bone palette and the device pose calls.
#include "tri_ctx.h"

using fsel::srgb_decode;
using fsel::unorm8_host;

int tri_internal_font_device(const tri_font* f) { return f->device; }
uint32_t tri_internal_pose_prefix(tri_ctx* c) { return c->nbones_prefix; }

namespace {

// Room for `extent` matrices in the palette, keeping the prefix: frames in flight read the old palette, so growing
// synchronises. (The one buffer DevBuf::grow does not serve: grow() drops the contents.)
int pose_reserve_palette(tri_ctx* c, uint32_t extent, const char* who) {
    DevBuf<float>& pal = c->d_bones;
    if (16ull * extent <= pal.cap && pal.p) return TRI_OK;
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    float* grown = nullptr;
    const size_t cap = std::max<size_t>(16ull * extent, 2 * pal.cap);
    TRI_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&grown), cap * sizeof(float)));
    hipError_t e = hipMemset(grown, 0, cap * sizeof(float));
    if (e == hipSuccess && c->nbones_prefix)
        e = hipMemcpy(grown, pal.p, 64ull * c->nbones_prefix, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();  // null-stream work: complete before the context's stream reads it
    if (e != hipSuccess) {
        (void)hipFree(grown);
        return fail(TRI_E_HIP, "%s: growing the palette: %s", who, hipGetErrorString(e));
    }
    if (pal.p) TRI_HIP_TRY(hipFree(pal.p));
    pal.p = grown;
    pal.cap = cap;
    return TRI_OK;
}

// The skeleton-size groups of the pose kernels, one launch each: a workgroup's LDS is sized by its launch's largest
// skeleton, and a 256-bone instance should not make every 20-bone one reserve 40 KiB.
const uint32_t kPoseBucket[3] = {32, 128, TRI_POSE_MAX_BONES};
inline int pose_bucket(uint32_t bones) { return bones <= kPoseBucket[0] ? 0 : bones <= kPoseBucket[1] ? 1 : 2; }

// The body of both pose calls behind their checks (scratch.bones[i]: instance i's bone count): the next stage of the
// ring (four calls back: long complete unless the device is that far behind) takes the n instance records grouped by
// skeleton size, then `tail` further 16-B records as given; one copy, one launch per group over the device twin —
// launch(first record of the group, the tail, its count, its LDS bones) — and the fence behind them.
template <typename Inst, typename Launch>
int pose_enqueue(tri_ctx* c, const Inst* inst, uint32_t n, const void* tail, uint32_t ntail, size_t min_records,
                 uint32_t extent, Launch launch) {
    static_assert(sizeof(Inst) == 16 && sizeof(tri_pose_op) == 16, "16-B records");
    Staged& st = c->pose_ring[c->pose_next];
    const size_t records = (size_t)n + ntail;
    if (const int rc = st.acquire(records * 16, std::max(records, min_records) * 16, true)) return rc;
    const std::vector<uint32_t>& bones = c->pose_scratch.bones;
    uint32_t first[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) ++first[pose_bucket(bones[i]) + 1];
    first[2] += first[1];
    first[3] += first[2];
    uint32_t at[3] = {0, first[1], first[2]};
    Inst* h = reinterpret_cast<Inst*>(st.h.p);
    for (uint32_t i = 0; i < n; ++i) h[at[pose_bucket(bones[i])]++] = inst[i];
    if (ntail) std::memcpy(h + n, tail, (size_t)ntail * 16);
    TRI_HIP_TRY(hipMemcpyAsync(st.d.p, st.h.p, records * 16, hipMemcpyHostToDevice, c->stream));
    const Inst* d = reinterpret_cast<const Inst*>(st.d.p);
    for (int b = 0; b < 3; ++b) TRI_HIP_TRY(launch(d + first[b], d + n, first[b + 1] - first[b], kPoseBucket[b]));
    if (const int rc = st.commit(c->stream)) return rc;
    c->pose_next = (c->pose_next + 1) % 4;
    c->nbones = extent;
    return TRI_OK;
}

}  // namespace

extern "C" {

int tri_upload_materials(tri_ctx* c, const tri_material_record* r, uint32_t n) {
    if (!c) return fail(TRI_E_INVALID, "tri_upload_materials: null context");
    if (n && !r) return fail(TRI_E_INVALID, "tri_upload_materials: null records");
    c->mat0 = n ? r[0] : tri_material_record{{1, 1, 1, 1}, {1, 1, 1, 0}};
    return TRI_OK;
}

int tri_upload_texture(tri_ctx* c, uint32_t slot, const uint8_t* rgba, uint32_t w, uint32_t h) {
    if (!c) return fail(TRI_E_INVALID, "tri_upload_texture: null context");
    if (slot >= TRI_MAX_TEXTURE_SLOTS) return fail(TRI_E_INVALID, "tri_upload_texture: slot %u >= %d", slot, TRI_MAX_TEXTURE_SLOTS);
    if (!rgba || w == 0 || h == 0 || (uint64_t)w * h > (1ull << 28))
        return fail(TRI_E_INVALID, "tri_upload_texture: bad texture %ux%u", w, h);
    int rc = make_current(c);
    if (rc) return rc;
    if ((rc = upload_blocking(c, c->d_tex[slot], (size_t)w * h, rgba, (size_t)w * h * 4))) return rc;
    c->tex_w[slot] = w;
    c->tex_h[slot] = h;
    std::memcpy(&c->tex_solid[slot], rgba, 4);
    c->tex_alpha[slot] = rgba[3];
    for (size_t i = 1, n = (size_t)w * h; i < n; ++i)
        if (rgba[4 * i + 3] != rgba[3]) {
            c->tex_alpha[slot] = -1;
            break;
        }
    c->tex_dirty = true;
    return TRI_OK;
}

int tri_upload_bone_palette(tri_ctx* c, const float* m, uint32_t n) {
    if (!c) return fail(TRI_E_INVALID, "tri_upload_bone_palette: null context");
    if (n && !m) return fail(TRI_E_INVALID, "tri_upload_bone_palette: null matrices");
    int rc = make_current(c);
    if (rc) return rc;
    if ((rc = upload_blocking(c, c->d_bones, std::max<size_t>(16ull * n, 16), m, 64ull * n))) return rc;
    c->nbones = n;
    c->nbones_prefix = n;  // the posed suffix, if any, is dropped
    return TRI_OK;
}

int tri_pose_palette(tri_ctx* c, tri_animset* set, const tri_pose_instance* inst, uint32_t n) {
    if (!c) return fail(TRI_E_INVALID, "tri_pose_palette: null context");
    if (!n) {
        c->nbones = c->nbones_prefix;
        return TRI_OK;
    }
    if (!set || !inst) return fail(TRI_E_INVALID, "tri_pose_palette: null argument");
    if (tri_internal_animset_device(set) != c->device) return fail(TRI_E_INVALID, "tri_pose_palette: the set is on another device");
    uint32_t extent = 0;
    int rc = tri_pose_check(set, inst, n, c->nbones_prefix, &extent, c->pose_scratch);
    if (rc) return rc;
    if ((rc = make_current(c))) return rc;
    if ((rc = pose_reserve_palette(c, extent, "tri_pose_palette"))) return rc;
    return pose_enqueue(c, inst, n, nullptr, 0, 256, extent,
                        [&](const tri_pose_instance* d, const tri_pose_instance*, uint32_t count, uint32_t lds_bones) {
                            return tri_launch_pose(set, d, count, lds_bones, c->d_bones, c->stream);
                        });
}

int tri_pose_graph(tri_ctx* c, tri_animset* set, const tri_pose_graph_instance* inst, uint32_t n, const tri_pose_op* ops,
                   uint32_t nops) {
    if (!c) return fail(TRI_E_INVALID, "tri_pose_graph: null context");
    if (!n) {
        c->nbones = c->nbones_prefix;
        return TRI_OK;
    }
    if (!set || !inst || !ops) return fail(TRI_E_INVALID, "tri_pose_graph: null argument");
    if (tri_internal_animset_device(set) != c->device) return fail(TRI_E_INVALID, "tri_pose_graph: the set is on another device");
    uint32_t extent = 0;
    int rc = tri_pose_graph_check(set, inst, n, ops, nops, c->nbones_prefix, &extent, c->pose_scratch);
    if (rc) return rc;
    if ((rc = make_current(c))) return rc;
    if ((rc = pose_reserve_palette(c, extent, "tri_pose_graph"))) return rc;
    // the operations follow the instances as given (op_first stays an index into them)
    return pose_enqueue(c, inst, n, ops, nops, 512, extent,
                        [&](const tri_pose_graph_instance* d, const tri_pose_graph_instance* tail, uint32_t count,
                            uint32_t lds_bones) {
                            return tri_launch_pose_graph(set, d, reinterpret_cast<const tri_pose_op*>(tail), count, lds_bones,
                                                         c->d_bones, c->stream);
                        });
}

int tri_read_bone_palette(tri_ctx* c, float* out, uint32_t n) {
    if (!c) return fail(TRI_E_INVALID, "tri_read_bone_palette: null context");
    if (n > c->nbones) return fail(TRI_E_INVALID, "tri_read_bone_palette: %u matrices of a palette of %u", n, c->nbones);
    if (!n) return TRI_OK;
    if (!out) return fail(TRI_E_INVALID, "tri_read_bone_palette: null destination");
    int rc = make_current(c);
    if (rc) return rc;
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    TRI_HIP_TRY(hipMemcpy(out, c->d_bones, 64ull * n, hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_upload_skybox(tri_ctx* c, const uint8_t* faces, uint32_t n) {
    if (!c) return fail(TRI_E_INVALID, "tri_upload_skybox: null context");
    if (!faces || n == 0) {
        c->sky_size = 0;
        return TRI_OK;
    }
    if (n > 16384) return fail(TRI_E_INVALID, "tri_upload_skybox: face size %u too large", n);
    int rc = make_current(c);
    if (rc) return rc;
    const size_t texels = 6ull * n * n;
    if ((rc = upload_blocking(c, c->d_sky, texels, faces, texels * 4))) return rc;
    c->sky_size = n;
    c->sky_prefill = false;
    c->sky_format = TRI_SKY_FMT_RGBA8_SRGB;
    c->sky_mips = 1;
    const uint32_t* t = reinterpret_cast<const uint32_t*>(faces);
    uint32_t t0;
    std::memcpy(&t0, faces, 4);
    c->sky_uniform = true;
    for (size_t i = 1; i < texels && c->sky_uniform; ++i) {
        uint32_t ti;
        std::memcpy(&ti, t + i, 4);
        c->sky_uniform = ti == t0;
    }
    // Skybox.frag writes the decoded linear colour, alpha 1, to the UNORM target
    c->sky_uniform_bgra = unorm8_host(srgb_decode((t0 >> 16) & 0xFF)) | (unorm8_host(srgb_decode((t0 >> 8) & 0xFF)) << 8) |
                          (unorm8_host(srgb_decode(t0 & 0xFF)) << 16) | (255u << 24);
    return TRI_OK;
}

int tri_upload_skybox_ex(tri_ctx* c, const tri_skybox_desc* d) {
    if (!c || !d) return fail(TRI_E_INVALID, "tri_upload_skybox_ex: null argument");
    if (!d->texels || d->size == 0) {
        if (d->texels) return fail(TRI_E_INVALID, "tri_upload_skybox_ex: face size 0");
        c->sky_size = 0;
        return TRI_OK;
    }
    const uint32_t n = d->size;
    if (n > 16384) return fail(TRI_E_INVALID, "tri_upload_skybox_ex: face size %u too large", n);
    if (d->format > TRI_SKY_FMT_RGBA16F) return fail(TRI_E_INVALID, "tri_upload_skybox_ex: unknown format %u", d->format);
    if (d->flags & ~TRI_SKYBOX_PREFILL) return fail(TRI_E_INVALID, "tri_upload_skybox_ex: unknown flags 0x%x", d->flags);
    uint32_t max_mips = 1;
    while ((n >> max_mips) != 0u) ++max_mips;  // floor(log2(n)) + 1
    if (d->mip_count == 0 || d->mip_count > max_mips)
        return fail(TRI_E_INVALID, "tri_upload_skybox_ex: %u levels for a face size of %u (1..%u)", d->mip_count, n, max_mips);
    const uint64_t texels = fsel::sky_chain_texels(n, d->mip_count, nullptr);
    const uint64_t bpt = d->format == TRI_SKY_FMT_RGBA16F ? 8u : 4u;
    if (d->bytes != texels * bpt)
        return fail(TRI_E_INVALID, "tri_upload_skybox_ex: %llu bytes, the chain holds %llu", (unsigned long long)d->bytes,
                    (unsigned long long)(texels * bpt));
    if (d->format == TRI_SKY_FMT_RGBA8_SRGB && d->mip_count == 1 && !(d->flags & TRI_SKYBOX_PREFILL))
        return tri_upload_skybox(c, static_cast<const uint8_t*>(d->texels), n);
    int rc = make_current(c);
    if (rc) return rc;
    if ((rc = upload_blocking(c, c->d_sky, (size_t)(d->bytes / 4), d->texels, (size_t)d->bytes))) return rc;
    c->sky_size = n;
    c->sky_prefill = true;
    c->sky_format = d->format;
    c->sky_mips = d->mip_count;
    c->sky_uniform = false;
    return TRI_OK;
}

// The AI frame-generation texture (EnsureAiTextureResources, Renderer.cpp:1390-1500; UploadAiInterpolationToGpu,
// :1560-1700): R8G8B8A8_UNORM, the extent of the frame it was generated for.
int tri_upload_ai_frame(tri_ctx* c, const uint8_t* rgba8, uint32_t w, uint32_t h) {
    if (!c) return fail(TRI_E_INVALID, "tri_upload_ai_frame: null context");
    if (!rgba8 || w == 0 || h == 0) {  // DestroyAiResources: no texture, no blend
        c->ai_w = c->ai_h = 0;
        return TRI_OK;
    }
    if (w > TRI_MAX_DIM || h > TRI_MAX_DIM)
        return fail(TRI_E_INVALID, "tri_upload_ai_frame: extent %ux%u outside 1..%d", w, h, TRI_MAX_DIM);
    int rc = make_current(c);
    if (rc) return rc;
    if ((rc = upload_blocking(c, c->d_ai, (size_t)w * h, rgba8, (size_t)w * h * 4))) return rc;
    c->ai_w = w;
    c->ai_h = h;
    return TRI_OK;
}

// The same texture from a tensor on the device (a generator's output): k_ai_pack on the context's stream, so the
// frames already queued still sample the previous texels and the next tri_render samples these.
int tri_upload_ai_frame_device(tri_ctx* c, const void* nhwc, uint32_t w, uint32_t h, uint32_t channels, tri_framegen* behind) {
    if (!c || !nhwc) return fail(TRI_E_INVALID, "tri_upload_ai_frame_device: null argument");
    if (w == 0 || h == 0 || w > TRI_MAX_DIM || h > TRI_MAX_DIM)
        return fail(TRI_E_INVALID, "tri_upload_ai_frame_device: extent %ux%u outside 1..%d", w, h, TRI_MAX_DIM);
    if (channels < 1 || channels > 4) return fail(TRI_E_INVALID, "tri_upload_ai_frame_device: %u channels outside 1..4", channels);
    if ((uintptr_t)nhwc & 3u) return fail(TRI_E_INVALID, "tri_upload_ai_frame_device: the tensor must be 4-B aligned");
    if (behind && tri_internal_framegen_device(behind) != c->device)
        return fail(TRI_E_INVALID, "tri_upload_ai_frame_device: the generator is on another device");
    int rc = make_current(c);
    if (rc) return rc;
    if ((size_t)w * h > c->d_ai.cap || !c->d_ai) {  // a queued frame may still sample the buffer that grow() frees
        TRI_HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = c->d_ai.grow((size_t)w * h))) return rc;
    }
    if (behind)
        if (hipEvent_t done = tri_internal_framegen_done(behind)) TRI_HIP_TRY(hipStreamWaitEvent(c->stream, done, 0));
    TRI_HIP_TRY(tri_launch_ai_pack(static_cast<const float*>(nhwc), (uint64_t)w * h, channels, c->d_ai, c->stream));
    if (behind) {  // the generator's next job overwrites the tensor: it waits for this read
        if ((rc = c->ai_packed.ensure(hipEventDisableTiming))) return rc;
        TRI_HIP_TRY(hipEventRecord(c->ai_packed.e, c->stream));
        TRI_HIP_TRY(tri_internal_framegen_reader(behind, c->ai_packed.e));
    }
    c->ai_w = w;
    c->ai_h = h;
    return TRI_OK;
}

int tri_read_ai_frame(tri_ctx* c, uint8_t* rgba8) {
    if (!c || !rgba8) return fail(TRI_E_INVALID, "tri_read_ai_frame: null argument");
    if (!c->ai_w || !c->d_ai) return fail(TRI_E_STATE, "tri_read_ai_frame: no AI frame uploaded");
    const int rc = make_current(c);
    if (rc) return rc;
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    TRI_HIP_TRY(hipMemcpy(rgba8, c->d_ai, (size_t)c->ai_w * c->ai_h * 4, hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_set_shadow(tri_ctx* c, const tri_shadow_config* cfg) {
    if (!c) return fail(TRI_E_INVALID, "tri_set_shadow: null context");
    if (!cfg || cfg->size == 0) {
        c->shadow = tri_shadow_config{};
        c->shadow_rendered = false;
        return TRI_OK;
    }
    if (cfg->size > TRI_MAX_DIM) return fail(TRI_E_INVALID, "tri_set_shadow: map size %u > %d", cfg->size, TRI_MAX_DIM);
    const float* m = cfg->light_view_proj;
    if (m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f)
        return fail(TRI_E_INVALID, "tri_set_shadow: light_view_proj must be affine (an orthographic light)");
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(m[i])) return fail(TRI_E_INVALID, "tri_set_shadow: non-finite light transform");
    if (!std::isfinite(cfg->depth_bias) || !std::isfinite(cfg->slope_bias))
        return fail(TRI_E_INVALID, "tri_set_shadow: non-finite depth bias");
    int rc = make_current(c);
    if (rc) return rc;
    const uint32_t nbx = (cfg->size + 31) / 32;
    if (cfg->size != c->shadow.size) {  // new map grid: fresh (zeroed) queue counters
        TRI_HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = c->d_sbin_count.grow((size_t)nbx * nbx))) return rc;
        TRI_HIP_TRY(hipMemsetAsync(c->d_sbin_count, 0, (size_t)nbx * nbx * 4, c->stream));
        c->s_bin_cap = 0;
        c->shadow_rendered = false;
    }
    c->shadow = *cfg;
    c->s_nbx = nbx;
    c->s_nbins = nbx * nbx;
    return TRI_OK;
}

int tri_shadow_fit_ortho(const float dir[3], const float mn[3], const float mx[3], float out[16]) {
    if (!dir || !mn || !mx || !out) return fail(TRI_E_INVALID, "tri_shadow_fit_ortho: null argument");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(mn[a]) || !std::isfinite(mx[a]) || mn[a] > mx[a])
            return fail(TRI_E_INVALID, "tri_shadow_fit_ortho: bad box");
    fsel::shadow_fit_ortho(dir, mn, mx, out);
    return TRI_OK;
}

int tri_read_shadow_map(tri_ctx* c, uint32_t* out) {
    if (!c || !out) return fail(TRI_E_INVALID, "tri_read_shadow_map: null argument");
    if (!c->shadow.size || !c->shadow_rendered) return fail(TRI_E_STATE, "tri_read_shadow_map: no shadow pass rendered");
    int rc = tri_synchronize(c);
    if (rc) return rc;
    TRI_HIP_TRY(hipMemcpy(out, c->d_shadow, (size_t)c->shadow.size * c->shadow.size * 4, hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_font_create(int32_t device, const uint8_t* alpha, uint32_t width, uint32_t height, tri_font** out) {
    if (!alpha || !out) return fail(TRI_E_INVALID, "tri_font_create: null argument");
    *out = nullptr;
    if (const int rc = tri_check_extent("tri_font_create", width, height, "atlas")) return rc;
    int dev = 0;
    if (const int rc = tri_resolve_device(device, "tri_font_create", &dev)) return rc;
    TRI_HIP_TRY(hipSetDevice(dev));
    tri_font* f = new tri_font();
    f->device = dev;
    f->w = width;
    f->h = height;
    const size_t bytes = (size_t)width * height;
    if (hipMalloc(reinterpret_cast<void**>(&f->d_alpha.p), bytes) != hipSuccess) {
        delete f;
        return fail(TRI_E_OOM, "tri_font_create: atlas allocation failed");
    }
    f->d_alpha.cap = bytes;
    // a blocking copy, then the device idle: contexts read the atlas on non-blocking streams of their own
    if (hipMemcpy(f->d_alpha, alpha, bytes, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete f;
        return fail(TRI_E_HIP, "tri_font_create: atlas upload failed");
    }
    *out = f;
    return TRI_OK;
}

int tri_font_destroy(tri_font* f) {
    if (!f) return TRI_OK;
    (void)hipSetDevice(f->device);
    delete f;  // (hipFree waits for the device: no text pass still samples the atlas)
    return TRI_OK;
}

int tri_set_text(tri_ctx* c, tri_font* font, const tri_text_quad* q, uint32_t n) {
    if (!c) return fail(TRI_E_INVALID, "tri_set_text: null context");
    if (n && !q) return fail(TRI_E_INVALID, "tri_set_text: null quads");
    if (n > TRI_MAX_TEXT_QUADS) return fail(TRI_E_INVALID, "tri_set_text: %u quads (at most %u)", n, TRI_MAX_TEXT_QUADS);
    if (font && n) {
        if (font->device != c->device)
            return fail(TRI_E_INVALID, "tri_set_text: font on device %d, context on device %d", font->device, c->device);
        if (!tri_text_quads_finite(q, n)) return fail(TRI_E_INVALID, "tri_set_text: non-finite quad coordinate");
    }
    if (!font || !n) {  // no overlay: tri_render enqueues exactly the frame's own launches
        c->text_font = nullptr;
        c->text_quads.clear();
        c->text_plan = TriTextPlan{};
        c->text_dirty = false;
        return TRI_OK;
    }
    c->text_font = font;
    if (n == c->text_quads.size() && std::memcmp(c->text_quads.data(), q, n * sizeof(tri_text_quad)) == 0)
        return TRI_OK;  // unchanged (a static label): keep the device image
    c->text_quads.assign(q, q + n);
    c->text_dirty = true;
    return TRI_OK;
}

}  // extern "C"
