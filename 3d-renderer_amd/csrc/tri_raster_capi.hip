// tri_raster_capi.hip — the C-ABI (include/tri_raster.h) over the gfx950 kernels: a context's life, its stream and
// output, the frame and draw setters, tri_render, synchronisation, readback, timing and statistics. tri_render only
// orchestrates: what a frame runs is decided by the pure functions of frame_select.h, and the objects are in
// tri_ctx.h. Geometry is in tri_geometry.hip, every other upload in tri_resources.hip. Mirrors Trident::Renderer's
// frame semantics (Renderer.cpp:5822-6051 uniforms, :5110-5151 draws, :5297-5338 readback).
#include "tri_ctx.h"

#include <chrono>
#include <string>

using fsel::unorm8_host;

namespace {

thread_local std::string g_last_error;

int upload_texture_table(tri_ctx* c) {
    if (!c->tex_dirty) return TRI_OK;
    TriTexDesc* h = c->texdesc;
    for (int s = 0; s < TRI_MAX_TEXTURE_SLOTS; ++s) {
        const int src = c->d_tex[s] ? s : 0;  // unused slots alias slot 0 (Renderer.cpp:3645-3656)
        h[s].texels = c->d_tex[src];
        h[s].w = c->tex_w[src];
        h[s].h = c->tex_h[src];
        const uint32_t p = c->tex_solid[src];
        for (int k = 0; k < 3; ++k) h[s].solid[k] = fsel::srgb_decode((p >> (8 * k)) & 0xFF);
        h[s].solid[3] = (float)(p >> 24) / 255.0f;  // alpha: linear UNORM decode
    }
    c->need_lut = fsel::slots_need_lut(h);
    c->tex_dirty = false;
    c->draws_dirty = true;  // the per-draw shade records carry the slot descriptors
    return TRI_OK;
}

// Resolve the draw list against the uploaded meshes (fsel::resolve_draws) and stage the records and base tables to
// the device: the pinned buffer is rewritten only after its previous copies ran, and the copies ride the stream.
int resolve_draws(tri_ctx* c) {
    if (!c->draws_dirty) return TRI_OK;
    fsel::DrawResolution& r = c->res;
    const uint32_t n = (uint32_t)c->draws.size();
    fsel::Msg msg;
    int rc = fsel::resolve_draws(c->draws.data(), n, c->texdesc, *c->geom, r, msg);
    if (rc) return fail(rc, "%s", msg.text);
    if ((rc = c->d_draws.grow(std::max<size_t>(n, 1)))) return rc;
    if ((rc = c->d_draw_shade.grow(std::max<size_t>(n, 1)))) return rc;
    if ((rc = c->d_vbase.grow(n + 1))) return rc;
    if ((rc = c->d_pbase.grow(n + 1))) return rc;
    if ((rc = c->d_cbase.grow(n + 1))) return rc;
    if ((rc = c->d_cvis.grow(std::max<size_t>(r.ncl_total, 1)))) return rc;
    const size_t o_shade = n * sizeof(TriDrawDev);
    const size_t o_vb = o_shade + n * sizeof(TriDrawShade);
    const size_t o_pb = o_vb + (n + 1) * 4;
    const size_t o_cb = o_pb + (n + 1) * 4;
    const size_t bytes = o_cb + (n + 1) * 4;
    if ((rc = c->draw_stage.acquire(bytes, bytes * 2, false))) return rc;
    char* st = c->draw_stage.h;
    std::memcpy(st, r.dd.data(), n * sizeof(TriDrawDev));
    std::memcpy(st + o_shade, r.ds.data(), n * sizeof(TriDrawShade));
    std::memcpy(st + o_vb, r.vb.data(), (n + 1) * 4);
    std::memcpy(st + o_pb, r.pb.data(), (n + 1) * 4);
    std::memcpy(st + o_cb, r.cb.data(), (n + 1) * 4);
    if (n) {
        TRI_HIP_TRY(hipMemcpyAsync(c->d_draws, st, n * sizeof(TriDrawDev), hipMemcpyHostToDevice, c->stream));
        TRI_HIP_TRY(hipMemcpyAsync(c->d_draw_shade, st + o_shade, n * sizeof(TriDrawShade), hipMemcpyHostToDevice,
                               c->stream));
    }
    TRI_HIP_TRY(hipMemcpyAsync(c->d_vbase, st + o_vb, (n + 1) * 4, hipMemcpyHostToDevice, c->stream));
    TRI_HIP_TRY(hipMemcpyAsync(c->d_pbase, st + o_pb, (n + 1) * 4, hipMemcpyHostToDevice, c->stream));
    TRI_HIP_TRY(hipMemcpyAsync(c->d_cbase, st + o_cb, (n + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = c->draw_stage.commit(c->stream))) return rc;
    c->draws_dirty = false;
    return TRI_OK;
}

// The text overlay's device image (TriTextPlan::blob), staged as resolve_draws stages the draws; the copy rides the
// stream behind the frames still reading the old image.
int upload_text(tri_ctx* c) {
    if (!c->text_dirty) return TRI_OK;
    tri_text_build(c->text_quads.data(), (uint32_t)c->text_quads.size(), c->W, c->y0, c->y1, c->text_plan);
    const size_t bytes = c->text_plan.blob.size();
    if (bytes) {
        Staged& st = c->text_stage;
        int rc;
        if ((rc = st.acquire(bytes, bytes * 2, true))) return rc;
        std::memcpy(st.h, c->text_plan.blob.data(), bytes);
        TRI_HIP_TRY(hipMemcpyAsync(st.d, st.h, bytes, hipMemcpyHostToDevice, c->stream));
        if ((rc = st.commit(c->stream))) return rc;
    }
    c->text_dirty = false;
    return TRI_OK;
}

int ensure_work_buffers(tri_ctx* c) {
    int rc;
    const uint32_t nslots = c->res.nslots, nprims = c->res.nprims;
    const size_t nrec = c->ovf_rec_cap;
    const size_t nvary = 3ull * ((size_t)nslots + c->ovf_vert_cap);
    // grown from the observed maximum after an overflow (check_overflow)
    c->bin_cap = fsel::bin_queue_cap(c->bin_cap, nprims, (uint32_t)std::max(c->nbins, 1));
    const size_t nlist = (size_t)c->nbins * c->bin_cap;
    if (nlist * 4 > (8ull << 30)) return fail(TRI_E_OOM, "bin queues would need %zu MB", nlist * 4 >> 20);
    // k_raster gathers varyings, snapped vertices and prim_vs records through raw buffer loads with
    // 32-bit byte offsets
    if (nvary * 16 > 0xFFFFFFFFull || (uint64_t)nprims * 16 > 0xFFFFFFFFull)
        return fail(TRI_E_INVALID, "too many vertex invocations or primitives (%zu varyings, %u primitives)", nvary,
                    nprims);
    const size_t slots1 = std::max<size_t>(nslots, 1), prims1 = std::max<size_t>(nprims, 1);
    bool realloc = c->d_clip.cap < slots1 || c->d_vary.cap < nvary || c->d_recs.cap < nrec || c->d_clip_slot.cap < prims1 ||
                   c->d_prim_vs.cap < prims1 || c->d_bin_list.cap < nlist;
    if (realloc) TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = c->d_clip.grow(slots1))) return rc;
    if ((rc = c->d_snap.grow(slots1))) return rc;
    if ((rc = c->d_oc.grow(slots1))) return rc;
    if ((rc = c->d_vary.grow(nvary))) return rc;
    if ((rc = c->d_recs.grow(nrec))) return rc;
    if ((rc = c->d_clip_slot.grow(prims1))) return rc;
    if ((rc = c->d_prim_vs.grow(prims1))) return rc;
    if ((rc = c->d_setup_stats.grow((size_t)nprims / TRI_BLOCK + 1))) return rc;
    if ((rc = c->d_bin_list.grow(nlist))) return rc;
    if (c->shadow.size) {
        c->s_bin_cap = fsel::bin_queue_cap(c->s_bin_cap, nprims, c->s_nbins);
        const size_t slist = (size_t)c->s_nbins * c->s_bin_cap;
        if (slist * 4 > (8ull << 30)) return fail(TRI_E_OOM, "shadow-map bin queues would need %zu MB", slist * 4 >> 20);
        const size_t smap = (size_t)c->shadow.size * c->shadow.size;
        if (c->d_lpos.cap < nvary / 3 || c->d_lsnap.cap < slots1 || c->d_sbin_list.cap < slist ||
            c->d_sbin_count.cap < c->s_nbins || c->d_shadow.cap < smap)
            TRI_HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = c->d_lpos.grow(nvary / 3))) return rc;
        if ((rc = c->d_lsnap.grow(slots1))) return rc;
        if ((rc = c->d_sbin_list.grow(slist))) return rc;
        if ((rc = c->d_shadow.grow(smap))) return rc;
    }
    return TRI_OK;
}

int collect_timing(tri_ctx* c) {
    if (c->pending.empty()) return TRI_OK;
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    for (TimingSet& t : c->pending) {
        float ms[kStageCount] = {}, tot;
        // stamps: vertex | setup (+ the map's binning) | shadow-map raster (only with the pre-pass) | raster
        TRI_HIP_TRY(hipEventElapsedTime(&ms[kStageVertex], t.ev[kStageVertex].e, t.ev[kStageSetup].e));
        TRI_HIP_TRY(hipEventElapsedTime(&ms[kStageSetup], t.ev[kStageSetup].e, t.ev[t.shadow ? kStageShadow : kStageRaster].e));
        if (t.shadow) TRI_HIP_TRY(hipEventElapsedTime(&ms[kStageShadow], t.ev[kStageShadow].e, t.ev[kStageRaster].e));
        TRI_HIP_TRY(hipEventElapsedTime(&ms[kStageRaster], t.ev[kStageRaster].e, t.ev[kStageCount].e));
        TRI_HIP_TRY(hipEventElapsedTime(&tot, t.ev[0].e, t.ev[kStageCount].e));
        if (t.has_id) {
            // the id pass runs between the set-up (or shadow) stamp and the raster stamp: its own stamps take it out
            // of that stage, so tri_timing's stages mean what they mean with the output off; ms_frame keeps it
            float id_ms = 0.0f;
            TRI_HIP_TRY(hipEventElapsedTime(&id_ms, t.id[0].e, t.id[1].e));
            ms[t.shadow ? kStageShadow : kStageSetup] -= id_ms;
            c->acc_id_ms += id_ms;
            c->acc_id_frames += 1;
        }
        if (t.has_motion) {  // k_motion runs behind the raster kernel, inside the raster stage's stamps: likewise
            float mo_ms = 0.0f;
            TRI_HIP_TRY(hipEventElapsedTime(&mo_ms, t.motion[0].e, t.motion[1].e));
            ms[kStageRaster] -= mo_ms;
            c->acc_motion_ms += mo_ms;
            c->acc_motion_frames += 1;
        }
        c->acc.ms_vertex += ms[kStageVertex];
        c->acc.ms_setup += ms[kStageSetup];
        c->acc.ms_shadow += ms[kStageShadow];
        c->acc.ms_raster += ms[kStageRaster];
        c->acc.ms_frame += tot;
        c->acc.frames += 1;
        c->free_sets.push_back(std::move(t));
    }
    c->pending.clear();
    return TRI_OK;
}

int check_overflow(tri_ctx* c, const TriCounters* pinned = nullptr) {
    TriCounters h;
    if (pinned) h = *pinned;  // (copied on the context's stream before the wait)
    else TRI_HIP_TRY(hipMemcpy(&h, c->d_ctr, sizeof h, hipMemcpyDeviceToHost));
    if (!h.flags) return TRI_OK;
    // the resets are stream-ordered before the next frame's kernels (the context's stream is non-blocking:
    // work on the null stream is not ordered with it)
    TRI_HIP_TRY(hipMemsetAsync(&c->d_ctr->flags, 0, 4, c->stream));
    if (h.flags & TRI_OVF_CLIP_RECORDS) c->ovf_rec_cap *= 4;
    if (h.flags & TRI_OVF_CLIP_VERTS) c->ovf_vert_cap *= 4;
    if (h.flags & TRI_OVF_BIN_LIST) {
        c->bin_cap = std::max<uint32_t>(c->bin_cap * 2, h.bin_max + h.bin_max / 4);
        c->bin_cap = (c->bin_cap + 63) & ~63u;
        TRI_HIP_TRY(hipMemsetAsync(&c->d_ctr->bin_max, 0, 4, c->stream));
    }
    if (h.flags & TRI_OVF_SHADOW_BIN_LIST) {
        c->s_bin_cap = std::max<uint32_t>(c->s_bin_cap * 2, h.sbin_max + h.sbin_max / 4);
        c->s_bin_cap = (c->s_bin_cap + 63) & ~63u;
        TRI_HIP_TRY(hipMemsetAsync(&c->d_ctr->sbin_max, 0, 4, c->stream));
    }
    int rc = ensure_work_buffers(c);
    if (rc) return rc;
    return fail(TRI_E_OVERFLOW, "frame overflowed an internal buffer (flags 0x%x); capacities grown, re-render",
                h.flags);
}

// The bin grid fsel::choose_bin_log2 picks for the resolved draws; a change waits for the queued frames.
int choose_bin_grid(tri_ctx* c) {
    const int bl = fsel::choose_bin_log2(c->W, c->H, c->y0, c->y1, c->res.nprims);
    if (bl == c->bin_log2) return TRI_OK;
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));  // queued frames still use the old grid
    int rc;
    const int32_t bs = 1 << bl;
    c->bin_log2 = bl;
    c->nbx = (c->W + bs - 1) / bs;
    c->nby = (c->y1 - c->y0 + bs - 1) / bs;
    c->nbins = c->nbx * c->nby;
    c->bin_cap = 0;  // re-derived for the new grid by ensure_work_buffers
    if ((rc = c->d_bin_count.grow((size_t)c->nbins))) return rc;
    TRI_HIP_TRY(hipMemsetAsync(c->d_bin_count, 0, (size_t)c->nbins * 4, c->stream));  // before this frame's k_setup
    return TRI_OK;
}

}  // namespace

hipStream_t tri_internal_stream(tri_ctx* c) { return c->stream; }
int tri_internal_device(tri_ctx* c) { return c->device; }
bool tri_internal_whole_frame(tri_ctx* c) { return c->y0 == 0 && c->y1 == c->H; }
int tri_internal_fail(int code, const char* msg) {
    g_last_error = msg;
    return code;
}
int tri_hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? TRI_E_OOM : TRI_E_HIP, "%s: %s", what, hipGetErrorString(e));
}
const float* tri_internal_unorm_lut(tri_ctx* c) { return c->d_lut + 256; }

int tri_resolve_device(int32_t requested, const char* who, int* device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TRI_E_HIP, "%s: no HIP device available", who);
    if (requested >= ndev) return fail(TRI_E_INVALID, "%s: device %d of %d", who, requested, ndev);
    *device = requested;
    if (requested < 0) {
        const hipError_t e = hipGetDevice(device);
        if (e != hipSuccess) return fail(TRI_E_HIP, "%s: hipGetDevice: %s", who, hipGetErrorString(e));
    }
    return TRI_OK;
}

int tri_check_extent(const char* who, uint32_t w, uint32_t h, const char* what) {
    if (w == 0 || h == 0 || w > TRI_MAX_DIM || h > TRI_MAX_DIM)
        return fail(TRI_E_INVALID, "%s: %s %ux%u outside 1..%d", who, what, w, h, TRI_MAX_DIM);
    return TRI_OK;
}

int tri_check_bgra_source(const char* who, const void* bgra, uint32_t w, uint32_t h, uint32_t pitch_bytes) {
    if (!bgra) return fail(TRI_E_INVALID, "%s: null pointer", who);
    if (const int rc = tri_check_extent(who, w, h)) return rc;
    if (pitch_bytes < w * 4u || (pitch_bytes & 3u))
        return fail(TRI_E_INVALID, "%s: pitch below width * 4 or not a multiple of 4", who);
    if ((uintptr_t)bgra & 3u) return fail(TRI_E_INVALID, "%s: source must be 4-B aligned", who);
    return TRI_OK;
}

extern "C" {

const char* tri_last_error(void) { return g_last_error.c_str(); }
int tri_abi_version(void) { return TRI_RASTER_ABI_VERSION; }

int tri_create(const tri_config* cfg, tri_ctx** out) {
    if (!cfg || !out) return fail(TRI_E_INVALID, "tri_create: null argument");
    *out = nullptr;
    int rc = tri_check_extent("tri_create", cfg->width, cfg->height, "framebuffer");
    if (rc) return rc;
    uint32_t y0 = cfg->band_y0, y1 = cfg->band_y1;
    if (y0 == 0 && y1 == 0) y1 = cfg->height;
    if (y0 >= y1 || y1 > cfg->height) return fail(TRI_E_INVALID, "tri_create: bad row band [%u,%u)", y0, y1);
    int dev = 0;
    if ((rc = tri_resolve_device(cfg->device, "tri_create", &dev))) return rc;
    tri_ctx* c = new tri_ctx();
    c->cfg = *cfg;
    c->device = dev;
    c->W = (int32_t)cfg->width;
    c->H = (int32_t)cfg->height;
    c->y0 = (int32_t)y0;
    c->y1 = (int32_t)y1;
    c->bin_log2 = 0;  // the bin grid is chosen at the first tri_render (choose_bin_grid)
    auto bail = [&](int rc) { tri_destroy(c); return rc; };
    if ((rc = make_current(c))) return bail(rc);
    if (hipDeviceGetAttribute(&c->cu_count, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess ||
        c->cu_count <= 0)
        c->cu_count = 256;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(TRI_E_HIP, "tri_create: stream creation failed"));
    c->stream = c->own_stream;
    const size_t px = (size_t)c->W * (size_t)(c->y1 - c->y0);
    if (hipMalloc(&c->d_color_own.p, px * 4) != hipSuccess || hipMalloc(&c->d_depth_own.p, px * 4) != hipSuccess ||
        hipMalloc(&c->d_ctr.p, sizeof(TriCounters)) != hipSuccess ||
        hipMalloc(&c->d_lut.p, 512 * sizeof(float)) != hipSuccess)
        return bail(fail(TRI_E_OOM, "tri_create: target allocation failed"));
    c->d_color = c->d_color_own;
    c->d_depth = c->d_depth_own;
    if (hipMemset(c->d_ctr, 0, sizeof(TriCounters)) != hipSuccess)
        return bail(fail(TRI_E_HIP, "tri_create: memset failed"));
    if (hipMalloc(&c->d_args.p, sizeof(TriLaunchArgs)) != hipSuccess)
        return bail(fail(TRI_E_OOM, "tri_create: argument copy allocation failed"));
    float lut[512];
    for (int i = 0; i < 256; ++i) {  // R8G8B8A8_SRGB decode (sRGB EOTF), evaluated in double
        lut[i] = fsel::srgb_decode(i);
        lut[256 + i] = (float)i / 255.0f;  // alpha: linear UNORM decode (IEEE float division)
    }
    if (hipMemcpy(c->d_lut, lut, sizeof lut, hipMemcpyHostToDevice) != hipSuccess)
        return bail(fail(TRI_E_HIP, "tri_create: LUT upload failed"));
    const uint8_t white[4] = {0xFF, 0xFF, 0xFF, 0xFF};  // CreateDefaultTexture (Renderer.cpp:3404-3436)
    if ((rc = tri_upload_texture(c, 0, white, 1, 1))) return bail(rc);
    const float clear[4] = {0.005f, 0.005f, 0.005f, 1.0f};  // m_ClearColor default (Renderer.h:469)
    c->clear_bgra = unorm8_host(clear[2]) | (unorm8_host(clear[1]) << 8) | (unorm8_host(clear[0]) << 16) |
                    (unorm8_host(clear[3]) << 24);
    // the counters, LUT and default texture above went through null-stream copies: complete them before
    // any kernel on the context's non-blocking stream can read them
    if (hipDeviceSynchronize() != hipSuccess) return bail(fail(TRI_E_HIP, "tri_create: device synchronisation failed"));
    *out = c;
    return TRI_OK;
}

int tri_destroy(tri_ctx* c) {
    if (!c) return TRI_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;  // its members free their device memory, pinned memory and events (tri_ctx.h)
    return TRI_OK;
}

int tri_set_stream(tri_ctx* c, void* s) {
    if (!c) return fail(TRI_E_INVALID, "tri_set_stream: null context");
    hipStream_t next = s ? static_cast<hipStream_t>(s) : c->own_stream;
    if (next != c->stream && c->launched) {
        // the next frame's argument copy must not overtake the previous frame's kernels on the old stream
        int rc = make_current(c);
        if (rc) return rc;
        hipEvent_t e;
        TRI_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        TRI_HIP_TRY(hipEventRecord(e, c->stream));
        TRI_HIP_TRY(hipStreamWaitEvent(next, e, 0));
        TRI_HIP_TRY(hipEventDestroy(e));
    }
    c->stream = next;
    return TRI_OK;
}

int tri_get_stream(tri_ctx* c, void** s) {
    if (!c || !s) return fail(TRI_E_INVALID, "tri_get_stream: null argument");
    *s = c->stream;
    return TRI_OK;
}

int tri_set_frame(tri_ctx* c, const tri_global_ubo* ubo, const float clear[4]) {
    if (!c || !ubo) return fail(TRI_E_INVALID, "tri_set_frame: null argument");
    c->ubo = *ubo;
    fsel::mat4_mul(ubo->projection, ubo->view, c->pv);  // (P*V), Default.vert:104
    if (clear)
        c->clear_bgra = unorm8_host(clear[2]) | (unorm8_host(clear[1]) << 8) | (unorm8_host(clear[0]) << 16) |
                        (unorm8_host(clear[3]) << 24);
    c->frame_set = true;
    return TRI_OK;
}

// Default.frag's alpha is (base.a * tint.a) * texture.a (the UNORM decode b / 255, bilinear taps of one value
// return it exactly), stored as unorm8 by both shading builds; background pixels hold the clear colour's alpha,
// or 1 where Skybox.frag writes. The same float operations here give the byte each draw can produce.
int tri_frame_alpha(tri_ctx* c, int32_t* alpha) {
    if (!c || !alpha) return fail(TRI_E_INVALID, "tri_frame_alpha: null argument");
    int32_t a = (int32_t)(c->clear_bgra >> 24);
    bool uniform = !c->sky_size || a == 255;
    // the AI frame blend mixes every mesh fragment's alpha with the AI frame's (not proven uniform here)
    if (c->ubo.ai_blend_config[3] > 0.0f && c->ubo.ai_blend_config[0] > 0.0f && !c->draws.empty()) uniform = false;
    for (const tri_draw& d : c->draws) {
        if (!uniform) break;
        int32_t slot = d.pc.texture_slot;
        if (slot < 0 || slot >= TRI_MAX_TEXTURE_SLOTS || !c->d_tex[slot]) slot = 0;  // unused slots alias slot 0
        const int16_t ta = c->tex_alpha[slot];
        if (ta < 0) {
            uniform = false;
            break;
        }
        const float t = (float)ta / 255.0f;
        uniform = (int32_t)unorm8_host((c->mat0.base_color_factor[3] * d.pc.tint[3]) * t) == a;
    }
    if (c->text_font && !c->text_quads.empty()) uniform = false;  // the text pass blends into the alpha channel
    if (c->outline_on && !c->outline_draws.empty()) uniform = false;  // so does the selection outline
    *alpha = uniform ? a : -1;
    return TRI_OK;
}

int tri_set_draws(tri_ctx* c, const tri_draw* d, uint32_t n) {
    if (!c) return fail(TRI_E_INVALID, "tri_set_draws: null context");
    if (n && !d) return fail(TRI_E_INVALID, "tri_set_draws: null draws");
    if (n == c->draws.size() && (n == 0 || std::memcmp(c->draws.data(), d, n * sizeof(tri_draw)) == 0))
        return TRI_OK;  // unchanged draw list: keep the device copy (no per-frame upload)
    c->draws.assign(d, d + n);
    c->draws_dirty = true;
    return TRI_OK;
}

int tri_bind_output(tri_ctx* c, void* color, void* depth) {
    if (!c) return fail(TRI_E_INVALID, "tri_bind_output: null context");
    c->d_color = color ? static_cast<uint32_t*>(color) : c->d_color_own.p;
    c->d_depth = depth ? static_cast<float*>(depth) : c->d_depth_own.p;
    return TRI_OK;
}

// Diagnostics builds only (-DTRI_HOST_TIMING): tri_render's host time split at its phase boundaries (entry,
// current device, state checks and buffers, frame arguments, launches), read by tools/host_breakdown.py.
#ifdef TRI_HOST_TIMING
static double g_host_ns[5];
static uint64_t g_host_calls;
#define TRI_HSTAMP(k) const auto hs##k = std::chrono::steady_clock::now()
extern "C" void tri_debug_host_times(double* out, int reset) {
    for (int i = 0; i < 5; ++i) out[i] = g_host_calls ? g_host_ns[i] / (double)g_host_calls : 0.0;
    if (reset) { for (double& x : g_host_ns) x = 0.0; g_host_calls = 0; }
}
#else
#define TRI_HSTAMP(k) do { } while (0)
#endif

int tri_render(tri_ctx* c) {
    TRI_HSTAMP(0);
    if (!c) return fail(TRI_E_INVALID, "tri_render: null context");
    if (!c->frame_set) return fail(TRI_E_STATE, "tri_render: tri_set_frame was not called");
    if (!c->draws.empty() && !c->geom->geometry_set) return fail(TRI_E_STATE, "tri_render: draws without geometry");
    int rc = make_current(c);
    if (rc) return rc;
    TRI_HSTAMP(1);
    if ((rc = upload_texture_table(c))) return rc;
    if (c->geom->version != c->geom_seen) {  // (shared) geometry changed since the draws were resolved
        c->draws_dirty = true;
        c->geom_seen = c->geom->version;
    }
    if ((rc = resolve_draws(c))) return rc;
    const fsel::DrawResolution& res = c->res;
    if (res.any_skin && !c->geom->has_skin_data) {
        // a skinned draw over vertices without weights: skin matrix = 0 -> everything collapses
        // to the origin, exactly like the shader with all-zero weights; give the kernel zeros. The
        // geometry may be shared with contexts on other streams, so the zeros are in place (device
        // synchronised) before the shared flag says so.
        if ((rc = c->geom->d_skin.grow(std::max<uint64_t>(c->geom->nverts, 1)))) return rc;
        TRI_HIP_TRY(hipMemset(c->geom->d_skin, 0, std::max<uint64_t>(c->geom->nverts, 1) * sizeof(TriVsSkin)));
        TRI_HIP_TRY(hipDeviceSynchronize());
        c->geom->has_skin_data = true;
    }
    if ((rc = choose_bin_grid(c))) return rc;
    if ((rc = ensure_work_buffers(c))) return rc;

    TRI_HSTAMP(2);
    TriLaunchArgs& ha = c->args;  // passed by value at launch: free to rewrite for the next frame
    TriFrameParams& fp = ha.fp;
    {
        fsel::FrameState s;
        s.W = c->W; s.H = c->H; s.y0 = c->y0; s.y1 = c->y1;
        s.nbx = c->nbx; s.nby = c->nby; s.nbins = c->nbins; s.bin_log2 = c->bin_log2;
        s.flags = c->cfg.flags;
        s.cu_count = c->cu_count;
        s.setup_wgs_resident = TRI_SETUP_WGS_PER_CU;
        s.res = &res;
        s.ucol = c->geom->ucol;
        s.need_lut = c->need_lut;
        s.ubo = &c->ubo;
        s.pv = c->pv;
        s.mat0 = &c->mat0;
        s.shadow = &c->shadow;
        s.s_nbx = c->s_nbx; s.s_nbins = c->s_nbins; s.s_bin_cap = c->s_bin_cap;
        s.ai_w = c->ai_w; s.ai_h = c->ai_h;
        s.sky_size = c->sky_size; s.sky_uniform_bgra = c->sky_uniform_bgra;
        s.sky_uniform = c->sky_uniform; s.sky_prefill = c->sky_prefill;
        s.ovf_rec_cap = c->ovf_rec_cap; s.ovf_vert_cap = c->ovf_vert_cap; s.bin_cap = c->bin_cap;
        s.nbones = c->nbones;
        s.clear_bgra = c->clear_bgra;
        const char* why = nullptr;
        if ((rc = fsel::derive_frame(s, fp, &c->last_path, &c->last_nchunks, &why))) return fail(rc, "%s", why);
    }

    TriDeviceBuffers& b = ha.b;
    b.vin = c->geom->d_vin;
    b.vpos = c->geom->d_pos;
    b.vattr = c->geom->d_attr;
    b.vskin = res.any_skin ? c->geom->d_skin.p : nullptr;
    b.bones = c->d_bones;
    b.vertex_count = c->geom->nverts;
    b.indices = c->geom->d_idx;
    b.draws = c->d_draws;
    b.draw_shade = c->d_draw_shade;
    b.draw_vbase = c->d_vbase;
    b.draw_pbase = c->d_pbase;
    b.srgb_lut = c->d_lut;
    b.sky = c->d_sky;
    b.ai_frame = fp.ai_on ? c->d_ai.p : nullptr;
    b.clip = c->d_clip;
    b.snap = c->d_snap;
    b.oc = c->d_oc;
    b.vary = c->d_vary;
    b.recs = c->d_recs;
    b.clip_slot = c->d_clip_slot;
    b.prim_vs = c->d_prim_vs;
    b.setup_stats = c->d_setup_stats;
    b.bin_count = c->d_bin_count;
    b.bin_list = c->d_bin_list;
    b.counters = c->d_ctr;
    b.color = c->d_color;
    b.depth = c->d_depth;
    b.clusters = c->geom->d_clusters;
    b.vbox = c->geom->d_vbox;
    b.draw_cbase = c->d_cbase;
    b.cvis = c->d_cvis;
    b.lpos = c->d_lpos;
    b.lsnap = c->d_lsnap;
    b.sbin_count = c->d_sbin_count;
    b.sbin_list = c->d_sbin_list;
    b.shadow_map = c->d_shadow;

    hipEvent_t stamps[kStageCount + 1], *ev = nullptr;
    TimingSet ts;
    const bool timed = c->timing && (c->timing_counter++ % c->timing_period) == 0;
    if (timed) {
        if (!c->free_sets.empty()) {
            ts = std::move(c->free_sets.back());
            c->free_sets.pop_back();
        } else {
            for (Event& e : ts.ev) TRI_HIP_TRY(hipEventCreate(&e.e));
        }
        for (int i = 0; i <= kStageCount; ++i) stamps[i] = ts.ev[i].e;
        ev = stamps;
    }
    ts.shadow = fp.shadow_on != 0;
    TriFramePlan plan;
    // the motion pass (tri_set_motion_output): its table rides the stream ahead of the frame's kernels
    TriMotionArgs moa{};
    TriMotionPass mo_pass = kMotionOff;
    if (c->motion_on && (rc = tri_motion_prepare(c, &moa, &mo_pass))) return rc;
    tri_plan_frame(fp, plan, c->id_on, mo_pass);
    hipEvent_t mo_stamps[2], *mo_ev = nullptr;
    ts.has_motion = timed && mo_pass != kMotionOff;
    if (ts.has_motion) {
        for (int i = 0; i < 2; ++i) {
            if ((rc = ts.motion[i].ensure(hipEventDefault))) return rc;
            mo_stamps[i] = ts.motion[i].e;
        }
        mo_ev = mo_stamps;
    }
    hipEvent_t id_stamps[2], *id_ev = nullptr;
    ts.has_id = timed && c->id_on && fp.nchunks > 0;  // (the plan holds the id pass)
    if (ts.has_id) {
        for (int i = 0; i < 2; ++i) {
            if ((rc = ts.id[i].ensure(hipEventDefault))) return rc;
            id_stamps[i] = ts.id[i].e;
        }
        id_ev = id_stamps;
    }
    if (const int kind = tri_raster_kind(fp); kind >= 0)  // the frame-kind kernel the plan took
        c->last_path |= TRI_PATH_KIND | ((uint32_t)kind << TRI_PATH_KIND_SHIFT);
#ifdef TRI_DIAG_FRONT
    if (c->diag_frames++ > 0) tri_diag_front_plan(plan);
#endif
    TRI_HSTAMP(3);
    if (fp.sky_size && fp.sky_mode == TRI_SKY_PREFILLED) {
        TriSkyFillArgs sa{};
        sa.W = fp.W; sa.H = fp.H; sa.y0 = fp.y0; sa.y1 = fp.y1;
        sa.clear_bgra = fp.clear_bgra;
        // as the raster kernels' own pass: the exact build always takes the oracle's ray / cube path
        sa.mode = fp.sky_pw[3] == 0.0f && !fp.exact_shading ? TRI_SKY_PERSP : TRI_SKY_RAY;
        sa.format = c->sky_format; sa.size = c->sky_size; sa.mips = c->sky_mips;
        std::memcpy(sa.ip, fp.sky_ip, sizeof sa.ip);
        std::memcpy(sa.R, fp.sky_R, sizeof sa.R);
        std::memcpy(sa.pw, fp.sky_pw, sizeof sa.pw);
        std::memcpy(sa.far, fp.sky_far, sizeof sa.far);
        fsel::sky_chain_texels(c->sky_size, c->sky_mips, sa.level_texel);
        sa.texels = c->d_sky; sa.lut = c->d_lut; sa.color = c->d_color;
        TRI_HIP_TRY(tri_launch_sky_fill(sa, c->stream));
    }
    // the id pass (tri_set_id_output): in the plan ahead of the raster kernel; a frame without primitives has no queues
    // to walk and takes an all-background image
    const TriIdArgs ida{c->d_ids.p};
    if (c->id_on && fp.nchunks == 0)
        TRI_HIP_TRY(hipMemsetAsync(c->d_ids, 0, (size_t)c->W * (size_t)(c->y1 - c->y0) * 4, c->stream));
    TRI_HIP_TRY(tri_run_plan(plan, ha, c->d_args, c->stream, ev, c->id_on ? &ida : nullptr, id_ev,
                             mo_pass != kMotionOff ? &moa : nullptr, mo_ev));
    c->launched = true;
    c->ids_rendered = c->id_on;
    c->motion_rendered = c->motion_on;
    // the selection outline (tri_set_outline): over the frame, under the text
    if (c->id_on && c->outline_on && (rc = tri_ids_outline_pass(c))) return rc;
    // the text pass (TextRenderer::RecordViewport, after the mesh / sky pass): only when quads are set. A
    // TRI_E_OVERFLOW re-render restarts from the clear, so the overlay is reapplied by construction.
    if (c->text_font && !c->text_quads.empty()) {
        if ((rc = upload_text(c))) return rc;
        TRI_HIP_TRY(tri_launch_text(c->d_color, c->W, c->y0, c->y1, c->text_plan,
                                reinterpret_cast<const uint8_t*>(c->text_stage.d.p), c->text_font->d_alpha, c->text_font->w,
                                c->text_font->h, c->stream));
    }
    if (timed) c->pending.push_back(std::move(ts));
    if (fp.shadow_on) c->shadow_rendered = true;
#ifdef TRI_HOST_TIMING
    const auto hs4 = std::chrono::steady_clock::now();
    const std::chrono::steady_clock::time_point t[5] = {hs0, hs1, hs2, hs3, hs4};
    for (int i = 0; i < 4; ++i) g_host_ns[i] += (double)std::chrono::duration_cast<std::chrono::nanoseconds>(t[i + 1] - t[i]).count();
    g_host_ns[4] += (double)std::chrono::duration_cast<std::chrono::nanoseconds>(hs4 - hs0).count();
    ++g_host_calls;
#endif
    return TRI_OK;
}

int tri_synchronize(tri_ctx* c) {
    if (!c) return fail(TRI_E_INVALID, "tri_synchronize: null context");
    int rc = make_current(c);
    if (rc) return rc;
    // the counters ride the stream into pinned memory, so one wait covers the frame and its flags (a blocking
    // hipMemcpy after the wait cost the engine's per-frame fence another round trip)
    if ((rc = c->h_ctr.grow(1))) return rc;
    TRI_HIP_TRY(hipMemcpyAsync(c->h_ctr, c->d_ctr, sizeof(TriCounters), hipMemcpyDeviceToHost, c->stream));
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    return check_overflow(c, c->h_ctr);
}

int tri_readback(tri_ctx* c, uint8_t* bgra, uint32_t* depth) {
    if (!c) return fail(TRI_E_INVALID, "tri_readback: null context");
    int rc = tri_synchronize(c);
    if (rc) return rc;
    const size_t px = (size_t)c->W * (size_t)(c->y1 - c->y0);
    if (bgra) TRI_HIP_TRY(hipMemcpy(bgra, c->d_color, px * 4, hipMemcpyDeviceToHost));
    if (depth) {
        if (c->cfg.flags & TRI_FLAG_NO_DEPTH_OUTPUT)
            return fail(TRI_E_STATE, "tri_readback: depth output disabled by TRI_FLAG_NO_DEPTH_OUTPUT");
        TRI_HIP_TRY(hipMemcpy(depth, c->d_depth, px * 4, hipMemcpyDeviceToHost));
    }
    return TRI_OK;
}

int tri_get_output(tri_ctx* c, tri_image* out) {
    if (!c || !out) return fail(TRI_E_INVALID, "tri_get_output: null argument");
    out->device_ptr = c->d_color;
    out->width = (uint32_t)c->W;
    out->height = (uint32_t)(c->y1 - c->y0);
    out->pitch_bytes = (uint32_t)c->W * 4u;
    out->format = TRI_FORMAT_B8G8R8A8_UNORM;
    out->device = c->device;
    out->reserved = 0;
    return TRI_OK;
}

int tri_blit_linear(tri_ctx* c, void* dst, uint32_t width, uint32_t height) {
    if (!c) return fail(TRI_E_INVALID, "tri_blit_linear: null context");
    if (const int rc = tri_check_extent("tri_blit_linear", width, height, "destination")) return rc;
    if (c->y0 != 0 || c->y1 != c->H) return fail(TRI_E_STATE, "tri_blit_linear: a row-band context has no whole frame");
    int rc = make_current(c);
    if (rc) return rc;
    uint32_t* out = static_cast<uint32_t*>(dst);
    if (!out) {
        if ((size_t)width * height > c->d_present.cap) {
            TRI_HIP_TRY(hipStreamSynchronize(c->stream));
        }
        if ((rc = c->d_present.grow((size_t)width * height))) return rc;
        out = c->d_present;
        c->present_w = width;
        c->present_h = height;
    } else {
        c->present_w = c->present_h = 0;  // the owned target no longer holds the latest blit: read_present fails
    }
    // the alpha half of the decode LUT is the UNORM8 decode b / 255 (IEEE float division)
    TRI_HIP_TRY(tri_launch_blit(c->d_color, c->W, c->H, out, (int32_t)width, (int32_t)height, c->d_lut + 256, c->stream));
    return TRI_OK;
}

int tri_read_present(tri_ctx* c, uint8_t* bgra) {
    if (!c || !bgra) return fail(TRI_E_INVALID, "tri_read_present: null argument");
    if (!c->d_present || !c->present_w) return fail(TRI_E_STATE, "tri_read_present: nothing was blitted");
    int rc = make_current(c);
    if (rc) return rc;
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    TRI_HIP_TRY(hipMemcpy(bgra, c->d_present, (size_t)c->present_w * c->present_h * 4, hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_set_timing(tri_ctx* c, int enable) {
    if (!c) return fail(TRI_E_INVALID, "tri_set_timing: null context");
    int rc = collect_timing(c);
    if (rc) return rc;
    if (enable < 0) return fail(TRI_E_INVALID, "tri_set_timing: negative period %d", enable);
    c->timing = enable != 0;
    c->timing_period = enable > 0 ? (uint32_t)enable : 1u;
    c->timing_counter = 0;
    c->acc = tri_timing{};
    c->acc_id_ms = 0.0;
    c->acc_id_frames = 0;
    c->acc_motion_ms = 0.0;
    c->acc_motion_frames = 0;
    return TRI_OK;
}

int tri_get_timing(tri_ctx* c, tri_timing* out) {
    if (!c || !out) return fail(TRI_E_INVALID, "tri_get_timing: null argument");
    int rc = collect_timing(c);
    if (rc) return rc;
    *out = c->acc;
    return TRI_OK;
}

int tri_get_id_timing(tri_ctx* c, double* ms_id, uint64_t* frames) {
    if (!c || !ms_id || !frames) return fail(TRI_E_INVALID, "tri_get_id_timing: null argument");
    int rc = collect_timing(c);
    if (rc) return rc;
    *ms_id = c->acc_id_ms;
    *frames = c->acc_id_frames;
    return TRI_OK;
}

int tri_get_motion_timing(tri_ctx* c, double* ms_motion, uint64_t* frames) {
    if (!c || !ms_motion || !frames) return fail(TRI_E_INVALID, "tri_get_motion_timing: null argument");
    int rc = collect_timing(c);
    if (rc) return rc;
    *ms_motion = c->acc_motion_ms;
    *frames = c->acc_motion_frames;
    return TRI_OK;
}

int tri_get_frame_stats(tri_ctx* c, tri_frame_stats* out) {
    if (!c || !out) return fail(TRI_E_INVALID, "tri_get_frame_stats: null argument");
    int rc = make_current(c);
    if (rc) return rc;
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    TriCounters h;
    TRI_HIP_TRY(hipMemcpy(&h, c->d_ctr, sizeof h, hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->triangles_in = c->res.nprims;
    std::vector<uint2> ws(c->last_nchunks);
    if (!ws.empty()) TRI_HIP_TRY(hipMemcpy(ws.data(), c->d_setup_stats, ws.size() * sizeof(uint2), hipMemcpyDeviceToHost));
    uint64_t setup = h.tris_setup, entries = h.bin_entries;  // per-frame counters (0 unless a kernel adds)
    for (const uint2& w : ws) {
        setup += w.x;
        entries += w.y;
    }
    out->triangles_setup = setup;
    out->triangles_clipped = h.tris_clipped;
    out->bin_entries = entries;
    out->vertices_shaded = c->res.nslots;
    out->bins_x = (uint32_t)c->nbx;
    out->bins_y = (uint32_t)c->nby;
    out->bin_size = 1u << c->bin_log2;
    out->path = c->last_path;
    return TRI_OK;
}

}  // extern "C"
