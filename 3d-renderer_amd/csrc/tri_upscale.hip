// tri_upscale.hip — the temporal upscaling entry points of the C-ABI (include/tri_raster.h "temporal upscaling"): an
// object of its own that keeps the accumulated colour of one view at the output extent (16-bit) and the ids of the last
// frame at the render extent, twice, outside any context, the pass that resolves a jittered render-extent frame over it
// (k_upscale_resolve, upscale_pass.hip), the readers, and the presentation blit of the resolved image. The per-pixel
// rule, the jitter period and every argument rule are in upscale_math.h (plain C++, checked on the CPU by
// host/tools/upscale_check.cpp). Every argument check comes before the device is made current.
//
// Ordering: as tri_taa's. A pass runs on the stream of the context it reads, behind that context's tri_render; the
// frame's ids are copied into the written set on the same stream behind the kernel. The object's event `done` is
// recorded behind every pass and waited for by the next one and by the blit, which may run on another context's stream;
// the readers wait for it on the host.
#include "upscale_math.h"
#include "tri_ctx.h"

struct tri_upscale {
    int device = 0;
    uint32_t Wr = 0, Hr = 0, Wo = 0, Ho = 0;
    DevBuf<uint2> acc[2];      // output extent: four uint16 per pixel, B G R A
    DevBuf<uint32_t> ids[2];   // render extent
    DevBuf<uint32_t> resolved; // output extent
    DevBuf<uint8_t> mask;
    history::Sets sets;
    uint32_t written = 0;     // the set the last pass stored into
    Event done;               // behind the last pass
    bool has_output = false;  // a pass was enqueued: the images hold (or will hold) a frame
    Event stamp[2];           // round a stamped pass
    bool stamped = false;     // ... whose interval has not been collected yet
    double acc_ms = 0.0;
    uint64_t acc_passes = 0;
};

namespace {

size_t out_pixels(const tri_upscale* u) { return (size_t)u->Wo * (size_t)u->Ho; }
size_t render_pixels(const tri_upscale* u) { return (size_t)u->Wr * (size_t)u->Hr; }

// Add a finished stamped pass to the sums. wait: block for it; otherwise leave it pending when it has not finished.
int collect(tri_upscale* u, bool wait) {
    if (!u->stamped) return TRI_OK;
    if (wait) TRI_HIP_TRY(hipEventSynchronize(u->stamp[1].e));
    else {
        const hipError_t q = hipEventQuery(u->stamp[1].e);
        if (q == hipErrorNotReady) return TRI_OK;
        TRI_HIP_TRY(q);
    }
    float ms = 0.0f;
    TRI_HIP_TRY(hipEventElapsedTime(&ms, u->stamp[0].e, u->stamp[1].e));
    u->acc_ms += ms;
    u->acc_passes += 1;
    u->stamped = false;
    return TRI_OK;
}

int reader_ready(tri_upscale* u, const char* who) {
    if (!u->has_output) return fail(TRI_E_STATE, "%s: no pass has run (tri_upscale_resolve)", who);
    TRI_HIP_TRY(hipSetDevice(u->device));
    TRI_HIP_TRY(hipEventSynchronize(u->done.e));
    return TRI_OK;
}

void fill_image(const tri_upscale* u, tri_image* out, void* p, uint32_t bytes_per_pixel, uint32_t format) {
    out->device_ptr = p;
    out->width = u->Wo;
    out->height = u->Ho;
    out->pitch_bytes = u->Wo * bytes_per_pixel;
    out->format = format;
    out->device = u->device;
    out->reserved = 0;
}

// The object against the context whose frame it reads (tri_upscale_resolve, tri_upscale_blit_linear): the context's
// extent is the object's render extent.
int check_pair(const tri_upscale* u, const tri_ctx* c, const char* who) {
    history::Msg m;
    if (const int rc = history::check_context(u->device, u->Wr, u->Hr, c->device, (uint32_t)c->W, (uint32_t)c->H, m))
        return fail(rc, "%s: %s (the render extent)", who, m.text);
    return TRI_OK;
}

}  // namespace

extern "C" {

int tri_upscale_jitter_period(uint32_t render_w, uint32_t render_h, uint32_t out_w, uint32_t out_h, uint32_t* period) {
    upscale::Msg m;
    if (const int rc = upscale::jitter_period(render_w, render_h, out_w, out_h, period, m))
        return fail(rc, "tri_upscale_jitter_period: %s", m.text);
    return TRI_OK;
}

int tri_upscale_create(int32_t device, uint32_t render_w, uint32_t render_h, uint32_t out_w, uint32_t out_h, tri_upscale** out) {
    if (!out) return fail(TRI_E_INVALID, "tri_upscale_create: null argument");
    *out = nullptr;
    upscale::Msg m;
    if (const int rc = upscale::check_extents(render_w, render_h, out_w, out_h, m)) return fail(rc, "tri_upscale_create: %s", m.text);
    int dev = 0;
    if (const int rc = tri_resolve_device(device, "tri_upscale_create", &dev)) return rc;
    TRI_HIP_TRY(hipSetDevice(dev));
    tri_upscale* u = new tri_upscale;
    u->device = dev;
    u->Wr = render_w;
    u->Hr = render_h;
    u->Wo = out_w;
    u->Ho = out_h;
    int rc = TRI_OK;
    for (int s = 0; s < 2 && !rc; ++s) {
        if (!rc) rc = u->acc[s].grow(out_pixels(u));
        if (!rc) rc = u->ids[s].grow(render_pixels(u));
    }
    if (!rc) rc = u->resolved.grow(out_pixels(u));
    if (!rc) rc = u->mask.grow(out_pixels(u));
    if (!rc) rc = u->done.ensure(hipEventDisableTiming);
    if (rc) {
        delete u;  // (the holders free what was allocated)
        return rc;
    }
    *out = u;
    return TRI_OK;
}

int tri_upscale_destroy(tri_upscale* u) {
    if (!u) return TRI_OK;
    (void)hipSetDevice(u->device);
    // a pass or a blit still queued on a context's stream reads and writes the buffers: wait for it before they go
    if (u->has_output) (void)hipEventSynchronize(u->done.e);
    delete u;
    return TRI_OK;
}

int tri_upscale_resolve(tri_upscale* u, tri_ctx* c, const tri_upscale_params* params) {
    if (!u || !c) return fail(TRI_E_INVALID, "tri_upscale_resolve: null argument");
    upscale::Msg m;
    if (const int rc = upscale::check_params(params, m)) return fail(rc, "tri_upscale_resolve: %s", m.text);
    if (const int rc = check_pair(u, c, "tri_upscale_resolve")) return rc;
    if (c->y0 != 0 || c->y1 != c->H)
        return fail(TRI_E_UNSUPPORTED, "tri_upscale_resolve: a row-band context (the samples and the 3 x 3 windows leave the band)");
    if (!c->motion_on) return fail(TRI_E_STATE, "tri_upscale_resolve: the context's motion output is off (tri_set_motion_output)");
    if (!c->motion_rendered || c->motion_table.size() < 16 || !c->motion_stage.d.p)
        return fail(TRI_E_STATE, "tri_upscale_resolve: no frame was rendered with the motion output on");
    int rc = make_current(c);
    if (rc) return rc;
    if ((rc = collect(u, false))) return rc;
    const bool stamp = c->timing && !u->stamped;
    if (stamp)
        for (int i = 0; i < 2; ++i)
            if ((rc = u->stamp[i].ensure(hipEventDefault))) return rc;
    // the object's previous pass (or a blit of its image) may have run on another context's stream
    if (u->has_output) TRI_HIP_TRY(hipStreamWaitEvent(c->stream, u->done.e, 0));

    history::Sets next = u->sets;  // committed once the pass is enqueued
    bool valid = false;
    const uint32_t rd = next.begin((params->flags & TRI_UPSCALE_REDO) != 0, &valid), wr = rd ^ 1u;
    const upscale::Scale s = upscale::make_scale(u->Wr, u->Hr, u->Wo, u->Ho);
    const history::Frame f = history::make_frame(u->Wo, u->Ho, 0.0f);
    TriUpscaleArgs a{};
    a.colour = c->d_color;
    a.ids = c->d_ids.p;
    a.depth = c->d_depth;
    a.table = reinterpret_cast<const float*>(c->motion_stage.d.p);
    a.prev_acc = u->acc[rd].p;
    a.prev_ids = u->ids[rd].p;
    a.next_acc = u->acc[wr].p;
    a.resolved = u->resolved.p;
    a.mask = u->mask.p;
    a.Wr = s.Wr;
    a.Hr = s.Hr;
    a.Wo = s.Wo;
    a.Ho = s.Ho;
    a.ndraws = (uint32_t)(c->motion_table.size() / 16 - 1);  // the rows of the table the frame staged
    a.rx = s.rx;
    a.ry = s.ry;
    a.ox = s.ox;
    a.oy = s.oy;
    a.sx = f.sx;
    a.sy = f.sy;
    a.hw = f.hw;
    a.hh = f.hh;
    a.alpha = params->alpha;
    a.jx = params->jitter[0];
    a.jy = params->jitter[1];
    a.has_prev = valid ? 1u : 0u;
    a.reject_id = (params->flags & TRI_UPSCALE_REJECT_ID) ? 1u : 0u;
    if (stamp) TRI_HIP_TRY(hipEventRecord(u->stamp[0].e, c->stream));
    TRI_HIP_TRY(tri_launch_upscale_resolve(a, c->stream));
    // I = the frame's ids, for every render pixel: a copy on the same stream, ahead of the event
    TRI_HIP_TRY(hipMemcpyAsync(u->ids[wr].p, c->d_ids.p, render_pixels(u) * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    if (stamp) {
        TRI_HIP_TRY(hipEventRecord(u->stamp[1].e, c->stream));
        u->stamped = true;
    }
    TRI_HIP_TRY(hipEventRecord(u->done.e, c->stream));
    u->sets = next;
    u->written = wr;
    u->has_output = true;
    return TRI_OK;
}

int tri_upscale_reset(tri_upscale* u) {
    if (!u) return fail(TRI_E_INVALID, "tri_upscale_reset: null object");
    u->sets.reset();
    return TRI_OK;
}

int tri_upscale_read(tri_upscale* u, uint8_t* bgra8, uint16_t* rgba16, uint8_t* mask) {
    if (!u) return fail(TRI_E_INVALID, "tri_upscale_read: null object");
    if (const int rc = reader_ready(u, "tri_upscale_read")) return rc;
    if (bgra8) TRI_HIP_TRY(hipMemcpy(bgra8, u->resolved.p, out_pixels(u) * 4, hipMemcpyDeviceToHost));
    if (rgba16) TRI_HIP_TRY(hipMemcpy(rgba16, u->acc[u->written].p, out_pixels(u) * 8, hipMemcpyDeviceToHost));
    if (mask) TRI_HIP_TRY(hipMemcpy(mask, u->mask.p, out_pixels(u), hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_upscale_read_ids(tri_upscale* u, uint32_t* ids) {
    if (!u) return fail(TRI_E_INVALID, "tri_upscale_read_ids: null object");
    if (const int rc = reader_ready(u, "tri_upscale_read_ids")) return rc;
    if (ids) TRI_HIP_TRY(hipMemcpy(ids, u->ids[u->written].p, render_pixels(u) * 4, hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_upscale_get_output(tri_upscale* u, tri_image* colour8, tri_image* colour16, tri_image* mask) {
    if (!u) return fail(TRI_E_INVALID, "tri_upscale_get_output: null object");
    if (!u->has_output) return fail(TRI_E_STATE, "tri_upscale_get_output: no pass has run (tri_upscale_resolve)");
    if (colour8) fill_image(u, colour8, u->resolved.p, 4, TRI_FORMAT_B8G8R8A8_UNORM);
    if (colour16) fill_image(u, colour16, u->acc[u->written].p, 8, TRI_FORMAT_R16G16B16A16_UNORM);
    if (mask) fill_image(u, mask, u->mask.p, 1, TRI_FORMAT_R8_UINT);
    return TRI_OK;
}

int tri_upscale_get_timing(tri_upscale* u, double* ms, uint64_t* passes) {
    if (!u || !ms || !passes) return fail(TRI_E_INVALID, "tri_upscale_get_timing: null argument");
    if (!u->has_output) return fail(TRI_E_STATE, "tri_upscale_get_timing: no pass has run (tri_upscale_resolve)");
    TRI_HIP_TRY(hipSetDevice(u->device));
    if (const int rc = collect(u, true)) return rc;
    *ms = u->acc_ms;
    *passes = u->acc_passes;
    return TRI_OK;
}

int tri_upscale_blit_linear(tri_upscale* u, tri_ctx* c, void* dst, uint32_t width, uint32_t height) {
    if (!u || !c) return fail(TRI_E_INVALID, "tri_upscale_blit_linear: null argument");
    if (const int rc = tri_check_extent("tri_upscale_blit_linear", width, height, "destination")) return rc;
    if (const int rc = check_pair(u, c, "tri_upscale_blit_linear")) return rc;
    if (c->y0 != 0 || c->y1 != c->H) return fail(TRI_E_STATE, "tri_upscale_blit_linear: a row-band context has no whole frame");
    if (!u->has_output) return fail(TRI_E_STATE, "tri_upscale_blit_linear: no pass has run (tri_upscale_resolve)");
    int rc = make_current(c);
    if (rc) return rc;
    uint32_t* out = static_cast<uint32_t*>(dst);
    if (!out) {  // the context's present image, as tri_blit_linear
        if ((size_t)width * height > c->d_present.cap) TRI_HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = c->d_present.grow((size_t)width * height))) return rc;
        out = c->d_present;
        c->present_w = width;
        c->present_h = height;
    } else {
        c->present_w = c->present_h = 0;  // the owned target no longer holds the latest blit: read_present fails
    }
    TRI_HIP_TRY(hipStreamWaitEvent(c->stream, u->done.e, 0));  // the pass may have run on another context's stream
    TRI_HIP_TRY(tri_launch_blit(u->resolved.p, (int32_t)u->Wo, (int32_t)u->Ho, out, (int32_t)width, (int32_t)height, c->d_lut + 256,
                                c->stream));
    TRI_HIP_TRY(hipEventRecord(u->done.e, c->stream));  // the next pass overwrites the image this blit reads
    return TRI_OK;
}

}  // extern "C"
