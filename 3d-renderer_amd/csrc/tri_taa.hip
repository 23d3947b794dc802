// tri_taa.hip — the temporal anti-aliasing entry points of the C-ABI (include/tri_raster.h "temporal anti-aliasing"):
// the jitter, an object of its own that keeps the accumulated colour of one view (16-bit) and the ids it was
// accumulated under, twice, outside any context, the pass that resolves a jittered frame over it (k_taa_resolve,
// taa_pass.hip), the readers, and the presentation blit of the resolved image. The per-pixel rule, the jitter and
// every argument rule are in taa_math.h (plain C++, checked on the CPU by host/tools/taa_check.cpp). Every argument
// check comes before the device is made current.
//
// Ordering: as tri_history's. A pass runs on the stream of the context it reads, behind that context's tri_render. The
// object's event `done` is recorded behind every pass and waited for by the next one and by the blit, which may run on
// another context's stream; the readers wait for it on the host.
#include "taa_math.h"
#include "tri_ctx.h"

struct tri_taa {
    int device = 0;
    uint32_t W = 0, H = 0;
    DevBuf<uint2> acc[2];  // four uint16 per pixel, B G R A
    DevBuf<uint32_t> ids[2];
    DevBuf<uint32_t> resolved;
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

size_t pixels(const tri_taa* t) { return (size_t)t->W * (size_t)t->H; }

// Add a finished stamped pass to the sums. wait: block for it; otherwise leave it pending when it has not finished.
int collect(tri_taa* t, bool wait) {
    if (!t->stamped) return TRI_OK;
    if (wait) TRI_HIP_TRY(hipEventSynchronize(t->stamp[1].e));
    else {
        const hipError_t q = hipEventQuery(t->stamp[1].e);
        if (q == hipErrorNotReady) return TRI_OK;
        TRI_HIP_TRY(q);
    }
    float ms = 0.0f;
    TRI_HIP_TRY(hipEventElapsedTime(&ms, t->stamp[0].e, t->stamp[1].e));
    t->acc_ms += ms;
    t->acc_passes += 1;
    t->stamped = false;
    return TRI_OK;
}

int reader_ready(tri_taa* t, const char* who) {
    if (!t->has_output) return fail(TRI_E_STATE, "%s: no pass has run (tri_taa_resolve)", who);
    TRI_HIP_TRY(hipSetDevice(t->device));
    TRI_HIP_TRY(hipEventSynchronize(t->done.e));
    return TRI_OK;
}

void fill_image(const tri_taa* t, tri_image* out, void* p, uint32_t bytes_per_pixel, uint32_t format) {
    out->device_ptr = p;
    out->width = t->W;
    out->height = t->H;
    out->pitch_bytes = t->W * bytes_per_pixel;
    out->format = format;
    out->device = t->device;
    out->reserved = 0;
}

// The object against the context whose frame it reads (tri_taa_resolve, tri_taa_blit_linear).
int check_pair(const tri_taa* t, const tri_ctx* c, const char* who) {
    history::Msg m;
    if (const int rc = history::check_context(t->device, t->W, t->H, c->device, (uint32_t)c->W, (uint32_t)c->H, m))
        return fail(rc, "%s: %s", who, m.text);
    return TRI_OK;
}

}  // namespace

extern "C" {

int tri_taa_jitter(uint32_t index, uint32_t period, float xy[2]) {
    taa::Msg m;
    if (const int rc = taa::jitter(index, period, xy, m)) return fail(rc, "tri_taa_jitter: %s", m.text);
    return TRI_OK;
}

int tri_taa_jitter_projection(const float proj[16], float jx, float jy, uint32_t width, uint32_t height, float out[16]) {
    taa::Msg m;
    if (const int rc = taa::jitter_projection(proj, jx, jy, width, height, out, m))
        return fail(rc, "tri_taa_jitter_projection: %s", m.text);
    return TRI_OK;
}

int tri_taa_create(int32_t device, uint32_t width, uint32_t height, tri_taa** out) {
    if (!out) return fail(TRI_E_INVALID, "tri_taa_create: null argument");
    *out = nullptr;
    history::Msg m;
    if (const int rc = history::check_extent(width, height, m)) return fail(rc, "tri_taa_create: %s", m.text);
    int dev = 0;
    if (const int rc = tri_resolve_device(device, "tri_taa_create", &dev)) return rc;
    TRI_HIP_TRY(hipSetDevice(dev));
    tri_taa* t = new tri_taa;
    t->device = dev;
    t->W = width;
    t->H = height;
    const size_t n = pixels(t);
    int rc = TRI_OK;
    for (int s = 0; s < 2 && !rc; ++s) {
        if (!rc) rc = t->acc[s].grow(n);
        if (!rc) rc = t->ids[s].grow(n);
    }
    if (!rc) rc = t->resolved.grow(n);
    if (!rc) rc = t->mask.grow(n);
    if (!rc) rc = t->done.ensure(hipEventDisableTiming);
    if (rc) {
        delete t;  // (the holders free what was allocated)
        return rc;
    }
    *out = t;
    return TRI_OK;
}

int tri_taa_destroy(tri_taa* t) {
    if (!t) return TRI_OK;
    (void)hipSetDevice(t->device);
    // a pass or a blit still queued on a context's stream reads and writes the buffers: wait for it before they go
    if (t->has_output) (void)hipEventSynchronize(t->done.e);
    delete t;
    return TRI_OK;
}

int tri_taa_resolve(tri_taa* t, tri_ctx* c, const tri_taa_params* params) {
    if (!t || !c) return fail(TRI_E_INVALID, "tri_taa_resolve: null argument");
    taa::Msg m;
    if (const int rc = taa::check_params(params, m)) return fail(rc, "tri_taa_resolve: %s", m.text);
    if (const int rc = check_pair(t, c, "tri_taa_resolve")) return rc;
    if (c->y0 != 0 || c->y1 != c->H)
        return fail(TRI_E_UNSUPPORTED, "tri_taa_resolve: a row-band context (the fetch and the 3 x 3 windows leave the band)");
    if (!c->motion_on) return fail(TRI_E_STATE, "tri_taa_resolve: the context's motion output is off (tri_set_motion_output)");
    if (!c->motion_rendered || c->motion_table.size() < 16 || !c->motion_stage.d.p)
        return fail(TRI_E_STATE, "tri_taa_resolve: no frame was rendered with the motion output on");
    int rc = make_current(c);
    if (rc) return rc;
    if ((rc = collect(t, false))) return rc;
    const bool stamp = c->timing && !t->stamped;
    if (stamp)
        for (int i = 0; i < 2; ++i)
            if ((rc = t->stamp[i].ensure(hipEventDefault))) return rc;
    // the object's previous pass (or a blit of its image) may have run on another context's stream
    if (t->has_output) TRI_HIP_TRY(hipStreamWaitEvent(c->stream, t->done.e, 0));

    history::Sets next = t->sets;  // committed once the pass is enqueued
    bool valid = false;
    const uint32_t rd = next.begin((params->flags & TRI_TAA_REDO) != 0, &valid), wr = rd ^ 1u;
    const history::Frame f = history::make_frame(t->W, t->H, 0.0f);
    TriTaaArgs a{};
    a.colour = c->d_color;
    a.ids = c->d_ids.p;
    a.depth = c->d_depth;
    a.table = reinterpret_cast<const float*>(c->motion_stage.d.p);
    a.prev_acc = t->acc[rd].p;
    a.prev_ids = t->ids[rd].p;
    a.next_acc = t->acc[wr].p;
    a.next_ids = t->ids[wr].p;
    a.resolved = t->resolved.p;
    a.mask = t->mask.p;
    a.W = t->W;
    a.H = t->H;
    a.ndraws = (uint32_t)(c->motion_table.size() / 16 - 1);  // the rows of the table the frame staged
    a.sx = f.sx;
    a.sy = f.sy;
    a.hw = f.hw;
    a.hh = f.hh;
    a.alpha = params->alpha;
    a.has_prev = valid ? 1u : 0u;
    a.reject_id = (params->flags & TRI_TAA_REJECT_ID) ? 1u : 0u;
    if (stamp) TRI_HIP_TRY(hipEventRecord(t->stamp[0].e, c->stream));
    TRI_HIP_TRY(tri_launch_taa_resolve(a, c->stream));
    if (stamp) {
        TRI_HIP_TRY(hipEventRecord(t->stamp[1].e, c->stream));
        t->stamped = true;
    }
    TRI_HIP_TRY(hipEventRecord(t->done.e, c->stream));
    t->sets = next;
    t->written = wr;
    t->has_output = true;
    return TRI_OK;
}

int tri_taa_reset(tri_taa* t) {
    if (!t) return fail(TRI_E_INVALID, "tri_taa_reset: null object");
    t->sets.reset();
    return TRI_OK;
}

int tri_taa_read(tri_taa* t, uint8_t* bgra8, uint16_t* rgba16, uint8_t* mask) {
    if (!t) return fail(TRI_E_INVALID, "tri_taa_read: null object");
    if (const int rc = reader_ready(t, "tri_taa_read")) return rc;
    if (bgra8) TRI_HIP_TRY(hipMemcpy(bgra8, t->resolved.p, pixels(t) * 4, hipMemcpyDeviceToHost));
    if (rgba16) TRI_HIP_TRY(hipMemcpy(rgba16, t->acc[t->written].p, pixels(t) * 8, hipMemcpyDeviceToHost));
    if (mask) TRI_HIP_TRY(hipMemcpy(mask, t->mask.p, pixels(t), hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_taa_get_output(tri_taa* t, tri_image* colour8, tri_image* colour16, tri_image* mask) {
    if (!t) return fail(TRI_E_INVALID, "tri_taa_get_output: null object");
    if (!t->has_output) return fail(TRI_E_STATE, "tri_taa_get_output: no pass has run (tri_taa_resolve)");
    if (colour8) fill_image(t, colour8, t->resolved.p, 4, TRI_FORMAT_B8G8R8A8_UNORM);
    if (colour16) fill_image(t, colour16, t->acc[t->written].p, 8, TRI_FORMAT_R16G16B16A16_UNORM);
    if (mask) fill_image(t, mask, t->mask.p, 1, TRI_FORMAT_R8_UINT);
    return TRI_OK;
}

int tri_taa_get_timing(tri_taa* t, double* ms, uint64_t* passes) {
    if (!t || !ms || !passes) return fail(TRI_E_INVALID, "tri_taa_get_timing: null argument");
    if (!t->has_output) return fail(TRI_E_STATE, "tri_taa_get_timing: no pass has run (tri_taa_resolve)");
    TRI_HIP_TRY(hipSetDevice(t->device));
    if (const int rc = collect(t, true)) return rc;
    *ms = t->acc_ms;
    *passes = t->acc_passes;
    return TRI_OK;
}

int tri_taa_blit_linear(tri_taa* t, tri_ctx* c, void* dst, uint32_t width, uint32_t height) {
    if (!t || !c) return fail(TRI_E_INVALID, "tri_taa_blit_linear: null argument");
    if (const int rc = tri_check_extent("tri_taa_blit_linear", width, height, "destination")) return rc;
    if (const int rc = check_pair(t, c, "tri_taa_blit_linear")) return rc;
    if (c->y0 != 0 || c->y1 != c->H) return fail(TRI_E_STATE, "tri_taa_blit_linear: a row-band context has no whole frame");
    if (!t->has_output) return fail(TRI_E_STATE, "tri_taa_blit_linear: no pass has run (tri_taa_resolve)");
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
    TRI_HIP_TRY(hipStreamWaitEvent(c->stream, t->done.e, 0));  // the pass may have run on another context's stream
    TRI_HIP_TRY(tri_launch_blit(t->resolved.p, (int32_t)t->W, (int32_t)t->H, out, (int32_t)width, (int32_t)height, c->d_lut + 256,
                                c->stream));
    TRI_HIP_TRY(hipEventRecord(t->done.e, c->stream));  // the next pass overwrites the image this blit reads
    return TRI_OK;
}

}  // extern "C"
