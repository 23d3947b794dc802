// tri_history.hip — the history reprojection entry points of the C-ABI (include/tri_raster.h "history reprojection"):
// an object of its own that keeps the previous frame of one view — colour, ids, depth, twice — outside any context, the
// pass that warps it by the frame's motion (k_reproject, history_pass.hip), and the readers. The per-pixel rule and
// every argument rule are in history_math.h (plain C++, checked on the CPU by host/tools/history_check.cpp). Every
// argument check comes before the device is made current.
//
// Ordering: a pass runs on the stream of the context it reads, behind that context's tri_render. The object's event
// `done` is recorded behind every pass and waited for by the next one, which may run on another context's stream (two
// frames in flight are two contexts); the readers wait for it on the host.
#include "history_math.h"
#include "tri_ctx.h"

struct tri_history {
    int device = 0;
    uint32_t W = 0, H = 0;
    DevBuf<uint32_t> colour[2], ids[2];
    DevBuf<float> depth[2];
    DevBuf<uint32_t> warped;
    DevBuf<uint8_t> mask;
    history::Sets sets;
    Event done;            // behind the last pass
    bool has_output = false;  // a pass was enqueued: warped and mask hold (or will hold) an image
    Event stamp[2];        // round a stamped pass
    bool stamped = false;  // ... whose interval has not been collected yet
    double acc_ms = 0.0;
    uint64_t acc_passes = 0;
};

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

size_t pixels(const tri_history* h) { return (size_t)h->W * (size_t)h->H; }

// Add a finished stamped pass to the sums. wait: block for it; otherwise leave it pending when it has not finished.
int collect(tri_history* h, bool wait) {
    if (!h->stamped) return TRI_OK;
    if (wait) TRI_HIP_TRY(hipEventSynchronize(h->stamp[1].e));
    else {
        const hipError_t q = hipEventQuery(h->stamp[1].e);
        if (q == hipErrorNotReady) return TRI_OK;
        TRI_HIP_TRY(q);
    }
    float ms = 0.0f;
    TRI_HIP_TRY(hipEventElapsedTime(&ms, h->stamp[0].e, h->stamp[1].e));
    h->acc_ms += ms;
    h->acc_passes += 1;
    h->stamped = false;
    return TRI_OK;
}

int reader_ready(tri_history* h, const char* who) {
    if (!h->has_output) return fail(TRI_E_STATE, "%s: no pass has run (tri_history_reproject)", who);
    TRI_HIP_TRY(hipSetDevice(h->device));
    TRI_HIP_TRY(hipEventSynchronize(h->done.e));
    return TRI_OK;
}

void fill_image(const tri_history* h, tri_image* out, void* p, uint32_t bytes_per_pixel, uint32_t format) {
    out->device_ptr = p;
    out->width = h->W;
    out->height = h->H;
    out->pitch_bytes = h->W * bytes_per_pixel;
    out->format = format;
    out->device = h->device;
    out->reserved = 0;
}

}  // namespace

extern "C" {

int tri_history_create(int32_t device, uint32_t width, uint32_t height, tri_history** out) {
    if (!out) return fail(TRI_E_INVALID, "tri_history_create: null argument");
    *out = nullptr;
    history::Msg m;
    if (const int rc = history::check_extent(width, height, m)) return fail(rc, "tri_history_create: %s", m.text);
    int dev = 0;
    if (const int rc = tri_resolve_device(device, "tri_history_create", &dev)) return rc;
    TRI_HIP_TRY(hipSetDevice(dev));
    tri_history* h = new tri_history;
    h->device = dev;
    h->W = width;
    h->H = height;
    const size_t n = pixels(h);
    int rc = TRI_OK;
    for (int s = 0; s < 2 && !rc; ++s) {
        if (!rc) rc = h->colour[s].grow(n);
        if (!rc) rc = h->ids[s].grow(n);
        if (!rc) rc = h->depth[s].grow(n);
    }
    if (!rc) rc = h->warped.grow(n);
    if (!rc) rc = h->mask.grow((n + 3) & ~(size_t)3);
    if (!rc) rc = h->done.ensure(hipEventDisableTiming);
    if (rc) {
        delete h;  // (the holders free what was allocated)
        return rc;
    }
    *out = h;
    return TRI_OK;
}

int tri_history_destroy(tri_history* h) {
    if (!h) return TRI_OK;
    (void)hipSetDevice(h->device);
    // a pass still queued on a context's stream reads and writes the buffers: wait for it before they go
    if (h->has_output) (void)hipEventSynchronize(h->done.e);
    delete h;
    return TRI_OK;
}

int tri_history_reproject(tri_history* h, tri_ctx* c, const tri_reproject_params* params) {
    if (!h || !c) return fail(TRI_E_INVALID, "tri_history_reproject: null argument");
    history::Msg m;
    if (const int rc = history::check_params(params, m)) return fail(rc, "tri_history_reproject: %s", m.text);
    if (const int rc = history::check_context(h->device, h->W, h->H, c->device, (uint32_t)c->W, (uint32_t)c->H, m))
        return fail(rc, "tri_history_reproject: %s", m.text);
    if (c->y0 != 0 || c->y1 != c->H)
        return fail(TRI_E_UNSUPPORTED, "tri_history_reproject: a row-band context (the fetch leaves the band)");
    if (!c->motion_on) return fail(TRI_E_STATE, "tri_history_reproject: the context's motion output is off (tri_set_motion_output)");
    if (!c->motion_rendered || c->motion_table.size() < 16 || !c->motion_stage.d.p)
        return fail(TRI_E_STATE, "tri_history_reproject: no frame was rendered with the motion output on");
    int rc = make_current(c);
    if (rc) return rc;
    if ((rc = collect(h, false))) return rc;
    const bool stamp = c->timing && !h->stamped;
    if (stamp)
        for (int i = 0; i < 2; ++i)
            if ((rc = h->stamp[i].ensure(hipEventDefault))) return rc;
    // the object's previous pass may have run on another context's stream
    if (h->has_output) TRI_HIP_TRY(hipStreamWaitEvent(c->stream, h->done.e, 0));

    history::Sets next = h->sets;  // committed once the pass is enqueued
    bool valid = false;
    const uint32_t rd = next.begin((params->flags & TRI_HISTORY_REDO) != 0, &valid), wr = rd ^ 1u;
    const history::Frame f = history::make_frame(h->W, h->H, params->depth_tolerance);
    TriReprojectArgs a{};
    a.colour = c->d_color;
    a.ids = c->d_ids.p;
    a.depth = c->d_depth;
    a.table = reinterpret_cast<const float*>(c->motion_stage.d.p);
    a.prev_colour = h->colour[rd].p;
    a.prev_ids = h->ids[rd].p;
    a.prev_depth = h->depth[rd].p;
    a.next_colour = h->colour[wr].p;
    a.next_ids = h->ids[wr].p;
    a.next_depth = h->depth[wr].p;
    a.warped = h->warped.p;
    a.mask = h->mask.p;
    a.W = h->W;
    a.H = h->H;
    a.npix = (uint32_t)pixels(h);  // (2^31 pixels at the most: check_extent; a context holds far fewer)
    a.ndraws = (uint32_t)(c->motion_table.size() / 16 - 1);  // the rows of the table the frame staged
    a.sx = f.sx;
    a.sy = f.sy;
    a.hw = f.hw;
    a.hh = f.hh;
    a.tolerance = f.tolerance;
    a.has_prev = valid ? 1u : 0u;
    // the object's images and the context's own come from hipMalloc; a caller's targets (tri_bind_output) may start anywhere
    const bool vec4 = aligned16(a.colour) && aligned16(a.ids) && aligned16(a.depth);
    if (stamp) TRI_HIP_TRY(hipEventRecord(h->stamp[0].e, c->stream));
    TRI_HIP_TRY(tri_launch_reproject(a, vec4, c->stream));
    if (stamp) {
        TRI_HIP_TRY(hipEventRecord(h->stamp[1].e, c->stream));
        h->stamped = true;
    }
    TRI_HIP_TRY(hipEventRecord(h->done.e, c->stream));
    h->sets = next;
    h->has_output = true;
    return TRI_OK;
}

int tri_history_reset(tri_history* h) {
    if (!h) return fail(TRI_E_INVALID, "tri_history_reset: null history");
    h->sets.reset();
    return TRI_OK;
}

int tri_history_read(tri_history* h, uint8_t* bgra8, uint8_t* mask) {
    if (!h) return fail(TRI_E_INVALID, "tri_history_read: null history");
    if (const int rc = reader_ready(h, "tri_history_read")) return rc;
    if (bgra8) TRI_HIP_TRY(hipMemcpy(bgra8, h->warped.p, pixels(h) * 4, hipMemcpyDeviceToHost));
    if (mask) TRI_HIP_TRY(hipMemcpy(mask, h->mask.p, pixels(h), hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_history_get_output(tri_history* h, tri_image* colour, tri_image* mask) {
    if (!h) return fail(TRI_E_INVALID, "tri_history_get_output: null history");
    if (!h->has_output) return fail(TRI_E_STATE, "tri_history_get_output: no pass has run (tri_history_reproject)");
    if (colour) fill_image(h, colour, h->warped.p, 4, TRI_FORMAT_B8G8R8A8_UNORM);
    if (mask) fill_image(h, mask, h->mask.p, 1, TRI_FORMAT_R8_UINT);
    return TRI_OK;
}

int tri_history_get_timing(tri_history* h, double* ms, uint64_t* passes) {
    if (!h || !ms || !passes) return fail(TRI_E_INVALID, "tri_history_get_timing: null argument");
    if (!h->has_output) return fail(TRI_E_STATE, "tri_history_get_timing: no pass has run (tri_history_reproject)");
    TRI_HIP_TRY(hipSetDevice(h->device));
    if (const int rc = collect(h, true)) return rc;
    *ms = h->acc_ms;
    *passes = h->acc_passes;
    return TRI_OK;
}

}  // extern "C"
