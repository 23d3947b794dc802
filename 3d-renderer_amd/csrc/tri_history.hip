// tri_history.hip — the history reprojection entry points of the C-ABI (include/tri_raster.h "history reprojection"):
// an object of its own that keeps the previous frame of one view — colour, ids, depth, twice — outside any context, the
// pass that warps it by the frame's motion (k_reproject, history_pass.hip), and the readers. The per-pixel rule and
// every argument rule are in history_math.h (plain C++, checked on the CPU by host/tools/history_check.cpp). Every
// argument check comes before the device is made current.
//
// The bookkeeping, the ordering between passes and the readers' wait are TemporalCore's (tri_temporal.h).
#include "history_math.h"
#include "tri_temporal.h"

struct tri_history : TemporalCore {
    uint32_t W = 0, H = 0;
    DevBuf<uint32_t> colour[2], ids[2];
    DevBuf<float> depth[2];
    DevBuf<uint32_t> warped;
    DevBuf<uint8_t> mask;
};

namespace {

constexpr char kPass[] = "tri_history_reproject";

size_t pixels(const tri_history* h) { return (size_t)h->W * (size_t)h->H; }

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
    if (!rc) rc = h->init(dev);
    if (rc) {
        delete h;  // (the holders free what was allocated)
        return rc;
    }
    *out = h;
    return TRI_OK;
}

int tri_history_destroy(tri_history* h) { return temporal_destroy(h); }

int tri_history_reproject(tri_history* h, tri_ctx* c, const tri_reproject_params* params) {
    if (!h || !c) return fail(TRI_E_INVALID, "tri_history_reproject: null argument");
    history::Msg m;
    if (const int rc = history::check_params(params, m)) return fail(rc, "tri_history_reproject: %s", m.text);
    if (const int rc = h->check_source(c, h->W, h->H, kPass, "", "the fetch leaves the band")) return rc;
    TemporalPass pass;
    if (const int rc = h->begin(c, (params->flags & TRI_HISTORY_REDO) != 0, &pass)) return rc;
    const uint32_t rd = pass.rd, wr = pass.wr;
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
    a.has_prev = pass.valid ? 1u : 0u;
    // the object's images and the context's own come from hipMalloc; a caller's targets (tri_bind_output) may start anywhere
    const bool vec4 = aligned16(a.colour) && aligned16(a.ids) && aligned16(a.depth);
    TRI_HIP_TRY(tri_launch_reproject(a, vec4, c->stream));
    return h->end(c, pass, nullptr);
}

int tri_history_reset(tri_history* h) {
    if (!h) return fail(TRI_E_INVALID, "tri_history_reset: null history");
    h->reset();
    return TRI_OK;
}

int tri_history_read(tri_history* h, uint8_t* bgra8, uint8_t* mask) {
    if (!h) return fail(TRI_E_INVALID, "tri_history_read: null history");
    if (const int rc = h->reader_ready("tri_history_read", kPass)) return rc;
    if (bgra8) TRI_HIP_TRY(hipMemcpy(bgra8, h->warped.p, pixels(h) * 4, hipMemcpyDeviceToHost));
    if (mask) TRI_HIP_TRY(hipMemcpy(mask, h->mask.p, pixels(h), hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_history_get_output(tri_history* h, tri_image* colour, tri_image* mask) {
    if (!h) return fail(TRI_E_INVALID, "tri_history_get_output: null history");
    if (!h->has_output) return h->no_pass("tri_history_get_output", kPass);
    if (colour) h->fill_image(colour, h->warped.p, h->W, h->H, 4, TRI_FORMAT_B8G8R8A8_UNORM);
    if (mask) h->fill_image(mask, h->mask.p, h->W, h->H, 1, TRI_FORMAT_R8_UINT);
    return TRI_OK;
}

int tri_history_get_timing(tri_history* h, double* ms, uint64_t* passes) {
    if (!h || !ms || !passes) return fail(TRI_E_INVALID, "tri_history_get_timing: null argument");
    return h->get_timing("tri_history_get_timing", kPass, ms, passes);
}

}  // extern "C"
