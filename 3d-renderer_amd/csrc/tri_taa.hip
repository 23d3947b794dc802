// tri_taa.hip — the temporal anti-aliasing entry points of the C-ABI (include/tri_raster.h "temporal anti-aliasing"):
// the jitter, an object of its own that keeps the accumulated colour of one view (16-bit) and the ids it was
// accumulated under, twice, outside any context, the pass that resolves a jittered frame over it (k_taa_resolve,
// taa_pass.hip), the readers, and the presentation blit of the resolved image. The per-pixel rule, the jitter and
// every argument rule are in taa_math.h (plain C++, checked on the CPU by host/tools/taa_check.cpp). Every argument
// check comes before the device is made current.
//
// The bookkeeping, the ordering between passes and blits, the readers' wait and the blit itself are TemporalCore's
// (tri_temporal.h).
#include "taa_math.h"
#include "tri_temporal.h"

struct tri_taa : TemporalCore {
    uint32_t W = 0, H = 0;
    DevBuf<uint2> acc[2];  // four uint16 per pixel, B G R A
    DevBuf<uint32_t> ids[2];
    DevBuf<uint32_t> resolved;
    DevBuf<uint8_t> mask;
    uint32_t written = 0;  // the set the last pass stored into
};

namespace {

constexpr char kPass[] = "tri_taa_resolve";

size_t pixels(const tri_taa* t) { return (size_t)t->W * (size_t)t->H; }

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
    if (!rc) rc = t->init(dev);
    if (rc) {
        delete t;  // (the holders free what was allocated)
        return rc;
    }
    *out = t;
    return TRI_OK;
}

int tri_taa_destroy(tri_taa* t) { return temporal_destroy(t); }

int tri_taa_resolve(tri_taa* t, tri_ctx* c, const tri_taa_params* params) {
    if (!t || !c) return fail(TRI_E_INVALID, "tri_taa_resolve: null argument");
    taa::Msg m;
    if (const int rc = taa::check_params(params, m)) return fail(rc, "tri_taa_resolve: %s", m.text);
    if (const int rc = t->check_source(c, t->W, t->H, kPass, "", "the fetch and the 3 x 3 windows leave the band")) return rc;
    TemporalPass pass;
    if (const int rc = t->begin(c, (params->flags & TRI_TAA_REDO) != 0, &pass)) return rc;
    const uint32_t rd = pass.rd, wr = pass.wr;
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
    a.has_prev = pass.valid ? 1u : 0u;
    a.reject_id = (params->flags & TRI_TAA_REJECT_ID) ? 1u : 0u;
    TRI_HIP_TRY(tri_launch_taa_resolve(a, c->stream));
    return t->end(c, pass, &t->written);
}

int tri_taa_reset(tri_taa* t) {
    if (!t) return fail(TRI_E_INVALID, "tri_taa_reset: null object");
    t->reset();
    return TRI_OK;
}

int tri_taa_read(tri_taa* t, uint8_t* bgra8, uint16_t* rgba16, uint8_t* mask) {
    if (!t) return fail(TRI_E_INVALID, "tri_taa_read: null object");
    if (const int rc = t->reader_ready("tri_taa_read", kPass)) return rc;
    if (bgra8) TRI_HIP_TRY(hipMemcpy(bgra8, t->resolved.p, pixels(t) * 4, hipMemcpyDeviceToHost));
    if (rgba16) TRI_HIP_TRY(hipMemcpy(rgba16, t->acc[t->written].p, pixels(t) * 8, hipMemcpyDeviceToHost));
    if (mask) TRI_HIP_TRY(hipMemcpy(mask, t->mask.p, pixels(t), hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_taa_get_output(tri_taa* t, tri_image* colour8, tri_image* colour16, tri_image* mask) {
    if (!t) return fail(TRI_E_INVALID, "tri_taa_get_output: null object");
    if (!t->has_output) return t->no_pass("tri_taa_get_output", kPass);
    if (colour8) t->fill_image(colour8, t->resolved.p, t->W, t->H, 4, TRI_FORMAT_B8G8R8A8_UNORM);
    if (colour16) t->fill_image(colour16, t->acc[t->written].p, t->W, t->H, 8, TRI_FORMAT_R16G16B16A16_UNORM);
    if (mask) t->fill_image(mask, t->mask.p, t->W, t->H, 1, TRI_FORMAT_R8_UINT);
    return TRI_OK;
}

int tri_taa_get_timing(tri_taa* t, double* ms, uint64_t* passes) {
    if (!t || !ms || !passes) return fail(TRI_E_INVALID, "tri_taa_get_timing: null argument");
    return t->get_timing("tri_taa_get_timing", kPass, ms, passes);
}

int tri_taa_blit_linear(tri_taa* t, tri_ctx* c, void* dst, uint32_t width, uint32_t height) {
    if (!t || !c) return fail(TRI_E_INVALID, "tri_taa_blit_linear: null argument");
    return t->blit_linear("tri_taa_blit_linear", kPass, c, t->W, t->H, "", t->resolved.p, t->W, t->H, dst, width, height);
}

}  // extern "C"
