// tri_upscale.hip — the temporal upscaling entry points of the C-ABI (include/tri_raster.h "temporal upscaling"): an
// object of its own that keeps the accumulated colour of one view at the output extent (16-bit) and the ids of the last
// frame at the render extent, twice, outside any context, the pass that resolves a jittered render-extent frame over it
// (k_upscale_resolve, upscale_pass.hip), the readers, and the presentation blit of the resolved image. The per-pixel
// rule, the jitter period and every argument rule are in upscale_math.h (plain C++, checked on the CPU by
// host/tools/upscale_check.cpp). Every argument check comes before the device is made current.
//
// The frame's ids are copied into the written set on the pass's stream behind the kernel, inside the stamped interval
// and ahead of `done`. The bookkeeping, the ordering between passes and blits, the readers' wait and the blit itself are
// TemporalCore's (tri_temporal.h).
#include "upscale_math.h"
#include "tri_temporal.h"

struct tri_upscale : TemporalCore {
    uint32_t Wr = 0, Hr = 0, Wo = 0, Ho = 0;
    DevBuf<uint2> acc[2];      // output extent: four uint16 per pixel, B G R A
    DevBuf<uint32_t> ids[2];   // render extent
    DevBuf<uint32_t> resolved; // output extent
    DevBuf<uint8_t> mask;
    uint32_t written = 0;  // the set the last pass stored into
};

namespace {

constexpr char kPass[] = "tri_upscale_resolve";
constexpr char kRenderExtent[] = " (the render extent)";  // the context's extent is the object's render extent

size_t out_pixels(const tri_upscale* u) { return (size_t)u->Wo * (size_t)u->Ho; }
size_t render_pixels(const tri_upscale* u) { return (size_t)u->Wr * (size_t)u->Hr; }

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
    if (!rc) rc = u->init(dev);
    if (rc) {
        delete u;  // (the holders free what was allocated)
        return rc;
    }
    *out = u;
    return TRI_OK;
}

int tri_upscale_destroy(tri_upscale* u) { return temporal_destroy(u); }

int tri_upscale_resolve(tri_upscale* u, tri_ctx* c, const tri_upscale_params* params) {
    if (!u || !c) return fail(TRI_E_INVALID, "tri_upscale_resolve: null argument");
    upscale::Msg m;
    if (const int rc = upscale::check_params(params, m)) return fail(rc, "tri_upscale_resolve: %s", m.text);
    if (const int rc = u->check_source(c, u->Wr, u->Hr, kPass, kRenderExtent, "the samples and the 3 x 3 windows leave the band"))
        return rc;
    TemporalPass pass;
    if (const int rc = u->begin(c, (params->flags & TRI_UPSCALE_REDO) != 0, &pass)) return rc;
    const uint32_t rd = pass.rd, wr = pass.wr;
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
    a.has_prev = pass.valid ? 1u : 0u;
    a.reject_id = (params->flags & TRI_UPSCALE_REJECT_ID) ? 1u : 0u;
    TRI_HIP_TRY(tri_launch_upscale_resolve(a, c->stream));
    // I = the frame's ids, for every render pixel: a copy on the same stream, ahead of end()
    TRI_HIP_TRY(hipMemcpyAsync(u->ids[wr].p, c->d_ids.p, render_pixels(u) * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    return u->end(c, pass, &u->written);
}

int tri_upscale_reset(tri_upscale* u) {
    if (!u) return fail(TRI_E_INVALID, "tri_upscale_reset: null object");
    u->reset();
    return TRI_OK;
}

int tri_upscale_read(tri_upscale* u, uint8_t* bgra8, uint16_t* rgba16, uint8_t* mask) {
    if (!u) return fail(TRI_E_INVALID, "tri_upscale_read: null object");
    if (const int rc = u->reader_ready("tri_upscale_read", kPass)) return rc;
    if (bgra8) TRI_HIP_TRY(hipMemcpy(bgra8, u->resolved.p, out_pixels(u) * 4, hipMemcpyDeviceToHost));
    if (rgba16) TRI_HIP_TRY(hipMemcpy(rgba16, u->acc[u->written].p, out_pixels(u) * 8, hipMemcpyDeviceToHost));
    if (mask) TRI_HIP_TRY(hipMemcpy(mask, u->mask.p, out_pixels(u), hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_upscale_read_ids(tri_upscale* u, uint32_t* ids) {
    if (!u) return fail(TRI_E_INVALID, "tri_upscale_read_ids: null object");
    if (const int rc = u->reader_ready("tri_upscale_read_ids", kPass)) return rc;
    if (ids) TRI_HIP_TRY(hipMemcpy(ids, u->ids[u->written].p, render_pixels(u) * 4, hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_upscale_get_output(tri_upscale* u, tri_image* colour8, tri_image* colour16, tri_image* mask) {
    if (!u) return fail(TRI_E_INVALID, "tri_upscale_get_output: null object");
    if (!u->has_output) return u->no_pass("tri_upscale_get_output", kPass);
    if (colour8) u->fill_image(colour8, u->resolved.p, u->Wo, u->Ho, 4, TRI_FORMAT_B8G8R8A8_UNORM);
    if (colour16) u->fill_image(colour16, u->acc[u->written].p, u->Wo, u->Ho, 8, TRI_FORMAT_R16G16B16A16_UNORM);
    if (mask) u->fill_image(mask, u->mask.p, u->Wo, u->Ho, 1, TRI_FORMAT_R8_UINT);
    return TRI_OK;
}

int tri_upscale_get_timing(tri_upscale* u, double* ms, uint64_t* passes) {
    if (!u || !ms || !passes) return fail(TRI_E_INVALID, "tri_upscale_get_timing: null argument");
    return u->get_timing("tri_upscale_get_timing", kPass, ms, passes);
}

int tri_upscale_blit_linear(tri_upscale* u, tri_ctx* c, void* dst, uint32_t width, uint32_t height) {
    if (!u || !c) return fail(TRI_E_INVALID, "tri_upscale_blit_linear: null argument");
    return u->blit_linear("tri_upscale_blit_linear", kPass, c, u->Wr, u->Hr, kRenderExtent, u->resolved.p, u->Wo, u->Ho, dst, width,
                          height);
}

}  // extern "C"
