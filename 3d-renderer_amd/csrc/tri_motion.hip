// tri_motion.hip — the motion-vector entry points of the C-ABI (include/tri_raster.h "motion vectors") over a context:
// the output's switch, the history, the readers, and what tri_render needs for the pass (the reprojection table staged
// like the draws, k_motion's arguments). The kernel is in motion_pass.hip, the table and the argument rules in
// motion_math.h (plain C++, checked on the CPU by host/tools/motion_check.cpp). Every argument check comes before the
// device is made current; tri_motion_matrices touches no device at all.
#include "motion_math.h"
#include "tri_ctx.h"

namespace {

size_t motion_pixels(const tri_ctx* c) { return (size_t)c->W * (size_t)(c->y1 - c->y0); }

int reader_ready(tri_ctx* c, const char* who) {
    if (!c->motion_on) return fail(TRI_E_STATE, "%s: the motion output is off (tri_set_motion_output)", who);
    if (!c->motion_rendered) return fail(TRI_E_STATE, "%s: no frame was rendered with the motion output on", who);
    return tri_synchronize(c);
}

}  // namespace

int tri_motion_release(tri_ctx* c) {
    c->motion_on = false;
    c->motion_rendered = false;
    return c->d_motion.release();
}

int tri_motion_prepare(tri_ctx* c, TriMotionArgs* a, TriMotionPass* pass) {
    const uint32_t ndraws = (uint32_t)c->draws.size();
    // ids count the caller's draws and so does the table: one and the same as long as fsel::resolve_draws keeps a
    // record per caller draw
    if (c->res.ndraws != ndraws) return fail(TRI_E_STATE, "motion: %u resolved draws for %u given", c->res.ndraws, ndraws);
    const tri_motion_history* hist = c->motion_has_history ? &c->motion_history : nullptr;
    if (hist && !motion::count_matches(hist->prev_models != nullptr, hist->draw_count, ndraws))
        return fail(TRI_E_STATE, "tri_render: the motion history holds %u previous models, the frame %u draws", hist->draw_count,
                    ndraws);
    const size_t floats = ((size_t)ndraws + 1) * 16, bytes = floats * 4;
    c->motion_table.resize(floats);
    motion::build_table(c->ubo, c->draws.data(), ndraws, hist, c->motion_table.data());
    Staged& st = c->motion_stage;
    int rc;
    if ((rc = st.acquire(bytes, bytes * 2, true))) return rc;
    std::memcpy(st.h, c->motion_table.data(), bytes);
    TRI_HIP_TRY(hipMemcpyAsync(st.d, st.h, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = st.commit(c->stream))) return rc;
    a->ids = c->d_ids.p;
    a->depth = c->d_depth;
    a->motion = c->d_motion.p;
    a->table = reinterpret_cast<const float*>(st.d.p);
    a->W = (uint32_t)c->W;
    a->npix = (uint32_t)motion_pixels(c);
    a->y0 = (uint32_t)c->y0;
    a->ndraws = ndraws;
    a->sx = 2.0f / (float)c->W;
    a->sy = 2.0f / (float)c->H;
    a->hw = 0.5f * (float)c->W;
    a->hh = 0.5f * (float)c->H;
    // the context's own images come from hipMalloc; a caller's depth target (tri_bind_output) may start anywhere
    *pass = aligned16(a->ids) && aligned16(a->depth) && aligned16(a->motion) ? kMotionVec4 : kMotionScalar;
    return TRI_OK;
}

extern "C" {

int tri_set_motion_output(tri_ctx* c, int enable) {
    if (!c) return fail(TRI_E_INVALID, "tri_set_motion_output: null context");
    if ((enable != 0) == c->motion_on) return TRI_OK;
    if (enable) {
        if (c->cfg.flags & TRI_FLAG_NO_DEPTH_OUTPUT)
            return fail(TRI_E_UNSUPPORTED, "tri_set_motion_output: the context has no depth output (TRI_FLAG_NO_DEPTH_OUTPUT)");
        if (!c->id_on) return fail(TRI_E_STATE, "tri_set_motion_output: the id output is off (tri_set_id_output)");
        if (motion_pixels(c) > 0x7FFFFFFFu) return fail(TRI_E_UNSUPPORTED, "tri_set_motion_output: more than 2^31 pixels");
    }
    int rc = make_current(c);
    if (rc) return rc;
    // queued frames still write the image (off) or must not be overtaken by its allocation's implicit wait (on)
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    if (!enable) return tri_motion_release(c);
    if ((rc = c->d_motion.grow(motion_pixels(c) * 2))) return rc;
    c->motion_rendered = false;
    c->motion_on = true;
    return TRI_OK;
}

int tri_set_motion_history(tri_ctx* c, const tri_motion_history* h) {
    if (!c) return fail(TRI_E_INVALID, "tri_set_motion_history: null context");
    if (!h) {
        c->motion_has_history = false;
        c->motion_prev_models.clear();
        return TRI_OK;
    }
    motion::Msg m;
    if (const int rc = motion::check_history(*h, m)) return fail(rc, "tri_set_motion_history: %s", m.text);
    c->motion_history = *h;
    c->motion_history.reserved = 0;
    c->motion_prev_models.clear();
    if (h->prev_models) {
        c->motion_prev_models.assign(h->prev_models, h->prev_models + (size_t)h->draw_count * 16);
        c->motion_history.prev_models = c->motion_prev_models.data();
    }
    c->motion_has_history = true;
    return TRI_OK;
}

int tri_read_motion(tri_ctx* c, float* xy) {
    if (!c || !xy) return fail(TRI_E_INVALID, "tri_read_motion: null argument");
    if (const int rc = reader_ready(c, "tri_read_motion")) return rc;
    TRI_HIP_TRY(hipMemcpy(xy, c->d_motion, motion_pixels(c) * 8, hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_get_motion_output(tri_ctx* c, tri_image* out) {
    if (!c || !out) return fail(TRI_E_INVALID, "tri_get_motion_output: null argument");
    if (!c->motion_on) return fail(TRI_E_STATE, "tri_get_motion_output: the motion output is off (tri_set_motion_output)");
    out->device_ptr = c->d_motion.p;
    out->width = (uint32_t)c->W;
    out->height = (uint32_t)(c->y1 - c->y0);
    out->pitch_bytes = (uint32_t)c->W * 8u;
    out->format = TRI_FORMAT_R32G32_SFLOAT;
    out->device = c->device;
    out->reserved = 0;
    return TRI_OK;
}

int tri_motion_matrices(const tri_global_ubo* ubo, const tri_draw* draws, uint32_t draw_count, const tri_motion_history* h,
                        float* out) {
    motion::Msg m;
    if (const int rc = motion::check_matrices(ubo, draws, draw_count, h, out, m)) return fail(rc, "tri_motion_matrices: %s", m.text);
    motion::build_table(*ubo, draws, draw_count, h, out);
    return TRI_OK;
}

}  // extern "C"
