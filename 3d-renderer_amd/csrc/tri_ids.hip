// tri_ids.hip — the entity-id entry points of the C-ABI (include/tri_raster.h "entity ids") over a context: the id
// output's switch, its readers (the whole image, one pixel, the distinct draws of a rectangle), the outline's state and
// tri_render's outline pass. The kernels are in id_pass.hip, the argument rules in id_select.h (plain C++, checked on
// the CPU by host/tools/id_check.cpp). Every argument check comes before the device is made current.
#include "id_select.h"
#include "tri_ctx.h"

namespace {

size_t id_pixels(const tri_ctx* c) { return (size_t)c->W * (size_t)(c->y1 - c->y0); }

// What every reader needs: the output on and a frame rendered with it, then that frame complete (TRI_E_OVERFLOW as
// tri_readback reports it: the frame's ids are as invalid as its colour).
int reader_ready(tri_ctx* c, const char* who) {
    if (!c->id_on) return fail(TRI_E_STATE, "%s: the id output is off (tri_set_id_output)", who);
    if (!c->ids_rendered) return fail(TRI_E_STATE, "%s: no frame was rendered with the id output on", who);
    return tri_synchronize(c);
}

}  // namespace

int tri_ids_outline_pass(tri_ctx* c) {
    const uint32_t ndraws = c->res.ndraws;
    // tri_set_outline checked the indices against the caller's draw list and the ids count that list, while the flags
    // are per resolved draw: one and the same as long as fsel::resolve_draws keeps a record per caller draw
    if (ndraws != c->draws.size()) return fail(TRI_E_STATE, "outline: %u resolved draws for %zu given", ndraws, c->draws.size());
    if (c->outline_draws.empty() || !ndraws) return TRI_OK;
    if (c->sel_dirty || c->sel_ndraws != ndraws) {  // the flags follow the outline and the draw count
        std::vector<uint32_t> flags;
        idsel::selection_flags(c->outline_draws.data(), (uint32_t)c->outline_draws.size(), ndraws, flags);
        const size_t bytes = flags.size() * 4;
        Staged& st = c->sel_stage;
        int rc;
        if ((rc = st.acquire(bytes, bytes * 2, true))) return rc;
        std::memcpy(st.h, flags.data(), bytes);
        TRI_HIP_TRY(hipMemcpyAsync(st.d, st.h, bytes, hipMemcpyHostToDevice, c->stream));
        if ((rc = st.commit(c->stream))) return rc;
        c->sel_dirty = false;
        c->sel_ndraws = ndraws;
    }
    TRI_HIP_TRY(tri_launch_id_outline(c->d_ids, reinterpret_cast<const uint32_t*>(c->sel_stage.d.p), ndraws, c->d_color, c->W,
                                  c->y1 - c->y0, (int32_t)c->outline_width, c->outline_rgba, c->stream));
    return TRI_OK;
}

extern "C" {

int tri_set_id_output(tri_ctx* c, int enable) {
    if (!c) return fail(TRI_E_INVALID, "tri_set_id_output: null context");
    if ((enable != 0) == c->id_on) return TRI_OK;
    int rc = make_current(c);
    if (rc) return rc;
    // queued frames still write the image (off) or must not be overtaken by its allocation's implicit wait (on)
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    c->ids_rendered = false;
    if (enable) {
        if ((rc = c->d_ids.grow(id_pixels(c)))) return rc;
        c->id_on = true;
        return TRI_OK;
    }
    c->id_on = false;
    c->outline_on = false;
    c->outline_draws.clear();
    if ((rc = tri_motion_release(c))) return rc;  // the motion pass reads the ids
    return c->d_ids.release();
}

int tri_read_ids(tri_ctx* c, uint32_t* ids) {
    if (!c || !ids) return fail(TRI_E_INVALID, "tri_read_ids: null argument");
    if (const int rc = reader_ready(c, "tri_read_ids")) return rc;
    TRI_HIP_TRY(hipMemcpy(ids, c->d_ids, id_pixels(c) * 4, hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_get_id_output(tri_ctx* c, tri_image* out) {
    if (!c || !out) return fail(TRI_E_INVALID, "tri_get_id_output: null argument");
    if (!c->id_on) return fail(TRI_E_STATE, "tri_get_id_output: the id output is off (tri_set_id_output)");
    out->device_ptr = c->d_ids.p;
    out->width = (uint32_t)c->W;
    out->height = (uint32_t)(c->y1 - c->y0);
    out->pitch_bytes = (uint32_t)c->W * 4u;
    out->format = TRI_FORMAT_R32_UINT;
    out->device = c->device;
    out->reserved = 0;
    return TRI_OK;
}

int tri_pick(tri_ctx* c, int32_t x, int32_t y, tri_pick_result* out) {
    if (!c || !out) return fail(TRI_E_INVALID, "tri_pick: null argument");
    if (!c->id_on) return fail(TRI_E_STATE, "tri_pick: the id output is off (tri_set_id_output)");
    idsel::Msg m;
    if (const int rc = idsel::check_pick(c->W, c->y0, c->y1, x, y, m)) return fail(rc, "tri_pick: %s", m.text);
    if (const int rc = reader_ready(c, "tri_pick")) return rc;
    const size_t o = (size_t)(y - c->y0) * (size_t)c->W + (size_t)x;
    *out = tri_pick_result{0u, 0u, 0u, 0u};
    TRI_HIP_TRY(hipMemcpy(&out->id, c->d_ids.p + o, 4, hipMemcpyDeviceToHost));
    if (!(c->cfg.flags & TRI_FLAG_NO_DEPTH_OUTPUT)) {
        TRI_HIP_TRY(hipMemcpy(&out->depth_bits, c->d_depth + o, 4, hipMemcpyDeviceToHost));
        out->has_depth = 1u;
    }
    return TRI_OK;
}

int tri_pick_rect(tri_ctx* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint32_t* draw_bits, uint32_t word_count,
                  uint32_t* distinct) {
    if (!c) return fail(TRI_E_INVALID, "tri_pick_rect: null context");
    if (!c->id_on) return fail(TRI_E_STATE, "tri_pick_rect: the id output is off (tri_set_id_output)");
    if (!c->ids_rendered) return fail(TRI_E_STATE, "tri_pick_rect: no frame was rendered with the id output on");
    idsel::Rect r{x0, y0, x1, y1};
    idsel::Msg m;
    bool empty = false;
    const uint32_t ndraws = c->res.ndraws, need = idsel::bitmap_words(ndraws);
    if (const int rc = idsel::check_rect(c->W, c->y0, c->y1, r, ndraws, word_count, draw_bits != nullptr, &empty, m))
        return fail(rc, "tri_pick_rect: %s", m.text);
    int rc = reader_ready(c, "tri_pick_rect");
    if (rc) return rc;
    for (uint32_t i = 0; draw_bits && i < word_count; ++i) draw_bits[i] = 0u;
    if (distinct) *distinct = 0u;
    if (empty || !need) return TRI_OK;
    if ((rc = c->d_pick_bits.grow(need))) return rc;
    if ((rc = c->h_pick.grow(need))) return rc;
    TRI_HIP_TRY(hipMemsetAsync(c->d_pick_bits, 0, (size_t)need * 4, c->stream));
    TRI_HIP_TRY(tri_launch_id_collect(c->d_ids, c->W, r.x0, r.y0 - c->y0, r.x1 - r.x0 + 1, r.y1 - r.y0 + 1, c->d_pick_bits, need,
                                  c->stream));
    TRI_HIP_TRY(hipMemcpyAsync(c->h_pick, c->d_pick_bits, (size_t)need * 4, hipMemcpyDeviceToHost, c->stream));
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t count = 0;
    for (uint32_t i = 0; i < need; ++i) {
        // (bits past the draw count cannot be set: every id is a draw's index + 1)
        draw_bits[i] = c->h_pick.p[i];
        count += (uint32_t)__builtin_popcount(draw_bits[i]);
    }
    if (distinct) *distinct = count;
    return TRI_OK;
}

int tri_set_outline(tri_ctx* c, const tri_outline* o) {
    if (!c) return fail(TRI_E_INVALID, "tri_set_outline: null context");
    if (!o) {
        c->outline_on = false;
        c->outline_draws.clear();
        return TRI_OK;
    }
    idsel::Msg m;
    if (const int rc = idsel::check_outline(*o, (uint32_t)c->draws.size(), m)) return fail(rc, "tri_set_outline: %s", m.text);
    if (!tri_internal_whole_frame(c))
        return fail(TRI_E_UNSUPPORTED, "tri_set_outline: a row-band context cannot outline (the halo lies in other bands)");
    if (!c->id_on) return fail(TRI_E_STATE, "tri_set_outline: the id output is off (tri_set_id_output)");
    c->outline_draws.clear();
    if (o->draw_count) c->outline_draws.assign(o->draws, o->draws + o->draw_count);
    for (int k = 0; k < 4; ++k) c->outline_rgba[k] = o->rgba[k];
    c->outline_width = o->width_px;
    c->outline_on = true;
    c->sel_dirty = true;
    return TRI_OK;
}

}  // extern "C"
