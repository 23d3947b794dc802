// tri_temporal.hip — TemporalCore's operations that are better not inline (tri_temporal.h says what they promise).
#include "tri_temporal.h"

int TemporalCore::collect(bool wait) {
    if (!stamped) return TRI_OK;
    if (wait) TRI_HIP_TRY(hipEventSynchronize(stamp[1].e));
    else {
        const hipError_t q = hipEventQuery(stamp[1].e);
        if (q == hipErrorNotReady) return TRI_OK;
        TRI_HIP_TRY(q);
    }
    float ms = 0.0f;
    TRI_HIP_TRY(hipEventElapsedTime(&ms, stamp[0].e, stamp[1].e));
    acc_ms += ms;
    acc_passes += 1;
    stamped = false;
    return TRI_OK;
}

int TemporalCore::reader_ready(const char* who, const char* pass_name) {
    if (!has_output) return no_pass(who, pass_name);
    TRI_HIP_TRY(hipSetDevice(device));
    TRI_HIP_TRY(hipEventSynchronize(done.e));
    return TRI_OK;
}

int TemporalCore::get_timing(const char* who, const char* pass_name, double* ms, uint64_t* passes) {
    if (!has_output) return no_pass(who, pass_name);
    TRI_HIP_TRY(hipSetDevice(device));
    if (const int rc = collect(true)) return rc;
    *ms = acc_ms;
    *passes = acc_passes;
    return TRI_OK;
}

int TemporalCore::check_pair(const tri_ctx* c, uint32_t width, uint32_t height, const char* who, const char* suffix) const {
    history::Msg m;
    if (const int rc = history::check_context(device, width, height, c->device, (uint32_t)c->W, (uint32_t)c->H, m))
        return fail(rc, "%s: %s%s", who, m.text, suffix);
    return TRI_OK;
}

int TemporalCore::check_source(const tri_ctx* c, uint32_t width, uint32_t height, const char* who, const char* suffix,
                               const char* band_why) const {
    if (const int rc = check_pair(c, width, height, who, suffix)) return rc;
    if (c->y0 != 0 || c->y1 != c->H) return fail(TRI_E_UNSUPPORTED, "%s: a row-band context (%s)", who, band_why);
    if (!c->motion_on) return fail(TRI_E_STATE, "%s: the context's motion output is off (tri_set_motion_output)", who);
    if (!c->motion_rendered || c->motion_table.size() < 16 || !c->motion_stage.d.p)
        return fail(TRI_E_STATE, "%s: no frame was rendered with the motion output on", who);
    return TRI_OK;
}

int TemporalCore::begin(tri_ctx* c, bool redo, TemporalPass* p) {
    int rc = make_current(c);
    if (rc) return rc;
    if ((rc = collect(false))) return rc;
    p->stamp = c->timing && !stamped;
    if (p->stamp)
        for (int i = 0; i < 2; ++i)
            if ((rc = stamp[i].ensure(hipEventDefault))) return rc;
    // the object's previous pass (or a blit of its image) may have run on another context's stream
    if (has_output) TRI_HIP_TRY(hipStreamWaitEvent(c->stream, done.e, 0));
    p->next = sets;  // committed by end()
    p->rd = p->next.begin(redo, &p->valid);
    p->wr = p->rd ^ 1u;
    if (p->stamp) TRI_HIP_TRY(hipEventRecord(stamp[0].e, c->stream));
    return TRI_OK;
}

int TemporalCore::end(tri_ctx* c, const TemporalPass& p, uint32_t* written) {
    if (p.stamp) {
        TRI_HIP_TRY(hipEventRecord(stamp[1].e, c->stream));
        stamped = true;
    }
    TRI_HIP_TRY(hipEventRecord(done.e, c->stream));
    sets = p.next;
    if (written) *written = p.wr;
    has_output = true;
    return TRI_OK;
}

int TemporalCore::blit_linear(const char* who, const char* pass_name, tri_ctx* c, uint32_t ctx_w, uint32_t ctx_h,
                              const char* suffix, const uint32_t* image, uint32_t image_w, uint32_t image_h, void* dst,
                              uint32_t width, uint32_t height) {
    if (const int rc = tri_check_extent(who, width, height, "destination")) return rc;
    if (const int rc = check_pair(c, ctx_w, ctx_h, who, suffix)) return rc;
    if (c->y0 != 0 || c->y1 != c->H) return fail(TRI_E_STATE, "%s: a row-band context has no whole frame", who);
    if (!has_output) return no_pass(who, pass_name);
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
    TRI_HIP_TRY(hipStreamWaitEvent(c->stream, done.e, 0));  // the pass may have run on another context's stream
    TRI_HIP_TRY(tri_launch_blit(image, (int32_t)image_w, (int32_t)image_h, out, (int32_t)width, (int32_t)height, c->d_lut + 256,
                                c->stream));
    TRI_HIP_TRY(hipEventRecord(done.e, c->stream));  // the next pass overwrites the image this blit reads
    return TRI_OK;
}
