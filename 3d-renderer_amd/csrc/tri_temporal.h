// tri_temporal.h — the core of an object that keeps state of one view between frames outside any context: tri_history,
// tri_taa and tri_upscale derive from it and add their planes, their extents and their argument marshalling. It holds
// the two-set bookkeeping, the ordering between passes, the stamped intervals behind get_timing, the readers' wait, the
// checks of the context a pass reads, and the presentation blit of a resolved image. `who` is the entry point's name,
// `pass_name` the object's pass ("tri_taa_resolve"), as the messages print them. Every check that can refuse a call
// comes before the device is made current.
//
// Ordering: a pass runs on the stream of the context it reads, behind that context's tri_render. The object's event
// `done` is recorded behind every pass and every blit, and waited for by the next pass and the next blit, which may run
// on another context's stream (two frames in flight are two contexts); the readers and destroy wait for it on the host.
// A pass's own enqueues lie between begin() and end(): inside the stamped interval and ahead of `done`. The sets are
// committed by end() alone, after every enqueue succeeded, so a call that fails leaves the object as it was. begin()
// collects a finished interval without blocking before it decides whether to stamp: one interval is pending at most.
#pragma once

#include "history_math.h"
#include "tri_ctx.h"

// One pass between begin() and end(): the sets as they will be once it is enqueued.
struct TemporalPass {
    history::Sets next;
    uint32_t rd = 0, wr = 0;  // the set to read, the set to store into
    bool valid = false;       // rd holds a frame
    bool stamp = false;       // the pass is timed
};

struct TemporalCore {
    int device = 0;
    history::Sets sets;
    Event done;               // behind the last pass or blit
    bool has_output = false;  // a pass was enqueued: the images hold (or will hold) a frame
    Event stamp[2];           // round a stamped pass
    bool stamped = false;     // ... whose interval has not been collected yet
    double acc_ms = 0.0;
    uint64_t acc_passes = 0;

    // The tail of create, with the device current.
    int init(int dev) {
        device = dev;
        return done.ensure(hipEventDisableTiming);
    }
    void reset() { sets.reset(); }
    // Add a finished stamped pass to the sums. wait: block for it; otherwise leave it pending when it has not finished.
    int collect(bool wait);
    int no_pass(const char* who, const char* pass_name) const {
        return fail(TRI_E_STATE, "%s: no pass has run (%s)", who, pass_name);
    }
    // A reader: fails before the first pass, else waits on the host for the last one.
    int reader_ready(const char* who, const char* pass_name);
    void fill_image(tri_image* out, void* p, uint32_t width, uint32_t height, uint32_t bytes_per_pixel, uint32_t format) const {
        *out = tri_image{p, width, height, width * bytes_per_pixel, format, device, 0};
    }
    int get_timing(const char* who, const char* pass_name, double* ms, uint64_t* passes);

    // The object, which reads contexts of width x height, against the context (suffix: appended to the message).
    int check_pair(const tri_ctx* c, uint32_t width, uint32_t height, const char* who, const char* suffix = "") const;
    // ... and what a pass needs of that context: every row, and a frame rendered with the motion output on. band_why
    // says what of the pass leaves a row band.
    int check_source(const tri_ctx* c, uint32_t width, uint32_t height, const char* who, const char* suffix,
                     const char* band_why) const;

    // Round a pass's own enqueues on c->stream (see Ordering). end() stores the written set where the object keeps one.
    int begin(tri_ctx* c, bool redo, TemporalPass* p);
    int end(tri_ctx* c, const TemporalPass& p, uint32_t* written);

    // The resolved image (image_w x image_h) scaled into dst (width x height), or into the context's present image where
    // dst is null, as tri_blit_linear; ctx_w x ctx_h as check_pair's.
    int blit_linear(const char* who, const char* pass_name, tri_ctx* c, uint32_t ctx_w, uint32_t ctx_h, const char* suffix,
                    const uint32_t* image, uint32_t image_w, uint32_t image_h, void* dst, uint32_t width, uint32_t height);
};

// destroy: a pass or a blit still queued on a context's stream reads and writes the buffers, so wait for it before they go.
template <typename T>
int temporal_destroy(T* o) {
    if (!o) return TRI_OK;
    (void)hipSetDevice(o->device);
    if (o->has_output) (void)hipEventSynchronize(o->done.e);
    delete o;
    return TRI_OK;
}
