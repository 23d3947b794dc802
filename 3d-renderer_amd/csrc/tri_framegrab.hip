// tri_framegrab.hip — the frame-tensor entry points of the C-ABI (include/tri_raster.h): tri_convert_rgba_f32 and
// tri_framegrab, the tensor counterpart of tri_recorder (tri_record.hip).
//
// A grab turns frames into the reference's AI input tensor (channels-last RGBA float32, Renderer.cpp:1111-1389)
// without stalling the renderer: tri_framegrab_capture enqueues the conversion behind the frame on the context's
// stream; the tensor stays on the device for a consumer there, and with TRI_GRAB_HOST_COPY it is also copied to pinned
// memory on the grab's own stream. Slot protocol: idle -> capture -> busy -> wait (any number of times) -> release
// -> idle.
#include "raster_launch.h"

#include <hip/hip_runtime.h>

#include <string>

namespace {

constexpr uint32_t kMaxSlots = 8;

int hip_fail(hipError_t e, const char* what) {
    const std::string m = std::string(what) + ": " + hipGetErrorString(e);
    return tri_internal_fail(e == hipErrorOutOfMemory ? TRI_E_OOM : TRI_E_HIP, m.c_str());
}

#define GH(expr)                                          \
    do {                                                  \
        const hipError_t _e = (expr);                     \
        if (_e != hipSuccess) return hip_fail(_e, #expr); \
    } while (0)

}  // namespace

struct tri_framegrab {
    int device = 0;
    uint32_t width = 0, height = 0, slots = 0;
    bool host_copy = false;
    size_t bytes = 0;                      // 16 * width * height
    hipStream_t copy = nullptr;            // the device-to-host copies (only with host_copy; never the render stream)
    float* d_f32[kMaxSlots] = {};          // the conversion's output: what a consumer on the device reads
    float* h_f32[kMaxSlots] = {};          // pinned (only with host_copy)
    hipEvent_t converted[kMaxSlots] = {};  // recorded on the context's stream behind the conversion
    hipEvent_t copied[kMaxSlots] = {};     // recorded on the copy stream behind the copy (only with host_copy)
    bool busy[kMaxSlots] = {};
};

extern "C" {

int tri_convert_rgba_f32(const void* bgra, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* f32, void* stream) {
    if (!bgra || !f32) return tri_internal_fail(TRI_E_INVALID, "tri_convert_rgba_f32: null pointer");
    if (width == 0 || height == 0 || width > TRI_MAX_DIM || height > TRI_MAX_DIM)
        return tri_internal_fail(TRI_E_INVALID, "tri_convert_rgba_f32: extent outside 1..TRI_MAX_DIM");
    if (pitch_bytes < width * 4u || (pitch_bytes & 3u))
        return tri_internal_fail(TRI_E_INVALID, "tri_convert_rgba_f32: pitch below width * 4 or not a multiple of 4");
    if ((uintptr_t)bgra & 3u) return tri_internal_fail(TRI_E_INVALID, "tri_convert_rgba_f32: source must be 4-B aligned");
    if ((uintptr_t)f32 & 3u) return tri_internal_fail(TRI_E_INVALID, "tri_convert_rgba_f32: output must be 4-B aligned");
    const hipError_t e = tri_launch_bgra_to_rgba_f32(bgra, width, height, pitch_bytes, static_cast<float*>(f32),
                                                     static_cast<hipStream_t>(stream));
    return e == hipSuccess ? TRI_OK : tri_internal_fail(TRI_E_HIP, hipGetErrorString(e));
}

int tri_framegrab_destroy(tri_framegrab* g) {
    if (!g) return TRI_OK;
    (void)hipSetDevice(g->device);
    if (g->copy) (void)hipStreamSynchronize(g->copy);
    for (uint32_t s = 0; s < kMaxSlots; ++s) {
        // (a conversion still queued on a context's stream writes d_f32: wait for it before the buffer goes)
        if (g->busy[s] && g->converted[s]) (void)hipEventSynchronize(g->converted[s]);
        if (g->d_f32[s]) (void)hipFree(g->d_f32[s]);
        if (g->h_f32[s]) (void)hipHostFree(g->h_f32[s]);
        if (g->converted[s]) (void)hipEventDestroy(g->converted[s]);
        if (g->copied[s]) (void)hipEventDestroy(g->copied[s]);
    }
    if (g->copy) (void)hipStreamDestroy(g->copy);
    delete g;
    return TRI_OK;
}

int tri_framegrab_create(int32_t device, uint32_t width, uint32_t height, uint32_t slots, uint32_t flags, tri_framegrab** out) {
    if (!out) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_create: null argument");
    *out = nullptr;
    if (width == 0 || height == 0 || width > TRI_MAX_DIM || height > TRI_MAX_DIM)
        return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_create: extent outside 1..TRI_MAX_DIM");
    if (slots == 0 || slots > kMaxSlots) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_create: slots outside 1..8");
    if (flags & ~(uint32_t)TRI_GRAB_HOST_COPY) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_create: unknown flag");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return tri_internal_fail(TRI_E_HIP, "tri_framegrab_create: no HIP device available");
    int dev = device;
    if (device < 0) {
        if (hipGetDevice(&dev) != hipSuccess) return tri_internal_fail(TRI_E_HIP, "tri_framegrab_create: hipGetDevice failed");
    } else if (device >= ndev) {
        return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_create: device ordinal out of range");
    }
    tri_framegrab* g = new tri_framegrab();
    g->device = dev;
    g->width = width;
    g->height = height;
    g->slots = slots;
    g->host_copy = (flags & TRI_GRAB_HOST_COPY) != 0;
    g->bytes = (size_t)16 * width * height;
    auto bail = [&](int rc) { tri_framegrab_destroy(g); return rc; };
    if (hipSetDevice(dev) != hipSuccess) return bail(tri_internal_fail(TRI_E_HIP, "tri_framegrab_create: hipSetDevice failed"));
    if (g->host_copy && hipStreamCreateWithFlags(&g->copy, hipStreamNonBlocking) != hipSuccess)
        return bail(tri_internal_fail(TRI_E_HIP, "tri_framegrab_create: stream creation failed"));
    for (uint32_t s = 0; s < slots; ++s) {
        if (hipMalloc(reinterpret_cast<void**>(&g->d_f32[s]), g->bytes) != hipSuccess)
            return bail(tri_internal_fail(TRI_E_OOM, "tri_framegrab_create: buffer allocation failed"));
        if (hipEventCreateWithFlags(&g->converted[s], hipEventDisableTiming) != hipSuccess)
            return bail(tri_internal_fail(TRI_E_HIP, "tri_framegrab_create: event creation failed"));
        if (!g->host_copy) continue;
        if (hipHostMalloc(reinterpret_cast<void**>(&g->h_f32[s]), g->bytes, hipHostMallocDefault) != hipSuccess)
            return bail(tri_internal_fail(TRI_E_OOM, "tri_framegrab_create: pinned allocation failed"));
        if (hipEventCreateWithFlags(&g->copied[s], hipEventDisableTiming) != hipSuccess)
            return bail(tri_internal_fail(TRI_E_HIP, "tri_framegrab_create: event creation failed"));
    }
    *out = g;
    return TRI_OK;
}

int tri_framegrab_capture(tri_framegrab* g, uint32_t slot, tri_ctx* ctx) {
    if (!g || !ctx) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_capture: null argument");
    if (slot >= g->slots) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_capture: slot out of range");
    if (!tri_internal_whole_frame(ctx))
        return tri_internal_fail(TRI_E_STATE, "tri_framegrab_capture: a row-band context has no whole frame");
    tri_image img;
    const int rc = tri_get_output(ctx, &img);
    if (rc) return rc;
    if (img.device != g->device) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_capture: the context is on another device");
    if (img.width != g->width || img.height != g->height)
        return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_capture: the context's extent differs from the grab's");
    if (g->busy[slot]) return tri_internal_fail(TRI_E_STATE, "tri_framegrab_capture: the slot is busy (wait for it and release it)");
    GH(hipSetDevice(g->device));
    hipStream_t s = tri_internal_stream(ctx);
    GH(tri_launch_bgra_to_rgba_f32(img.device_ptr, img.width, img.height, img.pitch_bytes, g->d_f32[slot], s));
    hipError_t e = hipEventRecord(g->converted[slot], s);
    if (g->host_copy) {
        if (e == hipSuccess) e = hipStreamWaitEvent(g->copy, g->converted[slot], 0);
        if (e == hipSuccess) e = hipMemcpyAsync(g->h_f32[slot], g->d_f32[slot], g->bytes, hipMemcpyDeviceToHost, g->copy);
        if (e == hipSuccess) e = hipEventRecord(g->copied[slot], g->copy);
    }
    if (e != hipSuccess) {  // the slot stays idle: nothing of this capture may still be running on its buffers
        (void)hipStreamSynchronize(s);
        if (g->copy) (void)hipStreamSynchronize(g->copy);
        return hip_fail(e, "tri_framegrab_capture");
    }
    g->busy[slot] = true;
    return TRI_OK;
}

int tri_framegrab_wait(tri_framegrab* g, uint32_t slot, const float** host, const float** device) {
    if (!g || (!host && !device)) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_wait: null argument");
    if (slot >= g->slots) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_wait: slot out of range");
    if (host && !g->host_copy)
        return tri_internal_fail(TRI_E_STATE, "tri_framegrab_wait: the grab was created without TRI_GRAB_HOST_COPY");
    if (!g->busy[slot]) return tri_internal_fail(TRI_E_STATE, "tri_framegrab_wait: the slot is idle (nothing was captured)");
    GH(hipSetDevice(g->device));
    if (device) {
        GH(hipEventSynchronize(g->converted[slot]));
        *device = g->d_f32[slot];
    }
    if (host) {
        GH(hipEventSynchronize(g->copied[slot]));
        *host = g->h_f32[slot];
    }
    return TRI_OK;
}

int tri_framegrab_release(tri_framegrab* g, uint32_t slot) {
    if (!g) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_release: null grab");
    if (slot >= g->slots) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_release: slot out of range");
    if (!g->busy[slot]) return TRI_OK;
    // a capture still in flight finishes first, so the slot's next capture cannot race this one's conversion or copy
    GH(hipSetDevice(g->device));
    GH(hipEventSynchronize(g->converted[slot]));
    if (g->host_copy) GH(hipEventSynchronize(g->copied[slot]));
    g->busy[slot] = false;
    return TRI_OK;
}

}  // extern "C"
