// tri_capture.hip — the capture entry points of the C-ABI (include/tri_raster.h): tri_convert_yuv444 with tri_recorder
// (the Y4M payload: planar YUV 4:4:4, VideoEncoder.cpp:370-412, :716-736) and tri_convert_rgba_f32 with tri_framegrab
// (the AI input tensor: channels-last RGBA float32, Renderer.cpp:1111-1389).
//
// Both products are one ring of slots around a conversion kernel (record_yuv.hip, frame_tensor.hip). A capture turns a
// frame into its product without stalling the renderer: the conversion is enqueued behind the frame on the context's
// stream, into the slot's device buffer; with host_copy the ring's own stream then copies it to pinned memory, and the
// caller collects it a few frames later while the next frames render. The recorder always copies; a grab copies with
// TRI_GRAB_HOST_COPY and otherwise leaves the tensor to a consumer on the device. Slot protocol: idle -> capture ->
// busy -> wait (any number of times) -> release -> idle.
#include "capi_util.h"
#include "raster_launch.h"

#include <hip/hip_runtime.h>

#include <cstdio>

namespace {

constexpr uint32_t kMaxSlots = 8;

// The conversion of one product: src width x height B8G8R8A8 at pitch_bytes -> dst, on `stream`.
using ConvertFn = hipError_t (*)(const void* src, uint32_t w, uint32_t h, uint32_t pitch, void* dst, hipStream_t stream);

hipError_t convert_yuv444(const void* src, uint32_t w, uint32_t h, uint32_t pitch, void* dst, hipStream_t s) {
    return tri_launch_bgra_to_yuv444(src, w, h, pitch, static_cast<uint8_t*>(dst), s);
}
hipError_t convert_rgba_f32(const void* src, uint32_t w, uint32_t h, uint32_t pitch, void* dst, hipStream_t s) {
    return tri_launch_bgra_to_rgba_f32(src, w, h, pitch, static_cast<float*>(dst), s);
}

// Record "<who>: <a><b><c>"; returns `code`.
int ring_fail(int code, const char* who, const char* a, const char* b = "", const char* c = "") {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s%s%s", who, a, b, c);
    return tri_internal_fail(code, msg);
}

// The operations take the entry point's name (`who`) and, where a message names the object, its noun ("recorder", "grab").
struct CaptureRing {
    int device = 0;
    uint32_t width = 0, height = 0, slots = 0;
    bool host_copy = false;
    size_t bytes = 0;                      // bytes per pixel * width * height
    hipStream_t copy = nullptr;            // the device-to-host copies (only with host_copy; never the render stream)
    void* d_out[kMaxSlots] = {};           // the conversion's output: what a consumer on the device reads
    void* h_out[kMaxSlots] = {};           // pinned (only with host_copy)
    hipEvent_t converted[kMaxSlots] = {};  // recorded on the context's stream behind the conversion
    hipEvent_t copied[kMaxSlots] = {};     // recorded on the copy stream behind the copy (only with host_copy)
    bool busy[kMaxSlots] = {};

    // The argument checks of a create, before any HIP call: extent, then slots (the grab's flags follow in its wrapper).
    static int check(const char* who, uint32_t width, uint32_t height, uint32_t slots) {
        if (const int rc = tri_check_extent(who, width, height)) return rc;
        if (slots == 0 || slots > kMaxSlots) return ring_fail(TRI_E_INVALID, who, "slots outside 1..8");
        return TRI_OK;
    }

    // After check(). `dev` as in tri_resolve_device; on an error nothing of the ring is left.
    int create(const char* who, int32_t dev, uint32_t w, uint32_t h, uint32_t nslots, uint32_t bytes_per_pixel, bool with_host_copy) {
        if (const int rc = tri_resolve_device(dev, who, &device)) return rc;
        const int rc = build(who, w, h, nslots, bytes_per_pixel, with_host_copy);
        if (rc) destroy();
        return rc;
    }

    int build(const char* who, uint32_t w, uint32_t h, uint32_t nslots, uint32_t bytes_per_pixel, bool with_host_copy) {
        width = w;
        height = h;
        slots = nslots;
        host_copy = with_host_copy;
        bytes = (size_t)bytes_per_pixel * w * h;
        if (hipSetDevice(device) != hipSuccess) return ring_fail(TRI_E_HIP, who, "hipSetDevice failed");
        if (host_copy && hipStreamCreateWithFlags(&copy, hipStreamNonBlocking) != hipSuccess)
            return ring_fail(TRI_E_HIP, who, "stream creation failed");
        for (uint32_t s = 0; s < slots; ++s) {
            if (hipMalloc(&d_out[s], bytes) != hipSuccess) return ring_fail(TRI_E_OOM, who, "buffer allocation failed");
            if (hipEventCreateWithFlags(&converted[s], hipEventDisableTiming) != hipSuccess)
                return ring_fail(TRI_E_HIP, who, "event creation failed");
            if (!host_copy) continue;
            if (hipHostMalloc(&h_out[s], bytes, hipHostMallocDefault) != hipSuccess)
                return ring_fail(TRI_E_OOM, who, "pinned allocation failed");
            if (hipEventCreateWithFlags(&copied[s], hipEventDisableTiming) != hipSuccess)
                return ring_fail(TRI_E_HIP, who, "event creation failed");
        }
        return TRI_OK;
    }

    // Safe with captures in flight and on a partly built ring.
    void destroy() {
        (void)hipSetDevice(device);
        if (copy) (void)hipStreamSynchronize(copy);
        for (uint32_t s = 0; s < kMaxSlots; ++s) {
            // (a conversion still queued on a context's stream writes d_out: wait for it before the buffer goes)
            if (busy[s] && converted[s]) (void)hipEventSynchronize(converted[s]);
            if (d_out[s]) (void)hipFree(d_out[s]);
            if (h_out[s]) (void)hipHostFree(h_out[s]);
            if (converted[s]) (void)hipEventDestroy(converted[s]);
            if (copied[s]) (void)hipEventDestroy(copied[s]);
        }
        if (copy) (void)hipStreamDestroy(copy);
    }

    int capture(const char* who, const char* noun, uint32_t slot, tri_ctx* ctx, ConvertFn convert) {
        if (slot >= slots) return ring_fail(TRI_E_INVALID, who, "slot out of range");
        if (!tri_internal_whole_frame(ctx)) return ring_fail(TRI_E_STATE, who, "a row-band context has no whole frame");
        tri_image img;
        const int rc = tri_get_output(ctx, &img);
        if (rc) return rc;
        if (img.device != device) return ring_fail(TRI_E_INVALID, who, "the context is on another device");
        if (img.width != width || img.height != height)
            return ring_fail(TRI_E_INVALID, who, "the context's extent differs from the ", noun, "'s");
        if (busy[slot]) return ring_fail(TRI_E_STATE, who, "the slot is busy (wait for it and release it)");
        TRI_HIP_TRY(hipSetDevice(device));
        hipStream_t s = tri_internal_stream(ctx);
        TRI_HIP_TRY(convert(img.device_ptr, img.width, img.height, img.pitch_bytes, d_out[slot], s));
        hipError_t e = hipEventRecord(converted[slot], s);
        if (host_copy) {
            if (e == hipSuccess) e = hipStreamWaitEvent(copy, converted[slot], 0);
            if (e == hipSuccess) e = hipMemcpyAsync(h_out[slot], d_out[slot], bytes, hipMemcpyDeviceToHost, copy);
            if (e == hipSuccess) e = hipEventRecord(copied[slot], copy);
        }
        if (e != hipSuccess) {  // the slot stays idle: nothing of this capture may still be running on its buffers
            (void)hipStreamSynchronize(s);
            if (copy) (void)hipStreamSynchronize(copy);
            return tri_hip_fail(e, who);
        }
        busy[slot] = true;
        return TRI_OK;
    }

    // The slot's product on the device, complete.
    int wait_converted(const char* who, uint32_t slot) {
        if (slot >= slots) return ring_fail(TRI_E_INVALID, who, "slot out of range");
        if (!busy[slot]) return ring_fail(TRI_E_STATE, who, "the slot is idle (nothing was captured)");
        TRI_HIP_TRY(hipSetDevice(device));
        TRI_HIP_TRY(hipEventSynchronize(converted[slot]));
        return TRI_OK;
    }
    // The slot's product in pinned memory, complete (and with it the one on the device: the copy follows the conversion).
    int wait_copied(const char* who, const char* noun, uint32_t slot) {
        if (slot >= slots) return ring_fail(TRI_E_INVALID, who, "slot out of range");
        if (!host_copy) return ring_fail(TRI_E_STATE, who, "the ", noun, " was created without TRI_GRAB_HOST_COPY");
        if (!busy[slot]) return ring_fail(TRI_E_STATE, who, "the slot is idle (nothing was captured)");
        TRI_HIP_TRY(hipSetDevice(device));
        TRI_HIP_TRY(hipEventSynchronize(copied[slot]));
        return TRI_OK;
    }

    int release(const char* who, uint32_t slot) {
        if (slot >= slots) return ring_fail(TRI_E_INVALID, who, "slot out of range");
        if (!busy[slot]) return TRI_OK;
        // a capture still in flight finishes first, so the slot's next capture cannot race this one's conversion or copy
        TRI_HIP_TRY(hipSetDevice(device));
        TRI_HIP_TRY(hipEventSynchronize(converted[slot]));
        if (host_copy) TRI_HIP_TRY(hipEventSynchronize(copied[slot]));
        busy[slot] = false;
        return TRI_OK;
    }
};

}  // namespace

struct tri_recorder {
    CaptureRing ring;  // 3 bytes per pixel, always with the host copy
};
struct tri_framegrab {
    CaptureRing ring;  // 16 bytes per pixel
};

extern "C" {

int tri_convert_yuv444(const void* bgra, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* yuv, void* stream) {
    if (!yuv) return tri_internal_fail(TRI_E_INVALID, "tri_convert_yuv444: null pointer");
    if (const int rc = tri_check_bgra_source("tri_convert_yuv444", bgra, width, height, pitch_bytes)) return rc;
    TRI_HIP_TRY(convert_yuv444(bgra, width, height, pitch_bytes, yuv, static_cast<hipStream_t>(stream)));
    return TRI_OK;
}

int tri_convert_rgba_f32(const void* bgra, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* f32, void* stream) {
    if (!f32) return tri_internal_fail(TRI_E_INVALID, "tri_convert_rgba_f32: null pointer");
    if (const int rc = tri_check_bgra_source("tri_convert_rgba_f32", bgra, width, height, pitch_bytes)) return rc;
    if ((uintptr_t)f32 & 3u) return tri_internal_fail(TRI_E_INVALID, "tri_convert_rgba_f32: output must be 4-B aligned");
    TRI_HIP_TRY(convert_rgba_f32(bgra, width, height, pitch_bytes, f32, static_cast<hipStream_t>(stream)));
    return TRI_OK;
}

int tri_recorder_create(int32_t device, uint32_t width, uint32_t height, uint32_t slots, tri_recorder** out) {
    if (!out) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_create: null argument");
    *out = nullptr;
    if (const int rc = CaptureRing::check("tri_recorder_create", width, height, slots)) return rc;
    CaptureRing ring;
    if (const int rc = ring.create("tri_recorder_create", device, width, height, slots, 3, true)) return rc;
    *out = new tri_recorder{ring};
    return TRI_OK;
}

int tri_recorder_destroy(tri_recorder* r) {
    if (!r) return TRI_OK;
    r->ring.destroy();
    delete r;
    return TRI_OK;
}

int tri_recorder_capture(tri_recorder* r, uint32_t slot, tri_ctx* ctx) {
    if (!r || !ctx) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_capture: null argument");
    return r->ring.capture("tri_recorder_capture", "recorder", slot, ctx, convert_yuv444);
}

int tri_recorder_wait(tri_recorder* r, uint32_t slot, const uint8_t** yuv) {
    if (!r || !yuv) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_wait: null argument");
    if (const int rc = r->ring.wait_copied("tri_recorder_wait", "recorder", slot)) return rc;
    *yuv = static_cast<const uint8_t*>(r->ring.h_out[slot]);
    return TRI_OK;
}

int tri_recorder_release(tri_recorder* r, uint32_t slot) {
    if (!r) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_release: null recorder");
    return r->ring.release("tri_recorder_release", slot);
}

int tri_framegrab_create(int32_t device, uint32_t width, uint32_t height, uint32_t slots, uint32_t flags, tri_framegrab** out) {
    if (!out) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_create: null argument");
    *out = nullptr;
    if (const int rc = CaptureRing::check("tri_framegrab_create", width, height, slots)) return rc;
    if (flags & ~(uint32_t)TRI_GRAB_HOST_COPY) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_create: unknown flag");
    CaptureRing ring;
    if (const int rc = ring.create("tri_framegrab_create", device, width, height, slots, 16, (flags & TRI_GRAB_HOST_COPY) != 0))
        return rc;
    *out = new tri_framegrab{ring};
    return TRI_OK;
}

int tri_framegrab_destroy(tri_framegrab* g) {
    if (!g) return TRI_OK;
    g->ring.destroy();
    delete g;
    return TRI_OK;
}

int tri_framegrab_capture(tri_framegrab* g, uint32_t slot, tri_ctx* ctx) {
    if (!g || !ctx) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_capture: null argument");
    return g->ring.capture("tri_framegrab_capture", "grab", slot, ctx, convert_rgba_f32);
}

int tri_framegrab_wait(tri_framegrab* g, uint32_t slot, const float** host, const float** device) {
    if (!g || (!host && !device)) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_wait: null argument");
    const int rc = host ? g->ring.wait_copied("tri_framegrab_wait", "grab", slot) : g->ring.wait_converted("tri_framegrab_wait", slot);
    if (rc) return rc;
    if (device) *device = static_cast<const float*>(g->ring.d_out[slot]);
    if (host) *host = static_cast<const float*>(g->ring.h_out[slot]);
    return TRI_OK;
}

int tri_framegrab_release(tri_framegrab* g, uint32_t slot) {
    if (!g) return tri_internal_fail(TRI_E_INVALID, "tri_framegrab_release: null grab");
    return g->ring.release("tri_framegrab_release", slot);
}

}  // extern "C"
