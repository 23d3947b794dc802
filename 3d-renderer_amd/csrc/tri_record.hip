// tri_record.hip — the recording entry points of the C-ABI (include/tri_raster.h): tri_convert_yuv444 and tri_recorder.
//
// A recorder turns frames into the Y4M payload (planar YUV 4:4:4, VideoEncoder.cpp:370-412, :716-736) without
// stalling the renderer: tri_recorder_capture enqueues the conversion behind the frame on the context's stream and
// the device-to-host copy on the recorder's own stream, into pinned memory; the caller collects the planes a few
// frames later (tri_recorder_wait) while the next frames render. Slot protocol: idle -> capture -> busy -> wait
// (any number of times) -> release -> idle.
#include "raster_launch.h"

#include <hip/hip_runtime.h>

#include <string>

namespace {

constexpr uint32_t kMaxSlots = 8;

int hip_fail(hipError_t e, const char* what) {
    const std::string m = std::string(what) + ": " + hipGetErrorString(e);
    return tri_internal_fail(e == hipErrorOutOfMemory ? TRI_E_OOM : TRI_E_HIP, m.c_str());
}

#define RH(expr)                                          \
    do {                                                  \
        const hipError_t _e = (expr);                     \
        if (_e != hipSuccess) return hip_fail(_e, #expr); \
    } while (0)

}  // namespace

struct tri_recorder {
    int device = 0;
    uint32_t width = 0, height = 0, slots = 0;
    size_t bytes = 0;                   // 3 * width * height
    hipStream_t copy = nullptr;         // the device-to-host copies (never the render stream)
    uint8_t* d_yuv[kMaxSlots] = {};     // the conversion's output
    uint8_t* h_yuv[kMaxSlots] = {};     // pinned: what tri_recorder_wait returns
    hipEvent_t converted[kMaxSlots] = {};  // recorded on the context's stream behind the conversion
    hipEvent_t copied[kMaxSlots] = {};     // recorded on the copy stream behind the copy
    bool busy[kMaxSlots] = {};
};

extern "C" {

int tri_convert_yuv444(const void* bgra, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* yuv, void* stream) {
    if (!bgra || !yuv) return tri_internal_fail(TRI_E_INVALID, "tri_convert_yuv444: null pointer");
    if (width == 0 || height == 0 || width > TRI_MAX_DIM || height > TRI_MAX_DIM)
        return tri_internal_fail(TRI_E_INVALID, "tri_convert_yuv444: extent outside 1..TRI_MAX_DIM");
    if (pitch_bytes < width * 4u || (pitch_bytes & 3u))
        return tri_internal_fail(TRI_E_INVALID, "tri_convert_yuv444: pitch below width * 4 or not a multiple of 4");
    if ((uintptr_t)bgra & 3u) return tri_internal_fail(TRI_E_INVALID, "tri_convert_yuv444: source must be 4-B aligned");
    const hipError_t e = tri_launch_bgra_to_yuv444(bgra, width, height, pitch_bytes, static_cast<uint8_t*>(yuv),
                                                   static_cast<hipStream_t>(stream));
    return e == hipSuccess ? TRI_OK : tri_internal_fail(TRI_E_HIP, hipGetErrorString(e));
}

int tri_recorder_destroy(tri_recorder* r) {
    if (!r) return TRI_OK;
    (void)hipSetDevice(r->device);
    if (r->copy) (void)hipStreamSynchronize(r->copy);
    for (uint32_t s = 0; s < kMaxSlots; ++s) {
        // (a conversion still queued on a context's stream writes d_yuv: wait for it before the buffer goes)
        if (r->busy[s] && r->converted[s]) (void)hipEventSynchronize(r->converted[s]);
        if (r->d_yuv[s]) (void)hipFree(r->d_yuv[s]);
        if (r->h_yuv[s]) (void)hipHostFree(r->h_yuv[s]);
        if (r->converted[s]) (void)hipEventDestroy(r->converted[s]);
        if (r->copied[s]) (void)hipEventDestroy(r->copied[s]);
    }
    if (r->copy) (void)hipStreamDestroy(r->copy);
    delete r;
    return TRI_OK;
}

int tri_recorder_create(int32_t device, uint32_t width, uint32_t height, uint32_t slots, tri_recorder** out) {
    if (!out) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_create: null argument");
    *out = nullptr;
    if (width == 0 || height == 0 || width > TRI_MAX_DIM || height > TRI_MAX_DIM)
        return tri_internal_fail(TRI_E_INVALID, "tri_recorder_create: extent outside 1..TRI_MAX_DIM");
    if (slots == 0 || slots > kMaxSlots) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_create: slots outside 1..8");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return tri_internal_fail(TRI_E_HIP, "tri_recorder_create: no HIP device available");
    int dev = device;
    if (device < 0) {
        if (hipGetDevice(&dev) != hipSuccess) return tri_internal_fail(TRI_E_HIP, "tri_recorder_create: hipGetDevice failed");
    } else if (device >= ndev) {
        return tri_internal_fail(TRI_E_INVALID, "tri_recorder_create: device ordinal out of range");
    }
    tri_recorder* r = new tri_recorder();
    r->device = dev;
    r->width = width;
    r->height = height;
    r->slots = slots;
    r->bytes = (size_t)3 * width * height;
    auto bail = [&](int rc) { tri_recorder_destroy(r); return rc; };
    if (hipSetDevice(dev) != hipSuccess) return bail(tri_internal_fail(TRI_E_HIP, "tri_recorder_create: hipSetDevice failed"));
    if (hipStreamCreateWithFlags(&r->copy, hipStreamNonBlocking) != hipSuccess)
        return bail(tri_internal_fail(TRI_E_HIP, "tri_recorder_create: stream creation failed"));
    for (uint32_t s = 0; s < slots; ++s) {
        if (hipMalloc(reinterpret_cast<void**>(&r->d_yuv[s]), r->bytes) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void**>(&r->h_yuv[s]), r->bytes, hipHostMallocDefault) != hipSuccess)
            return bail(tri_internal_fail(TRI_E_OOM, "tri_recorder_create: buffer allocation failed"));
        if (hipEventCreateWithFlags(&r->converted[s], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&r->copied[s], hipEventDisableTiming) != hipSuccess)
            return bail(tri_internal_fail(TRI_E_HIP, "tri_recorder_create: event creation failed"));
    }
    *out = r;
    return TRI_OK;
}

int tri_recorder_capture(tri_recorder* r, uint32_t slot, tri_ctx* ctx) {
    if (!r || !ctx) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_capture: null argument");
    if (slot >= r->slots) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_capture: slot out of range");
    if (!tri_internal_whole_frame(ctx))
        return tri_internal_fail(TRI_E_STATE, "tri_recorder_capture: a row-band context has no whole frame");
    tri_image img;
    const int rc = tri_get_output(ctx, &img);
    if (rc) return rc;
    if (img.device != r->device) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_capture: the context is on another device");
    if (img.width != r->width || img.height != r->height)
        return tri_internal_fail(TRI_E_INVALID, "tri_recorder_capture: the context's extent differs from the recorder's");
    if (r->busy[slot]) return tri_internal_fail(TRI_E_STATE, "tri_recorder_capture: the slot is busy (wait for it and release it)");
    RH(hipSetDevice(r->device));
    hipStream_t s = tri_internal_stream(ctx);
    RH(tri_launch_bgra_to_yuv444(img.device_ptr, img.width, img.height, img.pitch_bytes, r->d_yuv[slot], s));
    hipError_t e = hipEventRecord(r->converted[slot], s);
    if (e == hipSuccess) e = hipStreamWaitEvent(r->copy, r->converted[slot], 0);
    if (e == hipSuccess) e = hipMemcpyAsync(r->h_yuv[slot], r->d_yuv[slot], r->bytes, hipMemcpyDeviceToHost, r->copy);
    if (e == hipSuccess) e = hipEventRecord(r->copied[slot], r->copy);
    if (e != hipSuccess) {  // the slot stays idle: nothing of this capture may still be running on its buffers
        (void)hipStreamSynchronize(s);
        (void)hipStreamSynchronize(r->copy);
        return hip_fail(e, "tri_recorder_capture");
    }
    r->busy[slot] = true;
    return TRI_OK;
}

int tri_recorder_wait(tri_recorder* r, uint32_t slot, const uint8_t** yuv) {
    if (!r || !yuv) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_wait: null argument");
    if (slot >= r->slots) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_wait: slot out of range");
    if (!r->busy[slot]) return tri_internal_fail(TRI_E_STATE, "tri_recorder_wait: the slot is idle (nothing was captured)");
    RH(hipSetDevice(r->device));
    RH(hipEventSynchronize(r->copied[slot]));
    *yuv = r->h_yuv[slot];
    return TRI_OK;
}

int tri_recorder_release(tri_recorder* r, uint32_t slot) {
    if (!r) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_release: null recorder");
    if (slot >= r->slots) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_release: slot out of range");
    if (!r->busy[slot]) return TRI_OK;
    // a capture still in flight finishes first, so the slot's next capture cannot race this one's copy
    RH(hipSetDevice(r->device));
    RH(hipEventSynchronize(r->copied[slot]));
    r->busy[slot] = false;
    return TRI_OK;
}

}  // extern "C"
