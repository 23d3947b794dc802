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
//
// A product may be of variable size (the recorder's JPEG stream, jpeg_encode.hip): its conversion leaves the size in a
// word beside the buffer, the capture copies only that word, and the first wait copies the product's own bytes
// (rounded up to 256), never the worst-case buffer.
#include "capi_util.h"
#include "jpeg_math.h"
#include "raster_launch.h"

#include <hip/hip_runtime.h>

#include <cstdio>

namespace {

constexpr uint32_t kMaxSlots = 8;

struct CaptureRing;
// The conversion of one product: src (the ring's extent, B8G8R8A8 at pitch_bytes) -> the slot's buffers, on `stream`.
using ConvertFn = hipError_t (*)(const CaptureRing& ring, uint32_t slot, const void* src, uint32_t pitch, hipStream_t stream);

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
    size_t bytes = 0;                      // a slot's buffer: the product, or the largest one of a variable product
    bool variable = false;                 // the conversion writes the product's size to d_size[slot]
    void* product = nullptr;               // what the conversion needs besides the buffers (not owned)
    hipStream_t copy = nullptr;            // the device-to-host copies (only with host_copy; never the render stream)
    hipStream_t fetch = nullptr;           // (variable) a product's own bytes, copied by its wait: never behind a later capture
    void* d_out[kMaxSlots] = {};           // the conversion's output: what a consumer on the device reads
    void* h_out[kMaxSlots] = {};           // pinned (only with host_copy)
    hipEvent_t converted[kMaxSlots] = {};  // recorded on the context's stream behind the conversion
    hipEvent_t copied[kMaxSlots] = {};     // recorded on the copy stream behind the copy (only with host_copy)
    uint32_t* d_size[kMaxSlots] = {};      // (variable) the size word beside d_out
    uint32_t* h_size[kMaxSlots] = {};      // (variable) pinned; `copied` then stands for this word alone
    bool fetched[kMaxSlots] = {};          // (variable) the product's bytes are in h_out
    size_t h_bytes[kMaxSlots] = {};        // what h_out holds: `bytes`, or (variable) what the products have needed so far
    bool busy[kMaxSlots] = {};

    // The argument checks of a create, before any HIP call: extent, then slots (the grab's flags follow in its wrapper).
    static int check(const char* who, uint32_t width, uint32_t height, uint32_t slots) {
        if (const int rc = tri_check_extent(who, width, height)) return rc;
        if (slots == 0 || slots > kMaxSlots) return ring_fail(TRI_E_INVALID, who, "slots outside 1..8");
        return TRI_OK;
    }

    // After check(). `dev` as in tri_resolve_device; on an error nothing of the ring is left.
    int create(const char* who, int32_t dev, uint32_t w, uint32_t h, uint32_t nslots, uint32_t bytes_per_pixel, bool with_host_copy) {
        return create_sized(who, dev, w, h, nslots, (size_t)bytes_per_pixel * w * h, with_host_copy, false);
    }
    // A slot of slot_bytes; with variable_size a product of up to slot_bytes (then always with the host copy).
    int create_sized(const char* who, int32_t dev, uint32_t w, uint32_t h, uint32_t nslots, size_t slot_bytes, bool with_host_copy,
                     bool variable_size) {
        if (const int rc = tri_resolve_device(dev, who, &device)) return rc;
        variable = variable_size;
        const int rc = build(who, w, h, nslots, slot_bytes, with_host_copy);
        if (rc) destroy();
        return rc;
    }

    // A pinned size for a variable product of `need` bytes: whole pages, at most the slot's buffer.
    size_t pinned_size(size_t need) const {
        const size_t pages = (need + 4095) & ~(size_t)4095;
        return pages < bytes ? (pages ? pages : 4096) : bytes;
    }

    int build(const char* who, uint32_t w, uint32_t h, uint32_t nslots, size_t slot_bytes, bool with_host_copy) {
        width = w;
        height = h;
        slots = nslots;
        host_copy = with_host_copy;
        bytes = slot_bytes;
        if (hipSetDevice(device) != hipSuccess) return ring_fail(TRI_E_HIP, who, "hipSetDevice failed");
        if (host_copy && hipStreamCreateWithFlags(&copy, hipStreamNonBlocking) != hipSuccess)
            return ring_fail(TRI_E_HIP, who, "stream creation failed");
        if (host_copy && variable && hipStreamCreateWithFlags(&fetch, hipStreamNonBlocking) != hipSuccess)
            return ring_fail(TRI_E_HIP, who, "stream creation failed");
        for (uint32_t s = 0; s < slots; ++s) {
            if (hipMalloc(&d_out[s], bytes) != hipSuccess) return ring_fail(TRI_E_OOM, who, "buffer allocation failed");
            if (hipEventCreateWithFlags(&converted[s], hipEventDisableTiming) != hipSuccess)
                return ring_fail(TRI_E_HIP, who, "event creation failed");
            if (!host_copy) continue;
            // a variable product starts at half a byte per pixel and grows in wait_copied: pinning the worst case
            // (9.7 B/pixel for a JPEG) would cost more than a whole recording session of ordinary frames
            h_bytes[s] = variable ? pinned_size((size_t)width * height / 2) : bytes;
            if (hipHostMalloc(&h_out[s], h_bytes[s], hipHostMallocDefault) != hipSuccess)
                return ring_fail(TRI_E_OOM, who, "pinned allocation failed");
            if (hipEventCreateWithFlags(&copied[s], hipEventDisableTiming) != hipSuccess)
                return ring_fail(TRI_E_HIP, who, "event creation failed");
            if (!variable) continue;
            if (hipMalloc(reinterpret_cast<void**>(&d_size[s]), sizeof(uint32_t)) != hipSuccess)
                return ring_fail(TRI_E_OOM, who, "buffer allocation failed");
            if (hipHostMalloc(reinterpret_cast<void**>(&h_size[s]), sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
                return ring_fail(TRI_E_OOM, who, "pinned allocation failed");
        }
        return TRI_OK;
    }

    // Safe with captures in flight and on a partly built ring.
    void destroy() {
        (void)hipSetDevice(device);
        if (copy) (void)hipStreamSynchronize(copy);
        if (fetch) (void)hipStreamSynchronize(fetch);
        for (uint32_t s = 0; s < kMaxSlots; ++s) {
            // (a conversion still queued on a context's stream writes d_out: wait for it before the buffer goes)
            if (busy[s] && converted[s]) (void)hipEventSynchronize(converted[s]);
            if (d_out[s]) (void)hipFree(d_out[s]);
            if (h_out[s]) (void)hipHostFree(h_out[s]);
            if (d_size[s]) (void)hipFree(d_size[s]);
            if (h_size[s]) (void)hipHostFree(h_size[s]);
            if (converted[s]) (void)hipEventDestroy(converted[s]);
            if (copied[s]) (void)hipEventDestroy(copied[s]);
        }
        if (copy) (void)hipStreamDestroy(copy);
        if (fetch) (void)hipStreamDestroy(fetch);
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
        return capture_image(who, slot, img.device_ptr, img.pitch_bytes, tri_internal_stream(ctx), convert);
    }

    // The capture itself, from an image of the ring's extent on its device, ordered on `s`.
    int capture_image(const char* who, uint32_t slot, const void* src, uint32_t pitch_bytes, hipStream_t s, ConvertFn convert) {
        if (slot >= slots) return ring_fail(TRI_E_INVALID, who, "slot out of range");
        if (busy[slot]) return ring_fail(TRI_E_STATE, who, "the slot is busy (wait for it and release it)");
        TRI_HIP_TRY(hipSetDevice(device));
        TRI_HIP_TRY(convert(*this, slot, src, pitch_bytes, s));
        hipError_t e = hipEventRecord(converted[slot], s);
        if (host_copy) {
            if (e == hipSuccess) e = hipStreamWaitEvent(copy, converted[slot], 0);
            if (e == hipSuccess)
                e = variable ? hipMemcpyAsync(h_size[slot], d_size[slot], sizeof(uint32_t), hipMemcpyDeviceToHost, copy)
                             : hipMemcpyAsync(h_out[slot], d_out[slot], bytes, hipMemcpyDeviceToHost, copy);
            if (e == hipSuccess) e = hipEventRecord(copied[slot], copy);
        }
        if (e != hipSuccess) {  // the slot stays idle: nothing of this capture may still be running on its buffers
            (void)hipStreamSynchronize(s);
            if (copy) (void)hipStreamSynchronize(copy);
            return tri_hip_fail(e, who);
        }
        busy[slot] = true;
        fetched[slot] = false;
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
    // `product_bytes`, when given, receives the product's size; a variable product's bytes are copied here, once.
    int wait_copied(const char* who, const char* noun, uint32_t slot, uint64_t* product_bytes = nullptr) {
        if (slot >= slots) return ring_fail(TRI_E_INVALID, who, "slot out of range");
        if (!host_copy) return ring_fail(TRI_E_STATE, who, "the ", noun, " was created without TRI_GRAB_HOST_COPY");
        if (!busy[slot]) return ring_fail(TRI_E_STATE, who, "the slot is idle (nothing was captured)");
        TRI_HIP_TRY(hipSetDevice(device));
        TRI_HIP_TRY(hipEventSynchronize(copied[slot]));
        if (variable && !fetched[slot]) {
            const size_t size = *h_size[slot];
            if (size > bytes) return ring_fail(TRI_E_HIP, who, "the product's size word is beyond its buffer");
            const size_t rounded = (size + 255) & ~(size_t)255;
            const size_t copy_bytes = rounded < bytes ? rounded : bytes;
            if (copy_bytes > h_bytes[slot]) {  // grow by half again; nobody holds the old pointer before this wait returns
                if (h_out[slot]) (void)hipHostFree(h_out[slot]);
                h_out[slot] = nullptr;
                h_bytes[slot] = 0;
                const size_t grown = pinned_size(copy_bytes + copy_bytes / 2);
                if (hipHostMalloc(&h_out[slot], grown, hipHostMallocDefault) != hipSuccess)
                    return ring_fail(TRI_E_OOM, who, "pinned allocation failed");
                h_bytes[slot] = grown;
            }
            // the slot's conversion is complete (its size word followed it), so the copy depends on nothing; the copy
            // stream may already hold later slots' size words behind frames that still render, and this wait must not
            // wait for those: the fetch stream holds nothing but this copy
            TRI_HIP_TRY(hipMemcpyAsync(h_out[slot], d_out[slot], copy_bytes, hipMemcpyDeviceToHost, fetch));
            TRI_HIP_TRY(hipStreamSynchronize(fetch));
            fetched[slot] = true;
        }
        if (product_bytes) *product_bytes = variable ? *h_size[slot] : bytes;
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

// A JPEG recorder's device state besides the ring's output buffers (which hold the header from the start).
struct JpegState {
    jpeg::Layout layout{};
    void* tables = nullptr;
    int16_t* coef[kMaxSlots] = {};
    uint8_t* scratch[kMaxSlots] = {};
    uint32_t* counts[kMaxSlots] = {};  // counts, then offsets: 2 * intervals dwords

    void destroy() {
        if (tables) (void)hipFree(tables);
        for (uint32_t s = 0; s < kMaxSlots; ++s) {
            if (coef[s]) (void)hipFree(coef[s]);
            if (scratch[s]) (void)hipFree(scratch[s]);
            if (counts[s]) (void)hipFree(counts[s]);
        }
    }
};

hipError_t convert_yuv444(const CaptureRing& r, uint32_t slot, const void* src, uint32_t pitch, hipStream_t s) {
    return tri_launch_bgra_to_yuv444(src, r.width, r.height, pitch, static_cast<uint8_t*>(r.d_out[slot]), s);
}
hipError_t convert_rgba_f32(const CaptureRing& r, uint32_t slot, const void* src, uint32_t pitch, hipStream_t s) {
    return tri_launch_bgra_to_rgba_f32(src, r.width, r.height, pitch, static_cast<float*>(r.d_out[slot]), s);
}
hipError_t convert_jpeg(const CaptureRing& r, uint32_t slot, const void* src, uint32_t pitch, hipStream_t s) {
    const JpegState& j = *static_cast<const JpegState*>(r.product);
    tri_jpeg_job job{};
    job.src = src;
    job.pitch_bytes = pitch;
    job.width = r.width;
    job.height = r.height;
    job.restart = j.layout.restart;
    job.segment_bytes = j.layout.segment_bytes;
    job.header_bytes = jpeg::kHeaderBytes;
    job.tables = j.tables;
    job.coef = j.coef[slot];
    job.scratch = j.scratch[slot];
    job.counts = j.counts[slot];
    job.offsets = j.counts[slot] + j.layout.intervals;
    job.out = static_cast<uint8_t*>(r.d_out[slot]);
    job.size_word = r.d_size[slot];
    return tri_launch_jpeg_encode(job, s);
}

// The parameters of a JPEG entry point: `p` checked, then the extent by the format's own rule.
int jpeg_check(const char* who, uint32_t width, uint32_t height, const tri_record_params* p) {
    jpeg::Msg m;
    int rc = jpeg::check_params(p, m);
    if (!rc && p->format != TRI_RECORD_JPEG420) {
        snprintf(m.text, sizeof m.text, "the format is not TRI_RECORD_JPEG420");
        rc = TRI_E_INVALID;
    }
    if (!rc) rc = jpeg::check_extent(width, height, m);
    return rc ? ring_fail(rc, who, m.text) : TRI_OK;
}

}  // namespace

struct tri_recorder {
    CaptureRing ring;  // YUV444: 3 bytes per pixel; JPEG: a variable product. Always with the host copy
    uint32_t format = TRI_RECORD_YUV444;
    JpegState* jpeg = nullptr;
};

namespace {

// The JPEG recorder's buffers on the ring's device (the current one). On an error the caller destroys `j`.
int jpeg_build(const char* who, CaptureRing& ring, JpegState& j, const tri_record_params& p) {
    jpeg::Tables host_tables;
    jpeg::build_tables(p.quality, host_tables);
    uint8_t header[jpeg::kHeaderBytes];
    jpeg::write_header(j.layout, host_tables, header);
    if (hipMalloc(&j.tables, sizeof host_tables) != hipSuccess) return ring_fail(TRI_E_OOM, who, "buffer allocation failed");
    TRI_HIP_TRY(hipMemcpy(j.tables, &host_tables, sizeof host_tables, hipMemcpyHostToDevice));
    for (uint32_t s = 0; s < ring.slots; ++s) {
        if (hipMalloc(reinterpret_cast<void**>(&j.coef[s]), (size_t)j.layout.mcus * jpeg::kCoefPerMcu * sizeof(int16_t)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&j.scratch[s]), (size_t)j.layout.intervals * j.layout.segment_bytes) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&j.counts[s]), (size_t)j.layout.intervals * 2 * sizeof(uint32_t)) != hipSuccess)
            return ring_fail(TRI_E_OOM, who, "buffer allocation failed");
        TRI_HIP_TRY(hipMemcpy(ring.d_out[s], header, sizeof header, hipMemcpyHostToDevice));
    }
    return TRI_OK;
}

}  // namespace

struct tri_framegrab {
    CaptureRing ring;  // 16 bytes per pixel
};

extern "C" {

int tri_convert_yuv444(const void* bgra, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* yuv, void* stream) {
    if (!yuv) return tri_internal_fail(TRI_E_INVALID, "tri_convert_yuv444: null pointer");
    if (const int rc = tri_check_bgra_source("tri_convert_yuv444", bgra, width, height, pitch_bytes)) return rc;
    TRI_HIP_TRY(tri_launch_bgra_to_yuv444(bgra, width, height, pitch_bytes, static_cast<uint8_t*>(yuv), static_cast<hipStream_t>(stream)));
    return TRI_OK;
}

int tri_convert_rgba_f32(const void* bgra, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* f32, void* stream) {
    if (!f32) return tri_internal_fail(TRI_E_INVALID, "tri_convert_rgba_f32: null pointer");
    if (const int rc = tri_check_bgra_source("tri_convert_rgba_f32", bgra, width, height, pitch_bytes)) return rc;
    if ((uintptr_t)f32 & 3u) return tri_internal_fail(TRI_E_INVALID, "tri_convert_rgba_f32: output must be 4-B aligned");
    TRI_HIP_TRY(tri_launch_bgra_to_rgba_f32(bgra, width, height, pitch_bytes, static_cast<float*>(f32), static_cast<hipStream_t>(stream)));
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

int tri_recorder_create_ex(int32_t device, uint32_t width, uint32_t height, uint32_t slots, const tri_record_params* params,
                           tri_recorder** out) {
    const char* who = "tri_recorder_create_ex";
    if (!out) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_create_ex: null argument");
    *out = nullptr;
    if (params) {
        jpeg::Msg m;
        if (const int rc = jpeg::check_params(params, m)) return ring_fail(rc, who, m.text);
    }
    if (const int rc = CaptureRing::check(who, width, height, slots)) return rc;
    CaptureRing ring;
    if (!params || params->format == TRI_RECORD_YUV444) {
        if (const int rc = ring.create(who, device, width, height, slots, 3, true)) return rc;
        *out = new tri_recorder{ring};
        return TRI_OK;
    }
    JpegState* j = new JpegState;
    j->layout = jpeg::make_layout(width, height, params->restart_mcus);
    int rc = ring.create_sized(who, device, width, height, slots, (size_t)jpeg::max_bytes(j->layout), true, true);
    if (!rc) {
        rc = jpeg_build(who, ring, *j, *params);
        if (rc) ring.destroy();
    }
    if (rc) {
        j->destroy();
        delete j;
        return rc;
    }
    ring.product = j;
    *out = new tri_recorder{ring, TRI_RECORD_JPEG420, j};
    return TRI_OK;
}

int tri_recorder_destroy(tri_recorder* r) {
    if (!r) return TRI_OK;
    r->ring.destroy();  // (waits for the captures in flight, which read the JPEG state)
    if (r->jpeg) {
        r->jpeg->destroy();
        delete r->jpeg;
    }
    delete r;
    return TRI_OK;
}

int tri_recorder_capture(tri_recorder* r, uint32_t slot, tri_ctx* ctx) {
    if (!r || !ctx) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_capture: null argument");
    return r->ring.capture("tri_recorder_capture", "recorder", slot, ctx, r->jpeg ? convert_jpeg : convert_yuv444);
}

int tri_recorder_capture_image(tri_recorder* r, uint32_t slot, const void* bgra, uint32_t pitch_bytes, void* stream) {
    const char* who = "tri_recorder_capture_image";
    if (!r) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_capture_image: null recorder");
    if (const int rc = tri_check_bgra_source(who, bgra, r->ring.width, r->ring.height, pitch_bytes)) return rc;
    return r->ring.capture_image(who, slot, bgra, pitch_bytes, static_cast<hipStream_t>(stream),
                                 r->jpeg ? convert_jpeg : convert_yuv444);
}

int tri_recorder_wait_ex(tri_recorder* r, uint32_t slot, const uint8_t** data, uint64_t* bytes) {
    if (!r || !data || !bytes) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_wait_ex: null argument");
    if (const int rc = r->ring.wait_copied("tri_recorder_wait_ex", "recorder", slot, bytes)) return rc;
    *data = static_cast<const uint8_t*>(r->ring.h_out[slot]);
    return TRI_OK;
}

int tri_jpeg_header(uint32_t width, uint32_t height, const tri_record_params* params, uint8_t* out, uint32_t capacity,
                    uint32_t* bytes) {
    if (!out || !bytes) return tri_internal_fail(TRI_E_INVALID, "tri_jpeg_header: null argument");
    if (const int rc = jpeg_check("tri_jpeg_header", width, height, params)) return rc;
    jpeg::Msg m;
    if (const int rc = jpeg::check_capacity(jpeg::kHeaderBytes, capacity, m)) return ring_fail(rc, "tri_jpeg_header", m.text);
    jpeg::Tables t;
    jpeg::build_tables(params->quality, t);
    *bytes = jpeg::write_header(jpeg::make_layout(width, height, params->restart_mcus), t, out);
    return TRI_OK;
}

uint64_t tri_jpeg_max_bytes(uint32_t width, uint32_t height, const tri_record_params* params) {
    if (jpeg_check("tri_jpeg_max_bytes", width, height, params)) return 0;
    return jpeg::max_bytes(jpeg::make_layout(width, height, params->restart_mcus));
}

int tri_recorder_wait(tri_recorder* r, uint32_t slot, const uint8_t** yuv) {
    if (!r || !yuv) return tri_internal_fail(TRI_E_INVALID, "tri_recorder_wait: null argument");
    if (r->jpeg) return tri_internal_fail(TRI_E_STATE, "tri_recorder_wait: a JPEG recorder's product has a size (tri_recorder_wait_ex)");
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
