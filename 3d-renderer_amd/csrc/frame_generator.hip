// frame_generator.hip — tri_framegen (include/tri_raster.h "the frame generator"): the reference's InterpolationUNet
// as 20 tri_launch_nn_conv launches (nn_conv.hip) on a stream of the generator's own, behind an event on the
// producer's stream. The weights come from a container (framegen_container.h); every activation of one frozen extent
// is allocated at creation, as the reference's export freezes its shapes. No graph capture, no host thread: the
// device stream is the worker, and the host only records and queries events.
#include "capi_util.h"
#include "raster_launch.h"
#include "framegen_container.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

struct tri_framegen {
    int device = 0;
    uint32_t width = 0, height = 0, cin = 0;
    hipStream_t stream = nullptr;
    hipEvent_t input_copied = nullptr, started = nullptr, done = nullptr;
    float* buf[fgc::kBufCount] = {};
    float* weights[20] = {};
    float* scale[20] = {};  // scale, then shift, in one allocation per layer
    tri_nn_conv_desc desc[20] = {};
    bool submitted = false;   // `done` has been recorded at least once
    bool in_flight = false;   // from a submit until poll or wait has seen it finish
    bool have_output = false;
    float last_ms = 0.0f;
};

namespace {

int gen_fail(int code, const char* who, const std::string& what) {
    return tri_internal_fail(code, (std::string(who) + ": " + what).c_str());
}

void release(tri_framegen* g) {
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (float* p : g->buf)
        if (p) (void)hipFree(p);
    for (int l = 0; l < 20; ++l) {
        if (g->weights[l]) (void)hipFree(g->weights[l]);
        if (g->scale[l]) (void)hipFree(g->scale[l]);
    }
    if (g->input_copied) (void)hipEventDestroy(g->input_copied);
    if (g->started) (void)hipEventDestroy(g->started);
    if (g->done) (void)hipEventDestroy(g->done);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

// The extent of a level: full, half, quarter resolution (the extent is a multiple of 4).
uint32_t level_dim(uint32_t full, int level) { return full >> level; }

int build(tri_framegen* g, const fgc::Model& model) {
    const char* who = "tri_framegen_create";
    if (hipSetDevice(g->device) != hipSuccess) return gen_fail(TRI_E_HIP, who, "hipSetDevice failed");
    // the lowest priority the device has: the job runs behind the frames, whose kernels should not queue behind its blocks
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    if (hipStreamCreateWithPriority(&g->stream, hipStreamNonBlocking, least) != hipSuccess)
        return gen_fail(TRI_E_HIP, who, "stream creation failed");
    if (hipEventCreateWithFlags(&g->input_copied, hipEventDisableTiming) != hipSuccess || hipEventCreate(&g->started) != hipSuccess ||
        hipEventCreate(&g->done) != hipSuccess)
        return gen_fail(TRI_E_HIP, who, "event creation failed");
    for (int b = 0; b < fgc::kBufCount; ++b) {
        const int level = fgc::buffer_level((fgc::Buf)b);
        const size_t floats = (size_t)level_dim(g->width, level) * level_dim(g->height, level) *
                              fgc::buffer_channels((fgc::Buf)b, g->cin);
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&g->buf[b]), floats * sizeof(float));
        if (e != hipSuccess) return tri_hip_fail(e, "tri_framegen_create: activation allocation");
    }
    for (int l = 0; l < 20; ++l) {
        const fgc::LayerPlan& p = fgc::kFgPlan[l];
        const fgc::Layer& L = model.layers[l];
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&g->weights[l]), L.weights.size() * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&g->scale[l]), (size_t)2 * L.cout * sizeof(float));
        if (e != hipSuccess) return tri_hip_fail(e, "tri_framegen_create: weight allocation");
        // on the generator's own stream: ordered before its jobs, and no other stream of the device waits for them
        TRI_HIP_TRY(hipMemcpyAsync(g->weights[l], L.weights.data(), L.weights.size() * sizeof(float), hipMemcpyHostToDevice, g->stream));
        TRI_HIP_TRY(hipMemcpyAsync(g->scale[l], L.scale.data(), (size_t)L.cout * sizeof(float), hipMemcpyHostToDevice, g->stream));
        TRI_HIP_TRY(hipMemcpyAsync(g->scale[l] + L.cout, L.shift.data(), (size_t)L.cout * sizeof(float), hipMemcpyHostToDevice, g->stream));
        tri_nn_conv_desc& d = g->desc[l];
        d.op = p.op == fgc::kConvT4 ? TRI_NN_CONVT4X4 : TRI_NN_CONV3X3;
        d.stride = p.stride;
        d.in_height = level_dim(g->height, p.level);
        d.in_width = level_dim(g->width, p.level);
        d.in_channels = L.cin;
        d.out_channels = L.cout;
        d.activation = p.act;
        d.reserved = 0;
    }
    TRI_HIP_TRY(hipStreamSynchronize(g->stream));  // the model's host arrays are the caller's again
    return TRI_OK;
}

// A device error while a job was in flight: the job is lost. Once the stream has drained nothing of it runs any more,
// so the generator takes the next submit instead of refusing every one with TRI_E_STATE.
int lose_job(tri_framegen* g, hipError_t e, const char* who) {
    (void)hipStreamSynchronize(g->stream);
    g->in_flight = false;
    g->have_output = false;
    return tri_hip_fail(e, who);
}

// The job in flight has finished: its time, and the output is the generator's to hand out.
int complete(tri_framegen* g) {
    float ms = 0.0f;
    const hipError_t e = hipEventElapsedTime(&ms, g->started, g->done);
    if (e != hipSuccess) return lose_job(g, e, "tri_framegen: the job's time");
    g->last_ms = ms;
    g->in_flight = false;
    g->have_output = true;
    return TRI_OK;
}

}  // namespace

int tri_internal_framegen_device(const tri_framegen* g) { return g->device; }
hipEvent_t tri_internal_framegen_done(const tri_framegen* g) { return g->submitted ? g->done : nullptr; }
hipError_t tri_internal_framegen_reader(tri_framegen* g, hipEvent_t read) { return hipStreamWaitEvent(g->stream, read, 0); }

extern "C" {

int tri_framegen_create(int32_t device, const void* weights, uint64_t bytes, uint32_t width, uint32_t height, tri_framegen** out) {
    const char* who = "tri_framegen_create";
    if (!out) return tri_internal_fail(TRI_E_INVALID, "tri_framegen_create: null argument");
    *out = nullptr;
    if (!weights || bytes == 0) return tri_internal_fail(TRI_E_INVALID, "tri_framegen_create: null container");
    if (width < 4 || height < 4 || width > TRI_MAX_DIM || height > TRI_MAX_DIM || (width & 3u) || (height & 3u)) {
        char msg[160];
        snprintf(msg, sizeof msg, "extent %ux%u: width and height must be multiples of 4 within 4..%d", width, height, TRI_MAX_DIM);
        return gen_fail(TRI_E_INVALID, who, msg);
    }
    fgc::Model model;
    std::string err;
    if (!fgc::load(static_cast<const uint8_t*>(weights), (size_t)bytes, model, err)) return gen_fail(TRI_E_INVALID, who, err);
    int dev = 0;
    if (const int rc = tri_resolve_device(device, who, &dev)) return rc;
    tri_framegen* g = new tri_framegen;
    g->device = dev;
    g->width = width;
    g->height = height;
    g->cin = model.input_channels;
    if (const int rc = build(g, model)) {
        release(g);
        return rc;
    }
    *out = g;
    return TRI_OK;
}

int tri_framegen_destroy(tri_framegen* g) {
    if (!g) return TRI_OK;
    release(g);  // waits for a job in flight
    return TRI_OK;
}

int tri_framegen_info(const tri_framegen* g, uint32_t* input_channels, uint32_t* width, uint32_t* height) {
    if (!g) return tri_internal_fail(TRI_E_INVALID, "tri_framegen_info: null generator");
    if (input_channels) *input_channels = g->cin;
    if (width) *width = g->width;
    if (height) *height = g->height;
    return TRI_OK;
}

int tri_framegen_submit(tri_framegen* g, const void* input, void* producer_stream) {
    if (!g || !input) return tri_internal_fail(TRI_E_INVALID, "tri_framegen_submit: null argument");
    if ((uintptr_t)input & 3u) return tri_internal_fail(TRI_E_INVALID, "tri_framegen_submit: the input must be 4-B aligned");
    if (g->in_flight) return tri_internal_fail(TRI_E_STATE, "tri_framegen_submit: a job is in flight (poll or wait for it)");
    TRI_HIP_TRY(hipSetDevice(g->device));
    hipStream_t producer = static_cast<hipStream_t>(producer_stream);
    const size_t bytes = (size_t)g->width * g->height * g->cin * sizeof(float);
    TRI_HIP_TRY(hipMemcpyAsync(g->buf[fgc::X], input, bytes, hipMemcpyDeviceToDevice, producer));
    TRI_HIP_TRY(hipEventRecord(g->input_copied, producer));
    TRI_HIP_TRY(hipStreamWaitEvent(g->stream, g->input_copied, 0));
    hipError_t e = hipEventRecord(g->started, g->stream);
    for (int l = 0; l < 20 && e == hipSuccess; ++l) {
        const fgc::LayerPlan& p = fgc::kFgPlan[l];
        e = tri_launch_nn_conv(g->desc[l], g->buf[p.in], g->weights[l], g->scale[l], g->scale[l] + g->desc[l].out_channels,
                               p.res1 == fgc::NONE ? nullptr : g->buf[p.res1], p.res2 == fgc::NONE ? nullptr : g->buf[p.res2],
                               g->buf[p.out], g->stream);
    }
    if (e == hipSuccess) e = hipEventRecord(g->done, g->stream);
    if (e != hipSuccess) {  // no job: nothing of this submit may still be running on the buffers
        (void)hipStreamSynchronize(g->stream);
        g->have_output = false;
        return tri_hip_fail(e, "tri_framegen_submit");
    }
    g->submitted = true;
    g->in_flight = true;
    g->have_output = false;  // the layers are writing it
    return TRI_OK;
}

int tri_framegen_poll(tri_framegen* g, int32_t* done) {
    if (!g || !done) return tri_internal_fail(TRI_E_INVALID, "tri_framegen_poll: null argument");
    *done = 0;
    if (!g->in_flight) return TRI_OK;
    TRI_HIP_TRY(hipSetDevice(g->device));
    const hipError_t e = hipEventQuery(g->done);
    if (e == hipErrorNotReady) return TRI_OK;
    if (e != hipSuccess) return lose_job(g, e, "tri_framegen_poll");
    if (const int rc = complete(g)) return rc;
    *done = 1;
    return TRI_OK;
}

int tri_framegen_wait(tri_framegen* g) {
    if (!g) return tri_internal_fail(TRI_E_INVALID, "tri_framegen_wait: null generator");
    if (!g->submitted) return tri_internal_fail(TRI_E_STATE, "tri_framegen_wait: nothing was submitted");
    if (!g->in_flight) return TRI_OK;
    TRI_HIP_TRY(hipSetDevice(g->device));
    const hipError_t e = hipEventSynchronize(g->done);
    if (e != hipSuccess) return lose_job(g, e, "tri_framegen_wait");
    return complete(g);
}

int tri_framegen_output(tri_framegen* g, const float** device_hw3) {
    if (!g || !device_hw3) return tri_internal_fail(TRI_E_INVALID, "tri_framegen_output: null argument");
    if (!g->have_output) return tri_internal_fail(TRI_E_STATE, "tri_framegen_output: no finished job (poll or wait first)");
    *device_hw3 = g->buf[fgc::OUT];
    return TRI_OK;
}

int tri_framegen_read_output(tri_framegen* g, float* host_hw3) {
    if (!g || !host_hw3) return tri_internal_fail(TRI_E_INVALID, "tri_framegen_read_output: null argument");
    if (!g->have_output) return tri_internal_fail(TRI_E_STATE, "tri_framegen_read_output: no finished job (poll or wait first)");
    TRI_HIP_TRY(hipSetDevice(g->device));
    TRI_HIP_TRY(hipMemcpy(host_hw3, g->buf[fgc::OUT], (size_t)g->width * g->height * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return TRI_OK;
}

int tri_framegen_last_ms(tri_framegen* g, float* ms) {
    if (!g || !ms) return tri_internal_fail(TRI_E_INVALID, "tri_framegen_last_ms: null argument");
    if (!g->have_output) return tri_internal_fail(TRI_E_STATE, "tri_framegen_last_ms: no finished job (poll or wait first)");
    *ms = g->last_ms;
    return TRI_OK;
}

}  // extern "C"
