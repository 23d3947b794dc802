// capi_util.h — what the host translation units of the C-ABI (include/tri_raster.h) share: the error helper, the
// device and argument checks of the entry points, and the accessors into a context. Host only: no kernel launcher is
// declared here (raster_launch.h), and no RCCL type (tri_group.hip and tri_xfer.hip keep their own ncclResult_t pair).
// The functions are defined in tri_raster_capi.hip, next to the thread's error string; an accessor into a geometry or a
// font in the unit that owns the object (tri_geometry.hip, tri_resources.hip). The objects themselves: tri_ctx.h.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/tri_raster.h"

// Record an error message for tri_last_error (returns `code`).
int tri_internal_fail(int code, const char* msg);
// Record "<what>: <hipGetErrorString(e)>"; returns TRI_E_OOM for hipErrorOutOfMemory, TRI_E_HIP for every other error.
int tri_hip_fail(hipError_t e, const char* what);

// Return tri_hip_fail from the enclosing function when a HIP call fails (one compare on the success path: tri_render
// goes through it about ten times a frame).
#define TRI_HIP_TRY(expr)                                     \
    do {                                                      \
        const hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return tri_hip_fail(_e, #expr); \
    } while (0)

// The device a create call runs on: `requested`, or the current device when it is negative. TRI_E_HIP with
// "<who>: no HIP device available" on a host without one, TRI_E_INVALID for an ordinal at or past the count. Entry
// points call it after their own argument checks (a bad argument is TRI_E_INVALID on every host) and before they
// allocate anything.
int tri_resolve_device(int32_t requested, const char* who, int* device);

// TRI_E_INVALID unless 1 <= w, h <= TRI_MAX_DIM; `what` names the extent in the message ("framebuffer", "atlas").
int tri_check_extent(const char* who, uint32_t w, uint32_t h, const char* what = "extent");
// The source of a conversion: non-null, 4-B aligned, w x h within 1..TRI_MAX_DIM, pitch a multiple of 4 and at least w * 4.
int tri_check_bgra_source(const char* who, const void* bgra, uint32_t w, uint32_t h, uint32_t pitch_bytes);

// A context's stream and device.
hipStream_t tri_internal_stream(tri_ctx* ctx);
int tri_internal_device(tri_ctx* ctx);
// Whether the context renders every row of its frame (false: a row band).
bool tri_internal_whole_frame(tri_ctx* ctx);
// The device a geometry object or a font lives on; the UNORM8 decode table (b / 255) on a context's device.
int tri_internal_geometry_device(const tri_geometry* geometry);
int tri_internal_font_device(const tri_font* font);
const float* tri_internal_unorm_lut(tri_ctx* ctx);
