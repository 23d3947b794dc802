// tri_geometry.hip — the geometry entry points of the C-ABI (include/tri_raster.h): a context's own geometry and
// the tri_geometry objects several contexts of one device share. What an upload holds is worked out on the host by
// fsel::analyse_geometry (frame_select.h); this unit moves it to the device (Renderer.cpp:1784-2116).
#include "tri_ctx.h"

#include <atomic>

namespace {

template <typename T>
int put(DevBuf<T>& buf, const T* src, size_t n, size_t room) {
    if (const int rc = buf.grow(std::max(n, room))) return rc;
    if (n) TRI_HIP_TRY(hipMemcpy(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return TRI_OK;
}

// UploadMeshFromCache into a geometry object: the caller has made its device current and drained the
// streams that read it.
int geometry_upload(tri_geometry* g, const tri_vertex* v, uint64_t nv, const uint32_t* idx, uint64_t ni,
                    const tri_mesh_range* meshes, uint32_t nm) {
    if ((nv && !v) || (ni && !idx) || (nm && !meshes)) return fail(TRI_E_INVALID, "tri_upload_geometry: null array");
    if (nv * sizeof(TriVsIn) > 0xFFFFFFFFull)  // k_vertex reads the records with 32-bit byte offsets
        return fail(TRI_E_INVALID, "tri_upload_geometry: %llu vertices exceed the 4 GiB vertex-record buffer",
                    (unsigned long long)nv);
    fsel::GeomAnalysis a;
    fsel::Msg msg;
    if (const int rc = fsel::analyse_geometry(v, nv, idx, ni, meshes, nm, a, msg)) return fail(rc, "%s", msg.text);
    int rc;
    if (a.has_skin && (rc = put(g->d_skin, a.skin.data(), nv, 1))) return rc;
    if ((rc = put(g->d_vin, a.vin.data(), nv, 1))) return rc;
    if ((rc = put(g->d_pos, a.pos.data(), 3 * nv, 3))) return rc;
    if ((rc = put(g->d_attr, a.attr.data(), 9 * nv, 9))) return rc;
    if ((rc = put(g->d_idx, idx, ni, 1))) return rc;
    if ((rc = put(g->d_clusters, a.clusters.data(), a.clusters.size(), 1))) return rc;
    if ((rc = put(g->d_vbox, a.vbox.data(), a.vbox.size(), 1))) return rc;
    // null-stream copies are not ordered with the contexts' non-blocking streams: complete them before any
    // context can launch a frame that reads this geometry
    TRI_HIP_TRY(hipStreamSynchronize(nullptr));
    static_cast<fsel::GeomInfo&>(*g) = std::move(a.info);
    g->has_skin_data = a.has_skin;
    g->geometry_set = true;
    // versions come from one process-wide counter: a context that switches between geometry objects
    // (tri_bind_geometry, tri_upload_geometry) can never see an equal version on a different object
    static std::atomic<uint64_t> g_geometry_version{0};
    g->version = ++g_geometry_version;
    return TRI_OK;
}

}  // namespace

int tri_internal_geometry_device(const tri_geometry* g) { return g->device; }

extern "C" {

int tri_upload_geometry(tri_ctx* c, const tri_vertex* v, uint64_t nv, const uint32_t* idx, uint64_t ni,
                        const tri_mesh_range* meshes, uint32_t nm) {
    if (!c) return fail(TRI_E_INVALID, "tri_upload_geometry: null context");
    int rc = make_current(c);
    if (rc) return rc;
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    c->geom = &c->own_geom;
    c->own_geom.device = c->device;
    c->geom_seen = 0;  // re-resolve the draws against the new buffers even if the draw list is unchanged
    c->draws_dirty = true;
    return geometry_upload(&c->own_geom, v, nv, idx, ni, meshes, nm);
}

int tri_geometry_create(int32_t device, tri_geometry** out) {
    if (!out) return fail(TRI_E_INVALID, "tri_geometry_create: null argument");
    *out = nullptr;
    int d = 0;
    if (const int rc = tri_resolve_device(device, "tri_geometry_create", &d)) return rc;
    tri_geometry* g = new tri_geometry();
    g->device = d;
    g->shared = true;
    *out = g;
    return TRI_OK;
}

int tri_geometry_upload(tri_geometry* g, const tri_vertex* v, uint64_t nv, const uint32_t* idx, uint64_t ni,
                        const tri_mesh_range* meshes, uint32_t nm) {
    if (!g) return fail(TRI_E_INVALID, "tri_geometry_upload: null geometry");
    TRI_HIP_TRY(hipSetDevice(g->device));
    TRI_HIP_TRY(hipDeviceSynchronize());  // any context's stream may be reading the old buffers
    return geometry_upload(g, v, nv, idx, ni, meshes, nm);
}

int tri_geometry_destroy(tri_geometry* g) {
    if (!g) return TRI_OK;
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();
    delete g;
    return TRI_OK;
}

int tri_bind_geometry(tri_ctx* c, tri_geometry* g) {
    if (!c) return fail(TRI_E_INVALID, "tri_bind_geometry: null context");
    if (g && g->device != c->device)
        return fail(TRI_E_INVALID, "tri_bind_geometry: geometry on device %d, context on device %d", g->device, c->device);
    int rc = make_current(c);
    if (rc) return rc;
    TRI_HIP_TRY(hipStreamSynchronize(c->stream));
    c->geom = g ? g : &c->own_geom;
    c->geom_seen = 0;
    c->draws_dirty = true;
    return TRI_OK;
}

}  // extern "C"
