// abi_update.hip -- the C ABI, part 3: what changes on a grid that is on the device -- points, permeability and Neumann flags, as
// whole arrays or scattered rows -- and the launch that recomputes the rows they made dirty.
#include <new>

#include "abi_internal.hpp"

using namespace nin;

namespace {

// ---- moving meshes: the geometry made again from new coordinates (grid_update.hip) ---------------------------------------------
// The host mirror of a geometry that was updated on the device: the five arrays come back on first use (HostGrid::ensure), from
// wherever the DeviceGrid holds them at that moment.  Installed by an update when the grid has no fetcher (a grid built on the
// device still has its DeviceMirror, which reads the same buffers); HostGrid::ensure drops it once everything is on the host.
struct GeometryMirror : LazyArrays {
    const DeviceGrid *d;
    explicit GeometryMirror(const DeviceGrid *dg) : d(dg) {}
    template <class T>
    static int get(std::vector<T> &dst, const T *src, size_t n, std::string *err) {
        if (!src) { *err = "the device copy is gone"; return -3; }
        dst.resize(n);
        if (n && hipMemcpy(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) { *err = "hipMemcpy (device to host)"; return -3; }
        return 0;
    }
    int fetch(HostGrid &h, unsigned which, std::string *err) override {
        if (d->device < 0 || hipSetDevice(d->device) != hipSuccess) { *err = "the grid has no device copy"; return -3; }
        const size_t P = (size_t)h.n_points, E = (size_t)h.n_elems, F = (size_t)h.n_faces;
        int rc = 0;
        if (!rc && (which & A_COORDS)) rc = get(h.coords, d->v.coords, P * 3, err);
        if (!rc && (which & A_CENTROIDS)) rc = get(h.centroids, d->v.centroids, E * 3, err);
        if (!rc && (which & A_FCENTERS)) rc = get(h.faces_centers, d->v.face_center, F * 3, err);
        if (!rc && (which & A_NORMALS)) rc = get(h.normal_faces, d->v.face_normal, F * 3, err);
        if (!rc && (which & A_AREAS)) rc = get(h.faces_areas, const_cast<const double *>(d->up_areas), F, err);
        return rc;
    }
};

}  // namespace

// inpoel / etype / inpofa and the face-area array on the device (DeviceGrid::up_*): from the device builder's mirror if it still
// holds them, else uploaded from the host arrays.  Synchronous.  (The coordinate adjoint of abi_apply.hip reads inpofa through it too.)
int nin::ensure_update_inputs(nin_grid *g) {
    DeviceGrid &d = g->d;
    HostGrid &h = g->h;
    if (d.up_inpoel) return NIN_OK;
    LazyArrays::GeometryInputs gi;
    if (h.lazy && h.lazy->lend_geometry_inputs(&gi)) {
        for (void *q : {(void *)gi.inpoel, (void *)gi.etype, (void *)gi.inpofa, (void *)gi.areas}) d.allocs.push_back(q);
        d.up_inpoel = gi.inpoel; d.up_etype = gi.etype; d.up_inpofa = gi.inpofa; d.up_areas = gi.areas;
        d.up_areas_valid = true;   // the builder's own
        return NIN_OK;
    }
    std::string err;
    if (h.ensure(A_INPOEL | A_ETYPE | A_INPOFA, &err)) return fail(NIN_EHIP, "mirroring the connectivity: %s", err.c_str());
    int rc = dev_alloc(d, &d.up_inpoel, h.inpoel.size());
    if (!rc) rc = dev_alloc(d, &d.up_etype, h.etype.size());
    if (!rc) rc = dev_alloc(d, &d.up_inpofa, h.inpofa.size());
    if (!rc) rc = dev_alloc(d, &d.up_areas, (size_t)h.n_faces);
    auto up = [&](void *dst, const void *src, size_t bytes) {
        if (!rc && bytes && hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = fail(NIN_EHIP, "uploading the connectivity failed");
    };
    up(d.up_inpoel, h.inpoel.data(), h.inpoel.size() * 4);
    up(d.up_etype, h.etype.data(), h.etype.size());
    up(d.up_inpofa, h.inpofa.data(), h.inpofa.size() * 4);
    if (rc) { dev_release(d, d.up_inpoel); dev_release(d, d.up_etype); dev_release(d, d.up_inpofa); dev_release(d, d.up_areas); return rc; }
    d.up_areas_valid = false;   // room only: a whole-mesh update writes every area, a local one uploads the host's first
    return NIN_OK;
}

namespace {

// the points per cell of the element types, one byte each (grid_update.hip, fields_scatter.hip)
uint64_t pack_npoel8(const HostGrid &h) {
    uint64_t npoel8 = 0;
    for (int t = 0; t < kNumElementTypes; ++t) npoel8 |= (uint64_t)(h.npoel[t] & 0xff) << (8 * t);
    return npoel8;
}

// The end of a geometry update whose kernels are on `stream` (rc: how enqueueing them went): ev_geom marks it, and host input -- or
// an error -- waits for it.  The host copies of the five arrays are the old mesh's from here on (also after a failure half way):
// fetched again on first use.
int finish_geometry_update(nin_grid *g, int rc, bool on_host, hipStream_t stream, const char *what) {
    DeviceGrid &d = g->d;
    if (!rc && hipEventRecord(static_cast<hipEvent_t>(d.ev_geom), stream) != hipSuccess) rc = fail(NIN_EHIP, "hipEventRecord");
    if (on_host || rc) {
        const hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess && !rc) rc = fail(NIN_EHIP, "%s: %s", what, hipGetErrorString(e));
    }
    g->h.have &= ~A_GEOMETRY;
    if (!g->h.lazy) g->h.lazy.reset(new GeometryMirror(&g->d));
    ++d.geom_updates;
    return rc;
}

// xyz [P][cd] on the host (then stream = the null stream and the call waits) or on the grid's device
int update_points_on_device(nin_grid *g, const double *xyz, bool on_host, int cd, hipStream_t stream) {
    DeviceGrid &d = g->d;
    HostGrid &h = g->h;
    HIP_TRY(hipSetDevice(d.device));
    int rc = ensure_update_inputs(g);
    if (!rc) rc = lazy_event(d.ev_geom);
    if (rc) return rc;
    const size_t P = (size_t)h.n_points;
    double *coords = const_cast<double *>(d.v.coords);
    DevTmp<double> staged;   // (outlives the wait at the end)
    if (on_host && cd == 3) {
        HIP_TRY(hipMemcpy(coords, xyz, P * 24, hipMemcpyHostToDevice));
    } else {
        if (on_host) {
            HIP_TRY(hipMalloc((void **)&staged, P * cd * sizeof(double)));
            if (hipMemcpy(staged, xyz, P * cd * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = fail(NIN_EHIP, "uploading the coordinates failed");
        }
        if (!rc) rc = launch_update_coords(on_host ? staged.p : xyz, cd, (int64_t)P, coords, stream);
    }
    const uint64_t npoel8 = pack_npoel8(h);
    if (!rc)
        rc = launch_update_geometry(d.v, npoel8, d.up_inpoel, d.up_etype, d.up_inpofa, const_cast<double *>(d.v.centroids),
                                    const_cast<double *>(d.v.face_center), const_cast<float *>(d.v.face_normal), d.up_areas, stream);
    if (!rc && d.v.centroids4 && launch_pad_centroids(d.v.centroids, h.n_elems, const_cast<double *>(d.v.centroids4), stream))
        rc = fail(NIN_EHIP, "centroid padding kernel");
    rc = finish_geometry_update(g, rc, on_host, stream, "geometry update");
    d.up_areas_valid = true;
    d.all_dirty = true;   // every row reads the geometry
    return rc;
}

}  // namespace

int nin_grid_update_points(nin_grid *g, const double *xyz, int coords_dim) {
    if (!g || !xyz) return fail(NIN_EINVAL, "NULL argument");
    if (coords_dim != g->coords_dim) return fail(NIN_EINVAL, "coords_dim %d is not the grid's (%d)", coords_dim, g->coords_dim);
    // a grid that holds device arrays (a grid built on the device does before nin_grid_to_device too): the kernels
    if (g->d.device >= 0) return update_points_on_device(g, xyz, true, coords_dim, nullptr);
    try {
        g->h.update_points(xyz, coords_dim);   // host-only: grid_host.cpp's own geometry code again
    } catch (const std::bad_alloc &) {
        return fail(NIN_ENOMEM, "out of host memory while updating the geometry");
    }
    return NIN_OK;
}

int nin_grid_update_points_device(nin_grid *g, const double *dev_xyz, int coords_dim, void *stream) {
    if (!g || !dev_xyz) return fail(NIN_EINVAL, "NULL argument");
    if (coords_dim != g->coords_dim) return fail(NIN_EINVAL, "coords_dim %d is not the grid's (%d)", coords_dim, g->coords_dim);
    if (int rc = on_device(g, " (call nin_grid_to_device first, or nin_grid_update_points with a host array)")) return rc;
    return update_points_on_device(g, dev_xyz, false, coords_dim, static_cast<hipStream_t>(stream));
}

int64_t nin_grid_geometry_updates(const nin_grid *g) { return g ? g->d.geom_updates : 0; }

int nin_fields_set_permeability_device(nin_grid *g, const double *dev_permeability, const double *dev_scale, void *stream) {
    if (!g || !dev_permeability) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = on_device(g, " (call nin_grid_to_device first, or nin_fields_set with host arrays)")) return rc;
    DeviceGrid &d = g->d;
    HIP_TRY(hipSetDevice(d.device));
    const hipError_t e = launch_update_permeability(d.v.n_elems, dev_permeability, dev_scale, const_cast<double *>(d.v.perm),
                                                    const_cast<double *>(d.v.diff_mag), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(NIN_EHIP, "permeability kernel: %s", hipGetErrorString(e));
    d.have_perm = true;
    d.all_dirty = true;
    ++d.field_updates;
    return NIN_OK;
}

int nin_fields_get_permeability(nin_grid *g, double *permeability, double *diff_mag) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    if (int rc = on_device(g, kHintToDevice)) return rc;
    DeviceGrid &d = g->d;
    if (!d.have_perm) return fail(NIN_ESTATE, "no permeability is resident (nin_fields_set or nin_fields_set_permeability_device first)");
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(hipDeviceSynchronize());   // an update may still be in flight on any stream
    const size_t E = (size_t)g->h.n_elems;
    if (permeability) HIP_TRY(hipMemcpy(permeability, d.v.perm, E * 9 * 8, hipMemcpyDeviceToHost));
    if (diff_mag) HIP_TRY(hipMemcpy(diff_mag, d.v.diff_mag, E * 8, hipMemcpyDeviceToHost));
    return NIN_OK;
}

int64_t nin_grid_field_updates(const nin_grid *g) { return g ? g->d.field_updates : 0; }

// ---- local permeability updates (fields_scatter.hip) ---------------------------------------------------------------
// the marks and their header block: state of the grid from the first scatter on (P + 128 bytes)
int nin::ensure_dirty_state(DeviceGrid &d, int64_t P) {
    if (d.dirty) return NIN_OK;
    int rc = dev_alloc(d, &d.dirty, (size_t)P);
    if (!rc) rc = dev_alloc(d, &d.dirty_hdr, (size_t)kDirtyHdrInts);
    if (!rc && (hipMemset(d.dirty, 0, (size_t)P) != hipSuccess || hipMemset(d.dirty_hdr, 0, kDirtyHdrInts * sizeof(int32_t)) != hipSuccess))
        rc = fail(NIN_EHIP, "zeroing the dirty set failed");
    if (rc) { dev_release(d, d.dirty); dev_release(d, d.dirty_hdr); }
    return rc;
}

int nin_fields_scatter_permeability_device(nin_grid *g, const void *dev_cell_ids, int ids_are_int64, int64_t n, const double *dev_permeability,
                                           const double *dev_scale, void *stream) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    if (n < 0) return fail(NIN_EINVAL, "negative n");
    if (int rc = on_device(g, kHintToDevice)) return rc;
    if (n == 0) return NIN_OK;
    if (!dev_cell_ids || !dev_permeability) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (!d.have_perm) return fail(NIN_ESTATE, "no permeability is resident to patch (nin_fields_set or nin_fields_set_permeability_device first)");
    HIP_TRY(hipSetDevice(d.device));
    int rc = ensure_update_inputs(g);   // inpoel / etype on the device: the first call brings them (synchronous), as the first update of the points does
    if (!rc) rc = ensure_dirty_state(d, g->h.n_points);
    if (rc) return rc;
    rc = launch_scatter_permeability(d.v, pack_npoel8(g->h), d.up_inpoel, d.up_etype, dev_cell_ids, ids_are_int64, n, dev_permeability, dev_scale,
                                     d.dirty, d.dirty_hdr + kDirtyHdrRejected, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    d.scattered_cells = true;
    ++d.field_updates;
    return NIN_OK;
}

// ---- Neumann flags from device memory (flags_update.hip) -------------------------------------------------------------
int nin_fields_set_flags_device(nin_grid *g, const void *dev_flags, int flags_are_bytes, void *stream) {
    if (!g || !dev_flags) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = on_device(g, " (call nin_grid_to_device first, or nin_fields_set with host arrays)")) return rc;
    DeviceGrid &d = g->d;
    HIP_TRY(hipSetDevice(d.device));
    int rc = ensure_dirty_state(d, g->h.n_points);
    if (rc) return rc;
    // while everything is dirty no marks are needed; afterwards only the nodes whose byte changes are marked
    rc = launch_set_flags(d.v.n_points, dev_flags, flags_are_bytes, const_cast<uint8_t *>(d.v.flags), d.all_dirty ? nullptr : d.dirty,
                          static_cast<hipStream_t>(stream));
    if (rc) return rc;
    d.fields_set = true;
    d.flags_host_stale = true;
    ++d.flag_updates;
    return NIN_OK;
}

int nin_fields_scatter_flags_device(nin_grid *g, const void *dev_node_ids, int ids_are_int64, int64_t n, const void *dev_flags,
                                    int flags_are_bytes, void *stream) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    if (n < 0) return fail(NIN_EINVAL, "negative n");
    if (int rc = on_device(g, kHintToDevice)) return rc;
    if (n == 0) return NIN_OK;
    if (!dev_node_ids || !dev_flags) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (!d.fields_set) return fail(NIN_ESTATE, "no Neumann flags are resident to patch (nin_fields_set or nin_fields_set_flags_device first)");
    HIP_TRY(hipSetDevice(d.device));
    int rc = ensure_dirty_state(d, g->h.n_points);
    if (rc) return rc;
    rc = launch_scatter_flags(d.v.n_points, dev_node_ids, ids_are_int64, n, dev_flags, flags_are_bytes, const_cast<uint8_t *>(d.v.flags),
                              d.all_dirty ? nullptr : d.dirty, d.dirty_hdr + kDirtyHdrRejected, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    d.scattered_flags = true;
    d.flags_host_stale = true;
    ++d.flag_updates;
    return NIN_OK;
}

// the host's copy of the resident flag bytes (flag_staging), brought up to date; waits for the device when it has to fetch
int nin::fetch_flag_bytes(nin_grid *g) {
    DeviceGrid &d = g->d;
    if (d.flag_staging && !d.flags_host_stale) return NIN_OK;
    const size_t P = (size_t)g->h.n_points;
    if (!d.flag_staging) HIP_TRY(hipHostMalloc((void **)&d.flag_staging, std::max<size_t>(P, 1), hipHostMallocDefault));
    HIP_TRY(hipDeviceSynchronize());   // an update may still be in flight on any stream
    HIP_TRY(hipMemcpy(d.flag_staging, d.v.flags, P, hipMemcpyDeviceToHost));
    d.flags_host_stale = false;
    return NIN_OK;
}

int nin_fields_get_flags(nin_grid *g, uint8_t *neumann) {
    if (!g || !neumann) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = on_device(g, kHintToDevice)) return rc;
    DeviceGrid &d = g->d;
    if (!d.fields_set) return fail(NIN_ESTATE, "no Neumann flags are resident (nin_fields_set or nin_fields_set_flags_device first)");
    HIP_TRY(hipSetDevice(d.device));
    d.flags_host_stale = true;   // host-synchronous by contract: wait for the device and read what is there now
    const int rc = fetch_flag_bytes(g);
    if (rc) return rc;
    const int64_t P = g->h.n_points;
    for (int64_t p = 0; p < P; ++p) neumann[p] = (uint8_t)((d.flag_staging[p] >> 1) & 1);
    return NIN_OK;
}

int64_t nin_grid_flag_updates(const nin_grid *g) { return g ? g->d.flag_updates : 0; }

// ---- local mesh motion (grid_scatter.hip) ---------------------------------------------------------------------------
// ids [n] (int32 / int64) and xyz [n][cd] on the host (then int64 ids, stream = the null stream and the call waits) or on the grid's device
static int scatter_points_on_device(nin_grid *g, const void *ids, int ids_are_int64, int64_t n, const double *xyz, bool on_host, int cd,
                                    hipStream_t stream) {
    DeviceGrid &d = g->d;
    HostGrid &h = g->h;
    HIP_TRY(hipSetDevice(d.device));
    int rc = ensure_update_inputs(g);   // the first call brings the connectivity (synchronous), as the first nin_grid_update_points* does
    if (!rc) rc = ensure_dirty_state(d, h.n_points);
    if (rc) return rc;
    if (!d.up_areas_valid) {
        // the device's face areas are room only (no whole-mesh update wrote them yet): the kernels below write the faces around the
        // moved nodes, the others come from the host, which still holds them (only a geometry update on the device makes them stale)
        std::string err;
        if (h.ensure(A_AREAS, &err)) return fail(NIN_EHIP, "mirroring faces_areas: %s", err.c_str());
        if (h.n_faces > 0) HIP_TRY(hipMemcpy(d.up_areas, h.faces_areas.data(), (size_t)h.n_faces * sizeof(double), hipMemcpyHostToDevice));
        d.up_areas_valid = true;
    }
    if ((rc = lazy_event(d.ev_geom))) return rc;
    DevTmp<void> staged_ids;   // (both outlive the wait at the end)
    DevTmp<double> staged_xyz;
    if (on_host) {
        const size_t ib = (size_t)n * sizeof(int64_t), xb = (size_t)n * cd * sizeof(double);
        HIP_TRY(hipMalloc(&staged_ids, ib));
        if (hipMalloc((void **)&staged_xyz, xb) != hipSuccess) rc = fail(NIN_ENOMEM, "hipMalloc(%zu bytes) for the moved rows", xb);
        if (!rc && (hipMemcpy(staged_ids, ids, ib, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(staged_xyz, xyz, xb, hipMemcpyHostToDevice) != hipSuccess))
            rc = fail(NIN_EHIP, "uploading the moved nodes failed");
        if (rc) return rc;   // nothing was launched: the geometry is as it was
        ids = staged_ids; xyz = staged_xyz;
    }
    rc = launch_scatter_points(d.v, pack_npoel8(h), d.up_inpoel, d.up_etype, d.up_inpofa, ids, ids_are_int64, n, xyz, cd, d.up_areas, d.dirty,
                               d.dirty_hdr + kDirtyHdrRejected, stream);
    d.scattered_nodes = true;
    return finish_geometry_update(g, rc, on_host, stream, "local geometry update");   // all_dirty stays as it is: the kernels marked the rows that can move
}

int nin_grid_scatter_points_device(nin_grid *g, const void *dev_node_ids, int ids_are_int64, int64_t n, const double *dev_xyz, int coords_dim,
                                   void *stream) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    if (n < 0) return fail(NIN_EINVAL, "negative n");
    if (coords_dim != g->coords_dim) return fail(NIN_EINVAL, "coords_dim %d is not the grid's (%d)", coords_dim, g->coords_dim);
    if (int rc = on_device(g, " (call nin_grid_to_device first, or nin_grid_scatter_points with host arrays)")) return rc;
    if (n == 0) return NIN_OK;
    if (!dev_node_ids || !dev_xyz) return fail(NIN_EINVAL, "NULL argument");
    return scatter_points_on_device(g, dev_node_ids, ids_are_int64, n, dev_xyz, false, coords_dim, static_cast<hipStream_t>(stream));
}

int nin_grid_scatter_points(nin_grid *g, const int64_t *node_ids, int64_t n, const double *xyz, int coords_dim) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    if (n < 0) return fail(NIN_EINVAL, "negative n");
    if (coords_dim != g->coords_dim) return fail(NIN_EINVAL, "coords_dim %d is not the grid's (%d)", coords_dim, g->coords_dim);
    if (n == 0) return NIN_OK;
    if (!node_ids || !xyz) return fail(NIN_EINVAL, "NULL argument");
    HostGrid &h = g->h;
    int64_t bad = 0, first = 0;
    for (int64_t i = 0; i < n; ++i)
        if (node_ids[i] < 0 || node_ids[i] >= h.n_points) { if (!bad++) first = node_ids[i]; }
    if (bad) return fail(NIN_EINVAL, "%lld of %lld node ids lie outside [0, %lld) (the first: %lld); nothing was moved", (long long)bad, (long long)n,
                         (long long)h.n_points, (long long)first);
    // a grid that holds device arrays (a grid built on the device does before nin_grid_to_device too): the kernels
    if (g->d.device >= 0) return scatter_points_on_device(g, node_ids, 1, n, xyz, true, coords_dim, nullptr);
    try {   // host-only: the coordinates patched, then grid_host.cpp's own geometry code over the whole mesh (no dirty set without a device)
        for (int64_t i = 0; i < n; ++i)
            for (int k = 0; k < coords_dim && k < 3; ++k) h.coords[(size_t)node_ids[i] * 3 + k] = xyz[i * coords_dim + k];
        const std::vector<double> moved(h.coords);
        h.update_points(moved.data(), 3);
    } catch (const std::bad_alloc &) {
        return fail(NIN_ENOMEM, "out of host memory while updating the geometry");
    }
    return NIN_OK;
}

// ---- marks without an update (jacobian_dirty.hip) -------------------------------------------------------------------
int nin_grid_mark_dirty_device(nin_grid *g, const void *dev_ids, int ids_are_int64, int64_t n, int ids_are_cells, void *stream) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    if (n < 0) return fail(NIN_EINVAL, "negative n");
    if (int rc = on_device(g, kHintToDevice)) return rc;
    if (n == 0) return NIN_OK;
    if (!dev_ids) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    HIP_TRY(hipSetDevice(d.device));
    int rc = ids_are_cells ? ensure_update_inputs(g) : NIN_OK;   // inpoel / etype on the device: the first call brings them (synchronous)
    if (!rc) rc = ensure_dirty_state(d, g->h.n_points);
    if (rc) return rc;
    rc = launch_mark_dirty(d.v, pack_npoel8(g->h), d.up_inpoel, d.up_etype, dev_ids, ids_are_int64, n, ids_are_cells, d.dirty,
                           d.dirty_hdr + kDirtyHdrRejected, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    d.scattered_marks = true;
    return NIN_OK;
}

// Ids were refused by a scatter since the last dirty launch: the counter starts again from zero, and the error says how many and whose
// they can have been (nin_weights_dirty_device, and the dirty relinearisations of abi_jacobian_dirty.hip)
int nin::dirty_ids_refused(nin_grid *g, int32_t count, hipStream_t stream) {
    DeviceGrid &d = g->d;
    HIP_TRY(hipMemsetAsync(d.dirty_hdr + kDirtyHdrRejected, 0, sizeof(int32_t), stream));
    // one counter for the scatters: what was called since the last dirty launch says whose ids they can be (nin_grid_mark_dirty_device
    // takes cells or nodes)
    const bool nodes = d.scattered_nodes || d.scattered_marks, flags = d.scattered_flags,
               cells = d.scattered_cells || d.scattered_marks || !(nodes || flags);
    d.scattered_cells = d.scattered_nodes = d.scattered_flags = d.scattered_marks = false;
    char who[240];
    if (cells && (nodes || flags))
        snprintf(who, sizeof who, "cell ids outside [0, %lld) or node ids outside [0, %lld) were given to the local updates%s",
                 (long long)g->h.n_elems, (long long)g->h.n_points, flags ? " (nin_fields_scatter_flags_device among them)" : "");
    else if (nodes && flags)
        snprintf(who, sizeof who, "node ids outside [0, %lld) were given to nin_grid_scatter_points_device or nin_fields_scatter_flags_device",
                 (long long)g->h.n_points);
    else if (flags)
        snprintf(who, sizeof who, "node ids outside [0, %lld) were given to nin_fields_scatter_flags_device", (long long)g->h.n_points);
    else if (nodes)
        snprintf(who, sizeof who, "node ids outside [0, %lld) were given to nin_grid_scatter_points_device", (long long)g->h.n_points);
    else
        snprintf(who, sizeof who, "cell ids outside [0, %lld) were given to nin_fields_scatter_permeability_device", (long long)g->h.n_elems);
    return fail(NIN_EINVAL, "%d %s and written nowhere; nothing was launched, the dirty set is kept", (int)count, who);
}

int nin_weights_dirty_device(nin_grid *g, int method, int add_neumann, double *dev_csr_data, double *dev_neumann_ws, void *stream_, int clear,
                             int64_t *n_recomputed) {
    if (n_recomputed) *n_recomputed = 0;
    if (!g || !dev_csr_data || !dev_neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    int rc = on_device(g, kHintWeights);
    if (!rc) rc = weights_ready(d, method);
    if (rc) return rc;
    const bool gls = method == NIN_METHOD_GLS;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(d.device));
    const int32_t P = (int32_t)g->h.n_points;
    int32_t hdr[kDirtyHdrInts] = {0};
    DirtyLaps laps(stream);   // NIN_TIMING=1: the call's three phases on stderr
    laps.mark(0);
    if (d.dirty) {   // (no scatter yet: no marks, no refused ids)
        if (!d.all_dirty) {
            const size_t ints = 2 * dirty_compact_hist_ints(P);   // the histogram and its scan
            size_t tmp_bytes = 0;
            if (dirty_compact_tmp_bytes(P, &tmp_bytes)) return fail(NIN_EHIP, "sizing the scan of the dirty set failed");
            // both sized by the mesh alone: allocated by the first dirty launch (and again after nin_grid_release_scratch)
            if (!d.dirty_hist && (rc = dev_alloc(d, &d.dirty_hist, ints))) return rc;
            if (!d.dirty_lists && (rc = dev_alloc(d, &d.dirty_lists, (size_t)P))) return rc;
            if ((rc = grow(d, reinterpret_cast<char **>(&d.dirty_tmp), &d.dirty_tmp_bytes, std::max<size_t>(tmp_bytes, 16)))) return rc;
            if ((rc = launch_dirty_compact(P, gls ? 0 : 1, clear, d.dirty, d.node_class, d.dirty_hdr + kDirtyHdrRejected, d.dirty_hist,
                                           d.dirty_hist + ints / 2, d.dirty_tmp, d.dirty_tmp_bytes, d.dirty_lists, d.dirty_hdr, stream)))
                return rc;
        }
        // the one synchronisation of the call: the lists' offsets and the refused-id counter, 128 bytes
        HIP_TRY(hipMemcpyAsync(hdr, d.dirty_hdr, sizeof hdr, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (hdr[kDirtyHdrRejected] != 0) return dirty_ids_refused(g, hdr[kDirtyHdrRejected], stream);   // the marks are as they were (the fill pass clears nothing while the counter is set)
        d.scattered_cells = d.scattered_nodes = d.scattered_flags = d.scattered_marks = false;
    }
    if (d.all_dirty) {   // the ordinary full launch
        if ((rc = nin_weights_device(g, method, nullptr, 0, add_neumann, dev_csr_data, dev_neumann_ws, stream_))) return rc;
        if (clear) {
            if (d.dirty) HIP_TRY(hipMemsetAsync(d.dirty, 0, (size_t)P, stream));
            d.all_dirty = false;
        }
        if (n_recomputed) *n_recomputed = P;
        return NIN_OK;
    }
    const int32_t *off = hdr + kDirtyHdrOffsets;
    const int32_t total = off[kGlsPlanKernels];
    if (total < 0 || total > P) return fail(NIN_EHIP, "the dirty set's lists hold %d nodes of %d", (int)total, (int)P);
    if (n_recomputed) *n_recomputed = total;
    if (total == 0) return NIN_OK;
    size_t desc_first[kGlsPlanKernels], words = 0;
    for (int k = 0; gls && k < kGlsPlanKernels; ++k) {   // (IDW / LS: one list, no descriptors)
        if (off[k + 1] < off[k]) return fail(NIN_EHIP, "the dirty set's lists are out of order");
        desc_first[k] = words = desc_align(words);
        words += (size_t)(off[k + 1] - off[k]) * (size_t)gls_plan_row(k).desc_words;
    }
    if (words > d.dirty_desc_words && (rc = grow(d, &d.dirty_desc, &d.dirty_desc_words, words + words / 2))) return rc;
    if ((rc = launch_lists(d, method, d.dirty_lists, off, d.dirty_desc, desc_first, add_neumann, dev_csr_data, dev_neumann_ws, stream, &laps)))
        return rc;
    laps.report(total);
    return NIN_OK;
}

int64_t nin_grid_dirty_nodes(nin_grid *g) {
    if (!g || g->d.device < 0 || g->d.prebuilt) return 0;
    DeviceGrid &d = g->d;
    if (d.all_dirty) return -1;
    if (!d.dirty) return 0;
    int32_t n = 0;
    const int rc = [&]() -> int {
        HIP_TRY(hipSetDevice(d.device));
        HIP_TRY(hipDeviceSynchronize());   // a scatter may be in flight on any stream
        HIP_TRY(hipMemset(d.dirty_hdr + kDirtyHdrCount, 0, sizeof(int32_t)));
        if (int rc = launch_dirty_count((int32_t)g->h.n_points, d.dirty, d.dirty_hdr + kDirtyHdrCount, nullptr)) return rc;
        HIP_TRY(hipMemcpy(&n, d.dirty_hdr + kDirtyHdrCount, sizeof n, hipMemcpyDeviceToHost));
        return NIN_OK;
    }();
    return rc ? -2 : n;
}

int nin_grid_dirty_reset(nin_grid *g, int all_dirty, void *stream) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintToDevice)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    if (!all_dirty && d.dirty) {   // the marks and the refused-id counter
        HIP_TRY(hipMemsetAsync(d.dirty, 0, (size_t)g->h.n_points, static_cast<hipStream_t>(stream)));
        HIP_TRY(hipMemsetAsync(d.dirty_hdr + kDirtyHdrRejected, 0, sizeof(int32_t), static_cast<hipStream_t>(stream)));
    }
    d.all_dirty = all_dirty != 0;
    return NIN_OK;
}
