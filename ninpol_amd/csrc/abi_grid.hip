// abi_grid.hip -- the C ABI of include/ninpol_amd.h, part 1: the error text, the grid's lifetime, its arrays and its fields; what the
// other parts share with it (abi_internal.hpp).
#include <cstdarg>
#include <cstring>
#include <new>

#include "abi_internal.hpp"

using namespace nin;

static thread_local std::string g_err;

namespace nin {

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int on_device(const nin_grid *g, const char *hint, bool plan) {
    if (g->d.device < 0 || (plan && g->d.prebuilt)) return fail(NIN_ENODEVICE, "grid is not on a device%s", hint);
    return NIN_OK;
}

int weights_ready(const DeviceGrid &d, int method, bool size) {
    if (!d.fields_set) return fail(NIN_ESTATE, "nin_fields_set has not been called");
    if (method != NIN_METHOD_GLS && method != NIN_METHOD_IDW && method != NIN_METHOD_LS) return fail(NIN_EINVAL, "unknown method %d", method);
    if (method == NIN_METHOD_GLS && !d.have_perm) return fail(NIN_ESTATE, "GLS needs permeability and diff_mag");
    if (size && method == NIN_METHOD_GLS && d.gls_too_large)
        return fail(NIN_ERANGE, "a node's GLS system has more than 1024 rows (more than ~100 cells around one node): beyond the fallback kernel");
    return NIN_OK;
}

}  // namespace nin

namespace {

void dev_free_all(DeviceGrid &d) {
    if (d.device >= 0) (void)hipSetDevice(d.device);
    if (d.flag_staging) (void)hipHostFree(d.flag_staging);
    if (d.ev_weights) (void)hipEventDestroy(static_cast<hipEvent_t>(d.ev_weights));
    if (d.ev_scan) (void)hipEventDestroy(static_cast<hipEvent_t>(d.ev_scan));
    if (d.ev_geom) (void)hipEventDestroy(static_cast<hipEvent_t>(d.ev_geom));
    if (d.copy_stream) (void)hipStreamDestroy(static_cast<hipStream_t>(d.copy_stream));
    if (d.copy_stream2) (void)hipStreamDestroy(static_cast<hipStream_t>(d.copy_stream2));
    if (d.ev_fork) (void)hipEventDestroy(static_cast<hipEvent_t>(d.ev_fork));
    if (d.ev_join) (void)hipEventDestroy(static_cast<hipEvent_t>(d.ev_join));
    if (d.side_stream) (void)hipStreamDestroy(static_cast<hipStream_t>(d.side_stream));
    for (void *p : d.allocs) (void)hipFree(p);
    d.allocs.clear();
    d = DeviceGrid{};
}

struct ArrayRef {
    int dtype;      // NIN_I64 / NIN_F64
    int64_t count;
    int kind;       // source element type: 0 int32, 1 int64, 2 uint8, 3 int8, 4 double, 5 float
    const void *ptr;
};

unsigned array_bits(const std::string &name) {
    if (name == "esup") return A_ESUP;
    if (name == "esup_ptr") return A_ESUP_PTR;
    if (name == "fsup") return A_FSUP;
    if (name == "fsup_ptr") return A_FSUP_PTR;
    if (name == "esuf" || name == "esuf_ptr") return A_ESUF;
    if (name == "esuel") return A_ESUEL;
    if (name == "infael") return A_INFAEL;
    if (name == "inpofa") return A_INPOFA;
    if (name == "inpoel") return A_INPOEL;
    if (name == "boundary_faces") return A_BFACES;
    if (name == "boundary_points") return A_BPOINTS;
    if (name == "element_types") return A_ETYPE;
    if (name == "point_coords") return A_COORDS;
    if (name == "centroids") return A_CENTROIDS;
    if (name == "faces_centers") return A_FCENTERS;
    if (name == "faces_areas") return A_AREAS;
    if (name == "normal_faces") return A_NORMALS;
    return 0;   // psup / edges: their builders ask for what they read
}

bool lookup_array(nin_grid *g, const std::string &name, ArrayRef *r) {
    HostGrid &h = g->h;
    if ((array_bits(name) & A_GEOMETRY & ~h.have) && g->d.ev_geom) {   // geometry updated on the device: wait for the last update first
        if (hipSetDevice(g->d.device) != hipSuccess || hipEventSynchronize(static_cast<hipEvent_t>(g->d.ev_geom)) != hipSuccess) return false;
    }
    if (h.ensure(array_bits(name))) return false;   // a grid built on the device: bring the array over first
    auto I32 = [&](const std::vector<int32_t> &v) { *r = {NIN_I64, (int64_t)v.size(), 0, v.data()}; return true; };
    auto I64 = [&](const std::vector<int64_t> &v) { *r = {NIN_I64, (int64_t)v.size(), 1, v.data()}; return true; };
    auto U8 = [&](const std::vector<uint8_t> &v) { *r = {NIN_I64, (int64_t)v.size(), 2, v.data()}; return true; };
    auto F64 = [&](const std::vector<double> &v) { *r = {NIN_F64, (int64_t)v.size(), 4, v.data()}; return true; };
    if (name == "esup") return I32(h.esup);
    if (name == "esup_ptr") return I64(h.esup_ptr);
    if (name == "fsup") return I32(h.fsup);
    if (name == "fsup_ptr") return I64(h.fsup_ptr);
    if (name == "esuf") return I32(h.esuf);
    if (name == "esuf_ptr") return I64(h.esuf_ptr);
    if (name == "esuel") return I32(h.esuel);
    if (name == "infael") return I32(h.infael);
    if (name == "inpofa") return I32(h.inpofa);
    if (name == "inpoel") return I32(h.inpoel);
    if (name == "boundary_faces") return U8(h.boundary_faces);
    if (name == "boundary_points") return U8(h.boundary_points);
    if (name == "element_types") { *r = {NIN_I64, (int64_t)h.etype.size(), 3, h.etype.data()}; return true; }
    if (name == "psup" || name == "psup_ptr") {
        h.build_psup();
        return name == "psup" ? I32(h.psup) : I64(h.psup_ptr);
    }
    if (name == "inedel" || name == "inpoed") {
        if (!h.build_edges) { *r = {NIN_I64, 0, 0, nullptr}; return true; }  // empty, like the reference's (0,0) arrays
        h.build_inedel();
        return name == "inedel" ? I32(h.inedel) : I32(h.inpoed);
    }
    if (name == "point_coords") return F64(h.coords);
    if (name == "centroids") return F64(h.centroids);
    if (name == "faces_centers") return F64(h.faces_centers);
    if (name == "faces_areas") return F64(h.faces_areas);
    if (name == "normal_faces") { *r = {NIN_F64, (int64_t)h.normal_faces.size(), 5, h.normal_faces.data()}; return true; }
    return false;
}

}  // namespace

const char *nin_last_error(void) { return g_err.c_str(); }
const char *nin_version(void) { return "ninpol_amd 0.1 (gfx950)"; }

static int grid_create_common(int64_t dim, int64_t n_elems, int64_t n_points, const int64_t *npoel, const int64_t *nfael,
                              const int64_t *lnofa, const int64_t *lpofa, const int64_t *nedel, const int64_t *lpoed,
                              const int64_t *connectivity, const int64_t *element_types, const double *coords,
                              int coords_dim, int build_edges, int num_threads, int device, nin_grid **out) {
    if (!out) return fail(NIN_EINVAL, "out is NULL");
    *out = nullptr;
    // the three checks of grid.pyx:55-60 (the Python layer turns them into the reference's ValueErrors)
    if (dim < 1) return fail(NIN_EINVAL, "The number of dimensions must be greater than 0.");
    if (n_elems < 1) return fail(NIN_EINVAL, "The number of elements must be greater than 0.");
    if (n_points < 1) return fail(NIN_EINVAL, "The number of points must be greater than 0.");
    if (!npoel || !nfael || !lnofa || !lpofa || !nedel || !lpoed || !connectivity || !element_types || !coords)
        return fail(NIN_EINVAL, "NULL table or array");
    if (coords_dim < 1 || coords_dim > 3) return fail(NIN_EINVAL, "coords_dim must be 1..3");
    if (n_elems * 8 >= INT32_MAX || n_points >= INT32_MAX) return fail(NIN_ERANGE, "mesh too large for the int32 layout");
    if (device >= 0) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            return fail(NIN_ENODEVICE, "no HIP device visible: the device grid build has no CPU fallback (use nin_grid_create)");
        if (device >= ndev) return fail(NIN_EINVAL, "device %d out of range (%d visible)", device, ndev);
    }
    nin_grid *g = new (std::nothrow) nin_grid();
    if (!g) return fail(NIN_ENOMEM, "out of host memory");
    HostGrid &h = g->h;
    h.dim = dim; h.n_elems = n_elems; h.n_points = n_points;
    h.build_edges = build_edges; h.num_threads = num_threads;
    g->coords_dim = coords_dim;
    for (int t = 0; t < kNumElementTypes; ++t) {
        h.npoel[t] = (int32_t)npoel[t]; h.nfael[t] = (int32_t)nfael[t]; h.nedel[t] = (int32_t)nedel[t];
        for (int f = 0; f < kMaxFacesPerElement; ++f) {
            h.lnofa[t][f] = (int32_t)lnofa[t * kMaxFacesPerElement + f];
            for (int k = 0; k < kMaxPointsPerFace; ++k)
                h.lpofa[t][f][k] = (int32_t)lpofa[(t * kMaxFacesPerElement + f) * kMaxPointsPerFace + k];
        }
        for (int e = 0; e < kMaxEdgesPerElement; ++e)
            for (int k = 0; k < 2; ++k) h.lpoed[t][e][k] = (int32_t)lpoed[(t * kMaxEdgesPerElement + e) * 2 + k];
    }
    int rc;
    std::string err;
    try {
        if (device >= 0) rc = build_grid_on_device(h, g->d, device, connectivity, element_types, coords, coords_dim, &err);
        else rc = h.build(connectivity, element_types, coords, coords_dim);
    } catch (const std::bad_alloc &) {
        dev_free_all(g->d);
        delete g;
        return fail(NIN_ENOMEM, "out of host memory while building the grid");
    }
    if (rc) { dev_free_all(g->d); delete g; }
    if (rc == -5) return fail(NIN_ERANGE, "a connectivity count does not fit int32");
    if (rc == -2) return fail(NIN_ENOMEM, "device grid build: %s", err.c_str());
    if (rc == -3) return fail(NIN_EHIP, "device grid build: %s", err.c_str());
    if (rc) return fail(NIN_EINVAL, "connectivity references a point outside [0, n_points) or an unknown element type");
    *out = g;
    return NIN_OK;
}

int nin_grid_create(int64_t dim, int64_t n_elems, int64_t n_points, const int64_t *npoel, const int64_t *nfael,
                    const int64_t *lnofa, const int64_t *lpofa, const int64_t *nedel, const int64_t *lpoed,
                    const int64_t *connectivity, const int64_t *element_types, const double *coords, int coords_dim,
                    int build_edges, int num_threads, nin_grid **out) {
    return grid_create_common(dim, n_elems, n_points, npoel, nfael, lnofa, lpofa, nedel, lpoed, connectivity, element_types,
                              coords, coords_dim, build_edges, num_threads, -1, out);
}

int nin_grid_create_on_device(int64_t dim, int64_t n_elems, int64_t n_points, const int64_t *npoel, const int64_t *nfael,
                              const int64_t *lnofa, const int64_t *lpofa, const int64_t *nedel, const int64_t *lpoed,
                              const int64_t *connectivity, const int64_t *element_types, const double *coords,
                              int coords_dim, int build_edges, int device, nin_grid **out) {
    if (device < 0) return fail(NIN_EINVAL, "device must be >= 0");
    return grid_create_common(dim, n_elems, n_points, npoel, nfael, lnofa, lpofa, nedel, lpoed, connectivity, element_types,
                              coords, coords_dim, build_edges, 0, device, out);
}

void nin_grid_destroy(nin_grid *g) {
    if (!g) return;
    dev_free_all(g->d);
    delete g;
}

int64_t nin_grid_scalar(const nin_grid *g, const char *name) {
    if (!g || !name) return -1;
    const HostGrid &h = g->h;
    const std::string n(name);
    if (n == "dim") return h.dim;
    if (n == "n_elems") return h.n_elems;
    if (n == "n_points") return h.n_points;
    if (n == "n_faces") return h.n_faces;
    if (n == "n_edges") { if (h.build_edges) const_cast<HostGrid &>(h).build_inedel(); return h.n_edges; }
    if (n == "MX_ELEMENTS_PER_POINT") return h.mx_elems_per_point;
    if (n == "MX_POINTS_PER_POINT") { const_cast<HostGrid &>(h).build_psup(); return h.mx_points_per_point; }
    if (n == "MX_ELEMENTS_PER_FACE") return h.mx_elems_per_face;
    if (n == "MX_FACES_PER_POINT") return h.mx_faces_per_point;
    if (n == "coords_dim") return g->coords_dim;
    if (n == "nnz_esup") return h.nnz_esup;
    if (n == "nnz_fsup") return h.nnz_fsup;
    if (n == "gls_adjoint_contrib_bytes") return g->d.adj_contrib ? std::max<int64_t>(g->d.nnz_e, 1) * 80 : 0;
    if (n == "gls_shape_contrib_bytes")
        return g->d.shape_cell ? std::max<int64_t>(g->d.nnz_e, 1) * 24 + std::max<int64_t>(g->d.nnz_f, 1) * 48 + std::max<int64_t>(g->d.v.n_faces, 1) * 96 : 0;
    if (n == "gls_shape_tangent_bytes")
        return g->d.shape_tan_cell ? (int64_t)g->d.shape_tan_n * (std::max<int64_t>(h.n_elems, 1) * 24 + std::max<int64_t>(g->d.v.n_faces, 1) * 48) : 0;
    return -1;
}

int nin_grid_array_info(nin_grid *g, const char *name, int64_t *count, int *dtype) {
    if (!g || !name || !count || !dtype) return fail(NIN_EINVAL, "NULL argument");
    ArrayRef r;
    if (!lookup_array(g, name, &r)) return fail(NIN_EINVAL, "unknown grid array '%s'", name);
    *count = r.count;
    *dtype = r.dtype;
    return NIN_OK;
}

int nin_grid_array_copy(nin_grid *g, const char *name, void *dst, int64_t count) {
    if (!g || !name || (!dst && count)) return fail(NIN_EINVAL, "NULL argument");
    ArrayRef r;
    if (!lookup_array(g, name, &r)) return fail(NIN_EINVAL, "unknown grid array '%s'", name);
    if (count != r.count) return fail(NIN_EINVAL, "array '%s' has %lld elements, caller gave room for %lld", name, (long long)r.count, (long long)count);
    const int64_t n = r.count;
    switch (r.kind) {
        case 0: { auto s = (const int32_t *)r.ptr; auto d = (int64_t *)dst;
#pragma omp parallel for schedule(static)
                  for (int64_t i = 0; i < n; ++i) d[i] = s[i]; } break;
        case 1: if (n) memcpy(dst, r.ptr, (size_t)n * 8); break;
        case 2: { auto s = (const uint8_t *)r.ptr; auto d = (int64_t *)dst; for (int64_t i = 0; i < n; ++i) d[i] = s[i]; } break;
        case 3: { auto s = (const int8_t *)r.ptr; auto d = (int64_t *)dst; for (int64_t i = 0; i < n; ++i) d[i] = s[i]; } break;
        case 4: if (n) memcpy(dst, r.ptr, (size_t)n * 8); break;
        case 5: { auto s = (const float *)r.ptr; auto d = (double *)dst; for (int64_t i = 0; i < n; ++i) d[i] = (double)s[i]; } break;
    }
    return NIN_OK;
}

int nin_device_count(int *count) {
    if (!count) return fail(NIN_EINVAL, "NULL argument");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; return fail(NIN_ENODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = c;
    return NIN_OK;
}

// a grid built on the device holds its arrays there but has no launch plan yet: not "on the device" until to_device
int nin_grid_device(const nin_grid *g) { return (g && !g->d.prebuilt) ? g->d.device : -1; }

int nin_grid_to_device(nin_grid *g, int device) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(NIN_ENODEVICE, "no HIP device visible: libninpol_amd has no CPU fallback for the weight kernels");
    if (device < 0 || device >= ndev) return fail(NIN_EINVAL, "device %d out of range (%d visible)", device, ndev);
    const bool adopt = g->d.prebuilt && g->d.device == device;   // built on this device: the arrays are already there
    HostGrid &h = g->h;
    if (!adopt) {
        if (g->d.ev_geom) (void)hipEventSynchronize(static_cast<hipEvent_t>(g->d.ev_geom));   // (a geometry update still in flight)
        std::string err;   // a device-built grid moving elsewhere: everything comes to the host before its HBM copy goes
        if (h.ensure(A_ALL, &err)) return fail(NIN_EHIP, "mirroring the device-built grid: %s", err.c_str());
        dev_free_all(g->d);
    }
    HIP_TRY(hipSetDevice(device));
    DeviceGrid &d = g->d;
    d.device = device;
    d.prebuilt = false;
    const int64_t P = h.n_points, E = h.n_elems, F = h.n_faces;
    d.nnz_e = h.nnz_esup;
    d.nnz_f = h.nnz_fsup;
    GridView &v = d.v;
    v.n_points = (int32_t)P; v.n_elems = (int32_t)E; v.n_faces = (int32_t)F; v.dim = (int32_t)h.dim;
    int rc;
    if (!adopt) {
    {
        std::vector<int32_t> p32((size_t)P + 1);
        for (int64_t i = 0; i <= P; ++i) p32[i] = (int32_t)h.esup_ptr[i];
        if ((rc = dev_upload(d, &v.esup_ptr, p32))) return rc;
        for (int64_t i = 0; i <= P; ++i) p32[i] = (int32_t)h.fsup_ptr[i];
        if ((rc = dev_upload(d, &v.fsup_ptr, p32))) return rc;
    }
    if ((rc = dev_upload(d, &v.esup, h.esup))) return rc;
    if ((rc = dev_upload(d, &v.fsup, h.fsup))) return rc;
    if ((rc = dev_upload(d, &v.coords, h.coords))) return rc;
    if ((rc = dev_upload(d, &v.centroids, h.centroids))) return rc;
    if ((rc = dev_upload(d, &v.face_center, h.faces_centers))) return rc;
    if ((rc = dev_upload(d, &v.face_normal, h.normal_faces))) return rc;
    {
        std::vector<int32_t> fc((size_t)F * 2);
#pragma omp parallel for schedule(static)
        for (int64_t f = 0; f < F; ++f) {
            const int64_t b = h.esuf_ptr[f], n = h.esuf_ptr[f + 1] - b;
            fc[2 * f] = h.esuf[b];
            fc[2 * f + 1] = n > 1 ? h.esuf[b + 1] : -1;
        }
        if ((rc = dev_upload(d, &v.face_cells, fc))) return rc;
    }
    }
    {   // flags start as "boundary only"; nin_fields_set adds the Neumann bit
        uint8_t *fl = nullptr;
        if ((rc = dev_alloc(d, &fl, (size_t)P))) return rc;
        if (h.ensure(A_BPOINTS)) return fail(NIN_EHIP, "mirroring boundary_points failed");
        HIP_TRY(hipMemcpy(fl, h.boundary_points.data(), (size_t)P, hipMemcpyHostToDevice));
        v.flags = fl;
        double *perm = nullptr, *dm = nullptr;
        if ((rc = dev_alloc(d, &perm, (size_t)E * 9))) return rc;
        if ((rc = dev_alloc(d, &dm, (size_t)E))) return rc;
        v.perm = perm; v.diff_mag = dm;
    }
    v.centroids4 = nullptr;
    if (getenv("NIN_ROWS_PAD4") != nullptr) {   // experiment: (x, y, z, 0) per cell, a centroid in two 16-byte loads -- 3 % SLOWER than the packed array
        double *c4 = nullptr;
        if ((rc = dev_alloc(d, &c4, (size_t)E * 4))) return rc;
        if (launch_pad_centroids(v.centroids, E, c4, nullptr)) return fail(NIN_EHIP, "centroid padding kernel");
        v.centroids4 = c4;
    }
    if ((rc = build_gls_plan(g))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return NIN_OK;
}

int nin_fields_set(nin_grid *g, const double *permeability, const double *diff_mag, const double *neumann_flag,
                   const double *neumann_val) {
    (void)neumann_val;  // only feeds the Neumann RHS column, which gls.pyx:464-472 never reads back
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    if (int rc = on_device(g, kHintToDevice)) return rc;
    if (g->h.ensure(A_BPOINTS)) return fail(NIN_EHIP, "mirroring boundary_points failed");
    // NULL keeps the flags that are resident (nin_fields_set_flags_device put them there, or an earlier call), as a NULL permeability keeps the table
    if (!neumann_flag && !g->d.fields_set) return fail(NIN_EINVAL, "neumann_flag is required by every method");
    HIP_TRY(hipSetDevice(g->d.device));
    HostGrid &h = g->h;
    DeviceGrid &d = g->d;
    const int64_t P = h.n_points, E = h.n_elems;
    if (neumann_flag) {
        // packed by the host's OpenMP team (pack_host.cpp) into a page-locked staging buffer the grid keeps: 82 MB of float64
        // flags in, 10 MB out at 10 M nodes -- the serial loop + pageable copy this replaces took ~15 ms of every interpolate()
        if (!d.flag_staging) HIP_TRY(hipHostMalloc((void **)&d.flag_staging, (size_t)std::max<int64_t>(P, 1), hipHostMallocDefault));
        pack_node_flags(neumann_flag, h.boundary_points.data(), P, d.flag_staging);
        HIP_TRY(hipMemcpy(const_cast<uint8_t *>(d.v.flags), d.flag_staging, (size_t)P, hipMemcpyHostToDevice));
        d.flags_host_stale = false;
    }
    if (permeability && diff_mag) {   // NULL keeps what is resident (0.8 GB at 10 M cells: callers upload it once per mesh)
        HIP_TRY(hipMemcpy(const_cast<double *>(d.v.perm), permeability, (size_t)E * 9 * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(const_cast<double *>(d.v.diff_mag), diff_mag, (size_t)E * 8, hipMemcpyHostToDevice));
        d.have_perm = true;
        d.all_dirty = true;   // a full table: no record of which cells it changed
    }
    d.fields_set = true;
    return NIN_OK;
}

// Give the grid's call scratch back (the buffers nin_interpolate_csr_host / nin_csr_compact_host / nin_apply_* allocate
// on first use and keep: ~2.3 GB of HBM at 10 M cells, + 10 MB of page-locked host memory; the transpose index, 0.69 GB more);
// the next call allocates again.
int nin_grid_release_scratch(nin_grid *g) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    DeviceGrid &d = g->d;
    if (d.device < 0) return NIN_OK;
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(hipDeviceSynchronize());
    dev_release(d, d.e2e_weights); dev_release(d, d.e2e_nws); dev_release(d, d.e2e_data); dev_release(d, d.e2e_cnt);
    dev_release(d, d.e2e_ptr); dev_release(d, d.e2e_indices); dev_release(d, d.e2e_tmp); dev_release(d, d.apply_weights);
    dev_release(d, d.tr_cell_ptr); dev_release(d, d.tr_cell_pos); dev_release(d, d.tr_cell_node);
    d.e2e_tmp_bytes = 0;
    release_adjoint_state(d);   // the GLS adjoint's bins, contribution buffer and scratch slots
    // a dirty launch's lists, histogram, scan temporary and descriptors (the marks themselves and their header are state: they stay)
    dev_release(d, d.dirty_lists); dev_release(d, d.dirty_hist); dev_release(d, d.dirty_tmp); dev_release(d, d.dirty_desc);
    d.dirty_tmp_bytes = d.dirty_desc_words = 0;
    if (d.flag_staging) { (void)hipHostFree(d.flag_staging); d.flag_staging = nullptr; }
    // the connectivity copies of nin_grid_update_points*: kept while the device builder's mirror still fetches from them (they were its
    // own before the first update: no HBM is held that the grid did not hold anyway)
    if (d.up_inpoel && !(g->h.lazy && g->h.lazy->reads(d.up_inpoel))) {
        std::string err;   // the face areas live nowhere else on the device: to the host first, if the host copy is the old mesh's
        if (g->h.ensure(A_AREAS, &err)) return fail(NIN_EHIP, "mirroring faces_areas: %s", err.c_str());
        dev_release(d, d.up_inpoel); dev_release(d, d.up_etype); dev_release(d, d.up_inpofa); dev_release(d, d.up_areas);
        d.up_areas_valid = false;
    }
    return NIN_OK;
}

int64_t nin_algorithmic_bytes(const nin_grid *g, int method) {
    if (!g) return -1;
    // SURVEY 8(d), canonical device layout s_i = 4:
    //   B_idw/ls = 4(P+1) + 4 nnz_esup + 24P + 24E + 2P + (8+4) nnz_out + 8P          (nnz_out = nnz_esup)
    //   B_gls    = B_idw/ls + 4(P+1) + 4 nnz_fsup + F (2*4 + 1 + 24 + 24) + E (72+8) + 8P
    const int64_t P = g->h.n_points, E = g->h.n_elems, F = g->h.n_faces;
    const int64_t nze = g->h.nnz_esup, nzf = g->h.nnz_fsup;
    int64_t b = 4 * (P + 1) + 4 * nze + 24 * P + 24 * E + 2 * P + 12 * nze + 8 * P;
    if (method == NIN_METHOD_GLS) b += 4 * (P + 1) + 4 * nzf + F * 57 + E * 80 + 8 * P;
    return b;
}

const char *nin_kernel_name(int method) {
    if (method == NIN_METHOD_IDW) return "nin_rows_kernel<0>";
    if (method == NIN_METHOD_LS) return "nin_rows_kernel<1>";
    return kernel_name_gls_hex8mf();   // dominant on hexahedron meshes; kernel_name_gls_block() covers the other nodes
}

int nin_host_alloc(size_t bytes, void **ptr) {
    if (!ptr) return fail(NIN_EINVAL, "NULL argument");
    *ptr = nullptr;
    const hipError_t e = hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(NIN_ENOMEM, "hipHostMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    return NIN_OK;
}

int nin_host_free(void *ptr) {
    if (!ptr) return NIN_OK;
    const hipError_t e = hipHostFree(ptr);
    if (e != hipSuccess) return fail(NIN_EHIP, "hipHostFree: %s", hipGetErrorString(e));
    return NIN_OK;
}
