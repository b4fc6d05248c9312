// abi.hip -- the extern "C" surface declared in include/ninpol_amd.h.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cmath>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/ninpol_amd.h"
#include "device_grid.hpp"
#include "gls_adjoint.hpp"
#include "grid_host.hpp"
#include "hex8_desc.hpp"
#include "launch.hpp"
#include "mfw_desc.hpp"
#include "mfg_desc.hpp"
#include "mfx_desc.hpp"
#include "quad4_desc.hpp"

using namespace nin;

struct nin_grid {
    HostGrid h;
    DeviceGrid d;
    std::vector<uint8_t> node_class;  // GLS size class of every node (host copy, for target subsets)
    int coords_dim = 3;
};

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

}  // namespace

namespace nin {
// the same for the other translation units of the C ABI (exchange.hip): sets what nin_last_error() returns
int abi_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace nin

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(NIN_EHIP, "%s: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

template <class T>
int dev_alloc(DeviceGrid &d, T **ptr, size_t count) {
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) return fail(NIN_ENOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    d.allocs.push_back(p);
    *ptr = static_cast<T *>(p);
    return 0;
}

template <class T>
int dev_upload(DeviceGrid &d, const T **ptr, const std::vector<T> &src) {
    T *p = nullptr;
    int rc = dev_alloc(d, &p, src.size());
    if (rc) return rc;
    if (!src.empty()) HIP_TRY(hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    *ptr = p;
    return 0;
}

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


// ---- locality order of a kernel's node list --------------------------------------------------------------------------------
// A list in node order walks the mesh the way its nodes are numbered (a structured mesh: along x, row by row, plane by plane),
// and a node shares its cells and faces with neighbours that are a whole plane of the numbering away: with 2 x 256 groups of
// the cube-node kernel in flight per XCD the data comes in again for every plane (FETCH_SIZE 3.58 GiB per launch at 216^3
// against 2.6 with half as many waves).  So the list is reordered by where the nodes ARE -- inside each piece of interpolate()'s
// pipeline, whose pieces stay sub-ranges of the list:
//   default   strips of 16 mesh rows (axis 1 quantised to ~cbrt(P) levels) walked plane by plane (axis 2), node order inside:
//             the rows a plane apart meet in the 4 MB L2 and the requests stay as coalesced as the numbering makes them --
//             FETCH_SIZE 3.58 -> 1.97 GiB (traffic = the algorithmic bytes), 4.90 -> 4.78 ms in one session (s4 / s8 / s32: 4.84 /
//             4.85 / 4.82);
//   "m"       Morton order of the coordinates (10 bits an axis over the bounding cube): 3.05 GiB but 1.6 % SLOWER than node order
//             -- uncoalesced requests are instructions too, and the kernel is bound by what it issues;
//   "off"     node order.
// Any order gives the same weights bit for bit (a node's arithmetic does not depend on its neighbours in the list; tested).
// Runs of 16 consecutive entries (one pass of a 16-nodes-per-wavefront kernel) move as one: inside a run the rows of the CSR
// tables and of the output stay next to each other -- single nodes in Morton order cost more in uncoalesced requests than
// the order saves (5.09 against 4.83 ms at 216^3, measured; runs of 64 / 256 are slower still).
#ifndef NIN_LOCALITY_RUN
#define NIN_LOCALITY_RUN 16
#endif
constexpr int kLocalityRun = NIN_LOCALITY_RUN;
__device__ __forceinline__ uint32_t spread10(uint32_t v) {   // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// strip > 0: instead, strips of `strip` mesh rows (axis 1 at ~cbrt(P) levels) walked plane by plane (axis 2), node order inside:
// the rows a plane apart meet in the L2 while the requests stay as coalesced as the numbering makes them
__global__ void k_locality_keys(const double *__restrict__ coords, const int32_t *__restrict__ nodes, int32_t count, double lo,
                                double scale, int32_t c1, int32_t c2, int32_t c3, int32_t strip, double lscale,
                                uint32_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int32_t p = nodes[i & ~(int64_t)(kLocalityRun - 1)];   // the key of the run's first entry: the (stable) sort moves whole runs
    uint32_t q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double t = (coords[3 * (size_t)p + k] - lo) * scale;
        q[k] = t > 0.0 ? (t < 1023.0 ? (uint32_t)t : 1023u) : 0u;
    }
    const int32_t self = nodes[i];
    const uint32_t piece = (uint32_t)(self >= c1) + (uint32_t)(self >= c2) + (uint32_t)(self >= c3);
    if (strip > 0) {
        const double ty = (coords[3 * (size_t)p + 1] - lo) * lscale, tz = (coords[3 * (size_t)p + 2] - lo) * lscale;
        const uint32_t yq = ty > 0.0 ? (ty < 32767.0 ? (uint32_t)(ty + 0.5) : 32767u) : 0u;
        const uint32_t zq = tz > 0.0 ? (tz < 32767.0 ? (uint32_t)(tz + 0.5) : 32767u) : 0u;
        keys[i] = (piece << 30) | ((yq / (uint32_t)strip) << 15) | zq;
        return;
    }
    keys[i] = (piece << 30) | spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
}
// `list` (device, count entries, ascending node ids) -> the same entries in locality order; pieces = the pipeline's node boundaries
int locality_order(const DeviceGrid &d, int32_t *list, int32_t count, const int32_t *chunk_node) {
    if (count < 2048) return NIN_OK;
    double lo = 0.0, hi = 0.0;
    {   // the bounding cube: smallest and largest coordinate of any axis
        double *mm = nullptr;
        void *rt = nullptr;
        size_t rb = 0, rb2 = 0;
        const int n3 = 3 * d.v.n_points;
        bool ok = hipMalloc((void **)&mm, 16) == hipSuccess &&
                  hipcub::DeviceReduce::Min(nullptr, rb, d.v.coords, mm, n3) == hipSuccess &&
                  hipcub::DeviceReduce::Max(nullptr, rb2, d.v.coords, mm + 1, n3) == hipSuccess &&
                  hipMalloc(&rt, rb > rb2 ? rb : rb2) == hipSuccess;
        rb = rb > rb2 ? rb : rb2;
        ok = ok && hipcub::DeviceReduce::Min(rt, rb, d.v.coords, mm, n3) == hipSuccess &&
             hipcub::DeviceReduce::Max(rt, rb, d.v.coords, mm + 1, n3) == hipSuccess;
        double h2[2] = {0.0, 0.0};
        ok = ok && hipMemcpy(h2, mm, 16, hipMemcpyDeviceToHost) == hipSuccess;
        (void)hipFree(mm); (void)hipFree(rt);
        if (!ok) return fail(NIN_EHIP, "locality order: bounding cube: %s", hipGetErrorString(hipGetLastError()));
        lo = h2[0]; hi = h2[1];
    }
    if (!(hi > lo)) return NIN_OK;
    uint32_t *keys = nullptr, *keys_out = nullptr;
    int32_t *list_out = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    int rc = NIN_OK;
    auto step = [&](hipError_t e) { if (e != hipSuccess && rc == NIN_OK) rc = fail(NIN_EHIP, "locality order: %s", hipGetErrorString(e)); return e == hipSuccess; };
    if (step(hipMalloc((void **)&keys, (size_t)count * 4)) && step(hipMalloc((void **)&keys_out, (size_t)count * 4)) &&
        step(hipMalloc((void **)&list_out, (size_t)count * 4))) {
        const char *mode = getenv("NIN_GLS_LOCALITY_ORDER");
        const int32_t strip = !mode ? 16 : mode[0] == 's' ? (mode[1] ? atoi(mode + 1) : 16) : 0;   // default: strips of 16 rows; "m": Morton
        const double levels = std::cbrt((double)d.v.n_points) - 1.0;                          // mesh intervals per axis of a cube of this many nodes
        hipLaunchKernelGGL(k_locality_keys, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, nullptr, d.v.coords, list, count, lo,
                           1024.0 / (hi - lo), chunk_node[1], chunk_node[2], chunk_node[3], strip, (levels > 1.0 ? levels : 1.0) / (hi - lo), keys);
        if (step(hipGetLastError()) && step(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys, keys_out, list, list_out, count)) &&
            step(hipMalloc(&tmp, tmp_bytes)) &&
            step(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys, keys_out, list, list_out, count)))
            (void)step(hipMemcpy(list, list_out, (size_t)count * 4, hipMemcpyDeviceToDevice));
    }
    (void)hipFree(keys); (void)hipFree(keys_out); (void)hipFree(list_out); (void)hipFree(tmp);
    return rc;
}

// a buffer of d.allocs given back before the grid goes
void dev_release(DeviceGrid &d, void *p) {
    if (!p) return;
    auto it = std::find(d.allocs.begin(), d.allocs.end(), p);
    if (it != d.allocs.end()) d.allocs.erase(it);
    (void)hipFree(p);
}

// The cell-major index of the esup pattern (DeviceGrid::tr_*), built once per grid by the first transpose call: a stable radix sort
// of the pairs (esup[j], j) by cell keeps ascending j -- hence ascending node id -- within each cell; cell_ptr and the node of each
// position follow by binary search.  Synchronises `stream` (the sort's temporaries are freed before the call returns).
int ensure_transpose_index(DeviceGrid &d, hipStream_t stream) {
    if (d.tr_cell_ptr) return NIN_OK;
    const int32_t E = d.v.n_elems, nnz = (int32_t)d.nnz_e;
    int32_t *ptr = nullptr, *pos = nullptr, *node = nullptr, *cells_sorted = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    int end_bit = 1;
    while (end_bit < 31 && (int64_t{1} << end_bit) < (int64_t)E) ++end_bit;   // the cell ids fit in end_bit bits
    int rc = dev_alloc(d, &ptr, (size_t)E + 1);
    if (!rc) rc = dev_alloc(d, &pos, (size_t)nnz);
    if (!rc) rc = dev_alloc(d, &node, (size_t)nnz);   // holds the sort's values 0 .. nnz-1 until cell_node overwrites it
    auto step = [&](hipError_t e) { if (e != hipSuccess && rc == NIN_OK) rc = fail(NIN_EHIP, "transpose index: %s", hipGetErrorString(e)); return rc == NIN_OK; };
    if (!rc && nnz > 0) {
        if (step(hipMalloc((void **)&cells_sorted, (size_t)nnz * sizeof(int32_t))) &&
            step(launch_iota(node, nnz, stream) ? hipErrorLaunchFailure : hipSuccess) &&
            step(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d.v.esup, cells_sorted, node, pos, nnz, 0, end_bit, stream)) &&
            step(hipMalloc(&tmp, tmp_bytes)) &&
            step(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, d.v.esup, cells_sorted, node, pos, nnz, 0, end_bit, stream)))
            (void)step(launch_transpose_index_fill(d.v, cells_sorted, nnz, ptr, pos, node, stream) ? hipErrorLaunchFailure : hipSuccess);
        (void)step(hipStreamSynchronize(stream));
    } else if (!rc) {
        (void)step(launch_transpose_index_fill(d.v, nullptr, 0, ptr, pos, node, stream) ? hipErrorLaunchFailure : hipSuccess);
        (void)step(hipStreamSynchronize(stream));
    }
    (void)hipFree(cells_sorted); (void)hipFree(tmp);
    if (rc) { dev_release(d, ptr); dev_release(d, pos); dev_release(d, node); return rc; }
    d.tr_cell_ptr = ptr; d.tr_cell_pos = pos; d.tr_cell_node = node;
    return NIN_OK;
}

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

// inpoel / etype / inpofa and the face-area array on the device (DeviceGrid::up_*): from the device builder's mirror if it still
// holds them, else uploaded from the host arrays.  Synchronous.
int ensure_update_inputs(nin_grid *g) {
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
    int32_t *inpoel = nullptr, *inpofa = nullptr;
    int8_t *etype = nullptr;
    double *areas = nullptr;
    int rc = dev_alloc(d, &inpoel, h.inpoel.size());
    if (!rc) rc = dev_alloc(d, &etype, h.etype.size());
    if (!rc) rc = dev_alloc(d, &inpofa, h.inpofa.size());
    if (!rc) rc = dev_alloc(d, &areas, (size_t)h.n_faces);
    auto up = [&](void *dst, const void *src, size_t bytes) {
        if (!rc && bytes && hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = fail(NIN_EHIP, "uploading the connectivity failed");
    };
    up(inpoel, h.inpoel.data(), h.inpoel.size() * 4);
    up(etype, h.etype.data(), h.etype.size());
    up(inpofa, h.inpofa.data(), h.inpofa.size() * 4);
    if (rc) { dev_release(d, inpoel); dev_release(d, etype); dev_release(d, inpofa); dev_release(d, areas); return rc; }
    d.up_inpoel = inpoel; d.up_etype = etype; d.up_inpofa = inpofa; d.up_areas = areas;
    d.up_areas_valid = false;   // room only: a whole-mesh update writes every area, a local one uploads the host's first
    return NIN_OK;
}

// the points per cell of the element types, one byte each (grid_update.hip, fields_scatter.hip)
uint64_t pack_npoel8(const HostGrid &h) {
    uint64_t npoel8 = 0;
    for (int t = 0; t < kNumElementTypes; ++t) npoel8 |= (uint64_t)(h.npoel[t] & 0xff) << (8 * t);
    return npoel8;
}

// xyz [P][cd] on the host (then stream = the null stream and the call waits) or on the grid's device
int update_points_on_device(nin_grid *g, const double *xyz, bool on_host, int cd, hipStream_t stream) {
    DeviceGrid &d = g->d;
    HostGrid &h = g->h;
    HIP_TRY(hipSetDevice(d.device));
    int rc = ensure_update_inputs(g);
    if (rc) return rc;
    if (!d.ev_geom) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        d.ev_geom = e;
    }
    const size_t P = (size_t)h.n_points;
    double *coords = const_cast<double *>(d.v.coords);
    double *staged = nullptr;
    if (on_host && cd == 3) {
        HIP_TRY(hipMemcpy(coords, xyz, P * 24, hipMemcpyHostToDevice));
    } else {
        if (on_host) {
            HIP_TRY(hipMalloc((void **)&staged, P * cd * sizeof(double)));
            if (hipMemcpy(staged, xyz, P * cd * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = fail(NIN_EHIP, "uploading the coordinates failed");
        }
        if (!rc && launch_update_coords(on_host ? staged : xyz, cd, (int64_t)P, coords, stream)) rc = fail(NIN_EHIP, "coordinate copy: %s", hipGetErrorString(hipGetLastError()));
    }
    const uint64_t npoel8 = pack_npoel8(h);
    if (!rc && launch_update_geometry(d.v, npoel8, d.up_inpoel, d.up_etype, d.up_inpofa, const_cast<double *>(d.v.centroids),
                                      const_cast<double *>(d.v.face_center), const_cast<float *>(d.v.face_normal), d.up_areas, stream))
        rc = fail(NIN_EHIP, "geometry kernels: %s", hipGetErrorString(hipGetLastError()));
    if (!rc && d.v.centroids4 && launch_pad_centroids(d.v.centroids, h.n_elems, const_cast<double *>(d.v.centroids4), stream))
        rc = fail(NIN_EHIP, "centroid padding kernel");
    if (!rc && hipEventRecord(static_cast<hipEvent_t>(d.ev_geom), stream) != hipSuccess) rc = fail(NIN_EHIP, "hipEventRecord");
    if (on_host || rc) {
        const hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess && !rc) rc = fail(NIN_EHIP, "geometry update: %s", hipGetErrorString(e));
    }
    if (staged) (void)hipFree(staged);
    // the host copies of the five arrays are the old mesh's from here on (also after a failure half way): fetched again on first use
    h.have &= ~A_GEOMETRY;
    if (!h.lazy) h.lazy.reset(new GeometryMirror(&g->d));
    ++d.geom_updates;
    d.up_areas_valid = true;
    d.all_dirty = true;   // every row reads the geometry
    return rc;
}
// ---- the GLS launch plan (gls_plan.hpp): the two functions that switch over the launcher family -------------------------------
static_assert(kGlsDescHex8 == kHex8DescWords && kGlsDescQuad4 == kQuad4DescWords && kGlsDescMfw == kMfwDescWords &&
                  kGlsDescMfx == kMfxDescWords && kGlsDescMfg == kMfgDescWords, "gls_plan.hpp's descriptor sizes are not the descriptor headers'");

// the descriptors of `count` entries of a list of plan kernel k's nodes: gls_plan_row(k).desc_words words an entry
int launch_plan_desc(const DeviceGrid &d, GlsKernel k, const int32_t *nodes, int32_t count, uint32_t *desc, hipStream_t stream) {
    if (count <= 0) return 0;
    switch (gls_plan_row(k).family) {
        case GlsFamily::hex8: return launch_hex8_desc(d.v, nodes, count, reinterpret_cast<int32_t *>(desc), stream);
        case GlsFamily::quad4: return launch_quad4_desc(d.v, nodes, count, reinterpret_cast<int32_t *>(desc), stream);
        case GlsFamily::mfw: return launch_mfw_desc(d.v, nodes, count, desc, stream);
        case GlsFamily::mfx: return launch_mfx_desc(d.v, nodes, count, desc, stream);
        case GlsFamily::mfg: return launch_mfg_desc(d.v, nodes, count, desc, stream);
        default: return 0;   // the kernel reads no descriptors
    }
}

// plan kernel k on `count` entries of a list of its nodes and their descriptors (nodes == nullptr: the block / scratch kernels walk
// 0 .. count - 1).  The block / scratch parameters are the plan's own list's; the work counter is the table's.
int launch_plan_kernel(const DeviceGrid &d, GlsKernel k, const int32_t *nodes, const uint32_t *desc, int32_t count, int add_neumann,
                       double *out, double *nws, hipStream_t stream) {
    const GlsPlanRow r = gls_plan_row(k);
    const DeviceGrid::GlsList &l = d.plan[k];
    int32_t *queue = r.counter >= 0 ? d.gls_queue + r.counter : nullptr;
    const int32_t *idesc = reinterpret_cast<const int32_t *>(desc);
    switch (r.family) {
        case GlsFamily::block: return launch_gls_block(d.v, nodes, count, l.waves, l.col_slots, l.lds_bytes, add_neumann, out, nws, queue, stream);
        case GlsFamily::scratch:
            return launch_gls_class(d.v, nodes, count, 0, l.rows_per_lane, add_neumann, out, nws, d.gls_scratch, d.gls_scratch_stride,
                                    d.gls_scratch_slots, stream);
        case GlsFamily::hex8: return launch_gls_hex8mf(d.v, nodes, idesc, count, add_neumann, out, nws, queue, stream);
        case GlsFamily::mfw: return launch_gls_mfw(d.v, nodes, desc, count, r.sub, add_neumann, out, nws, queue, stream);
        case GlsFamily::small: return launch_gls_small(d.v, nodes, count, r.sub, add_neumann, out, nws, stream);
        case GlsFamily::quad4: return launch_gls_quad4(d.v, nodes, idesc, count, add_neumann, out, nws, stream);
        case GlsFamily::mfx: return launch_gls_mfx(d.v, nodes, desc, count, r.sub, add_neumann, out, nws, queue, stream);
        case GlsFamily::mfg: return launch_gls_mfg(d.v, nodes, desc, count, add_neumann, out, nws, queue, d.mfg_tiles, d.mfg_slots, stream);
    }
    return NIN_EINVAL;
}

// nin_grid_to_device's launch plan: the nodes binned by kernel (classified on the device), every list with its descriptors and its
// cuts for interpolate()'s pipeline
int build_gls_plan(nin_grid *g) {
    DeviceGrid &d = g->d;
    const int64_t P = g->h.n_points;
    int rc;
    g->node_class.assign((size_t)P, 0);
    // debugging switches: keep nodes away from a kernel (gls_plan.hpp: GlsRoute)
    auto unless = [](const char *name, int bit) { return getenv(name) == nullptr ? bit : 0; };
    const int use_group = unless("NIN_GLS_NO_GROUP", kRouteHex8) | unless("NIN_GLS_NO_MFW", kRouteMfw) |
                          unless("NIN_GLS_NO_MFW_GENERAL", kRouteMfwGeneral) | unless("NIN_GLS_NO_SMALL", kRouteSmall) |
                          unless("NIN_GLS_NO_QUAD4", kRouteQuad4) | unless("NIN_GLS_NO_MFX", kRouteMfx) |
                          unless("NIN_GLS_NO_MFX_7X12", kRouteMfx7x12) | unless("NIN_GLS_NO_MFX_SMALL", kRouteMfxSmall) |
                          unless("NIN_GLS_NO_MFG", kRouteMfg) | (getenv("NIN_GLS_MFX_NO_BOUNDARY") != nullptr ? kRouteMfxNoBoundary : 0) |
                          unless("NIN_GLS_MFW_GENERAL", kRouteMfxTakesGeneral);
    const bool force_global = getenv("NIN_GLS_FORCE_GLOBAL") != nullptr;   // testing switch: systems in global scratch
    int64_t need_max[kGlsClasses] = {0}, rows_max[kGlsClasses] = {0}, cols_max[kGlsClasses] = {0};
    {
        uint8_t *dcls = nullptr;   // stays resident (P bytes): a dirty launch bins its nodes on the device (fields_scatter.hip)
        unsigned long long *dmax = nullptr, hmax[3 * kGlsClasses];
        if ((rc = dev_alloc(d, &dcls, (size_t)P))) return rc;
        d.node_class = dcls;
        if (hipMalloc((void **)&dmax, sizeof hmax) != hipSuccess) return fail(NIN_ENOMEM, "hipMalloc");
        hipError_t e1 = hipMemset(dmax, 0, sizeof hmax);
        const int lrc = launch_classify(d.v, use_group, force_global, dcls, dmax, nullptr);
        if (e1 == hipSuccess) e1 = hipMemcpy(g->node_class.data(), dcls, (size_t)P, hipMemcpyDeviceToHost);
        if (e1 == hipSuccess) e1 = hipMemcpy(hmax, dmax, sizeof hmax, hipMemcpyDeviceToHost);
        (void)hipFree(dmax);
        if (lrc || e1 != hipSuccess) return fail(NIN_EHIP, "node classification: %s", hipGetErrorString(e1));
        for (int c = 0; c < kGlsClasses; ++c) { need_max[c] = (int64_t)hmax[3 * c]; rows_max[c] = (int64_t)hmax[3 * c + 1]; cols_max[c] = (int64_t)hmax[3 * c + 2]; }
    }
    std::vector<int32_t> lists[kGlsPlanKernels];
    {
        int8_t kernel_of[256];
        for (int c = 0; c < 256; ++c) kernel_of[c] = (int8_t)gls_class_kernel(c);
        for (int64_t p = 0; p < P; ++p) {
            const int k = kernel_of[g->node_class[p]];
            if (k < 0) return fail(NIN_EHIP, "node classification: class byte %d belongs to no kernel", (int)g->node_class[p]);
            lists[k].push_back((int32_t)p);
        }
        // every node the cube-node kernel does not take, ascending: what the fused apply leaves to the list kernel
        std::vector<int32_t> rest;
        rest.reserve((size_t)P - lists[gk::hex8].size());
        for (int64_t p = 0; p < P; ++p)
            if (g->node_class[p] != gls_class_byte(gk::hex8)) rest.push_back((int32_t)p);
        d.noncube_count = (int32_t)rest.size();
        const int32_t *lp = nullptr;
        if (d.noncube_count && (rc = dev_upload(d, &lp, rest))) return rc;
        d.noncube_nodes = lp;
        d.noncube_nodes_ready = true;
    }
    for (int c = 0; c < kGlsClasses; ++c) {   // the block kernel's classes and the scratch class: plan kernels 0 .. kGlsClasses - 1
        auto &k = d.plan[c];
        k.lds_bytes = c == kGlsClasses - 1 ? 0 : (int32_t)need_max[c];
        k.rows_per_lane = (int32_t)std::max<int64_t>(1, (rows_max[c] + 63) / 64);
        k.waves = gls_class_waves(c);
        k.col_slots = (int32_t)std::max<int64_t>(1, (cols_max[c] + 63) / 64);
    }
    // interpolate()'s pipeline: its pieces' node boundaries (multiples of 64 nodes)
    constexpr int K = DeviceGrid::kE2eChunks;
    for (int j = 0; j <= K; ++j) d.chunk_node[j] = j == K ? (int32_t)P : (int32_t)((P * j / K) & ~(int64_t)63);
    // (NIN_GLS_LOCALITY_ORDER: "s<rows>" = strips of that many mesh rows, the default s16; "m" = Morton order; "off" = node order)
    const char *lo_env = getenv("NIN_GLS_LOCALITY_ORDER");
    const bool locality = !(lo_env && (lo_env[0] == 'o' || lo_env[0] == '0'));
    for (int k = 0; k < kGlsPlanKernels; ++k) {
        auto &l = d.plan[k];
        l.count = (int32_t)lists[k].size();
        // where the pieces' boundaries fall in the list (ascending here on the host; a list in locality order on the device is
        // permuted inside the pieces only)
        for (int j = 0; j <= K; ++j) l.chunk_off[j] = (int32_t)(std::lower_bound(lists[k].begin(), lists[k].end(), d.chunk_node[j]) - lists[k].begin());
        if (!l.count) continue;
        const int32_t *lp = nullptr;
        if ((rc = dev_upload(d, &lp, lists[k]))) return rc;
        l.nodes = const_cast<int32_t *>(lp);
        if (k == gk::hex8 && locality && (rc = locality_order(d, l.nodes, l.count, d.chunk_node))) return rc;
        if (const int words = gls_plan_row(k).desc_words) {   // one record per list entry
            if ((rc = dev_alloc(d, &l.desc, (size_t)l.count * words))) return rc;
            if (launch_plan_desc(d, GlsKernel(k), l.nodes, l.count, l.desc, nullptr)) return fail(NIN_EHIP, "descriptor kernel of plan kernel %d", k);
        }
    }
    if (d.plan[gk::mfg_tiles].count) {   // one slot of tiles per resident wavefront
        d.mfg_slots = std::min<int32_t>(d.plan[gk::mfg_tiles].count, kMfgResidentWaves);
        if ((rc = dev_alloc(d, &d.mfg_tiles, (size_t)d.mfg_slots * kMfgSlotDoubles))) return rc;
    }
    d.gls_too_large = rows_max[gk::scratch] > 1024;
    if ((rc = dev_alloc(d, &d.gls_queue, (size_t)kGlsQueueInts))) return rc;
    if (d.plan[gk::scratch].count) {
        d.gls_scratch_slots = std::min<int32_t>(d.plan[gk::scratch].count, 512);   // one per resident team (kernels_gls.hip)
        d.gls_scratch_stride = need_max[gk::scratch] / 8;
        if ((rc = dev_alloc(d, &d.gls_scratch, (size_t)d.gls_scratch_slots * d.gls_scratch_stride))) return rc;
    }
    const char *mn = getenv("NIN_E2E_MIN_NODES");                                // (tests: the pipeline on small meshes too)
    d.chunkable = P >= (mn ? atoll(mn) : 64 * 1024) && P >= 64 * K && getenv("NIN_E2E_NO_PIPELINE") == nullptr;   // small meshes: one piece
    // a single class holding every node in order needs no list: the kernel walks 0..P-1 directly
    for (int c = 0; c < kGlsClasses; ++c)
        if (d.plan[c].count == P) { d.plan[c].nodes = nullptr; d.chunkable = false; }
    return NIN_OK;
}
}  // namespace

extern "C" {

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
    if (g->d.device < 0 || g->d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first, or nin_grid_update_points with a host array)");
    return update_points_on_device(g, dev_xyz, false, coords_dim, static_cast<hipStream_t>(stream));
}

int64_t nin_grid_geometry_updates(const nin_grid *g) { return g ? g->d.geom_updates : 0; }
int nin_grid_has_transpose_index(const nin_grid *g) { return g && g->d.tr_cell_ptr ? 1 : 0; }

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
    if (g->d.device < 0 || g->d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first)");
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

int nin_fields_set_permeability_device(nin_grid *g, const double *dev_permeability, const double *dev_scale, void *stream) {
    if (!g || !dev_permeability) return fail(NIN_EINVAL, "NULL argument");
    if (g->d.device < 0 || g->d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first, or nin_fields_set with host arrays)");
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
    if (g->d.device < 0 || g->d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first)");
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

// ---- one launch of the plan: every walk over its kernels goes through the two arrays below ---------------------------------------
// The long poles first, on the side stream when it is on (a node on global-memory tiles takes ~0.5 ms, one of the global-scratch class ~2 ms,
// on a wavefront of its own); then kMainOrder, where the two come up again for a launch whose side stream did not take them.
static constexpr GlsKernel kSideOrder[] = {gk::mfg_tiles, gk::scratch};
static constexpr GlsKernel kMainOrder[] = {gk::hex8,     gk::mfw_large, gk::mfw_small, gk::mfw_general, gk::small4,       gk::small8,
                                           gk::small12,  gk::quad4,     gk::mfx_6x10,  gk::mfx_7x11,    gk::mfx_8x13,     gk::mfx_9x15,
                                           gk::mfx_10x16, gk::mfx_boundary, gk::mfx_4x7, gk::mfx_7x12,  gk::mfg_tiles,    gk::block1,
                                           gk::block2,   gk::block4,    gk::block8,    gk::scratch};
static constexpr bool main_order_is_complete() {
    unsigned seen = 0;
    for (GlsKernel k : kMainOrder) seen |= 1u << k;
    return sizeof kMainOrder / sizeof kMainOrder[0] == kGlsPlanKernels && seen == (1u << kGlsPlanKernels) - 1;
}
static_assert(main_order_is_complete(), "kMainOrder must name every kernel of the plan once");
static bool on_side_stream(GlsKernel k) { return std::find(std::begin(kSideOrder), std::end(kSideOrder), k) != std::end(kSideOrder); }

// the entries of plan kernel k's list that lie in piece `piece` of interpolate()'s pipeline (piece < 0: the whole list)
struct PlanRange { const int32_t *nodes; const uint32_t *desc; int32_t count; };
static PlanRange plan_range(const DeviceGrid &d, GlsKernel k, int piece) {
    const auto &l = d.plan[k];
    const int32_t b = piece < 0 ? 0 : l.chunk_off[piece], n = (piece < 0 ? l.count : l.chunk_off[piece + 1]) - b;
    return {l.nodes ? l.nodes + b : nullptr, l.desc ? l.desc + (size_t)gls_plan_row(k).desc_words * b : nullptr, n};
}

// kSideOrder's kernels on the side stream: ordered behind everything enqueued on `stream` so far (the zeroed work counters, the
// caller's buffers) and joined by gls_side_end.  NIN_GLS_NO_SIDE_STREAM=1: off.
static int gls_side_begin(DeviceGrid &d, int piece, int add_neumann, double *out, double *nws, hipStream_t stream) {
    d.side_pending = false;
    bool any = false;
    for (GlsKernel k : kSideOrder) any = any || plan_range(d, k, piece).count > 0;
    if (!any || getenv("NIN_GLS_NO_SIDE_STREAM") != nullptr) return 0;
    if (!d.side_stream) {
        hipStream_t s = nullptr;
        hipEvent_t a = nullptr, e = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&a, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
            return -3;
        d.side_stream = s; d.ev_fork = a; d.ev_join = e;
    }
    hipStream_t side = static_cast<hipStream_t>(d.side_stream);
    if (hipEventRecord(static_cast<hipEvent_t>(d.ev_fork), stream) != hipSuccess || hipStreamWaitEvent(side, static_cast<hipEvent_t>(d.ev_fork), 0) != hipSuccess)
        return -3;
    int rc = 0;
    for (GlsKernel k : kSideOrder) {
        const PlanRange r = plan_range(d, k, piece);
        if (!rc && r.count > 0) rc = launch_plan_kernel(d, k, r.nodes, r.desc, r.count, add_neumann, out, nws, side);
    }
    if (!rc && hipEventRecord(static_cast<hipEvent_t>(d.ev_join), side) != hipSuccess) rc = -3;
    d.side_pending = rc == 0;
    return rc;
}
static int gls_side_end(DeviceGrid &d, hipStream_t stream) {
    if (!d.side_pending) return 0;
    d.side_pending = false;
    return hipStreamWaitEvent(stream, static_cast<hipEvent_t>(d.ev_join), 0) == hipSuccess ? 0 : -3;
}

// NIN_GLS_ONLY=<k>: launch only kernel k of the plan (a GlsKernel: numbered as nin_gls_plan counts them; measurement: bench.py times
// the kernels of a plan one by one; read at every launch)
static int gls_only() {
    const char *e = getenv("NIN_GLS_ONLY");
    return e && *e ? atoi(e) : -1;
}

// The plan's kernels on the main stream for one piece of the pipeline (piece < 0: all nodes), then the join with the side stream.  The
// work counters are zeroed by the caller; what gls_side_begin took is left out.  cube = false: without the cube-node kernel (the fused
// apply launches its own form of it); only >= 0: that kernel alone.
static int gls_main(DeviceGrid &d, int piece, bool cube, int only, int add_neumann, double *out, double *nws, hipStream_t stream) {
    int rc = 0;
    for (GlsKernel k : kMainOrder) {
        if ((k == gk::hex8 && !cube) || (only >= 0 && only != k) || (d.side_pending && on_side_stream(k))) continue;
        const PlanRange r = plan_range(d, k, piece);
        if (!rc && r.count > 0) rc = launch_plan_kernel(d, k, r.nodes, r.desc, r.count, add_neumann, out, nws, stream);
    }
    if (!rc) rc = gls_side_end(d, stream);
    return rc;
}

int nin_weights_device(nin_grid *g, int method, const int64_t *targets, int64_t n_targets, int add_neumann,
                       double *dev_csr_data, double *dev_neumann_ws, void *stream_) {
    if (!g || !dev_csr_data || !dev_neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device: the weight kernels are HIP only");
    if (!d.fields_set) return fail(NIN_ESTATE, "nin_fields_set has not been called");
    if (method != NIN_METHOD_GLS && method != NIN_METHOD_IDW && method != NIN_METHOD_LS)
        return fail(NIN_EINVAL, "unknown method %d", method);
    if (method == NIN_METHOD_GLS && !d.have_perm) return fail(NIN_ESTATE, "GLS needs permeability and diff_mag");
    if (method == NIN_METHOD_GLS && d.gls_too_large)
        return fail(NIN_ERANGE, "a node's GLS system has more than 1024 rows (more than ~100 cells around one node): beyond the fallback kernel");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(d.device));
    const int64_t P = g->h.n_points;
    const bool all = targets == nullptr;
    if (!all && n_targets < 0) return fail(NIN_EINVAL, "negative n_targets");
    int rc = 0;
    if (all) {
        if (method == NIN_METHOD_IDW) rc = launch_idw(d.v, nullptr, (int32_t)P, (int32_t)g->h.mx_elems_per_point, d.nnz_e, dev_csr_data, dev_neumann_ws, stream);
        else if (method == NIN_METHOD_LS) rc = launch_ls(d.v, nullptr, (int32_t)P, (int32_t)g->h.mx_elems_per_point, d.nnz_e, dev_csr_data, dev_neumann_ws, stream);
        else {
            HIP_TRY(hipMemsetAsync(d.gls_queue, 0, kGlsQueueInts * sizeof(int32_t), stream));   // the launches' work counters
            const int only = gls_only();
            if (only < 0) rc = gls_side_begin(d, -1, add_neumann, dev_csr_data, dev_neumann_ws, stream);
            if (!rc) rc = gls_main(d, -1, true, only, add_neumann, dev_csr_data, dev_neumann_ws, stream);
        }
        if (rc) return fail(rc, "kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        return NIN_OK;
    }
    // explicit target list: outputs of every other node are zero
    for (int64_t i = 0; i < n_targets; ++i)
        if (targets[i] < 0 || targets[i] >= P) return fail(NIN_EINVAL, "target %lld out of range", (long long)targets[i]);
    HIP_TRY(hipMemsetAsync(dev_csr_data, 0, (size_t)d.nnz_e * 8, stream));
    HIP_TRY(hipMemsetAsync(dev_neumann_ws, 0, (size_t)P * 8, stream));
    if (n_targets == 0) return NIN_OK;
    const bool gls = method == NIN_METHOD_GLS;
    std::vector<int32_t> lists[kGlsPlanKernels];   // the targets by plan kernel (IDW / LS: all in the first)
    for (int64_t i = 0; i < n_targets; ++i) lists[gls ? gls_class_kernel(g->node_class[targets[i]]) : 0].push_back((int32_t)targets[i]);
    // one device buffer for all lists and their descriptors, filled before the first launch: a per-list allocate / copy / free
    // cycle lets the allocator hand the same memory to the next list while the previous kernel still reads it
    // (the pageable copy is not ordered behind that kernel).  One descriptor launch per non-empty list, not per family: a few tiny launches more
    std::vector<int32_t> flat;
    size_t first[kGlsPlanKernels], desc_first[kGlsPlanKernels], words = 0;   // where a list begins; where its descriptors begin, behind the lists
    for (int k = 0; k < kGlsPlanKernels; ++k) {
        first[k] = flat.size();
        desc_first[k] = words;
        flat.insert(flat.end(), lists[k].begin(), lists[k].end());
        if (gls) words += lists[k].size() * (size_t)gls_plan_row(k).desc_words;
    }
    int32_t *dl0 = nullptr;
    HIP_TRY(hipMalloc((void **)&dl0, (flat.size() + words) * 4));
    hipError_t e = hipMemcpy(dl0, flat.data(), flat.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(dl0); return fail(NIN_EHIP, "hipMemcpy: %s", hipGetErrorString(e)); }
    uint32_t *ddesc = reinterpret_cast<uint32_t *>(dl0 + flat.size());
    if (!gls) {
        rc = method == NIN_METHOD_IDW ? launch_idw(d.v, dl0, (int32_t)flat.size(), 0, 0, dev_csr_data, dev_neumann_ws, stream)
                                      : launch_ls(d.v, dl0, (int32_t)flat.size(), 0, 0, dev_csr_data, dev_neumann_ws, stream);
    } else {
        for (int k = 0; k < kGlsPlanKernels; ++k)
            if (launch_plan_desc(d, GlsKernel(k), dl0 + first[k], (int32_t)lists[k].size(), ddesc + desc_first[k], stream)) {
                (void)hipFree(dl0);
                return fail(NIN_EHIP, "descriptor kernel of plan kernel %d", k);
            }
        e = hipMemsetAsync(d.gls_queue, 0, kGlsQueueInts * sizeof(int32_t), stream);
        if (e != hipSuccess) { (void)hipFree(dl0); return fail(NIN_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e)); }
        for (GlsKernel k : kMainOrder)   // (no side stream: every target's row is written by exactly one kernel, in any order)
            if (!rc && !lists[k].empty())
                rc = launch_plan_kernel(d, k, dl0 + first[k], ddesc + desc_first[k], (int32_t)lists[k].size(),
                                        add_neumann, dev_csr_data, dev_neumann_ws, stream);
    }
    const hipError_t sy = hipStreamSynchronize(stream);   // the lists must outlive the kernels
    (void)hipFree(dl0);
    if (sy != hipSuccess) return fail(NIN_EHIP, "target kernels: %s", hipGetErrorString(sy));
    if (rc) return fail(rc, "kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return NIN_OK;
}

// ---- local permeability updates (fields_scatter.hip) ---------------------------------------------------------------
namespace {

// the marks and their header block: state of the grid from the first scatter on (P + 128 bytes)
int ensure_dirty_state(DeviceGrid &d, int64_t P) {
    if (d.dirty) return NIN_OK;
    uint8_t *marks = nullptr;
    int32_t *hdr = nullptr;
    int rc = dev_alloc(d, &marks, (size_t)P);
    if (!rc) rc = dev_alloc(d, &hdr, (size_t)kDirtyHdrInts);
    if (!rc && (hipMemset(marks, 0, (size_t)P) != hipSuccess || hipMemset(hdr, 0, kDirtyHdrInts * sizeof(int32_t)) != hipSuccess))
        rc = fail(NIN_EHIP, "zeroing the dirty set failed");
    if (rc) { dev_release(d, marks); dev_release(d, hdr); return rc; }
    d.dirty = marks; d.dirty_hdr = hdr;
    return NIN_OK;
}

// a scratch buffer of the dirty launch with room for `count` elements: kept while it is large enough (hipFree waits for the device)
extern "C++" {
template <class T>
int grow(DeviceGrid &d, T **buf, size_t *have, size_t count) {
    if (*buf && *have >= count) return NIN_OK;
    dev_release(d, *buf);
    *buf = nullptr;
    *have = 0;
    const int rc = dev_alloc(d, buf, count);
    if (!rc) *have = count;
    return rc;
}
}

// NIN_TIMING=1: HIP events on the launch's stream around its three phases -- compaction + read-back, descriptor kernels, weight
// kernels -- and one line on stderr; the call then waits for its kernels (tools/time_update_fields.py --local reads the lines)
struct DirtyLaps {
    bool on = getenv("NIN_TIMING") != nullptr;
    hipStream_t stream;
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    explicit DirtyLaps(hipStream_t s) : stream(s) {}
    ~DirtyLaps() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    void mark(int i) { if (on && !e[i] && hipEventCreate(&e[i]) == hipSuccess) (void)hipEventRecord(e[i], stream); }
    void report(int64_t n) {
        if (!on || !e[0] || !e[1] || !e[2] || !e[3] || hipEventSynchronize(e[3]) != hipSuccess) return;
        float ms[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&ms[i], e[i], e[i + 1]);
        fprintf(stderr, "[nin_dirty] nodes %lld compact+readback %.4f descriptors %.4f weights %.4f ms\n", (long long)n, ms[0], ms[1], ms[2]);
    }
};

}  // namespace

int nin_fields_scatter_permeability_device(nin_grid *g, const void *dev_cell_ids, int ids_are_int64, int64_t n, const double *dev_permeability,
                                           const double *dev_scale, void *stream) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    if (n < 0) return fail(NIN_EINVAL, "negative n");
    if (g->d.device < 0 || g->d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first)");
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
    if (rc) return fail(rc, "scatter kernel: %s", hipGetErrorString(hipGetLastError()));
    d.scattered_cells = true;
    ++d.field_updates;
    return NIN_OK;
}

// ---- Neumann flags from device memory (flags_update.hip) -------------------------------------------------------------
int nin_fields_set_flags_device(nin_grid *g, const void *dev_flags, int flags_are_bytes, void *stream) {
    if (!g || !dev_flags) return fail(NIN_EINVAL, "NULL argument");
    if (g->d.device < 0 || g->d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first, or nin_fields_set with host arrays)");
    DeviceGrid &d = g->d;
    HIP_TRY(hipSetDevice(d.device));
    int rc = ensure_dirty_state(d, g->h.n_points);
    if (rc) return rc;
    // while everything is dirty no marks are needed; afterwards only the nodes whose byte changes are marked
    rc = launch_set_flags(d.v.n_points, dev_flags, flags_are_bytes, const_cast<uint8_t *>(d.v.flags), d.all_dirty ? nullptr : d.dirty,
                          static_cast<hipStream_t>(stream));
    if (rc) return fail(rc, "flag kernel: %s", hipGetErrorString(hipGetLastError()));
    d.fields_set = true;
    d.flags_host_stale = true;
    ++d.flag_updates;
    return NIN_OK;
}

int nin_fields_scatter_flags_device(nin_grid *g, const void *dev_node_ids, int ids_are_int64, int64_t n, const void *dev_flags,
                                    int flags_are_bytes, void *stream) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    if (n < 0) return fail(NIN_EINVAL, "negative n");
    if (g->d.device < 0 || g->d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first)");
    if (n == 0) return NIN_OK;
    if (!dev_node_ids || !dev_flags) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (!d.fields_set) return fail(NIN_ESTATE, "no Neumann flags are resident to patch (nin_fields_set or nin_fields_set_flags_device first)");
    HIP_TRY(hipSetDevice(d.device));
    int rc = ensure_dirty_state(d, g->h.n_points);
    if (rc) return rc;
    rc = launch_scatter_flags(d.v.n_points, dev_node_ids, ids_are_int64, n, dev_flags, flags_are_bytes, const_cast<uint8_t *>(d.v.flags),
                              d.all_dirty ? nullptr : d.dirty, d.dirty_hdr + kDirtyHdrRejected, static_cast<hipStream_t>(stream));
    if (rc) return fail(rc, "flag scatter kernel: %s", hipGetErrorString(hipGetLastError()));
    d.scattered_flags = true;
    d.flags_host_stale = true;
    ++d.flag_updates;
    return NIN_OK;
}

// the host's copy of the resident flag bytes (flag_staging), brought up to date; waits for the device when it has to fetch
static int fetch_flag_bytes(nin_grid *g) {
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
    if (g->d.device < 0 || g->d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first)");
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
namespace {

// ids [n] (int32 / int64) and xyz [n][cd] on the host (then int64 ids, stream = the null stream and the call waits) or on the grid's device
int scatter_points_on_device(nin_grid *g, const void *ids, int ids_are_int64, int64_t n, const double *xyz, bool on_host, int cd,
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
    if (!d.ev_geom) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        d.ev_geom = e;
    }
    void *staged_ids = nullptr;
    double *staged_xyz = nullptr;
    if (on_host) {
        const size_t ib = (size_t)n * sizeof(int64_t), xb = (size_t)n * cd * sizeof(double);
        HIP_TRY(hipMalloc(&staged_ids, ib));
        if (hipMalloc((void **)&staged_xyz, xb) != hipSuccess) rc = fail(NIN_ENOMEM, "hipMalloc(%zu bytes) for the moved rows", xb);
        if (!rc && (hipMemcpy(staged_ids, ids, ib, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(staged_xyz, xyz, xb, hipMemcpyHostToDevice) != hipSuccess))
            rc = fail(NIN_EHIP, "uploading the moved nodes failed");
        if (rc) { (void)hipFree(staged_ids); (void)hipFree(staged_xyz); return rc; }   // nothing was launched: the geometry is as it was
        ids = staged_ids; xyz = staged_xyz;
    }
    if (launch_scatter_points(d.v, pack_npoel8(h), d.up_inpoel, d.up_etype, d.up_inpofa, ids, ids_are_int64, n, xyz, cd, d.up_areas, d.dirty,
                              d.dirty_hdr + kDirtyHdrRejected, stream))
        rc = fail(NIN_EHIP, "local geometry kernels: %s", hipGetErrorString(hipGetLastError()));
    if (!rc && hipEventRecord(static_cast<hipEvent_t>(d.ev_geom), stream) != hipSuccess) rc = fail(NIN_EHIP, "hipEventRecord");
    if (on_host || rc) {
        const hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess && !rc) rc = fail(NIN_EHIP, "local geometry update: %s", hipGetErrorString(e));
    }
    if (staged_ids) (void)hipFree(staged_ids);
    if (staged_xyz) (void)hipFree(staged_xyz);
    // the host copies of the five arrays are the old mesh's from here on (also after a failure half way): fetched again on first use
    h.have &= ~A_GEOMETRY;
    if (!h.lazy) h.lazy.reset(new GeometryMirror(&g->d));
    ++d.geom_updates;
    d.scattered_nodes = true;
    return rc;   // all_dirty stays as it is: the kernels marked the rows that can move
}

}  // namespace

int nin_grid_scatter_points_device(nin_grid *g, const void *dev_node_ids, int ids_are_int64, int64_t n, const double *dev_xyz, int coords_dim,
                                   void *stream) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    if (n < 0) return fail(NIN_EINVAL, "negative n");
    if (coords_dim != g->coords_dim) return fail(NIN_EINVAL, "coords_dim %d is not the grid's (%d)", coords_dim, g->coords_dim);
    if (g->d.device < 0 || g->d.prebuilt)
        return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first, or nin_grid_scatter_points with host arrays)");
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

int nin_weights_dirty_device(nin_grid *g, int method, int add_neumann, double *dev_csr_data, double *dev_neumann_ws, void *stream_, int clear,
                             int64_t *n_recomputed) {
    if (n_recomputed) *n_recomputed = 0;
    if (!g || !dev_csr_data || !dev_neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device: the weight kernels are HIP only");
    if (!d.fields_set) return fail(NIN_ESTATE, "nin_fields_set has not been called");
    if (method != NIN_METHOD_GLS && method != NIN_METHOD_IDW && method != NIN_METHOD_LS) return fail(NIN_EINVAL, "unknown method %d", method);
    const bool gls = method == NIN_METHOD_GLS;
    if (gls && !d.have_perm) return fail(NIN_ESTATE, "GLS needs permeability and diff_mag");
    if (gls && d.gls_too_large)
        return fail(NIN_ERANGE, "a node's GLS system has more than 1024 rows (more than ~100 cells around one node): beyond the fallback kernel");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(d.device));
    const int32_t P = (int32_t)g->h.n_points;
    int32_t hdr[kDirtyHdrInts] = {0};
    int rc = NIN_OK;
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
            if (launch_dirty_compact(P, gls ? 0 : 1, clear, d.dirty, d.node_class, d.dirty_hdr + kDirtyHdrRejected, d.dirty_hist,
                                     d.dirty_hist + ints / 2, d.dirty_tmp, d.dirty_tmp_bytes, d.dirty_lists, d.dirty_hdr, stream))
                return fail(NIN_EHIP, "compacting the dirty set: %s", hipGetErrorString(hipGetLastError()));
        }
        // the one synchronisation of the call: the lists' offsets and the refused-id counter, 128 bytes
        HIP_TRY(hipMemcpyAsync(hdr, d.dirty_hdr, sizeof hdr, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (hdr[kDirtyHdrRejected] != 0) {   // the marks are as they were (the fill pass clears nothing while the counter is set)
            HIP_TRY(hipMemsetAsync(d.dirty_hdr + kDirtyHdrRejected, 0, sizeof(int32_t), stream));
            // one counter for the three scatters: what was called since the last dirty launch says whose ids they can be
            const bool nodes = d.scattered_nodes, flags = d.scattered_flags, cells = d.scattered_cells || !(nodes || flags);
            d.scattered_cells = d.scattered_nodes = d.scattered_flags = false;
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
            return fail(NIN_EINVAL, "%d %s and written nowhere; nothing was launched, the dirty set is kept", (int)hdr[kDirtyHdrRejected], who);
        }
        d.scattered_cells = d.scattered_nodes = d.scattered_flags = false;
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
    if (!gls) {   // one list
        laps.mark(1); laps.mark(2);
        rc = method == NIN_METHOD_IDW ? launch_idw(d.v, d.dirty_lists, total, 0, 0, dev_csr_data, dev_neumann_ws, stream)
                                      : launch_ls(d.v, d.dirty_lists, total, 0, 0, dev_csr_data, dev_neumann_ws, stream);
        if (rc) return fail(rc, "kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        laps.mark(3);
        laps.report(total);
        return NIN_OK;
    }
    size_t desc_first[kGlsPlanKernels], words = 0;
    for (int k = 0; k < kGlsPlanKernels; ++k) {
        if (off[k + 1] < off[k]) return fail(NIN_EHIP, "the dirty set's lists are out of order");
        desc_first[k] = words;
        words += (size_t)(off[k + 1] - off[k]) * (size_t)gls_plan_row(k).desc_words;
    }
    if (words > d.dirty_desc_words && (rc = grow(d, &d.dirty_desc, &d.dirty_desc_words, words + words / 2))) return rc;
    laps.mark(1);
    for (int k = 0; k < kGlsPlanKernels; ++k)
        if (launch_plan_desc(d, GlsKernel(k), d.dirty_lists + off[k], off[k + 1] - off[k], d.dirty_desc + desc_first[k], stream))
            return fail(NIN_EHIP, "descriptor kernel of plan kernel %d", k);
    HIP_TRY(hipMemsetAsync(d.gls_queue, 0, kGlsQueueInts * sizeof(int32_t), stream));   // the launches' work counters
    laps.mark(2);
    for (GlsKernel k : kMainOrder)   // (no side stream: every listed row is written by exactly one kernel, in any order)
        if (!rc && off[k + 1] > off[k])
            rc = launch_plan_kernel(d, k, d.dirty_lists + off[k], d.dirty_desc + desc_first[k], off[k + 1] - off[k], add_neumann, dev_csr_data,
                                    dev_neumann_ws, stream);
    if (rc) return fail(rc, "kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    laps.mark(3);
    laps.report(total);
    return NIN_OK;
}

int64_t nin_grid_dirty_nodes(nin_grid *g) {
    if (!g || g->d.device < 0 || g->d.prebuilt) return 0;
    DeviceGrid &d = g->d;
    if (d.all_dirty) return -1;
    if (!d.dirty) return 0;
    int32_t n = 0;
    if (hipSetDevice(d.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||   // a scatter may be in flight on any stream
        hipMemset(d.dirty_hdr + kDirtyHdrCount, 0, sizeof(int32_t)) != hipSuccess ||
        launch_dirty_count((int32_t)g->h.n_points, d.dirty, d.dirty_hdr + kDirtyHdrCount, nullptr) ||
        hipMemcpy(&n, d.dirty_hdr + kDirtyHdrCount, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)fail(NIN_EHIP, "counting the dirty nodes: %s", hipGetErrorString(hipGetLastError()));
        return -2;
    }
    return n;
}

int nin_grid_dirty_reset(nin_grid *g, int all_dirty, void *stream) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first)");
    HIP_TRY(hipSetDevice(d.device));
    if (!all_dirty && d.dirty) {   // the marks and the refused-id counter
        HIP_TRY(hipMemsetAsync(d.dirty, 0, (size_t)g->h.n_points, static_cast<hipStream_t>(stream)));
        HIP_TRY(hipMemsetAsync(d.dirty_hdr + kDirtyHdrRejected, 0, sizeof(int32_t), static_cast<hipStream_t>(stream)));
    }
    d.all_dirty = all_dirty != 0;
    return NIN_OK;
}

int nin_weights_host(nin_grid *g, int method, const int64_t *targets, int64_t n_targets, int add_neumann,
                     double *csr_data, double *neumann_ws) {
    if (!g || !csr_data || !neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (d.device < 0) return fail(NIN_ENODEVICE, "grid is not on a device: the weight kernels are HIP only");
    HIP_TRY(hipSetDevice(d.device));
    const size_t nb = (size_t)std::max<int64_t>(d.nnz_e, 1) * 8, pb = (size_t)g->h.n_points * 8;
    double *dd = nullptr, *dn = nullptr;
    HIP_TRY(hipMalloc((void **)&dd, nb));
    hipError_t e = hipMalloc((void **)&dn, pb);
    if (e != hipSuccess) { (void)hipFree(dd); return fail(NIN_ENOMEM, "hipMalloc: %s", hipGetErrorString(e)); }
    int rc = nin_weights_device(g, method, targets, n_targets, add_neumann, dd, dn, nullptr);
    if (!rc) {
        e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(csr_data, dd, (size_t)d.nnz_e * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(neumann_ws, dn, pb, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(NIN_EHIP, "weights kernel / copy back: %s", hipGetErrorString(e));
    }
    (void)hipFree(dd);
    (void)hipFree(dn);
    return rc;
}

namespace {

struct Laps {   // NIN_TIMING=1: host-side laps of one call on stderr
    bool on = getenv("NIN_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[nin_e2e] %-22s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

int e2e_streams(DeviceGrid &d) {
    if (!d.copy_stream) {
        hipStream_t s;
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        d.copy_stream = s;
        hipEvent_t a, b;
        HIP_TRY(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        d.ev_weights = a;
        d.ev_scan = b;
    }
    return 0;
}

// The finish of interpolator.pyx:622-624 with the transfers overlapped: `weights_ready` (an event on `stream`, or null)
// marks the weights + neumann_ws written; dev_nws / neumann_ws (optional) ride the copy stream under the count / scan /
// compaction kernels, as does indptr; indices and data follow in pieces, each as soon as the copy engine is free.
int csr_compact_pipelined(nin_grid *g, const double *dev_csr_data, const double *dev_nws, int32_t *indptr, int32_t *indices,
                          double *data, int64_t *nnz_out, double *neumann_ws, hipStream_t stream) {
    DeviceGrid &d = g->d;
    const int64_t P = g->h.n_points;
    size_t tmp_bytes = 0;
    int rc = NIN_OK;
    Laps L;
    if ((rc = e2e_streams(d))) return rc;
    hipStream_t cs = static_cast<hipStream_t>(d.copy_stream);
    hipEvent_t ev_w = static_cast<hipEvent_t>(d.ev_weights), ev_s = static_cast<hipEvent_t>(d.ev_scan);
#define TRY_C(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(NIN_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
    // scratch of the compaction: owned by the grid, allocated on first use (sized by the mesh: P + 1 counters, nnz_e entries)
    if (!d.e2e_cnt && (rc = dev_alloc(d, &d.e2e_cnt, (size_t)(P + 1)))) return rc;
    if (!d.e2e_ptr && (rc = dev_alloc(d, &d.e2e_ptr, (size_t)(P + 1)))) return rc;
    int32_t *cnt = d.e2e_cnt, *ptr = d.e2e_ptr;
    if (dev_nws && neumann_ws) {   // 8 B per node: leaves as soon as the weight kernels are done
        TRY_C(hipEventRecord(ev_w, stream));
        TRY_C(hipStreamWaitEvent(cs, ev_w, 0));
        TRY_C(hipMemcpyAsync(neumann_ws, dev_nws, (size_t)P * 8, hipMemcpyDeviceToHost, cs));
    }
    TRY_C(hipMemsetAsync(cnt, 0, (size_t)(P + 1) * 4, stream));
    if ((rc = launch_row_nnz(d.v, dev_csr_data, cnt, stream))) return fail(rc, "launch failed");
    TRY_C(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt, ptr, (int)(P + 1), stream));
    if (tmp_bytes > d.e2e_tmp_bytes) {
        char *t = nullptr;
        if ((rc = dev_alloc(d, &t, std::max<size_t>(tmp_bytes, 16)))) return rc;   // (a smaller one stays in d.allocs until the grid goes)
        d.e2e_tmp = t;
        d.e2e_tmp_bytes = tmp_bytes;
    }
    TRY_C(hipcub::DeviceScan::ExclusiveSum(d.e2e_tmp, tmp_bytes, cnt, ptr, (int)(P + 1), stream));
    TRY_C(hipEventRecord(ev_s, stream));
    const size_t cap = (size_t)std::max<int64_t>(d.nnz_e, 1);
    const bool want_entries = indices && data;
    if (want_entries) {   // the compaction does not need the count on the host: it starts right behind the scan
        if (!d.e2e_indices && (rc = dev_alloc(d, &d.e2e_indices, cap))) return rc;
        if (!d.e2e_data && (rc = dev_alloc(d, &d.e2e_data, cap))) return rc;
        if ((rc = launch_compact(d.v, dev_csr_data, ptr, d.e2e_indices, d.e2e_data, stream))) return fail(rc, "launch failed");
    }
    TRY_C(hipStreamWaitEvent(cs, ev_s, 0));
    TRY_C(hipMemcpyAsync(indptr, ptr, (size_t)(P + 1) * 4, hipMemcpyDeviceToHost, cs));   // under the compaction kernel
    TRY_C(hipStreamSynchronize(cs));
    L.lap("weights+count+scan");
    const int64_t nnz = indptr[P];
    *nnz_out = nnz;
    if (nnz > 0 && want_entries) {
        TRY_C(hipStreamSynchronize(stream));
        L.lap("compaction");
        // two copy queues: the index and the value stream each keep a DMA engine busy
        TRY_C(hipMemcpyAsync(indices, d.e2e_indices, (size_t)nnz * 4, hipMemcpyDeviceToHost, stream));
        TRY_C(hipMemcpyAsync(data, d.e2e_data, (size_t)nnz * 8, hipMemcpyDeviceToHost, cs));
        TRY_C(hipStreamSynchronize(cs));
        TRY_C(hipStreamSynchronize(stream));
        L.lap("D2H indices+data");
    }
#undef TRY_C
    return NIN_OK;
}

}  // namespace

namespace {

// The weight kernels for the nodes of chunk k only (all nodes of the chunk, add_neumann fused): sub-ranges of the launch plan's lists.
int weights_chunk(nin_grid *g, int method, int k, double *out, double *nws, hipStream_t stream) {
    DeviceGrid &d = g->d;
    const int32_t P = (int32_t)g->h.n_points;
    if (method != NIN_METHOD_GLS)
        return launch_rows_range(d.v, method == NIN_METHOD_LS ? 1 : 0, P, d.chunk_node[k], d.chunk_node[k + 1],
                                 (int32_t)g->h.mx_elems_per_point, d.nnz_e, out, nws, stream);
    HIP_TRY(hipMemsetAsync(d.gls_queue, 0, kGlsQueueInts * sizeof(int32_t), stream));   // the launches' work counters
    int rc = gls_side_begin(d, k, 1, out, nws, stream);
    if (!rc) rc = gls_main(d, k, true, -1, 1, out, nws, stream);
    return rc ? fail(rc, "kernel launch failed: %s", hipGetErrorString(hipGetLastError())) : NIN_OK;
}

// interpolate() as a pipeline over kE2eChunks pieces of the node range: while piece k's surviving entries cross PCIe (the floor
// of this path: 0.95 GB at 57 GB/s = 16.7 ms at 10 M cells), piece k + 1 is computed, counted, scanned and compacted.  Per piece:
// weight kernels -> non-zeros per row -> exclusive scan seeded with the entries of the pieces before -> (4 bytes back: the
// running total) -> compaction -> its slices of indptr / indices / data leave on the copy queues.
int interpolate_chunked(nin_grid *g, int method, int32_t *indptr, int32_t *indices, double *data, int64_t *nnz_out,
                        double *neumann_ws) {
    DeviceGrid &d = g->d;
    constexpr int K = DeviceGrid::kE2eChunks;
    const int64_t P = g->h.n_points;
    Laps L;
    int rc = NIN_OK;
    if ((rc = e2e_streams(d))) return rc;
    hipStream_t cs = static_cast<hipStream_t>(d.copy_stream), stream = nullptr;
    hipEvent_t ev = static_cast<hipEvent_t>(d.ev_scan);
    // an error in the middle must not leave copies into the caller's buffers in flight
    auto drain = [&]() {
        (void)hipStreamSynchronize(cs);
        if (d.copy_stream2) (void)hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream2));
        (void)hipStreamSynchronize(stream);
    };
#define TRY_C(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { drain(); return fail(NIN_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); } } while (0)
    if (!d.e2e_cnt && (rc = dev_alloc(d, &d.e2e_cnt, (size_t)(P + 1)))) return rc;
    if (!d.e2e_ptr && (rc = dev_alloc(d, &d.e2e_ptr, (size_t)(P + 1)))) return rc;
    const size_t cap = (size_t)std::max<int64_t>(d.nnz_e, 1);
    if (!d.e2e_indices && (rc = dev_alloc(d, &d.e2e_indices, cap))) return rc;
    if (!d.e2e_data && (rc = dev_alloc(d, &d.e2e_data, cap))) return rc;
    size_t tmp_bytes = 0;
    TRY_C(hipcub::DeviceScan::ExclusiveScan(nullptr, tmp_bytes, d.e2e_cnt, d.e2e_ptr, hipcub::Sum(), (int32_t)0, (int)(P + 1), stream));
    if (tmp_bytes > d.e2e_tmp_bytes) {
        char *t = nullptr;
        if ((rc = dev_alloc(d, &t, std::max<size_t>(tmp_bytes, 16)))) return rc;
        d.e2e_tmp = t;
        d.e2e_tmp_bytes = tmp_bytes;
    }
    TRY_C(hipMemsetAsync(d.e2e_cnt, 0, (size_t)(P + 1) * 4, stream));
    int32_t base = 0;
    for (int k = 0; k < K; ++k) {
        const int32_t pb = d.chunk_node[k], pe = d.chunk_node[k + 1];
        if (pe <= pb) continue;
        if ((rc = weights_chunk(g, method, k, d.e2e_weights, d.e2e_nws, stream))) { drain(); return rc; }
        if ((rc = launch_row_nnz(d.v, d.e2e_weights, d.e2e_cnt, stream, pb, pe))) { drain(); return fail(rc, "launch failed"); }
        size_t tb = d.e2e_tmp_bytes;
        // ptr[pb .. pe] (one past the piece: the next piece's seed and, in the end, nnz); cnt[pe] is not part of that sum
        TRY_C(hipcub::DeviceScan::ExclusiveScan(d.e2e_tmp, tb, d.e2e_cnt + pb, d.e2e_ptr + pb, hipcub::Sum(), base, (int)(pe - pb + 1), stream));
        if ((rc = launch_compact(d.v, d.e2e_weights, d.e2e_ptr, d.e2e_indices, d.e2e_data, stream, pb, pe))) { drain(); return fail(rc, "launch failed"); }
        int32_t next_base = 0;
        TRY_C(hipMemcpyAsync(&next_base, d.e2e_ptr + pe, 4, hipMemcpyDeviceToHost, stream));
        TRY_C(hipEventRecord(ev, stream));
        TRY_C(hipStreamSynchronize(stream));             // (the piece is compacted; the copies of the piece before still run)
        const int64_t n_k = (int64_t)next_base - base;
        // this piece's slices: rows on the copy stream, entries split over two queues
        TRY_C(hipMemcpyAsync(indptr + pb, d.e2e_ptr + pb, (size_t)(pe - pb + (k == K - 1 ? 1 : 0)) * 4, hipMemcpyDeviceToHost, cs));
        TRY_C(hipMemcpyAsync(neumann_ws + pb, d.e2e_nws + pb, (size_t)(pe - pb) * 8, hipMemcpyDeviceToHost, cs));
        if (n_k > 0) {
            TRY_C(hipMemcpyAsync(data + base, d.e2e_data + base, (size_t)n_k * 8, hipMemcpyDeviceToHost, cs));
            if (!d.copy_stream2) {
                hipStream_t s2;
                TRY_C(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
                d.copy_stream2 = s2;
            }
            TRY_C(hipMemcpyAsync(indices + base, d.e2e_indices + base, (size_t)n_k * 4, hipMemcpyDeviceToHost,
                                 static_cast<hipStream_t>(d.copy_stream2)));
        }
        base = next_base;
        if (L.on) { char nm[32]; snprintf(nm, sizeof nm, "piece %d computed", k); L.lap(nm); }
    }
    TRY_C(hipStreamSynchronize(cs));
    if (d.copy_stream2) TRY_C(hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream2)));
    L.lap("copies drained");
    *nnz_out = base;
#undef TRY_C
    return NIN_OK;
}

}  // namespace

int nin_csr_compact_host(nin_grid *g, const double *dev_csr_data, int32_t *indptr, int32_t *indices, double *data,
                         int64_t *nnz_out, void *stream_) {
    if (!g || !dev_csr_data || !indptr || !nnz_out) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (d.device < 0) return fail(NIN_ENODEVICE, "grid is not on a device");
    HIP_TRY(hipSetDevice(d.device));
    return csr_compact_pipelined(g, dev_csr_data, nullptr, indptr, indices, data, nnz_out, nullptr,
                                 static_cast<hipStream_t>(stream_));
}

int nin_interpolate_csr_host(nin_grid *g, int method, int32_t *indptr, int32_t *indices, double *data,
                             int64_t *nnz_out, double *neumann_ws) {
    if (!g || !indptr || !indices || !data || !nnz_out || !neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (d.device < 0) return fail(NIN_ENODEVICE, "grid is not on a device: the weight kernels are HIP only");
    HIP_TRY(hipSetDevice(d.device));
    int rc = NIN_OK;
    if (!d.e2e_weights && (rc = dev_alloc(d, &d.e2e_weights, (size_t)std::max<int64_t>(d.nnz_e, 1)))) return rc;
    if (!d.e2e_nws && (rc = dev_alloc(d, &d.e2e_nws, (size_t)std::max<int64_t>(g->h.n_points, 1)))) return rc;
    if (d.chunkable) {
        if (!d.fields_set) return fail(NIN_ESTATE, "nin_fields_set has not been called");
        if (method != NIN_METHOD_GLS && method != NIN_METHOD_IDW && method != NIN_METHOD_LS) return fail(NIN_EINVAL, "unknown method %d", method);
        if (method == NIN_METHOD_GLS && !d.have_perm) return fail(NIN_ESTATE, "GLS needs permeability and diff_mag");
        if (method == NIN_METHOD_GLS && d.gls_too_large)
            return fail(NIN_ERANGE, "a node's GLS system has more than 1024 rows (more than ~100 cells around one node): beyond the fallback kernel");
        return interpolate_chunked(g, method, indptr, indices, data, nnz_out, neumann_ws);
    }
    rc = nin_weights_device(g, method, nullptr, 0, 1, d.e2e_weights, d.e2e_nws, nullptr);
    if (!rc) rc = csr_compact_pipelined(g, d.e2e_weights, d.e2e_nws, indptr, indices, data, nnz_out, neumann_ws, nullptr);
    return rc;
}

// ---- a host matrix kept current: only the dirty rows cross PCIe (csr_dirty.hip, csr_patch.cpp) ----------------------
struct nin_hostmatrix {
    nin_grid *g = nullptr;
    int method = 0;
    int device = -1;                // the grid's, as it was at creation: nin_hostmatrix_destroy does not look at the grid, which may be gone
    // the matrix's own device state: weights in esup position, neumann_ws, surviving entries per row (not the grid's e2e_* scratch,
    // which any interpolate() overwrites)
    double *weights = nullptr, *nws = nullptr;
    int32_t *cnt = nullptr;
    bool weights_current = false;   // nin_hostmatrix_update found every node dirty and ran the full launch: nin_hostmatrix_full finishes it
    // scratch of an update, sized by the dirty list and grown on demand: per listed row (pack_off has two more: the total and the
    // counter of rows whose count changed, read back together) and per packed entry; the same again page-locked on the host
    size_t rows_cap = 0, entries_cap = 0, h_rows_cap = 0, h_entries_cap = 0;
    int32_t *pack_cnt = nullptr, *pack_off = nullptr, *pack_node = nullptr, *pack_indices = nullptr;
    double *pack_nws = nullptr, *pack_data = nullptr;
    void *scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
    int32_t *h_cnt = nullptr, *h_off = nullptr, *h_node = nullptr, *h_indices = nullptr;
    double *h_nws = nullptr, *h_data = nullptr;
    int64_t pending_rows = -1;      // rows of the last update whose pack is on its way to the host (nin_hostmatrix_patch takes them)
};

namespace {

struct HmLaps {   // NIN_TIMING=1: the phases of one update on stderr; each lap then waits for the work it names
    bool on = getenv("NIN_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what, std::initializer_list<hipStream_t> wait_for) {
        if (!on) return;
        for (hipStream_t s : wait_for) (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[nin_hostmatrix] %-14s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

extern "C++" {
template <class T>
int hm_grow(T **buf, size_t count, bool on_host) {
    if (*buf) (void)(on_host ? hipHostFree(*buf) : hipFree(*buf));
    *buf = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    const hipError_t e = on_host ? hipHostMalloc((void **)buf, bytes, hipHostMallocDefault) : hipMalloc((void **)buf, bytes);
    return e == hipSuccess ? NIN_OK : fail(NIN_ENOMEM, "%s(%zu bytes): %s", on_host ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
}
}

// room for `rows` listed rows and `entries` packed entries, on the device or in page-locked host memory (half as much again: a time
// loop's dirty set wobbles).  Growing frees first, which waits for the device: nothing of an earlier update is in flight by then.
int hm_reserve(nin_hostmatrix *m, size_t rows, size_t entries, bool on_host) {
    size_t &rc_ = on_host ? m->h_rows_cap : m->rows_cap, &ec_ = on_host ? m->h_entries_cap : m->entries_cap;
    int rc = NIN_OK;
    if (rows > rc_) {
        const size_t n = rows + rows / 2;
        rc_ = 0;
        if (!rc) rc = hm_grow(on_host ? &m->h_cnt : &m->pack_cnt, n + 1, on_host);
        if (!rc) rc = hm_grow(on_host ? &m->h_off : &m->pack_off, n + 2, on_host);
        if (!rc) rc = hm_grow(on_host ? &m->h_node : &m->pack_node, n, on_host);
        if (!rc) rc = hm_grow(on_host ? &m->h_nws : &m->pack_nws, n, on_host);
        if (rc) return rc;
        rc_ = n;
    }
    if (entries > ec_ || !(on_host ? m->h_data : m->pack_data)) {
        const size_t n = entries + entries / 2;
        ec_ = 0;
        if (!rc) rc = hm_grow(on_host ? &m->h_indices : &m->pack_indices, n, on_host);
        if (!rc) rc = hm_grow(on_host ? &m->h_data : &m->pack_data, n, on_host);
        if (rc) return rc;
        ec_ = n;
    }
    return NIN_OK;
}

}  // namespace

int nin_hostmatrix_create(nin_grid *g, int method, nin_hostmatrix **out) {
    if (!g || !out) return fail(NIN_EINVAL, "NULL argument");
    *out = nullptr;
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first)");
    if (method != NIN_METHOD_GLS && method != NIN_METHOD_IDW && method != NIN_METHOD_LS) return fail(NIN_EINVAL, "unknown method %d", method);
    HIP_TRY(hipSetDevice(d.device));
    nin_hostmatrix *m = new (std::nothrow) nin_hostmatrix();
    if (!m) return fail(NIN_ENOMEM, "out of host memory");
    m->g = g;
    m->method = method;
    m->device = d.device;
    int rc = hm_grow(&m->weights, (size_t)d.nnz_e, false);
    if (!rc) rc = hm_grow(&m->nws, (size_t)g->h.n_points, false);
    if (!rc) rc = hm_grow(&m->cnt, (size_t)g->h.n_points, false);
    if (rc) { nin_hostmatrix_destroy(m); return rc; }
    *out = m;
    return NIN_OK;
}

void nin_hostmatrix_destroy(nin_hostmatrix *m) {
    if (!m) return;
    if (m->device >= 0) (void)hipSetDevice(m->device);
    for (void *p : {(void *)m->weights, (void *)m->nws, (void *)m->cnt, (void *)m->pack_cnt, (void *)m->pack_off, (void *)m->pack_node,
                    (void *)m->pack_indices, (void *)m->pack_nws, (void *)m->pack_data, m->scan_tmp})
        if (p) (void)hipFree(p);   // (waits for the device)
    for (void *p : {(void *)m->h_cnt, (void *)m->h_off, (void *)m->h_node, (void *)m->h_indices, (void *)m->h_nws, (void *)m->h_data})
        if (p) (void)hipHostFree(p);
    delete m;
}

int nin_hostmatrix_full(nin_hostmatrix *m, int32_t *indptr, int32_t *indices, double *data, double *neumann_ws, int64_t *nnz_out,
                        void *stream_) {
    if (!m || !indptr || !indices || !data || !neumann_ws || !nnz_out) return fail(NIN_EINVAL, "NULL argument");
    nin_grid *g = m->g;
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device: the weight kernels are HIP only");
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = NIN_OK;
    if (!m->weights_current) {   // (else nin_hostmatrix_update has run the launch and cleared the set)
        if ((rc = nin_weights_device(g, m->method, nullptr, 0, 1, m->weights, m->nws, stream_))) return rc;
        if ((rc = nin_grid_dirty_reset(g, 0, stream_))) return rc;
    }
    m->weights_current = false;
    m->pending_rows = -1;
    // the existing finish: count, scan and compaction in the grid's scratch, the transfers under them; the row counts stay with the matrix
    rc = csr_compact_pipelined(g, m->weights, m->nws, indptr, indices, data, nnz_out, neumann_ws, stream);
    if (!rc) {
        const hipError_t e = hipMemcpyAsync(m->cnt, d.e2e_cnt, (size_t)g->h.n_points * sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) rc = fail(NIN_EHIP, "keeping the row counts: %s", hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess && !rc) rc = fail(NIN_EHIP, "full run of the host matrix: %s", hipGetErrorString(e));
    if (rc) d.all_dirty = true;   // the matrix holds no full result: the next update starts over
    return rc;
}

int nin_hostmatrix_update(nin_hostmatrix *m, int clear, void *stream_, int64_t *n_rows, int64_t *n_changed, int64_t *n_entries) {
    if (!m || !n_rows || !n_changed || !n_entries) return fail(NIN_EINVAL, "NULL argument");
    *n_rows = *n_changed = *n_entries = 0;
    nin_grid *g = m->g;
    DeviceGrid &d = g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (m->pending_rows >= 0) {   // an update nobody patched in: its copies must not be in flight when the staging buffers are reused
        (void)hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream));
        (void)hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream2));
        m->pending_rows = -1;
        d.all_dirty = true;       // ... and the host's arrays missed those rows
    }
    const bool full = d.all_dirty;
    HmLaps L;
    int64_t n = 0;
    // refused ids: nothing is launched, the matrix and the set stay as they are (nin_weights_dirty_device's contract)
    int rc = nin_weights_dirty_device(g, m->method, 1, m->weights, m->nws, stream_, clear, &n);
    if (rc) return rc;
    *n_rows = n;
    if (full) {   // every row was launched: the ordinary finish follows (nin_hostmatrix_full)
        m->weights_current = true;
        *n_entries = -1;
        return NIN_OK;
    }
    if (n == 0) return NIN_OK;
    L.lap("dirty launch", {stream});
    const int32_t total = (int32_t)n;
    // what the rows of the list can hold at most: the pack's size is not known on the host before the kernels that fill it are enqueued
    const size_t bound = (size_t)std::min<int64_t>(n * std::max<int64_t>(g->h.mx_elems_per_point, 1), d.nnz_e);
    size_t tmp_bytes = 0;
    int32_t back[2] = {0, 0};   // pack_off[total] = the packed entries, pack_off[total + 1] = the rows whose count changed
    auto step = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && !rc) rc = fail(NIN_EHIP, "%s: %s", what, hipGetErrorString(e));
        return rc == NIN_OK;
    };
    rc = hm_reserve(m, (size_t)total, bound, false);
    if (!rc) rc = e2e_streams(d);
    if (!rc && !d.copy_stream2) {
        hipStream_t s2 = nullptr;
        if (step(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking), "hipStreamCreate")) d.copy_stream2 = s2;
    }
    hipStream_t cs = static_cast<hipStream_t>(d.copy_stream), cs2 = static_cast<hipStream_t>(d.copy_stream2);
    hipEvent_t ev_scan = static_cast<hipEvent_t>(d.ev_scan), ev_pack = static_cast<hipEvent_t>(d.ev_weights);
    if (!rc && step(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, m->pack_cnt, m->pack_off, total + 1, stream), "sizing the scan") &&
        tmp_bytes > m->scan_tmp_bytes) {
        m->scan_tmp_bytes = 0;
        if (!(rc = hm_grow(reinterpret_cast<char **>(&m->scan_tmp), std::max<size_t>(tmp_bytes, 16), false))) m->scan_tmp_bytes = std::max<size_t>(tmp_bytes, 16);
    }
    if (!rc) {
        (void)(step(hipMemsetAsync(m->pack_cnt + total, 0, sizeof(int32_t), stream), "hipMemsetAsync") &&
               step(hipMemsetAsync(m->pack_off + total + 1, 0, sizeof(int32_t), stream), "hipMemsetAsync"));
        if (!rc && launch_dirty_row_nnz(d.v, m->weights, d.dirty_lists, total, m->pack_cnt, m->cnt, m->pack_off + total + 1, stream))
            rc = fail(NIN_EHIP, "row count kernel: %s", hipGetErrorString(hipGetLastError()));
        size_t tb = m->scan_tmp_bytes;
        // the sizes leave on the copy stream as soon as the scan is done, under the pack kernel: the call's second and last wait
        (void)(step(hipcub::DeviceScan::ExclusiveSum(m->scan_tmp, tb, m->pack_cnt, m->pack_off, total + 1, stream), "scan of the row counts") &&
               step(hipEventRecord(ev_scan, stream), "hipEventRecord") && step(hipStreamWaitEvent(cs, ev_scan, 0), "hipStreamWaitEvent") &&
               step(hipMemcpyAsync(back, m->pack_off + total, sizeof back, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync"));
        if (!rc && launch_dirty_pack(d.v, m->weights, m->nws, d.dirty_lists, total, m->pack_off, m->pack_node, m->pack_nws, m->pack_indices,
                                     m->pack_data, stream))
            rc = fail(NIN_EHIP, "pack kernel: %s", hipGetErrorString(hipGetLastError()));
        (void)(step(hipEventRecord(ev_pack, stream), "hipEventRecord") && step(hipStreamSynchronize(cs), "reading the pack's size back"));
    }
    if (!rc && (back[0] < 0 || (size_t)back[0] > bound || back[1] < 0 || back[1] > total))
        rc = fail(NIN_EHIP, "the pack holds %d entries (room for %zu) and %d changed rows of %d", (int)back[0], bound, (int)back[1], (int)total);
    L.lap("count + pack", {stream});
    if (!rc) rc = hm_reserve(m, (size_t)total, (size_t)back[0], true);
    if (!rc) {
        const size_t rows = (size_t)total, ents = (size_t)back[0];
        (void)(step(hipStreamWaitEvent(cs, ev_pack, 0), "hipStreamWaitEvent") && step(hipStreamWaitEvent(cs2, ev_pack, 0), "hipStreamWaitEvent") &&
               step(hipMemcpyAsync(m->h_node, m->pack_node, rows * 4, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync") &&
               step(hipMemcpyAsync(m->h_cnt, m->pack_cnt, rows * 4, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync") &&
               step(hipMemcpyAsync(m->h_off, m->pack_off, (rows + 1) * 4, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync") &&
               step(hipMemcpyAsync(m->h_nws, m->pack_nws, rows * 8, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync"));
        if (!rc && ents)   // two copy queues, as interpolate()'s pipeline: the index and the value stream each keep a DMA engine busy
            (void)(step(hipMemcpyAsync(m->h_data, m->pack_data, ents * 8, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync") &&
                   step(hipMemcpyAsync(m->h_indices, m->pack_indices, ents * 4, hipMemcpyDeviceToHost, cs2), "hipMemcpyAsync"));
    }
    if (rc) {   // rows were rewritten on the device that the host will not get: everything counts as dirty again
        (void)hipStreamSynchronize(stream); (void)hipStreamSynchronize(cs);
        if (cs2) (void)hipStreamSynchronize(cs2);
        d.all_dirty = true;
        return rc;
    }
    L.lap("D2H", {cs, cs2});
    m->pending_rows = total;
    *n_changed = back[1];
    *n_entries = back[0];
    return NIN_OK;
}

int nin_hostmatrix_patch(nin_hostmatrix *m, const int32_t *indptr, int32_t *indices, double *data, double *neumann_ws, int32_t *out_indptr,
                         int32_t *out_indices, double *out_data) {
    if (!m || !indptr || !indices || !data || !neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    if (m->pending_rows < 0) return fail(NIN_ESTATE, "no update is waiting to be patched in (nin_hostmatrix_update first)");
    DeviceGrid &d = m->g->d;
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream2)));
    HmLaps L;
    const int64_t rows = m->pending_rows;
    m->pending_rows = -1;
    const int rc = nin_csr_patch_rows(m->g->h.n_points, indptr, indices, data, neumann_ws, rows, m->h_node, m->h_cnt, m->h_off, m->h_indices,
                                      m->h_data, m->h_nws, out_indptr, out_indices, out_data);
    L.lap("host patch", {});
    if (rc) {
        d.all_dirty = true;   // the device is ahead of the host's arrays
        return fail(rc, rc == NIN_ERANGE ? "the patched matrix has more entries than int32 indices hold"
                                         : "the packed rows do not fit the matrix they are patched into (out_* missing for a new structure, or other arrays)");
    }
    return NIN_OK;
}

// Give the grid's call scratch back (the buffers nin_interpolate_csr_host / nin_csr_compact_host / nin_apply_* allocate
// on first use and keep: ~2.3 GB of HBM at 10 M cells, + 10 MB of page-locked host memory; the transpose index, 0.69 GB more);
// the next call allocates again.
static void release_adjoint_state(DeviceGrid &d);   // (with the adjoint, below)
int nin_grid_release_scratch(nin_grid *g) {
    if (!g) return fail(NIN_EINVAL, "NULL grid");
    DeviceGrid &d = g->d;
    if (d.device < 0) return NIN_OK;
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(hipDeviceSynchronize());
    void *scratch[] = {d.e2e_weights, d.e2e_nws, d.e2e_data, d.e2e_cnt, d.e2e_ptr, d.e2e_indices, d.e2e_tmp, d.apply_weights,
                       d.tr_cell_ptr, d.tr_cell_pos, d.tr_cell_node};
    for (void *p : scratch) dev_release(d, p);
    d.e2e_weights = d.e2e_nws = d.e2e_data = nullptr;
    d.e2e_cnt = d.e2e_ptr = d.e2e_indices = nullptr;
    d.e2e_tmp = nullptr;
    d.e2e_tmp_bytes = 0;
    d.apply_weights = nullptr;
    d.tr_cell_ptr = d.tr_cell_pos = d.tr_cell_node = nullptr;
    release_adjoint_state(d);   // the GLS adjoint's bins, contribution buffer and scratch slots
    // a dirty launch's lists, histogram, scan temporary and descriptors (the marks themselves and their header are state: they stay)
    for (void *p : {(void *)d.dirty_lists, (void *)d.dirty_hist, d.dirty_tmp, (void *)d.dirty_desc}) dev_release(d, p);
    d.dirty_lists = d.dirty_hist = nullptr;
    d.dirty_tmp = nullptr;
    d.dirty_desc = nullptr;
    d.dirty_tmp_bytes = d.dirty_desc_words = 0;
    if (d.flag_staging) { (void)hipHostFree(d.flag_staging); d.flag_staging = nullptr; }
    // the connectivity copies of nin_grid_update_points*: kept while the device builder's mirror still fetches from them (they were its
    // own before the first update: no HBM is held that the grid did not hold anyway)
    if (d.up_inpoel && !(g->h.lazy && g->h.lazy->reads(d.up_inpoel))) {
        std::string err;   // the face areas live nowhere else on the device: to the host first, if the host copy is the old mesh's
        if (g->h.ensure(A_AREAS, &err)) return fail(NIN_EHIP, "mirroring faces_areas: %s", err.c_str());
        dev_release(d, d.up_inpoel); dev_release(d, d.up_etype); dev_release(d, d.up_inpofa); dev_release(d, d.up_areas);
        d.up_inpoel = d.up_inpofa = nullptr;
        d.up_etype = nullptr;
        d.up_areas = nullptr;
        d.up_areas_valid = false;
    }
    return NIN_OK;
}

int nin_apply_device(nin_grid *g, int method, const double *dev_u_cells, int32_t n_fields, double *dev_node_values,
                     double *dev_neumann_ws, void *stream_) {
    if (!g || !dev_u_cells || !dev_node_values || !dev_neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device: the weight kernels are HIP only");
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!d.apply_weights) {   // the weights of the last apply: one buffer per grid, allocated on first use
        int rc = dev_alloc(d, &d.apply_weights, (size_t)std::max<int64_t>(d.nnz_e, 1));
        if (rc) return rc;
    }
    // GLS on a mesh with cube nodes: the cube-node kernel forms W . u itself (the 64 bytes of a node's row are neither written
    // nor read again); the other kernels write their rows as always and a list kernel applies those (NIN_APPLY_NO_FUSION: off)
    const DeviceGrid::GlsList &cube = d.plan[gk::hex8];
    if (method == NIN_METHOD_GLS && cube.count > 0 && d.noncube_nodes_ready && getenv("NIN_APPLY_NO_FUSION") == nullptr) {
        if (!d.fields_set) return fail(NIN_ESTATE, "nin_fields_set has not been called");
        if (!d.have_perm) return fail(NIN_ESTATE, "GLS needs permeability and diff_mag");
        if (d.gls_too_large) return fail(NIN_ERANGE, "a node's GLS system has more than 1024 rows: beyond the fallback kernel");
        HIP_TRY(hipMemsetAsync(d.gls_queue, 0, kGlsQueueInts * sizeof(int32_t), stream));
        int rc = gls_side_begin(d, -1, 1, d.apply_weights, dev_neumann_ws, stream);
        if (!rc) rc = launch_gls_hex8mf_apply(d.v, cube.nodes, reinterpret_cast<const int32_t *>(cube.desc), cube.count, 1, dev_u_cells, n_fields,
                                              dev_node_values, dev_neumann_ws, d.gls_queue + gls_plan_row(gk::hex8).counter, stream);
        if (!rc) rc = gls_main(d, -1, false, gls_only(), 1, d.apply_weights, dev_neumann_ws, stream);
        if (!rc) rc = launch_apply_list(d.v, d.apply_weights, dev_u_cells, n_fields, dev_node_values, d.noncube_nodes, d.noncube_count, stream);
        if (rc) return fail(rc, "launch failed: %s", hipGetErrorString(hipGetLastError()));
        return NIN_OK;
    }
    // the weights are computed ONCE, whatever the number of fields (they depend on the mesh, the permeability and the
    // Neumann flags only: the reference's callers do `weights.dot(u)` per field with the same matrix)
    int rc = nin_weights_device(g, method, nullptr, 0, 1, d.apply_weights, dev_neumann_ws, stream_);
    if (rc) return rc;
    rc = n_fields == 1 ? launch_apply(d.v, d.apply_weights, dev_u_cells, dev_node_values, (int32_t)g->h.mx_elems_per_point, d.nnz_e, stream)
                       : launch_apply_fields(d.v, d.apply_weights, dev_u_cells, n_fields, dev_node_values, (int32_t)g->h.mx_elems_per_point, d.nnz_e, stream);
    if (rc) return fail(rc, "launch failed");
    return NIN_OK;
}

int nin_apply_fields_host(nin_grid *g, int method, const double *u_cells, int32_t n_fields, double *node_values,
                          double *neumann_ws) {
    if (!g || !u_cells || !node_values || !neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (d.device < 0) return fail(NIN_ENODEVICE, "grid is not on a device: the weight kernels are HIP only");
    HIP_TRY(hipSetDevice(d.device));
    const size_t pb = (size_t)g->h.n_points * 8, eb = (size_t)g->h.n_elems * 8;
    double *dn = nullptr, *du = nullptr, *dv = nullptr;
    auto cleanup = [&]() { (void)hipFree(dn); (void)hipFree(du); (void)hipFree(dv); };
#define TRY_A(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { cleanup(); return fail(NIN_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); } } while (0)
    TRY_A(hipMalloc((void **)&dn, pb));
    TRY_A(hipMalloc((void **)&du, eb * n_fields));
    TRY_A(hipMalloc((void **)&dv, pb * n_fields));
    TRY_A(hipMemcpy(du, u_cells, eb * n_fields, hipMemcpyHostToDevice));
    const int rc = nin_apply_device(g, method, du, n_fields, dv, dn, nullptr);
    if (rc) { cleanup(); return rc; }
    TRY_A(hipMemcpy(node_values, dv, pb * n_fields, hipMemcpyDeviceToHost));
    TRY_A(hipMemcpy(neumann_ws, dn, pb, hipMemcpyDeviceToHost));
#undef TRY_A
    cleanup();
    return NIN_OK;
}

int nin_apply_host(nin_grid *g, int method, const double *u_cells, double *node_values, double *neumann_ws) {
    return nin_apply_fields_host(g, method, u_cells, 1, node_values, neumann_ws);
}

int nin_spmv_device(nin_grid *g, const double *dev_csr_data, const double *dev_u_cells, int32_t n_fields, double *dev_node_values,
                    void *stream_) {
    if (!g || !dev_csr_data || !dev_u_cells || !dev_node_values) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device: the kernels are HIP only");
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // the kernels nin_apply_device runs after its weights, on the caller's weights
    const int rc = n_fields == 1 ? launch_apply(d.v, dev_csr_data, dev_u_cells, dev_node_values, (int32_t)g->h.mx_elems_per_point, d.nnz_e, stream)
                                 : launch_apply_fields(d.v, dev_csr_data, dev_u_cells, n_fields, dev_node_values, (int32_t)g->h.mx_elems_per_point,
                                                       d.nnz_e, stream);
    if (rc) return fail(rc, "launch failed: %s", hipGetErrorString(hipGetLastError()));
    return NIN_OK;
}

int nin_spmv_transpose_device(nin_grid *g, const double *dev_csr_data, const double *dev_node_values, int32_t n_fields,
                              double *dev_cell_values, void *stream_) {
    if (!g || !dev_csr_data || !dev_node_values || !dev_cell_values) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device: the kernels are HIP only");
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = ensure_transpose_index(d, stream);
    if (rc) return rc;
    rc = launch_apply_transpose(d.v, d.tr_cell_ptr, d.tr_cell_pos, d.tr_cell_node, d.v.dim == 2 ? 4 : 8, dev_csr_data, dev_node_values,
                                n_fields, dev_cell_values, stream);
    if (rc) return fail(rc, "launch failed: %s", hipGetErrorString(hipGetLastError()));
    return NIN_OK;
}

int nin_apply_transpose_fields_host(nin_grid *g, int method, const double *node_values, int32_t n_fields, double *cell_values) {
    if (!g || !node_values || !cell_values) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device: the weight kernels are HIP only");
    if (!d.fields_set) return fail(NIN_ESTATE, "nin_fields_set has not been called");
    if (method != NIN_METHOD_GLS && method != NIN_METHOD_IDW && method != NIN_METHOD_LS) return fail(NIN_EINVAL, "unknown method %d", method);
    if (method == NIN_METHOD_GLS && !d.have_perm) return fail(NIN_ESTATE, "GLS needs permeability and diff_mag");
    HIP_TRY(hipSetDevice(d.device));
    if (!d.apply_weights) {   // the weights of the last apply: one buffer per grid, allocated on first use
        int rc = dev_alloc(d, &d.apply_weights, (size_t)std::max<int64_t>(d.nnz_e, 1));
        if (rc) return rc;
    }
    const size_t pb = (size_t)g->h.n_points * 8, eb = (size_t)g->h.n_elems * 8;
    double *dn = nullptr, *dv = nullptr, *dx = nullptr;
    auto cleanup = [&]() { (void)hipFree(dn); (void)hipFree(dv); (void)hipFree(dx); };
#define TRY_A(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { cleanup(); return fail(NIN_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); } } while (0)
    TRY_A(hipMalloc((void **)&dn, pb));
    TRY_A(hipMalloc((void **)&dv, pb * n_fields));
    TRY_A(hipMalloc((void **)&dx, eb * n_fields));
    TRY_A(hipMemcpy(dv, node_values, pb * n_fields, hipMemcpyHostToDevice));
    // the unfused weights (the fused cube-node apply writes no rows for cube nodes), with `+ neumann_ws[row]` as apply() uses them
    int rc = nin_weights_device(g, method, nullptr, 0, 1, d.apply_weights, dn, nullptr);
    if (!rc) rc = nin_spmv_transpose_device(g, d.apply_weights, dv, n_fields, dx, nullptr);
    if (rc) { cleanup(); return rc; }
    TRY_A(hipMemcpy(cell_values, dx, eb * n_fields, hipMemcpyDeviceToHost));
#undef TRY_A
    cleanup();
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

// ---- algorithmic flops of a launch plan, kernel by kernel (tools/count_algorithmic_flops.py holds the same formulas) ----
namespace {
// n_pivot Householder steps on an m-row block with n_cols columns in all (pivot columns included): 2 m for the norm, 8 for the
// scalar chain, 4 m per trailing column (dot + update)
double hh_flops(int64_t m, int64_t n_pivot, int64_t n_cols) {
    double f = 0;
    for (int64_t k = 0; k < n_pivot; ++k) {
        const double rows = (double)(m - k);
        f += 2 * rows + 8 + 4 * rows * (double)(n_cols - k - 1);
    }
    return f;
}
// fronts of 3-face cells + a dense rest (kernels_gls_hex8mf / mfw / mfx): F fronts, D dense cells, `faces` internal faces of which
// `free_faces` join two dense cells
double multifrontal_flops(int64_t F, int64_t D, int64_t faces, int64_t free_faces, int64_t neumann_rows = 0) {
    const double face = 52.0 * faces + 15.0 * neumann_rows;
    const double p1 = F * (hh_flops(10, 3, 3 + 9 + 1) + 9 + 54 + 6);
    const int64_t m2 = 7 * F + D + 3 * free_faces + neumann_rows, n2 = 3 * D;
    const double p2 = hh_flops(m2, n2, n2 + 1);
    const double tail = (double)n2 * n2 + F * (2 * 9 + 2) + D * (2 * 3 + 1) + 2 * (m2 - n2) + (F + D) + 1;
    return face + p1 + p2 + tail;
}
// the dense m x (n + 1) system with the last-row identity (one Householder QR of the first n columns, no right-hand sides):
// the small-node, block (one wavefront) and global-scratch kernels; n_if internal faces, n_nb Neumann rows
double dense_flops(int64_t ne, int64_t n_if, int64_t n_nb) {
    const int64_t m = ne + 3 * n_if + n_nb, n = 3 * ne;
    return 52.0 * n_if + 15.0 * n_nb + hh_flops(m, n, n + 1) + (double)n * n + 7.0 * ne + 2.0 * (m - n) + ne + 1;
}
// dgels on the reference's dense m x n system with nrhs right-hand sides
double dgels_flops(double m, double n, double nrhs) { return 2 * m * n * n - 2 * n * n * n / 3 + nrhs * (4 * m * n - 2 * n * n) + nrhs * n * n; }
}  // namespace

int nin_gls_plan_flops(nin_grid *g, double alg[22], double ref[22], int64_t computed[22]) {
    if (!g || !alg || !ref || !computed) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    HostGrid &h = g->h;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first)");
    if (!d.fields_set || (!d.flag_staging && !d.flags_host_stale))
        return fail(NIN_ESTATE, "nin_fields_set has not been called (the Neumann flags decide which boundary nodes are computed)");
    if (h.ensure(A_ESUP_PTR | A_ESUP | A_FSUP_PTR | A_FSUP | A_ESUF)) return fail(NIN_EHIP, "mirroring the connectivity failed");
    HIP_TRY(hipSetDevice(d.device));
    {   // after an update of the flags from device memory the host's copy of the bytes is fetched again (waits for the device)
        const int frc = fetch_flag_bytes(g);
        if (frc) return frc;
    }
    for (int k = 0; k < kGlsPlanKernels; ++k) { alg[k] = ref[k] = 0.0; computed[k] = 0; }
    const int64_t P = h.n_points;
    // (F, D, free faces) of the nodes of the multifrontal kernels: the low 24 bits of the descriptor word the plan's table names
    std::vector<uint32_t> fdq((size_t)P, 0u);
    for (int k = 0; k < kGlsPlanKernels; ++k) {
        const GlsPlanRow row = gls_plan_row(k);
        const auto &l = d.plan[k];
        if (row.fdq_word < 0 || l.count <= 0) continue;
        std::vector<int32_t> hn((size_t)l.count);
        std::vector<uint32_t> hd((size_t)l.count * row.desc_words);
        if (hipMemcpy(hn.data(), l.nodes, hn.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hd.data(), l.desc, hd.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(NIN_EHIP, "reading the descriptors back failed");
        for (int32_t i = 0; i < l.count; ++i) fdq[hn[i]] = hd[(size_t)i * row.desc_words + row.fdq_word] & 0xFFFFFFu;
    }
    for (int64_t p = 0; p < P; ++p) {
        const int k = gls_class_kernel(g->node_class[p]);
        const GlsPlanRow row = gls_plan_row(k);
        const int fl = d.flag_staging[p];
        if ((fl & 1) && !(fl & 2)) continue;                   // a Dirichlet boundary node: the zero row, nothing computed (gls.pyx:165-166)
        const int64_t eb = h.esup_ptr[p], ne = h.esup_ptr[p + 1] - eb, fb = h.fsup_ptr[p], nf = h.fsup_ptr[p + 1] - fb;
        int64_t n_if = 0;
        for (int64_t q = fb; q < fb + nf; ++q) {
            const int64_t f = h.fsup[q];
            n_if += h.esuf_ptr[f + 1] - h.esuf_ptr[f] > 1;
        }
        const int64_t n_bf = nf - n_if, n_nb = (fl & 2) ? n_bf : 0;
        const int64_t m = ne + 3 * n_if + n_nb;
        if (n_if == 0 || m < 3 * ne) continue;                 // outside the parity set: the zero row
        ++computed[k];
        ref[k] += dgels_flops((double)(ne + 3 * nf + n_nb), (double)(3 * ne + 1), (double)(ne + (n_nb ? 1 : 0)));
        if (k == gk::hex8) alg[k] += multifrontal_flops(4, 4, 12, 0);
        else if (row.fdq_word >= 0) {   // the multifrontal kernels with descriptors; all but the one-wavefront kernel take Neumann rows
            const uint32_t w = fdq[p];
            alg[k] += multifrontal_flops(w & 255u, (w >> 8) & 255u, n_if, (w >> 16) & 255u, row.family != GlsFamily::mfw ? n_nb : 0);
        } else if (k == gk::quad4) {
            // two fronts of 8 rows (cell row, two internal faces, the Neumann row) x (3 | 6 | c), then 14 x 6 over the pair
            alg[k] += 52.0 * 4 + 15.0 * 4 + 2 * (hh_flops(8, 3, 3 + 6 + 1) + 9 + 36 + 6) + hh_flops(14, 6, 7) + 36 + 2 * 20 + 2 * 7 + 2 * 8 + 5;
        } else if (k >= gk::block2 && k <= gk::block8) {
            // the block kernel on more than one wavefront: fronts = the greedy independent set (esup order) of the cells with 1 .. 4
            // internal faces at the node that own no Neumann row; a front of a cell with f faces is (1 + 3 f) x (3 + 3 f + 1)
            const int n_c = (int)std::min<int64_t>(ne, 64);
            uint64_t adj[64] = {0};
            int nfi[64] = {0};
            uint64_t blocked = 0;
            for (int64_t q = fb; q < fb + nf; ++q) {
                const int64_t f = h.fsup[q], e0 = h.esuf_ptr[f];
                const bool internal = h.esuf_ptr[f + 1] - e0 > 1;
                int ia = -1, ib = -1;
                for (int i = 0; i < n_c; ++i) {
                    if (h.esup[eb + i] == h.esuf[e0]) ia = i;
                    if (internal && h.esup[eb + i] == h.esuf[e0 + 1]) ib = i;
                }
                if (internal && ia >= 0 && ib >= 0) { adj[ia] |= 1ull << ib; adj[ib] |= 1ull << ia; ++nfi[ia]; ++nfi[ib]; }
                else if (!internal && ia >= 0 && n_nb) blocked |= 1ull << ia;
            }
            uint64_t chosen = 0;
            double p1 = 0;
            int64_t rows_gone = 0, Fb = 0;
            for (int i = 0; i < n_c; ++i)
                if (nfi[i] >= 1 && nfi[i] <= 4 && !((blocked >> i) & 1ull) && !(adj[i] & chosen)) {
                    chosen |= 1ull << i;
                    p1 += hh_flops(1 + 3 * nfi[i], 3, 3 + 3 * nfi[i] + 1);
                    rows_gone += 3;
                    ++Fb;
                }
            const int64_t m2 = m - rows_gone, n2 = 3 * (ne - Fb);
            alg[k] += 52.0 * n_if + 15.0 * n_nb + p1 + hh_flops(m2, n2, n2 + 1) + (double)(3 * ne) * (3 * ne) + 7.0 * ne + 2.0 * (m - 3 * ne) + ne + 1;
        } else {
            alg[k] += dense_flops(ne, n_if, n_nb);             // small-node kernel, block kernel on one wavefront, global scratch
        }
    }
    return NIN_OK;
}

// ---- the GLS adjoint: dL/dK from dL/d(stored weights) (kernels_gls_adjoint.hip) ---------------------------------------
static void release_adjoint_state(DeviceGrid &d) {
    for (auto &b : d.adj_bin) { dev_release(d, b.nodes); b = DeviceGrid::AdjBin{}; }
    dev_release(d, d.adj_contrib);
    dev_release(d, d.adj_scratch);
    d.adj_contrib = d.adj_scratch = nullptr;
    d.adj_scratch_stride = 0;
    d.adj_scratch_slots = 0;
    d.adj_ready = false;
}

// The bins, the contribution buffer and the scratch slots, on first use.  Synchronises `stream` (one device-to-host copy of 8 bytes a node).
static int ensure_adjoint_state(DeviceGrid &d, hipStream_t stream) {
    if (d.adj_ready) return NIN_OK;
    const int32_t P = d.v.n_points;
    const bool force_global = getenv("NIN_GLS_ADJ_FORCE_GLOBAL") != nullptr;   // testing switch: every system in global scratch
    std::vector<int64_t> bytes((size_t)std::max(P, 1));
    {
        int64_t *dev_bytes = nullptr;
        HIP_TRY(hipMalloc((void **)&dev_bytes, bytes.size() * sizeof(int64_t)));
        hipError_t e = launch_adjoint_bytes(d.v, dev_bytes, stream) ? hipErrorLaunchFailure : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e == hipSuccess && P > 0) e = hipMemcpy(bytes.data(), dev_bytes, (size_t)P * sizeof(int64_t), hipMemcpyDeviceToHost);
        (void)hipFree(dev_bytes);
        if (e != hipSuccess) return fail(NIN_EHIP, "adjoint bins: %s", hipGetErrorString(e));
    }
    std::vector<int32_t> lists[kAdjBins];
    int64_t mx[kAdjBins] = {};
    for (int32_t p = 0; p < P; ++p) {
        const int b = adj_node_bin(bytes[p], force_global);
        lists[b].push_back(p);
        mx[b] = std::max(mx[b], bytes[p]);
    }
    int rc = NIN_OK;
    for (int b = 0; b < kAdjBins && !rc; ++b) {
        DeviceGrid::AdjBin &bin = d.adj_bin[b];
        bin.count = (int32_t)lists[b].size();
        bin.bytes = mx[b];
        if (bin.count == 0) continue;
        rc = dev_alloc(d, &bin.nodes, lists[b].size());
        if (!rc && hipMemcpy(bin.nodes, lists[b].data(), lists[b].size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(NIN_EHIP, "adjoint bins: upload failed");
    }
    if (!rc) rc = dev_alloc(d, &d.adj_contrib, (size_t)std::max<int64_t>(d.nnz_e, 1) * 10);
    if (!rc && d.adj_bin[kAdjBins - 1].count > 0) {
        d.adj_scratch_slots = std::min<int32_t>(d.adj_bin[kAdjBins - 1].count, 256);
        d.adj_scratch_stride = mx[kAdjBins - 1] / 8;
        rc = dev_alloc(d, &d.adj_scratch, (size_t)d.adj_scratch_slots * (size_t)d.adj_scratch_stride);
    }
    if (rc) { release_adjoint_state(d); return rc; }
    d.adj_ready = true;
    return NIN_OK;
}

int nin_gls_weights_backward_device(nin_grid *g, int add_neumann, const double *dev_grad_csr, const double *dev_grad_neumann_ws,
                                    double *dev_grad_perm, double *dev_grad_diff_mag, void *stream_) {
    if (!g || !dev_grad_csr || !dev_grad_perm) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device: the kernels are HIP only");
    if (!d.fields_set) return fail(NIN_ESTATE, "nin_fields_set has not been called");
    if (!d.have_perm) return fail(NIN_ESTATE, "GLS needs permeability and diff_mag");
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = ensure_adjoint_state(d, stream);
    if (!rc) rc = ensure_transpose_index(d, stream);
    if (rc) return rc;
    const char *only_env = getenv("NIN_GLS_ADJ_ONLY");   // per-bin timing (tools/time_adjoint.py): launch only that bin; read at every call
    const int only = only_env ? atoi(only_env) : -1;
    for (int b = 0; b < kAdjBins && !rc; ++b) {
        const DeviceGrid::AdjBin &bin = d.adj_bin[b];
        if (only >= 0 && b != only) continue;
        rc = launch_gls_adjoint(d.v, b, bin.nodes, bin.count, bin.bytes, add_neumann ? 1 : 0, dev_grad_csr, dev_grad_neumann_ws, d.adj_contrib,
                                d.adj_scratch, d.adj_scratch_stride, d.adj_scratch_slots, stream);
    }
    if (!rc) rc = launch_adjoint_gather(d.v, d.tr_cell_ptr, d.tr_cell_pos, d.adj_contrib, dev_grad_perm, dev_grad_diff_mag, stream);
    if (rc) return fail(rc, "launch failed: %s", hipGetErrorString(hipGetLastError()));
    return NIN_OK;
}

int nin_sddmm_device(nin_grid *g, const double *dev_u_cells, const double *dev_node_values, int32_t n_fields, double *dev_grad_csr,
                     void *stream_) {
    if (!g || !dev_u_cells || !dev_node_values || !dev_grad_csr) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device: the kernels are HIP only");
    HIP_TRY(hipSetDevice(d.device));
    const int rc = launch_sddmm(d.v, dev_u_cells, dev_node_values, n_fields, dev_grad_csr, static_cast<hipStream_t>(stream_));
    if (rc) return fail(rc, "launch failed: %s", hipGetErrorString(hipGetLastError()));
    return NIN_OK;
}

int nin_gls_permeability_gradient_host(nin_grid *g, const double *node_values, const double *cell_values, int32_t n_fields,
                                       double *grad_permeability) {
    if (!g || !node_values || !cell_values || !grad_permeability) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device: the kernels are HIP only");
    if (!d.fields_set) return fail(NIN_ESTATE, "nin_fields_set has not been called");
    if (!d.have_perm) return fail(NIN_ESTATE, "GLS needs permeability and diff_mag");
    HIP_TRY(hipSetDevice(d.device));
    const size_t pb = (size_t)g->h.n_points * 8, eb = (size_t)g->h.n_elems * 8;
    double *dv = nullptr, *du = nullptr, *dg = nullptr, *dk = nullptr;
    auto cleanup = [&]() { (void)hipFree(dv); (void)hipFree(du); (void)hipFree(dg); (void)hipFree(dk); };
#define TRY_A(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { cleanup(); return fail(NIN_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); } } while (0)
    TRY_A(hipMalloc((void **)&dv, pb * n_fields));
    TRY_A(hipMalloc((void **)&du, eb * n_fields));
    TRY_A(hipMalloc((void **)&dg, (size_t)std::max<int64_t>(d.nnz_e, 1) * 8));
    TRY_A(hipMalloc((void **)&dk, std::max<size_t>(eb, 8) * 9));
    TRY_A(hipMemcpy(dv, node_values, pb * n_fields, hipMemcpyHostToDevice));
    TRY_A(hipMemcpy(du, cell_values, eb * n_fields, hipMemcpyHostToDevice));
    // W as apply() uses it (`+ neumann_ws[row]` included): add_neumann = 1, nothing flows through neumann_ws itself
    int rc = nin_sddmm_device(g, du, dv, n_fields, dg, nullptr);
    if (!rc) rc = nin_gls_weights_backward_device(g, 1, dg, nullptr, dk, nullptr, nullptr);
    if (rc) { cleanup(); return rc; }
    TRY_A(hipMemcpy(grad_permeability, dk, eb * 9, hipMemcpyDeviceToHost));
#undef TRY_A
    cleanup();
    return NIN_OK;
}

int nin_gls_adjoint_plan(nin_grid *g, int64_t counts[4]) {
    if (!g || !counts) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (d.device < 0 || d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first)");
    HIP_TRY(hipSetDevice(d.device));
    const int rc = ensure_adjoint_state(d, nullptr);
    if (rc) return rc;
    for (int b = 0; b < kAdjBins; ++b) counts[b] = d.adj_bin[b].count;
    return NIN_OK;
}

int nin_gls_plan(const nin_grid *g, int64_t counts[22]) {
    if (!g || !counts) return fail(NIN_EINVAL, "NULL argument");
    if (g->d.device < 0 || g->d.prebuilt) return fail(NIN_ENODEVICE, "grid is not on a device (call nin_grid_to_device first)");
    for (int k = 0; k < kGlsPlanKernels; ++k) counts[k] = g->d.plan[k].count;
    return NIN_OK;
}

}  // extern "C"
