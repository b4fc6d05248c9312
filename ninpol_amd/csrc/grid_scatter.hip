// grid_scatter.hip -- local mesh motion: a SUBSET of nodes moved from device memory, the geometry around them made again and the
// nodes whose weights that can move marked (nin_grid_scatter_points*).
//
// Which rows can move.  A row of node v reads coords[v], the centroids (and permeability) of the cells of esup(v) and the centres and
// normals of the faces of fsup(v).  Moving node p changes coords[p], the centroids of the cells of esup(p) and the centre, normal and
// area of the faces of fsup(p); every face of fsup(p) lies in a cell of esup(p).  So the rows that can move are those of the vertices
// of the cells around the moved nodes, and no others (pinned on the oracle's own arithmetic by tests/test_update_points_local_host.py).
//
// Two kernels on one stream, no atomics on values:
//   nin_scatter_points_kernel<Id>   a lane per entry i of the id list: coords[ids[i]] = xyz[i], zero-padded to three columns as
//       nin_update_pad_coords_kernel pads.  The id is checked against [0, P) BEFORE any access; a refused id writes nothing and adds
//       one to the counter the permeability scatter uses (nin_weights_dirty_device reports it).  Nothing else is written here: a cell
//       around a moved node usually holds OTHER moved nodes, so its centroid may be taken only once every new coordinate is in place --
//       the kernel boundary is that barrier.
//   nin_regeom_around_kernel<Id, DIM3>   SLOTS = 16 lanes per accepted entry p: lane s takes the cells esup(p)[s], [s + 16], ... -- the
//       centroid from inpoel / etype / coords with grid_update.hip's arithmetic (geom_math.hpp, the same -ffp-contract=off: the bits
//       are a whole-mesh update's), dirty[v] = 1 for the cell's vertices -- and then the faces fsup(p)[s], [s + 16], ...: centre,
//       float32 normal, area.  A cell shared by two moved nodes is computed twice from the same coordinates and both lanes store the
//       same bits; the marks are plain stores of 1.
//       Why 16 lanes an entry and not one: a node of a hexahedron mesh has 8 cells and 12 faces, a node of a Delaunay mesh 14 ... 65
//       cells and one and a half times as many faces.  With a lane per entry a wavefront runs as long as its longest row, every lane
//       walking its row through dependent gathers (row -> index row -> coordinates) one cell at a time; with 16 lanes an entry the trip
//       count is ceil(row / 16) -- 1 for hexahedra, 1 ... 5 for the cells and 2 ... 7 for the faces of Delaunay nodes -- the 16 lanes
//       read consecutive words of one esup / fsup row, and up to 16 independent gather chains are in flight per entry.  The two
//       loops (cells, then faces) keep the lanes of a wavefront in the same body: no lane computes a centroid while its neighbour
//       computes a normal.
//       The records leave as 8- and 4-byte stores 24 / 12 bytes apart: the list is a small part of the mesh and its cells are
//       scattered, so there is no contiguous run to widen (grid_update.hip's LDS transposition has one).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "geom_math.hpp"
#include "launch.hpp"

namespace nin {

namespace {

constexpr int TPB = 256;
constexpr int SLOTS = 16;               // lanes per list entry in the geometry kernel
constexpr int ENTRIES = TPB / SLOTS;    // list entries per workgroup
static_assert(TPB % SLOTS == 0 && 64 % SLOTS == 0, "an entry's lanes share a wavefront");

template <class Id>
__global__ __launch_bounds__(TPB) void nin_scatter_points_kernel(int64_t m, const Id *__restrict__ ids, const double *__restrict__ xyz, int cd,
                                                                  int32_t P, double *__restrict__ coords, int32_t *__restrict__ rejected) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const int64_t p = (int64_t)ids[i];
    if (p < 0 || p >= (int64_t)P) {   // before any access through the id
        atomicAdd(rejected, 1);
        return;
    }
    for (int k = 0; k < 3; ++k) coords[p * 3 + k] = k < cd ? xyz[i * cd + k] : 0.0;   // zero-padded, as nin_update_pad_coords_kernel
}

template <class Id, bool DIM3>
__global__ __launch_bounds__(TPB) void nin_regeom_around_kernel(int64_t m, const Id *__restrict__ ids, GridView g, uint64_t npoel8,
                                                                 const int4 *__restrict__ inpoel, const int8_t *__restrict__ etype,
                                                                 const int4 *__restrict__ inpofa, double *__restrict__ cen,
                                                                 double *__restrict__ cen4, double *__restrict__ fc, float *__restrict__ fn,
                                                                 double *__restrict__ fa, uint8_t *__restrict__ dirty) {
    const int64_t i = (int64_t)blockIdx.x * ENTRIES + threadIdx.x / SLOTS;
    const int s = threadIdx.x % SLOTS;
    if (i >= m) return;
    const int64_t p = (int64_t)ids[i];
    if (p < 0 || p >= (int64_t)g.n_points) return;   // refused (and counted) by the scatter
    const int32_t P = g.n_points, d = g.dim;
    const double *__restrict__ X = g.coords;
    const int32_t e_end = g.esup_ptr[p + 1];
    for (int32_t j = g.esup_ptr[p] + s; j < e_end; j += SLOTS) {
        const int64_t e = g.esup[j];
        if (e < 0 || e >= (int64_t)g.n_elems) continue;   // (the builders checked every index; a damaged row writes nothing outside the arrays)
        const int4 a = inpoel[2 * e], b = inpoel[2 * e + 1];
        const int n = npoel_of(npoel8, etype[e]);
        double c[3];
        cell_centroid_of(a, b, n, d, P, X, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) cen[e * 3 + k] = c[k];
        if (cen4) {   // the NIN_ROWS_PAD4 build: (x, y, z, 0), as launch_pad_centroids
#pragma unroll
            for (int k = 0; k < 3; ++k) cen4[e * 4 + k] = c[k];
            cen4[e * 4 + 3] = 0.0;
        }
        const int32_t q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
            if (jj < n && q[jj] >= 0 && q[jj] < P) dirty[q[jj]] = 1;
    }
    const int32_t f_end = g.fsup_ptr[p + 1];
    for (int32_t j = g.fsup_ptr[p] + s; j < f_end; j += SLOTS) {
        const int64_t f = g.fsup[j];
        if (f < 0 || f >= (int64_t)g.n_faces) continue;
        double c[3], area;
        float nx, ny, nz;
        face_geometry_of<DIM3>(inpofa[f], d, P, X, c, nx, ny, nz, area);
#pragma unroll
        for (int k = 0; k < 3; ++k) fc[f * 3 + k] = c[k];
        fn[f * 3 + 0] = nx; fn[f * 3 + 1] = ny; fn[f * 3 + 2] = nz;
        fa[f] = area;
    }
}

template <class Id>
int scatter_variant(const GridView &g, uint64_t npoel8, const int32_t *inpoel, const int8_t *etype, const int32_t *inpofa, const void *ids_,
                    int64_t n, const double *xyz, int cd, double *fa, uint8_t *dirty, int32_t *rejected, hipStream_t stream) {
    const Id *ids = static_cast<const Id *>(ids_);
    hipLaunchKernelGGL((nin_scatter_points_kernel<Id>), blocks_for(n, TPB), dim3(TPB), 0, stream, n, ids, xyz, cd, g.n_points,
                       const_cast<double *>(g.coords), rejected);
    if (int rc = launch_status()) return rc;
    const dim3 grid = blocks_for(n, ENTRIES);
    const int4 *poel = reinterpret_cast<const int4 *>(inpoel), *pofa = reinterpret_cast<const int4 *>(inpofa);
    double *cen = const_cast<double *>(g.centroids), *cen4 = const_cast<double *>(g.centroids4), *fc = const_cast<double *>(g.face_center);
    float *fn = const_cast<float *>(g.face_normal);
    if (g.dim == 3)
        hipLaunchKernelGGL((nin_regeom_around_kernel<Id, true>), grid, dim3(TPB), 0, stream, n, ids, g, npoel8, poel, etype, pofa, cen, cen4, fc, fn,
                           fa, dirty);
    else
        hipLaunchKernelGGL((nin_regeom_around_kernel<Id, false>), grid, dim3(TPB), 0, stream, n, ids, g, npoel8, poel, etype, pofa, cen, cen4, fc, fn,
                           fa, dirty);
    return launch_status();
}

}  // namespace

int launch_scatter_points(const GridView &g, uint64_t npoel8, const int32_t *inpoel, const int8_t *etype, const int32_t *inpofa,
                          const void *dev_ids, int ids_are_int64, int64_t n, const double *dev_xyz, int coords_dim, double *face_area,
                          uint8_t *dirty, int32_t *rejected, hipStream_t stream) {
    if (n <= 0) return 0;
    if (coords_dim < 1 || coords_dim > 3) return fail(NIN_ERANGE, "coords_dim is %d, not 1, 2 or 3", coords_dim);
    if (n > (int64_t)INT32_MAX * ENTRIES) return fail(NIN_ERANGE, "%lld ids are more than one launch takes", (long long)n);
    return ids_are_int64
               ? scatter_variant<int64_t>(g, npoel8, inpoel, etype, inpofa, dev_ids, n, dev_xyz, coords_dim, face_area, dirty, rejected, stream)
               : scatter_variant<int32_t>(g, npoel8, inpoel, etype, inpofa, dev_ids, n, dev_xyz, coords_dim, face_area, dirty, rejected, stream);
}

}  // namespace nin
