// geom_math.hpp -- the geometry of one cell and of one face from the node coordinates, for the device units that write the resident
// geometry (grid_update.hip: every cell and face of the mesh; grid_scatter.hip: the cells and faces around a list of moved nodes;
// internal).  Both are built with -ffp-contract=off (build.py) and compile these expressions, so they write the same bits: what
// grid_device.hip's k_centroids / k_faces_geometry, grid_host.cpp and the reference's calculate_centroids() +
// calculate_normal_faces() (grid.pyx:669-809) make of the same coordinates.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nin {

// The centroid of the cell whose [8] index row is (a, b), n of them real: divide-then-add in vertex order (grid.pyx:699-704).  The -1
// padding of a row costs no divergent region: a padded slot loads the row's first point again (a valid address, the line is already
// there) and contributes a selected +0.0.  The running sums start at +0.0 and therefore never hold -0.0, so adding +0.0 leaves every
// bit alone.  X: [P][3]; d: the mesh's dimension (components k >= d stay 0).
__device__ __forceinline__ void cell_centroid_of(const int4 a, const int4 b, int n, int d, int32_t P, const double *__restrict__ X, double c[3]) {
    const int32_t q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const double dn = (double)n;
    c[0] = 0.0; c[1] = 0.0; c[2] = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool on = j < n;
        const int64_t p = min(max(on ? q[j] : q[0], 0), P - 1);   // (the builders checked every index; the clamp keeps a damaged row inside the array)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double x = X[p * 3 + k];
            c[k] += (on && k < d) ? x / dn : 0.0;
        }
    }
}

// The centre (sum, then divide: grid.pyx:716-727), the float32 unit normal and the area of the face whose [4] index row is r.  The
// face's points end at the first -1 (at least two are there); a slot past the end reads the first point again.
template <bool DIM3>
__device__ __forceinline__ void face_geometry_of(const int4 r, int d, int32_t P, const double *__restrict__ X, double c[3], float &nx, float &ny,
                                                 float &nz, double &area) {
    const int32_t p1 = min(max(r.x, 0), P - 1);
    const bool on1 = r.y != -1, on2 = on1 && r.z != -1, on3 = on2 && r.w != -1;
    const int32_t q[4] = {p1, on1 ? min(r.y, P - 1) : p1, on2 ? min(r.z, P - 1) : p1, on3 ? min(r.w, P - 1) : p1};
    const bool on[4] = {true, on1, on2, on3};
    const int npofa = 1 + (int)on1 + (int)on2 + (int)on3;
    double x[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) x[j][k] = X[(int64_t)q[j] * 3 + k];
    c[0] = 0.0; c[1] = 0.0; c[2] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += (on[j] && k < d) ? x[j][k] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < d) c[k] /= (double)npofa;
    if (DIM3) {
        // float locals exactly as grid.pyx:732-736 (k_faces_geometry); points 1, 2, 3 of the row, and 4 where there is one
        float v1x = (float)(x[0][0] - x[1][0]), v1y = (float)(x[0][1] - x[1][1]), v1z = (float)(x[0][2] - x[1][2]);
        float v2x = (float)(x[2][0] - x[1][0]), v2y = (float)(x[2][1] - x[1][1]), v2z = (float)(x[2][2] - x[1][2]);
        nx = v1y * v2z - v1z * v2y; ny = v1z * v2x - v1x * v2z; nz = v1x * v2y - v1y * v2x;
        const float norm = fabsf(sqrtf(nx * nx + ny * ny + nz * nz));
        nx = nx / norm; ny = ny / norm; nz = nz / norm;
        v1x = (float)(x[0][0] - x[3][0]); v1y = (float)(x[0][1] - x[3][1]); v1z = (float)(x[0][2] - x[3][2]);
        v2x = (float)(x[2][0] - x[3][0]); v2y = (float)(x[2][1] - x[3][1]); v2z = (float)(x[2][2] - x[3][2]);
        const float mx = v1y * v2z - v1z * v2y, my = v1z * v2x - v1x * v2z, mz = v1x * v2y - v1y * v2x;
        const double quad = (double)(norm + sqrtf(mx * mx + my * my + mz * mz)) / 2.0, tri = (double)norm / 2.0;
        area = on3 ? quad : tri;
    } else {
        const float v1x = (float)(x[0][0] - x[1][0]), v1y = (float)(x[0][1] - x[1][1]);
        nx = -v1y; ny = v1x;
        const float norm = fabsf(sqrtf(nx * nx + ny * ny));
        nx = nx / norm; ny = ny / norm; nz = 0.0f;
        area = (double)norm;
    }
}

// the points per cell of element type t: byte t of npoel8
__device__ __forceinline__ int npoel_of(uint64_t npoel8, int8_t t) { return (int)((npoel8 >> (8 * (t & 7))) & 0xff); }

}  // namespace nin
