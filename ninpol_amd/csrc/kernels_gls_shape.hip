// kernels_gls_shape.hip -- the GLS weights differentiated with respect to the node coordinates, part 2: from the geometric inputs of
// the nodes' systems to the vertices, gfx950.
//
// The adjoint kernel in its coordinate mode (kernels_gls_adjoint.hip, PTS) leaves, per computed node p,
//   xbar_own [p][3]               what the node's own position gets through the rows of its system (in grad_points itself),
//   cbar [esup position][3]       dL/d centroid_e through node p's system,
//   (fcbar, Nbar) [fsup position][6]   dL/d face centre and dL/d unit normal of face f through node p's system.
// The geometry of geom_math.hpp (3-D) is differentiated here, in three kernels that follow each other on one stream:
//   nin_shape_face_kernel, thread f: Fcbar_f and Nbar_f summed over the face's points in inpofa order (the position of f in a point's
//     fsup row by binary search: the rows are ascending).  fc_f = sum x_v / npofa gives every point Fcbar_f / npofa, the fourth point
//     of a quadrilateral too; n = v1 x v2 with v1 = x_0 - x_1, v2 = x_2 - x_1, N = n / |n| gives
//       nbar = (Nbar_f - (Nbar_f . N) N) / |n|,  v1bar = v2 x nbar,  v2bar = nbar x v1,  x_0 += v1bar, x_2 += v2bar, x_1 -= v1bar + v2bar
//     (v1, v2 and |n| in float64 from the resident coordinates, N the resident float32 normal: the derivative is that of the real-valued
//     model, the float32 casts of face_geometry_of count as the identity).  One 3-vector per point slot of the face, face_slot [F][4][3].
//   nin_shape_cell_kernel, thread e: Cbar_e over the cell's nodes in ascending node id through the transpose index; centroid_e =
//     sum x_v / n_e, so Cbar_e / n_e replaces the records of the cell in cbar, in place (they are the cell's alone).
//   nin_shape_node_kernel, thread p: grad_points[p] = xbar_own[p] + sum over esup[p] of cbar + sum over fsup[p] of the slot of p in f,
//     each sum in row order.
// No atomics: two calls agree bit for bit.
//
// The tangent reads the same geometry forwards, before the adjoint kernel's tangent mode runs: a direction dX [P][3] to
//   nin_shape_tangent_cell_kernel, thread (direction, e): dC_e = sum dx_v / n_e over the cell's inpoel row,
//   nin_shape_tangent_face_kernel, thread (direction, f): dFc_f = sum dx_v / npofa (the fourth point of a quadrilateral too) and
//     dN_f = (dn - (dn.N) N) / |n| with dn = dv1 x v2 + v1 x dv2, dv1 = dx_0 - dx_1, dv2 = dx_2 - dx_1 -- v1, v2, |n| and N as above.
#include <hip/hip_runtime.h>

#include "device_grid.hpp"
#include "gls_shape_chain.hpp"
#include "launch.hpp"

namespace nin {

namespace {

__global__ __launch_bounds__(256) void nin_shape_face_kernel(GridView g, const int4 *__restrict__ inpofa, const double *__restrict__ face_bar,
                                                             double *__restrict__ face_slot) {
    const int32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= g.n_faces) return;
    const int4 r = inpofa[f];
    const int32_t q[4] = {r.x, r.y, r.z, r.w};
    int npofa = 0;
    while (npofa < 4 && q[npofa] >= 0 && q[npofa] < g.n_points) ++npofa;   // (a row ends at the first -1; the builders checked every index)
    double *slot = face_slot + 12 * (size_t)f;
    if (npofa < 3) {   // (no face of a 3-D mesh)
        for (int i = 0; i < 12; ++i) slot[i] = 0.0;
        return;
    }
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < npofa; ++k) {
        int32_t lo = g.fsup_ptr[q[k]], hi = g.fsup_ptr[q[k] + 1];
        while (lo < hi) {   // the first position with fsup >= f
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (g.fsup[mid] < f) lo = mid + 1; else hi = mid;
        }
        if (lo >= g.fsup_ptr[q[k] + 1] || g.fsup[lo] != f) continue;
        const double *rec = face_bar + 6 * (size_t)lo;
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] += rec[c];
    }
    double x[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) x[j][c] = g.coords[3 * (size_t)q[j] + c];
    const double v1[3] = {x[0][0] - x[1][0], x[0][1] - x[1][1], x[0][2] - x[1][2]};
    const double v2[3] = {x[2][0] - x[1][0], x[2][1] - x[1][1], x[2][2] - x[1][2]};
    const double n[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    // (no guard on |n| = 0: a face whose first three points are collinear has no normal, the forward's rows of it are NaN already, and
    // so is the gradient of its three points -- also where Nbar_f itself is zero)
    const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double N[3] = {(double)g.face_normal[3 * (size_t)f + 0], (double)g.face_normal[3 * (size_t)f + 1], (double)g.face_normal[3 * (size_t)f + 2]};
    shape_face_chain(acc, v1, v2, nn, N, npofa, slot);
}

__global__ __launch_bounds__(256) void nin_shape_cell_kernel(int32_t n_elems, const int32_t *__restrict__ cell_ptr, const int32_t *__restrict__ cell_pos,
                                                             double *__restrict__ cell_bar) {
    const int32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    const int32_t jb = cell_ptr[e], je = cell_ptr[e + 1];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int32_t j = jb; j < je; ++j) {
        const double *c = cell_bar + 3 * (size_t)cell_pos[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += c[k];
    }
    const double dn = (double)(je - jb);   // the points of the cell
    for (int32_t j = jb; j < je; ++j) {
        double *c = cell_bar + 3 * (size_t)cell_pos[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = acc[k] / dn;
    }
}

__global__ __launch_bounds__(256) void nin_shape_node_kernel(GridView g, const int4 *__restrict__ inpofa, const double *__restrict__ cell_bar,
                                                             const double *__restrict__ face_slot, double *__restrict__ grad_points) {
    const int32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.n_points) return;
    double acc[3] = {grad_points[3 * (size_t)p + 0], grad_points[3 * (size_t)p + 1], grad_points[3 * (size_t)p + 2]};   // xbar_own
    for (int32_t j = g.esup_ptr[p]; j < g.esup_ptr[p + 1]; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += cell_bar[3 * (size_t)j + c];
    for (int32_t j = g.fsup_ptr[p]; j < g.fsup_ptr[p + 1]; ++j) {
        const int32_t f = g.fsup[j];
        const int4 r = inpofa[f];
        const int k = r.x == p ? 0 : (r.y == p ? 1 : (r.z == p ? 2 : (r.w == p ? 3 : -1)));
        if (k < 0) continue;
        const double *s = face_slot + 12 * (size_t)f + 3 * k;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += s[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_points[3 * (size_t)p + c] = acc[c];
}

// ---- the same geometry read forwards: a direction dX [P][3] of the coordinates to dC, dFc and dN.  One thread per
//      (direction, cell) or (direction, face), the direction in blockIdx.y; every entry is written, sums in row order, no atomics ----
__global__ __launch_bounds__(256) void nin_shape_tangent_cell_kernel(int32_t n_elems, int32_t n_points, int32_t n_tan, const int4 *__restrict__ inpoel,
                                                                     const double *__restrict__ dX, double *__restrict__ dC) {
    const int32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    const int4 a = inpoel[2 * (size_t)e], b = inpoel[2 * (size_t)e + 1];
    const int32_t q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    int n = 0;
    while (n < 8 && q[n] >= 0 && q[n] < n_points) ++n;   // (a row ends at the first -1; the builders checked every index)
    const double dn = (double)n;
    for (int32_t t = blockIdx.y; t < n_tan; t += gridDim.y) {
        const double *dx = dX + (size_t)t * 3 * (size_t)n_points;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int j = 0; j < n; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += dx[3 * (size_t)q[j] + c];
        double *o = dC + ((size_t)t * (size_t)n_elems + (size_t)e) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = n > 0 ? acc[c] / dn : 0.0;
    }
}

__global__ __launch_bounds__(256) void nin_shape_tangent_face_kernel(GridView g, int32_t n_tan, const int4 *__restrict__ inpofa,
                                                                     const double *__restrict__ dX, double *__restrict__ dFN) {
    const int32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= g.n_faces) return;
    const int4 r = inpofa[f];
    const int32_t q[4] = {r.x, r.y, r.z, r.w};
    int npofa = 0;
    while (npofa < 4 && q[npofa] >= 0 && q[npofa] < g.n_points) ++npofa;
    if (npofa < 3) {   // (no face of a 3-D mesh)
        for (int32_t t = blockIdx.y; t < n_tan; t += gridDim.y) {
            double *o = dFN + ((size_t)t * (size_t)g.n_faces + (size_t)f) * 6;
            for (int i = 0; i < 6; ++i) o[i] = 0.0;
        }
        return;
    }
    double x[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) x[j][c] = g.coords[3 * (size_t)q[j] + c];
    const double v1[3] = {x[0][0] - x[1][0], x[0][1] - x[1][1], x[0][2] - x[1][2]};
    const double v2[3] = {x[2][0] - x[1][0], x[2][1] - x[1][1], x[2][2] - x[1][2]};
    const double n[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    // (no guard on |n| = 0, as in nin_shape_face_kernel: such a face has no normal and the forward's rows of it are NaN already)
    const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double N[3] = {(double)g.face_normal[3 * (size_t)f + 0], (double)g.face_normal[3 * (size_t)f + 1], (double)g.face_normal[3 * (size_t)f + 2]};
    const double dnp = (double)npofa;
    for (int32_t t = blockIdx.y; t < n_tan; t += gridDim.y) {
        const double *dx = dX + (size_t)t * 3 * (size_t)g.n_points;
        double d[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) d[j][c] = j < npofa ? dx[3 * (size_t)q[j] + c] : 0.0;
        const double dv1[3] = {d[0][0] - d[1][0], d[0][1] - d[1][1], d[0][2] - d[1][2]};
        const double dv2[3] = {d[2][0] - d[1][0], d[2][1] - d[1][1], d[2][2] - d[1][2]};
        const double dn[3] = {(dv1[1] * v2[2] - dv1[2] * v2[1]) + (v1[1] * dv2[2] - v1[2] * dv2[1]),
                              (dv1[2] * v2[0] - dv1[0] * v2[2]) + (v1[2] * dv2[0] - v1[0] * dv2[2]),
                              (dv1[0] * v2[1] - dv1[1] * v2[0]) + (v1[0] * dv2[1] - v1[1] * dv2[0])};
        const double dot = (dn[0] * N[0] + dn[1] * N[1]) + dn[2] * N[2];
        double *o = dFN + ((size_t)t * (size_t)g.n_faces + (size_t)f) * 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = (((d[0][c] + d[1][c]) + d[2][c]) + d[3][c]) / dnp;   // the fourth point of a quadrilateral too (a triangle: + 0.0)
            o[3 + c] = (dn[c] - dot * N[c]) / nn;
        }
    }
}

}  // namespace

int launch_shape_tangent_geometry(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, int32_t n_tangents, const double *tangent_points,
                                  double *tangent_cell, double *tangent_face, hipStream_t stream) {
    const unsigned ny = (unsigned)(n_tangents < 65535 ? n_tangents : 65535);
    if (g.n_elems > 0)
        hipLaunchKernelGGL(nin_shape_tangent_cell_kernel, dim3((unsigned)((g.n_elems + 255) / 256), ny), dim3(256), 0, stream, g.n_elems, g.n_points,
                           n_tangents, reinterpret_cast<const int4 *>(inpoel), tangent_points, tangent_cell);
    if (g.n_faces > 0)
        hipLaunchKernelGGL(nin_shape_tangent_face_kernel, dim3((unsigned)((g.n_faces + 255) / 256), ny), dim3(256), 0, stream, g, n_tangents,
                           reinterpret_cast<const int4 *>(inpofa), tangent_points, tangent_face);
    return launch_status();
}

int launch_shape_gather(const GridView &g, const int32_t *inpofa, const int32_t *cell_ptr, const int32_t *cell_pos, double *cell_bar,
                        const double *face_bar, double *face_slot, double *grad_points, hipStream_t stream) {
    const int4 *rows = reinterpret_cast<const int4 *>(inpofa);
    if (g.n_faces > 0)
        hipLaunchKernelGGL(nin_shape_face_kernel, blocks_for(g.n_faces), dim3(256), 0, stream, g, rows, face_bar, face_slot);
    if (g.n_elems > 0)
        hipLaunchKernelGGL(nin_shape_cell_kernel, blocks_for(g.n_elems), dim3(256), 0, stream, g.n_elems, cell_ptr, cell_pos,
                           cell_bar);
    if (g.n_points > 0)
        hipLaunchKernelGGL(nin_shape_node_kernel, blocks_for(g.n_points), dim3(256), 0, stream, g, rows, cell_bar, face_slot,
                           grad_points);
    return launch_status();
}

}  // namespace nin
