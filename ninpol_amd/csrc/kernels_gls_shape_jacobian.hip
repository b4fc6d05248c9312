// kernels_gls_shape_jacobian.hip -- the GLS Jacobian in the node coordinates, kept and applied, gfx950.
//
// For a fixed cell field u (and optional Neumann values b) the node values F_p(X) = sum_i d_i(X) u[c_i] + nws_p(X) b_p are a function of
// the node coordinates.  The adjoint kernel's coordinate mode (kernels_gls_adjoint.hip, PTS) is linear in its cotangent node by node, so
// ONE launch of it with grad_csr[pos] = u[esup[pos]] and grad_neumann_ws = b leaves, per computed node p, the derivative of F_p in the
// geometric inputs of its system:
//   cbar [esup position][3]          dF_p / d centroid_e,
//   (fcbar, Nbar) [fsup position][6]  dF_p / d face centre_f and dF_p / d unit normal_f,
//   xown [p][3]                       dF_p / d x_p through the rows of the system itself.
// What follows is mesh geometry only (kernels_gls_shape.hip), so the Jacobian is kept factored through it:
//   nin_xjac_apply_kernel   out[t][p] = sum_row cbar . dC_t[esup] + sum_row (fcbar . dFc_t[fsup] + Nbar . dN_t[fsup]) + xown[p] . dx_t[p]
//                           node-major, J . dX; dC, dFc and dN from launch_shape_tangent_geometry, unchanged
//   nin_xjac_face_kernel / nin_xjac_cell_kernel / nin_xjac_node_kernel   the three gathers of the shape adjoint with every record of node p
//                           multiplied by v_t[p] where it is first read, J^T . v
// The records are the large operand (24 nnz_esup + 48 nnz_fsup + 24 P bytes) and are read once per chunk of directions, accumulators in
// registers.  Every product is an explicit fma and every order is fixed and depends on the row alone: no atomics, no memset, two calls
// agree bit for bit, a batch equals its members one by one (the instantiations differ in the number of accumulators only), 2 dX and 2 v
// give exactly twice, and v = 1 reproduces launch_shape_gather bit for bit (fma(1, x, a) = a + x; the face chain is gls_shape_chain.hpp's
// one expression).
//
// nin_xjac_apply_kernel: 16 lanes per node, four consecutive nodes per wavefront, no row split.  A node's row is two contiguous runs, 3 ne
// doubles of cbar and 6 nf doubles of (fcbar, Nbar), plus three.  Lane l takes the records l, l + 16, ... of each run WHOLE -- a record is
// what one gather through esup / fsup serves, and a 16-byte pair mapping as nin_jac_apply_kernel's would split a cell's 3-vector over two
// lanes and gather twice.  The face run is 16-byte aligned (48-byte records): three 16-byte loads a record.  The cell run is 16-byte
// aligned only at even positions, so a cell record is three 8-byte loads, whatever the parity: the three instructions of 16 lanes cover
// 384 contiguous bytes, every byte of every line is used, and there is no odd head to peel.  kXjacAhead records of a run are loaded
// before the first is used, and the first block of the face run is loaded before the cell run is summed.  Lane sums in that order, the
// node's own term on lane 0 last, then the 16 lanes by wave_sum's first four DPP steps.  Every out[t][p] is written; a zero row of the
// forward has zero records and gives an exact 0.
//
// The transpose's kernels are one thread per face, cell and node as their models in kernels_gls_shape.hip: a face has 3 or 4 points and a
// cell 4 to 8 nodes, short even lists; the node kernel's rows are the long ones, but it reads 24 bytes per entry where the apply kernel
// reads 72, and it must add in launch_shape_gather's row order to reproduce it.
#include <hip/hip_runtime.h>

#include "device_grid.hpp"
#include "gls_shape_chain.hpp"
#include "launch.hpp"
#include "wave_ops.hpp"

namespace nin {

namespace {

using namespace waveops;

constexpr int kXjacAhead = 2;   // records of a run a lane loads before it uses the first (a cube node's runs are 8 and 12 records: one)

struct FaceRec {
    double2 a, b, c;   // (fcbar, Nbar)
};

__device__ __forceinline__ FaceRec load_face_rec(const double *__restrict__ face_bar, int32_t row, int j, int n) {
    FaceRec r{{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    if (j < n) {
        const double2 *q = reinterpret_cast<const double2 *>(face_bar + 6 * ((size_t)row + (size_t)j));
        r.a = q[0];
        r.b = q[1];
        r.c = q[2];
    }
    return r;
}

template <int NT>
__global__ __launch_bounds__(256) void nin_xjac_apply_kernel(GridView g, const double *__restrict__ cell_bar, const double *__restrict__ face_bar,
                                                            const double *__restrict__ own_bar, const double *__restrict__ dX,
                                                            const double *__restrict__ dC, const double *__restrict__ dFN,
                                                            double *__restrict__ out) {
    const int lane = threadIdx.x & 15;
    const size_t p = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const size_t P = (size_t)g.n_points, E = (size_t)g.n_elems, F = (size_t)g.n_faces;
    const bool live = p < P;
    int32_t eb = 0, ne = 0, fb = 0, nf = 0;
    if (live) {
        eb = g.esup_ptr[p];
        ne = g.esup_ptr[p + 1] - eb;
        fb = g.fsup_ptr[p];
        nf = g.fsup_ptr[p + 1] - fb;
    }
    double acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = 0.0;
    // the first block of the face run, in flight under the cell run
    FaceRec fr[kXjacAhead];
#pragma unroll
    for (int s = 0; s < kXjacAhead; ++s) fr[s] = load_face_rec(face_bar, fb, lane + 16 * s, nf);
    for (int j0 = lane; j0 < ne; j0 += 16 * kXjacAhead) {
        double c[kXjacAhead][3];
#pragma unroll
        for (int s = 0; s < kXjacAhead; ++s) {
            const bool in = j0 + 16 * s < ne;
            const double *q = cell_bar + 3 * ((size_t)eb + (size_t)(in ? j0 + 16 * s : 0));
#pragma unroll
            for (int k = 0; k < 3; ++k) c[s][k] = in ? q[k] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < kXjacAhead; ++s) {
            const int j = j0 + 16 * s;
            if (j >= ne) break;
            const size_t e = (size_t)g.esup[eb + j];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double *d = dC + ((size_t)t * E + e) * 3;
                acc[t] = fma(c[s][0], d[0], acc[t]);
                acc[t] = fma(c[s][1], d[1], acc[t]);
                acc[t] = fma(c[s][2], d[2], acc[t]);
            }
        }
    }
    for (int j0 = lane; j0 < nf; j0 += 16 * kXjacAhead) {
        if (j0 != lane) {
#pragma unroll
            for (int s = 0; s < kXjacAhead; ++s) fr[s] = load_face_rec(face_bar, fb, j0 + 16 * s, nf);
        }
#pragma unroll
        for (int s = 0; s < kXjacAhead; ++s) {
            const int j = j0 + 16 * s;
            if (j >= nf) break;
            const size_t f = (size_t)g.fsup[fb + j];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double2 *d = reinterpret_cast<const double2 *>(dFN + ((size_t)t * F + f) * 6);
                const double2 d0 = d[0], d1 = d[1], d2 = d[2];
                acc[t] = fma(fr[s].a.x, d0.x, acc[t]);
                acc[t] = fma(fr[s].a.y, d0.y, acc[t]);
                acc[t] = fma(fr[s].b.x, d1.x, acc[t]);
                acc[t] = fma(fr[s].b.y, d1.y, acc[t]);
                acc[t] = fma(fr[s].c.x, d2.x, acc[t]);
                acc[t] = fma(fr[s].c.y, d2.y, acc[t]);
            }
        }
    }
    if (live && lane == 0) {   // the node's own position
        const double *o = own_bar + 3 * p;
        const double o0 = o[0], o1 = o[1], o2 = o[2];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double *d = dX + ((size_t)t * P + p) * 3;
            acc[t] = fma(o0, d[0], acc[t]);
            acc[t] = fma(o1, d[1], acc[t]);
            acc[t] = fma(o2, d[2], acc[t]);
        }
    }
    double mine = 0.0;   // lane t of the group writes direction t
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const double s = group_sum<16>(acc[t]);
        if (lane == t) mine = s;
    }
    if (live && lane < NT) out[(size_t)lane * P + p] = mine;
}

// ---- J^T . v: launch_shape_gather's three kernels with v_t[p] as a factor on every record of node p ------------------------------------
template <int NT>
__global__ __launch_bounds__(256) void nin_xjac_face_kernel(GridView g, const int4 *__restrict__ inpofa, const double *__restrict__ face_bar,
                                                           const double *__restrict__ v, double *__restrict__ face_slot) {
    const int32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= g.n_faces) return;
    const size_t P = (size_t)g.n_points, F = (size_t)g.n_faces;
    const int4 r = inpofa[f];
    const int32_t q[4] = {r.x, r.y, r.z, r.w};
    int npofa = 0;
    while (npofa < 4 && q[npofa] >= 0 && q[npofa] < g.n_points) ++npofa;   // (a row ends at the first -1; the builders checked every index)
    if (npofa < 3) {   // (no face of a 3-D mesh)
#pragma unroll
        for (int t = 0; t < NT; ++t)
            for (int i = 0; i < 12; ++i) face_slot[12 * ((size_t)t * F + (size_t)f) + i] = 0.0;
        return;
    }
    double acc[NT][6];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[t][c] = 0.0;
    for (int k = 0; k < npofa; ++k) {
        int32_t lo = g.fsup_ptr[q[k]], hi = g.fsup_ptr[q[k] + 1];
        while (lo < hi) {   // the first position with fsup >= f
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (g.fsup[mid] < f) lo = mid + 1; else hi = mid;
        }
        if (lo >= g.fsup_ptr[q[k] + 1] || g.fsup[lo] != f) continue;
        const double *rec = face_bar + 6 * (size_t)lo;
        double x[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) x[c] = rec[c];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double vt = v[(size_t)t * P + (size_t)q[k]];
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[t][c] = fma(vt, x[c], acc[t][c]);
        }
    }
    double x[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) x[j][c] = g.coords[3 * (size_t)q[j] + c];
    const double v1[3] = {x[0][0] - x[1][0], x[0][1] - x[1][1], x[0][2] - x[1][2]};
    const double v2[3] = {x[2][0] - x[1][0], x[2][1] - x[1][1], x[2][2] - x[1][2]};
    const double n[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    // (no guard on |n| = 0, as in nin_shape_face_kernel)
    const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double N[3] = {(double)g.face_normal[3 * (size_t)f + 0], (double)g.face_normal[3 * (size_t)f + 1], (double)g.face_normal[3 * (size_t)f + 2]};
#pragma unroll
    for (int t = 0; t < NT; ++t) shape_face_chain(acc[t], v1, v2, nn, N, npofa, face_slot + 12 * ((size_t)t * F + (size_t)f));
}

// cell_share [NT][E][3] = (sum over the nodes of e, ascending node id, of v_t[p] cbar(p, e)) / n_e: a buffer of its own, the kept records stay
template <int NT>
__global__ __launch_bounds__(256) void nin_xjac_cell_kernel(int32_t n_elems, size_t n_points, const int32_t *__restrict__ cell_ptr,
                                                           const int32_t *__restrict__ cell_pos, const int32_t *__restrict__ cell_node,
                                                           const double *__restrict__ cell_bar, const double *__restrict__ v,
                                                           double *__restrict__ cell_share) {
    const int32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    const int32_t jb = cell_ptr[e], je = cell_ptr[e + 1];
    double acc[NT][3];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[t][k] = 0.0;
    for (int32_t j = jb; j < je; ++j) {
        const double *c = cell_bar + 3 * (size_t)cell_pos[j];
        const size_t node = (size_t)cell_node[j];
        const double c0 = c[0], c1 = c[1], c2 = c[2];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double vt = v[(size_t)t * n_points + node];
            acc[t][0] = fma(vt, c0, acc[t][0]);
            acc[t][1] = fma(vt, c1, acc[t][1]);
            acc[t][2] = fma(vt, c2, acc[t][2]);
        }
    }
    const double dn = (double)(je - jb);   // the points of the cell
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int k = 0; k < 3; ++k) cell_share[3 * ((size_t)t * (size_t)n_elems + (size_t)e) + k] = acc[t][k] / dn;
}

template <int NT>
__global__ __launch_bounds__(256) void nin_xjac_node_kernel(GridView g, const int4 *__restrict__ inpofa, const double *__restrict__ own_bar,
                                                           const double *__restrict__ cell_share, const double *__restrict__ face_slot,
                                                           const double *__restrict__ v, double *__restrict__ grad_points) {
    const int32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.n_points) return;
    const size_t P = (size_t)g.n_points, E = (size_t)g.n_elems, F = (size_t)g.n_faces;
    double acc[NT][3];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const double vt = v[(size_t)t * P + (size_t)p];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[t][c] = vt * own_bar[3 * (size_t)p + c];
    }
    for (int32_t j = g.esup_ptr[p]; j < g.esup_ptr[p + 1]; ++j) {
        const size_t e = (size_t)g.esup[j];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[t][c] += cell_share[3 * ((size_t)t * E + e) + c];
    }
    for (int32_t j = g.fsup_ptr[p]; j < g.fsup_ptr[p + 1]; ++j) {
        const int32_t f = g.fsup[j];
        const int4 r = inpofa[f];
        const int k = r.x == p ? 0 : (r.y == p ? 1 : (r.z == p ? 2 : (r.w == p ? 3 : -1)));
        if (k < 0) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double *s = face_slot + 12 * ((size_t)t * F + (size_t)f) + 3 * k;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[t][c] += s[c];
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int c = 0; c < 3; ++c) grad_points[3 * ((size_t)t * P + (size_t)p) + c] = acc[t][c];
}

template <int NT>
int apply_chunk(const GridView &g, const double *cell_bar, const double *face_bar, const double *own_bar, const double *dX, const double *dC,
                const double *dFN, double *out, hipStream_t stream) {
    hipLaunchKernelGGL(nin_xjac_apply_kernel<NT>, blocks_for(g.n_points, 16), dim3(256), 0, stream, g, cell_bar, face_bar, own_bar, dX, dC, dFN, out);
    return launch_status();
}

template <int NT>
int transpose_chunk(const GridView &g, const int32_t *inpofa, const int32_t *cell_ptr, const int32_t *cell_pos, const int32_t *cell_node,
                    const double *cell_bar, const double *face_bar, const double *own_bar, const double *v, double *cell_share,
                    double *face_slot, double *grad_points, hipStream_t stream) {
    const int4 *rows = reinterpret_cast<const int4 *>(inpofa);
    if (g.n_faces > 0) {
        hipLaunchKernelGGL(nin_xjac_face_kernel<NT>, blocks_for(g.n_faces), dim3(256), 0, stream, g, rows, face_bar, v, face_slot);
        if (int rc = launch_status()) return rc;
    }
    if (g.n_elems > 0) {
        hipLaunchKernelGGL(nin_xjac_cell_kernel<NT>, blocks_for(g.n_elems), dim3(256), 0, stream, g.n_elems, (size_t)g.n_points, cell_ptr, cell_pos,
                           cell_node, cell_bar, v, cell_share);
        if (int rc = launch_status()) return rc;
    }
    hipLaunchKernelGGL(nin_xjac_node_kernel<NT>, blocks_for(g.n_points), dim3(256), 0, stream, g, rows, own_bar, cell_share, face_slot, v, grad_points);
    return launch_status();
}

}  // namespace

int launch_xjac_apply(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, const double *cell_bar, const double *face_bar,
                      const double *own_bar, int32_t n, const double *dX, double *tangent_cell, double *tangent_face, double *out,
                      hipStream_t stream) {
    if (g.n_points <= 0) return 0;
    const size_t P = (size_t)g.n_points;
    return for_each_chunk<kXjacApplyChunk>(n, [&](auto nt, int32_t t0) {
        const double *dx = dX + (size_t)t0 * P * 3;
        if (int rc = launch_shape_tangent_geometry(g, inpoel, inpofa, nt, dx, tangent_cell, tangent_face, stream)) return rc;
        return apply_chunk<decltype(nt)::value>(g, cell_bar, face_bar, own_bar, dx, tangent_cell, tangent_face, out + (size_t)t0 * P, stream);
    });
}

int launch_xjac_apply_transpose(const GridView &g, const int32_t *inpofa, const int32_t *cell_ptr, const int32_t *cell_pos,
                                const int32_t *cell_node, const double *cell_bar, const double *face_bar, const double *own_bar, int32_t n,
                                const double *v, double *cell_share, double *face_slot, double *grad_points, hipStream_t stream) {
    if (g.n_points <= 0) return 0;
    const size_t P = (size_t)g.n_points;
    return for_each_chunk<kXjacTransposeChunk>(n, [&](auto nt, int32_t t0) {
        return transpose_chunk<decltype(nt)::value>(g, inpofa, cell_ptr, cell_pos, cell_node, cell_bar, face_bar, own_bar, v + (size_t)t0 * P,
                                                    cell_share, face_slot, grad_points + (size_t)t0 * P * 3, stream);
    });
}

}  // namespace nin
