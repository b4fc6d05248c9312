// kernels_gls_jacobian.hip -- the GLS Jacobian in the permeability, kept and applied, gfx950.
//
// For a fixed cell field u (and optional Neumann values b) the node values F_p(K) = sum_i d_i(K) u[c_i] + nws_p(K) b_p are a function of
// the permeability.  The adjoint kernel (kernels_gls_adjoint.hip) is linear in its cotangent node by node, so ONE launch of it with
// grad_csr[pos] = u[esup[pos]] and grad_neumann_ws = b leaves in its contribution buffer the sparse Jacobian itself:
//   C[pos][k] = dF_p / d perm_e[k] (k < 9),  C[pos][9] = dF_p / d diff_mag_e      for the pair (p, e) at esup position pos.
// The kernels here apply that buffer, 80 bytes per entry of esup read once per chunk of kJacChunk directions, accumulators in registers:
//   nin_jac_apply_kernel            out[t][p] = sum over row p of C . (dperm_t, ddm_t)          node-major, J . dK
//   nin_jac_apply_transpose_kernel  grad[t][e] = sum over the nodes of e of v_t[p] C[pos]         cell-major, J^T . v
// ddm / grad_diff_mag NULL: the chain through the table's diff_mag = (1 - 3 / tr K)^2 is folded with fold[e] = 2 (1 - 3 / tr K_e) 3 /
// tr K_e^2, a snapshot nin_jac_fold_kernel takes of the resident perm at linearisation (the expression of tangent_dm / the gather).
// Every product is an explicit fma and every order is fixed: no atomics, two calls agree bit for bit, a batch equals its members one
// by one (the instantiations differ in the number of accumulators only), 2 dK and 2 v give exactly twice.
//
// nin_jac_apply_kernel: 16 lanes per node, four consecutive nodes per wavefront.  A row is 10 ne contiguous doubles at a 16-byte
// boundary; lane l reads the pairs l, l + 16, ... of it (16 bytes a lane, 256 contiguous bytes a group, the rows of the four groups
// adjacent), each pair (k, k + 1) of one cell, and gathers that cell's dperm through esup (reused ~8 x on hexahedra: L2 / Infinity
// Cache), kJacAhead loads of the row issued before the first is used.  Lane sums in that order, then the 16 lanes by a fixed butterfly: the order depends on the row alone, not on the grid size or
// on n.  Every out[t][p] is written; a zero row of the forward has C = 0 and gives an exact 0.
//
// nin_jac_apply_transpose_kernel: thread e walks cell e's nodes in ascending node id through the transpose index, as
// nin_adjoint_gather_kernel does, with v_t[node] as a factor: acc[k] = fma(v, C[pos][k], acc[k]) from 0.0, so v = 1 adds exactly what the
// gather adds, and the fold follows the sum in the gather's expression.  A cell has 4 to 8 nodes on every mesh: the lists are short and
// even, nothing to split (the skewed-destination pitfall of store-then-sum does not arise on this side; the long rows are the nodes',
// and those are nin_jac_apply_kernel's, which spreads a row over 16 lanes).
#include <hip/hip_runtime.h>

#include "device_grid.hpp"
#include "diff_mag.hpp"
#include "launch.hpp"
#include "wave_ops.hpp"

namespace nin {

namespace {

using namespace waveops;

constexpr int kJacChunk = 4;   // directions per pass over the contribution buffer
constexpr int kJacAhead = 3;   // 16-byte loads of a row a lane issues before it uses the first (a cube node's row is 2.5 per lane)

// grad_csr[pos] = u[esup[pos]]: the cotangent whose adjoint launch leaves the Jacobian of W u in the contribution buffer
__global__ __launch_bounds__(256) void nin_jac_seed_kernel(const int32_t *__restrict__ esup, size_t nnz, const double *__restrict__ u,
                                                          double *__restrict__ grad_csr) {
    const size_t pos = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pos < nnz) grad_csr[pos] = u[esup[pos]];
}

// fold[e] = d diff_mag_e / d K_dd of the resident perm (diff_mag.hpp: diff_mag = (1 - 3 / tr K)^2)
__global__ __launch_bounds__(256) void nin_jac_fold_kernel(int32_t n_elems, const double *__restrict__ perm, double *__restrict__ fold) {
    const int32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    fold[e] = diff_mag_fold(perm + 9 * (size_t)e);
}

template <int NT>
__global__ __launch_bounds__(256) void nin_jac_apply_kernel(int32_t n_points, size_t n_elems, const int32_t *__restrict__ esup_ptr,
                                                           const int32_t *__restrict__ esup, const double *__restrict__ contrib,
                                                           const double *__restrict__ fold, const double *__restrict__ dperm,
                                                           const double *__restrict__ ddm, double *__restrict__ out) {
    const int lane = threadIdx.x & 15;
    const size_t p = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = p < (size_t)n_points;
    int32_t eb = 0, ne = 0;
    if (live) {
        eb = esup_ptr[p];
        ne = esup_ptr[p + 1] - eb;
    }
    double acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = 0.0;
    const double2 *row = reinterpret_cast<const double2 *>(contrib + 10 * (size_t)eb);
    const int n5 = 5 * ne;
    for (int q0 = lane; q0 < n5; q0 += 16 * kJacAhead) {   // kJacAhead pairs of the row in flight per lane
        double2 c[kJacAhead];
#pragma unroll
        for (int s = 0; s < kJacAhead; ++s) c[s] = q0 + 16 * s < n5 ? row[q0 + 16 * s] : double2{0.0, 0.0};
#pragma unroll
        for (int s = 0; s < kJacAhead; ++s) {
            const int q = q0 + 16 * s;
            if (q >= n5) break;
            const int j = q / 5, k = 2 * (q - 5 * j);   // the pair (k, k + 1) of the row's cell j
            const size_t e = (size_t)esup[eb + j];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double *d = dperm + ((size_t)t * n_elems + e) * 9;
                const double m0 = d[k];
                double m1;
                if (k < 8) m1 = d[k + 1];
                else if (ddm) m1 = ddm[(size_t)t * n_elems + e];
                else m1 = fold[e] * ((d[0] + d[4]) + d[8]);
                acc[t] = fma(c[s].x, m0, acc[t]);
                acc[t] = fma(c[s].y, m1, acc[t]);
            }
        }
    }
    double mine = 0.0;   // lane t of the group writes direction t
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const double s = group_sum<16>(acc[t]);
        if (lane == t) mine = s;
    }
    if (live && lane < NT) out[(size_t)lane * (size_t)n_points + p] = mine;
}

template <int NT>
__global__ __launch_bounds__(256) void nin_jac_apply_transpose_kernel(int32_t n_elems, size_t n_points, const int32_t *__restrict__ cell_ptr,
                                                                     const int32_t *__restrict__ cell_pos, const int32_t *__restrict__ cell_node,
                                                                     const double *__restrict__ contrib, const double *__restrict__ fold,
                                                                     const double *__restrict__ v, double *__restrict__ grad_perm,
                                                                     double *__restrict__ grad_dm) {
    const int32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    double acc[NT][10];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int k = 0; k < 10; ++k) acc[t][k] = 0.0;
    for (int32_t j = cell_ptr[e]; j < cell_ptr[e + 1]; ++j) {
        const double2 *c = reinterpret_cast<const double2 *>(contrib + 10 * (size_t)cell_pos[j]);
        const size_t node = (size_t)cell_node[j];
        double vt[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) vt[t] = v[(size_t)t * n_points + node];
#pragma unroll
        for (int h = 0; h < 5; ++h) {
            const double2 x = c[h];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc[t][2 * h] = fma(vt[t], x.x, acc[t][2 * h]);
                acc[t][2 * h + 1] = fma(vt[t], x.y, acc[t][2 * h + 1]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const size_t te = (size_t)t * (size_t)n_elems + (size_t)e;
        if (grad_dm) {
            grad_dm[te] = acc[t][9];
        } else {   // the gather's fold: the three diagonal entries take acc[9] . d diff_mag / d K_dd, each one fma as the gather compiles
            const double f = fold[e];
            acc[t][0] = fma(acc[t][9], f, acc[t][0]);
            acc[t][4] = fma(acc[t][9], f, acc[t][4]);
            acc[t][8] = fma(acc[t][9], f, acc[t][8]);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) grad_perm[9 * te + k] = acc[t][k];
    }
}

template <int NT>
int apply_chunk(const GridView &g, const double *contrib, const double *fold, const double *dperm, const double *ddm, double *out,
                hipStream_t stream) {
    hipLaunchKernelGGL(nin_jac_apply_kernel<NT>, blocks_for(g.n_points, 16), dim3(256), 0, stream, g.n_points, (size_t)g.n_elems, g.esup_ptr,
                       g.esup, contrib, fold, dperm, ddm, out);
    return launch_status();
}

template <int NT>
int transpose_chunk(const GridView &g, const int32_t *cell_ptr, const int32_t *cell_pos, const int32_t *cell_node, const double *contrib,
                    const double *fold, const double *v, double *grad_perm, double *grad_dm, hipStream_t stream) {
    hipLaunchKernelGGL(nin_jac_apply_transpose_kernel<NT>, blocks_for(g.n_elems), dim3(256), 0, stream, g.n_elems, (size_t)g.n_points,
                       cell_ptr, cell_pos, cell_node, contrib, fold, v, grad_perm, grad_dm);
    return launch_status();
}

}  // namespace

int launch_jac_seed(const GridView &g, int64_t nnz, const double *u, double *grad_csr, hipStream_t stream) {
    if (nnz <= 0) return 0;
    hipLaunchKernelGGL(nin_jac_seed_kernel, blocks_for(nnz), dim3(256), 0, stream, g.esup, (size_t)nnz, u, grad_csr);
    return launch_status();
}

int launch_jac_fold(const GridView &g, double *fold, hipStream_t stream) {
    if (g.n_elems <= 0) return 0;
    hipLaunchKernelGGL(nin_jac_fold_kernel, blocks_for(g.n_elems), dim3(256), 0, stream, g.n_elems, g.perm, fold);
    return launch_status();
}

int launch_jac_apply(const GridView &g, const double *contrib, const double *fold, int32_t n, const double *dperm, const double *ddm,
                     double *out, hipStream_t stream) {
    if (g.n_points <= 0) return 0;
    const size_t P = (size_t)g.n_points, E = (size_t)g.n_elems;
    return for_each_chunk<kJacChunk>(n, [&](auto nt, int32_t t0) {
        return apply_chunk<decltype(nt)::value>(g, contrib, fold, dperm + (size_t)t0 * E * 9, ddm ? ddm + (size_t)t0 * E : nullptr,
                                                out + (size_t)t0 * P, stream);
    });
}

int launch_jac_apply_transpose(const GridView &g, const int32_t *cell_ptr, const int32_t *cell_pos, const int32_t *cell_node,
                               const double *contrib, const double *fold, int32_t n, const double *v, double *grad_perm, double *grad_dm,
                               hipStream_t stream) {
    if (g.n_elems <= 0) return 0;
    const size_t P = (size_t)g.n_points, E = (size_t)g.n_elems;
    return for_each_chunk<kJacChunk>(n, [&](auto nt, int32_t t0) {
        return transpose_chunk<decltype(nt)::value>(g, cell_ptr, cell_pos, cell_node, contrib, fold, v + (size_t)t0 * P,
                                                    grad_perm + (size_t)t0 * E * 9, grad_dm ? grad_dm + (size_t)t0 * E : nullptr, stream);
    });
}

}  // namespace nin
