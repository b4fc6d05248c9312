// kernels_gls_jacobian_reduced.hip -- the GLS Jacobian in a reduced parametrisation of the permeability, applied, gfx950.
//
// The permeability moves along M parameters per cell, perm_e = sum_m theta_(e,m) B_(e,m).  The adjoint kernel's RED mode
// (kernels_gls_adjoint.hip) leaves R [nnz_esup][M], row-major in esup position: R[pos][m] = dF_p / d theta_(e,m) for the pair (p, e) at
// pos, the diff_mag chain folded.  The kernels here apply it, 8 M bytes per entry of esup read once per chunk of kJacrChunk directions,
// accumulators in registers:
//   nin_jacr_apply_kernel<M, NT>            out[t][p]  = sum over row p, sum_m R[pos][m] dtheta_t[e][m]       node-major, J_theta . dtheta
//   nin_jacr_apply_transpose_kernel<M, NT>  grad[t][e][m] = sum over the nodes of e of v_t[p] R[pos][m]       cell-major, J_theta^T . v
// Every product is an explicit fma and every order is fixed: no atomics, no memset, two calls agree bit for bit, a batch equals its
// members one by one (the NT instantiations differ in the number of accumulators only), 2 dtheta and 2 v give exactly twice.
//
// nin_jacr_apply_kernel: kLanes<M> lanes per node -- 8 for M = 1, 16 for M = 3 and 6 -- and 64 / kLanes consecutive nodes per wavefront,
// whose rows are adjacent in R.  A row is M ne contiguous doubles at R + M eb, at a 16-byte boundary only when M eb is even: M = 6 loads
// 16 bytes a lane (the pair (m, m + 1) of one cell), M = 1 and 3 load 8.  Lane l takes the loads l, l + kLanes, ... of the row, kJacrAhead
// of them issued before the first is used, and gathers dtheta through esup; then the lanes of the node by a fixed butterfly.  The
// order depends on the row and on M alone: not on the grid size, on n, or on which nodes share the wavefront.  Every out[t][p] is
// written; a zero row of the forward has R = 0 and gives an exact 0.
//
// nin_jacr_apply_transpose_kernel: thread e walks cell e's nodes in ascending node id through the transpose index, as
// nin_jac_apply_transpose_kernel does: acc[t][m] = fma(v_t[node], R[pos][m], acc[t][m]) from 0.0.  A cell has 4 to 8 nodes; the loads
// of kGroup of them are issued together, as nin_apply_transpose_kernel issues eight.
#include <hip/hip_runtime.h>

#include "device_grid.hpp"
#include "launch.hpp"
#include "wave_ops.hpp"

namespace nin {

namespace {

using namespace waveops;

constexpr int kJacrChunk = 4;   // directions per pass over R
constexpr int kJacrAhead = 3;   // loads of a row a lane issues before it uses the first

template <int M> constexpr int kLanes = M == 1 ? 8 : 16;   // lanes per node
template <int M> constexpr int kWide = M % 2 == 0 ? 2 : 1;  // doubles per load: 2 where every row begins at a 16-byte boundary
template <int M> constexpr int kGroup = M == 1 ? 8 : 4;     // entries of a cell the transpose has in flight (a hexahedron has 8 nodes)

template <int M, int NT>
__global__ __launch_bounds__(256) void nin_jacr_apply_kernel(int32_t n_points, size_t n_elems, const int32_t *__restrict__ esup_ptr,
                                                            const int32_t *__restrict__ esup, const double *__restrict__ R,
                                                            const double *__restrict__ dtheta, double *__restrict__ out) {
    constexpr int L = kLanes<M>, W = kWide<M>, Q = M / W;   // Q loads per cell
    const int lane = threadIdx.x & (L - 1);
    const size_t p = (size_t)blockIdx.x * (256 / L) + (threadIdx.x / L);
    const bool live = p < (size_t)n_points;
    int32_t eb = 0, ne = 0;
    if (live) {
        eb = esup_ptr[p];
        ne = esup_ptr[p + 1] - eb;
    }
    double acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = 0.0;
    const double *row = R + (size_t)M * (size_t)eb;
    const int nq = Q * ne;
    for (int q0 = lane; q0 < nq; q0 += L * kJacrAhead) {
        double c[kJacrAhead][W];
#pragma unroll
        for (int s = 0; s < kJacrAhead; ++s) {
            const int q = q0 + L * s;
            if constexpr (W == 2) {
                const double2 x = q < nq ? reinterpret_cast<const double2 *>(row)[q] : double2{0.0, 0.0};
                c[s][0] = x.x;
                c[s][1] = x.y;
            } else {
                c[s][0] = q < nq ? row[q] : 0.0;
            }
        }
#pragma unroll
        for (int s = 0; s < kJacrAhead; ++s) {
            const int q = q0 + L * s;
            if (q >= nq) break;
            const int j = q / Q, m = W * (q - Q * j);   // entries m .. m + W - 1 of the row's cell j
            const size_t e = (size_t)esup[eb + j];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double *d = dtheta + ((size_t)t * n_elems + e) * M + m;
#pragma unroll
                for (int w = 0; w < W; ++w) acc[t] = fma(c[s][w], d[w], acc[t]);
            }
        }
    }
    double mine = 0.0;   // lane t of the node's group writes direction t
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const double s = group_sum<L>(acc[t]);
        if (lane == t) mine = s;
    }
    if (live && lane < NT) out[(size_t)lane * (size_t)n_points + p] = mine;
}

template <int M, int NT>
__global__ __launch_bounds__(256) void nin_jacr_apply_transpose_kernel(int32_t n_elems, size_t n_points, const int32_t *__restrict__ cell_ptr,
                                                                      const int32_t *__restrict__ cell_pos,
                                                                      const int32_t *__restrict__ cell_node, const double *__restrict__ R,
                                                                      const double *__restrict__ v, double *__restrict__ grad) {
    constexpr int W = kWide<M>;
    const int32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    double acc[NT][M];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[t][m] = 0.0;
    // kGroup entries at a time: their index loads, then their gathers of R and v, are issued together (a lane's walk is a chain of
    // dependent loads otherwise); the sums stay in node order.  An entry past the cell's end reads the last one again and adds nothing
    constexpr int G = kGroup<M>;
    const int32_t end = cell_ptr[e + 1];
    for (int32_t j0 = cell_ptr[e]; j0 < end; j0 += G) {
        size_t pos[G], node[G];
#pragma unroll
        for (int s = 0; s < G; ++s) {
            const int32_t j = j0 + s < end ? j0 + s : end - 1;
            pos[s] = (size_t)cell_pos[j];
            node[s] = (size_t)cell_node[j];
        }
        double x[G][M], vt[G][NT];
#pragma unroll
        for (int s = 0; s < G; ++s) {
            const double *r = R + (size_t)M * pos[s];
            if constexpr (W == 2) {
#pragma unroll
                for (int h = 0; h < M / 2; ++h) {
                    const double2 y = reinterpret_cast<const double2 *>(r)[h];
                    x[s][2 * h] = y.x;
                    x[s][2 * h + 1] = y.y;
                }
            } else {
#pragma unroll
                for (int m = 0; m < M; ++m) x[s][m] = r[m];
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) vt[s][t] = v[(size_t)t * n_points + node[s]];
        }
#pragma unroll
        for (int s = 0; s < G; ++s) {
            const bool in = j0 + s < end;   // (a select, not a branch: a branch here makes the compiler sink the loads under it)
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const double a = fma(vt[s][t], x[s][m], acc[t][m]);
                    acc[t][m] = in ? a : acc[t][m];
                }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        double *o = grad + ((size_t)t * (size_t)n_elems + (size_t)e) * M;
#pragma unroll
        for (int m = 0; m < M; ++m) o[m] = acc[t][m];
    }
}

template <int M, int NT>
int apply_chunk(const GridView &g, const double *R, const double *dtheta, double *out, hipStream_t stream) {
    hipLaunchKernelGGL((nin_jacr_apply_kernel<M, NT>), blocks_for(g.n_points, 256 / kLanes<M>), dim3(256), 0, stream, g.n_points,
                       (size_t)g.n_elems, g.esup_ptr, g.esup, R, dtheta, out);
    return launch_status();
}

template <int M, int NT>
int transpose_chunk(const GridView &g, const int32_t *cell_ptr, const int32_t *cell_pos, const int32_t *cell_node, const double *R,
                    const double *v, double *grad, hipStream_t stream) {
    hipLaunchKernelGGL((nin_jacr_apply_transpose_kernel<M, NT>), blocks_for(g.n_elems), dim3(256), 0, stream, g.n_elems, (size_t)g.n_points,
                       cell_ptr, cell_pos, cell_node, R, v, grad);
    return launch_status();
}

template <int M>
int apply_all(const GridView &g, const double *R, int32_t n, const double *dtheta, double *out, hipStream_t stream) {
    const size_t P = (size_t)g.n_points, E = (size_t)g.n_elems;
    return for_each_chunk<kJacrChunk>(n, [&](auto nt, int32_t t0) {
        return apply_chunk<M, decltype(nt)::value>(g, R, dtheta + (size_t)t0 * E * M, out + (size_t)t0 * P, stream);
    });
}

template <int M>
int transpose_all(const GridView &g, const int32_t *cell_ptr, const int32_t *cell_pos, const int32_t *cell_node, const double *R, int32_t n,
                  const double *v, double *grad, hipStream_t stream) {
    const size_t P = (size_t)g.n_points, E = (size_t)g.n_elems;
    return for_each_chunk<kJacrChunk>(n, [&](auto nt, int32_t t0) {
        return transpose_chunk<M, decltype(nt)::value>(g, cell_ptr, cell_pos, cell_node, R, v + (size_t)t0 * P, grad + (size_t)t0 * E * M, stream);
    });
}

}  // namespace

int launch_jacr_apply(const GridView &g, int32_t M, const double *R, int32_t n, const double *dtheta, double *out, hipStream_t stream) {
    if (g.n_points <= 0) return 0;
    switch (M) {
        case 1: return apply_all<1>(g, R, n, dtheta, out, stream);
        case 3: return apply_all<3>(g, R, n, dtheta, out, stream);
        case 6: return apply_all<6>(g, R, n, dtheta, out, stream);
    }
    return fail(NIN_EINVAL, "the reduced Jacobian is built for 1, 3 or 6 parameters per cell, not %d", (int)M);
}

int launch_jacr_apply_transpose(const GridView &g, int32_t M, const int32_t *cell_ptr, const int32_t *cell_pos, const int32_t *cell_node,
                                const double *R, int32_t n, const double *v, double *grad_theta, hipStream_t stream) {
    if (g.n_elems <= 0) return 0;
    switch (M) {
        case 1: return transpose_all<1>(g, cell_ptr, cell_pos, cell_node, R, n, v, grad_theta, stream);
        case 3: return transpose_all<3>(g, cell_ptr, cell_pos, cell_node, R, n, v, grad_theta, stream);
        case 6: return transpose_all<6>(g, cell_ptr, cell_pos, cell_node, R, n, v, grad_theta, stream);
    }
    return fail(NIN_EINVAL, "the reduced Jacobian is built for 1, 3 or 6 parameters per cell, not %d", (int)M);
}

}  // namespace nin
