// kernels_gls_gradient.hip -- what follows the corner gradients of the GLS reconstruction, gfx950: two streaming
// kernels over grad [n_fields][nnz_esup][3] as the adjoint kernel's gradient mode (kernels_gls_adjoint.hip, GRD) left it.  The
// factorisation is not here.  Built with -ffp-contract=off: a caller that computes -K_e g or the mean of a row on the host in the
// expression order stated below gets the same bits.  No atomics: a thread owns an entry of esup, or a node.
#include <hip/hip_runtime.h>

#include "device_grid.hpp"
#include "launch.hpp"

namespace nin {

namespace {

// thread pos: flux[f][pos][c] = -((K[3c] g[0] + K[3c + 1] g[1]) + K[3c + 2] g[2]) with K = perm of cell esup[pos], row-major, and
// g = grad[f][pos]: products rounded one by one, summed left to right, then negated
__global__ __launch_bounds__(256) void nin_corner_flux_kernel(GridView g, long long nnz, int32_t n_fields, const double *__restrict__ grad,
                                                             double *__restrict__ flux) {
    const long long pos = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pos >= nnz) return;
    const double *K = g.perm + 9 * (size_t)g.esup[pos];
    double k[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) k[c] = K[c];
    for (int32_t f = 0; f < n_fields; ++f) {
        const size_t at = 3 * ((size_t)f * (size_t)nnz + (size_t)pos);
        const double g0 = grad[at + 0], g1 = grad[at + 1], g2 = grad[at + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) flux[at + c] = -((k[3 * c + 0] * g0 + k[3 * c + 1] * g1) + k[3 * c + 2] * g2);
    }
}

// thread p: node_gradient[f][p][c] = (sum of grad[f][pos][c] over the row of p, from 0.0 in row order) / ne; a node without cells gets
// zeros, and so does a node with the zero row (its corner gradients are zeros)
__global__ __launch_bounds__(256) void nin_node_gradient_kernel(GridView g, long long nnz, int32_t n_fields, const double *__restrict__ grad,
                                                               double *__restrict__ node_gradient) {
    const int32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.n_points) return;
    const int32_t eb = g.esup_ptr[p], ee = g.esup_ptr[p + 1];
    for (int32_t f = 0; f < n_fields; ++f) {
        double a[3] = {0.0, 0.0, 0.0};
        for (int32_t pos = eb; pos < ee; ++pos) {
            const double *gp = grad + 3 * ((size_t)f * (size_t)nnz + (size_t)pos);
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] += gp[c];
        }
        double *o = node_gradient + 3 * ((size_t)f * (size_t)g.n_points + (size_t)p);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = ee > eb ? a[c] / (double)(ee - eb) : 0.0;
    }
}

}  // namespace

int launch_corner_flux(const GridView &g, int64_t nnz, int32_t n_fields, const double *grad, double *flux, hipStream_t stream) {
    if (nnz <= 0) return 0;
    hipLaunchKernelGGL(nin_corner_flux_kernel, blocks_for(nnz), dim3(256), 0, stream, g, (long long)nnz, n_fields, grad, flux);
    return launch_status();
}

int launch_node_gradient(const GridView &g, int64_t nnz, int32_t n_fields, const double *grad, double *node_gradient, hipStream_t stream) {
    if (g.n_points <= 0) return 0;
    hipLaunchKernelGGL(nin_node_gradient_kernel, blocks_for(g.n_points), dim3(256), 0, stream, g, (long long)nnz, n_fields, grad,
                       node_gradient);
    return launch_status();
}

}  // namespace nin
