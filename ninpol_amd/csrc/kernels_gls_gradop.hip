// kernels_gls_gradop.hip -- the corner-gradient operator of the GLS reconstruction, kept and applied, gfx950.  The
// factorisation is not here: the adjoint kernel's gradient mode writes the operator (kernels_gls_adjoint.hip, GOP).  Here are its layout --
// gop_ptr, the exclusive sum of 3 ne^2, and the node of every esup position -- and the two streaming products.  Node p with ne cells owns
// G_p [3 ne x ne], column-major: gop[gop_ptr[p] + j * 3 ne + i], column j for the node's cell j, i = 3 * (cell slot) + component.
// Both products are HBM-bound passes over gop, up to kGradopChunk fields a pass.  Built with -ffp-contract=off: a caller that restates
// the sums below on the host, in the stated order, gets the same bits.  No atomics: a thread owns an output entry, or a column.
#include <hip/hip_runtime.h>

#include "device_grid.hpp"
#include "launch.hpp"

namespace nin {

namespace {

// thread p < P: count[p] = 3 ne^2, pos_node[row of p] = p; thread P: count[P] = 0 (the scan's last input)
__global__ __launch_bounds__(256) void nin_gradop_layout_kernel(GridView g, int64_t *__restrict__ count, int32_t *__restrict__ pos_node) {
    const int32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p > g.n_points) return;
    if (p == g.n_points) { count[p] = 0; return; }
    const int32_t eb = g.esup_ptr[p], ne = g.esup_ptr[p + 1] - eb;
    count[p] = 3 * (int64_t)ne * (int64_t)ne;
    for (int32_t i = 0; i < ne; ++i) pos_node[eb + i] = p;
}

// thread r = 3 pos + c, one entry of grad: grad[f][r] = sum_j gop[base_p + j * 3 ne + i] * u[f][cells_p[j]] with i = r - 3 esup_ptr[p],
// j ascending from 0.0, each product rounded, then added.  Neighbouring threads take neighbouring i: a step of j reads one contiguous run
// of a column, and the blocks of consecutive nodes follow each other in gop
template <int NF>
__global__ __launch_bounds__(256) void nin_gradop_apply_kernel(GridView g, long long nnz, const long long *__restrict__ gop_ptr,
                                                              const int32_t *__restrict__ pos_node, const double *__restrict__ gop,
                                                              const double *__restrict__ u, double *__restrict__ grad) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= 3 * nnz) return;
    const int32_t p = pos_node[r / 3];
    const int32_t eb = g.esup_ptr[p], ne = g.esup_ptr[p + 1] - eb;
    const double *col = gop + ((size_t)gop_ptr[p] + (size_t)(r - 3 * (long long)eb));
    const size_t ld = 3 * (size_t)ne;
    double acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = 0.0;
    for (int32_t j = 0; j < ne; ++j) {
        const double a = col[(size_t)j * ld];
        const size_t e = (size_t)g.esup[eb + j];
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] += a * u[(size_t)f * (size_t)g.n_elems + e];
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) grad[(size_t)f * 3 * (size_t)nnz + (size_t)r] = acc[f];
}

// thread pos, one column (p, j = pos - esup_ptr[p]): dots[f][pos] = sum_i gop[base_p + j * 3 ne + i] * gbar[f][3 esup_ptr[p] + i], i
// ascending from 0.0.  The 256 columns of a workgroup are one contiguous stretch of gop (the columns of a node follow each other, and so
// do the blocks of consecutive nodes), but a thread walking its own column puts the lanes of a wavefront 3 ne doubles apart: 64 cache
// lines a load.  So the workgroup stages the stretch through LDS, kDotTile doubles at a time with coalesced loads, and a thread adds
// the part of its column that lies in the tile -- tiles ascending, so the order of the sum is i ascending whatever the tiling.  (An LDS
// read with that stride conflicts, up to every lane of a group on one bank for ne a multiple of 32; the LDS then still delivers more
// than HBM does.)
constexpr int kDotTile = 6144;   // 48 KiB: the stretch of 256 columns of a hexahedron mesh's interior nodes (ne = 8), three workgroups a CU
template <int NF>
__global__ __launch_bounds__(256) void nin_gradop_dot_kernel(GridView g, long long nnz, const long long *__restrict__ gop_ptr,
                                                            const int32_t *__restrict__ pos_node, const double *__restrict__ gop,
                                                            const double *__restrict__ gbar, double *__restrict__ dots) {
    __shared__ double tile[kDotTile];
    __shared__ long long span[2];
    const int tid = threadIdx.x;
    const long long pos = (long long)blockIdx.x * 256 + tid;
    const bool on = pos < nnz;
    long long cs = 0;   // where the thread's column begins in gop
    int32_t ld = 0;
    const double *gb = gbar;
    if (on) {
        const int32_t p = pos_node[pos];
        const int32_t eb = g.esup_ptr[p];
        ld = 3 * (g.esup_ptr[p + 1] - eb);
        cs = gop_ptr[p] + (pos - eb) * (long long)ld;
        gb = gbar + 3 * (size_t)eb;
    }
    if (tid == 0) span[0] = cs;                                       // (thread 0 of a launched workgroup is always a column)
    if (on && (tid == 255 || pos == nnz - 1)) span[1] = cs + ld;      // the end of the workgroup's last column
    __syncthreads();
    const long long s0 = span[0], s1 = span[1];
    double acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = 0.0;
    for (long long ts = s0; ts < s1; ts += kDotTile) {
        const int len = (int)(s1 - ts < (long long)kDotTile ? s1 - ts : (long long)kDotTile);
        for (int k = tid; k < len; k += 256) tile[k] = gop[(size_t)ts + (size_t)k];
        __syncthreads();
        if (on) {
            const long long lo = cs > ts ? cs : ts, hi = cs + ld < ts + len ? cs + ld : ts + len;
            for (long long x = lo; x < hi; ++x) {
                const double a = tile[x - ts];
#pragma unroll
                for (int f = 0; f < NF; ++f) acc[f] += a * gb[(size_t)f * 3 * (size_t)nnz + (size_t)(x - cs)];
            }
        }
        __syncthreads();   // (the tile is the next stretch's)
    }
    if (on) {
#pragma unroll
        for (int f = 0; f < NF; ++f) dots[(size_t)f * (size_t)nnz + (size_t)pos] = acc[f];
    }
}

// thread e: ubar[f][e] = the sum of dots[f][cell_pos[k]] over the cell's entries of the transpose index, k ascending (ascending node id)
// from 0.0 -- the order of nin_adjoint_gather_kernel
template <int NF>
__global__ __launch_bounds__(256) void nin_gradop_gather_kernel(int32_t n_elems, long long nnz, const int32_t *__restrict__ cell_ptr,
                                                               const int32_t *__restrict__ cell_pos, const double *__restrict__ dots,
                                                               double *__restrict__ ubar) {
    const int32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    double acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = 0.0;
    for (int32_t k = cell_ptr[e]; k < cell_ptr[e + 1]; ++k) {
        const size_t pos = (size_t)cell_pos[k];
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] += dots[(size_t)f * (size_t)nnz + pos];
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) ubar[(size_t)f * (size_t)n_elems + (size_t)e] = acc[f];
}

template <int NF>
int apply_chunk(const GridView &g, int64_t nnz, const long long *gop_ptr, const int32_t *pos_node, const double *gop, const double *u,
                double *grad, hipStream_t stream) {
    hipLaunchKernelGGL(nin_gradop_apply_kernel<NF>, blocks_for(3 * nnz), dim3(256), 0, stream, g, (long long)nnz, gop_ptr, pos_node, gop, u, grad);
    return launch_status();
}

template <int NF>
int transpose_chunk(const GridView &g, int64_t nnz, const int32_t *cell_ptr, const int32_t *cell_pos, const long long *gop_ptr,
                    const int32_t *pos_node, const double *gop, const double *gbar, double *dots, double *ubar, hipStream_t stream) {
    if (nnz > 0) {
        hipLaunchKernelGGL(nin_gradop_dot_kernel<NF>, blocks_for(nnz), dim3(256), 0, stream, g, (long long)nnz, gop_ptr, pos_node, gop, gbar, dots);
        if (int rc = launch_status()) return rc;
    }
    hipLaunchKernelGGL(nin_gradop_gather_kernel<NF>, blocks_for(g.n_elems), dim3(256), 0, stream, g.n_elems, (long long)nnz, cell_ptr, cell_pos,
                       dots, ubar);
    return launch_status();
}

}  // namespace

int launch_gradop_layout(const GridView &g, int64_t nnz, int64_t *count, void *tmp, size_t *tmp_bytes, int64_t *gop_ptr, int32_t *pos_node,
                         hipStream_t stream) {
    if (!tmp) return xjac_pattern_scan(nullptr, tmp_bytes, count, gop_ptr, g.n_points, stream);   // (the size of the scan's scratch alone)
    (void)nnz;
    hipLaunchKernelGGL(nin_gradop_layout_kernel, blocks_for((int64_t)g.n_points + 1), dim3(256), 0, stream, g, count, pos_node);
    if (int rc = launch_status()) return rc;
    return xjac_pattern_scan(tmp, tmp_bytes, count, gop_ptr, g.n_points, stream);
}

int launch_gradop_apply(const GridView &g, int64_t nnz, const int64_t *gop_ptr_, const int32_t *pos_node, const double *gop, int32_t n,
                        const double *u, double *grad, hipStream_t stream) {
    static_assert(sizeof(long long) == sizeof(int64_t), "gop_ptr is read as long long");
    if (nnz <= 0) return 0;
    const long long *gop_ptr = reinterpret_cast<const long long *>(gop_ptr_);
    return for_each_chunk<kGradopChunk>(n, [&](auto nf, int32_t t) {
        return apply_chunk<decltype(nf)::value>(g, nnz, gop_ptr, pos_node, gop, u + (size_t)t * (size_t)g.n_elems, grad + (size_t)t * 3 * (size_t)nnz,
                                                stream);
    });
}

int launch_gradop_apply_transpose(const GridView &g, int64_t nnz, const int32_t *cell_ptr, const int32_t *cell_pos, const int64_t *gop_ptr_,
                                  const int32_t *pos_node, const double *gop, int32_t n, const double *gbar, double *dots, double *ubar,
                                  hipStream_t stream) {
    if (g.n_elems <= 0) return 0;
    const long long *gop_ptr = reinterpret_cast<const long long *>(gop_ptr_);
    return for_each_chunk<kGradopChunk>(n, [&](auto nf, int32_t t) {
        return transpose_chunk<decltype(nf)::value>(g, nnz, cell_ptr, cell_pos, gop_ptr, pos_node, gop, gbar + (size_t)t * 3 * (size_t)nnz, dots,
                                                    ubar + (size_t)t * (size_t)g.n_elems, stream);
    });
}

}  // namespace nin
