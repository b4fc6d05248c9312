// csr_dirty.hip -- the device half of an incremental interpolate(): the rows a dirty launch has just rewritten, counted
// and packed for the trip over PCIe.
//
// kernels_csr.hip finishes ALL rows: a wavefront owns 64 consecutive nodes, whose rows are one contiguous run of `data`, and walks
// the run in whole lines.  The rows of a dirty launch's list are not neighbours -- the list is in launch-plan order, unique, unsorted
// -- so here the run is the single row, and what is left of that reasoning is: never a lane per row (a lane walking its own row
// strides by the row length, 64 bytes on hexahedra, 200 on tetrahedra, and the axis node of a fan has more than 64 entries), and whole
// lines in.  Sixteen lanes own a row: 16 x 8 bytes is one 128-byte line of `data` per step, a hexahedron row (8 entries) takes one
// step with half the lanes idle, a tetrahedron row (~24) two, a 100-entry row seven.  The four rows of a wavefront step together: one
// ballot marks the entries that stay (`!= 0.0`, what eliminate_zeros keeps: NaNs stay, +-0 go), and each group takes its 16 bits of
// it -- popcount for the count, popcount below the lane for an entry's place.
#include <hip/hip_runtime.h>

#include "device_grid.hpp"
#include "launch.hpp"

namespace nin {

namespace {

constexpr int kRowLanes = 16;                  // lanes per listed row
constexpr int kRowsPerWave = 64 / kRowLanes;

// pack_cnt[i] = surviving entries of the row of node list[i]; cnt[p] (the matrix's resident row counts) follows, and *changed counts
// the rows whose count moved.  The list is unique: no two groups touch the same cnt[p].
__global__ __launch_bounds__(256) void nin_dirty_row_nnz_kernel(const int32_t *__restrict__ esup_ptr, const double *__restrict__ data,
                                                                const int32_t *__restrict__ list, int32_t total,
                                                                int32_t *__restrict__ pack_cnt, int32_t *__restrict__ cnt,
                                                                int32_t *__restrict__ changed) {
    const int lane = threadIdx.x & 63, sub = lane & (kRowLanes - 1), shift = lane & ~(kRowLanes - 1);
    const int32_t waves = (int32_t)(gridDim.x * (blockDim.x >> 6));
    for (int32_t i0 = (int32_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * kRowsPerWave; i0 < total; i0 += waves * kRowsPerWave) {
        const int32_t i = i0 + (lane >> 4);
        const bool live = i < total;
        const int32_t p = live ? list[i] : 0;
        const int32_t b = live ? esup_ptr[p] : 0, e = live ? esup_ptr[p + 1] : 0;
        int32_t c = 0;
        for (int32_t k = 0; __any(b + k < e); k += kRowLanes) {   // (uniform: the four rows of the wavefront step together)
            const int32_t j = b + k + sub;
            const unsigned long long m = __ballot(j < e && data[j] != 0.0);
            c += __popcll((m >> shift) & ((1ull << kRowLanes) - 1ull));
        }
        const bool moved = live && sub == 0 && cnt[p] != c;
        if (live && sub == 0) pack_cnt[i] = c;
        if (moved) cnt[p] = c;
        const unsigned long long mm = __ballot(moved);
        if (lane == 0 && mm) atomicAdd(changed, __popcll(mm));
    }
}

// after the exclusive scan of pack_cnt: the surviving (column, value) pairs of row i, in row order, from pack_off[i] on; its node
// and its neumann_ws
__global__ __launch_bounds__(256) void nin_dirty_pack_kernel(const int32_t *__restrict__ esup_ptr, const int32_t *__restrict__ esup,
                                                             const double *__restrict__ data, const double *__restrict__ nws,
                                                             const int32_t *__restrict__ list, int32_t total,
                                                             const int32_t *__restrict__ pack_off, int32_t *__restrict__ pack_node,
                                                             double *__restrict__ pack_nws, int32_t *__restrict__ pack_indices,
                                                             double *__restrict__ pack_data) {
    const int lane = threadIdx.x & 63, sub = lane & (kRowLanes - 1), shift = lane & ~(kRowLanes - 1);
    const int32_t waves = (int32_t)(gridDim.x * (blockDim.x >> 6));
    for (int32_t i0 = (int32_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * kRowsPerWave; i0 < total; i0 += waves * kRowsPerWave) {
        const int32_t i = i0 + (lane >> 4);
        const bool live = i < total;
        const int32_t p = live ? list[i] : 0;
        const int32_t b = live ? esup_ptr[p] : 0, e = live ? esup_ptr[p + 1] : 0;
        int32_t at = live ? pack_off[i] : 0;
        for (int32_t k = 0; __any(b + k < e); k += kRowLanes) {
            const int32_t j = b + k + sub;
            const bool in = j < e;
            const double d = in ? data[j] : 0.0;
            const int32_t col = in ? esup[j] : 0;
            const bool keep = in && d != 0.0;
            const unsigned long long m = (__ballot(keep) >> shift) & ((1ull << kRowLanes) - 1ull);
            if (keep) {
                const int32_t pos = at + __popcll(m & ((1ull << sub) - 1ull));
                pack_indices[pos] = col;
                pack_data[pos] = d;
            }
            at += __popcll(m);
        }
        if (live && sub == 0) {
            pack_node[i] = p;
            pack_nws[i] = nws[p];
        }
    }
}

int grid_for_rows(int32_t total) {   // four wavefronts a block, four rows a wavefront; at most 2048 blocks (then the loop strides)
    const int64_t b = ((int64_t)total + 4 * kRowsPerWave - 1) / (4 * kRowsPerWave);
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

}  // namespace

int launch_dirty_row_nnz(const GridView &g, const double *data, const int32_t *list, int32_t total, int32_t *pack_cnt, int32_t *cnt,
                         int32_t *changed, hipStream_t stream) {
    if (total <= 0) return 0;
    hipLaunchKernelGGL(nin_dirty_row_nnz_kernel, dim3(grid_for_rows(total)), dim3(256), 0, stream, g.esup_ptr, data, list, total, pack_cnt, cnt,
                       changed);
    return launch_status();
}

int launch_dirty_pack(const GridView &g, const double *data, const double *nws, const int32_t *list, int32_t total, const int32_t *pack_off,
                      int32_t *pack_node, double *pack_nws, int32_t *pack_indices, double *pack_data, hipStream_t stream) {
    if (total <= 0) return 0;
    hipLaunchKernelGGL(nin_dirty_pack_kernel, dim3(grid_for_rows(total)), dim3(256), 0, stream, g.esup_ptr, g.esup, data, nws, list, total,
                       pack_off, pack_node, pack_nws, pack_indices, pack_data);
    return launch_status();
}

}  // namespace nin
