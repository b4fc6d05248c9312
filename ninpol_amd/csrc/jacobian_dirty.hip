// jacobian_dirty.hip -- what a dirty relinearisation of a kept GLS Jacobian runs before the adjoint kernel: the grid's
// marked nodes binned by ADJOINT bin, the cotangent seeded for their rows alone, and marks set without an update
// (nin_gls_jacobian_linearize_dirty and its two siblings, nin_grid_mark_dirty_device).  The adjoint kernel itself is
// kernels_gls_adjoint.hip's, launched unchanged on the lists made here.
//
// Five kernels, no work counters, no atomic whose order reaches an output:
//   nin_adj_bin_byte_kernel     bin_of[nodes[i]] = b for the nodes of one adjoint bin: the per-node bin byte [P], made from the bins'
//       own lists (abi_apply.hip: ensure_adjoint_bins), so the two cannot disagree -- NIN_GLS_ADJ_FORCE_GLOBAL included.
//   nin_adj_dirty_compact_kernel<false / true>   fields_scatter.hip's compaction with the adjoint's four bins as keys: count, (hipcub
//       exclusive scan), fill.  A workgroup of 256 threads takes 256 consecutive nodes; inside a wavefront the lanes of one key are
//       ranked by ballot + popcount, the wavefronts of a workgroup by counters in LDS, the workgroups by the scan of hist[key][block]
//       -- bin-major, so the scanned value is the position in one flat buffer in which bin b follows bin b - 1 and every list is in
//       ascending node id.  The fill pass writes where every list begins, the total and the refused-id counter as it read it to a
//       header of its own, and clears the marks it reads when asked to -- unless ids were refused: then the caller gets an error and
//       the set must survive.
//   nin_jac_seed_rows_kernel    grad_csr[pos] = u[esup[pos]] for the rows of the listed nodes, 16 lanes a node: nothing proportional to
//       nnz_esup.
//   nin_mark_dirty_kernel       dirty[v] = 1 for the given nodes, or for the vertices of the given cells (fields_scatter.hip's walk
//       of inpoel); an id is checked BEFORE any access, a refused one marks nothing and adds one to the grid's counter.  The marks
//       are plain stores of 1: idempotent.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>

#include "gls_adjoint.hpp"
#include "launch.hpp"

namespace nin {

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int NK = kAdjBins;
static_assert(NK + 2 <= kAdjDirtyHdrInts, "the header of the adjoint's dirty lists is too small for the bins");


__global__ __launch_bounds__(TPB) void nin_adj_bin_byte_kernel(const int32_t *__restrict__ nodes, int32_t count, int32_t P, uint8_t b,
                                                                uint8_t *__restrict__ bin_of) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= count) return;
    const int32_t p = nodes[i];
    if (p >= 0 && p < P) bin_of[p] = b;
}

// hist: [NK][nblocks] + one int.  FILL = false writes the counts (and 0 into the last int); FILL = true reads their exclusive scan.
template <bool FILL>
__global__ __launch_bounds__(TPB) void nin_adj_dirty_compact_kernel(int32_t P, int32_t nblocks, int clear, uint8_t *__restrict__ dirty,
                                                                     const uint8_t *__restrict__ bin_of, const int32_t *__restrict__ rejected,
                                                                     int32_t *__restrict__ hist, int32_t *__restrict__ lists,
                                                                     int32_t *__restrict__ hdr) {
    __shared__ int32_t wave_cnt[WAVES][NK];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < WAVES * NK) (&wave_cnt[0][0])[tid] = 0;
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * TPB + tid;
    bool has = p < P && dirty[p] != 0;
    const int key = has ? (int)bin_of[p] : -1;
    has = has && key < NK;   // (every node is in a bin: the byte was written from the bins' lists)
    int rank = 0;
    unsigned long long todo = __ballot(has);
    while (todo) {   // one round per key present in the wavefront (wave-uniform: `todo` is a ballot)
        const int leader = __ffsll(todo) - 1;
        const int kk = __shfl(key, leader);
        const unsigned long long mk = __ballot(has && key == kk);
        if (has && key == kk) rank = __popcll(mk & ((1ull << lane) - 1ull));
        if (lane == leader) wave_cnt[w][kk] = __popcll(mk);
        todo &= ~mk;
    }
    __syncthreads();
    if (!FILL) {
        if (tid < NK) {
            int32_t c = 0;
            for (int ww = 0; ww < WAVES; ++ww) c += wave_cnt[ww][tid];
            hist[(int64_t)tid * nblocks + blockIdx.x] = c;
        }
        if (blockIdx.x == 0 && tid == NK) hist[(int64_t)NK * nblocks] = 0;
    } else {
        if (has) {
            int32_t at = hist[(int64_t)key * nblocks + blockIdx.x];
            for (int ww = 0; ww < w; ++ww) at += wave_cnt[ww][key];
            lists[at + rank] = (int32_t)p;   // at + rank < the scan's total <= P
            if (clear && *rejected == 0) dirty[p] = 0;
        }
        if (blockIdx.x == 0 && tid <= NK) hdr[tid] = hist[(int64_t)tid * nblocks];   // where bin tid's list begins; [NK]: the total
        if (blockIdx.x == 0 && tid == NK + 1) hdr[NK + 1] = *rejected;
    }
}

__global__ __launch_bounds__(TPB) void nin_jac_seed_rows_kernel(const int32_t *__restrict__ esup_ptr, const int32_t *__restrict__ esup,
                                                                 const int32_t *__restrict__ list, int32_t total, const double *__restrict__ u,
                                                                 double *__restrict__ grad_csr) {
    const int64_t i = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    if (i >= total) return;
    const int32_t p = list[i];
    const int32_t end = esup_ptr[p + 1];
    for (int32_t pos = esup_ptr[p] + (int32_t)(threadIdx.x & 15); pos < end; pos += 16) grad_csr[pos] = u[esup[pos]];
}

template <class Id>
__global__ __launch_bounds__(TPB) void nin_mark_dirty_kernel(int64_t m, const Id *__restrict__ ids, int cells, int32_t E, int32_t P,
                                                              uint64_t npoel8, const int4 *__restrict__ inpoel, const int8_t *__restrict__ etype,
                                                              uint8_t *__restrict__ dirty, int32_t *__restrict__ rejected) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const int64_t id = (int64_t)ids[i];
    if (id < 0 || id >= (int64_t)(cells ? E : P)) {   // before any access through the id
        atomicAdd(rejected, 1);
        return;
    }
    if (!cells) {
        dirty[id] = 1;
        return;
    }
    const int4 a = inpoel[2 * id], b = inpoel[2 * id + 1];
    const int32_t q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const int n = (int)((npoel8 >> (8 * (etype[id] & 7))) & 0xff);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < n && q[j] >= 0 && q[j] < P) dirty[q[j]] = 1;   // (the builders checked every index; a damaged row marks nothing outside the array)
}

}  // namespace

int launch_adj_bin_byte(const int32_t *nodes, int32_t count, int32_t n_points, int bin, uint8_t *bin_of, hipStream_t stream) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL(nin_adj_bin_byte_kernel, blocks_for(count), dim3(TPB), 0, stream, nodes, count, n_points, (uint8_t)bin, bin_of);
    return launch_status();
}

size_t adj_dirty_hist_ints(int32_t n_points) { return (size_t)NK * blocks_for(n_points).x + 1; }

int adj_dirty_tmp_bytes(int32_t n_points, size_t *bytes) {
    *bytes = 0;
    int32_t *none = nullptr;
    return launch_status(hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, none, none, (int)adj_dirty_hist_ints(n_points), nullptr));
}

int launch_adj_dirty_compact(int32_t n_points, int clear, uint8_t *dirty, const uint8_t *bin_of, const int32_t *rejected, int32_t *hist,
                             int32_t *scanned, void *tmp, size_t tmp_bytes, int32_t *lists, int32_t *hdr, hipStream_t stream) {
    if (n_points <= 0) return 0;
    const int32_t nblocks = (int32_t)blocks_for(n_points).x;
    hipLaunchKernelGGL((nin_adj_dirty_compact_kernel<false>), dim3(nblocks), dim3(TPB), 0, stream, n_points, nblocks, 0, dirty, bin_of, rejected,
                       hist, lists, hdr);
    if (int rc = launch_status()) return rc;
    if (int rc = launch_status(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, hist, scanned, (int)adj_dirty_hist_ints(n_points), stream))) return rc;
    hipLaunchKernelGGL((nin_adj_dirty_compact_kernel<true>), dim3(nblocks), dim3(TPB), 0, stream, n_points, nblocks, clear, dirty, bin_of, rejected,
                       scanned, lists, hdr);
    return launch_status();
}

int launch_jac_seed_rows(const GridView &g, const int32_t *list, int32_t total, const double *u, double *grad_csr, hipStream_t stream) {
    if (total <= 0) return 0;
    hipLaunchKernelGGL(nin_jac_seed_rows_kernel, blocks_for(total, TPB / 16), dim3(TPB), 0, stream, g.esup_ptr,
                       g.esup, list, total, u, grad_csr);
    return launch_status();
}

int launch_mark_dirty(const GridView &g, uint64_t npoel8, const int32_t *inpoel, const int8_t *etype, const void *dev_ids, int ids_are_int64,
                      int64_t n, int ids_are_cells, uint8_t *dirty, int32_t *rejected, hipStream_t stream) {
    if (n <= 0) return 0;
    if (n > (int64_t)INT32_MAX * TPB) return fail(NIN_ERANGE, "%lld ids are more than one launch takes", (long long)n);
    const int4 *cells = reinterpret_cast<const int4 *>(inpoel);
    if (ids_are_int64)
        hipLaunchKernelGGL((nin_mark_dirty_kernel<int64_t>), blocks_for(n), dim3(TPB), 0, stream, n, static_cast<const int64_t *>(dev_ids),
                           ids_are_cells ? 1 : 0, g.n_elems, g.n_points, npoel8, cells, etype, dirty, rejected);
    else
        hipLaunchKernelGGL((nin_mark_dirty_kernel<int32_t>), blocks_for(n), dim3(TPB), 0, stream, n, static_cast<const int32_t *>(dev_ids),
                           ids_are_cells ? 1 : 0, g.n_elems, g.n_points, npoel8, cells, etype, dirty, rejected);
    return launch_status();
}

}  // namespace nin
