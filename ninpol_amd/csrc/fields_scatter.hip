// fields_scatter.hip -- local permeability updates: a SUBSET of cells rewritten from device memory, the nodes whose weights that
// can move marked, and the marked nodes binned by plan kernel (nin_fields_scatter_permeability_device, nin_weights_dirty_device).
//
// Which rows can move.  A GLS row of node n reads perm and diff_mag of the cells around n only; its face rows join two cells that
// both contain n.  So a change to cell e can move the rows of the vertices of e and no others (pinned on the oracle's own
// arithmetic by tests/test_update_local_host.py).
//
// Three kernels, no work counters:
//   nin_scatter_perm_kernel   a lane per entry i of the id list: perm[ids[i]] = K[i] (times scale[i]: one multiplication, rounded
//       once), diff_mag[ids[i]] = diff_mag_of(...) with fields_update.hip's arithmetic (same header, same -ffp-contract=off: the bits
//       are the host's), dirty[v] = 1 for the vertices v of the cell (inpoel / etype as nin_grid_update_points* keeps them).  The id
//       is checked against [0, E) BEFORE any access; a refused id writes nothing and adds one to a device counter.  The marks are
//       plain stores of 1: idempotent, no atomics.  Duplicate ids with the same row are harmless; with different rows one of them
//       wins and which one is unspecified (two lanes store to the same nine doubles, in no order).
//       The list is a small part of the mesh (that is the point of the path), so the 72-byte stride of a lane per row is left as it
//       is; what it costs is measured by tools/time_update_fields.py --local.
//   nin_dirty_compact_kernel<false / true>   count, (hipcub exclusive scan), fill: a workgroup of 256 threads takes 256 consecutive
//       nodes; a node's key is the plan kernel of its class byte (gls_plan.hpp: gls_class_kernel -- the table is walked, not copied;
//       IDW / LS: key 0 for every node).  Inside a wavefront the lanes of one key are ranked by ballot + popcount, the wavefronts of
//       a workgroup by four counters in LDS, the workgroups by the scan of hist[key][block] -- kernel-major, so the scanned value IS
//       the position in one flat buffer in which list k follows list k - 1, and every list is in ascending node id.  The fill pass
//       clears the marks it reads when asked to -- unless ids were refused since the last launch: then the caller gets an error and
//       the set must survive (the counter is read on the device; it was written by earlier kernels of the same stream).
//   nin_dirty_count_kernel    the number of marked nodes (nin_grid_dirty_nodes).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>

#include "diff_mag.hpp"
#include "launch.hpp"

namespace nin {

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int NK = kGlsPlanKernels;
static_assert(TPB == 256, "the compaction fills its class-byte table with one thread per byte value");


template <bool SCALED, class Id>
__global__ __launch_bounds__(TPB) void nin_scatter_perm_kernel(int64_t m, const Id *__restrict__ ids, const double *__restrict__ K,
                                                                const double *__restrict__ scale, int32_t E, int32_t P, uint64_t npoel8,
                                                                const int4 *__restrict__ inpoel, const int8_t *__restrict__ etype,
                                                                double *__restrict__ perm, double *__restrict__ diff_mag,
                                                                uint8_t *__restrict__ dirty, int32_t *__restrict__ rejected) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const int64_t e = (int64_t)ids[i];
    if (e < 0 || e >= (int64_t)E) {   // before any access through the id
        atomicAdd(rejected, 1);
        return;
    }
    double v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = K[i * 9 + k];
    if (SCALED) {
        const double s = scale[i];
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = s * v[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) perm[e * 9 + k] = v[k];
    diff_mag[e] = diff_mag_of(v[0], v[4], v[8]);
    const int4 a = inpoel[2 * e], b = inpoel[2 * e + 1];
    const int32_t q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const int n = (int)((npoel8 >> (8 * (etype[e] & 7))) & 0xff);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < n && q[j] >= 0 && q[j] < P) dirty[q[j]] = 1;   // (the builders checked every index; a damaged row marks nothing outside the array)
}

// hist: [NK][nblocks] + one int.  FILL = false writes the counts (and 0 into the last int); FILL = true reads their exclusive scan.
template <bool FILL>
__global__ __launch_bounds__(TPB) void nin_dirty_compact_kernel(int32_t P, int32_t nblocks, int single, int clear, uint8_t *__restrict__ dirty,
                                                                 const uint8_t *__restrict__ cls, const int32_t *__restrict__ rejected,
                                                                 int32_t *__restrict__ hist, int32_t *__restrict__ lists,
                                                                 int32_t *__restrict__ hdr) {
    __shared__ int32_t wave_cnt[WAVES][NK];
    __shared__ int8_t kernel_of[256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    kernel_of[tid] = single ? (int8_t)0 : (int8_t)gls_class_kernel(tid);
    for (int i = tid; i < WAVES * NK; i += TPB) (&wave_cnt[0][0])[i] = 0;
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * TPB + tid;
    bool has = p < P && dirty[p] != 0;
    const int key = has ? (int)kernel_of[cls[p]] : -1;
    has = has && key >= 0;   // (nin_grid_to_device refuses a class byte that belongs to no kernel)
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
        if (blockIdx.x == 0 && tid <= NK) hdr[kDirtyHdrOffsets + tid] = hist[(int64_t)tid * nblocks];   // where list tid begins; [NK]: the total
    }
}

__global__ __launch_bounds__(TPB) void nin_dirty_count_kernel(int32_t P, const uint8_t *__restrict__ dirty, int32_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const unsigned long long mk = __ballot(p < P && dirty[p] != 0);
    if ((threadIdx.x & 63) == 0 && mk) atomicAdd(out, (int32_t)__popcll(mk));
}

template <bool SCALED, class Id>
void scatter_variant(int64_t n, const void *ids, const double *K, const double *scale, const GridView &g, uint64_t npoel8, const int32_t *inpoel,
                     const int8_t *etype, uint8_t *dirty, int32_t *rejected, hipStream_t stream) {
    hipLaunchKernelGGL((nin_scatter_perm_kernel<SCALED, Id>), blocks_for(n), dim3(TPB), 0, stream, n, static_cast<const Id *>(ids), K, scale,
                       g.n_elems, g.n_points, npoel8, reinterpret_cast<const int4 *>(inpoel), etype, const_cast<double *>(g.perm),
                       const_cast<double *>(g.diff_mag), dirty, rejected);
}

}  // namespace

int launch_scatter_permeability(const GridView &g, uint64_t npoel8, const int32_t *inpoel, const int8_t *etype, const void *dev_ids,
                                int ids_are_int64, int64_t n, const double *dev_K, const double *dev_scale, uint8_t *dirty, int32_t *rejected,
                                hipStream_t stream) {
    if (n <= 0) return 0;
    if (n > (int64_t)INT32_MAX * TPB) return fail(NIN_ERANGE, "%lld ids are more than one launch takes", (long long)n);
    if (dev_scale) {
        if (ids_are_int64) scatter_variant<true, int64_t>(n, dev_ids, dev_K, dev_scale, g, npoel8, inpoel, etype, dirty, rejected, stream);
        else scatter_variant<true, int32_t>(n, dev_ids, dev_K, dev_scale, g, npoel8, inpoel, etype, dirty, rejected, stream);
    } else {
        if (ids_are_int64) scatter_variant<false, int64_t>(n, dev_ids, dev_K, dev_scale, g, npoel8, inpoel, etype, dirty, rejected, stream);
        else scatter_variant<false, int32_t>(n, dev_ids, dev_K, dev_scale, g, npoel8, inpoel, etype, dirty, rejected, stream);
    }
    return launch_status();
}

size_t dirty_compact_hist_ints(int32_t n_points) { return (size_t)NK * blocks_for(n_points).x + 1; }

int dirty_compact_tmp_bytes(int32_t n_points, size_t *bytes) {
    *bytes = 0;
    int32_t *none = nullptr;
    return launch_status(hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, none, none, (int)dirty_compact_hist_ints(n_points), nullptr));
}

int launch_dirty_compact(int32_t n_points, int single, int clear, uint8_t *dirty, const uint8_t *node_class, const int32_t *rejected,
                         int32_t *hist, int32_t *scanned, void *tmp, size_t tmp_bytes, int32_t *lists, int32_t *hdr, hipStream_t stream) {
    if (n_points <= 0) return 0;
    const int32_t nblocks = (int32_t)blocks_for(n_points).x;
    hipLaunchKernelGGL((nin_dirty_compact_kernel<false>), dim3(nblocks), dim3(TPB), 0, stream, n_points, nblocks, single, 0, dirty, node_class, rejected,
                       hist, lists, hdr);
    if (int rc = launch_status()) return rc;
    if (int rc = launch_status(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, hist, scanned, (int)dirty_compact_hist_ints(n_points), stream))) return rc;
    hipLaunchKernelGGL((nin_dirty_compact_kernel<true>), dim3(nblocks), dim3(TPB), 0, stream, n_points, nblocks, single, clear, dirty, node_class, rejected,
                       scanned, lists, hdr);
    return launch_status();
}

int launch_dirty_count(int32_t n_points, const uint8_t *dirty, int32_t *out, hipStream_t stream) {
    if (n_points <= 0) return 0;
    hipLaunchKernelGGL(nin_dirty_count_kernel, blocks_for(n_points), dim3(TPB), 0, stream, n_points, dirty, out);
    return launch_status();
}

}  // namespace nin
