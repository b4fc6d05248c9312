// csr_patch.cpp -- the host half of an incremental interpolate(): m recomputed rows, packed by csr_dirty.hip and
// brought over PCIe, go into the CSR matrix the caller holds.  No HIP in here: plain OpenMP loops on the library's own team
// (host_threads.hpp), callable without a GPU.
#include <omp.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ninpol_amd.h"
#include "host_threads.hpp"

namespace {

// out[0] = 0, out[p + 1] = out[p] + len[p + 1] for the row lengths the caller left in out[1 .. P]: two passes over one chunk per
// thread.  Returns the total (it may not fit the int32 the entries have: the caller checks).
int64_t scan_row_lengths(int64_t P, int32_t *out) {
    const int nt = nin::host_team();
    std::vector<int64_t> chunk_sum((size_t)nt + 1, 0);
#pragma omp parallel num_threads(nt)
    {
        const int t = omp_get_thread_num(), n = omp_get_num_threads();
        const int64_t b = P * t / n, e = P * (t + 1) / n;
        int64_t s = 0;
        for (int64_t p = b; p < e; ++p) s += out[p + 1];
        chunk_sum[(size_t)t + 1] = s;
#pragma omp barrier
#pragma omp single
        for (int k = 0; k < n; ++k) chunk_sum[(size_t)k + 1] += chunk_sum[(size_t)k];
        // (the implicit barrier of `single`: every thread sees the seeds; a total beyond int32 is refused before anyone reads the result)
        int64_t at = chunk_sum[(size_t)t];
        for (int64_t p = b; p < e; ++p) {
            at += out[p + 1];
            out[p + 1] = (int32_t)at;
        }
        if (t == n - 1) chunk_sum[(size_t)nt] = at;
    }
    out[0] = 0;
    return P > 0 ? chunk_sum[(size_t)nt] : 0;
}

}  // namespace

extern "C" int nin_csr_patch_rows(int64_t P, const int32_t *indptr, int32_t *indices, double *data, double *nws, int64_t m,
                                  const int32_t *nodes, const int32_t *counts, const int32_t *off, const int32_t *pack_indices,
                                  const double *pack_data, const double *pack_nws, int32_t *out_indptr, int32_t *out_indices,
                                  double *out_data) {
    if (P < 0 || m < 0 || !indptr || !indices || !data || !nws || !nodes || !counts || !off || !pack_indices || !pack_data || !pack_nws)
        return NIN_EINVAL;
    const bool in_place = !out_indptr && !out_indices && !out_data;
    if (!in_place && (!out_indptr || !out_indices || !out_data)) return NIN_EINVAL;
    // ---- everything is checked before anything is written ----
    if (off[0] != 0) return NIN_EINVAL;
    std::vector<uint64_t> listed(((size_t)P + 63) / 64, 0);   // one bit per row: set for the rows of `nodes` (1.25 MB at 10 M rows)
    int bad = 0;
#pragma omp parallel for schedule(static) reduction(| : bad) num_threads(nin::host_team())
    for (int64_t i = 0; i < m; ++i) {
        const int64_t p = nodes[i];
        if (p < 0 || p >= P || counts[i] < 0 || (int64_t)off[i + 1] - off[i] != counts[i]) { bad |= 1; continue; }
        const uint64_t bit = 1ull << (p & 63);
        if (__atomic_fetch_or(&listed[(size_t)(p >> 6)], bit, __ATOMIC_RELAXED) & bit) bad |= 1;   // a duplicate
        if (in_place && counts[i] != indptr[p + 1] - indptr[p]) bad |= 1;                            // a new structure needs out_*
    }
    if (bad) return NIN_EINVAL;
    if (in_place) {
        // equal counts do not imply an equal pattern (a weight that became zero next to one that stopped being zero): indices too
#pragma omp parallel for schedule(static) num_threads(nin::host_team())
        for (int64_t i = 0; i < m; ++i) {
            const int64_t p = nodes[i];
            const size_t n = (size_t)counts[i];
            if (n) {
                std::memcpy(indices + indptr[p], pack_indices + off[i], n * sizeof(int32_t));
                std::memcpy(data + indptr[p], pack_data + off[i], n * sizeof(double));
            }
            nws[p] = pack_nws[i];
        }
        return NIN_OK;
    }
    // ---- a new structure: the row lengths (old ones, the listed rows' replaced), their prefix sum, then the segments ----
#pragma omp parallel for schedule(static) num_threads(nin::host_team())
    for (int64_t p = 0; p < P; ++p) out_indptr[p + 1] = indptr[p + 1] - indptr[p];
#pragma omp parallel for schedule(static) num_threads(nin::host_team())
    for (int64_t i = 0; i < m; ++i) out_indptr[(int64_t)nodes[i] + 1] = counts[i];
    if (scan_row_lengths(P, out_indptr) > INT32_MAX) return NIN_ERANGE;   // (out_indptr is the caller's scratch until the call succeeds)
#pragma omp parallel for schedule(static, 4096) num_threads(nin::host_team())
    for (int64_t p = 0; p < P; ++p) {
        if ((listed[(size_t)(p >> 6)] >> (p & 63)) & 1) continue;
        const size_t n = (size_t)(indptr[p + 1] - indptr[p]);
        if (n) {
            std::memcpy(out_indices + out_indptr[p], indices + indptr[p], n * sizeof(int32_t));
            std::memcpy(out_data + out_indptr[p], data + indptr[p], n * sizeof(double));
        }
    }
#pragma omp parallel for schedule(static) num_threads(nin::host_team())
    for (int64_t i = 0; i < m; ++i) {
        const int64_t p = nodes[i];
        const size_t n = (size_t)counts[i];
        if (n) {
            std::memcpy(out_indices + out_indptr[p], pack_indices + off[i], n * sizeof(int32_t));
            std::memcpy(out_data + out_indptr[p], pack_data + off[i], n * sizeof(double));
        }
        nws[p] = pack_nws[i];
    }
    return NIN_OK;
}
