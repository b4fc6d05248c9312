// abi_csr.hip -- the C ABI, part 4: from the weights in esup position to a CSR matrix on the host -- count, scan and compaction with
// the transfers under them, interpolate()'s pipeline -- and the host matrix that takes only the dirty rows.
#include <hipcub/hipcub.hpp>
#include <new>

#include "abi_internal.hpp"

using namespace nin;

namespace {

int e2e_streams(DeviceGrid &d) {
    int rc = lazy_stream(d.copy_stream);
    if (!rc) rc = lazy_event(d.ev_weights);
    if (!rc) rc = lazy_event(d.ev_scan);
    return rc;
}

// The grid's scratch of the CSR finish, allocated on first need and kept (sized by the mesh): P + 1 row counters and row pointers;
// with `entries`, room for every entry of esup; a scan temporary of at least tmp_bytes (a smaller one stays in d.allocs until the
// grid goes)
int ensure_e2e_scratch(DeviceGrid &d, int64_t P, bool entries, size_t tmp_bytes) {
    int rc = NIN_OK;
    const size_t cap = (size_t)std::max<int64_t>(d.nnz_e, 1);
    if (!d.e2e_cnt && (rc = dev_alloc(d, &d.e2e_cnt, (size_t)(P + 1)))) return rc;
    if (!d.e2e_ptr && (rc = dev_alloc(d, &d.e2e_ptr, (size_t)(P + 1)))) return rc;
    if (entries && !d.e2e_indices && (rc = dev_alloc(d, &d.e2e_indices, cap))) return rc;
    if (entries && !d.e2e_data && (rc = dev_alloc(d, &d.e2e_data, cap))) return rc;
    if (tmp_bytes > d.e2e_tmp_bytes) {
        char *t = nullptr;
        if ((rc = dev_alloc(d, &t, std::max<size_t>(tmp_bytes, 16)))) return rc;
        d.e2e_tmp = t;
        d.e2e_tmp_bytes = tmp_bytes;
    }
    return NIN_OK;
}

// The finish of interpolator.pyx:622-624 with the transfers overlapped: dev_nws / neumann_ws (optional) ride the copy stream under the
// count / scan / compaction kernels, as does indptr; indices and data follow in pieces, each as soon as the copy engine is free.
int csr_compact_pipelined(nin_grid *g, const double *dev_csr_data, const double *dev_nws, int32_t *indptr, int32_t *indices,
                          double *data, int64_t *nnz_out, double *neumann_ws, hipStream_t stream) {
    DeviceGrid &d = g->d;
    const int64_t P = g->h.n_points;
    size_t tmp_bytes = 0;
    int rc = NIN_OK;
    Laps L{"nin_e2e", 22};
    if ((rc = e2e_streams(d))) return rc;
    hipStream_t cs = static_cast<hipStream_t>(d.copy_stream);
    hipEvent_t ev_w = static_cast<hipEvent_t>(d.ev_weights), ev_s = static_cast<hipEvent_t>(d.ev_scan);
    if ((rc = ensure_e2e_scratch(d, P, false, 0))) return rc;
    int32_t *cnt = d.e2e_cnt, *ptr = d.e2e_ptr;
    if (dev_nws && neumann_ws) {   // 8 B per node: leaves as soon as the weight kernels are done
        HIP_TRY(hipEventRecord(ev_w, stream));
        HIP_TRY(hipStreamWaitEvent(cs, ev_w, 0));
        HIP_TRY(hipMemcpyAsync(neumann_ws, dev_nws, (size_t)P * 8, hipMemcpyDeviceToHost, cs));
    }
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)(P + 1) * 4, stream));
    if ((rc = launch_row_nnz(d.v, dev_csr_data, cnt, stream))) return fail(rc, "launch failed");
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt, ptr, (int)(P + 1), stream));
    if ((rc = ensure_e2e_scratch(d, P, false, tmp_bytes))) return rc;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d.e2e_tmp, tmp_bytes, cnt, ptr, (int)(P + 1), stream));
    HIP_TRY(hipEventRecord(ev_s, stream));
    const bool want_entries = indices && data;
    if (want_entries) {   // the compaction does not need the count on the host: it starts right behind the scan
        if ((rc = ensure_e2e_scratch(d, P, true, 0))) return rc;
        if ((rc = launch_compact(d.v, dev_csr_data, ptr, d.e2e_indices, d.e2e_data, stream))) return fail(rc, "launch failed");
    }
    HIP_TRY(hipStreamWaitEvent(cs, ev_s, 0));
    HIP_TRY(hipMemcpyAsync(indptr, ptr, (size_t)(P + 1) * 4, hipMemcpyDeviceToHost, cs));   // under the compaction kernel
    HIP_TRY(hipStreamSynchronize(cs));
    L.lap("weights+count+scan");
    const int64_t nnz = indptr[P];
    *nnz_out = nnz;
    if (nnz > 0 && want_entries) {
        HIP_TRY(hipStreamSynchronize(stream));
        L.lap("compaction");
        // two copy queues: the index and the value stream each keep a DMA engine busy
        HIP_TRY(hipMemcpyAsync(indices, d.e2e_indices, (size_t)nnz * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(data, d.e2e_data, (size_t)nnz * 8, hipMemcpyDeviceToHost, cs));
        HIP_TRY(hipStreamSynchronize(cs));
        HIP_TRY(hipStreamSynchronize(stream));
        L.lap("D2H indices+data");
    }
    return NIN_OK;
}

// The weight kernels for the nodes of chunk k only (all nodes of the chunk, add_neumann fused): sub-ranges of the launch plan's lists.
int weights_chunk(nin_grid *g, int method, int k, double *out, double *nws, hipStream_t stream) {
    DeviceGrid &d = g->d;
    const int32_t P = (int32_t)g->h.n_points;
    if (method != NIN_METHOD_GLS)
        return launch_rows_range(d.v, method == NIN_METHOD_LS ? 1 : 0, P, d.chunk_node[k], d.chunk_node[k + 1],
                                 (int32_t)g->h.mx_elems_per_point, d.nnz_e, out, nws, stream);
    HIP_TRY(hipMemsetAsync(d.gls_queue, 0, kGlsQueueInts * sizeof(int32_t), stream));   // the launches' work counters
    int rc = gls_side_begin(d, k, 1, out, nws, stream);
    if (!rc) rc = gls_main(d, k, true, -1, 1, out, nws, stream);
    return rc;
}

// interpolate() as a pipeline over kE2eChunks pieces of the node range: while piece k's surviving entries cross PCIe (the floor
// of this path: 0.95 GB at 57 GB/s = 16.7 ms at 10 M cells), piece k + 1 is computed, counted, scanned and compacted.  Per piece:
// weight kernels -> non-zeros per row -> exclusive scan seeded with the entries of the pieces before -> (4 bytes back: the
// running total) -> compaction -> its slices of indptr / indices / data leave on the copy queues.  After an error the caller drains them.
int interpolate_chunked(nin_grid *g, int method, int32_t *indptr, int32_t *indices, double *data, int64_t *nnz_out,
                        double *neumann_ws) {
    DeviceGrid &d = g->d;
    constexpr int K = DeviceGrid::kE2eChunks;
    const int64_t P = g->h.n_points;
    Laps L{"nin_e2e", 22};
    int rc = NIN_OK;
    if ((rc = e2e_streams(d))) return rc;
    hipStream_t cs = static_cast<hipStream_t>(d.copy_stream), stream = nullptr;
    hipEvent_t ev = static_cast<hipEvent_t>(d.ev_scan);
    if ((rc = ensure_e2e_scratch(d, P, true, 0))) return rc;
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveScan(nullptr, tmp_bytes, d.e2e_cnt, d.e2e_ptr, hipcub::Sum(), (int32_t)0, (int)(P + 1), stream));
    if ((rc = ensure_e2e_scratch(d, P, true, tmp_bytes))) return rc;
    HIP_TRY(hipMemsetAsync(d.e2e_cnt, 0, (size_t)(P + 1) * 4, stream));
    int32_t base = 0;
    for (int k = 0; k < K; ++k) {
        const int32_t pb = d.chunk_node[k], pe = d.chunk_node[k + 1];
        if (pe <= pb) continue;
        if ((rc = weights_chunk(g, method, k, d.e2e_weights, d.e2e_nws, stream))) return rc;
        if ((rc = launch_row_nnz(d.v, d.e2e_weights, d.e2e_cnt, stream, pb, pe))) return fail(rc, "launch failed");
        size_t tb = d.e2e_tmp_bytes;
        // ptr[pb .. pe] (one past the piece: the next piece's seed and, in the end, nnz); cnt[pe] is not part of that sum
        HIP_TRY(hipcub::DeviceScan::ExclusiveScan(d.e2e_tmp, tb, d.e2e_cnt + pb, d.e2e_ptr + pb, hipcub::Sum(), base, (int)(pe - pb + 1), stream));
        if ((rc = launch_compact(d.v, d.e2e_weights, d.e2e_ptr, d.e2e_indices, d.e2e_data, stream, pb, pe))) return fail(rc, "launch failed");
        int32_t next_base = 0;
        HIP_TRY(hipMemcpyAsync(&next_base, d.e2e_ptr + pe, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(ev, stream));
        HIP_TRY(hipStreamSynchronize(stream));             // (the piece is compacted; the copies of the piece before still run)
        const int64_t n_k = (int64_t)next_base - base;
        // this piece's slices: rows on the copy stream, entries split over two queues
        HIP_TRY(hipMemcpyAsync(indptr + pb, d.e2e_ptr + pb, (size_t)(pe - pb + (k == K - 1 ? 1 : 0)) * 4, hipMemcpyDeviceToHost, cs));
        HIP_TRY(hipMemcpyAsync(neumann_ws + pb, d.e2e_nws + pb, (size_t)(pe - pb) * 8, hipMemcpyDeviceToHost, cs));
        if (n_k > 0) {
            HIP_TRY(hipMemcpyAsync(data + base, d.e2e_data + base, (size_t)n_k * 8, hipMemcpyDeviceToHost, cs));
            if ((rc = lazy_stream(d.copy_stream2))) return rc;   // (the second copy queue: opened by the first piece that has entries)
            HIP_TRY(hipMemcpyAsync(indices + base, d.e2e_indices + base, (size_t)n_k * 4, hipMemcpyDeviceToHost,
                                 static_cast<hipStream_t>(d.copy_stream2)));
        }
        base = next_base;
        if (L.on) { char nm[32]; snprintf(nm, sizeof nm, "piece %d computed", k); L.lap(nm); }
    }
    HIP_TRY(hipStreamSynchronize(cs));
    if (d.copy_stream2) HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream2)));
    L.lap("copies drained");
    *nnz_out = base;
    return NIN_OK;
}

}  // namespace

int nin_csr_compact_host(nin_grid *g, const double *dev_csr_data, int32_t *indptr, int32_t *indices, double *data,
                         int64_t *nnz_out, void *stream_) {
    if (!g || !dev_csr_data || !indptr || !nnz_out) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, "", false)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    return csr_compact_pipelined(g, dev_csr_data, nullptr, indptr, indices, data, nnz_out, nullptr,
                                 static_cast<hipStream_t>(stream_));
}

int nin_interpolate_csr_host(nin_grid *g, int method, int32_t *indptr, int32_t *indices, double *data,
                             int64_t *nnz_out, double *neumann_ws) {
    if (!g || !indptr || !indices || !data || !nnz_out || !neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintWeights, false)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    int rc = NIN_OK;
    if (!d.e2e_weights && (rc = dev_alloc(d, &d.e2e_weights, (size_t)std::max<int64_t>(d.nnz_e, 1)))) return rc;
    if (!d.e2e_nws && (rc = dev_alloc(d, &d.e2e_nws, (size_t)std::max<int64_t>(g->h.n_points, 1)))) return rc;
    if (d.chunkable) {
        if ((rc = weights_ready(d, method))) return rc;
        if ((rc = interpolate_chunked(g, method, indptr, indices, data, nnz_out, neumann_ws))) {
            // an error in the middle must not leave copies into the caller's buffers in flight
            if (d.copy_stream) (void)hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream));
            if (d.copy_stream2) (void)hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream2));
            (void)hipStreamSynchronize(nullptr);   // (the pipeline's own stream)
        }
        return rc;
    }
    rc = nin_weights_device(g, method, nullptr, 0, 1, d.e2e_weights, d.e2e_nws, nullptr);
    if (!rc) rc = csr_compact_pipelined(g, d.e2e_weights, d.e2e_nws, indptr, indices, data, nnz_out, neumann_ws, nullptr);
    return rc;
}

// ---- a host matrix kept current: only the dirty rows cross PCIe (csr_dirty.hip, csr_patch.cpp) ----------------------
struct nin_hostmatrix {
    nin_grid *g = nullptr;
    int method = 0;
    int device = -1;                // the grid's, as it was at creation: nin_hostmatrix_destroy does not look at the grid, which may be gone
    // the matrix's own device state: weights in esup position, neumann_ws, surviving entries per row (not the grid's e2e_* scratch,
    // which any interpolate() overwrites)
    double *weights = nullptr, *nws = nullptr;
    int32_t *cnt = nullptr;
    bool weights_current = false;   // nin_hostmatrix_update found every node dirty and ran the full launch: nin_hostmatrix_full finishes it
    // scratch of an update, sized by the dirty list and grown on demand: per listed row (pack_off has two more: the total and the
    // counter of rows whose count changed, read back together) and per packed entry; the same again page-locked on the host
    size_t rows_cap = 0, entries_cap = 0, h_rows_cap = 0, h_entries_cap = 0;
    int32_t *pack_cnt = nullptr, *pack_off = nullptr, *pack_node = nullptr, *pack_indices = nullptr;
    double *pack_nws = nullptr, *pack_data = nullptr;
    void *scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
    int32_t *h_cnt = nullptr, *h_off = nullptr, *h_node = nullptr, *h_indices = nullptr;
    double *h_nws = nullptr, *h_data = nullptr;
    int64_t pending_rows = -1;      // rows of the last update whose pack is on its way to the host (nin_hostmatrix_patch takes them)
};

namespace {

template <class T>
int hm_grow(T **buf, size_t count, bool on_host) {
    if (*buf) (void)(on_host ? hipHostFree(*buf) : hipFree(*buf));
    *buf = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    const hipError_t e = on_host ? hipHostMalloc((void **)buf, bytes, hipHostMallocDefault) : hipMalloc((void **)buf, bytes);
    return e == hipSuccess ? NIN_OK : fail(NIN_ENOMEM, "%s(%zu bytes): %s", on_host ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
}

// room for `rows` listed rows and `entries` packed entries, on the device or in page-locked host memory (half as much again: a time
// loop's dirty set wobbles).  Growing frees first, which waits for the device: nothing of an earlier update is in flight by then.
int hm_reserve(nin_hostmatrix *m, size_t rows, size_t entries, bool on_host) {
    size_t &rc_ = on_host ? m->h_rows_cap : m->rows_cap, &ec_ = on_host ? m->h_entries_cap : m->entries_cap;
    int rc = NIN_OK;
    if (rows > rc_) {
        const size_t n = rows + rows / 2;
        rc_ = 0;
        if (!rc) rc = hm_grow(on_host ? &m->h_cnt : &m->pack_cnt, n + 1, on_host);
        if (!rc) rc = hm_grow(on_host ? &m->h_off : &m->pack_off, n + 2, on_host);
        if (!rc) rc = hm_grow(on_host ? &m->h_node : &m->pack_node, n, on_host);
        if (!rc) rc = hm_grow(on_host ? &m->h_nws : &m->pack_nws, n, on_host);
        if (rc) return rc;
        rc_ = n;
    }
    if (entries > ec_ || !(on_host ? m->h_data : m->pack_data)) {
        const size_t n = entries + entries / 2;
        ec_ = 0;
        if (!rc) rc = hm_grow(on_host ? &m->h_indices : &m->pack_indices, n, on_host);
        if (!rc) rc = hm_grow(on_host ? &m->h_data : &m->pack_data, n, on_host);
        if (rc) return rc;
        ec_ = n;
    }
    return NIN_OK;
}

}  // namespace

int nin_hostmatrix_create(nin_grid *g, int method, nin_hostmatrix **out) {
    if (!g || !out) return fail(NIN_EINVAL, "NULL argument");
    *out = nullptr;
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintToDevice)) return rc;
    if (method != NIN_METHOD_GLS && method != NIN_METHOD_IDW && method != NIN_METHOD_LS) return fail(NIN_EINVAL, "unknown method %d", method);
    HIP_TRY(hipSetDevice(d.device));
    nin_hostmatrix *m = new (std::nothrow) nin_hostmatrix();
    if (!m) return fail(NIN_ENOMEM, "out of host memory");
    m->g = g;
    m->method = method;
    m->device = d.device;
    int rc = hm_grow(&m->weights, (size_t)d.nnz_e, false);
    if (!rc) rc = hm_grow(&m->nws, (size_t)g->h.n_points, false);
    if (!rc) rc = hm_grow(&m->cnt, (size_t)g->h.n_points, false);
    if (rc) { nin_hostmatrix_destroy(m); return rc; }
    *out = m;
    return NIN_OK;
}

void nin_hostmatrix_destroy(nin_hostmatrix *m) {
    if (!m) return;
    if (m->device >= 0) (void)hipSetDevice(m->device);
    for (void *p : {(void *)m->weights, (void *)m->nws, (void *)m->cnt, (void *)m->pack_cnt, (void *)m->pack_off, (void *)m->pack_node,
                    (void *)m->pack_indices, (void *)m->pack_nws, (void *)m->pack_data, m->scan_tmp})
        if (p) (void)hipFree(p);   // (waits for the device)
    for (void *p : {(void *)m->h_cnt, (void *)m->h_off, (void *)m->h_node, (void *)m->h_indices, (void *)m->h_nws, (void *)m->h_data})
        if (p) (void)hipHostFree(p);
    delete m;
}

int nin_hostmatrix_full(nin_hostmatrix *m, int32_t *indptr, int32_t *indices, double *data, double *neumann_ws, int64_t *nnz_out,
                        void *stream_) {
    if (!m || !indptr || !indices || !data || !neumann_ws || !nnz_out) return fail(NIN_EINVAL, "NULL argument");
    nin_grid *g = m->g;
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintWeights)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = NIN_OK;
    if (!m->weights_current) {   // (else nin_hostmatrix_update has run the launch and cleared the set)
        if ((rc = nin_weights_device(g, m->method, nullptr, 0, 1, m->weights, m->nws, stream_))) return rc;
        if ((rc = nin_grid_dirty_reset(g, 0, stream_))) return rc;
    }
    m->weights_current = false;
    m->pending_rows = -1;
    // the existing finish: count, scan and compaction in the grid's scratch, the transfers under them; the row counts stay with the matrix
    rc = csr_compact_pipelined(g, m->weights, m->nws, indptr, indices, data, nnz_out, neumann_ws, stream);
    if (!rc) {
        const hipError_t e = hipMemcpyAsync(m->cnt, d.e2e_cnt, (size_t)g->h.n_points * sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) rc = fail(NIN_EHIP, "keeping the row counts: %s", hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess && !rc) rc = fail(NIN_EHIP, "full run of the host matrix: %s", hipGetErrorString(e));
    if (rc) d.all_dirty = true;   // the matrix holds no full result: the next update starts over
    return rc;
}

int nin_hostmatrix_update(nin_hostmatrix *m, int clear, void *stream_, int64_t *n_rows, int64_t *n_changed, int64_t *n_entries) {
    if (!m || !n_rows || !n_changed || !n_entries) return fail(NIN_EINVAL, "NULL argument");
    *n_rows = *n_changed = *n_entries = 0;
    nin_grid *g = m->g;
    DeviceGrid &d = g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (m->pending_rows >= 0) {   // an update nobody patched in: its copies must not be in flight when the staging buffers are reused
        (void)hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream));
        (void)hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream2));
        m->pending_rows = -1;
        d.all_dirty = true;       // ... and the host's arrays missed those rows
    }
    const bool full = d.all_dirty;
    Laps L{"nin_hostmatrix", 14};   // (each lap waits for the work it names)
    int64_t n = 0;
    // refused ids: nothing is launched, the matrix and the set stay as they are (nin_weights_dirty_device's contract)
    int rc = nin_weights_dirty_device(g, m->method, 1, m->weights, m->nws, stream_, clear, &n);
    if (rc) return rc;
    *n_rows = n;
    if (full) {   // every row was launched: the ordinary finish follows (nin_hostmatrix_full)
        m->weights_current = true;
        *n_entries = -1;
        return NIN_OK;
    }
    if (n == 0) return NIN_OK;
    L.lap("dirty launch", {stream});
    const int32_t total = (int32_t)n;
    // what the rows of the list can hold at most: the pack's size is not known on the host before the kernels that fill it are enqueued
    const size_t bound = (size_t)std::min<int64_t>(n * std::max<int64_t>(g->h.mx_elems_per_point, 1), d.nnz_e);
    size_t tmp_bytes = 0;
    int32_t back[2] = {0, 0};   // pack_off[total] = the packed entries, pack_off[total + 1] = the rows whose count changed
    auto step = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && !rc) rc = fail(NIN_EHIP, "%s: %s", what, hipGetErrorString(e));
        return rc == NIN_OK;
    };
    rc = hm_reserve(m, (size_t)total, bound, false);
    if (!rc) rc = e2e_streams(d);
    if (!rc) rc = lazy_stream(d.copy_stream2);
    hipStream_t cs = static_cast<hipStream_t>(d.copy_stream), cs2 = static_cast<hipStream_t>(d.copy_stream2);
    hipEvent_t ev_scan = static_cast<hipEvent_t>(d.ev_scan), ev_pack = static_cast<hipEvent_t>(d.ev_weights);
    if (!rc && step(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, m->pack_cnt, m->pack_off, total + 1, stream), "sizing the scan") &&
        tmp_bytes > m->scan_tmp_bytes) {
        m->scan_tmp_bytes = 0;
        if (!(rc = hm_grow(reinterpret_cast<char **>(&m->scan_tmp), std::max<size_t>(tmp_bytes, 16), false))) m->scan_tmp_bytes = std::max<size_t>(tmp_bytes, 16);
    }
    if (!rc) {
        (void)(step(hipMemsetAsync(m->pack_cnt + total, 0, sizeof(int32_t), stream), "hipMemsetAsync") &&
               step(hipMemsetAsync(m->pack_off + total + 1, 0, sizeof(int32_t), stream), "hipMemsetAsync"));
        if (!rc) rc = launch_dirty_row_nnz(d.v, m->weights, d.dirty_lists, total, m->pack_cnt, m->cnt, m->pack_off + total + 1, stream);
        size_t tb = m->scan_tmp_bytes;
        // the sizes leave on the copy stream as soon as the scan is done, under the pack kernel: the call's second and last wait
        (void)(step(hipcub::DeviceScan::ExclusiveSum(m->scan_tmp, tb, m->pack_cnt, m->pack_off, total + 1, stream), "scan of the row counts") &&
               step(hipEventRecord(ev_scan, stream), "hipEventRecord") && step(hipStreamWaitEvent(cs, ev_scan, 0), "hipStreamWaitEvent") &&
               step(hipMemcpyAsync(back, m->pack_off + total, sizeof back, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync"));
        if (!rc)
            rc = launch_dirty_pack(d.v, m->weights, m->nws, d.dirty_lists, total, m->pack_off, m->pack_node, m->pack_nws, m->pack_indices, m->pack_data, stream);
        (void)(step(hipEventRecord(ev_pack, stream), "hipEventRecord") && step(hipStreamSynchronize(cs), "reading the pack's size back"));
    }
    if (!rc && (back[0] < 0 || (size_t)back[0] > bound || back[1] < 0 || back[1] > total))
        rc = fail(NIN_EHIP, "the pack holds %d entries (room for %zu) and %d changed rows of %d", (int)back[0], bound, (int)back[1], (int)total);
    L.lap("count + pack", {stream});
    if (!rc) rc = hm_reserve(m, (size_t)total, (size_t)back[0], true);
    if (!rc) {
        const size_t rows = (size_t)total, ents = (size_t)back[0];
        (void)(step(hipStreamWaitEvent(cs, ev_pack, 0), "hipStreamWaitEvent") && step(hipStreamWaitEvent(cs2, ev_pack, 0), "hipStreamWaitEvent") &&
               step(hipMemcpyAsync(m->h_node, m->pack_node, rows * 4, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync") &&
               step(hipMemcpyAsync(m->h_cnt, m->pack_cnt, rows * 4, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync") &&
               step(hipMemcpyAsync(m->h_off, m->pack_off, (rows + 1) * 4, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync") &&
               step(hipMemcpyAsync(m->h_nws, m->pack_nws, rows * 8, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync"));
        if (!rc && ents)   // two copy queues, as interpolate()'s pipeline: the index and the value stream each keep a DMA engine busy
            (void)(step(hipMemcpyAsync(m->h_data, m->pack_data, ents * 8, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync") &&
                   step(hipMemcpyAsync(m->h_indices, m->pack_indices, ents * 4, hipMemcpyDeviceToHost, cs2), "hipMemcpyAsync"));
    }
    if (rc) {   // rows were rewritten on the device that the host will not get: everything counts as dirty again
        (void)hipStreamSynchronize(stream); (void)hipStreamSynchronize(cs);
        if (cs2) (void)hipStreamSynchronize(cs2);
        d.all_dirty = true;
        return rc;
    }
    L.lap("D2H", {cs, cs2});
    m->pending_rows = total;
    *n_changed = back[1];
    *n_entries = back[0];
    return NIN_OK;
}

int nin_hostmatrix_patch(nin_hostmatrix *m, const int32_t *indptr, int32_t *indices, double *data, double *neumann_ws, int32_t *out_indptr,
                         int32_t *out_indices, double *out_data) {
    if (!m || !indptr || !indices || !data || !neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    if (m->pending_rows < 0) return fail(NIN_ESTATE, "no update is waiting to be patched in (nin_hostmatrix_update first)");
    DeviceGrid &d = m->g->d;
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(d.copy_stream2)));
    Laps L{"nin_hostmatrix", 14};   // (each lap waits for the work it names)
    const int64_t rows = m->pending_rows;
    m->pending_rows = -1;
    const int rc = nin_csr_patch_rows(m->g->h.n_points, indptr, indices, data, neumann_ws, rows, m->h_node, m->h_cnt, m->h_off, m->h_indices,
                                      m->h_data, m->h_nws, out_indptr, out_indices, out_data);
    L.lap("host patch");
    if (rc) {
        d.all_dirty = true;   // the device is ahead of the host's arrays
        return fail(rc, rc == NIN_ERANGE ? "the patched matrix has more entries than int32 indices hold"
                                         : "the packed rows do not fit the matrix they are patched into (out_* missing for a new structure, or other arrays)");
    }
    return NIN_OK;
}
