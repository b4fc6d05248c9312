// abi_jacobian_dirty.hip -- the C ABI, part 9: a kept GLS Jacobian follows local updates.  The three *_linearize_dirty
// entry points (abi_jacobian.hip, abi_jacobian_reduced.hip, abi_jacobian_points.hip: each knows its own buffers and its mode of the
// adjoint kernel) share the body below: the grid's dirty set binned by adjoint bin (jacobian_dirty.hip), one read-back, the cotangent
// seeded for the listed rows, the adjoint kernel on the lists through the launch functions a full linearisation uses.
#include "abi_internal.hpp"

using namespace nin;

namespace {

// NIN_TIMING=1: HIP events on the call's stream around its three phases -- compaction + read-back, seed, adjoint launches (and what
// follows them: the fold) -- and one line on stderr; the call then waits for its kernels (tools/time_jacobian.py --dirty reads the lines)
struct JacDirtyLaps {
    bool on = getenv("NIN_TIMING") != nullptr;
    hipStream_t stream;
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    explicit JacDirtyLaps(hipStream_t s) : stream(s) {}
    ~JacDirtyLaps() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    void mark(int i) { if (on && !e[i] && hipEventCreate(&e[i]) == hipSuccess) (void)hipEventRecord(e[i], stream); }
    void report(int64_t n) {
        if (!on || !e[0] || !e[1] || !e[2] || !e[3] || hipEventSynchronize(e[3]) != hipSuccess) return;
        float ms[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&ms[i], e[i], e[i + 1]);
        fprintf(stderr, "[nin_jac_dirty] rows %lld compact+readback %.4f seed %.4f adjoint %.4f ms\n", (long long)n, ms[0], ms[1], ms[2]);
    }
};

// the per-node bin byte and the compaction's buffers, sized by the mesh alone: made by the first dirty relinearisation (and again after
// nin_grid_release_scratch, which gives them back with the bins they were made from)
int ensure_adjoint_dirty_state(DeviceGrid &d, int32_t P, hipStream_t stream) {
    int rc = NIN_OK;
    if (!d.adj_node_bin) {
        if ((rc = dev_alloc(d, &d.adj_node_bin, (size_t)P))) return rc;
        hipError_t e = hipMemsetAsync(d.adj_node_bin, 0xff, (size_t)std::max(P, 1), stream);
        for (int b = 0; b < kAdjBins && e == hipSuccess; ++b)
            if (launch_adj_bin_byte(d.adj_bin[b].nodes, d.adj_bin[b].count, P, b, d.adj_node_bin, stream)) e = hipErrorLaunchFailure;
        if (e != hipSuccess) {
            dev_release(d, d.adj_node_bin);
            return fail(NIN_EHIP, "the adjoint bin of every node: %s", hipGetErrorString(e));
        }
    }
    size_t tmp_bytes = 0;
    if (adj_dirty_tmp_bytes(P, &tmp_bytes)) return fail(NIN_EHIP, "sizing the scan of the dirty set failed");
    if (!d.adj_dirty_hist && (rc = dev_alloc(d, &d.adj_dirty_hist, 2 * adj_dirty_hist_ints(P)))) return rc;   // the histogram and its scan
    if (!d.adj_dirty_lists && (rc = dev_alloc(d, &d.adj_dirty_lists, (size_t)P))) return rc;
    if (!d.adj_dirty_hdr && (rc = dev_alloc(d, &d.adj_dirty_hdr, (size_t)kAdjDirtyHdrInts))) return rc;
    return grow(d, reinterpret_cast<char **>(&d.adj_dirty_tmp), &d.adj_dirty_tmp_bytes, std::max<size_t>(tmp_bytes, 16));
}

}  // namespace

int nin::jacobian_linearize_dirty(KeptJacobian *J, const double *dev_u_cells, hipStream_t stream, int clear, int64_t *n_rows,
                                  const DirtyLinearize &how) {
    if (n_rows) *n_rows = 0;
    if (!J || !dev_u_cells) return fail(NIN_EINVAL, "NULL argument");
    nin_grid *g = J->g;
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintKernels)) return rc;
    if (!J->linearized) return fail(NIN_ESTATE, "the Jacobian has not been linearised (call %s first)", how.linearize_name);
    if (int rc = derivative_ready(g, stream, how.coordinates)) return rc;   // (the bins: made again if the scratch was released)
    const int32_t P = (int32_t)g->h.n_points;
    int32_t hdr[kAdjDirtyHdrInts] = {0};
    int32_t *const rejected = hdr + kAdjBins + 1;
    JacDirtyLaps laps(stream);   // NIN_TIMING=1: the call's three phases on stderr
    laps.mark(0);
    if (d.dirty) {   // (no scatter and no mark yet: no marks, no refused ids)
        if (!d.all_dirty) {
            if (int rc = ensure_adjoint_dirty_state(d, P, stream)) return rc;
            const size_t ints = adj_dirty_hist_ints(P);
            if (int rc = launch_adj_dirty_compact(P, clear, d.dirty, d.adj_node_bin, d.dirty_hdr + kDirtyHdrRejected, d.adj_dirty_hist, d.adj_dirty_hist + ints,
                                                  d.adj_dirty_tmp, d.adj_dirty_tmp_bytes, d.adj_dirty_lists, d.adj_dirty_hdr, stream))
                return rc;
            // the one synchronisation of the call: where every bin's list begins and the refused-id counter, 32 bytes
            HIP_TRY(hipMemcpyAsync(hdr, d.adj_dirty_hdr, sizeof hdr, hipMemcpyDeviceToHost, stream));
        } else {
            HIP_TRY(hipMemcpyAsync(rejected, d.dirty_hdr + kDirtyHdrRejected, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        if (*rejected != 0) return dirty_ids_refused(g, *rejected, stream);   // the marks are as they were (the fill pass clears nothing while the counter is set)
        d.scattered_cells = d.scattered_nodes = d.scattered_flags = d.scattered_marks = false;
    }
    laps.mark(1);
    if (!J->seed) {   // the first call that gets here; the object keeps it
        const size_t sb = (size_t)std::max<int64_t>(d.nnz_e, 1) * sizeof(double);
        const hipError_t e = hipMalloc((void **)&J->seed, sb);
        if (e != hipSuccess) {
            J->seed = nullptr;
            d.all_dirty = true;   // the compaction may have cleared marks whose rows were not recomputed: everything counts as dirty again
            return fail(NIN_ENOMEM, "hipMalloc(%zu bytes): %s", sb, hipGetErrorString(e));
        }
    }
    if (d.all_dirty) {   // the ordinary full relinearisation
        if (int rc = how.full()) return rc;
        if (clear) {
            if (d.dirty) HIP_TRY(hipMemsetAsync(d.dirty, 0, (size_t)P, stream));
            d.all_dirty = false;
        }
        if (n_rows) *n_rows = P;
        return NIN_OK;
    }
    if (!d.dirty) {   // nothing was ever marked: the empty set
        J->record_stamp(d);
        return NIN_OK;
    }
    const int32_t total = hdr[kAdjBins];
    if (total < 0 || total > P) return fail(NIN_EHIP, "the dirty set's lists hold %d nodes of %d", (int)total, (int)P);
    for (int b = 0; b < kAdjBins; ++b)
        if (hdr[b] < 0 || hdr[b + 1] < hdr[b] || hdr[b + 1] - hdr[b] > d.adj_bin[b].count)
            return fail(NIN_EHIP, "the dirty set's lists are out of order");
    if (n_rows) *n_rows = total;
    if (total == 0) {   // no adjoint kernel; the object is the Jacobian at the grid's state as it is now
        J->record_stamp(d);
        return NIN_OK;
    }
    J->linearized = false;   // (until every launch below is enqueued: a failure half way leaves rows of two points)
    int rc = launch_jac_seed_rows(d.v, d.adj_dirty_lists, total, dev_u_cells, J->seed, stream);
    laps.mark(2);
    for (int b = 0; b < kAdjBins && !rc; ++b) {
        if (hdr[b + 1] == hdr[b]) continue;
        AdjBinRun run = adjoint_bin_run(d, b);   // bytes, scratch stride and slots stay the bin's own: the instantiation and the LDS per node of the full launch
        run.nodes = d.adj_dirty_lists + hdr[b];
        run.count = hdr[b + 1] - hdr[b];
        rc = how.bin(b, run, J->seed);
    }
    if (!rc && how.finish) rc = how.finish();
    if (rc) return rc;
    laps.mark(3);
    J->record_stamp(d);
    laps.report(total);
    return NIN_OK;
}

int nin::jacobian_linearize_dirty_host(KeptJacobian *J, const double *u_cells, const double *neumann_values,
                                       const std::function<int(const double *, const double *)> &launch) {
    if (!J || !u_cells) return fail(NIN_EINVAL, "NULL argument");
    nin_grid *g = J->g;
    if (int rc = on_device(g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(g->d.device));
    DevTmp<double> du, db;
    if (int rc = dev_stage(du, u_cells, (size_t)g->h.n_elems)) return rc;
    if (neumann_values)
        if (int rc = dev_stage(db, neumann_values, (size_t)g->h.n_points)) return rc;
    if (int rc = launch(du, db)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NIN_OK;
}
