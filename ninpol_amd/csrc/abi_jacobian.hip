// abi_jacobian.hip -- the C ABI, part 6: the GLS Jacobian in the permeability as an object the caller keeps: one adjoint
// launch linearises, two streaming kernels apply J and J^T from the object's own buffers (kernels_gls_jacobian.hip).
#include "abi_internal.hpp"

using namespace nin;

struct nin_gls_jacobian : KeptJacobian {
    double *contrib = nullptr;       // [nnz_esup][10]: the adjoint's contribution buffer, this object's own -- the Jacobian
    double *fold = nullptr;          // [E]: d diff_mag / d K_dd of the permeability that was resident at the linearisation
};

static const char *const kLinearize = "nin_gls_jacobian_linearize";

// ---- what a linearisation of a kept Jacobian begins with (abi_jacobian_reduced.hip and abi_jacobian_points.hip call it too) -------------------------------
int nin::jacobian_seed(nin_grid *g, const double *dev_u_cells, hipStream_t stream, DevTmp<double> &seed, bool coordinates) {
    DeviceGrid &d = g->d;
    if (int rc = derivative_ready(g, stream, coordinates)) return rc;
    // the cotangent of F = W u + neumann_ws b: grad_csr[pos] = u[esup[pos]], grad_neumann_ws = b
    if (int rc = dev_stage(seed, nullptr, (size_t)d.nnz_e)) return rc;
    if (int rc = launch_jac_seed(d.v, d.nnz_e, dev_u_cells, seed, stream)) return rc;
    return NIN_OK;
}

int nin_gls_jacobian_create(nin_grid *g, nin_gls_jacobian **out) {
    if (!g || !out) return fail(NIN_EINVAL, "NULL argument");
    *out = nullptr;
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintToDevice)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    nin_gls_jacobian *J = new (std::nothrow) nin_gls_jacobian();
    if (!J) return fail(NIN_ENOMEM, "out of host memory");
    J->g = g;
    J->device = d.device;
    const size_t cb = (size_t)std::max<int64_t>(d.nnz_e, 1) * 10 * sizeof(double), fb = (size_t)std::max<int64_t>(g->h.n_elems, 1) * sizeof(double);
    hipError_t e = hipMalloc((void **)&J->contrib, cb);
    if (e == hipSuccess) e = hipMalloc((void **)&J->fold, fb);
    if (e != hipSuccess) {
        nin_gls_jacobian_destroy(J);
        return fail(NIN_ENOMEM, "hipMalloc(%zu + %zu bytes): %s", cb, fb, hipGetErrorString(e));
    }
    *out = J;
    return NIN_OK;
}

void nin_gls_jacobian_destroy(nin_gls_jacobian *J) {
    if (!J) return;
    if (J->device >= 0) (void)hipSetDevice(J->device);
    if (J->contrib) (void)hipFree(J->contrib);   // (waits for the device)
    if (J->fold) (void)hipFree(J->fold);
    if (J->seed) (void)hipFree(J->seed);
    delete J;
}

int nin_gls_jacobian_linearize(nin_gls_jacobian *J, const double *dev_u_cells, const double *dev_neumann_values, void *stream_) {
    if (!J || !dev_u_cells) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = J->g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DevTmp<double> seed;
    int rc = jacobian_seed(J->g, dev_u_cells, stream, seed);
    if (rc) return rc;
    J->linearized = false;
    rc = launch_adjoint_bins(d, 1, -1, seed, dev_neumann_values, J->contrib, stream);   // always every bin
    if (!rc) rc = launch_jac_fold(d.v, J->fold, stream);
    if (rc) return rc;
    J->record_stamp(d);
    return NIN_OK;   // (the seed is freed on the way out: hipFree waits for the kernels that read it)
}

// the records of the grid's dirty nodes alone, and the fold whole (8 E bytes: it reads the resident perm, which a scatter rewrote)
int nin_gls_jacobian_linearize_dirty(nin_gls_jacobian *J, const double *dev_u_cells, const double *dev_neumann_values, void *stream_, int clear,
                                     int64_t *n_rows) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DirtyLinearize how{kLinearize, false, nullptr, nullptr, nullptr};
    how.full = [&] { return nin_gls_jacobian_linearize(J, dev_u_cells, dev_neumann_values, stream_); };
    how.bin = [&](int b, const AdjBinRun &run, const double *seed) {
        return launch_gls_adjoint(J->g->d.v, b, run, 1, seed, dev_neumann_values, J->contrib, stream);
    };
    how.finish = [&] { return launch_jac_fold(J->g->d.v, J->fold, stream); };
    return jacobian_linearize_dirty(J, dev_u_cells, stream, clear, n_rows, how);
}

int nin_gls_jacobian_apply(nin_gls_jacobian *J, int32_t n, const double *dev_dperm, const double *dev_ddiff_mag, double *dev_dnode,
                           void *stream_) {
    if (int rc = jacobian_apply_ready(J, n, dev_dperm, dev_dnode, kLinearize)) return rc;
    DeviceGrid &d = J->g->d;
    HIP_TRY(hipSetDevice(d.device));
    const int rc = launch_jac_apply(d.v, J->contrib, J->fold, n, dev_dperm, dev_ddiff_mag, dev_dnode, static_cast<hipStream_t>(stream_));
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_jacobian_apply_transpose(nin_gls_jacobian *J, int32_t n, const double *dev_v, double *dev_grad_perm, double *dev_grad_diff_mag,
                                     void *stream_) {
    if (int rc = jacobian_apply_ready(J, n, dev_v, dev_grad_perm, kLinearize)) return rc;
    DeviceGrid &d = J->g->d;
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = ensure_transpose_index(d, stream);   // (every time: nin_grid_release_scratch may have dropped it)
    if (rc) return rc;
    rc = launch_jac_apply_transpose(d.v, d.tr_cell_ptr, d.tr_cell_pos, d.tr_cell_node, J->contrib, J->fold, n, dev_v, dev_grad_perm,
                                    dev_grad_diff_mag, stream);
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_jacobian_contrib(nin_gls_jacobian *J, const double **dev_contrib, const double **dev_fold) {
    if (!J || !dev_contrib || !dev_fold) return fail(NIN_EINVAL, "NULL argument");
    *dev_contrib = J->contrib;
    *dev_fold = J->fold;
    return NIN_OK;
}

int nin_gls_jacobian_stamp(const nin_gls_jacobian *J, int64_t stamp[3]) { return copy_stamp(J, stamp); }

// ---- host pointers: what Interpolator.permeability_jacobian calls (synchronous) ------------------------------------------------------
int nin_gls_jacobian_linearize_host(nin_gls_jacobian *J, const double *u_cells, const double *neumann_values) {
    if (!J || !u_cells) return fail(NIN_EINVAL, "NULL argument");
    nin_grid *g = J->g;
    if (int rc = on_device(g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(g->d.device));
    DevTmp<double> du, db;
    if (int rc = dev_stage(du, u_cells, (size_t)g->h.n_elems)) return rc;
    if (neumann_values)
        if (int rc = dev_stage(db, neumann_values, (size_t)g->h.n_points)) return rc;
    if (int rc = nin_gls_jacobian_linearize(J, du, db, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NIN_OK;
}

int nin_gls_jacobian_linearize_dirty_host(nin_gls_jacobian *J, const double *u_cells, const double *neumann_values, int clear, int64_t *n_rows) {
    if (n_rows) *n_rows = 0;
    return jacobian_linearize_dirty_host(J, u_cells, neumann_values, [&](const double *du, const double *db) {
        return nin_gls_jacobian_linearize_dirty(J, du, db, nullptr, clear, n_rows);
    });
}

int nin_gls_jacobian_apply_host(nin_gls_jacobian *J, int32_t n, const double *dperm, const double *ddiff_mag, double *dnode) {
    const size_t P = J ? (size_t)J->g->h.n_points : 0, E = J ? (size_t)J->g->h.n_elems : 0;
    return jacobian_apply_host(J, n, kLinearize, dperm, 9 * E, dnode, P, ddiff_mag, nullptr, E, [&](const double *dk, double *dv, double *dm) {
        return nin_gls_jacobian_apply(J, n, dk, dm, dv, nullptr);
    });
}

int nin_gls_jacobian_apply_transpose_host(nin_gls_jacobian *J, int32_t n, const double *v, double *grad_perm, double *grad_diff_mag) {
    const size_t P = J ? (size_t)J->g->h.n_points : 0, E = J ? (size_t)J->g->h.n_elems : 0;
    return jacobian_apply_host(J, n, kLinearize, v, P, grad_perm, 9 * E, nullptr, grad_diff_mag, E, [&](const double *dv, double *dk, double *dm) {
        return nin_gls_jacobian_apply_transpose(J, n, dv, dk, dm, nullptr);
    });
}

int nin_gls_jacobian_fetch_host(nin_gls_jacobian *J, double *contrib, double *fold) {
    if (!J || !contrib || !fold) return fail(NIN_EINVAL, "NULL argument");
    if (!J->linearized) return fail(NIN_ESTATE, "the Jacobian has not been linearised (call nin_gls_jacobian_linearize first)");
    nin_grid *g = J->g;
    if (int rc = on_device(g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(g->d.device));
    if (int rc = dev_fetch(contrib, J->contrib, (size_t)g->d.nnz_e * 10)) return rc;
    return dev_fetch(fold, J->fold, (size_t)g->h.n_elems);
}
