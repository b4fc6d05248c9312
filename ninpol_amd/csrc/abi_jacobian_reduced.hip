// abi_jacobian_reduced.hip -- the C ABI, part 7: the GLS Jacobian in a reduced parametrisation of the permeability, perm_e = sum_m
// theta_(e,m) B_(e,m) with M = 1, 3 or 6 parameters per cell, as an object the caller keeps.  One adjoint launch in its
// RED mode linearises straight into R [nnz_esup][M] -- the 80-byte record of abi_jacobian.hip is never stored -- and two streaming
// kernels apply J_theta and its transpose (kernels_gls_jacobian_reduced.hip).  The preconditions are abi_jacobian.hip's
// (abi_internal.hpp: KeptJacobian, jacobian_seed, jacobian_apply_ready, jacobian_apply_host).
#include "abi_internal.hpp"

using namespace nin;

struct nin_gls_rjacobian : KeptJacobian {
    int32_t n_params = 0;            // M
    double *R = nullptr;             // [nnz_esup][M]: this object's own -- the Jacobian
};

namespace {

const char *const kLinearize = "nin_gls_rjacobian_linearize";

// how many cells' worth of basis the caller passes: NULL is the resident perm and goes with one parameter only
int basis_ready(const nin_gls_rjacobian *J, const void *basis) {
    if (!basis && J->n_params != 1) return fail(NIN_EINVAL, "a NULL basis (the resident permeability) needs n_params = 1, not %d", (int)J->n_params);
    return NIN_OK;
}

}  // namespace

int nin_gls_rjacobian_create(nin_grid *g, int32_t n_params, nin_gls_rjacobian **out) {
    if (!g || !out) return fail(NIN_EINVAL, "NULL argument");
    *out = nullptr;
    if (n_params != 1 && n_params != 3 && n_params != 6) return fail(NIN_EINVAL, "n_params must be 1, 3 or 6, not %d", (int)n_params);
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintToDevice)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    nin_gls_rjacobian *J = new (std::nothrow) nin_gls_rjacobian();
    if (!J) return fail(NIN_ENOMEM, "out of host memory");
    J->g = g;
    J->device = d.device;
    J->n_params = n_params;
    const size_t rb = (size_t)std::max<int64_t>(d.nnz_e, 1) * (size_t)n_params * sizeof(double);   // the result: 8 M bytes per entry of esup
    const hipError_t e = hipMalloc((void **)&J->R, rb);
    if (e != hipSuccess) {
        nin_gls_rjacobian_destroy(J);
        return fail(NIN_ENOMEM, "hipMalloc(%zu bytes): %s", rb, hipGetErrorString(e));
    }
    *out = J;
    return NIN_OK;
}

void nin_gls_rjacobian_destroy(nin_gls_rjacobian *J) {
    if (!J) return;
    if (J->device >= 0) (void)hipSetDevice(J->device);
    if (J->R) (void)hipFree(J->R);   // (waits for the device)
    if (J->seed) (void)hipFree(J->seed);
    delete J;
}

int nin_gls_rjacobian_linearize(nin_gls_rjacobian *J, const double *dev_u_cells, const double *dev_neumann_values, const double *dev_basis,
                                int32_t basis_per_cell, void *stream_) {
    if (!J || !dev_u_cells) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = basis_ready(J, dev_basis)) return rc;
    DeviceGrid &d = J->g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DevTmp<double> seed;   // the 8 nnz_esup bytes of the cotangent: with J->R the only allocations of this path
    int rc = jacobian_seed(J->g, dev_u_cells, stream, seed);
    if (rc) return rc;
    J->linearized = false;
    const AdjointReduce red{J->n_params, dev_basis, dev_basis && basis_per_cell ? (int64_t)9 * J->n_params : 0};
    rc = launch_adjoint_bins(d, 1, -1, seed, dev_neumann_values, J->R, stream, &red);   // always every bin: every entry of R is written
    if (rc) return rc;
    J->record_stamp(d);
    return NIN_OK;   // (the seed is freed on the way out: hipFree waits for the kernels that read it)
}

// the rows of R of the grid's dirty nodes alone; the basis is read again, for those rows only
int nin_gls_rjacobian_linearize_dirty(nin_gls_rjacobian *J, const double *dev_u_cells, const double *dev_neumann_values, const double *dev_basis,
                                      int32_t basis_per_cell, void *stream_, int clear, int64_t *n_rows) {
    if (n_rows) *n_rows = 0;
    if (!J || !dev_u_cells) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = basis_ready(J, dev_basis)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const AdjointReduce red{J->n_params, dev_basis, dev_basis && basis_per_cell ? (int64_t)9 * J->n_params : 0};
    DirtyLinearize how{kLinearize, false, nullptr, nullptr, nullptr};
    how.full = [&] { return nin_gls_rjacobian_linearize(J, dev_u_cells, dev_neumann_values, dev_basis, basis_per_cell, stream_); };
    how.bin = [&](int b, const AdjBinRun &run, const double *seed) {
        return launch_gls_adjoint_reduced(J->g->d.v, b, run, 1, seed, dev_neumann_values, red, J->R, stream);
    };
    return jacobian_linearize_dirty(J, dev_u_cells, stream, clear, n_rows, how);
}

int nin_gls_rjacobian_apply(nin_gls_rjacobian *J, int32_t n, const double *dev_dtheta, double *dev_dnode, void *stream_) {
    if (int rc = jacobian_apply_ready(J, n, dev_dtheta, dev_dnode, kLinearize)) return rc;
    DeviceGrid &d = J->g->d;
    HIP_TRY(hipSetDevice(d.device));
    const int rc = launch_jacr_apply(d.v, J->n_params, J->R, n, dev_dtheta, dev_dnode, static_cast<hipStream_t>(stream_));
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_rjacobian_apply_transpose(nin_gls_rjacobian *J, int32_t n, const double *dev_v, double *dev_grad_theta, void *stream_) {
    if (int rc = jacobian_apply_ready(J, n, dev_v, dev_grad_theta, kLinearize)) return rc;
    DeviceGrid &d = J->g->d;
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = ensure_transpose_index(d, stream);   // (every time: nin_grid_release_scratch may have dropped it)
    if (rc) return rc;
    rc = launch_jacr_apply_transpose(d.v, J->n_params, d.tr_cell_ptr, d.tr_cell_pos, d.tr_cell_node, J->R, n, dev_v, dev_grad_theta, stream);
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_rjacobian_buffer(nin_gls_rjacobian *J, const double **dev_R, int32_t *n_params) {
    if (!J || !dev_R || !n_params) return fail(NIN_EINVAL, "NULL argument");
    *dev_R = J->R;
    *n_params = J->n_params;
    return NIN_OK;
}

int nin_gls_rjacobian_stamp(const nin_gls_rjacobian *J, int64_t stamp[3]) { return copy_stamp(J, stamp); }

// ---- host pointers: what Interpolator.permeability_jacobian(basis=...) calls (synchronous) ---------------------------------------------
int nin_gls_rjacobian_linearize_host(nin_gls_rjacobian *J, const double *u_cells, const double *neumann_values, const double *basis,
                                     int32_t basis_per_cell) {
    if (!J || !u_cells) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = basis_ready(J, basis)) return rc;
    nin_grid *g = J->g;
    if (int rc = on_device(g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(g->d.device));
    DevTmp<double> du, db, dB;
    if (int rc = dev_stage(du, u_cells, (size_t)g->h.n_elems)) return rc;
    if (neumann_values)
        if (int rc = dev_stage(db, neumann_values, (size_t)g->h.n_points)) return rc;
    if (basis)
        if (int rc = dev_stage(dB, basis, (basis_per_cell ? (size_t)g->h.n_elems : 1) * 9 * (size_t)J->n_params)) return rc;
    if (int rc = nin_gls_rjacobian_linearize(J, du, db, dB, basis_per_cell, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NIN_OK;
}

int nin_gls_rjacobian_linearize_dirty_host(nin_gls_rjacobian *J, const double *u_cells, const double *neumann_values, const double *basis,
                                           int32_t basis_per_cell, int clear, int64_t *n_rows) {
    if (n_rows) *n_rows = 0;
    if (!J || !u_cells) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = basis_ready(J, basis)) return rc;
    if (int rc = on_device(J->g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(J->g->d.device));
    DevTmp<double> dB;   // (outlives the wait at the end of the call below)
    if (basis)
        if (int rc = dev_stage(dB, basis, (basis_per_cell ? (size_t)J->g->h.n_elems : 1) * 9 * (size_t)J->n_params)) return rc;
    return jacobian_linearize_dirty_host(J, u_cells, neumann_values, [&](const double *du, const double *db) {
        return nin_gls_rjacobian_linearize_dirty(J, du, db, dB, basis_per_cell, nullptr, clear, n_rows);
    });
}

int nin_gls_rjacobian_apply_host(nin_gls_rjacobian *J, int32_t n, const double *dtheta, double *dnode) {
    const size_t P = J ? (size_t)J->g->h.n_points : 0, EM = J ? (size_t)J->g->h.n_elems * (size_t)J->n_params : 0;
    return jacobian_apply_host(J, n, kLinearize, dtheta, EM, dnode, P, nullptr, nullptr, 0, [&](const double *dt, double *dv, double *) {
        return nin_gls_rjacobian_apply(J, n, dt, dv, nullptr);
    });
}

int nin_gls_rjacobian_apply_transpose_host(nin_gls_rjacobian *J, int32_t n, const double *v, double *grad_theta) {
    const size_t P = J ? (size_t)J->g->h.n_points : 0, EM = J ? (size_t)J->g->h.n_elems * (size_t)J->n_params : 0;
    return jacobian_apply_host(J, n, kLinearize, v, P, grad_theta, EM, nullptr, nullptr, 0, [&](const double *dv, double *dt, double *) {
        return nin_gls_rjacobian_apply_transpose(J, n, dv, dt, nullptr);
    });
}

int nin_gls_rjacobian_fetch_host(nin_gls_rjacobian *J, double *R) {
    if (!J || !R) return fail(NIN_EINVAL, "NULL argument");
    if (!J->linearized) return fail(NIN_ESTATE, "the Jacobian has not been linearised (call nin_gls_rjacobian_linearize first)");
    nin_grid *g = J->g;
    if (int rc = on_device(g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(g->d.device));
    return dev_fetch(R, J->R, (size_t)g->d.nnz_e * (size_t)J->n_params);
}
