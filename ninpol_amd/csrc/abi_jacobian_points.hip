// abi_jacobian_points.hip -- the C ABI, part 8: the GLS Jacobian in the node coordinates as an object the caller keeps: one
// launch of the adjoint kernel's coordinate mode linearises, and the kernels of kernels_gls_shape_jacobian.hip apply J and J^T from the
// object's own records through the grid's resident geometry.  The kernels of kernels_gls_shape_assemble.hip assemble the same records
// into a block-CSR matrix whose pattern the object makes once and keeps.
#include "abi_internal.hpp"

using namespace nin;

struct nin_gls_xjacobian : KeptJacobian {
    // the records of the linearisation: cbar [nnz_esup][3], (fcbar, Nbar) [nnz_fsup][6], xbar_own [P][3]
    double *cell = nullptr, *face = nullptr, *own = nullptr;
    // scratch of the applies, made by the first call that needs it and grown to the largest chunk seen: the geometry tangents of J . dX
    // ([tan_n][E][3] and [tan_n][F][6], tan_n <= kXjacApplyChunk), the cells' shares and the faces' point slots of J^T . v ([tr_n][E][3]
    // and [tr_n][F][4][3], tr_n <= kXjacTransposeChunk)
    double *tan_cell = nullptr, *tan_face = nullptr, *tr_share = nullptr, *tr_slot = nullptr;
    int32_t tan_n = 0, tr_n = 0;
    // the pattern of the assembled matrix, made by the first call that needs it and kept until the object goes: block_ptr [P + 1],
    // block_col [n_blocks] ascending within a row; from the connectivity alone, so no update of the grid touches it
    int64_t *block_ptr = nullptr;
    int32_t *block_col = nullptr;
    int64_t n_blocks = 0, points = 0;   // (points: P of the grid at creation)
    int64_t scratch_bytes() const {
        return (int64_t)tan_n * (24 * cells + 48 * faces) + (int64_t)tr_n * (24 * cells + 96 * faces) +
               (block_col ? 8 * (points + 1) + 4 * n_blocks : 0);
    }
    int64_t cells = 1, faces = 1;   // max(E, 1) and max(F, 1) of the grid at creation
};

static const char *const kLinearize = "nin_gls_xjacobian_linearize";

static size_t at_least_one(int64_t n) { return (size_t)std::max<int64_t>(n, 1); }

// a pair of scratch buffers of the object for `want` directions, kept while they are large enough
static int grow_pair(double *&a, size_t a_per, double *&b, size_t b_per, int32_t &have, int32_t want) {
    if (a && b && want <= have) return NIN_OK;
    if (a) (void)hipFree(a);   // (waits for the device)
    if (b) (void)hipFree(b);
    a = b = nullptr;
    have = 0;
    hipError_t e = hipMalloc((void **)&a, (size_t)want * a_per * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&b, (size_t)want * b_per * sizeof(double));
    if (e != hipSuccess) {
        if (a) (void)hipFree(a);
        a = b = nullptr;
        return fail(NIN_ENOMEM, "hipMalloc(%zu + %zu bytes): %s", (size_t)want * a_per * sizeof(double), (size_t)want * b_per * sizeof(double),
                    hipGetErrorString(e));
    }
    have = want;
    return NIN_OK;
}

int nin_gls_xjacobian_create(nin_grid *g, nin_gls_xjacobian **out) {
    if (!g || !out) return fail(NIN_EINVAL, "NULL argument");
    *out = nullptr;
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintToDevice)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    nin_gls_xjacobian *J = new (std::nothrow) nin_gls_xjacobian();
    if (!J) return fail(NIN_ENOMEM, "out of host memory");
    J->g = g;
    J->device = d.device;
    J->cells = (int64_t)at_least_one(d.v.n_elems);
    J->faces = (int64_t)at_least_one(d.v.n_faces);
    J->points = (int64_t)g->h.n_points;
    const size_t cb = at_least_one(d.nnz_e) * 3 * sizeof(double), fb = at_least_one(d.nnz_f) * 6 * sizeof(double),
                 ob = at_least_one(g->h.n_points) * 3 * sizeof(double);
    hipError_t e = hipMalloc((void **)&J->cell, cb);
    if (e == hipSuccess) e = hipMalloc((void **)&J->face, fb);
    if (e == hipSuccess) e = hipMalloc((void **)&J->own, ob);
    if (e != hipSuccess) {
        nin_gls_xjacobian_destroy(J);
        return fail(NIN_ENOMEM, "hipMalloc(%zu + %zu + %zu bytes): %s", cb, fb, ob, hipGetErrorString(e));
    }
    *out = J;
    return NIN_OK;
}

void nin_gls_xjacobian_destroy(nin_gls_xjacobian *J) {
    if (!J) return;
    if (J->device >= 0) (void)hipSetDevice(J->device);
    for (void *p : {(void *)J->cell, (void *)J->face, (void *)J->own, (void *)J->tan_cell, (void *)J->tan_face, (void *)J->tr_share,
                    (void *)J->tr_slot, (void *)J->block_ptr, (void *)J->block_col, (void *)J->seed})
        if (p) (void)hipFree(p);   // (waits for the device)
    delete J;
}

int nin_gls_xjacobian_linearize(nin_gls_xjacobian *J, const double *dev_u_cells, const double *dev_neumann_values, void *stream_) {
    if (!J || !dev_u_cells) return fail(NIN_EINVAL, "NULL argument");
    nin_grid *g = J->g;
    DeviceGrid &d = g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DevTmp<double> seed;
    int rc = jacobian_seed(g, dev_u_cells, stream, seed, true);
    if (!rc) rc = ensure_update_inputs(g);   // inpoel and inpofa for the applies, as the update path brings them
    if (rc) return rc;
    J->linearized = false;
    // always every bin, add_neumann = 1 (the W of apply()); every record of every node is written, zeros where the forward has its zero row
    rc = for_each_adjoint_bin(d, -1, [&](int b, const AdjBinRun &run) {
        return launch_gls_adjoint_points(d.v, b, run, 1, seed, dev_neumann_values, J->cell, J->face, J->own, stream);
    });
    if (rc) return rc;
    J->record_stamp(d);
    return NIN_OK;   // (the seed is freed on the way out: hipFree waits for the kernels that read it)
}

// the records of the grid's dirty nodes alone: after a local move of the points those are the nodes whose cells or faces moved, so the
// other nodes' records are still those of the resident geometry and the applies answer again
int nin_gls_xjacobian_linearize_dirty(nin_gls_xjacobian *J, const double *dev_u_cells, const double *dev_neumann_values, void *stream_, int clear,
                                      int64_t *n_rows) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DirtyLinearize how{kLinearize, true, nullptr, nullptr, nullptr};
    how.full = [&] { return nin_gls_xjacobian_linearize(J, dev_u_cells, dev_neumann_values, stream_); };
    how.bin = [&](int b, const AdjBinRun &run, const double *seed) {
        return launch_gls_adjoint_points(J->g->d.v, b, run, 1, seed, dev_neumann_values, J->cell, J->face, J->own, stream);
    };
    return jacobian_linearize_dirty(J, dev_u_cells, stream, clear, n_rows, how);
}

// jacobian_apply_ready, and the geometry the records are applied through still that of the linearisation
static int xjacobian_apply_ready(const nin_gls_xjacobian *J, int32_t n, const void *in, const void *out) {
    if (int rc = jacobian_apply_ready(J, n, in, out, kLinearize)) return rc;
    const DeviceGrid &d = J->g->d;
    if (d.geom_updates != J->stamp[1])
        return fail(NIN_ESTATE, "the node coordinates were updated after the linearisation (geometry_updates %lld -> %lld) and the Jacobian is "
                                "applied through the resident geometry: call %s again",
                    (long long)J->stamp[1], (long long)d.geom_updates, kLinearize);
    return NIN_OK;
}

int nin_gls_xjacobian_apply(nin_gls_xjacobian *J, int32_t n, const double *dev_dpoints, double *dev_dnode, void *stream_) {
    if (int rc = xjacobian_apply_ready(J, n, dev_dpoints, dev_dnode)) return rc;
    nin_grid *g = J->g;
    DeviceGrid &d = g->d;
    HIP_TRY(hipSetDevice(d.device));
    int rc = ensure_update_inputs(g);   // (every time: nin_grid_release_scratch may have dropped them)
    if (!rc) rc = grow_pair(J->tan_cell, (size_t)J->cells * 3, J->tan_face, (size_t)J->faces * 6, J->tan_n,
                            std::min<int32_t>(n, kXjacApplyChunk));
    if (rc) return rc;
    rc = launch_xjac_apply(d.v, d.up_inpoel, d.up_inpofa, J->cell, J->face, J->own, n, dev_dpoints, J->tan_cell, J->tan_face, dev_dnode,
                           static_cast<hipStream_t>(stream_));
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_xjacobian_apply_transpose(nin_gls_xjacobian *J, int32_t n, const double *dev_v, double *dev_grad_points, void *stream_) {
    if (int rc = xjacobian_apply_ready(J, n, dev_v, dev_grad_points)) return rc;
    nin_grid *g = J->g;
    DeviceGrid &d = g->d;
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = ensure_transpose_index(d, stream);   // (every time: nin_grid_release_scratch may have dropped it)
    if (!rc) rc = ensure_update_inputs(g);
    if (!rc) rc = grow_pair(J->tr_share, (size_t)J->cells * 3, J->tr_slot, (size_t)J->faces * 12, J->tr_n,
                            std::min<int32_t>(n, kXjacTransposeChunk));
    if (rc) return rc;
    rc = launch_xjac_apply_transpose(d.v, d.up_inpofa, d.tr_cell_ptr, d.tr_cell_pos, d.tr_cell_node, J->cell, J->face, J->own, n, dev_v,
                                     J->tr_share, J->tr_slot, dev_grad_points, stream);
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_xjacobian_records(nin_gls_xjacobian *J, const double **dev_cell, const double **dev_face, const double **dev_own,
                              int64_t *scratch_bytes) {
    if (!J || !dev_cell || !dev_face || !dev_own) return fail(NIN_EINVAL, "NULL argument");
    *dev_cell = J->cell;
    *dev_face = J->face;
    *dev_own = J->own;
    if (scratch_bytes)   // (and the cotangent a dirty relinearisation keeps, 8 bytes per entry of esup)
        *scratch_bytes = J->scratch_bytes() + (J->seed ? 8 * std::max<int64_t>(J->g->d.nnz_e, 1) : 0);
    return NIN_OK;
}

int nin_gls_xjacobian_stamp(const nin_gls_xjacobian *J, int64_t stamp[3]) { return copy_stamp(J, stamp); }

// ---- the assembled matrix -------------------------------------------------------------------------------------------------
// The pattern of the object, made if it is not there: count, scan, one synchronisation of `stream` for the number of blocks, fill.
// NIN_GLS_XJAC_PATTERN_FORCE_SLOW (testing switch, read when the pattern is made): every row through the symbolic pass's slow path.
static int ensure_pattern(nin_gls_xjacobian *J, hipStream_t stream) {
    if (J->block_col) return NIN_OK;
    nin_grid *g = J->g;
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintKernels)) return rc;
    if (d.v.dim != 3)
        return fail(NIN_EINVAL, "the derivative with respect to the node coordinates is for 3-D grids only (this grid is %d-D)", (int)d.v.dim);
    HIP_TRY(hipSetDevice(d.device));
    if (int rc = ensure_update_inputs(g)) return rc;
    const int force_slow = getenv("NIN_GLS_XJAC_PATTERN_FORCE_SLOW") != nullptr;
    const int32_t P = d.v.n_points;
    DevTmp<int64_t> count, ptr;
    DevTmp<char> tmp;
    DevTmp<int32_t> col;
    size_t tmp_bytes = 0;
    HIP_TRY(hipMalloc((void **)&count, ((size_t)P + 1) * sizeof(int64_t)));
    HIP_TRY(hipMalloc((void **)&ptr, ((size_t)P + 1) * sizeof(int64_t)));
    if (P == 0) HIP_TRY(hipMemsetAsync(count, 0, sizeof(int64_t), stream));
    int rc = launch_xjac_pattern_count(d.v, d.up_inpoel, d.up_inpofa, force_slow, count, stream);
    if (!rc) rc = xjac_pattern_scan(nullptr, &tmp_bytes, count, ptr, P, stream);
    if (rc) return rc;
    HIP_TRY(hipMalloc((void **)&tmp, std::max<size_t>(tmp_bytes, 1)));
    if ((rc = xjac_pattern_scan(tmp, &tmp_bytes, count, ptr, P, stream))) return rc;
    int64_t n_blocks = 0;
    HIP_TRY(hipMemcpyAsync(&n_blocks, ptr.p + P, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    hipError_t e = hipMalloc((void **)&col, at_least_one(n_blocks) * sizeof(int32_t));
    if (e != hipSuccess) return fail(NIN_ENOMEM, "hipMalloc(%zu bytes): %s", at_least_one(n_blocks) * sizeof(int32_t), hipGetErrorString(e));
    if ((rc = launch_xjac_pattern_fill(d.v, d.up_inpoel, d.up_inpofa, force_slow, ptr, col, stream))) return rc;
    J->block_ptr = ptr.p;
    J->block_col = col.p;
    ptr.p = nullptr;   // (the object's now)
    col.p = nullptr;
    J->n_blocks = n_blocks;
    return NIN_OK;   // (count and tmp are freed on the way out: hipFree waits for the kernels that read them)
}

int nin_gls_xjacobian_pattern(nin_gls_xjacobian *J, int64_t *n_blocks, const int64_t **dev_block_ptr, const int32_t **dev_block_col, void *stream) {
    if (!J || !n_blocks || !dev_block_ptr || !dev_block_col) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = ensure_pattern(J, static_cast<hipStream_t>(stream))) return rc;
    *n_blocks = J->n_blocks;
    *dev_block_ptr = J->block_ptr;
    *dev_block_col = J->block_col;
    return NIN_OK;
}

int nin_gls_xjacobian_pattern_copy(nin_gls_xjacobian *J, int64_t *dev_block_ptr_out, int32_t *dev_block_col_out, void *stream_) {
    if (!J || !dev_block_ptr_out || !dev_block_col_out) return fail(NIN_EINVAL, "NULL argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = ensure_pattern(J, stream)) return rc;
    HIP_TRY(hipSetDevice(J->g->d.device));
    HIP_TRY(hipMemcpyAsync(dev_block_ptr_out, J->block_ptr, ((size_t)J->points + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
    if (J->n_blocks > 0)
        HIP_TRY(hipMemcpyAsync(dev_block_col_out, J->block_col, (size_t)J->n_blocks * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    return NIN_OK;
}

int nin_gls_xjacobian_assemble(nin_gls_xjacobian *J, double *dev_values, void *stream_) {
    if (int rc = xjacobian_apply_ready(J, 1, dev_values, dev_values)) return rc;
    nin_grid *g = J->g;
    DeviceGrid &d = g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(d.device));
    int rc = ensure_update_inputs(g);   // (every time: nin_grid_release_scratch may have dropped them)
    if (!rc) rc = ensure_pattern(J, stream);
    if (rc) return rc;
    rc = launch_xjac_assemble(d.v, d.up_inpoel, d.up_inpofa, J->cell, J->face, J->own, J->block_ptr, J->block_col, dev_values, stream);
    if (rc) return rc;
    return NIN_OK;
}

// ---- host pointers: what Interpolator.points_jacobian calls (synchronous) -------------------------------------------------------------
int nin_gls_xjacobian_linearize_host(nin_gls_xjacobian *J, const double *u_cells, const double *neumann_values) {
    if (!J || !u_cells) return fail(NIN_EINVAL, "NULL argument");
    nin_grid *g = J->g;
    if (int rc = on_device(g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(g->d.device));
    DevTmp<double> du, db;
    if (int rc = dev_stage(du, u_cells, (size_t)g->h.n_elems)) return rc;
    if (neumann_values)
        if (int rc = dev_stage(db, neumann_values, (size_t)g->h.n_points)) return rc;
    if (int rc = nin_gls_xjacobian_linearize(J, du, db, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NIN_OK;
}

int nin_gls_xjacobian_linearize_dirty_host(nin_gls_xjacobian *J, const double *u_cells, const double *neumann_values, int clear, int64_t *n_rows) {
    if (n_rows) *n_rows = 0;
    return jacobian_linearize_dirty_host(J, u_cells, neumann_values, [&](const double *du, const double *db) {
        return nin_gls_xjacobian_linearize_dirty(J, du, db, nullptr, clear, n_rows);
    });
}

int nin_gls_xjacobian_apply_host(nin_gls_xjacobian *J, int32_t n, const double *dpoints, double *dnode) {
    const size_t P = J ? (size_t)J->g->h.n_points : 0;
    return jacobian_apply_host(J, n, kLinearize, dpoints, 3 * P, dnode, P, nullptr, nullptr, 0, [&](const double *dx, double *dv, double *) {
        return nin_gls_xjacobian_apply(J, n, dx, dv, nullptr);
    });
}

int nin_gls_xjacobian_apply_transpose_host(nin_gls_xjacobian *J, int32_t n, const double *v, double *grad_points) {
    const size_t P = J ? (size_t)J->g->h.n_points : 0;
    return jacobian_apply_host(J, n, kLinearize, v, P, grad_points, 3 * P, nullptr, nullptr, 0, [&](const double *dv, double *dx, double *) {
        return nin_gls_xjacobian_apply_transpose(J, n, dv, dx, nullptr);
    });
}

int nin_gls_xjacobian_fetch_host(nin_gls_xjacobian *J, double *cell, double *face, double *own) {
    if (!J || !cell || !face || !own) return fail(NIN_EINVAL, "NULL argument");
    if (!J->linearized) return fail(NIN_ESTATE, "the Jacobian has not been linearised (call nin_gls_xjacobian_linearize first)");
    nin_grid *g = J->g;
    if (int rc = on_device(g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(g->d.device));
    if (int rc = dev_fetch(cell, J->cell, (size_t)g->d.nnz_e * 3)) return rc;
    if (int rc = dev_fetch(face, J->face, (size_t)g->d.nnz_f * 6)) return rc;
    return dev_fetch(own, J->own, (size_t)g->h.n_points * 3);
}

int nin_gls_xjacobian_pattern_host(nin_gls_xjacobian *J, int64_t *block_ptr, int32_t *block_col, int64_t *n_blocks) {
    if (!J || !block_ptr || !n_blocks) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = ensure_pattern(J, nullptr)) return rc;
    HIP_TRY(hipSetDevice(J->g->d.device));
    HIP_TRY(hipMemcpy(block_ptr, J->block_ptr, ((size_t)J->points + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (block_col && J->n_blocks > 0)   // (NULL: the caller asks for the size)
        HIP_TRY(hipMemcpy(block_col, J->block_col, (size_t)J->n_blocks * sizeof(int32_t), hipMemcpyDeviceToHost));
    *n_blocks = J->n_blocks;
    return NIN_OK;
}

int nin_gls_xjacobian_assemble_host(nin_gls_xjacobian *J, double *values) {
    if (int rc = xjacobian_apply_ready(J, 1, values, values)) return rc;
    HIP_TRY(hipSetDevice(J->g->d.device));
    if (int rc = ensure_pattern(J, nullptr)) return rc;
    DevTmp<double> dv;
    if (int rc = dev_stage(dv, nullptr, 3 * (size_t)J->n_blocks)) return rc;
    if (int rc = nin_gls_xjacobian_assemble(J, dv, nullptr)) return rc;
    return dev_fetch(values, dv, 3 * (size_t)J->n_blocks);
}
