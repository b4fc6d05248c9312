// abi_gradop.hip -- the corner-gradient operator of the GLS reconstruction as an object the caller keeps: G maps a cell
// field u [E] to the corner gradients g [nnz_esup][3] of nin_gls_corner_gradients_*, depends on the points, the permeability and the
// Neumann flags alone, and is block diagonal over the nodes.  One launch of the adjoint kernel's gradient mode with the unit columns as
// its fields (kernels_gls_adjoint.hip, GOP) factorises every node once and leaves G in a buffer the object owns; G . u and G^T . v then
// stream that buffer (kernels_gls_gradop.hip).  Host code only.  tools/sanitize_gradop.sh runs the argument checks and the sizing below
// under ASan + UBSan.
#include "abi_internal.hpp"

using namespace nin;

static const char *const kFactorize = "nin_gls_gradop_factorize";
static const char *const kWhat = "the gradient operator is";

// gop_ptr [P + 1] and pos_node [nnz_esup] of g, made on the device from its resident esup_ptr (a grid built on the device may have no host
// copy), and n_values = gop_ptr[P]; synchronises `stream` for that one number.  The buffers are the caller's, of those sizes at least
static int gradop_layout(DeviceGrid &d, int64_t *gop_ptr, int32_t *pos_node, int64_t *n_values, hipStream_t stream) {
    const int32_t P = d.v.n_points;
    DevTmp<int64_t> count;
    DevTmp<char> tmp;
    size_t tmp_bytes = 0;
    HIP_TRY(hipMalloc((void **)&count, ((size_t)P + 1) * sizeof(int64_t)));
    if (int rc = launch_gradop_layout(d.v, d.nnz_e, count, nullptr, &tmp_bytes, gop_ptr, pos_node, stream)) return rc;
    HIP_TRY(hipMalloc((void **)&tmp, std::max<size_t>(tmp_bytes, 1)));
    if (int rc = launch_gradop_layout(d.v, d.nnz_e, count, tmp, &tmp_bytes, gop_ptr, pos_node, stream)) return rc;
    HIP_TRY(hipMemcpyAsync(n_values, gop_ptr + P, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return NIN_OK;   // (count and tmp are freed on the way out)
}

// what nin_gls_gradop_create and nin_gls_gradop_bytes begin with: the arguments and the dimension before the residency
static int gradop_grid_ready(nin_grid *g, const void *out) {
    if (int rc = gradient_args(g, out, out, 1, "n", kWhat)) return rc;
    if (int rc = on_device(g, kHintToDevice)) return rc;
    HIP_TRY(hipSetDevice(g->d.device));
    return NIN_OK;
}

int nin_gls_gradop_bytes(nin_grid *g, int64_t *bytes) {
    if (int rc = gradop_grid_ready(g, bytes)) return rc;
    DeviceGrid &d = g->d;
    DevTmp<int64_t> ptr;
    DevTmp<int32_t> node;
    HIP_TRY(hipMalloc((void **)&ptr, ((size_t)d.v.n_points + 1) * sizeof(int64_t)));
    HIP_TRY(hipMalloc((void **)&node, (size_t)std::max<int64_t>(d.nnz_e, 1) * sizeof(int32_t)));
    int64_t n_values = 0;
    if (int rc = gradop_layout(d, ptr, node, &n_values, nullptr)) return rc;
    *bytes = gradop_bytes(n_values, d.v.n_points, d.nnz_e).gop;
    return NIN_OK;
}

int nin_gls_gradop_create(nin_grid *g, nin_gls_gradop **out) {
    if (out) *out = nullptr;
    if (int rc = gradop_grid_ready(g, out)) return rc;
    DeviceGrid &d = g->d;
    nin_gls_gradop *op = new (std::nothrow) nin_gls_gradop();
    if (!op) return fail(NIN_ENOMEM, "out of host memory");
    op->g = g;
    op->device = d.device;
    op->nnz = d.nnz_e;
    op->points = d.v.n_points;
    op->elems = d.v.n_elems;
    const GradopBytes fixed = gradop_bytes(0, op->points, op->nnz);
    hipError_t e = hipMalloc((void **)&op->gop_ptr, (size_t)fixed.gop_ptr);
    if (e == hipSuccess) e = hipMalloc((void **)&op->pos_node, (size_t)std::max<int64_t>(fixed.pos_node, 4));
    int rc = e == hipSuccess ? gradop_layout(d, op->gop_ptr, op->pos_node, &op->n_values, nullptr)
                             : fail(NIN_ENOMEM, "hipMalloc(%lld + %lld bytes): %s", (long long)fixed.gop_ptr, (long long)fixed.pos_node, hipGetErrorString(e));
    if (!rc) {
        const size_t bytes = (size_t)std::max<int64_t>(gradop_bytes(op->n_values, op->points, op->nnz).gop, 8);
        e = hipMalloc((void **)&op->gop, bytes);
        if (e != hipSuccess) rc = fail(NIN_ENOMEM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    }
    if (rc) {
        nin_gls_gradop_destroy(op);
        return rc;
    }
    *out = op;
    return NIN_OK;
}

void nin_gls_gradop_destroy(nin_gls_gradop *op) {
    if (!op) return;
    if (op->device >= 0) (void)hipSetDevice(op->device);
    for (void *p : {(void *)op->gop_ptr, (void *)op->pos_node, (void *)op->gop, (void *)op->dots})
        if (p) (void)hipFree(p);   // (waits for the device)
    delete op;
}

int nin_gls_gradop_factorize(nin_gls_gradop *op, void *stream_) {
    if (!op) return fail(NIN_EINVAL, "NULL argument");
    nin_grid *g = op->g;
    DeviceGrid &d = g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = derivative_ready(g, stream)) return rc;
    op->linearized = false;
    // always every bin (NIN_GLS_ADJ_ONLY is not read): every entry of every node's block is written, zeros where the forward has its zero row
    const int rc = for_each_adjoint_bin(d, -1, [&](int b, const AdjBinRun &run) {
        return launch_gls_gradop_factorize(d.v, b, run, op->gop_ptr, op->gop, stream);
    });
    if (rc) return rc;
    op->record_stamp(d);
    return NIN_OK;
}

// a product can go: the arguments, the count and the dimension first, then the grid on its device, a factorisation, and none of the
// three inputs of the operator updated since
static int gradop_product_ready(const nin_gls_gradop *op, int32_t n, const void *in, const void *out) {
    if (int rc = gradient_args(op ? op->g : nullptr, in, out, n, "n", kWhat)) return rc;
    if (int rc = on_device(op->g, kHintKernels)) return rc;
    if (!op->linearized) return fail(NIN_ESTATE, "the gradient operator has not been factorised (call %s first)", kFactorize);
    const DeviceGrid &d = op->g->d;
    if (d.field_updates != op->stamp[0] || d.geom_updates != op->stamp[1] || d.flag_updates != op->stamp[2])
        return fail(NIN_ESTATE, "the permeability, the node coordinates or the Neumann flags were updated after the factorisation ((field_updates, "
                                "geometry_updates, flag_updates) (%lld, %lld, %lld) -> (%lld, %lld, %lld)): call %s again",
                    (long long)op->stamp[0], (long long)op->stamp[1], (long long)op->stamp[2], (long long)d.field_updates,
                    (long long)d.geom_updates, (long long)d.flag_updates, kFactorize);
    return NIN_OK;
}

int nin_gls_gradop_apply(nin_gls_gradop *op, int32_t n, const double *dev_u, double *dev_grad, double *dev_flux, double *dev_node_gradient,
                         void *stream_) {
    if (int rc = gradop_product_ready(op, n, dev_u, dev_grad)) return rc;
    DeviceGrid &d = op->g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(d.device));
    int rc = launch_gradop_apply(d.v, op->nnz, op->gop_ptr, op->pos_node, op->gop, n, dev_u, dev_grad, stream);
    if (!rc && dev_flux) rc = launch_corner_flux(d.v, op->nnz, n, dev_grad, dev_flux, stream);
    if (!rc && dev_node_gradient) rc = launch_node_gradient(d.v, op->nnz, n, dev_grad, dev_node_gradient, stream);
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_gradop_apply_transpose(nin_gls_gradop *op, int32_t n, const double *dev_gbar, double *dev_ubar, void *stream_) {
    if (int rc = gradop_product_ready(op, n, dev_gbar, dev_ubar)) return rc;
    DeviceGrid &d = op->g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(d.device));
    if (int rc = ensure_transpose_index(d, stream)) return rc;   // (every time: nin_grid_release_scratch may have dropped it)
    const int32_t want = std::min<int32_t>(n, kGradopChunk);
    if (!op->dots || op->dots_n < want) {
        if (op->dots) (void)hipFree(op->dots);   // (waits for the device)
        op->dots = nullptr;
        op->dots_n = 0;
        const size_t bytes = std::max<size_t>(gradop_dots_count(op->nnz, want), 1) * sizeof(double);
        hipError_t e = hipMalloc((void **)&op->dots, bytes);
        if (e != hipSuccess) return fail(NIN_ENOMEM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
        op->dots_n = want;
    }
    if (int rc = launch_gradop_apply_transpose(d.v, op->nnz, d.tr_cell_ptr, d.tr_cell_pos, op->gop_ptr, op->pos_node, op->gop, n, dev_gbar, op->dots,
                                               dev_ubar, stream))
        return rc;
    return NIN_OK;
}

int nin_gls_gradop_records(nin_gls_gradop *op, const int64_t **dev_gop_ptr, const double **dev_gop, int64_t *n_values, int64_t *scratch_bytes) {
    if (!op || !dev_gop_ptr || !dev_gop || !n_values) return fail(NIN_EINVAL, "NULL argument");
    *dev_gop_ptr = op->gop_ptr;
    *dev_gop = op->gop;
    *n_values = op->n_values;
    if (scratch_bytes) {   // what the object holds beside gop: its layout and the transposed product's dots
        const GradopBytes b = gradop_bytes(op->n_values, op->points, op->nnz);
        *scratch_bytes = b.gop_ptr + b.pos_node + 8 * (int64_t)gradop_dots_count(op->nnz, op->dots_n);
    }
    return NIN_OK;
}

int nin_gls_gradop_stamp(const nin_gls_gradop *op, int64_t stamp[3]) { return copy_stamp(op, stamp); }

// ---- host pointers: what Interpolator.gradient_operator calls (synchronous) -------------------------------------------------------------
int nin_gls_gradop_factorize_host(nin_gls_gradop *op) {
    if (int rc = nin_gls_gradop_factorize(op, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NIN_OK;
}

int nin_gls_gradop_apply_host(nin_gls_gradop *op, int32_t n, const double *u, double *grad, double *flux, double *node_gradient) {
    if (int rc = gradop_product_ready(op, n, u, grad)) return rc;
    HIP_TRY(hipSetDevice(op->g->d.device));
    const CornerGradientCounts c = corner_gradient_counts(op->elems, op->points, op->nnz, n);
    DevTmp<double> du, dg, df, dn;
    int rc = dev_stage(du, u, c.u);
    if (!rc) rc = dev_stage(dg, nullptr, c.grad);
    if (!rc && flux) rc = dev_stage(df, nullptr, c.grad);
    if (!rc && node_gradient) rc = dev_stage(dn, nullptr, c.node_gradient);
    if (!rc) rc = nin_gls_gradop_apply(op, n, du, dg, df, dn, nullptr);
    if (!rc) rc = dev_fetch(grad, dg, c.grad);
    if (!rc && flux) rc = dev_fetch(flux, df, c.grad);
    if (!rc && node_gradient) rc = dev_fetch(node_gradient, dn, c.node_gradient);
    return rc;
}

int nin_gls_gradop_apply_transpose_host(nin_gls_gradop *op, int32_t n, const double *gbar, double *ubar) {
    if (int rc = gradop_product_ready(op, n, gbar, ubar)) return rc;
    return jacobian_apply_host(op, n, kFactorize, gbar, 3 * (size_t)op->nnz, ubar, (size_t)op->elems, nullptr, nullptr, 0,
                               [&](const double *dg, double *du, double *) { return nin_gls_gradop_apply_transpose(op, n, dg, du, nullptr); });
}

int nin_gls_gradop_fetch_host(nin_gls_gradop *op, int64_t *gop_ptr, double *gop) {
    if (!op || !gop_ptr) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = on_device(op->g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(op->g->d.device));
    HIP_TRY(hipDeviceSynchronize());   // (a factorisation may be in flight on a stream the copies below do not wait for)
    HIP_TRY(hipMemcpy(gop_ptr, op->gop_ptr, ((size_t)op->points + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (!gop) return NIN_OK;   // (NULL: the caller asks for the layout alone, which needs no factorisation)
    if (!op->linearized) return fail(NIN_ESTATE, "the gradient operator has not been factorised (call %s first)", kFactorize);
    return dev_fetch(gop, op->gop, (size_t)op->n_values);
}
