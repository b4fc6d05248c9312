// abi_gradient.hip -- the corner gradients of the GLS reconstruction behind include/ninpol_amd.h: the gradient half of
// the per-node least-squares solve, per entry of esup, with the node values, the fluxes -K g and the nodal mean beside it.  Host code
// only: the factorisation is the adjoint kernel's gradient mode (kernels_gls_adjoint.hip), the two streaming kernels are
// kernels_gls_gradient.hip's.  tools/sanitize_gradient.sh runs the argument checks and the buffer sizing below under ASan + UBSan.
#include "abi_internal.hpp"

using namespace nin;

CornerGradientCounts nin::corner_gradient_counts(int64_t n_elems, int64_t n_points, int64_t nnz_esup, int32_t n_fields) {
    const size_t k = (size_t)n_fields;
    return {k * (size_t)n_elems, k * (size_t)nnz_esup * 3, k * (size_t)n_points, k * (size_t)n_points * 3};
}

// what both entry points answer before they look at a device: NULL arguments first, then the count, then the grid's dimension
static int corner_gradient_args(const nin_grid *g, const void *u, const void *grad, int32_t n_fields) {
    return gradient_args(g, u, grad, n_fields, "n_fields", "the corner gradients are");
}

int nin_gls_corner_gradients_device(nin_grid *g, int32_t n_fields, const double *dev_u_cells, double *dev_grad, double *dev_node_values,
                                    double *dev_flux, double *dev_node_gradient, void *stream_) {
    if (int rc = corner_gradient_args(g, dev_u_cells, dev_grad, n_fields)) return rc;
    DeviceGrid &d = g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = derivative_ready(g, stream)) return rc;
    // (per-bin timing, as in the tangent call: the other bins' rows are not written)
    int rc = for_each_adjoint_bin(d, adjoint_only_from_env(), [&](int b, const AdjBinRun &run) {
        return launch_gls_corner_gradients(d.v, b, run, n_fields, dev_u_cells, dev_grad, dev_node_values, d.nnz_e, stream);
    });
    if (!rc && dev_flux) rc = launch_corner_flux(d.v, d.nnz_e, n_fields, dev_grad, dev_flux, stream);
    if (!rc && dev_node_gradient) rc = launch_node_gradient(d.v, d.nnz_e, n_fields, dev_grad, dev_node_gradient, stream);
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_corner_gradients_host(nin_grid *g, const double *cell_values, int32_t n_fields, double *grad, double *node_values, double *flux,
                                  double *node_gradient) {
    if (int rc = corner_gradient_args(g, cell_values, grad, n_fields)) return rc;
    if (int rc = derivative_ready(g, nullptr)) return rc;
    const CornerGradientCounts n = corner_gradient_counts(g->h.n_elems, g->h.n_points, g->d.nnz_e, n_fields);
    DevTmp<double> du, dg, dv, df, dn;
    int rc = dev_stage(du, cell_values, n.u);
    if (!rc) rc = dev_stage(dg, nullptr, n.grad);
    if (!rc && node_values) rc = dev_stage(dv, nullptr, n.node_values);
    if (!rc && flux) rc = dev_stage(df, nullptr, n.grad);
    if (!rc && node_gradient) rc = dev_stage(dn, nullptr, n.node_gradient);
    if (!rc) rc = nin_gls_corner_gradients_device(g, n_fields, du, dg, dv, df, dn, nullptr);
    if (!rc) rc = dev_fetch(grad, dg, n.grad);
    if (!rc && node_values) rc = dev_fetch(node_values, dv, n.node_values);
    if (!rc && flux) rc = dev_fetch(flux, df, n.grad);
    if (!rc && node_gradient) rc = dev_fetch(node_gradient, dn, n.node_gradient);
    return rc;
}
