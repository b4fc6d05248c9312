// abi_apply.hip -- the C ABI, part 5: W u, W^T v with the cell-major index behind it, the GLS adjoint and the GLS tangent.
#include <hipcub/hipcub.hpp>

#include "abi_internal.hpp"
#include "gls_adjoint.hpp"

using namespace nin;

// The cell-major index of the esup pattern (DeviceGrid::tr_*), built once per grid by the first transpose call: a stable radix sort
// of the pairs (esup[j], j) by cell keeps ascending j -- hence ascending node id -- within each cell; cell_ptr and the node of each
// position follow by binary search.  Synchronises `stream` (the sort's temporaries are freed before the call returns).
int nin::ensure_transpose_index(DeviceGrid &d, hipStream_t stream) {
    if (d.tr_cell_ptr) return NIN_OK;
    const int32_t E = d.v.n_elems, nnz = (int32_t)d.nnz_e;
    int32_t *&ptr = d.tr_cell_ptr, *&pos = d.tr_cell_pos, *&node = d.tr_cell_node;   // (cleared again if the build fails)
    DevTmp<int32_t> cells_sorted;
    DevTmp<void> tmp;
    size_t tmp_bytes = 0;
    int end_bit = 1;
    while (end_bit < 31 && (int64_t{1} << end_bit) < (int64_t)E) ++end_bit;   // the cell ids fit in end_bit bits
    int rc = dev_alloc(d, &ptr, (size_t)E + 1);
    if (!rc) rc = dev_alloc(d, &pos, (size_t)nnz);
    if (!rc) rc = dev_alloc(d, &node, (size_t)nnz);   // holds the sort's values 0 .. nnz-1 until cell_node overwrites it
    auto step = [&](hipError_t e) { if (e != hipSuccess && rc == NIN_OK) rc = fail(NIN_EHIP, "transpose index: %s", hipGetErrorString(e)); return rc == NIN_OK; };
    if (!rc && nnz > 0) {
        if (step(hipMalloc((void **)&cells_sorted, (size_t)nnz * sizeof(int32_t))) &&
            step(launch_iota(node, nnz, stream) ? hipErrorLaunchFailure : hipSuccess) &&
            step(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d.v.esup, cells_sorted.p, node, pos, nnz, 0, end_bit, stream)) &&
            step(hipMalloc(&tmp, tmp_bytes)) &&
            step(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, d.v.esup, cells_sorted.p, node, pos, nnz, 0, end_bit, stream)))
            (void)step(launch_transpose_index_fill(d.v, cells_sorted, nnz, ptr, pos, node, stream) ? hipErrorLaunchFailure : hipSuccess);
        (void)step(hipStreamSynchronize(stream));
    } else if (!rc) {
        (void)step(launch_transpose_index_fill(d.v, nullptr, 0, ptr, pos, node, stream) ? hipErrorLaunchFailure : hipSuccess);
        (void)step(hipStreamSynchronize(stream));
    }
    if (rc) { dev_release(d, ptr); dev_release(d, pos); dev_release(d, node); }
    return rc;
}

// the weights of the last apply: one buffer per grid, allocated on first use
static int ensure_apply_weights(DeviceGrid &d) {
    return d.apply_weights ? NIN_OK : dev_alloc(d, &d.apply_weights, (size_t)std::max<int64_t>(d.nnz_e, 1));
}

int nin_grid_has_transpose_index(const nin_grid *g) { return g && g->d.tr_cell_ptr ? 1 : 0; }

int nin_apply_device(nin_grid *g, int method, const double *dev_u_cells, int32_t n_fields, double *dev_node_values,
                     double *dev_neumann_ws, void *stream_) {
    if (!g || !dev_u_cells || !dev_node_values || !dev_neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintWeights)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = ensure_apply_weights(d)) return rc;
    // GLS on a mesh with cube nodes: the cube-node kernel forms W . u itself (the 64 bytes of a node's row are neither written
    // nor read again); the other kernels write their rows as always and a list kernel applies those (NIN_APPLY_NO_FUSION: off)
    const DeviceGrid::GlsList &cube = d.plan[gk::hex8];
    if (method == NIN_METHOD_GLS && cube.count > 0 && d.noncube_nodes_ready && getenv("NIN_APPLY_NO_FUSION") == nullptr) {
        int rc = weights_ready(d, method);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(d.gls_queue, 0, kGlsQueueInts * sizeof(int32_t), stream));
        rc = gls_side_begin(d, -1, 1, d.apply_weights, dev_neumann_ws, stream);
        if (!rc) rc = launch_gls_hex8mf_apply(d.v, cube.nodes, reinterpret_cast<const int32_t *>(cube.desc), cube.count, 1, dev_u_cells, n_fields,
                                              dev_node_values, dev_neumann_ws, d.gls_queue + gls_plan_row(gk::hex8).counter, stream);
        if (!rc) rc = gls_main(d, -1, false, gls_only(), 1, d.apply_weights, dev_neumann_ws, stream);
        if (!rc) rc = launch_apply_list(d.v, d.apply_weights, dev_u_cells, n_fields, dev_node_values, d.noncube_nodes, d.noncube_count, stream);
        if (rc) return rc;
        return NIN_OK;
    }
    // the weights are computed ONCE, whatever the number of fields (they depend on the mesh, the permeability and the
    // Neumann flags only: the reference's callers do `weights.dot(u)` per field with the same matrix)
    int rc = nin_weights_device(g, method, nullptr, 0, 1, d.apply_weights, dev_neumann_ws, stream_);
    if (rc) return rc;
    rc = n_fields == 1 ? launch_apply(d.v, d.apply_weights, dev_u_cells, dev_node_values, (int32_t)g->h.mx_elems_per_point, d.nnz_e, stream)
                       : launch_apply_fields(d.v, d.apply_weights, dev_u_cells, n_fields, dev_node_values, (int32_t)g->h.mx_elems_per_point, d.nnz_e, stream);
    if (rc) return fail(rc, "launch failed");
    return NIN_OK;
}

int nin_apply_fields_host(nin_grid *g, int method, const double *u_cells, int32_t n_fields, double *node_values,
                          double *neumann_ws) {
    if (!g || !u_cells || !node_values || !neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintWeights, false)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    const size_t pb = (size_t)g->h.n_points * 8, eb = (size_t)g->h.n_elems * 8;
    DevTmp<double> dn, du, dv;
    HIP_TRY(hipMalloc((void **)&dn, pb));
    HIP_TRY(hipMalloc((void **)&du, eb * n_fields));
    HIP_TRY(hipMalloc((void **)&dv, pb * n_fields));
    HIP_TRY(hipMemcpy(du, u_cells, eb * n_fields, hipMemcpyHostToDevice));
    const int rc = nin_apply_device(g, method, du, n_fields, dv, dn, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(node_values, dv, pb * n_fields, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(neumann_ws, dn, pb, hipMemcpyDeviceToHost));
    return NIN_OK;
}

int nin_apply_host(nin_grid *g, int method, const double *u_cells, double *node_values, double *neumann_ws) {
    return nin_apply_fields_host(g, method, u_cells, 1, node_values, neumann_ws);
}

int nin_spmv_device(nin_grid *g, const double *dev_csr_data, const double *dev_u_cells, int32_t n_fields, double *dev_node_values,
                    void *stream_) {
    if (!g || !dev_csr_data || !dev_u_cells || !dev_node_values) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // the kernels nin_apply_device runs after its weights, on the caller's weights
    const int rc = n_fields == 1 ? launch_apply(d.v, dev_csr_data, dev_u_cells, dev_node_values, (int32_t)g->h.mx_elems_per_point, d.nnz_e, stream)
                                 : launch_apply_fields(d.v, dev_csr_data, dev_u_cells, n_fields, dev_node_values, (int32_t)g->h.mx_elems_per_point,
                                                       d.nnz_e, stream);
    if (rc) return rc;
    return NIN_OK;
}

int nin_spmv_transpose_device(nin_grid *g, const double *dev_csr_data, const double *dev_node_values, int32_t n_fields,
                              double *dev_cell_values, void *stream_) {
    if (!g || !dev_csr_data || !dev_node_values || !dev_cell_values) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = ensure_transpose_index(d, stream);
    if (rc) return rc;
    rc = launch_apply_transpose(d.v, d.tr_cell_ptr, d.tr_cell_pos, d.tr_cell_node, d.v.dim == 2 ? 4 : 8, dev_csr_data, dev_node_values,
                                n_fields, dev_cell_values, stream);
    if (rc) return rc;
    return NIN_OK;
}

int nin_apply_transpose_fields_host(nin_grid *g, int method, const double *node_values, int32_t n_fields, double *cell_values) {
    if (!g || !node_values || !cell_values) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintWeights)) return rc;
    if (int rc = weights_ready(d, method, false)) return rc;   // (the weight launch below adds the size check)
    HIP_TRY(hipSetDevice(d.device));
    if (int rc = ensure_apply_weights(d)) return rc;
    const size_t P = (size_t)g->h.n_points, E = (size_t)g->h.n_elems, k = (size_t)n_fields;
    DevTmp<double> dn, dv, dx;
    int rc = dev_stage(dn, nullptr, P);
    if (!rc) rc = dev_stage(dv, node_values, P * k);
    if (!rc) rc = dev_stage(dx, nullptr, E * k);
    // the unfused weights (the fused cube-node apply writes no rows for cube nodes), with `+ neumann_ws[row]` as apply() uses them
    if (!rc) rc = nin_weights_device(g, method, nullptr, 0, 1, d.apply_weights, dn, nullptr);
    if (!rc) rc = nin_spmv_transpose_device(g, d.apply_weights, dv, n_fields, dx, nullptr);
    return rc ? rc : dev_fetch(cell_values, dx, E * k);
}

// ---- the GLS adjoint: dL/dK from dL/d(stored weights) (kernels_gls_adjoint.hip) ---------------------------------------
void nin::release_adjoint_state(DeviceGrid &d) {
    for (auto &b : d.adj_bin) { dev_release(d, b.nodes); b = DeviceGrid::AdjBin{}; }
    dev_release(d, d.adj_contrib);
    dev_release(d, d.shape_cell);
    dev_release(d, d.shape_face);
    dev_release(d, d.shape_slot);
    dev_release(d, d.shape_tan_cell);
    dev_release(d, d.shape_tan_face);
    d.shape_tan_n = 0;
    dev_release(d, d.adj_node_bin);
    dev_release(d, d.adj_dirty_lists);
    dev_release(d, d.adj_dirty_hist);
    dev_release(d, d.adj_dirty_hdr);
    dev_release(d, d.adj_dirty_tmp);
    d.adj_dirty_tmp_bytes = 0;
    dev_release(d, d.adj_scratch);
    d.adj_scratch_stride = 0;
    d.adj_scratch_slots = 0;
    d.adj_ready = false;
}

// The bins and the scratch slots, made by whichever of the backward, tangent and plan calls comes first.  Synchronises `stream` (one
// device-to-host copy of 8 bytes a node).
int nin::ensure_adjoint_bins(DeviceGrid &d, hipStream_t stream) {
    if (d.adj_ready) return NIN_OK;
    const int32_t P = d.v.n_points;
    const bool force_global = getenv("NIN_GLS_ADJ_FORCE_GLOBAL") != nullptr;   // testing switch: every system in global scratch
    std::vector<int64_t> bytes((size_t)std::max(P, 1));
    {
        DevTmp<int64_t> dev_bytes;
        HIP_TRY(hipMalloc((void **)&dev_bytes, bytes.size() * sizeof(int64_t)));
        hipError_t e = launch_adjoint_bytes(d.v, dev_bytes, stream) ? hipErrorLaunchFailure : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e == hipSuccess && P > 0) e = hipMemcpy(bytes.data(), dev_bytes, (size_t)P * sizeof(int64_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(NIN_EHIP, "adjoint bins: %s", hipGetErrorString(e));
    }
    std::vector<int32_t> lists[kAdjBins];
    int64_t mx[kAdjBins] = {};
    for (int32_t p = 0; p < P; ++p) {
        const int b = adj_node_bin(bytes[p], force_global);
        lists[b].push_back(p);
        mx[b] = std::max(mx[b], bytes[p]);
    }
    int rc = NIN_OK;
    for (int b = 0; b < kAdjBins && !rc; ++b) {
        DeviceGrid::AdjBin &bin = d.adj_bin[b];
        bin.count = (int32_t)lists[b].size();
        bin.bytes = mx[b];
        if (bin.count == 0) continue;
        rc = dev_alloc(d, &bin.nodes, lists[b].size());
        if (!rc && hipMemcpy(bin.nodes, lists[b].data(), lists[b].size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(NIN_EHIP, "adjoint bins: upload failed");
    }
    if (!rc && d.adj_bin[kAdjBins - 1].count > 0) {
        d.adj_scratch_slots = std::min<int32_t>(d.adj_bin[kAdjBins - 1].count, 256);
        d.adj_scratch_stride = mx[kAdjBins - 1] / 8;
        rc = dev_alloc(d, &d.adj_scratch, (size_t)d.adj_scratch_slots * (size_t)d.adj_scratch_stride);
    }
    if (rc) { release_adjoint_state(d); return rc; }
    d.adj_ready = true;
    return NIN_OK;
}

// The contribution buffer, 80 bytes per entry of esup: the backward call's alone -- the tangent writes straight into CSR position
static int ensure_adjoint_contrib(DeviceGrid &d) {
    return d.adj_contrib ? NIN_OK : dev_alloc(d, &d.adj_contrib, (size_t)std::max<int64_t>(d.nnz_e, 1) * 10);
}

AdjBinRun nin::adjoint_bin_run(const DeviceGrid &d, int b) {
    const DeviceGrid::AdjBin &bin = d.adj_bin[b];
    return {bin.nodes, bin.count, bin.bytes, d.adj_scratch, d.adj_scratch_stride, d.adj_scratch_slots};
}

int nin::adjoint_only_from_env() {
    const char *only = getenv("NIN_GLS_ADJ_ONLY");
    return only ? atoi(only) : -1;
}

int nin::derivative_ready(nin_grid *g, hipStream_t stream, bool coordinates) {
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintKernels)) return rc;
    if (coordinates && d.v.dim != 3)
        return fail(NIN_EINVAL, "the derivative with respect to the node coordinates is for 3-D grids only (this grid is %d-D)", (int)d.v.dim);
    if (int rc = weights_ready(d, NIN_METHOD_GLS, false)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    return ensure_adjoint_bins(d, stream);
}

// The adjoint kernel on the nodes of every bin (only >= 0: of that bin alone), the ten values of every (node, cell) pair into `contrib`:
// the grid's buffer for the backward call, a nin_gls_jacobian's own for a linearisation, a nin_gls_rjacobian's [nnz_esup][n_params]
// with `reduce`
int nin::launch_adjoint_bins(DeviceGrid &d, int add_neumann, int only, const double *grad_csr, const double *grad_nws, double *contrib,
                             hipStream_t stream, const AdjointReduce *reduce) {
    return for_each_adjoint_bin(d, only, [&](int b, const AdjBinRun &run) {
        return reduce ? launch_gls_adjoint_reduced(d.v, b, run, add_neumann ? 1 : 0, grad_csr, grad_nws, *reduce, contrib, stream)
                      : launch_gls_adjoint(d.v, b, run, add_neumann ? 1 : 0, grad_csr, grad_nws, contrib, stream);
    });
}

int nin_gls_weights_backward_device(nin_grid *g, int add_neumann, const double *dev_grad_csr, const double *dev_grad_neumann_ws,
                                    double *dev_grad_perm, double *dev_grad_diff_mag, void *stream_) {
    if (!g || !dev_grad_csr || !dev_grad_perm) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = derivative_ready(g, stream);
    if (!rc) rc = ensure_adjoint_contrib(d);
    if (!rc) rc = ensure_transpose_index(d, stream);
    if (rc) return rc;
    rc = launch_adjoint_bins(d, add_neumann, adjoint_only_from_env(), dev_grad_csr, dev_grad_neumann_ws, d.adj_contrib, stream);
    if (!rc) rc = launch_adjoint_gather(d.v, d.tr_cell_ptr, d.tr_cell_pos, d.adj_contrib, dev_grad_perm, dev_grad_diff_mag, stream);
    if (rc) return rc;
    return NIN_OK;
}

int nin_sddmm_device(nin_grid *g, const double *dev_u_cells, const double *dev_node_values, int32_t n_fields, double *dev_grad_csr,
                     void *stream_) {
    if (!g || !dev_u_cells || !dev_node_values || !dev_grad_csr) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintKernels)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    const int rc = launch_sddmm(d.v, dev_u_cells, dev_node_values, n_fields, dev_grad_csr, static_cast<hipStream_t>(stream_));
    if (rc) return rc;
    return NIN_OK;
}

// The two gradients of <v, W u> from host arrays: v [n_fields][P] and u [n_fields][E] up, grad_csr = the sampled product, `backward`
// (dev_grad_csr, dev_out) the device sibling, `out` [out_count] down.  W as apply() uses it (`+ neumann_ws[row]` included): the siblings
// run with add_neumann = 1, and nothing flows through neumann_ws itself
template <class Backward>
static int gradient_host(nin_grid *g, bool coordinates, const double *node_values, const double *cell_values, int32_t n_fields, double *out,
                         size_t out_count, Backward backward) {
    if (!g || !node_values || !cell_values || !out) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    if (int rc = derivative_ready(g, nullptr, coordinates)) return rc;
    const size_t k = (size_t)n_fields;
    DevTmp<double> dv, du, dg, dout;
    int rc = dev_stage(dv, node_values, (size_t)g->h.n_points * k);
    if (!rc) rc = dev_stage(du, cell_values, (size_t)g->h.n_elems * k);
    if (!rc) rc = dev_stage(dg, nullptr, (size_t)g->d.nnz_e);
    if (!rc) rc = dev_stage(dout, nullptr, out_count);
    if (!rc) rc = nin_sddmm_device(g, du, dv, n_fields, dg, nullptr);
    if (!rc) rc = backward(dg.p, dout.p);
    return rc ? rc : dev_fetch(out, dout, out_count);
}

int nin_gls_permeability_gradient_host(nin_grid *g, const double *node_values, const double *cell_values, int32_t n_fields,
                                       double *grad_permeability) {
    return gradient_host(g, false, node_values, cell_values, n_fields, grad_permeability, g ? (size_t)g->h.n_elems * 9 : 0,
                         [&](const double *dg, double *dk) { return nin_gls_weights_backward_device(g, 1, dg, nullptr, dk, nullptr, nullptr); });
}

// ---- the GLS adjoint in the node coordinates: dL/d point_coords from dL/d(stored weights) -----------------------------
// cbar, (fcbar, Nbar) and the faces' point slots: 24 bytes per entry of esup, 48 per entry of fsup, 96 per face; the first call's
static int ensure_shape_buffers(DeviceGrid &d) {
    int rc = d.shape_cell ? NIN_OK : dev_alloc(d, &d.shape_cell, (size_t)std::max<int64_t>(d.nnz_e, 1) * 3);
    if (!rc && !d.shape_face) rc = dev_alloc(d, &d.shape_face, (size_t)std::max<int64_t>(d.nnz_f, 1) * 6);
    if (!rc && !d.shape_slot) rc = dev_alloc(d, &d.shape_slot, (size_t)std::max<int32_t>(d.v.n_faces, 1) * 12);
    if (rc) { dev_release(d, d.shape_cell); dev_release(d, d.shape_face); dev_release(d, d.shape_slot); }
    return rc;
}

int nin_gls_weights_backward_points_device(nin_grid *g, int add_neumann, const double *dev_grad_csr, const double *dev_grad_neumann_ws,
                                           double *dev_grad_points, void *stream_) {
    if (!g || !dev_grad_csr || !dev_grad_points) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = derivative_ready(g, stream, true);
    if (!rc) rc = ensure_shape_buffers(d);
    if (!rc) rc = ensure_transpose_index(d, stream);
    if (!rc) rc = ensure_update_inputs(g);   // inpofa, as the update path brings it
    if (rc) return rc;
    // per-bin timing (tools/time_shape_adjoint.py), as in the backward call.  Timing only: a skipped bin's nodes keep stale records and
    // write no xbar_own, so the gathers add onto what dev_grad_points held -- NIN_OK, but the result means nothing (ninpol_amd.h)
    rc = for_each_adjoint_bin(d, adjoint_only_from_env(), [&](int b, const AdjBinRun &run) {
        return launch_gls_adjoint_points(d.v, b, run, add_neumann ? 1 : 0, dev_grad_csr, dev_grad_neumann_ws, d.shape_cell, d.shape_face,
                                         dev_grad_points, stream);
    });
    if (!rc) rc = launch_shape_gather(d.v, d.up_inpofa, d.tr_cell_ptr, d.tr_cell_pos, d.shape_cell, d.shape_face, d.shape_slot, dev_grad_points, stream);
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_points_gradient_host(nin_grid *g, const double *node_values, const double *cell_values, int32_t n_fields, double *grad_points) {
    return gradient_host(g, true, node_values, cell_values, n_fields, grad_points, g ? (size_t)g->h.n_points * 3 : 0,
                         [&](const double *dg, double *dx) { return nin_gls_weights_backward_points_device(g, 1, dg, nullptr, dx, nullptr); });
}

// ---- the GLS tangent: d(stored weights) along a direction dK (kernels_gls_adjoint.hip's tangent mode) -------------------
int nin_gls_weights_tangent_device(nin_grid *g, int add_neumann, int32_t n_tangents, const double *dev_tangent_perm,
                                   const double *dev_tangent_diff_mag, double *dev_tangent_csr, double *dev_tangent_neumann_ws,
                                   void *stream_) {
    if (!g || !dev_tangent_perm || !dev_tangent_csr) return fail(NIN_EINVAL, "NULL argument");
    if (n_tangents < 1) return fail(NIN_EINVAL, "n_tangents must be >= 1");
    DeviceGrid &d = g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = derivative_ready(g, stream)) return rc;
    // (per-bin timing, as in the backward call: the other bins' rows are not written)
    const int rc = for_each_adjoint_bin(d, adjoint_only_from_env(), [&](int b, const AdjBinRun &run) {
        return launch_gls_tangent(d.v, b, run, add_neumann ? 1 : 0, n_tangents, dev_tangent_perm, dev_tangent_diff_mag, dev_tangent_csr,
                                  dev_tangent_neumann_ws, d.nnz_e, stream);
    });
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_permeability_tangent_host(nin_grid *g, const double *tangent_permeability, const double *cell_values, int32_t n_fields,
                                      double *node_values, double *neumann_ws) {
    if (!g || !tangent_permeability || !cell_values || !node_values || !neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (int rc = derivative_ready(g, nullptr)) return rc;
    const size_t P = (size_t)g->h.n_points, E = (size_t)g->h.n_elems, k = (size_t)n_fields;
    DevTmp<double> dk, du, dw, dv, dn;
    int rc = dev_stage(dk, tangent_permeability, E * 9 * k);
    if (!rc) rc = dev_stage(du, cell_values, E * k);
    if (!rc) rc = dev_stage(dw, nullptr, (size_t)d.nnz_e * k);
    if (!rc) rc = dev_stage(dv, nullptr, P * k);
    if (!rc) rc = dev_stage(dn, nullptr, P * k);
    // dW as apply() uses W (`+ neumann_ws[row]` included): add_neumann = 1, the diff_mag chain folded; direction f meets field f
    if (!rc) rc = nin_gls_weights_tangent_device(g, 1, n_fields, dk, nullptr, dw, dn, nullptr);
    for (size_t f = 0; f < k && !rc; ++f) rc = nin_spmv_device(g, dw.p + f * (size_t)d.nnz_e, du.p + f * E, 1, dv.p + f * P, nullptr);
    if (!rc) rc = dev_fetch(node_values, dv, P * k);
    return rc ? rc : dev_fetch(neumann_ws, dn, P * k);
}

// ---- the GLS tangent in the node coordinates: d(stored weights) along a direction dX ---------------------------------
// dC and (dFc, dN) of n_tangents directions: 24 bytes per cell and 48 per face, per direction; grown to the largest batch seen
static int ensure_shape_tangent_buffers(DeviceGrid &d, int32_t n_tangents) {
    if (d.shape_tan_cell && d.shape_tan_face && n_tangents <= d.shape_tan_n) return NIN_OK;
    dev_release(d, d.shape_tan_cell);
    dev_release(d, d.shape_tan_face);
    d.shape_tan_n = 0;
    int rc = dev_alloc(d, &d.shape_tan_cell, (size_t)n_tangents * (size_t)std::max<int32_t>(d.v.n_elems, 1) * 3);
    if (!rc) rc = dev_alloc(d, &d.shape_tan_face, (size_t)n_tangents * (size_t)std::max<int32_t>(d.v.n_faces, 1) * 6);
    if (rc) { dev_release(d, d.shape_tan_cell); dev_release(d, d.shape_tan_face); return rc; }
    d.shape_tan_n = n_tangents;
    return NIN_OK;
}

int nin_gls_weights_tangent_points_device(nin_grid *g, int add_neumann, int32_t n_tangents, const double *dev_tangent_points,
                                          double *dev_tangent_csr, double *dev_tangent_neumann_ws, void *stream_) {
    if (!g || !dev_tangent_points || !dev_tangent_csr) return fail(NIN_EINVAL, "NULL argument");
    if (n_tangents < 1) return fail(NIN_EINVAL, "n_tangents must be >= 1");
    DeviceGrid &d = g->d;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = derivative_ready(g, stream, true);
    if (!rc) rc = ensure_update_inputs(g);   // inpoel and inpofa, as the update path brings them
    if (!rc) rc = ensure_shape_tangent_buffers(d, n_tangents);
    if (rc) return rc;
    rc = launch_shape_tangent_geometry(d.v, d.up_inpoel, d.up_inpofa, n_tangents, dev_tangent_points, d.shape_tan_cell, d.shape_tan_face, stream);
    // (per-bin timing, as in the K tangent: the other bins' rows are not written)
    if (!rc) rc = for_each_adjoint_bin(d, adjoint_only_from_env(), [&](int b, const AdjBinRun &run) {
        return launch_gls_tangent_points(d.v, b, run, add_neumann ? 1 : 0, n_tangents, dev_tangent_points, d.shape_tan_cell, d.shape_tan_face,
                                         dev_tangent_csr, dev_tangent_neumann_ws, d.nnz_e, stream);
    });
    if (rc) return rc;
    return NIN_OK;
}

int nin_gls_points_tangent_host(nin_grid *g, const double *tangent_points, const double *cell_values, int32_t n_fields, double *node_values,
                                double *neumann_ws) {
    if (!g || !tangent_points || !cell_values || !node_values || !neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    if (n_fields < 1) return fail(NIN_EINVAL, "n_fields must be >= 1");
    DeviceGrid &d = g->d;
    if (int rc = derivative_ready(g, nullptr, true)) return rc;
    const size_t P = (size_t)g->h.n_points, E = (size_t)g->h.n_elems, k = (size_t)n_fields;
    DevTmp<double> dx, du, dw, dv, dn;
    int rc = dev_stage(dx, tangent_points, P * 3 * k);
    if (!rc) rc = dev_stage(du, cell_values, E * k);
    if (!rc) rc = dev_stage(dw, nullptr, (size_t)d.nnz_e * k);
    if (!rc) rc = dev_stage(dv, nullptr, P * k);
    if (!rc) rc = dev_stage(dn, nullptr, P * k);
    // dW as apply() uses W (`+ neumann_ws[row]` included): add_neumann = 1; direction f meets field f
    if (!rc) rc = nin_gls_weights_tangent_points_device(g, 1, n_fields, dx, dw, dn, nullptr);
    for (size_t f = 0; f < k && !rc; ++f) rc = nin_spmv_device(g, dw.p + f * (size_t)d.nnz_e, du.p + f * E, 1, dv.p + f * P, nullptr);
    if (!rc) rc = dev_fetch(node_values, dv, P * k);
    return rc ? rc : dev_fetch(neumann_ws, dn, P * k);
}

int nin_gls_adjoint_plan(nin_grid *g, int64_t counts[4]) {
    if (!g || !counts) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintToDevice)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    const int rc = ensure_adjoint_bins(d, nullptr);
    if (rc) return rc;
    for (int b = 0; b < kAdjBins; ++b) counts[b] = d.adj_bin[b].count;
    return NIN_OK;
}
