// launch.hpp -- kernel launchers shared between the .hip translation units and the C ABI (internal), and the layer they are written in.
//
// A launcher (launch_*) returns 0 or a negative NIN_E* code; its launches are asynchronous on `stream`.  It ends -- and, where it
// launches more than once, follows every launch -- with launch_status(), which reads hipGetLastError() ONCE (the call clears the error)
// and, on failure, sets the text of nin_last_error() to "launch failed: <HIP's words>" right there and returns NIN_EHIP.  An argument a
// launcher refuses gets its code and its text through fail() at that place.  So whoever gets a non-zero code from a launcher hands it on
// as it is: the text stands, and asking HIP a second time would find "no error".
// blocks_for(n, per_block) is the grid of a kernel with one thread, or one group of lanes, per item and no grid stride; the capped,
// grid-stride grids (kernels_csr.hip's grid_for / apply_grid, the 256 * 32 caps, the per-XCD grids of the forward kernels) are other
// expressions and stay where they are.
// for_each_chunk<MAX>(n, fn) is the walk of a batched product over its n directions, MAX at a time: fn gets the size of the chunk as a
// compile-time constant (the kernel instantiation) and where the chunk begins, and a non-zero return ends the walk.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <type_traits>

#include "../../include/ninpol_amd.h"
#include "device_grid.hpp"

namespace nin {

// sets what nin_last_error() returns (per thread) and hands `code` back (abi_grid.hip); not a dynamic symbol
__attribute__((visibility("hidden"))) int fail(int code, const char *fmt, ...);

// the status of a launch: 0, or NIN_EHIP with HIP's words for `e` as the text of nin_last_error().  Without an argument: of the launch
// just made, read -- and thereby cleared -- once
inline int launch_status(hipError_t e) { return e == hipSuccess ? 0 : fail(NIN_EHIP, "launch failed: %s", hipGetErrorString(e)); }
inline int launch_status() { return launch_status(hipGetLastError()); }

// ceil(n / per_block) workgroups
inline dim3 blocks_for(int64_t n, int64_t per_block = 256) { return dim3((unsigned)((n + per_block - 1) / per_block)); }

// fn(std::integral_constant<int, NT>{}, t0) for t0 = 0, MAX, 2 MAX, ... < n with NT = min(MAX, n - t0); stops at the first non-zero
// return and hands it back, 0 otherwise
template <int NT, class Fn>
int call_chunk(int64_t left, Fn &fn, int32_t t0) {
    if constexpr (NT > 1)
        if (left < NT) return call_chunk<NT - 1>(left, fn, t0);
    return fn(std::integral_constant<int, NT>{}, t0);
}
template <int MAX, class Fn>
int for_each_chunk(int32_t n, Fn fn) {
    for (int64_t t0 = 0; t0 < n; t0 += MAX)
        if (int rc = call_chunk<MAX>(n - t0, fn, (int32_t)t0)) return rc;
    return 0;
}

#ifdef __HIPCC__
// dynamic LDS beyond the default limit: the attribute belongs to the (kernel, device) pair; raised once per new maximum, which the
// cache remembers under a lock (two host threads may launch on one grid).  A device the cache has no slot for, or none at all, sets the
// attribute every time
template <auto KERN>
inline int allow_dynamic_lds(size_t bytes) {
    if (bytes <= 48 * 1024) return 0;
    constexpr int kSlots = 64;
    static std::mutex lock;
    static size_t allowed[kSlots] = {};
    int dev = -1;
    const bool cached = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kSlots;
    std::lock_guard<std::mutex> hold(lock);
    if (cached && bytes <= allowed[dev]) return 0;
    if (int rc = launch_status(hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)))
        return rc;
    if (cached) allowed[dev] = bytes;
    return 0;
}
#endif

// all return 0 or a negative NIN_E* code; launches are asynchronous on `stream`
// targets == nullptr: all nodes 0 .. n_targets-1 (the wave-cooperative kernel); mx_row = MX_ELEMENTS_PER_POINT, nnz = the length of esup
// (the mean row length decides how many nodes make a tile)
int launch_idw(const GridView &g, const int32_t *targets, int32_t n_targets, int32_t mx_row, int64_t nnz, double *out, double *nws,
               hipStream_t stream);
int launch_ls(const GridView &g, const int32_t *targets, int32_t n_targets, int32_t mx_row, int64_t nnz, double *out, double *nws,
              hipStream_t stream);
// one GLS size class: `nodes` lists the class members (device), lds_bytes is per wave
int launch_gls_class(const GridView &g, const int32_t *nodes, int32_t count, int32_t lds_bytes,
                     int32_t rows_per_lane, int add_neumann, double *out, double *nws,
                     double *scratch, int64_t scratch_stride, int32_t scratch_slots, hipStream_t stream);
// the block kernel (kernels_gls_block.hip): one node per workgroup of `waves` wavefronts, system in LDS
// `queue`: one zeroed device int (the launch's work counter)
int launch_gls_block(const GridView &g, const int32_t *nodes, int32_t count, int32_t waves, int32_t col_slots,
                     int32_t lds_bytes, int add_neumann, double *out, double *nws, int32_t *queue, hipStream_t stream);
const char *kernel_name_gls_block();
// the multifrontal kernel for cube nodes (kernels_gls_hex8mf.hip): 4 lanes per node; `desc` = kHex8DescWords (32) words per list
// entry, one 32-byte gather record per lane (hex8_desc.hpp, filled by launch_hex8_desc), 16-byte aligned;
// `queue`: the grid's zeroed counter block + kGlsQueueHex8 (one work counter per XCD at queue + 16 * xcd, each on its own cache line:
// ints kGlsQueueHex8 .. + 112 are the kernel's, gls_plan.hpp)
int launch_hex8_desc(const GridView &g, const int32_t *nodes, int32_t count, int32_t *desc, hipStream_t stream);
int launch_gls_hex8mf(const GridView &g, const int32_t *nodes, const int32_t *desc, int32_t count, int add_neumann,
                      double *out, double *nws, int32_t *queue, hipStream_t stream);
int launch_gls_hex8mf_apply(const GridView &g, const int32_t *nodes, const int32_t *desc, int32_t count, int add_neumann,
                            const double *u_cells, int32_t n_fields, double *values, double *nws, int32_t *queue, hipStream_t stream);
const char *kernel_name_gls_hex8mf();
// the one-wavefront multifrontal kernel for two-coloured nodes (kernels_gls_mfw.hip); `desc` = kMfwDescWords (40) descriptor words per
// list entry (mfw_desc.hpp, filled by launch_mfw_desc); `queue`: one zeroed device int (the work counter)
int launch_mfw_desc(const GridView &g, const int32_t *nodes, int32_t count, uint32_t *desc, hipStream_t stream);
// `kind`: 0 = two-coloured nodes, 1 = those among them with at most kMfwSmallFronts fronts and kMfwSmallDense dense cells,
// 2 = the general kind (free faces, up to kMfwWideDense dense cells)
int launch_gls_mfw(const GridView &g, const int32_t *nodes, const uint32_t *desc, int32_t count, int kind, int add_neumann,
                   double *out, double *nws, int32_t *queue, hipStream_t stream);
const char *kernel_name_gls_mfw();
// the WIDE one-wavefront multifrontal kernel for interior nodes of unstructured meshes (kernels_gls_mfx.hip: up to 16 fronts + 21 dense
// cells, one wavefront per SIMD, the tiles in the accumulation registers); `desc` = kMfxDescWords (56) words per list entry
// (mfx_desc.hpp, filled by launch_mfx_desc); `queue`: one zeroed device int (the work counter)
int launch_mfx_desc(const GridView &g, const int32_t *nodes, int32_t count, uint32_t *desc, hipStream_t stream);
// `cls`: the size class of every node of the list (mfx_desc.hpp: mfx_size_class -- one kernel instantiation per class)
int launch_gls_mfx(const GridView &g, const int32_t *nodes, const uint32_t *desc, int32_t count, int cls, int add_neumann, double *out,
                   double *nws, int32_t *queue, hipStream_t stream);
const char *kernel_name_gls_mfx();
// interior nodes beyond the wide kernel's limits (kernels_gls_mfg.hip: up to 32 fronts + 40 dense cells; the tiles of the dense problem in a
// global-memory slot per resident wavefront); `desc` = kMfgDescWords (124) words per list entry (mfg_desc.hpp, filled by launch_mfg_desc);
// `tiles` = n_slots slots of kMfgSlotDoubles doubles; `queue`: one zeroed device int
int launch_mfg_desc(const GridView &g, const int32_t *nodes, int32_t count, uint32_t *desc, hipStream_t stream);
int launch_gls_mfg(const GridView &g, const int32_t *nodes, const uint32_t *desc, int32_t count, int add_neumann, double *out, double *nws,
                   int32_t *queue, double *tiles, int32_t n_slots, hipStream_t stream);
const char *kernel_name_gls_mfg();
// quad nodes (kernels_gls_quad4.hip: 4 cells, 4 internal + 4 boundary faces -- the nodes inside a boundary face of a hexahedron
// mesh): 2 lanes per node; `desc` = 2 descriptor words per list entry (quad4_desc.hpp), filled by launch_quad4_desc
int launch_quad4_desc(const GridView &g, const int32_t *nodes, int32_t count, int32_t *desc, hipStream_t stream);
int launch_gls_quad4(const GridView &g, const int32_t *nodes, const int32_t *desc, int32_t count, int add_neumann, double *out,
                     double *nws, hipStream_t stream);
// the one-wavefront dense kernel for small nodes (kernels_gls_mfw.hip): kind 0 / 1 / 2 = at most 4 / 8 / 12 cells, at most 64 rows
int launch_gls_small(const GridView &g, const int32_t *nodes, int32_t count, int kind, int add_neumann, double *out, double *nws,
                     hipStream_t stream);
// out[j] += nws[row(j)] for IDW / LS is a no-op (their neumann_ws is 0): nothing to launch.

// CSR finish (interpolator.pyx:622-624): count non-zeros per row, scan, compact
// rows [p_begin, p_end) only (p_end < 0: to the last node; p_begin: a multiple of 64)
int launch_row_nnz(const GridView &g, const double *data, int32_t *row_nnz, hipStream_t stream, int32_t p_begin = 0, int32_t p_end = -1);
int launch_compact(const GridView &g, const double *data, const int32_t *new_ptr, int32_t *indices,
                   double *vals, hipStream_t stream, int32_t p_begin = 0, int32_t p_end = -1);
// IDW (method_ls = 0) / LS (1) weights of the nodes [p_begin, p_end) (p_begin: a multiple of 64)
int launch_rows_range(const GridView &g, int method_ls, int32_t n_points, int32_t p_begin, int32_t p_end, int32_t mx_row, int64_t nnz,
                      double *out, double *nws, hipStream_t stream);

int launch_apply(const GridView &g, const double *data, const double *u, double *values, int32_t mx_row, int64_t nnz, hipStream_t stream);
// the same for the listed nodes only (one lane per node, rows straight from HBM)
int launch_apply_list(const GridView &g, const double *data, const double *u, int32_t k, double *values, const int32_t *list,
                      int32_t count, hipStream_t stream);
// k fields at once: u [k][n_elems], values [k][n_points]
int launch_apply_fields(const GridView &g, const double *data, const double *u, int32_t k, double *values, int32_t mx_row, int64_t nnz,
                        hipStream_t stream);

// the adjoint, x = W^T v: the cell-major index of the esup pattern (DeviceGrid::tr_*) and k node fields v [k][n_points] ->
// x [k][n_elems]; mx_cell = the most nodes of any cell (8 in 3-D, 4 in 2-D)
int launch_apply_transpose(const GridView &g, const int32_t *cell_ptr, const int32_t *cell_pos, const int32_t *cell_node, int32_t mx_cell,
                           const double *data, const double *v, int32_t k, double *x, hipStream_t stream);
// building that index (abi_apply.hip sorts the pairs (esup[j], j) by cell in between): dst[i] = i; then cell_ptr from the sorted cells and
// cell_node from the sorted positions
int launch_iota(int32_t *dst, int32_t n, hipStream_t stream);
int launch_transpose_index_fill(const GridView &g, const int32_t *sorted_cells, int32_t nnz, int32_t *cell_ptr, const int32_t *cell_pos,
                                int32_t *cell_node, hipStream_t stream);

// the sampled product (kernels_csr.hip): grad[pos] = sum_f v[f][p] u[f][esup[pos]] for every entry pos of every row p -- the gradient of
// <v, W u> with respect to the stored weights; u [k][n_elems], v [k][n_points], grad [nnz_esup]
int launch_sddmm(const GridView &g, const double *u, const double *v, int32_t k, double *grad, hipStream_t stream);

// the GLS adjoint (kernels_gls_adjoint.hip, gls_adjoint.hpp), all DEVICE pointers.
// launch_adjoint_bytes: bytes[p] = adj_node_bytes of node p.
// launch_gls_adjoint: the nodes of one bin (run.bytes: the largest slot among them; bin 3: run.scratch holds scratch_slots slots of
//   scratch_stride doubles); grad_csr [nnz_esup] = dL/d stored weights, grad_nws [n_points] = dL/d neumann_ws or null; writes the ten
//   values (Kbar[9], etabar) of every (node, cell) pair of the listed nodes to contrib [nnz_esup][10].
// launch_adjoint_gather: grad_perm [E][9] (and grad_diff_mag [E]; null: its term folded into the diagonal of grad_perm through the
//   resident g.perm) = per cell the sum of its nodes' slots, ascending node id, through the transpose index (cell_ptr, cell_pos)
// AdjBinRun: what every launch of the adjoint kernel on one bin takes from the grid -- the bin's nodes, the largest slot among them, the
//   scratch slots of bin 3 (abi_apply.hip makes one from DeviceGrid::adj_bin[b] and adj_scratch*)
struct AdjBinRun {
    const int32_t *nodes;
    int32_t count;
    int64_t bytes;
    double *scratch;
    int64_t scratch_stride;
    int32_t scratch_slots;
};
int launch_adjoint_bytes(const GridView &g, int64_t *bytes, hipStream_t stream);
int launch_gls_adjoint(const GridView &g, int bin, const AdjBinRun &run, int add_neumann, const double *grad_csr, const double *grad_nws,
                       double *contrib, hipStream_t stream);
int launch_adjoint_gather(const GridView &g, const int32_t *cell_ptr, const int32_t *cell_pos, const double *contrib, double *grad_perm,
                          double *grad_diff_mag, hipStream_t stream);
// launch_gls_adjoint_reduced: the same launch with the chain rule of perm_e = sum_m theta_(e,m) B_(e,m) folded in where the
//   ten values are: every (node, cell) pair writes its n_params values to reduced [nnz_esup][n_params], the diff_mag chain folded from
//   the resident g.perm; the 80-byte record is not stored.  basis: [E][n_params][9] with stride = 9 n_params, [n_params][9] with
//   stride = 0 (one set for every cell), or null (n_params = 1): the resident g.perm itself
struct AdjointReduce {
    int32_t n_params;
    const double *basis;
    int64_t stride;
};
int launch_gls_adjoint_reduced(const GridView &g, int bin, const AdjBinRun &run, int add_neumann, const double *grad_csr,
                               const double *grad_nws, const AdjointReduce &red, double *reduced, hipStream_t stream);
// launch_gls_adjoint_points: the same launch in the kernel's coordinate mode -- every listed node writes cbar of its cells to
//   cell_bar [nnz_esup][3], (fcbar, Nbar) of its faces to face_bar [nnz_fsup][6] and xbar_own to own_bar [P][3], zeros where the forward
//   has its zero row.  launch_shape_gather (kernels_gls_shape.hip) then takes them through the geometry to the vertices: inpofa [F][4] as
//   launch_update_geometry reads it, the transpose index (cell_ptr, cell_pos), face_slot [F][4][3] its own scratch; cell_bar is
//   overwritten; grad_points [P][3] holds xbar_own on entry and dL/d coords on return (3-D grids only)
int launch_gls_adjoint_points(const GridView &g, int bin, const AdjBinRun &run, int add_neumann, const double *grad_csr,
                              const double *grad_nws, double *cell_bar, double *face_bar, double *own_bar, hipStream_t stream);
int launch_shape_gather(const GridView &g, const int32_t *inpofa, const int32_t *cell_ptr, const int32_t *cell_pos, double *cell_bar,
                        const double *face_bar, double *face_slot, double *grad_points, hipStream_t stream);
// launch_gls_tangent: the same kernel's tangent mode on the nodes of one bin -- n_tangents directions tangent_perm [n_tangents][E][9]
//   (tangent_diff_mag [n_tangents][E], or null: folded from the resident g.perm) -> the directional derivative of the stored weights,
//   tangent_csr [n_tangents][nnz] in esup position, and of neumann_ws, tangent_nws [n_tangents][P] or null; every row of every listed
//   node is written
int launch_gls_tangent(const GridView &g, int bin, const AdjBinRun &run, int add_neumann, int32_t n_tangents, const double *tangent_perm,
                       const double *tangent_diff_mag, double *tangent_csr, double *tangent_nws, int64_t nnz, hipStream_t stream);
// launch_shape_tangent_geometry (kernels_gls_shape.hip): n_tangents directions tangent_points [n_tangents][P][3] of the
//   node coordinates through the geometry -- tangent_cell [n_tangents][E][3] = d centroid, tangent_face [n_tangents][F][6] = (d face
//   centre, d unit normal); inpoel [E][8] and inpofa [F][4] as launch_update_geometry reads them; every entry written (3-D grids only).
// launch_gls_tangent_points: the tangent mode of the adjoint kernel along those directions on the nodes of one bin, the outputs of
//   launch_gls_tangent
int launch_shape_tangent_geometry(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, int32_t n_tangents, const double *tangent_points,
                                  double *tangent_cell, double *tangent_face, hipStream_t stream);
int launch_gls_tangent_points(const GridView &g, int bin, const AdjBinRun &run, int add_neumann, int32_t n_tangents, const double *tangent_points,
                              const double *tangent_cell, const double *tangent_face, double *tangent_csr, double *tangent_nws, int64_t nnz,
                              hipStream_t stream);
// launch_gls_corner_gradients: the same kernel's gradient mode on the nodes of one bin -- n_fields cell fields u_cells
//   [n_fields][E] -> the gradient of the node's least-squares reconstruction in each of its cells, grad [n_fields][nnz][3] in esup
//   position, and the node value u_p = (r.b) / rho, node_values [n_fields][P] or null; every row of every listed node is written, zeros
//   where the forward has its zero row.  launch_corner_flux / launch_node_gradient (kernels_gls_gradient.hip) stream that buffer:
//   flux [n_fields][nnz][3] = -K_e g with the resident permeability, node_gradient [n_fields][P][3] = the mean of a row in row order
int launch_gls_corner_gradients(const GridView &g, int bin, const AdjBinRun &run, int32_t n_fields, const double *u_cells, double *grad,
                                double *node_values, int64_t nnz, hipStream_t stream);
int launch_corner_flux(const GridView &g, int64_t nnz, int32_t n_fields, const double *grad, double *flux, hipStream_t stream);
int launch_node_gradient(const GridView &g, int64_t nnz, int32_t n_fields, const double *grad, double *node_gradient, hipStream_t stream);

// the corner-gradient operator kept and applied, all DEVICE pointers.  Node p with ne cells owns the block G_p [3 ne x ne] at
// gop[gop_ptr[p] + j * 3 ne + i]: column j = the 3 ne corner gradients of p for the indicator of its cell j, i = 3 * (cell slot) + component.
// launch_gradop_layout: gop_ptr [P + 1] = the exclusive sum of 3 ne^2 (count [P + 1] and tmp scratch; tmp = null: *tmp_bytes is set to what
//   the scan needs and nothing is launched) and pos_node [nnz] = the node whose row holds the esup position.
// launch_gls_gradop_factorize (kernels_gls_adjoint.hip): the gradient mode on the nodes of one bin with the unit columns as its fields;
//   every entry of every listed node's block is written, zeros where the forward has its zero row.
// launch_gradop_apply: grad [n][nnz][3] = G . u [n][E], per entry j ascending from 0.0, up to kGradopChunk fields per pass over gop.
// launch_gradop_apply_transpose: ubar [n][E] = G^T . gbar [n][nnz][3]: dots [min(n, kGradopChunk)][nnz] takes the product of every column
//   with its node's slice of gbar (i ascending from 0.0), then a cell sums its entries in the order of the transpose index
constexpr int kGradopChunk = 4;
int launch_gradop_layout(const GridView &g, int64_t nnz, int64_t *count, void *tmp, size_t *tmp_bytes, int64_t *gop_ptr, int32_t *pos_node,
                         hipStream_t stream);
int launch_gls_gradop_factorize(const GridView &g, int bin, const AdjBinRun &run, const int64_t *gop_ptr, double *gop, hipStream_t stream);
int launch_gradop_apply(const GridView &g, int64_t nnz, const int64_t *gop_ptr, const int32_t *pos_node, const double *gop, int32_t n,
                        const double *u, double *grad, hipStream_t stream);
int launch_gradop_apply_transpose(const GridView &g, int64_t nnz, const int32_t *cell_ptr, const int32_t *cell_pos, const int64_t *gop_ptr,
                                  const int32_t *pos_node, const double *gop, int32_t n, const double *gbar, double *dots, double *ubar,
                                  hipStream_t stream);

// the GLS Jacobian kept and applied (kernels_gls_jacobian.hip), all DEVICE pointers; contrib [nnz_esup][10] as an adjoint
// launch with grad_csr = u[esup] left it, fold [E] = d diff_mag / d K_dd at the linearisation point.
// launch_jac_seed: grad_csr[pos] = u[esup[pos]].  launch_jac_fold: fold from the resident g.perm.
// launch_jac_apply: out [n][P] = J . (dperm [n][E][9], ddm [n][E] or null: folded); every entry written.
// launch_jac_apply_transpose: grad_perm [n][E][9] (grad_dm [n][E], or null: folded into the diagonal) = J^T . v [n][P], per cell in
//   ascending node id through the transpose index, the order of launch_adjoint_gather
int launch_jac_seed(const GridView &g, int64_t nnz, const double *u, double *grad_csr, hipStream_t stream);
int launch_jac_fold(const GridView &g, double *fold, hipStream_t stream);
int launch_jac_apply(const GridView &g, const double *contrib, const double *fold, int32_t n, const double *dperm, const double *ddm,
                     double *out, hipStream_t stream);
int launch_jac_apply_transpose(const GridView &g, const int32_t *cell_ptr, const int32_t *cell_pos, const int32_t *cell_node,
                               const double *contrib, const double *fold, int32_t n, const double *v, double *grad_perm, double *grad_dm,
                               hipStream_t stream);

// the reduced GLS Jacobian applied (kernels_gls_jacobian_reduced.hip), all DEVICE pointers; R [nnz_esup][M] as
// launch_gls_adjoint_reduced left it, M in {1, 3, 6} (anything else: NIN_EINVAL).
// launch_jacr_apply: out [n][P] = J_theta . dtheta [n][E][M]; every entry written.
// launch_jacr_apply_transpose: grad_theta [n][E][M] = J_theta^T . v [n][P], per cell in ascending node id through the transpose index
int launch_jacr_apply(const GridView &g, int32_t M, const double *R, int32_t n, const double *dtheta, double *out, hipStream_t stream);
int launch_jacr_apply_transpose(const GridView &g, int32_t M, const int32_t *cell_ptr, const int32_t *cell_pos, const int32_t *cell_node,
                                const double *R, int32_t n, const double *v, double *grad_theta, hipStream_t stream);

// the GLS Jacobian in the node coordinates applied (kernels_gls_shape_jacobian.hip), all DEVICE pointers; cell_bar
// [nnz_esup][3], face_bar [nnz_fsup][6] and own_bar [P][3] as launch_gls_adjoint_points with grad_csr = u[esup] left them, kept (read
// only here); inpoel / inpofa as launch_update_geometry reads them; the resident coordinates and normals are those of the linearisation.
// launch_xjac_apply: out [n][P] = J . dX [n][P][3], kXjacApplyChunk directions per pass over the records; tangent_cell / tangent_face: scratch
//   for launch_shape_tangent_geometry of one chunk ([min(n, chunk)][E][3] and [..][F][6]); every entry of out written.
// launch_xjac_apply_transpose: grad_points [n][P][3] = J^T . v [n][P], kXjacTransposeChunk fields per pass; cell_share [min(n, chunk)][E][3]
//   and face_slot [..][F][4][3] scratch; the transpose index as launch_shape_gather; with v = 1 what launch_shape_gather gives, bit for bit
constexpr int kXjacApplyChunk = 4, kXjacTransposeChunk = 2;
int launch_xjac_apply(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, const double *cell_bar, const double *face_bar,
                      const double *own_bar, int32_t n, const double *dX, double *tangent_cell, double *tangent_face, double *out,
                      hipStream_t stream);
int launch_xjac_apply_transpose(const GridView &g, const int32_t *inpofa, const int32_t *cell_ptr, const int32_t *cell_pos,
                                const int32_t *cell_node, const double *cell_bar, const double *face_bar, const double *own_bar, int32_t n,
                                const double *v, double *cell_share, double *face_slot, double *grad_points, hipStream_t stream);

// the same Jacobian assembled as a block-CSR matrix (kernels_gls_shape_assemble.hip), all DEVICE pointers: block (p, q) =
// dF_p / d x_q [3] for q in C(p) = {p} + the vertices of the cells of esup[p] + the points of the faces of fsup[p], ascending.
// The pattern, from the connectivity alone: launch_xjac_pattern_count writes |C(p)| to count [P + 1] (count[P] = 0), xjac_pattern_scan
//   is the exclusive sum of those P + 1 values into block_ptr (tmp = null: *tmp_bytes is set to what it needs), launch_xjac_pattern_fill
//   writes the columns at block_ptr[p] into block_col [block_ptr[P]].  force_slow != 0: every row through the path that stages nothing
//   (the same bytes).
// launch_xjac_assemble: values [block_ptr[P]][3] from the kept records through the resident coordinates and normals; every entry written.
int launch_xjac_pattern_count(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, int force_slow, int64_t *count, hipStream_t stream);
int xjac_pattern_scan(void *tmp, size_t *tmp_bytes, const int64_t *count, int64_t *block_ptr, int32_t n_points, hipStream_t stream);
int launch_xjac_pattern_fill(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, int force_slow, const int64_t *block_ptr,
                             int32_t *block_col, hipStream_t stream);
int launch_xjac_assemble(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, const double *cell_bar, const double *face_bar,
                         const double *own_bar, const int64_t *block_ptr, const int32_t *block_col, double *values, hipStream_t stream);

// kernels_csr.hip: dst[e] = (src[3 e], src[3 e + 1], src[3 e + 2], 0)
int launch_pad_centroids(const double *src, int64_t n_elems, double *dst, hipStream_t stream);
// GLS launch plan (grid_device.hip): the class byte of every node (gls_plan.hpp: gls_class_byte of the kernel that takes it; use_group =
// the GlsRoute bits) and, per block / scratch class, the maxima of (bytes, rows, columns) as 3 * kGlsClasses unsigned 64-bit values; all
// DEVICE pointers
int launch_classify(const GridView &g, int use_group, int force_global, uint8_t *node_class,
                    unsigned long long *class_max, hipStream_t stream);

// grid_update.hip: a moving mesh's geometry from new coordinates (nin_grid_update_points*), all DEVICE pointers.  First the grid's
// [P][3] coordinates from the caller's [P][coords_dim] (zero-padded), then centroids / face centres / float32 normals / areas from
// g.coords and the [E][8] / [E] / [F][4] connectivity the builders made; npoel8 = points per cell of element type t in byte t
int launch_update_coords(const double *dev_xyz, int coords_dim, int64_t n_points, double *coords, hipStream_t stream);
int launch_update_geometry(const GridView &g, uint64_t npoel8, const int32_t *inpoel, const int8_t *etype, const int32_t *inpofa,
                           double *centroids, double *face_center, float *face_normal, double *face_area, hipStream_t stream);

// fields_update.hip: the grid's perm [E][9] and diff_mag [E] from a caller's K [E][9] and an optional scale [E] (null: none), all
// DEVICE pointers; perm from hipMalloc (16-byte aligned), dev_K at any multiple of 8 bytes, neither overlapping the outputs.  Returns
// the launch's own error (read once: hipGetLastError clears it)
hipError_t launch_update_permeability(int32_t n_elems, const double *dev_K, const double *dev_scale, double *perm, double *diff_mag,
                                      hipStream_t stream);

// fields_scatter.hip: local permeability updates, all DEVICE pointers.
// The header block of the dirty set (DeviceGrid::dirty_hdr): where each plan kernel's list begins in the flat list buffer
// ([kGlsPlanKernels]: the total), the ids refused by scatters since the last dirty launch, and the cell of nin_grid_dirty_nodes
constexpr int kDirtyHdrOffsets = 0, kDirtyHdrRejected = kGlsPlanKernels + 2, kDirtyHdrCount = kGlsPlanKernels + 3, kDirtyHdrInts = 32;
static_assert(kDirtyHdrCount < kDirtyHdrInts, "the dirty set's header block is too small for the plan");
// perm / diff_mag of the cells dev_ids[0 .. n) (int32, or int64 when ids_are_int64) from dev_K [n][9] and dev_scale [n] (null: none), and
// dirty[v] = 1 for their vertices (inpoel [E][8], etype [E], npoel8 as launch_update_geometry); an id outside [0, n_elems) writes nothing
// and adds one to *rejected
int launch_scatter_permeability(const GridView &g, uint64_t npoel8, const int32_t *inpoel, const int8_t *etype, const void *dev_ids,
                                int ids_are_int64, int64_t n, const double *dev_K, const double *dev_scale, uint8_t *dirty, int32_t *rejected,
                                hipStream_t stream);
// grid_scatter.hip: local mesh motion, all DEVICE pointers.  coords[dev_ids[i]] = dev_xyz[i] ([n][coords_dim], zero-padded to three
// columns) for the ids (int32, or int64 when ids_are_int64) inside [0, n_points) -- one outside writes nothing and adds one to *rejected
// -- then, in a second kernel behind it, the centroids (g.centroids, and g.centroids4 where it is not null) of the cells around those
// nodes, the centres, normals and areas of the faces around them (launch_update_geometry's arithmetic and arrays), and dirty[v] = 1 for
// the vertices of those cells
int launch_scatter_points(const GridView &g, uint64_t npoel8, const int32_t *inpoel, const int8_t *etype, const int32_t *inpofa,
                          const void *dev_ids, int ids_are_int64, int64_t n, const double *dev_xyz, int coords_dim, double *face_area,
                          uint8_t *dirty, int32_t *rejected, hipStream_t stream);
// flags_update.hip: the Neumann bit of the resident flag bytes (flags [P]: bit0 boundary point, kept; bit1 Neumann) from DEVICE memory.
// dev_flags: float64 (set when (long long)x != 0, the host packer's rule) or, flags_are_bytes != 0, one byte per value (set when
// non-zero).  A byte is written only where it changes, and where it does dirty[p] = 1 (dirty null: no marks).  launch_set_flags: all
// n_points nodes from dev_flags [n_points]; launch_scatter_flags: the nodes dev_ids[0 .. n) (int32, or int64 when ids_are_int64) from
// dev_flags [n] -- an id outside [0, n_points) writes nothing, marks nothing and adds one to *rejected
int launch_set_flags(int32_t n_points, const void *dev_flags, int flags_are_bytes, uint8_t *flags, uint8_t *dirty, hipStream_t stream);
int launch_scatter_flags(int32_t n_points, const void *dev_ids, int ids_are_int64, int64_t n, const void *dev_flags, int flags_are_bytes,
                         uint8_t *flags, uint8_t *dirty, int32_t *rejected, hipStream_t stream);
// the marked nodes binned by plan kernel (single != 0: one list, IDW / LS) into `lists` [n_points], ascending node ids, list k at
// hdr[kDirtyHdrOffsets + k] .. hdr[kDirtyHdrOffsets + k + 1]; hist / scanned: dirty_compact_hist_ints() ints each, tmp: the scan's
// (dirty_compact_tmp_bytes).  clear != 0: the marks are cleared as they are read, unless *rejected is non-zero
size_t dirty_compact_hist_ints(int32_t n_points);
int dirty_compact_tmp_bytes(int32_t n_points, size_t *bytes);
int launch_dirty_compact(int32_t n_points, int single, int clear, uint8_t *dirty, const uint8_t *node_class, const int32_t *rejected,
                         int32_t *hist, int32_t *scanned, void *tmp, size_t tmp_bytes, int32_t *lists, int32_t *hdr, hipStream_t stream);
// *out += the number of marked nodes
int launch_dirty_count(int32_t n_points, const uint8_t *dirty, int32_t *out, hipStream_t stream);

// csr_dirty.hip: the rows of a dirty launch's list (`list` [total]: unique node ids in any order) counted and packed, all DEVICE
// pointers; `data` / `nws` as the weight kernels wrote them (esup position).  launch_dirty_row_nnz: pack_cnt[i] = entries != 0.0 of the
// row of list[i]; cnt [n_points], the resident count of every row, follows, and *changed += the rows whose count moved.
// launch_dirty_pack, behind the exclusive scan pack_off of pack_cnt: row i's surviving (column, value) pairs at pack_off[i] of
// pack_indices / pack_data (room for pack_off[total] entries), pack_node[i] = list[i], pack_nws[i] = nws[list[i]]
int launch_dirty_row_nnz(const GridView &g, const double *data, const int32_t *list, int32_t total, int32_t *pack_cnt, int32_t *cnt,
                         int32_t *changed, hipStream_t stream);
int launch_dirty_pack(const GridView &g, const double *data, const double *nws, const int32_t *list, int32_t total, const int32_t *pack_off,
                      int32_t *pack_node, double *pack_nws, int32_t *pack_indices, double *pack_data, hipStream_t stream);

// jacobian_dirty.hip: what a dirty relinearisation of a kept Jacobian runs before the adjoint kernel, all DEVICE pointers.
// The header of the adjoint's dirty lists: [b] where bin b's list begins in the flat list buffer ([kAdjBins]: the total) and
// [kAdjBins + 1] the grid's refused-id counter as the fill pass read it
constexpr int kAdjDirtyHdrInts = 8;
// bin_of[nodes[i]] = bin for the count nodes of one adjoint bin (bin_of [n_points])
int launch_adj_bin_byte(const int32_t *nodes, int32_t count, int32_t n_points, int bin, uint8_t *bin_of, hipStream_t stream);
// the marked nodes binned by adjoint bin into `lists` [n_points], ascending node ids, bin b at hdr[b] .. hdr[b + 1]; hist / scanned:
// adj_dirty_hist_ints() ints each, tmp: the scan's (adj_dirty_tmp_bytes).  clear != 0: the marks are cleared as they are read, unless
// *rejected is non-zero
size_t adj_dirty_hist_ints(int32_t n_points);
int adj_dirty_tmp_bytes(int32_t n_points, size_t *bytes);
int launch_adj_dirty_compact(int32_t n_points, int clear, uint8_t *dirty, const uint8_t *bin_of, const int32_t *rejected, int32_t *hist,
                             int32_t *scanned, void *tmp, size_t tmp_bytes, int32_t *lists, int32_t *hdr, hipStream_t stream);
// launch_jac_seed for the rows of list[0 .. total) alone: grad_csr[pos] = u[esup[pos]]
int launch_jac_seed_rows(const GridView &g, const int32_t *list, int32_t total, const double *u, double *grad_csr, hipStream_t stream);
// dirty[v] = 1 for the nodes dev_ids[0 .. n) (int32, or int64 when ids_are_int64) or, ids_are_cells != 0, for the vertices of those cells
// (inpoel / etype / npoel8 as launch_scatter_permeability); an id outside its range marks nothing and adds one to *rejected
int launch_mark_dirty(const GridView &g, uint64_t npoel8, const int32_t *inpoel, const int8_t *etype, const void *dev_ids, int ids_are_int64,
                      int64_t n, int ids_are_cells, uint8_t *dirty, int32_t *rejected, hipStream_t stream);

const char *kernel_name_idw();
const char *kernel_name_ls();
const char *kernel_name_gls();

}  // namespace nin
