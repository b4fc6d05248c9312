/*
 * ninpol_amd.h -- C ABI of libninpol_amd.so: the MI355X-native nodal-interpolation hot path.
 *
 * The reference (daviyan5/ninpol) has no C ABI: its extension points are the Python class
 * `ninpol.Interpolator` and the in-process Cython method-plugin convention
 *     prepare(Grid grid, cells_data, points_data, faces_data, variable_to_index, variable,
 *             target_points, weights[out], neumann_ws[out])
 * (ninpol/_methods/idw.pxd:19-24, ls.pxd:20-25, gls.pxd:22-27; called at
 * ninpol/_interpolator/interpolator.pyx:657-665).  The entry points below are what a ctypes / cgo /
 * Cython binding for that path binds instead; each cites the reference interface it replaces.
 * Plain pointers and sizes only: no Python, numpy or torch types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success or a negative NIN_E* code; nin_last_error() gives text.
 *     Nothing throws, nothing aborts (the reference's inner helpers are `noexcept nogil` too).
 *   - index arrays crossing the boundary are int64 (`ctypedef long long DTYPE_I_t`, grid.pxd:13),
 *     reals are float64 (grid.pxd:14); inside the library and on the device indices are int32.
 *   - "host" pointers are ordinary memory owned by the caller; "dev" pointers are HIP device
 *     pointers (e.g. torch tensor .data_ptr()) owned by the caller; `stream` is a hipStream_t passed
 *     as void* (NULL = the null stream).
 *   - a nin_grid is NOT thread-safe (like one reference Interpolator instance); distinct handles are
 *     independent.
 */
#ifndef NINPOL_AMD_H
#define NINPOL_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nin_grid nin_grid; /* host connectivity + geometry (+ device mirror once uploaded) */

enum {
    NIN_OK = 0,
    NIN_EINVAL = -1,   /* bad argument (NULL, negative size, unknown name / method)            */
    NIN_ENOMEM = -2,   /* host or device allocation failed                                       */
    NIN_EHIP = -3,     /* a HIP runtime call failed (text in nin_last_error)                     */
    NIN_ENODEVICE = -4,/* no usable GPU / grid not uploaded: the product path has no CPU fallback */
    NIN_ERANGE = -5,   /* a count does not fit the int32 device layout, or a node is too large   */
    NIN_ESTATE = -6    /* call order (fields not set, grid not built ...)                        */
};

enum { NIN_METHOD_GLS = 0, NIN_METHOD_IDW = 1, NIN_METHOD_LS = 2 }; /* interpolator.pyx:60-64 order */

/* dtype codes reported by nin_grid_array */
enum { NIN_I64 = 0, NIN_F64 = 1 };

const char *nin_last_error(void);
const char *nin_version(void);

/* ---- Grid: connectivity + geometry, built once on the host ---------------------------------
 * Replaces Grid.__cinit__ (grid.pyx:47-140) + Grid.build() (:142-231) + load_point_coords (:661)
 * + calculate_centroids (:669) + calculate_normal_faces (:721), i.e. interpolator.pyx:194,204-207.
 * Arguments are the reference's Grid ctor arguments (same meaning, same -1 padding):
 *   npoel[8], nfael[8], lnofa[8][6], lpofa[8][6][4], nedel[8], lpoed[8][12][2],
 *   connectivity[n_elems][8], element_types[n_elems], coords[n_points][coords_dim].
 * Results are bit-identical to the reference's for conforming meshes (integers, float64 centroids
 * and face centres, float32-valued normals and areas).  num_threads <= 0 picks the OpenMP default. */
int nin_grid_create(int64_t dim, int64_t n_elems, int64_t n_points,
                    const int64_t *npoel, const int64_t *nfael, const int64_t *lnofa,
                    const int64_t *lpofa, const int64_t *nedel, const int64_t *lpoed,
                    const int64_t *connectivity, const int64_t *element_types,
                    const double *coords, int coords_dim, int build_edges, int num_threads,
                    nin_grid **out);
void nin_grid_destroy(nin_grid *g);

/* The same Grid, built ON `device` (grid.pyx:142-231, 233-525, 669-809 as data-parallel HIP kernels,
 * csrc/grid_device.hip): same arguments, same arrays bit for bit.  The arrays the weight kernels read stay in
 * HBM -- a later nin_grid_to_device(g, device) adopts them instead of uploading -- and all of them are mirrored
 * to the host for nin_grid_array_*.  No CPU fallback: NIN_ENODEVICE without a GPU. */
int nin_grid_create_on_device(int64_t dim, int64_t n_elems, int64_t n_points,
                              const int64_t *npoel, const int64_t *nfael, const int64_t *lnofa,
                              const int64_t *lpofa, const int64_t *nedel, const int64_t *lpoed,
                              const int64_t *connectivity, const int64_t *element_types,
                              const double *coords, int coords_dim, int build_edges, int device,
                              nin_grid **out);

/* Readonly attributes of Grid (grid.pxd:128-187).  Scalars: dim n_elems n_points n_faces n_edges
 * MX_ELEMENTS_PER_POINT MX_POINTS_PER_POINT MX_ELEMENTS_PER_FACE MX_FACES_PER_POINT; of the library's own: coords_dim nnz_esup
 * nnz_fsup gls_adjoint_contrib_bytes (the GLS adjoint's contribution buffer as allocated now, 0: not there) gls_shape_contrib_bytes
 * (the same for the three buffers of the adjoint in the node coordinates).  Unknown -> -1. */
int64_t nin_grid_scalar(const nin_grid *g, const char *name);

/* Number of elements of array `name` and its dtype code; arrays: esup esup_ptr psup psup_ptr fsup
 * fsup_ptr esuf esuf_ptr esuel infael inpofa inpoel inpoed inedel boundary_faces boundary_points
 * point_coords centroids faces_centers normal_faces faces_areas element_types. */
int nin_grid_array_info(nin_grid *g, const char *name, int64_t *count, int *dtype);
/* Copy array `name` into caller memory of `count` elements (int64 or float64 as reported). */
int nin_grid_array_copy(nin_grid *g, const char *name, void *dst, int64_t count);

/* ---- device residency --------------------------------------------------------------------- */
int nin_device_count(int *count);
/* Push the CSR connectivity (esup, fsup), the per-face pair/centre/normal and the geometry to the
 * HBM of `device` in the canonical int32 / SoA layout.  north_star: "built once as CSR
 * on host and pushed to HBM". */
int nin_grid_to_device(nin_grid *g, int device);
int nin_grid_device(const nin_grid *g); /* device id or -1 */

/* ---- moving meshes ---------------------------------------------------------------------------
 * New node coordinates for a loaded grid whose connectivity stays: point_coords, centroids, faces_centers, normal_faces and
 * faces_areas are made again (the reference's load_point_coords() + calculate_centroids() + calculate_normal_faces(),
 * grid.pyx:661-809), bit for bit what a fresh nin_grid_create* of the moved mesh holds.  Nothing else changes: connectivity
 * arrays, scalars, boundary flags, the resident permeability and Neumann flags, the GLS launch plan and the transpose index stay
 * (the plan's node lists keep the locality order of the coordinates they were planned with: that order affects speed only, never a
 * weight).  Weights computed before the update (a caller's csr_data buffers) are those of the old geometry.
 *
 * nin_grid_update_points: xyz is a HOST array [n_points][coords_dim]; synchronous.  On a grid that holds device arrays (built on a
 * device, or after nin_grid_to_device) the coordinates are uploaded and the kernels of csrc/grid_update.hip run; on a host-only
 * grid the host builder's geometry code runs again.  Both give the same bits.
 * nin_grid_update_points_device: dev_xyz is a DEVICE array of the same shape on the grid's device, not overlapping any grid array;
 * asynchronous on `stream` (hipStream_t): later launches on that stream -- the GLS side stream forks from it -- see the new
 * geometry; work on other streams, and the host-synchronous entry points (nin_weights_host, nin_interpolate_csr_host,
 * nin_apply_*_host: they run on the null stream), must be ordered behind `stream` by the caller.  NIN_ENODEVICE when
 * nin_grid_device(g) is -1.
 * Both: NIN_EINVAL for a NULL argument or a coords_dim other than the grid's.  The first update of a grid on a device puts inpoel,
 * element_types, inpofa and a face-area array there (0.32 + 0.01 + 0.48 + 0.24 GB of HBM at 10 M hexahedra; a grid built on the device
 * already has them) and is synchronous; they go with nin_grid_release_scratch and come back at the next update.  The host mirror
 * does not go stale: nin_grid_array_copy of the five arrays after an update waits for it and fetches the new values on first use
 * (nothing is copied back by the update itself). */
int nin_grid_update_points(nin_grid *g, const double *xyz, int coords_dim);
int nin_grid_update_points_device(nin_grid *g, const double *dev_xyz, int coords_dim, void *stream);
/* Geometry updates the grid's device copy has seen since it was made (0 without one): a cheap way to tell that an update went
 * through the device path. */
int64_t nin_grid_geometry_updates(const nin_grid *g);
/* 1 if the transpose index of nin_spmv_transpose_device is resident, else 0 (it survives an update of the points). */
int nin_grid_has_transpose_index(const nin_grid *g);

/* Per-call fields the plugins read from the data tables (idw.pyx:27-28, ls.pyx:27-28,
 * gls.pyx:47-59): permeability[E][3][3] row-major and diff_mag[E] (may be NULL for IDW / LS),
 * neumann_flag[P] (the points_data row, cast to integer like `.astype(int)`), neumann_val[P]
 * (may be NULL for IDW / LS).  Host pointers; uploaded to the grid's device.  permeability / diff_mag NULL leaves
 * the copies already on the device in place (they belong to the mesh, not to the variable).  neumann_flag NULL leaves the
 * flags already on the device in place (an earlier call's, or nin_fields_set_flags_device's); before any flags are resident
 * it is NIN_EINVAL: every method needs them. */
int nin_fields_set(nin_grid *g, const double *permeability, const double *diff_mag,
                   const double *neumann_flag, const double *neumann_val);

/* ---- changing permeability ---------------------------------------------------------------------
 * The permeability of a grid on a device replaced from DEVICE memory (nonlinear diffusion, mobility times absolute permeability
 * under Picard / Newton iteration: K changes every step and already lives on the GPU).  Nothing crosses the host.
 *
 * nin_fields_set_permeability_device: dev_permeability is a DEVICE array [n_elems][3][3] row-major on the grid's device, at any
 * 8-byte aligned address (at a 16-byte aligned one it is read in 16-byte pieces, else in 8-byte pieces: same result), dev_scale a DEVICE
 * array [n_elems] or NULL; neither overlaps a grid array.
 * The resident table becomes permeability[e][k] (dev_scale NULL) or dev_scale[e] * permeability[e][k] (one multiplication, rounded
 * once) and the resident diff_mag what nin_diff_mag makes of that table, bit for bit (csrc/fields_update.hip).  Asynchronous on
 * `stream` (hipStream_t), with the ordering rules of nin_grid_update_points_device: later launches on that stream see the new K;
 * work on other streams, and the host-synchronous entry points (nin_weights_host, nin_interpolate_csr_host, nin_apply_*_host: they
 * run on the null stream), must be ordered behind `stream` by the caller.  Needs no prior nin_fields_set and leaves the Neumann
 * flags as they are; GLS finds its permeability set afterwards.  A later nin_fields_set with a permeability replaces the table again.
 * NIN_EINVAL for a NULL grid or dev_permeability, NIN_ENODEVICE when nin_grid_device(g) is -1.
 * nin_fields_get_permeability: the resident tables copied to HOST arrays permeability [n_elems][9] and diff_mag [n_elems] (either
 * may be NULL); host-synchronous, waits for everything enqueued on the device first.  NIN_EINVAL for a NULL grid, NIN_ENODEVICE as
 * above, NIN_ESTATE when no permeability is resident. */
int nin_fields_set_permeability_device(nin_grid *g, const double *dev_permeability, const double *dev_scale, void *stream);
int nin_fields_get_permeability(nin_grid *g, double *permeability, double *diff_mag);
/* Permeability updates from device memory the grid's device copy has seen since it was made (0 without one): the sibling of
 * nin_grid_geometry_updates -- a cheap way to tell which path an update took. */
int64_t nin_grid_field_updates(const nin_grid *g);

/* ---- local permeability updates: recompute only the rows that changed ---------------------------------------------------
 * A GLS row of node n reads the permeability of the cells around n only, so a change to cell e can move the rows of the vertices of e
 * and no others.  The grid keeps a DIRTY SET of nodes on the device: a scatter writes a subset of cells and marks their vertices, a
 * dirty launch recomputes exactly the marked rows IN PLACE in the caller's buffers.  Contract: if the caller's buffers held a full
 * result as of the last clear, they hold, after a dirty launch, what a full launch would write now, bit for bit.  The set does not
 * record why a node is dirty: IDW and LS recompute their marked rows too (and get the same bits).  All calls that touch the set of one
 * grid belong on ONE stream (or are ordered by the caller).
 *
 * nin_fields_scatter_permeability_device: dev_cell_ids [n] cell ids (int32, or int64 when ids_are_int64 != 0), dev_permeability [n][9]
 *   and dev_scale [n] or NULL, all DEVICE arrays on the grid's device.  Cell dev_cell_ids[i] of the resident table becomes row i
 *   (times dev_scale[i]: one multiplication, rounded once), its diff_mag what nin_diff_mag makes of that row, bit for bit; the vertices
 *   of the cell are marked.  Every id is checked on the device before any access: an id outside [0, n_elems) writes nothing and is
 *   counted; the next nin_weights_dirty_device reports the count.  Duplicate ids with identical rows are fine; with different rows one
 *   of them wins, and which one is unspecified.  Asynchronous on `stream`, no host copy (the first call on a grid brings the
 *   cell -> vertex table to the device and synchronises, as the first nin_grid_update_points* does).  Counts in
 *   nin_grid_field_updates.  n == 0 is a no-op.  NIN_ESTATE when no permeability is resident to patch.
 * nin_weights_dirty_device: the marked nodes are binned by kernel on the device (ascending node id per kernel), the counts and the
 *   refused-id counter come back in one 128-byte copy -- the ONLY synchronisation of the call (of `stream`) -- and the weight kernels run on
 *   the lists.  Rows outside the set are not touched and nothing is zeroed; a row IN the set is written by its kernel whether it is computed or
 *   the zero row of a Dirichlet node.  clear != 0: the set is empty afterwards.  *n_recomputed
 *   (may be NULL): the number of rows recomputed.  If ids were refused since the last dirty launch: NIN_EINVAL with the count in
 *   nin_last_error(), nothing is launched, the set is kept and the counter starts again from zero.
 *   "Everything is dirty" after nin_grid_to_device, a nin_fields_set with a permeability, nin_fields_set_permeability_device,
 *   the whole-mesh nin_grid_update_points* and nin_grid_dirty_reset(g, 1, ...): then the call is the ordinary full launch (and, with clear, ends that
 *   state).  nin_weights_device never touches the set: two buffers may be served from one grid (clear = 0 for all but the last).
 * nin_grid_dirty_nodes: the number of marked nodes; -1 when everything is dirty; 0 for a grid on no device.  A diagnostic: it waits for
 *   the WHOLE device (a scatter may be in flight on any stream) and works on the null stream, so it stalls every stream of the
 *   process -- not for a time loop (nin_weights_dirty_device returns the count of the rows it recomputed without that).
 * nin_grid_dirty_reset: all_dirty = 0 empties the set -- "the caller's buffers hold a full result as of now" -- and forgets refused ids;
 *   all_dirty != 0 marks everything (the Python layer does so when the Neumann flags of another variable are uploaded).  Asynchronous
 *   on `stream`. */
int nin_fields_scatter_permeability_device(nin_grid *g, const void *dev_cell_ids, int ids_are_int64, int64_t n,
                                           const double *dev_permeability, const double *dev_scale, void *stream);
int nin_weights_dirty_device(nin_grid *g, int method, int add_neumann, double *dev_csr_data, double *dev_neumann_ws, void *stream,
                             int clear, int64_t *n_recomputed);
int64_t nin_grid_dirty_nodes(nin_grid *g);
int nin_grid_dirty_reset(nin_grid *g, int all_dirty, void *stream);

/* ---- local mesh motion: move a subset of nodes, recompute only their rows -------------------------------------------------
 * A row of node v reads coords[v], the centroids of the cells around v and the centres and normals of the faces around v.  Moving node p
 * changes coords[p], the centroids of the cells around p and the centre, normal and area of the faces around p, and every such face lies
 * in such a cell: the rows that can move are those of the vertices of the cells around the moved nodes, and no others.  These calls
 * write the new coordinates, make the geometry of those cells and faces again -- bit for bit what the whole-mesh nin_grid_update_points*
 * writes there, and it would change nothing elsewhere -- and mark those vertices in the dirty set of the block above (GLS, IDW and LS
 * alike: every method reads the geometry); nin_weights_dirty_device then recomputes exactly the marked rows.  They do NOT make
 * everything dirty.  Connectivity, fields, the GLS launch plan and all scratch stay, as for nin_grid_update_points*.
 *
 * nin_grid_scatter_points_device: dev_node_ids [n] node ids (int32, or int64 when ids_are_int64 != 0) and dev_xyz [n][coords_dim], row i
 *   for node dev_node_ids[i], DEVICE arrays on the grid's device; coords_dim as at construction (columns beyond it stay zero).  Every id
 *   is checked on the device before any access: an id outside [0, n_points) moves nothing, marks nothing and is counted in the counter
 *   of nin_fields_scatter_permeability_device; the next nin_weights_dirty_device reports the count.  Duplicate ids with identical rows
 *   are fine; with different rows one of them wins, which one is unspecified, and the geometry is that of the coordinates that ended up
 *   in the grid.  Asynchronous on `stream` with the ordering rules of nin_grid_update_points_device (the first call on a grid brings the
 *   connectivity to the device and allocates the dirty set, and synchronises); host reads of the five geometry arrays wait for the
 *   update and fetch them again.  Counts in nin_grid_geometry_updates.  n == 0 is a no-op.  NIN_EINVAL for a NULL argument or a
 *   coords_dim that is not the grid's, NIN_ENODEVICE when nin_grid_device(g) is -1.
 * nin_grid_scatter_points: HOST arrays, int64 ids.  The ids are checked here: NIN_EINVAL with the count in nin_last_error() if any lies
 *   outside [0, n_points), and nothing is moved.  A grid that holds device arrays: ids and rows are staged, the same kernels run, the
 *   call waits.  A host-only grid: the host coordinates are patched and the host builder's geometry code runs over the mesh (there is
 *   no dirty set without a device). */
int nin_grid_scatter_points_device(nin_grid *g, const void *dev_node_ids, int ids_are_int64, int64_t n, const double *dev_xyz,
                                   int coords_dim, void *stream);
int nin_grid_scatter_points(nin_grid *g, const int64_t *node_ids, int64_t n, const double *xyz, int coords_dim);

/* ---- changing boundary conditions: Neumann flags from device memory -------------------------------------------------------
 * Which boundary nodes are computed and which get the zero row -- a boundary that switches between Dirichlet and Neumann, wells that
 * open and close, two variables with different Neumann sets served in turn -- changed where the flags already live.  Nothing crosses
 * the host.  The resident flag byte of a node is bit0 = boundary point (the mesh's, on the device since nin_grid_to_device, never
 * changed here) and bit1 = Neumann; these calls rewrite bit1.  A value is SET when, as float64, (long long)x != 0 -- truncation toward
 * zero, the rule of nin_fields_set (`.astype(int)`): 0.5, -0.5 and 1e-300 are not set, -1.0, 2.0 and 255.0 are; NaN and values of
 * magnitude >= 2^63 are outside the contract (the host's cast is undefined for them, and so is the result here) -- or, as one byte per
 * value (flags_are_bytes != 0: bool / uint8), when it is non-zero.
 * The flag of node n is read by row n of the weights and by no other (gls.pyx:165-214, idw.pyx:62-63, ls.pyx:58-59), so both setters
 * mark, in the dirty set of the blocks above, exactly the nodes whose Neumann bit CHANGED: an update that rewrites equal values marks
 * nothing.  nin_weights_dirty_device then writes those rows in place -- a node that became Dirichlet gets the zero row and
 * neumann_ws = 0 of a full launch.  Neither setter makes everything dirty, and while everything is dirty neither marks (no marks are
 * needed then); neumann_val is not part of the state (nin_fields_set ignores it too).  The GLS launch plan does not depend on the
 * flags and stays.
 *
 * nin_fields_set_flags_device: dev_flags is a DEVICE array [n_points] on the grid's device, float64 or one byte per node, at any
 *   address its type allows (bytes at an 8-byte aligned address are read eight at a time: same result), not overlapping a grid array.  One streaming pass; a byte is written only where it changes.  Needs no prior nin_fields_set: the methods find their
 *   fields set afterwards (GLS still needs a permeability).
 * nin_fields_scatter_flags_device: dev_node_ids [n] node ids (int32, or int64 when ids_are_int64 != 0) and dev_flags [n], value i for
 *   node dev_node_ids[i], DEVICE arrays on the grid's device.  Every id is checked on the device before any access: an id outside
 *   [0, n_points) writes nothing, marks nothing and is counted in the counter of nin_fields_scatter_permeability_device; the next
 *   nin_weights_dirty_device reports the count and names this call.  Duplicate ids with equal values are fine; with different values
 *   one of them wins, which one is unspecified, and the node is marked if its bit ends up different from what it was before the call.
 *   n == 0 is a no-op.  NIN_ESTATE when no flags are resident yet to patch.
 * Both: asynchronous on `stream` (hipStream_t) with the ordering rules of nin_fields_set_permeability_device -- later launches on that
 *   stream see the new flags; work on other streams, and the host-synchronous entry points (they run on the null stream), must be
 *   ordered behind `stream` by the caller; calls that touch the dirty set of one grid belong on one stream.  The first call on a grid
 *   allocates the dirty set and may synchronise once.  Both count in nin_grid_flag_updates.  NIN_EINVAL for a NULL argument or a
 *   negative n, NIN_ENODEVICE when nin_grid_device(g) is -1.  A later nin_fields_set with a neumann_flag replaces the flags again (and
 *   marks nothing: its caller decides what is dirty).
 * nin_fields_get_flags: the resident Neumann bits copied to a HOST array neumann [n_points], 0 or 1 each; host-synchronous, waits for
 *   everything enqueued on the device first.  NIN_EINVAL for a NULL argument, NIN_ENODEVICE as above, NIN_ESTATE when no flags are
 *   resident.
 * nin_grid_flag_updates: flag updates from device memory the grid's device copy has seen since it was made (0 without one): the
 *   sibling of nin_grid_field_updates. */
int nin_fields_set_flags_device(nin_grid *g, const void *dev_flags, int flags_are_bytes, void *stream);
int nin_fields_scatter_flags_device(nin_grid *g, const void *dev_node_ids, int ids_are_int64, int64_t n,
                                    const void *dev_flags, int flags_are_bytes, void *stream);
int nin_fields_get_flags(nin_grid *g, uint8_t *neumann /* [n_points], 0 or 1 */);
int64_t nin_grid_flag_updates(const nin_grid *g);

/* ---- the hot path -------------------------------------------------------------------------
 * Replaces supported_methods[method](grid, ..., target_points, weights, neumann_ws)
 * (interpolator.pyx:657-665 -> idw.pyx:14-84, ls.pyx:21-135, gls.pyx:38-474).
 *
 * Output layout: instead of the dense weights[n_target][MX_ELEMENTS_PER_POINT] table, weight j of
 * node p is written to csr_data[esup_ptr[p] + j] -- exactly the position the reference's COO fill
 * reads it into (interpolator.pyx:612-618), with column esup[esup_ptr[p] + j].  neumann_ws has
 * n_points entries.  Entries of nodes that the method skips (Dirichlet boundary nodes,
 * idw.pyx:62-63) and of nodes outside `targets` are 0.
 *
 * targets: int64 node ids (host pointer) or NULL for all nodes.  add_neumann != 0 applies
 * `data[j] = weights + neumann_ws[row]` of interpolator.pyx:618 in the same kernel.
 * dev_csr_data [nnz_esup] and dev_neumann_ws [n_points] are DEVICE pointers; with targets == NULL the
 * launch is asynchronous on `stream`; with a target list the call returns once the kernels have run
 * (the device copy of the list is owned by the call).
 * Threading: as in the reference, one Interpolator / grid is not re-entrant (interpolator.pxd: load_mesh mutates
 * self.grid): the GLS launches of a grid share its work counters, so keep ONE nin_weights_* / nin_apply_* call in
 * flight per grid (any number of grids may run concurrently, on the same or on different streams and devices). */
int nin_weights_device(nin_grid *g, int method, const int64_t *targets, int64_t n_targets,
                       int add_neumann, double *dev_csr_data, double *dev_neumann_ws, void *stream);

/* Same, with host outputs (allocates scratch on the device, synchronises, copies back). */
int nin_weights_host(nin_grid *g, int method, const int64_t *targets, int64_t n_targets,
                     int add_neumann, double *csr_data, double *neumann_ws);

/* Device-side finish of interpolator.pyx:622-624 (csr_matrix + eliminate_zeros): compacts the
 * esup-shaped (indptr = esup_ptr, indices = esup, data) triplet, dropping exact zeros.
 * Host outputs: indptr[n_points+1] (int32, what scipy picks for these sizes), indices / data sized
 * by the caller to nnz_esup; *nnz_out receives the surviving count. */
int nin_csr_compact_host(nin_grid *g, const double *dev_csr_data, int32_t *indptr, int32_t *indices,
                         double *data, int64_t *nnz_out, void *stream);

/* interpolate() in one call, host outputs: weights (with `+ neumann_ws[row]`, interpolator.pyx:618) for ALL nodes,
 * then the device-side csr_matrix + eliminate_zeros of interpolator.pyx:622-624.  indptr [n_points+1], indices and
 * data sized by the caller to nnz_esup (upper bound), neumann_ws [n_points]; *nnz_out = surviving entries. */
int nin_interpolate_csr_host(nin_grid *g, int method, int32_t *indptr, int32_t *indices, double *data,
                             int64_t *nnz_out, double *neumann_ws);

/* ---- a host matrix kept current: only the dirty rows cross PCIe -----------------------------------------------------------
 * nin_interpolate_csr_host runs every row and sends the whole matrix on every call.  A caller in a time loop -- a few cells' K edited,
 * a boundary layer moved, some flags flipped, and the scipy matrix needed again -- keeps a nin_hostmatrix instead: it owns device
 * buffers of its own (weights [nnz_esup], neumann_ws [n_points], surviving entries per row [n_points]; NOT the grid's call scratch,
 * which any nin_interpolate_csr_host overwrites), and after the local updates of the blocks above only the rows of the grid's dirty
 * set are recomputed (nin_weights_dirty_device into those buffers), counted, packed, transferred and patched into the caller's
 * arrays.  The result is bit for bit what nin_interpolate_csr_host returns for the mesh as it is now.  The caller owns the host arrays
 * (indptr [n_points + 1], indices and data with room for nnz_esup entries, neumann_ws [n_points]; page-locked for speed) and passes
 * them to every call.  One consumer per grid, as for nin_weights_dirty_device with clear != 0: the dirty set is the grid's.
 *
 * nin_hostmatrix_create: the device buffers; `method` is fixed.  NIN_ENODEVICE when nin_grid_device(g) is -1.
 * nin_hostmatrix_full: all rows (add_neumann = 1) into the matrix's buffers, then the count / scan / compaction of
 *   nin_csr_compact_host into the host arrays; *nnz_out = surviving entries.  Clears the grid's dirty set (marks, every-node flag and the
 *   counter of refused ids).  Host-synchronous on `stream`.  Also the second half of an update that found every node dirty (below).
 * nin_hostmatrix_update: the first half of an update.  *n_rows = the rows recomputed, 0 with an empty set (nothing is touched then).
 *   While every node is dirty the full launch runs, *n_entries = -1, and the caller finishes with nin_hostmatrix_full (which then does
 *   not launch again).  Otherwise the dirty rows are recomputed in the matrix's buffers, two kernels over the launch's list and one
 *   scan count and pack them -- what survives is `!= 0.0`: NaNs stay, +-0 go, the rule of nin_csr_compact_host -- 8 bytes come back
 *   (*n_entries = the packed entries, *n_changed = the rows whose count of surviving entries differs from what the matrix held), and
 *   the pack leaves for page-locked staging buffers on the grid's copy streams.  The call waits for `stream` twice: once inside
 *   nin_weights_dirty_device, once for those 8 bytes.  `clear` as there.  If ids were refused since the last call: NIN_EINVAL with
 *   nin_weights_dirty_device's text, nothing was launched, matrix and dirty set are as they were.
 * nin_hostmatrix_patch: the second half: waits for the transfers and patches the rows into the caller's arrays (nin_csr_patch_rows
 *   below).  *n_changed == 0: out_* NULL, the arrays are patched in place.  Otherwise out_indptr [n_points + 1], out_indices and out_data
 *   (room for nnz_esup entries; not overlapping the old arrays) receive the new matrix; neumann_ws is always patched in place.
 *   NIN_ESTATE when no update is waiting.  After a failure of either half every node counts as dirty.
 * nin_hostmatrix_destroy: gives the device and staging buffers back (waits for the device).
 * NIN_TIMING=1: the phases of an update on stderr ("[nin_hostmatrix] dirty launch | count + pack | D2H | host patch"), each waiting
 *   for its work. */
typedef struct nin_hostmatrix nin_hostmatrix;
int nin_hostmatrix_create(nin_grid *g, int method, nin_hostmatrix **out);
int nin_hostmatrix_full(nin_hostmatrix *m, int32_t *indptr, int32_t *indices, double *data, double *neumann_ws, int64_t *nnz_out,
                        void *stream);
int nin_hostmatrix_update(nin_hostmatrix *m, int clear, void *stream, int64_t *n_rows, int64_t *n_changed, int64_t *n_entries);
int nin_hostmatrix_patch(nin_hostmatrix *m, const int32_t *indptr, int32_t *indices, double *data, double *neumann_ws,
                         int32_t *out_indptr, int32_t *out_indices, double *out_data);
void nin_hostmatrix_destroy(nin_hostmatrix *m);

/* m rows of a CSR matrix replaced, on the host (OpenMP, no device involved): row nodes[i] becomes the counts[i] entries
 * pack_indices / pack_data [off[i] .. off[i + 1]) and neumann_ws[nodes[i]] = pack_nws[i].  The matrix is indptr [P + 1], indices, data;
 * `nodes` are distinct rows in any order, off [m + 1] the exclusive prefix sum of counts.
 *   out_* all NULL: every counts[i] must equal the row's length, and indices, data and neumann_ws are overwritten in place (the indices
 *     too: equal counts do not imply an equal pattern).
 *   out_* all given (not overlapping the inputs): out_indptr [P + 1] = the prefix sum of the patched row lengths, out_indices / out_data =
 *     the rows in order, unchanged ones copied from the old arrays, listed ones from the pack; neumann_ws is patched in place.
 * NIN_EINVAL, with every array as it was: a NULL argument (out_* aside) or only some of out_*, a negative P or m, a node outside
 * [0, P), a node listed twice, a negative count, off[0] != 0 or off[i + 1] - off[i] != counts[i], and -- in place -- a count that is not
 * the row's length.  NIN_ERANGE: the new matrix has more entries than int32 holds (out_indptr is then undefined).  Sets no
 * nin_last_error() text. */
int nin_csr_patch_rows(int64_t P, const int32_t *indptr, int32_t *indices, double *data, double *neumann_ws, int64_t m,
                       const int32_t *nodes, const int32_t *counts, const int32_t *off, const int32_t *pack_indices,
                       const double *pack_data, const double *pack_nws, int32_t *out_indptr, int32_t *out_indices, double *out_data);

/* Interpolate a cell field to the nodes without materialising the matrix on the host: weights for all nodes (with the
 * `+ neumann_ws[row]` of interpolator.pyx:618), then node_values = W . u_cells on the device -- what the reference's
 * callers compute next as `weights.dot(u)` (tests/utils/analytical.py:236).  Host pointers: u_cells [n_elems],
 * node_values [n_points] (0 on the empty rows of Dirichlet nodes), neumann_ws [n_points]. */
int nin_apply_host(nin_grid *g, int method, const double *u_cells, double *node_values, double *neumann_ws);

/* The same for n_fields cell fields at once -- the weights are computed ONCE and applied to every field (the
 * reference's callers loop `weights.dot(u)` over their variables with one matrix, tests/utils/analytical.py:236):
 * u_cells [n_fields][n_elems] -> node_values [n_fields][n_points], row-major.  _device: DEVICE pointers, asynchronous
 * on `stream` (hipStream_t, NULL = default); _fields_host: host pointers, synchronous. */
int nin_apply_device(nin_grid *g, int method, const double *dev_u_cells, int32_t n_fields, double *dev_node_values,
                     double *dev_neumann_ws, void *stream);
int nin_apply_fields_host(nin_grid *g, int method, const double *u_cells, int32_t n_fields, double *node_values,
                          double *neumann_ws);

/* ---- the adjoint: W^T v, and W . u on weights the caller holds -----------------------------------------------------------
 * W is exactly the matrix nin_apply_* use and interpolate() returns, `+ neumann_ws[row]` of interpolator.pyx:618 included: the weights
 * nin_weights_device(..., add_neumann = 1, ...) writes in esup / CSR position (entry j of node p at csr_data[esup_ptr[p] + j], column
 * esup[esup_ptr[p] + j]).  With that W, <W u, v> = <u, W^T v>; the empty rows of Dirichlet nodes contribute nothing.  The reference's
 * callers form W.T @ v in scipy on the host (no reference counterpart on the device).
 *
 * nin_spmv_device: node_values = W . u_cells for n_fields cell fields, u_cells [n_fields][n_elems] -> node_values [n_fields][n_points],
 *   row-major (the layout of nin_apply_fields_host): the kernels nin_apply_device runs after its weights, without recomputing them.
 * nin_spmv_transpose_device: cell_values[f][e] = sum over the nodes p of cell e of W[p, e] * node_values[f][p], node_values
 *   [n_fields][n_points] -> cell_values [n_fields][n_elems].  Deterministic, no atomics: each cell sums its nodes' terms in ascending node
 *   id (the order scipy's W.T @ v accumulates in); two calls agree bit for bit, and so do a batch of k fields and k single calls.  The
 *   first call on a grid builds the cell-major index of the esup pattern on the device (4 (E+1) + 8 nnz_esup bytes of HBM, kept by the
 *   grid until nin_grid_release_scratch) and synchronises `stream`; later calls are asynchronous on `stream`.
 * Both take DEVICE pointers (dev_csr_data [nnz_esup]) and a hipStream_t `stream` (NULL = default); neither needs nin_fields_set.
 * nin_apply_transpose_fields_host: the host-pointer counterpart of nin_apply_fields_host -- the weights of `method` (add_neumann = 1,
 *   unfused) into the grid's apply buffer, then nin_spmv_transpose_device; node_values [n_fields][n_points] -> cell_values
 *   [n_fields][n_elems]; synchronous.  NIN_ESTATE before nin_fields_set, or for GLS without permeability.
 * All three: NIN_EINVAL for a NULL pointer or n_fields < 1, NIN_ENODEVICE for a grid that is not on a device. */
int nin_spmv_device(nin_grid *g, const double *dev_csr_data, const double *dev_u_cells, int32_t n_fields, double *dev_node_values,
                    void *stream);
int nin_spmv_transpose_device(nin_grid *g, const double *dev_csr_data, const double *dev_node_values, int32_t n_fields,
                              double *dev_cell_values, void *stream);
int nin_apply_transpose_fields_host(nin_grid *g, int method, const double *node_values, int32_t n_fields, double *cell_values);

/* ---- the GLS weights differentiated with respect to the permeability ---------------------------------------------------------
 * The GLS weights are a function of the resident permeability K (and of diff_mag = (1 - 3 / tr K)^2, which the table derives from
 * it).  Given the gradient of a scalar L with respect to the STORED weights -- the entries nin_weights_device(NIN_METHOD_GLS, ...,
 * add_neumann, ...) writes, esup / CSR position -- these calls return dL/dK.  IDW and LS do not depend on K.  The reference has no
 * counterpart (its callers would difference the whole computation).  All pointers are DEVICE pointers, `stream` a hipStream_t.
 *
 * nin_gls_weights_backward_device: dev_grad_csr [nnz_esup] = dL/d csr_data; dev_grad_neumann_ws [n_points] = dL/d neumann_ws, or
 *   NULL (none); add_neumann as in the forward call whose weights were differentiated.  Writes dev_grad_perm [n_elems][9] = dL/dK
 *   (row-major 3 x 3 per cell) with diff_mag held fixed and dev_grad_diff_mag [n_elems] = dL/d diff_mag; with dev_grad_diff_mag
 *   NULL the chain through the table's diff_mag is folded into the diagonal of dev_grad_perm, which is then dL/dK altogether.
 *   Nodes the forward gives the zero row (Dirichlet boundary nodes, too few rows, a singular or non-finite system) contribute
 *   nothing.  It differentiates at what is resident NOW: geometry, flags, K.  One node per workgroup, a dense Householder QR kept
 *   for two least-squares solves; per (node, cell) pair ten values go to a contribution buffer, and every cell then sums its nodes'
 *   in ascending node id: deterministic, no atomics, two calls agree bit for bit.
 *   The first call on a grid bins the nodes by system size, allocates the contribution buffer -- 80 bytes per entry of esup: 6.4 GB
 *   at 216^3 hexahedra -- and the scratch slots of the systems that do not fit a CU's LDS, builds the transpose index of
 *   nin_spmv_transpose_device if it is not there, and synchronises `stream`; later calls are asynchronous on it.  All of it is kept
 *   by the grid until nin_grid_release_scratch.  NIN_ESTATE before nin_fields_set or without permeability, NIN_ENODEVICE for a grid
 *   that is not on a device, NIN_EINVAL for a NULL grid, dev_grad_csr or dev_grad_perm.
 *   The environment variable NIN_GLS_ADJ_FORCE_GLOBAL (read when the bins are made) sends every node through the global-scratch
 *   class: a testing switch.  NIN_GLS_ADJ_ONLY=<bin> (read at every call) launches only that bin's kernel before the gather:
 *   per-bin timing, the other nodes' slots keep what they held.
 * nin_sddmm_device: the sampled product dev_grad_csr[pos] = sum_f node_values[f][p] * u_cells[f][esup[pos]] for every entry pos of
 *   every row p -- the gradient of <node_values, W u_cells> with respect to the stored weights; u_cells [n_fields][n_elems],
 *   node_values [n_fields][n_points].  Asynchronous on `stream`; needs no fields.  NIN_EINVAL for a NULL pointer or n_fields < 1,
 *   NIN_ENODEVICE as above.
 * nin_gls_permeability_gradient_host: the host-pointer counterpart, the sibling of nin_apply_transpose_fields_host -- grad_permeability
 *   [n_elems][9] = d <node_values, W cell_values> / dK for the W of nin_apply_* (add_neumann = 1), the diff_mag chain folded;
 *   node_values [n_fields][n_points], cell_values [n_fields][n_elems]; synchronous.  Errors as the two calls it makes.
 * nin_gls_adjoint_plan: nodes per bin of the adjoint kernel -- the LDS classes of one, two and four wavefronts per node, then the
 *   global-scratch class (diagnostics and tests).  Makes the bins if they are not there (synchronous).
 *
 * The forward derivative, for Newton-Krylov, Gauss-Newton and forward-mode AD: the change of the stored weights along a direction dK.
 * nin_gls_weights_tangent_device: dev_tangent_perm [n_tangents][n_elems][9] = the directions dK (row-major 3 x 3 per cell);
 *   dev_tangent_diff_mag [n_tangents][n_elems] = the directions of diff_mag as an independent input, or NULL: folded,
 *   d diff_mag_e = 2 (1 - 3 / tr K_e) 3 / tr K_e^2 tr dK_e from the resident K.  Writes dev_tangent_csr [n_tangents][nnz_esup] =
 *   (d csr_data / dK) . dK in esup / CSR position, for the csr_data of nin_weights_device(NIN_METHOD_GLS, ..., add_neumann, ...) at
 *   what is resident NOW, and dev_tangent_neumann_ws [n_tangents][n_points] = the same for neumann_ws (NULL: not wanted).  Every
 *   entry of both is written: zeros for the nodes the forward gives the zero row, and for neumann_ws of the nodes that are not
 *   Neumann nodes.  The adjoint's kernel in its tangent mode: the same assembly and the same Householder QR, factored once per node
 *   for all n_tangents directions; per direction one application of Q^T, one forward substitution with R^T and one application of
 *   Q, written straight into CSR position -- no contribution buffer, no gather, no transpose index, no atomics; two calls agree bit
 *   for bit, and a batch equals its directions one by one.  With the backward call's dL/dK = Kbar:
 *   <grad_csr, tangent_csr> + <grad_neumann_ws, tangent_neumann_ws> = <Kbar, dK>.
 *   The first of the backward, tangent and plan calls on a grid bins the nodes and allocates the scratch slots (and synchronises
 *   `stream`); the 80 bytes per entry of the contribution buffer are allocated by the first BACKWARD call only
 *   (nin_grid_scalar "gls_adjoint_contrib_bytes": what is allocated now).  Later calls are asynchronous on `stream`.  Errors as
 *   nin_gls_weights_backward_device; NIN_EINVAL also for n_tangents < 1.  NIN_GLS_ADJ_FORCE_GLOBAL and NIN_GLS_ADJ_ONLY as there
 *   (with NIN_GLS_ADJ_ONLY the other bins' rows are not written).
 * nin_gls_permeability_tangent_host: the host-pointer counterpart, the sibling of nin_gls_permeability_gradient_host -- direction f
 *   meets field f: node_values[f] = dW_f . cell_values[f] with dW_f the tangent of the W of nin_apply_* (add_neumann = 1, the
 *   diff_mag chain folded) along tangent_permeability[f], and neumann_ws[f] the tangent of neumann_ws; tangent_permeability
 *   [n_fields][n_elems][9], cell_values [n_fields][n_elems], node_values and neumann_ws [n_fields][n_points]; synchronous.  Errors
 *   as the calls it makes (the tangent, then nin_spmv_device). */
int nin_gls_weights_backward_device(nin_grid *g, int add_neumann, const double *dev_grad_csr, const double *dev_grad_neumann_ws,
                                    double *dev_grad_perm, double *dev_grad_diff_mag, void *stream);
int nin_sddmm_device(nin_grid *g, const double *dev_u_cells, const double *dev_node_values, int32_t n_fields, double *dev_grad_csr,
                     void *stream);
int nin_gls_permeability_gradient_host(nin_grid *g, const double *node_values, const double *cell_values, int32_t n_fields,
                                       double *grad_permeability);
int nin_gls_adjoint_plan(nin_grid *g, int64_t counts[4]);
int nin_gls_weights_tangent_device(nin_grid *g, int add_neumann, int32_t n_tangents, const double *dev_tangent_perm,
                                   const double *dev_tangent_diff_mag, double *dev_tangent_csr, double *dev_tangent_neumann_ws,
                                   void *stream);
int nin_gls_permeability_tangent_host(nin_grid *g, const double *tangent_permeability, const double *cell_values, int32_t n_fields,
                                      double *node_values, double *neumann_ws);

/* ---- the GLS weights differentiated with respect to the node coordinates: a shape adjoint ---------------------------------------
 * The GLS weights are a function of the resident geometry too: the centroids of a node's cells, the centres and unit normals of its
 * faces and the node's own position fill its system, and all of them follow the node coordinates (nin_grid_update_points*).  Given
 * the gradient of a scalar L with respect to the STORED weights these calls return dL/d point_coords, for shape fitting, shape
 * optimisation and error-driven mesh motion -- one backward pass instead of two launches per coordinate.  3-D grids, GLS only: IDW
 * and LS depend on the coordinates as well but are not differentiated.  Not provided: a kept Jacobian in the coordinates, dirty-row /
 * local-motion variants, 2-D meshes, the sharded path, the Neumann values.  The tangent (forward mode) follows below.
 *
 * nin_gls_weights_backward_points_device: dev_grad_csr, dev_grad_neumann_ws and add_neumann as in nin_gls_weights_backward_device;
 *   writes dev_grad_points [n_points][3] = dL/d point_coords at what is resident NOW (geometry, flags, K).  The derivative is that
 *   of the real-valued model: the float32 casts of the stored normals count as the identity.  Nodes the forward gives the zero row
 *   contribute nothing, but every node -- Dirichlet nodes too -- receives gradient as a vertex of its cells and faces.  The adjoint
 *   kernel in its coordinate mode (the same bins, factorisation and slots) writes per node three records in a fixed order --
 *   xbar_own, cbar per entry of esup, (fcbar, Nbar) per entry of fsup -- and three gather kernels take them through the geometry
 *   (centroid, face centre, normal of the first three points of a face) to the vertices: per face in inpofa order, per cell in
 *   ascending node id, per node in row order.  No atomics: two calls agree bit for bit.
 *   The first call allocates 24 bytes per entry of esup, 48 per entry of fsup and 96 per face (1.9 + 5.8 + 2.9 GB at 216^3
 *   hexahedra; nin_grid_scalar "gls_shape_contrib_bytes": what is allocated now), makes the adjoint's bins, the transpose index and
 *   the connectivity copies of nin_grid_update_points* if they are not there, and synchronises `stream`; later calls are
 *   asynchronous on it.  Kept until nin_grid_release_scratch.  Errors as nin_gls_weights_backward_device (NULL: grid, dev_grad_csr,
 *   dev_grad_points), and NIN_EINVAL for a grid that is not 3-D.  NIN_GLS_ADJ_FORCE_GLOBAL as there.  NIN_GLS_ADJ_ONLY=<bin> is a
 *   TIMING switch only: the other bins' kernels are skipped, so their nodes' records keep what an earlier call left, xbar_own of
 *   those nodes is not written (the gathers add onto whatever dev_grad_points held) and the call still returns NIN_OK -- with a
 *   value that is no bin (tools/time_shape_adjoint.py: the three gathers alone) nothing of the result means anything.
 * nin_gls_points_gradient_host: the host-pointer counterpart, the sibling of nin_gls_permeability_gradient_host -- grad_points
 *   [n_points][3] = d <node_values, W cell_values> / d point_coords for the W of nin_apply_* (add_neumann = 1); node_values
 *   [n_fields][n_points], cell_values [n_fields][n_elems]; synchronous.  Errors as the two calls it makes. */
int nin_gls_weights_backward_points_device(nin_grid *g, int add_neumann, const double *dev_grad_csr, const double *dev_grad_neumann_ws,
                                           double *dev_grad_points, void *stream);
int nin_gls_points_gradient_host(nin_grid *g, const double *node_values, const double *cell_values, int32_t n_fields,
                                 double *grad_points);

/* ---- the GLS weights along a direction of the node coordinates: a shape tangent ---------------------------------------------------
 * The forward derivative in the coordinates, for a solver that moves the mesh (ALE, r-adaptivity, Newton-Krylov on a mesh-motion
 * residual, a Gauss-Newton shape fit) and for sensitivities along a few design directions: dW = (dW/dX) . dX without differencing
 * two nin_grid_update_points* + weight launches.  3-D grids, GLS only, as the shape adjoint above.
 *
 * nin_gls_weights_tangent_points_device: dev_tangent_points [n_tangents][n_points][3] = the directions dX.  Writes dev_tangent_csr
 *   [n_tangents][nnz_esup] and dev_tangent_neumann_ws [n_tangents][n_points] (NULL: not wanted) as nin_gls_weights_tangent_device
 *   does, at what is resident NOW (geometry, flags, K): every entry is written, zeros for the nodes the forward gives the zero row
 *   and for neumann_ws of the nodes that are not Neumann nodes.  The derivative is that of the real-valued model: the float32 casts
 *   of the stored normals count as the identity.  Two small kernels take dX through the geometry (d centroid per cell, d face
 *   centre and d unit normal per face: 24 bytes per cell and 48 per face, per direction; nin_grid_scalar
 *   "gls_shape_tangent_bytes": what is allocated now, grown to the largest n_tangents seen, kept until nin_grid_release_scratch),
 *   then the adjoint's kernel in its tangent mode factors every node once for all directions.  No contribution buffer, no
 *   transpose index, no atomics: two calls agree bit for bit and a batch equals its directions one by one.  With the shape
 *   adjoint's dL/dX = Xbar:  <grad_csr, tangent_csr> + <grad_neumann_ws, tangent_neumann_ws> = <Xbar, dX>.
 *   The first call makes the adjoint's bins and the connectivity copies of nin_grid_update_points* if they are not there (and
 *   synchronises `stream`); a call with more directions than any before reallocates the two buffers (hipFree waits for the
 *   device).  Errors as nin_gls_weights_tangent_device (NULL: grid, dev_tangent_points, dev_tangent_csr; n_tangents < 1), and
 *   NIN_EINVAL for a grid that is not 3-D; a refused call writes nothing.  NIN_GLS_ADJ_FORCE_GLOBAL and NIN_GLS_ADJ_ONLY as there.
 * nin_gls_points_tangent_host: the host-pointer counterpart, the sibling of nin_gls_permeability_tangent_host -- direction f meets
 *   field f: node_values[f] = dW_f . cell_values[f] along tangent_points[f] (add_neumann = 1), neumann_ws[f] the tangent of
 *   neumann_ws; tangent_points [n_fields][n_points][3], cell_values [n_fields][n_elems], node_values and neumann_ws
 *   [n_fields][n_points]; synchronous.  Errors as the calls it makes (the tangent, then nin_spmv_device). */
int nin_gls_weights_tangent_points_device(nin_grid *g, int add_neumann, int32_t n_tangents, const double *dev_tangent_points,
                                          double *dev_tangent_csr, double *dev_tangent_neumann_ws, void *stream);
int nin_gls_points_tangent_host(nin_grid *g, const double *tangent_points, const double *cell_values, int32_t n_fields,
                                double *node_values, double *neumann_ws);

/* ---- the corner gradients of the GLS reconstruction: the gradient half of the per-node solve --------------------------------------
 * A GLS node solves one least-squares system in 3 ne + 1 unknowns: a gradient for each of the ne cells around it, and the node
 * value.  The weights keep the node value alone.  These calls return the other 3 ne unknowns -- the gradient of the piecewise-linear
 * reconstruction in every cell around the node, continuous in flux and in the tangential derivative across the faces -- for MPFA-D
 * and nonlinear finite-volume fluxes, for the Darcy velocity -K grad u at the nodes, for error indicators.  Per node, with A, c, r and
 * rho of the weights (csrc/kernels_gls.hip) and a cell field u:  b = u on the cell rows and 0 on EVERY face row (the Neumann boundary
 * rows too: the values are those of a homogeneous system, as the stored weights are),  u_p = (r.b) / rho,
 * g = argmin |(b - c u_p) - A g|;  (g, u_p) is the full least-squares solution of [A | c] x = b.  3-D grids, GLS only.  Not provided:
 * 2-D meshes, IDW / LS, nonzero Neumann data on the face rows, derivatives of the gradients, the sharded path, dirty-row launches.
 *
 * nin_gls_corner_gradients_device: dev_u_cells [n_fields][n_elems] -> dev_grad [n_fields][nnz_esup][3], the gradient in cell
 *   esup[pos] as seen from the node whose row holds pos, at what is resident NOW (geometry, flags, K).  Optional (NULL: not wanted):
 *   dev_node_values [n_fields][n_points] = u_p (sum_i w_i u_i with the weights of add_neumann = 0, without `+ neumann_ws`);
 *   dev_flux [n_fields][nnz_esup][3] = -K_e g with the resident permeability of cell e = esup[pos], row c computed as
 *   -((K[3c] g[0] + K[3c+1] g[1]) + K[3c+2] g[2]) without contraction; dev_node_gradient [n_fields][n_points][3] = the mean of a
 *   node's corner gradients, summed from 0.0 in row order and divided by their number -- an average for visualisation, not a
 *   projection.  Every entry of every output is written: zeros for the nodes the forward gives the zero row (Dirichlet nodes, no
 *   internal face, too few rows, a singular or non-finite system), u_p included.  The adjoint's kernel in its gradient mode: the
 *   same bins, assembly and Householder QR, factored once per node for all n_fields fields; per field one application of Q^T and
 *   one triangular solve.  Two streaming kernels follow for the flux and the mean.  No atomics: two calls agree bit for bit and a
 *   batch equals its fields one by one.  The first of the backward, tangent, gradient and plan calls on a grid bins the nodes and
 *   allocates the scratch slots (and synchronises `stream`); later calls are asynchronous on `stream`.  NIN_EINVAL for a NULL grid,
 *   dev_u_cells or dev_grad, for n_fields < 1 and for a grid that is not 3-D (answered in this order, before the grid's residency);
 *   otherwise errors as nin_gls_weights_tangent_device (NIN_ENODEVICE; fields without a permeability are refused: only GLS has
 *   such a system).  A refused call writes nothing.  NIN_GLS_ADJ_FORCE_GLOBAL and NIN_GLS_ADJ_ONLY as there.
 * nin_gls_corner_gradients_host: the host-pointer counterpart -- cell_values [n_fields][n_elems] up, grad and the optional
 *   node_values, flux and node_gradient (NULL: not wanted) down; synchronous.  Errors as the device call. */
int nin_gls_corner_gradients_device(nin_grid *g, int32_t n_fields, const double *dev_u_cells, double *dev_grad, double *dev_node_values,
                                    double *dev_flux, double *dev_node_gradient, void *stream);
int nin_gls_corner_gradients_host(nin_grid *g, const double *cell_values, int32_t n_fields, double *grad, double *node_values, double *flux,
                                  double *node_gradient);

/* ---- the GLS Jacobian in the permeability, kept on the device: linearise once, apply J and J^T many times ----------------------
 * The two calls above repeat the dense QR of every node at every call.  A Krylov solver applies J . dK or J^T . v once per iteration
 * at ONE linearisation point; for it, a nin_gls_jacobian keeps the derivative itself.  For a fixed cell field u (and optional node
 * values b) the node values  F_p(K) = sum_i d_i(K) u[c_i] + neumann_ws_p(K) b_p  (d: the stored weights with add_neumann = 1, the W of
 * nin_apply_*) have the sparse Jacobian
 *   C[pos][k] = dF_p / d perm_e[k], k < 9 (diff_mag held fixed),   C[pos][9] = dF_p / d diff_mag_e
 * with pos the esup position of the pair (p, e) -- exactly what one launch of the adjoint kernel with dev_grad_csr[pos] = u[esup[pos]]
 * and dev_grad_neumann_ws = b leaves in its contribution buffer.  The object owns such a buffer (80 bytes per entry of esup: 6.4 GB at
 * 216^3 hexahedra; NOT the grid's, which the next backward call overwrites) and `fold` [n_elems] = 2 (1 - 3 / tr K_e) 3 / tr K_e^2, the
 * derivative of the table's diff_mag at the linearisation point.  Lifetime as nin_hostmatrix: the object refers to its grid in every
 * call but nin_gls_jacobian_destroy, which may come after nin_grid_destroy.  All dev_* pointers are DEVICE pointers, `stream` a
 * hipStream_t (NULL = default).
 *
 * nin_gls_jacobian_create: the two buffers.  NIN_ENOMEM (nothing is left behind), NIN_ENODEVICE for a grid that is not on a device.
 * nin_gls_jacobian_linearize: dev_u_cells [n_elems], dev_neumann_values [n_points] or NULL (b = 0).  One launch of the adjoint kernel
 *   on every bin (NIN_GLS_ADJ_ONLY is not read: a linearisation is always complete) at what is resident NOW -- geometry, flags, K --
 *   into the object's buffer, and `fold` from the resident K; the cost of one backward call.  Makes the grid's bins if they are not
 *   there, never the grid's own contribution buffer; needs a temporary of 8 bytes per entry of esup and waits for the device when it
 *   frees it.  May be called again on the same object.  Errors as nin_gls_weights_backward_device.
 * nin_gls_jacobian_apply: dev_dnode[t][p] = sum over the row of p of ( sum_k C[pos][k] dev_dperm[t][e][k] + C[pos][9] ddm[t][e] ) for n
 *   directions dev_dperm [n][n_elems][9]; ddm = dev_ddiff_mag [n][n_elems], or with NULL folded: ddm[t][e] = fold[e] tr dperm[t][e].
 *   Every entry of dev_dnode [n][n_points] is written, exact zeros for the nodes the forward gives the zero row.
 * nin_gls_jacobian_apply_transpose: dev_grad_perm[t][e][k] = sum over the nodes p of cell e, ascending node id, of dev_v[t][p]
 *   C[pos][k] for dev_v [n][n_points], and dev_grad_diff_mag [n][n_elems] the same for k = 9; with NULL that sum times fold[e] is
 *   added to the three diagonal entries.  dev_v = 1 gives, bit for bit, what nin_gls_weights_backward_device(g, 1, u[esup], b, ...)
 *   returned at the linearisation point.  Uses the transpose index of nin_spmv_transpose_device (built, with a wait for `stream`,
 *   when it is not there).
 *   Both are single passes over the buffer, read once per four directions; asynchronous on `stream`, deterministic, no atomics: two
 *   calls agree bit for bit, a batch equals its members one by one.  Both read only the object's buffers and the connectivity: a
 *   later update of the permeability, the points or the flags does not change their answers -- the object IS the Jacobian at its
 *   linearisation point.  NIN_ESTATE before the first nin_gls_jacobian_linearize, NIN_EINVAL for n < 1 or a NULL argument.
 * nin_gls_jacobian_contrib: the two device buffers, read-only.  nin_gls_jacobian_stamp: the grid's (nin_grid_field_updates,
 *   nin_grid_geometry_updates, nin_grid_flag_updates) as the last linearisation found them, -1 before it.
 * nin_gls_jacobian_*_host: the same with HOST pointers, synchronous (temporaries on the device per call);
 *   nin_gls_jacobian_fetch_host copies contrib [nnz_esup][10] and fold [n_elems] to the host. */
typedef struct nin_gls_jacobian nin_gls_jacobian;
int nin_gls_jacobian_create(nin_grid *g, nin_gls_jacobian **out);
int nin_gls_jacobian_linearize(nin_gls_jacobian *J, const double *dev_u_cells, const double *dev_neumann_values, void *stream);
int nin_gls_jacobian_apply(nin_gls_jacobian *J, int32_t n, const double *dev_dperm, const double *dev_ddiff_mag, double *dev_dnode,
                           void *stream);
int nin_gls_jacobian_apply_transpose(nin_gls_jacobian *J, int32_t n, const double *dev_v, double *dev_grad_perm,
                                     double *dev_grad_diff_mag, void *stream);
int nin_gls_jacobian_contrib(nin_gls_jacobian *J, const double **dev_contrib, const double **dev_fold);
int nin_gls_jacobian_stamp(const nin_gls_jacobian *J, int64_t stamp[3]);
void nin_gls_jacobian_destroy(nin_gls_jacobian *J);
int nin_gls_jacobian_linearize_host(nin_gls_jacobian *J, const double *u_cells, const double *neumann_values);
int nin_gls_jacobian_apply_host(nin_gls_jacobian *J, int32_t n, const double *dperm, const double *ddiff_mag, double *dnode);
int nin_gls_jacobian_apply_transpose_host(nin_gls_jacobian *J, int32_t n, const double *v, double *grad_perm, double *grad_diff_mag);
int nin_gls_jacobian_fetch_host(nin_gls_jacobian *J, double *contrib, double *fold);

/* ---- the same Jacobian in a reduced parametrisation of K: 8 M bytes per entry of esup instead of 80 -----------------------------
 * A permeability that moves along M parameters per cell,  perm_e = sum_{m < M} theta_(e,m) B_(e,m)  with B_(e,m) a 3 x 3 tensor of 9
 * doubles, row-major like perm: M = 1 (k_r(S(u)) K_abs, a log-multiplier), 3 (principal values in a fixed frame) or 6 (a symmetric
 * tensor).  With C and fold as above the reduced Jacobian is
 *   R[pos][m] = sum_{k < 9} C[pos][k] B_(e,m)[k] + C[pos][9] fold[e] (B_(e,m)[0] + B_(e,m)[4] + B_(e,m)[8]),   e = esup[pos]
 * [nnz_esup][M] doubles, row-major in esup position; the diff_mag chain is always folded (an explicit d diff_mag has no meaning in
 * theta).  The adjoint kernel contracts the ten values of a pair with the cell's basis where it has them: C is never stored and
 * nothing of 80 bytes per entry is allocated.  Lifetime and ownership as nin_gls_jacobian.
 *
 * nin_gls_rjacobian_create: the buffer, 8 n_params bytes per entry of esup.  NIN_EINVAL unless n_params is 1, 3 or 6; NIN_ENOMEM,
 *   NIN_ENODEVICE as nin_gls_jacobian_create.
 * nin_gls_rjacobian_linearize: as nin_gls_jacobian_linearize, with the basis: dev_basis [n_elems][n_params][9] (basis_per_cell != 0),
 *   [n_params][9] shared by every cell (basis_per_cell = 0), or NULL with n_params = 1 (else NIN_EINVAL): the resident perm itself, so
 *   theta is a log-multiplier and dperm = perm dtheta.  The basis is read by this call only.  Every entry of R is written.  May be
 *   called again, with another basis too.
 * nin_gls_rjacobian_apply: dev_dnode[t][p] = sum over the row of p, sum_m R[pos][m] dev_dtheta[t][esup[pos]][m] for n directions
 *   dev_dtheta [n][n_elems][n_params]; every entry of dev_dnode [n][n_points] is written.
 * nin_gls_rjacobian_apply_transpose: dev_grad_theta[t][e][m] = sum over the nodes p of cell e, ascending node id, of dev_v[t][p]
 *   R[pos][m].  Determinism, state, errors and the independence of later updates as for nin_gls_jacobian_apply / _apply_transpose.
 * nin_gls_rjacobian_buffer: the device buffer, read-only, and n_params.  nin_gls_rjacobian_stamp as nin_gls_jacobian_stamp.
 * nin_gls_rjacobian_*_host: the same with HOST pointers, synchronous; nin_gls_rjacobian_fetch_host copies R to the host. */
typedef struct nin_gls_rjacobian nin_gls_rjacobian;
int nin_gls_rjacobian_create(nin_grid *g, int32_t n_params, nin_gls_rjacobian **out);
int nin_gls_rjacobian_linearize(nin_gls_rjacobian *J, const double *dev_u_cells, const double *dev_neumann_values, const double *dev_basis,
                                int32_t basis_per_cell, void *stream);
int nin_gls_rjacobian_apply(nin_gls_rjacobian *J, int32_t n, const double *dev_dtheta, double *dev_dnode, void *stream);
int nin_gls_rjacobian_apply_transpose(nin_gls_rjacobian *J, int32_t n, const double *dev_v, double *dev_grad_theta, void *stream);
int nin_gls_rjacobian_buffer(nin_gls_rjacobian *J, const double **dev_R, int32_t *n_params);
int nin_gls_rjacobian_stamp(const nin_gls_rjacobian *J, int64_t stamp[3]);
void nin_gls_rjacobian_destroy(nin_gls_rjacobian *J);
int nin_gls_rjacobian_linearize_host(nin_gls_rjacobian *J, const double *u_cells, const double *neumann_values, const double *basis,
                                     int32_t basis_per_cell);
int nin_gls_rjacobian_apply_host(nin_gls_rjacobian *J, int32_t n, const double *dtheta, double *dnode);
int nin_gls_rjacobian_apply_transpose_host(nin_gls_rjacobian *J, int32_t n, const double *v, double *grad_theta);
int nin_gls_rjacobian_fetch_host(nin_gls_rjacobian *J, double *R);

/* ---- the GLS Jacobian in the node coordinates, kept on the device: linearise once, apply J . dX and J^T . v many times ------------
 * nin_gls_weights_backward_points_device and nin_gls_weights_tangent_points_device repeat the dense QR of every node at every call.
 * A solver that moves the mesh (ALE, r-adaptivity, Newton-Krylov on a mesh-motion residual, a Gauss-Newton shape fit) applies J . dX
 * or J^T . v once per iteration at ONE linearisation point; for it, a nin_gls_xjacobian keeps the derivative.  For a fixed cell field
 * u (and optional node values b) the node values  F_p(X) = sum_i d_i(X) u[c_i] + neumann_ws_p(X) b_p  (d: the stored weights with
 * add_neumann = 1, the W of nin_apply_*) depend on the coordinates through the centroids of p's cells, the centres and unit normals
 * of its faces and its own position.  One launch of the adjoint kernel's coordinate mode with dev_grad_csr[pos] = u[esup[pos]] and
 * dev_grad_neumann_ws = b leaves the derivative in exactly those inputs, and the object owns them:
 *   cell [nnz_esup][3] = dF_p / d centroid_e,   face [nnz_fsup][6] = (dF_p / d face centre_f, dF_p / d unit normal_f),
 *   own [n_points][3] = dF_p / d x_p through the rows of p's own system
 * (24 nnz_esup + 48 nnz_fsup + 24 n_points bytes: 8.0 GB at 216^3 hexahedra).  The Jacobian is kept FACTORED through the mesh
 * geometry: an apply call takes its direction, or its result, through the chain centroid / face centre / normal <-> vertices with
 * the grid's RESIDENT coordinates and normals.  Hence the one difference from nin_gls_jacobian: an apply call after the coordinates
 * moved (nin_grid_geometry_updates differs from the stamp) is refused with NIN_ESTATE and writes nothing -- linearise again; a snapshot
 * of the geometry would cost about 80 bytes per face, and the solvers above apply at the linearisation point.  Later updates of
 * the permeability or the flags do not change the answers and are not refused.  Lifetime and ownership as nin_gls_jacobian.  Scratch of
 * the applies is the object's too, made by the first call that needs it and kept: 24 bytes per cell and 48 per face per direction of a
 * chunk of nin_gls_xjacobian_apply (up to 4), 24 per cell and 96 per face per field of a chunk of _apply_transpose (up to 2: the
 * faces' point slots are 2.9 GB per field at 216^3).  One apply call at a time per object: the calls share that scratch.  None of
 * the grid's buffers of the two calls above is used or made.  3-D grids.
 *
 * nin_gls_xjacobian_create: the three record buffers.  Errors as nin_gls_jacobian_create.
 * nin_gls_xjacobian_linearize: dev_u_cells [n_elems], dev_neumann_values [n_points] or NULL (b = 0).  One launch of the adjoint kernel's
 *   coordinate mode on every bin (NIN_GLS_ADJ_ONLY is not read) at what is resident NOW; every record is written, zeros for the nodes
 *   the forward gives the zero row.  NIN_EINVAL for a grid that is not 3-D; otherwise as nin_gls_jacobian_linearize.
 * nin_gls_xjacobian_apply: dev_dnode [n][n_points] = J . dev_dpoints [n][n_points][3]; every entry written, exact zeros for zero rows.
 * nin_gls_xjacobian_apply_transpose: dev_grad_points [n][n_points][3] = J^T . dev_v [n][n_points]; dev_v = 1 gives, bit for bit, what
 *   nin_gls_weights_backward_points_device(g, 1, u[esup], b, ...) returned at the linearisation point.  A Dirichlet node receives
 *   gradient as a vertex of its cells and faces.  Uses the transpose index (built, with a wait for `stream`, when it is not there).
 *   Both asynchronous on `stream`, deterministic, no atomics: two calls agree bit for bit, a batch equals its members one by one.
 *   NIN_ESTATE before the first linearisation and after an update of the points, NIN_EINVAL for n < 1 or a NULL argument.
 * nin_gls_xjacobian_records: the three device buffers, read-only, and (scratch_bytes not NULL) the bytes of scratch the object holds.
 * nin_gls_xjacobian_stamp as nin_gls_jacobian_stamp.  nin_gls_xjacobian_*_host: the same with HOST pointers, synchronous;
 *   nin_gls_xjacobian_fetch_host copies the three record buffers to the host. */
typedef struct nin_gls_xjacobian nin_gls_xjacobian;
int nin_gls_xjacobian_create(nin_grid *g, nin_gls_xjacobian **out);
int nin_gls_xjacobian_linearize(nin_gls_xjacobian *J, const double *dev_u_cells, const double *dev_neumann_values, void *stream);
int nin_gls_xjacobian_apply(nin_gls_xjacobian *J, int32_t n, const double *dev_dpoints, double *dev_dnode, void *stream);
int nin_gls_xjacobian_apply_transpose(nin_gls_xjacobian *J, int32_t n, const double *dev_v, double *dev_grad_points, void *stream);
int nin_gls_xjacobian_records(nin_gls_xjacobian *J, const double **dev_cell, const double **dev_face, const double **dev_own,
                              int64_t *scratch_bytes);
int nin_gls_xjacobian_stamp(const nin_gls_xjacobian *J, int64_t stamp[3]);
void nin_gls_xjacobian_destroy(nin_gls_xjacobian *J);
int nin_gls_xjacobian_linearize_host(nin_gls_xjacobian *J, const double *u_cells, const double *neumann_values);
int nin_gls_xjacobian_apply_host(nin_gls_xjacobian *J, int32_t n, const double *dpoints, double *dnode);
int nin_gls_xjacobian_apply_transpose_host(nin_gls_xjacobian *J, int32_t n, const double *v, double *grad_points);
int nin_gls_xjacobian_fetch_host(nin_gls_xjacobian *J, double *cell, double *face, double *own);

/* ---- the same Jacobian assembled: a block-CSR matrix on the device ----------------------------------------------------------------
 * A simulator that assembles a global sparse Jacobian, builds an ILU or AMG preconditioner or calls a direct solver needs the block
 * d(W u + neumann_ws b) / dX as a matrix.  J is [n_points][3 n_points]: row p, column 3 q + c; block (p, q) = dF_p / d x_q, three
 * doubles.  The columns of row p come from the connectivity alone,
 *   C(p) = {p} + the vertices of the cells in esup[p] + the points of the faces in fsup[p],   ascending in q, each once,
 * so the pattern -- block_ptr [n_points + 1] (int64: a large mesh has more than 2^31 blocks), block_col [n_blocks] (int32) -- is made
 * once per object, by the first call below that needs it (one wait for the stream, for the count), and survives linearisations and
 * every update of the grid: a caller can keep a symbolic factorisation.  It counts in nin_gls_xjacobian_records' scratch_bytes
 * (8 (n_points + 1) + 4 n_blocks) from then on.  Rows the forward gives as zero keep their blocks, as exact zeros.
 * The values [n_blocks][3] are assembled per linearisation from the object's records through the RESIDENT coordinates and normals:
 * block (p, q) = own[p] if q == p, + cell[pos(p, e)] / n_e for the cells e of esup[p] that contain q in row order, + for the faces f of
 * fsup[p] with q their point k in row order the slot values 3 k .. 3 k + 2 of the face chain applied to the one record face[pos(p, f)].
 * That order is fixed and depends on the row alone: no atomics, two calls agree bit for bit, every entry is written (no memset).
 *
 * nin_gls_xjacobian_pattern: the object's own device arrays, valid until nin_gls_xjacobian_destroy; needs no linearisation.
 * nin_gls_xjacobian_pattern_copy: the same arrays copied device-to-device into the caller's buffers ([n_points + 1] and [n_blocks]),
 *   asynchronous on `stream` once the pattern exists.
 * nin_gls_xjacobian_assemble: dev_values [n_blocks][3]; asynchronous on `stream` once the pattern exists.  It reads the resident
 *   geometry, so as the apply calls: NIN_ESTATE before the first linearisation and after an update of the points, nothing written;
 *   updates of the permeability or the flags are not refused.
 * nin_gls_xjacobian_pattern_host / _assemble_host: the same with HOST pointers, synchronous; block_col may be NULL to ask for
 *   *n_blocks alone.
 * All refuse a NULL object or a NULL required pointer with NIN_EINVAL; NIN_EINVAL for a grid that is not 3-D. */
int nin_gls_xjacobian_pattern(nin_gls_xjacobian *J, int64_t *n_blocks, const int64_t **dev_block_ptr, const int32_t **dev_block_col,
                              void *stream);
int nin_gls_xjacobian_pattern_copy(nin_gls_xjacobian *J, int64_t *dev_block_ptr_out, int32_t *dev_block_col_out, void *stream);
int nin_gls_xjacobian_assemble(nin_gls_xjacobian *J, double *dev_values, void *stream);
int nin_gls_xjacobian_pattern_host(nin_gls_xjacobian *J, int64_t *block_ptr, int32_t *block_col, int64_t *n_blocks);
int nin_gls_xjacobian_assemble_host(nin_gls_xjacobian *J, double *values);

/* ---- kept Jacobians follow local updates: relinearise only the dirty rows --------------------------------------
 * nin_weights_dirty_device's contract restated for the three kept Jacobians.  PRECONDITION: the object held the Jacobian of
 * W u_old + neumann_ws b_old at the grid's state as of the last clear of the dirty set; u may differ from u_old only in cells all of whose
 * vertices are marked, b from b_old only at marked nodes.  RESULT: the object's buffers equal, byte for byte, what its *_linearize
 * writes now for (u, b).  Rows of nodes outside the set are not touched, whatever u holds there; a row in the set is written whether it
 * is computed or the zero row of a Dirichlet node.  *n_rows (may be NULL): the number of rows recomputed.
 *
 * nin_gls_jacobian_linearize_dirty / nin_gls_rjacobian_linearize_dirty / nin_gls_xjacobian_linearize_dirty: the arguments of the
 *   object's *_linearize (DEVICE pointers; the reduced one reads its basis again, for the listed rows only), then clear and n_rows.  The
 *   marked nodes are binned by the adjoint kernel's bins on the device (ascending node id per bin); the per-bin counts and the
 *   refused-id counter come back in one 32-byte copy -- the ONLY synchronisation of the call (of `stream`); the cotangent
 *   grad_csr[pos] = u[esup[pos]] is written for the listed rows into a buffer the object keeps from its first such call on
 *   (8 bytes per entry of esup); the adjoint kernel runs on the lists, a bin without marked nodes is skipped; nin_gls_jacobian's fold
 *   [n_elems] is recomputed whole.  Beyond the listed rows the work is proportional to n_points and n_elems, never to nnz_esup.
 *   clear != 0: the set is empty afterwards; clear = 0 keeps it: several consumers -- a weights buffer, a nin_hostmatrix, Jacobians --
 *   are served from one grid on one stream, all but the last with clear = 0.  While everything is dirty (nin_grid_dirty_nodes == -1) the
 *   call is the object's full *_linearize (and, with clear, ends that state), *n_rows = n_points.  With an empty set no adjoint kernel
 *   is launched and *n_rows = 0.  In every case the object's stamp becomes the grid's current one: for nin_gls_xjacobian the applies and
 *   nin_gls_xjacobian_assemble answer again after a local move of the points.  If ids were refused since the last dirty launch:
 *   NIN_EINVAL with the count in nin_last_error() (the text of nin_weights_dirty_device), nothing is launched, the set and the object
 *   are kept and the counter starts again from zero.  NIN_ESTATE before the object's first full linearisation.  A NULL object or a NULL
 *   dev_u_cells is NIN_EINVAL.
 * nin_gls_*jacobian_linearize_dirty_host: the same with HOST pointers, on the null stream, synchronous.
 * nin_grid_mark_dirty_device: marks without an update, for a u or b that changed where K, the points and the flags did not.  dev_ids [n]
 *   node ids (int32, or int64 when ids_are_int64 != 0) join the dirty set, or, ids_are_cells != 0, the vertices of those cells.  Every id
 *   is checked on the device before any access: one outside [0, n_points) (resp. [0, n_elems)) marks nothing and is counted in the
 *   counter of the scatters; the next dirty launch reports the count.  Asynchronous on `stream`, no host copy (with cells the first
 *   call on a grid brings the cell -> vertex table to the device and synchronises).  It counts in none of the update counters.  n == 0
 *   is a no-op. */
int nin_gls_jacobian_linearize_dirty(nin_gls_jacobian *J, const double *dev_u_cells, const double *dev_neumann_values, void *stream, int clear,
                                     int64_t *n_rows);
int nin_gls_rjacobian_linearize_dirty(nin_gls_rjacobian *J, const double *dev_u_cells, const double *dev_neumann_values, const double *dev_basis,
                                      int32_t basis_per_cell, void *stream, int clear, int64_t *n_rows);
int nin_gls_xjacobian_linearize_dirty(nin_gls_xjacobian *J, const double *dev_u_cells, const double *dev_neumann_values, void *stream, int clear,
                                      int64_t *n_rows);
int nin_gls_jacobian_linearize_dirty_host(nin_gls_jacobian *J, const double *u_cells, const double *neumann_values, int clear, int64_t *n_rows);
int nin_gls_rjacobian_linearize_dirty_host(nin_gls_rjacobian *J, const double *u_cells, const double *neumann_values, const double *basis,
                                           int32_t basis_per_cell, int clear, int64_t *n_rows);
int nin_gls_xjacobian_linearize_dirty_host(nin_gls_xjacobian *J, const double *u_cells, const double *neumann_values, int clear, int64_t *n_rows);
int nin_grid_mark_dirty_device(nin_grid *g, const void *dev_ids, int ids_are_int64, int64_t n, int ids_are_cells, void *stream);

/* ---- the corner-gradient operator, kept on the device: factorise once, apply G . u and G^T . v many times ----------
 * nin_gls_corner_gradients_device assembles and factorises every node at every call.  The map u -> g is linear and depends on the
 * points, the permeability and the Neumann flags alone: in a time loop or a Krylov solve on a fixed mesh every call after the first
 * repeats the same factorisation, and the call has no transpose.  A nin_gls_gradop keeps the map.  It is block diagonal over the nodes:
 * node p with ne = esup_ptr[p + 1] - esup_ptr[p] cells cells[0 .. ne) owns G_p [3 ne x ne], stored by columns,
 *   gop[gop_ptr[p] + j * 3 ne + i],   i = 3 * (cell slot) + component,
 * column j = the 3 ne corner gradients of p for the cell field that is 1 on cells[j] and 0 elsewhere -- bit for bit what
 * nin_gls_corner_gradients_device writes for such a field.  gop_ptr [n_points + 1] (int64) is the exclusive sum of 3 ne^2, made on the
 * device at creation from the connectivity alone; no update invalidates it.  The buffer takes 24 sum_p ne_p^2 bytes (15.4 GB at 216^3
 * hexahedra): ask nin_gls_gradop_bytes before creating one.  A node the forward gives the zero row has zeros in every entry of its
 * block; every entry is written by a factorisation (no memset, no atomics).  The face rows of the right-hand side are zero, as there.
 * The operator depends on all three inputs, so a product after ANY of nin_grid_field_updates, nin_grid_geometry_updates or
 * nin_grid_flag_updates moved from the stamp is refused with NIN_ESTATE and writes nothing; nin_gls_gradop_factorize answers for the new
 * state (whole: following the dirty set is not provided).  Lifetime and ownership as nin_gls_jacobian.  3-D grids, GLS.
 *
 * nin_gls_gradop_bytes: *bytes = the size of gop for this grid (one scan on the device and a wait for it).
 * nin_gls_gradop_create: gop_ptr, the node of every esup position (4 bytes per entry) and gop.  NIN_EINVAL for a NULL argument or a
 *   grid that is not 3-D (both before the residency is looked at), NIN_ENODEVICE for a grid that is not on a device, NIN_ENOMEM.
 * nin_gls_gradop_factorize: one launch of the adjoint kernel's gradient mode on every bin (NIN_GLS_ADJ_ONLY is not read) with the unit
 *   columns as its fields, at what is resident NOW; asynchronous on `stream` after the first derivative call on a grid (which makes the
 *   bins and synchronises).  Errors as nin_gls_corner_gradients_device.
 * nin_gls_gradop_apply: dev_grad [n][nnz_esup][3] = G . dev_u [n][n_elems]: per entry the sum over the node's cells j ascending, from
 *   0.0, each product rounded and then added; up to four fields share a pass over gop.  dev_flux [n][nnz_esup][3] and
 *   dev_node_gradient [n][n_points][3] (either may be NULL) as nin_gls_corner_gradients_device derives them from dev_grad.
 * nin_gls_gradop_apply_transpose: dev_ubar [n][n_elems] = G^T . dev_gbar [n][nnz_esup][3]: per (node, cell) pair the product of its
 *   column with the node's slice of gbar, i ascending from 0.0, then per cell the sum of its pairs in ascending node id (the
 *   transpose index, built, with a wait for `stream`, when it is not there).  The per-pair products are the object's scratch.
 *   Both asynchronous on `stream`, deterministic: two calls agree bit for bit, a batch equals its members one by one.  Refusals in this
 *   order: NIN_EINVAL for a NULL argument, for n < 1, for a grid that is not 3-D; NIN_ENODEVICE; NIN_ESTATE before the first
 *   factorisation and after an update of the permeability, the points or the flags.
 * nin_gls_gradop_records: the object's device arrays, read-only, the number of doubles in gop and (scratch_bytes not NULL) the bytes the
 *   object holds beside gop.  nin_gls_gradop_stamp as nin_gls_jacobian_stamp.
 * nin_gls_gradop_*_host: the same with HOST pointers, on the null stream, synchronous; nin_gls_gradop_fetch_host copies gop_ptr
 *   [n_points + 1] and gop [gop_ptr[n_points]] to the host (gop NULL: gop_ptr alone, which needs no factorisation). */
typedef struct nin_gls_gradop nin_gls_gradop;
int nin_gls_gradop_bytes(nin_grid *g, int64_t *bytes);
int nin_gls_gradop_create(nin_grid *g, nin_gls_gradop **out);
int nin_gls_gradop_factorize(nin_gls_gradop *op, void *stream);
int nin_gls_gradop_apply(nin_gls_gradop *op, int32_t n, const double *dev_u, double *dev_grad, double *dev_flux, double *dev_node_gradient,
                         void *stream);
int nin_gls_gradop_apply_transpose(nin_gls_gradop *op, int32_t n, const double *dev_gbar, double *dev_ubar, void *stream);
int nin_gls_gradop_records(nin_gls_gradop *op, const int64_t **dev_gop_ptr, const double **dev_gop, int64_t *n_values, int64_t *scratch_bytes);
int nin_gls_gradop_stamp(const nin_gls_gradop *op, int64_t stamp[3]);
void nin_gls_gradop_destroy(nin_gls_gradop *op);
int nin_gls_gradop_factorize_host(nin_gls_gradop *op);
int nin_gls_gradop_apply_host(nin_gls_gradop *op, int32_t n, const double *u, double *grad, double *flux, double *node_gradient);
int nin_gls_gradop_apply_transpose_host(nin_gls_gradop *op, int32_t n, const double *gbar, double *ubar);
int nin_gls_gradop_fetch_host(nin_gls_gradop *op, int64_t *gop_ptr, double *gop);

/* ---- native table packing (replaces the Python loops of interpolator.pyx:255-451, 501-509) ---------------------
 * nin_pack_connectivity: interpolator.pyx:333-361 -- per-type cell blocks (block b: rows[b] x cols[b] int64 node ids,
 *   element type type_id[b]) -> fixed-width, -1 padded connectivity [n_elems][8] + element_types [n_elems].
 * nin_pack_table_row: interpolator.pyx:397-419 -- the first `take` columns of a row-major (n, src_cols) float64 array,
 *   flattened into one row of a (n_vars, n * max_shape) data table.
 * nin_diff_mag: interpolator.pyx:501-509 as compiled (`** (1 / 3)` is `** 0` under cdivision): (1 - 3 / tr K)^2. */
int nin_pack_connectivity(int32_t n_blocks, const int64_t *const *block_data, const int64_t *rows, const int64_t *cols,
                          const int64_t *type_id, int64_t *connectivity, int64_t *element_types);
int nin_pack_table_row(const double *src, int64_t n, int64_t src_cols, int64_t take, double *dst);
int nin_diff_mag(const double *permeability, int64_t n_elems, double *diff_mag);
/* 64-bit hash of ALL bytes of a table, OpenMP-parallel (is the permeability resident on the device still the caller's?
 * the reference re-reads its tables on every call, interpolator.pyx:583-600). */
int nin_hash64(const void *data, size_t bytes, uint64_t *out);

/* Page-locked host memory for the arrays that come back over PCIe (nin_interpolate_csr_host's outputs: 57 GB/s into
 * pinned memory against 10-15 GB/s into pageable memory on the MI355X box).  The reference returns ordinary numpy
 * arrays (interpolator.pyx:622-628); ninpol_amd.Interpolator wraps these buffers as numpy arrays and recycles them. */
int nin_host_alloc(size_t bytes, void **ptr);
int nin_host_free(void *ptr);

/* Give back the scratch a grid keeps between calls: the device buffers nin_interpolate_csr_host / nin_csr_compact_host /
 * nin_apply_* allocate on first use (weights, compacted triplets, counters: ~2.3 GB of HBM at 10 M cells, 8 x that at
 * 80 M), the transpose index of nin_spmv_transpose_device (~0.69 GB at 10 M hexahedra), the bins, contribution buffer and scratch slots of nin_gls_weights_backward_device (6.4 GB at 10 M hexahedra), the three buffers of nin_gls_weights_backward_points_device (10.7 GB at 10 M hexahedra), the connectivity copies of nin_grid_update_points* (~1.05 GB at 10 M hexahedra; kept while a grid built on the device still mirrors from them) and the page-locked flag staging buffer.  The next call allocates them again.  (The reference frees its dense
 * weight table when interpolate() returns, interpolator.pyx:650-651.) */
int nin_grid_release_scratch(nin_grid *g);

/* Algorithmic HBM bytes one nin_weights call moves for `method` over all nodes (DESIGN.md formula,
 * SURVEY 8d): used by bench.py for the roofline line. */
int64_t nin_algorithmic_bytes(const nin_grid *g, int method);

/* Name of the dominant kernel of `method` as it appears in rocprofv3 traces. */
const char *nin_kernel_name(int method);

/* The GLS launch plan of a grid on the device: how many nodes each kernel takes.  counts[0..4]: the block kernel's
 * size classes (1 / 2 / 4 / 8 wavefronts per node, then the global-scratch class), counts[5]: the cube-node kernel,
 * counts[6], counts[7], counts[8]: the one-wavefront multifrontal kernel -- two-coloured nodes (large / small
 * instantiation) and the general kind, counts[9], counts[10], counts[11]: the one-wavefront dense kernel for small nodes
 * (at most 4 / 8 / 12 cells; in practice the boundary nodes that are computed), counts[12]: the two-lanes-per-node kernel for
 * the nodes inside a boundary face of a hexahedron mesh, counts[13..17]: the wide one-wavefront multifrontal kernel (interior nodes
 * of unstructured meshes: up to 16 fronts + 21 dense cells) by size class of its dense problem -- at most 96 x 40, 112 x 44,
 * 128 x 52, 144 x 60, 160 x 64 (rows x columns), counts[18]: its list of BOUNDARY nodes (computed only when flagged Neumann),
 * counts[19]: the multifrontal kernel whose dense problem lives in global-memory tiles (interior nodes beyond the wide kernel: up to 32 fronts +
 * 40 dense cells, 256 x 121), counts[20]: the wide kernel's SMALL class (interior nodes of 9 .. 14 cells that are not two-coloured: at most
 * 64 x 28), counts[21]: its class (7, 12) -- at most 112 x 48, between 112 x 44 and 128 x 52.  (Diagnostics and tests: the reference has one code path, gls.pyx:138-197,
 * for every node.) */
int nin_gls_plan(const nin_grid *g, int64_t counts[22]);

/* Measurement: the FP64 flops one GLS launch performs, kernel by kernel of the launch plan (numbered as in
 * nin_gls_plan): alg[k] = ALGORITHMIC flops of the formulation kernel k runs on its nodes (fronts + dense rest for the
 * multifrontal kernels, from each node's own descriptor; one dense Householder QR with the last-row identity for the small-node /
 * one-wavefront block / global-scratch kernels), ref[k] = the reference's dense dgels on the same nodes (gls.pyx:420-474),
 * computed[k] = the nodes that are computed at all (Dirichlet boundary nodes and nodes outside the parity set get the zero row).
 * Needs nin_fields_set (the Neumann flags decide which boundary nodes are computed). */
int nin_gls_plan_flops(nin_grid *g, double alg[22], double ref[22], int64_t computed[22]);

/* ---- multi-GPU: the all-gather of the path as direct peer-to-peer writes ------------------------------------------
 * Replaces nothing in the reference (it is single-process); it is the exchange step north_star adds -- "a single allgatherv to
 * reassemble the COO triplets" -- without a collective library: rank r writes its block straight into slot r of every peer's
 * gathered buffer, one device-to-device copy per peer, each on its own stream (an MI355X has one xGMI link to each of its seven
 * peers: seven copies in flight on seven links; a ring all-gather uses one link at a time).  The library does no rendezvous: the
 * caller exchanges the 64-byte handles by its own means (MPI, torch.distributed, a file) and puts a barrier of its own between
 * "every rank's pushes are complete" and "read the gathered buffer".  INTEGRATION.md shows the call sequence.
 *
 *   nin_exchange_create     a gathered buffer of world slots of slot_bytes (rounded up to 256) on `device`
 *   nin_exchange_handle     this rank's 64-byte IPC handle (hipIpcMemHandle_t) -> handle64
 *   nin_exchange_connect    all_handles: world x 64 bytes, rank-major; opens the peers' buffers (once)
 *   nin_exchange_push       bytes from dev_src (device memory of this rank) -> offset `offset` of slot `rank` in EVERY rank's buffer,
 *                           this rank's own included; asynchronous, ordered behind everything enqueued on `stream` so far
 *   nin_exchange_wait_sent  host_wait = 0: `stream` waits for this rank's pushes; 1: the host does
 *   nin_exchange_buffer     this rank's gathered buffer (device pointer): slot r at r * nin_exchange_slot_bytes() */
#define NIN_EXCHANGE_HANDLE_BYTES 64
typedef struct nin_exchange nin_exchange;
int nin_exchange_create(int device, int rank, int world, size_t slot_bytes, nin_exchange **out);
void nin_exchange_destroy(nin_exchange *x);
int nin_exchange_handle(nin_exchange *x, void *handle64);
int nin_exchange_connect(nin_exchange *x, const void *all_handles);
int nin_exchange_push(nin_exchange *x, const void *dev_src, size_t bytes, size_t offset, void *stream);
int nin_exchange_wait_sent(nin_exchange *x, void *stream, int host_wait);
void *nin_exchange_buffer(nin_exchange *x);
size_t nin_exchange_slot_bytes(const nin_exchange *x);

#ifdef __cplusplus
}
#endif
#endif /* NINPOL_AMD_H */
