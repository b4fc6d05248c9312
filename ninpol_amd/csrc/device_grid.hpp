// device_grid.hpp -- the grid as it lives in HBM (internal).
//
// Canonical device layout (DESIGN.md "Data layout in HBM"): all indices int32 (every count of an
// 80 M-cell mesh is < 2^31), flags one byte per node, reals float64 except the face normals, which
// the reference computes in float32 (grid.pyx:732-767) and which are therefore stored as the float32
// values they are.  Everything is structure-of-arrays; rows of esup / fsup are contiguous.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "gls_plan.hpp"

namespace nin {

struct GridView {  // passed to kernels by value
    int32_t n_points, n_elems, n_faces, dim;
    const int32_t *esup_ptr;   // [P+1]
    const int32_t *esup;       // [nnz_e]   cells around node, ascending
    const int32_t *fsup_ptr;   // [P+1]
    const int32_t *fsup;       // [nnz_f]   faces around node, ascending
    const double *coords;      // [P][3]
    const double *centroids;   // [E][3]
    const double *centroids4;  // [E][4] = (x, y, z, 0): one 32-byte record per cell for the IDW / LS gathers (null unless NIN_ROWS_PAD4: measured slower)
    const int32_t *face_cells; // [F][2]    esuf pair, second = -1 on a boundary face
    const double *face_center; // [F][3]
    const float *face_normal;  // [F][3]
    const double *perm;        // [E][9]    row-major 3x3 (may be null until nin_fields_set)
    const double *diff_mag;    // [E]
    const uint8_t *flags;      // [P]       bit0 boundary_points, bit1 neumann flag
};

// LDS bytes a node's system may take in class c and the waves per node the block kernel runs it with
// (16 / 5 / 2 / 1 workgroups per CU); the last class keeps its systems in global-memory scratch.
NIN_HD inline int32_t gls_class_budget(int c) { return c == 0 ? 10240 : c == 1 ? 32768 : c == 2 ? 81920 : c == 3 ? 159744 : 0; }
NIN_HD inline int32_t gls_class_waves(int c) { return c == 0 ? 1 : c == 1 ? 2 : c == 2 ? 4 : c == 3 ? 8 : 1; }
// LDS bytes of one node's system in the block kernel (kernels_gls_block.hip): the work-queue word, (n + 1) columns of odd pitch m | 1,
// the partial-dot buffers (later y and the weight row), the staged cell ids and their column blocks
NIN_HD inline int64_t gls_block_lds_bytes(int64_t ne, int64_t m, int64_t n, int waves) {
    const int64_t doubles = 2 + (n + 1) * (m | 1) + (waves == 1 ? 2 : (waves != 4 ? 2 : 1) * waves) * n + ((ne + 1) >> 1) +
                            ((ne + 7) >> 3);   // + the cells' column blocks (uint8)
    return ((doubles * 8 + 15) / 16) * 16;
}
// Size class of a node with ne cells, nf faces of which nbf on the boundary; *bytes = what it needs there.
NIN_HD inline int gls_node_class(int64_t ne, int64_t nf, int64_t nbf, bool force_global, int64_t *bytes, int64_t *rows,
                                 int64_t *cols) {
    const int64_t m = ne + 3 * (nf - nbf) + nbf, n = 3 * ne + 1;
    int c = kGlsClasses - 1;
    int64_t b = ((((ne + 1) >> 1) + n + m * n) * 8 + 15) / 16 * 16;   // the scratch slot of the wave kernel
    for (int k = 0; k < kGlsClasses - 1 && !force_global && n <= 256; ++k) {
        const int64_t need = gls_block_lds_bytes(ne, m, n, gls_class_waves(k));
        if (need <= gls_class_budget(k)) { c = k; b = need; break; }
    }
    *bytes = b; *rows = m; *cols = n;
    return c;
}

struct DeviceGrid {
    int device = -1;
    GridView v{};
    int64_t nnz_e = 0, nnz_f = 0;
    bool fields_set = false, have_perm = false;
    bool prebuilt = false;  // arrays came from build_grid_on_device(): nin_grid_to_device adopts them, no upload
    std::vector<void *> allocs;  // everything hipMalloc'd, freed together

    // interpolate()'s pipeline (abi_csr.hip, interpolate_chunked): the node range is cut into kE2eChunks pieces at multiples of 64 nodes
    static constexpr int kE2eChunks = 4;
    int32_t chunk_node[kE2eChunks + 1] = {0, 0, 0, 0, 0};
    bool chunkable = false;
    // GLS launch plan: one node list per kernel of gls_plan.hpp, indexed by GlsKernel
    struct GlsList {
        int32_t count = 0;
        int32_t *nodes = nullptr;  // device list (ascending node ids; the cube-node kernel's in locality order inside each piece)
        uint32_t *desc = nullptr;  // [gls_plan_row(k).desc_words * count] descriptor words (the *_desc.hpp of the kernel), null: none
        // every list is ascending, so a piece of the pipeline is a sub-range of it: chunk_off[j] .. chunk_off[j + 1]
        int32_t chunk_off[kE2eChunks + 1] = {};
        // the block kernel's classes (nodes binned by the LDS bytes their least-squares system needs) and the scratch class
        int32_t lds_bytes = 0;     // per node (workgroup)
        int32_t waves = 1;         // wavefronts per node
        int32_t col_slots = 1;     // ceil(max columns / 64)
        int32_t rows_per_lane = 1; // ceil(max rows / 64): the wave kernel of the scratch class
    } plan[kGlsPlanKernels];
    double *mfg_tiles = nullptr;    // [mfg_slots][kMfgSlotDoubles]: kernels_gls_mfg.hip's dense problems, a global-memory slot per resident wavefront
    int32_t mfg_slots = 0;
    const int32_t *noncube_nodes = nullptr;   // every node the cube-node kernel does not take (the fused apply's list kernel)
    int32_t noncube_count = 0;
    bool noncube_nodes_ready = false;
    double *gls_scratch = nullptr;  // global-memory systems for the oversize class
    int64_t gls_scratch_stride = 0; // doubles per wave slot
    int32_t gls_scratch_slots = 0;
    int32_t *gls_queue = nullptr;   // [kGlsQueueInts] the work counters (gls_plan.hpp: kGlsQueue*)
    // buffers of nin_interpolate_csr_host / nin_csr_compact_host, allocated on first use and kept (0.65 + 0.98 GB at
    // 10 M cells; allocating and freeing them cost ~10 ms of every call)
    double *e2e_weights = nullptr, *e2e_nws = nullptr, *e2e_data = nullptr;
    int32_t *e2e_cnt = nullptr, *e2e_ptr = nullptr, *e2e_indices = nullptr;
    void *e2e_tmp = nullptr;
    size_t e2e_tmp_bytes = 0;
    double *apply_weights = nullptr;   // [nnz_e] weights of the last nin_apply_device (allocated on first use)
    // the cell-major index of the esup pattern (the CSC of W's sparsity) for x = W^T v (nin_spmv_transpose_device): built on the
    // device by the first transpose call, released with the scratch.  tr_cell_ptr [E+1]; tr_cell_pos [nnz_e] = the position in esup /
    // csr_data of the pair (p, e); tr_cell_node [nnz_e] = p, ascending within a cell
    int32_t *tr_cell_ptr = nullptr, *tr_cell_pos = nullptr, *tr_cell_node = nullptr;
    // the GLS adjoint (nin_gls_weights_backward_device, kernels_gls_adjoint.hip): the node list of every bin (gls_adjoint.hpp) with the
    // largest slot among its nodes, the contribution buffer [nnz_e][10] (80 bytes per entry of esup: 6.4 GB at 216^3 hexahedra) and the
    // global-scratch bin's slots; built by the first call, kept until nin_grid_release_scratch.  The bins depend on the connectivity
    // alone.  The tangent (nin_gls_weights_tangent_device) shares the bins and the slots; the contribution buffer is the backward call's
    // alone and is made by the first of those.  The kernels take their nodes by a static stride: no work counter, and no line of gls_queue
    struct AdjBin {
        int32_t count = 0;
        int32_t *nodes = nullptr;
        int64_t bytes = 0;
    } adj_bin[4];
    bool adj_ready = false;
    double *adj_contrib = nullptr, *adj_scratch = nullptr;
    int64_t adj_scratch_stride = 0;   // doubles per slot
    int32_t adj_scratch_slots = 0;
    // the adjoint in the node coordinates (nin_gls_weights_backward_points_device): cbar [nnz_e][3], (fcbar, Nbar)
    // [nnz_f][6] and the faces' point slots [F][4][3] -- 24 bytes per entry of esup, 48 per entry of fsup, 96 per face (1.9 + 5.8 + 2.9 GB at 216^3
    // hexahedra); made by the first call, given back with the adjoint's state.  It shares the bins and the scratch slots above
    double *shape_cell = nullptr, *shape_face = nullptr, *shape_slot = nullptr;
    // the tangent in the node coordinates (nin_gls_weights_tangent_points_device): dC [shape_tan_n][E][3] and (dFc, dN)
    // [shape_tan_n][F][6] -- 24 bytes per cell and 48 per face, per direction; grown to the largest n_tangents seen, given back with the
    // adjoint's state.  None of the three buffers above is made by that path
    double *shape_tan_cell = nullptr, *shape_tan_face = nullptr;
    int32_t shape_tan_n = 0;
    // a dirty relinearisation of a kept Jacobian (jacobian_dirty.hip): the adjoint bin of every node as a byte [P], written
    // from the bins' lists above, and what its compaction of the dirty set needs -- the flat list buffer [P], the block histogram and its
    // scan, the scan's temporary, the header [kAdjDirtyHdrInts].  Made by the first such call, given back with the adjoint's state
    uint8_t *adj_node_bin = nullptr;
    int32_t *adj_dirty_lists = nullptr, *adj_dirty_hist = nullptr, *adj_dirty_hdr = nullptr;
    void *adj_dirty_tmp = nullptr;
    size_t adj_dirty_tmp_bytes = 0;
    // what a geometry refresh (nin_grid_update_points*, grid_update.hip) reads next to the coordinates and the one array it writes that
    // no weight kernel reads: inpoel [E][8], etype [E], inpofa [F][4], face areas [F].  Put here by the first update -- handed over by the
    // device builder's mirror, or uploaded from the host arrays -- and given back with the scratch (0.32 + 0.01 + 0.48 + 0.24 GB at 10 M
    // hexahedra); the next update brings them again.  geom_updates counts the updates; ev_geom (hipEvent_t) marks the last one's end.
    int32_t *up_inpoel = nullptr, *up_inpofa = nullptr;
    int8_t *up_etype = nullptr;
    double *up_areas = nullptr;
    bool up_areas_valid = false;   // up_areas holds the mesh's areas (the builder's, or a whole-mesh update's), not just room for them
    int64_t geom_updates = 0;
    void *ev_geom = nullptr;
    int64_t field_updates = 0;   // permeability updates from device memory (nin_fields_set_permeability_device, fields_update.hip)
    // Local permeability updates (fields_scatter.hip).  node_class: the class bytes k_classify wrote, kept ([P]).  The dirty
    // set: dirty [P] (1 = the node's row may have moved since the last clear) and dirty_hdr [kDirtyHdrInts] (launch.hpp), allocated by the
    // first scatter and kept -- they are state, not scratch; all_dirty: everything is (a full nin_fields_set, a full permeability update,
    // the whole mesh's points moved: the marks are not looked at until a dirty launch clears the flag).  A local move of the points
    // (grid_scatter.hip) marks nodes in the same set.  Scratch of a dirty launch, grown on demand, reused across calls and
    // given back with the rest: the flat list buffer [P], the block histogram and its scan, the scan's temporary, the
    // descriptors of the listed nodes.
    const uint8_t *node_class = nullptr;
    uint8_t *dirty = nullptr;
    int32_t *dirty_hdr = nullptr;
    bool all_dirty = true;
    // which of the three scatters (fields_scatter.hip's cells, grid_scatter.hip's nodes, flags_update.hip's flags) ran since the last
    // dirty launch: they share the refused-id counter, and the error that reports it names the ids they can have been
    bool scattered_cells = false, scattered_nodes = false, scattered_flags = false;
    bool scattered_marks = false;   // nin_grid_mark_dirty_device ran too: its ids are cells' or nodes', counted in the same counter
    // Neumann flags from device memory (flags_update.hip): flag_updates counts the updates; flags_host_stale: flag_staging,
    // the host's copy of the resident bytes, is older than the device's (fetched again by whoever reads it)
    int64_t flag_updates = 0;
    bool flags_host_stale = false;
    int32_t *dirty_lists = nullptr, *dirty_hist = nullptr;
    void *dirty_tmp = nullptr;
    size_t dirty_tmp_bytes = 0;
    uint32_t *dirty_desc = nullptr;
    size_t dirty_desc_words = 0;
    uint8_t *flag_staging = nullptr;   // page-locked [n_points]: nin_fields_set packs the node flags here and uploads from it
    void *copy_stream = nullptr, *copy_stream2 = nullptr;   // hipStream_t of the device-to-host copies that run under the kernels
    void *ev_weights = nullptr, *ev_scan = nullptr;   // hipEvent_t: weights written / row pointers scanned
    // The long pole of a GLS launch plan: the few nodes of the global-scratch class (more cells than any in-register / in-LDS kernel
    // holds: ~0.03 % of a Delaunay mesh) take ~2 ms EACH on a wavefront of their own.  They start first, on a stream of their own,
    // and run under the other kernels (abi_plan.hip: gls_side_begin / gls_side_end).
    void *side_stream = nullptr, *ev_fork = nullptr, *ev_join = nullptr;
    bool side_pending = false;
    bool gls_too_large = false;     // some node's system has more rows than the scratch kernel handles (1024)
};

struct HostGrid;
// grid_device.hip: connectivity + geometry built on `device`, left in `d` and mirrored into `h`.
// 0, -1 bad connectivity, -2 memory, -3 HIP (text in *err), -5 a count does not fit int32.
int build_grid_on_device(HostGrid &h, DeviceGrid &d, int device, const int64_t *connectivity,
                         const int64_t *element_types, const double *xyz, int coords_dim, std::string *err);

}  // namespace nin
