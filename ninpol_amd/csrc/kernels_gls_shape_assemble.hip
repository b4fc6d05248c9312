// kernels_gls_shape_assemble.hip -- the GLS Jacobian in the node coordinates assembled as a block-CSR matrix, gfx950.
//
// The kept Jacobian (kernels_gls_shape_jacobian.hip) is factored through the mesh geometry: records per (node, cell), per
// (node, face) and per node.  The matrix J [P][3 P] has its entries per (node, vertex): block (p, q) = dF_p / d x_q, three doubles.  So
// the assembly is a sparse product with a column set of its own,
//   C(p) = {p} + the vertices of the cells in esup[p] + the points of the faces in fsup[p],  ascending, each once,
// which depends on the connectivity alone: a symbolic pass once per object, a numeric pass per linearisation.
//
// Symbolic pass, nin_xjac_pattern_kernel<FILL>, one wavefront per row (four rows per workgroup), run twice around an exclusive scan:
// FILL = false counts |C(p)|, FILL = true writes the columns at block_ptr[p].  The row's candidates are the valid ids of 8 ne + 4 nf + 1
// slots (a cube node: 113 of 113, a node of 50 tetrahedra: about 500 of 700).  The columns come out by selection, no sort and no
// dedup: the next column is the smallest candidate above the last one (one pass of the lanes over the candidates, one wave-wide minimum),
// until there is none -- ascending and unique by construction, |C(p)| passes (27 for a cube node).  Fast path: the valid candidates are
// first packed into the wave's kPatternStage ints of LDS (ballot + popcount; their order does not matter to a minimum) and every pass
// reads LDS.  Slow path, for a row with more valid candidates than that, or for every row under the host's testing switch: every pass
// walks the slots in global memory again.  Nothing is capped: the two paths write the same bytes.
//
// Numeric pass, nin_xjac_assemble_kernel: 32 lanes per row, two rows per wavefront, eight per workgroup.  The row's cells, then its
// faces, go through the group's LDS stage in chunks of 32, in row order: lane j of the group puts entry j of the chunk there -- a cell
// as its ids (the inpoel row, -1 behind its end) and its share cbar / n_e, a face as its ids and the twelve slot values of
// shape_face_chain (gls_shape_chain.hpp) applied to the ONE record (fcbar, Nbar) of (p, f), with v1, v2, |n| from the resident
// coordinates and N the resident float32 normal, exactly as nin_xjac_face_kernel takes them.  Then lane c owns column c of the row: it
// walks the chunk's entries in order, tests its q against the 8 or 4 ids (LDS broadcasts) and adds the share or the three slot values of
// its position.  So block (p, q) is  own[p] if q == p,  + the cells of the row that contain q in row order,  + the faces of the row that
// contain q in row order -- the order depends on the row alone, never on the launch shape; no two lanes write one block; no atomics, no
// memset: every one of the row's blocks is written, exact zeros where the records are zero.  A row of more than 32 columns takes the
// walk once per 32 of them (the stage is filled again); a row of any number of cells and faces takes as many chunks as it needs.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>

#include "device_grid.hpp"
#include "gls_shape_chain.hpp"
#include "launch.hpp"
#include "wave_ops.hpp"

namespace nin {

namespace {

using namespace waveops;

constexpr int kPatternStage = 1024;   // valid candidates of a row the symbolic pass holds in LDS (ints per wavefront)

// the points of an inpoel ([8]) or inpofa ([4]) row: it ends at the first -1 (the builders checked every index)
template <int N>
__device__ __forceinline__ int row_len(const int32_t (&q)[N], int32_t n_points) {
    int n = 0;
    while (n < N && q[n] >= 0 && q[n] < n_points) ++n;
    return n;
}

// the minimum over the 64 lanes, in every lane (all 64 lanes active)
__device__ __forceinline__ int wave_min(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true));   // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true));   // row_mirror -> every lane holds its 16-lane row's
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

template <bool FILL>
__global__ __launch_bounds__(256) void nin_xjac_pattern_kernel(GridView g, const int4 *__restrict__ inpoel, const int4 *__restrict__ inpofa,
                                                              int force_slow, int64_t *__restrict__ count, const int64_t *__restrict__ block_ptr,
                                                              int32_t *__restrict__ block_col) {
    __shared__ int32_t stage[4][kPatternStage];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= g.n_points) return;   // (the whole wavefront)
    const int32_t p = (int32_t)row;
    const int32_t eb = g.esup_ptr[p], ne = g.esup_ptr[p + 1] - eb, fb = g.fsup_ptr[p], nf = g.fsup_ptr[p + 1] - fb;
    const int64_t cell_slots = 8 * (int64_t)ne, slots = cell_slots + 4 * (int64_t)nf + 1;
    // slot i of the row: an id, or -1
    auto slot = [&](int64_t i) -> int32_t {
        if (i >= slots) return -1;
        if (i == slots - 1) return p;
        if (i < cell_slots) {
            const size_t e = (size_t)g.esup[eb + (int32_t)(i >> 3)];
            const int4 a = inpoel[2 * e], b = inpoel[2 * e + 1];
            const int32_t q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            const int k = (int)(i & 7);
            return k < row_len(q, g.n_points) ? q[k] : -1;
        }
        const int64_t j = i - cell_slots;
        const int4 r = inpofa[g.fsup[fb + (int32_t)(j >> 2)]];
        const int32_t q[4] = {r.x, r.y, r.z, r.w};
        const int k = (int)(j & 3);
        return k < row_len(q, g.n_points) ? q[k] : -1;
    };
    // the valid candidates packed into LDS, while they fit
    int32_t *mine = stage[wave];
    int64_t n = 0;
    if (!force_slow) {
        for (int64_t i0 = 0; i0 < slots && n <= kPatternStage; i0 += 64) {
            const int32_t v = slot(i0 + lane);
            const unsigned long long valid = __ballot(v >= 0);
            const int64_t at = n + __popcll(valid & ((1ull << lane) - 1ull));
            if (v >= 0 && at < kPatternStage) mine[at] = v;
            n += __popcll(valid);
        }
    }
    const bool staged = !force_slow && n <= kPatternStage;   // (wave-uniform)
    wave_lds_sync();
    // selection: the smallest candidate above the last column, until there is none
    const int64_t base = FILL ? block_ptr[p] : 0;
    int64_t cols = 0;
    int32_t last = -1, keep = 0;
    for (;;) {
        int m = INT_MAX;
        if (staged) {
            for (int i = lane; i < (int)n; i += 64) {
                const int32_t v = mine[i];
                if (v > last && v < m) m = v;
            }
        } else {
            for (int64_t i = lane; i < slots; i += 64) {
                const int32_t v = slot(i);
                if (v > last && v < m) m = v;
            }
        }
        m = wave_min(m);
        if (m == INT_MAX) break;
        if (FILL) {   // lane (cols mod 64) keeps the column; 64 of them go out as one store
            if (lane == (int)(cols & 63)) keep = m;
            if ((cols & 63) == 63) block_col[base + (cols & ~(int64_t)63) + lane] = keep;
        }
        last = m;
        ++cols;
    }
    if (FILL) {
        if (lane < (int)(cols & 63)) block_col[base + (cols & ~(int64_t)63) + lane] = keep;
    } else if (lane == 0) {
        count[p] = cols;
        if (p == g.n_points - 1) count[p + 1] = 0;   // (the scan's last input: block_ptr[P] is the total)
    }
}

struct AssembleStage {    // of one row's chunk of 32 entries: 4096 bytes
    double val[32 * 12];  // a cell: its share [3] at 3 j; a face: its slot values [4][3] at 12 j
    int32_t id[32 * 8];   // a cell: its ids [8] at 8 j; a face: its ids [4] at 4 j; -1 behind the end of the row
};

__global__ __launch_bounds__(256) void nin_xjac_assemble_kernel(GridView g, const int4 *__restrict__ inpoel, const int4 *__restrict__ inpofa,
                                                               const double *__restrict__ cell_bar, const double *__restrict__ face_bar,
                                                               const double *__restrict__ own_bar, const int64_t *__restrict__ block_ptr,
                                                               const int32_t *__restrict__ block_col, double *__restrict__ values) {
    __shared__ __attribute__((aligned(16))) AssembleStage stage[8];
    const int lane = threadIdx.x & 31, group = threadIdx.x >> 5;
    const int64_t row = (int64_t)blockIdx.x * 8 + group;
    if (row >= g.n_points) return;   // (the whole group; nothing below waits for another group)
    const int32_t p = (int32_t)row;
    AssembleStage &s = stage[group];
    const int32_t eb = g.esup_ptr[p], ne = g.esup_ptr[p + 1] - eb, fb = g.fsup_ptr[p], nf = g.fsup_ptr[p + 1] - fb;
    const int64_t bb = block_ptr[p], nb = block_ptr[p + 1] - bb;
    for (int64_t c0 = 0; c0 < nb; c0 += 32) {   // (a row of more than 32 columns: the walk again for the next 32)
        const bool has = c0 + lane < nb;
        const int32_t q = has ? block_col[bb + c0 + lane] : -2;   // (-2: no id, and not the -1 behind the end of a row)
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        if (q == p) {
            a0 = own_bar[3 * (size_t)p + 0];
            a1 = own_bar[3 * (size_t)p + 1];
            a2 = own_bar[3 * (size_t)p + 2];
        }
        for (int32_t j0 = 0; j0 < ne; j0 += 32) {
            wave_lds_sync();   // (the chunk before has been read)
            if (j0 + lane < ne) {
                const size_t pos = (size_t)eb + (size_t)(j0 + lane);
                const size_t e = (size_t)g.esup[pos];
                const int4 a = inpoel[2 * e], b = inpoel[2 * e + 1];
                const int32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                const int n_e = row_len(v, g.n_points);
                int4 *ids = reinterpret_cast<int4 *>(&s.id[8 * lane]);
                ids[0] = make_int4(0 < n_e ? v[0] : -1, 1 < n_e ? v[1] : -1, 2 < n_e ? v[2] : -1, 3 < n_e ? v[3] : -1);
                ids[1] = make_int4(4 < n_e ? v[4] : -1, 5 < n_e ? v[5] : -1, 6 < n_e ? v[6] : -1, 7 < n_e ? v[7] : -1);
                const double dn = (double)n_e;   // the points of the cell
#pragma unroll
                for (int c = 0; c < 3; ++c) s.val[3 * lane + c] = cell_bar[3 * pos + c] / dn;
            }
            wave_lds_sync();
            const int m = ne - j0 < 32 ? ne - j0 : 32;
            for (int j = 0; j < m; ++j) {
                const int4 a = *reinterpret_cast<const int4 *>(&s.id[8 * j]), b = *reinterpret_cast<const int4 *>(&s.id[8 * j + 4]);
                if (a.x == q || a.y == q || a.z == q || a.w == q || b.x == q || b.y == q || b.z == q || b.w == q) {
                    a0 += s.val[3 * j + 0];
                    a1 += s.val[3 * j + 1];
                    a2 += s.val[3 * j + 2];
                }
            }
        }
        for (int32_t j0 = 0; j0 < nf; j0 += 32) {
            wave_lds_sync();
            if (j0 + lane < nf) {
                const size_t pos = (size_t)fb + (size_t)(j0 + lane);
                const size_t f = (size_t)g.fsup[pos];
                const int4 r = inpofa[f];
                const int32_t v[4] = {r.x, r.y, r.z, r.w};
                const int npofa = row_len(v, g.n_points);
                int4 *ids = reinterpret_cast<int4 *>(&s.id[4 * lane]);
                if (npofa < 3) {   // (no face of a 3-D mesh: nin_xjac_face_kernel gives its points nothing)
                    *ids = make_int4(-1, -1, -1, -1);
                } else {
                    *ids = make_int4(v[0], v[1], v[2], npofa == 4 ? v[3] : -1);
                    const double2 *rec = reinterpret_cast<const double2 *>(face_bar + 6 * pos);
                    const double2 r0 = rec[0], r1 = rec[1], r2 = rec[2];
                    const double acc[6] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y};
                    double x[3][3];
#pragma unroll
                    for (int k = 0; k < 3; ++k)
#pragma unroll
                        for (int c = 0; c < 3; ++c) x[k][c] = g.coords[3 * (size_t)v[k] + c];
                    const double v1[3] = {x[0][0] - x[1][0], x[0][1] - x[1][1], x[0][2] - x[1][2]};
                    const double v2[3] = {x[2][0] - x[1][0], x[2][1] - x[1][1], x[2][2] - x[1][2]};
                    const double nv[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
                    // (no guard on |n| = 0, as in nin_xjac_face_kernel)
                    const double nn = sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
                    const double N[3] = {(double)g.face_normal[3 * f + 0], (double)g.face_normal[3 * f + 1], (double)g.face_normal[3 * f + 2]};
                    shape_face_chain(acc, v1, v2, nn, N, npofa, &s.val[12 * lane]);
                }
            }
            wave_lds_sync();
            const int m = nf - j0 < 32 ? nf - j0 : 32;
            for (int j = 0; j < m; ++j) {
                const int4 a = *reinterpret_cast<const int4 *>(&s.id[4 * j]);
                const int k = a.x == q ? 0 : (a.y == q ? 1 : (a.z == q ? 2 : (a.w == q ? 3 : -1)));
                if (k >= 0) {
                    a0 += s.val[12 * j + 3 * k + 0];
                    a1 += s.val[12 * j + 3 * k + 1];
                    a2 += s.val[12 * j + 3 * k + 2];
                }
            }
        }
        if (has) {
            double *o = values + 3 * (size_t)(bb + c0 + lane);
            o[0] = a0;
            o[1] = a1;
            o[2] = a2;
        }
    }
}

template <bool FILL>
int pattern_pass(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, int force_slow, int64_t *count, const int64_t *block_ptr,
                 int32_t *block_col, hipStream_t stream) {
    if (g.n_points <= 0) return 0;
    hipLaunchKernelGGL(nin_xjac_pattern_kernel<FILL>, blocks_for(g.n_points, 4), dim3(256), 0, stream, g,
                       reinterpret_cast<const int4 *>(inpoel), reinterpret_cast<const int4 *>(inpofa), force_slow, count, block_ptr, block_col);
    return launch_status();
}

}  // namespace

int launch_xjac_pattern_count(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, int force_slow, int64_t *count, hipStream_t stream) {
    return pattern_pass<false>(g, inpoel, inpofa, force_slow, count, nullptr, nullptr, stream);
}

int xjac_pattern_scan(void *tmp, size_t *tmp_bytes, const int64_t *count, int64_t *block_ptr, int32_t n_points, hipStream_t stream) {
    return launch_status(hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, count, block_ptr, (int)(n_points + 1), stream));
}

int launch_xjac_pattern_fill(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, int force_slow, const int64_t *block_ptr,
                             int32_t *block_col, hipStream_t stream) {
    return pattern_pass<true>(g, inpoel, inpofa, force_slow, nullptr, block_ptr, block_col, stream);
}

int launch_xjac_assemble(const GridView &g, const int32_t *inpoel, const int32_t *inpofa, const double *cell_bar, const double *face_bar,
                         const double *own_bar, const int64_t *block_ptr, const int32_t *block_col, double *values, hipStream_t stream) {
    if (g.n_points <= 0) return 0;
    hipLaunchKernelGGL(nin_xjac_assemble_kernel, blocks_for(g.n_points, 8), dim3(256), 0, stream, g,
                       reinterpret_cast<const int4 *>(inpoel), reinterpret_cast<const int4 *>(inpofa), cell_bar, face_bar, own_bar, block_ptr,
                       block_col, values);
    return launch_status();
}

}  // namespace nin
