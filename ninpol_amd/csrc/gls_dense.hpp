// gls_dense.hpp -- the dense GLS system of one node, once: who the node is, whether it gets the zero row, and the rows of the
// reference's m x n matrix (gls.pyx:252-416; the layout is in kernels_gls.hip's header).  Shared by nin_gls_block_kernel
// and nin_gls_team_kernel, so a node gets the same matrix whichever of them its size class runs on (nin_gls_adjoint_kernel keeps its own
// text of the same, see kernels_gls_adjoint.hip).
// Internal, device code only; both units are built with contraction on, and the order of the floating-point expressions
// below is part of their results.
#pragma once
#include <hip/hip_runtime.h>

#include "device_grid.hpp"
#include "wave_ops.hpp"

namespace nin {
namespace glsdense {

struct DenseNode {     // wave-uniform
    int32_t p, eb, ne, fb, nf;   // the node, its rows of esup and fsup
    int fl;
    bool is_neu;
    int n_if, n_bf;    // internal faces (n_esuf == 2, gls.pyx:293-296) and boundary faces of the node
    int n, m;          // columns (3 per cell + c, the last one) and the rows actually populated
    // Dirichlet boundary node (gls.pyx:165-166), n_bface >= n_face (gls.pyx:266-267: the system stays empty and dgels returns an
    // all-zero row n-1), or fewer rows than unknowns next to the node value: the zero row, and nothing depends on K
    __device__ __forceinline__ bool zero_row() const { return ((fl & 1) && !is_neu) || n_if == 0 || m < n - 1; }
};

// Every wave of the workgroup reads the header itself (all 64 lanes active: the faces are counted by ballot).
__device__ __forceinline__ DenseNode read_node(const GridView &g, int32_t node, int lane) {
    using waveops::ufirst;
    DenseNode d;
    d.p = ufirst(node);
    d.eb = ufirst(g.esup_ptr[d.p]); d.ne = ufirst(g.esup_ptr[d.p + 1]) - d.eb;
    d.fb = ufirst(g.fsup_ptr[d.p]); d.nf = ufirst(g.fsup_ptr[d.p + 1]) - d.fb;
    d.fl = ufirst((int)g.flags[d.p]);
    d.is_neu = (d.fl & 2) != 0;
    d.n_if = 0;
    for (int f0 = 0; f0 < d.nf; f0 += 64) {
        const int fi = f0 + lane;
        const bool internal = fi < d.nf && g.face_cells[2 * (size_t)g.fsup[d.fb + fi] + 1] >= 0;
        d.n_if += __popcll(__ballot(internal));
    }
    d.n_bf = d.nf - d.n_if;
    d.n = 3 * d.ne + 1;
    d.m = d.ne + 3 * d.n_if + (d.is_neu ? d.n_bf : 0);
    return d;
}

// The positions of cells ca and cb in the node's esup row (0 for a cell that is not there: cb = -1 of a boundary face)
__device__ __forceinline__ void local_index(const int32_t *cells, int ne, int ca, int cb, int &Ia, int &Ib) {
    Ia = 0; Ib = 0;
    for (int q = 0; q < ne; ++q) {
        const int cq = cells[q];
        Ia = cq == ca ? q : Ia;
        Ib = cq == cb ? q : Ib;
    }
}

// All helpers below store column-major with pitch ld (rows x columns of one node stay far below 2^31 words).

// The row of cell c (gls.pyx:269-281): x_K - x_v on the cell's own column block, 1 in the last column.  `row`: the row's word in
// column 0, cb3: the first column of the cell's block.
__device__ __forceinline__ void cell_row(const GridView &g, size_t c, double xv0, double xv1, double xv2, double *row, int cb3, int n, int ld) {
    row[(cb3 + 0) * ld] = g.centroids[3 * c + 0] - xv0;
    row[(cb3 + 1) * ld] = g.centroids[3 * c + 1] - xv1;
    row[(cb3 + 2) * ld] = g.centroids[3 * c + 2] - xv2;
    row[(n - 1) * ld] = 1.0;
}
// ... of all the node's cells in esup order, a lane per cell: cell i in row i, columns 3 i .. 3 i + 2
__device__ __forceinline__ void cell_rows(const GridView &g, const int32_t *cells, int ne, double xv0, double xv1, double xv2, double *A, int n,
                                          int ld, int lane) {
    for (int i = lane; i < ne; i += 64) cell_row(g, (size_t)cells[i], xv0, xv1, xv2, A + i, 3 * i, n, ld);
}

// The three rows of internal face f between cells ca and cb (gls.pyx:293-356): K N, T1 = x_v - x_f, tau T2 with T2 = N x T1,
// tau = |T2|^(-eta), eta = max diff_mag of the two cells (gls.pyx:304-318); minus on cell a's columns, plus on cell b's.
// ra / rb: the word (row 0, first column of cell a's / b's block); r0, r1, r2: the three rows from there.  `tau(|T2|, eta)` is the
// caller's: the kernels do not all compute the power the same way, and each one's form is part of its results.
template <class Tau>
__device__ __forceinline__ void internal_face_rows(const GridView &g, size_t f, int ca, int cb, double xv0, double xv1, double xv2, double *ra,
                                                   double *rb, int ld, int r0, int r1, int r2, Tau tau) {
    const double N0 = g.face_normal[3 * f + 0], N1 = g.face_normal[3 * f + 1], N2 = g.face_normal[3 * f + 2];
    const double T0 = xv0 - g.face_center[3 * f + 0], T1 = xv1 - g.face_center[3 * f + 1], T2 = xv2 - g.face_center[3 * f + 2];
    const double U0 = N1 * T2 - N2 * T1, U1 = N2 * T0 - N0 * T2, U2 = N0 * T1 - N1 * T0;
    const double da = g.diff_mag[ca], db = g.diff_mag[cb];
    double eta = 0.0;
    eta = da > eta ? da : eta;
    eta = db > eta ? db : eta;
    const double tj = tau(sqrt(U0 * U0 + U1 * U1 + U2 * U2), eta);
    const double *Ka = g.perm + 9 * (size_t)ca, *Kb = g.perm + 9 * (size_t)cb;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double nLa = Ka[c * 3 + 0] * N0 + Ka[c * 3 + 1] * N1 + Ka[c * 3 + 2] * N2;  // row c of K . N
        const double nLb = Kb[c * 3 + 0] * N0 + Kb[c * 3 + 1] * N1 + Kb[c * 3 + 2] * N2;
        const double t1 = c == 0 ? T0 : (c == 1 ? T1 : T2);
        const double u = tj * (c == 0 ? U0 : (c == 1 ? U1 : U2));
        ra[c * ld + r0] = -nLa; rb[c * ld + r0] = nLb;
        ra[c * ld + r1] = -t1;  rb[c * ld + r1] = t1;
        ra[c * ld + r2] = -u;   rb[c * ld + r2] = u;
    }
}

// The row of boundary face f of a Neumann node (set_neumann_rows, gls.pyx:394-416; its RHS column is never read back): -(K N) on the
// owner's columns.  ra: the word (the face's row, first column of the owner's block).
__device__ __forceinline__ void neumann_face_row(const GridView &g, size_t f, int ca, double *ra, int ld) {
    const double N0 = g.face_normal[3 * f + 0], N1 = g.face_normal[3 * f + 1], N2 = g.face_normal[3 * f + 2];
    const double *Ka = g.perm + 9 * (size_t)ca;
#pragma unroll
    for (int c = 0; c < 3; ++c) ra[c * ld] = -(Ka[c * 3 + 0] * N0 + Ka[c * 3 + 1] * N1 + Ka[c * 3 + 2] * N2);
}

}  // namespace glsdense
}  // namespace nin
