// kernels_gls_adjoint.hip -- the GLS weights differentiated with respect to the permeability and to the node coordinates, gfx950.
// DESIGN.md 4.11 has the mathematics, the bins and the layout of this unit; 4.12, 4.14, 4.15, 4.17 and 4.21 the other five modes, 4.22
// the unit-column variant of the last.
//
// nin_gls_adjoint_kernel<TW, LDS, TAN, RED, PTS, GRD, GOP> serves six modes (listed at its static_assert; GRD, the corner gradients of DESIGN.md
// 4.21, differentiates nothing: it solves for the other 3 ne unknowns of the node's system).  They share the head: node header,
// assembly, Householder QR with R kept, y, r, rho and the verdict.  The header, the zero-row rule and the assembly are this unit's OWN
// TEXT of what gls_dense.hpp holds for the forward kernels (read_node, DenseNode::zero_row, cell_rows, internal_face_rows with
// glsmath::face_tau, neumann_face_row): a change there is made here too.  Calling the helpers gives the same bits, but every form tried
// reallocated this kernel's registers and moved one of the del20 timings by ~0.5 %, more than the parent's spread (profiles/r16).
// The steps after the head are inline for the same reason: each was hoisted alone into a function, and one face frame tried at each of
// its two function sites, and every one changes the device code of the instantiations that run it (profiles/r20).
// Determinism: no atomics anywhere.  A thread owns a cell or a face of the node and sums over the node's faces in fsup order, wavefront
// 0 sums in lane order, nin_adjoint_gather_kernel sums a cell's nodes in ascending node id: two calls agree bit for bit.
// Storage: every row of every listed node is written, zeros where the forward has its zero row.  RED: the lane contracts its ten values
// with the cell's basis B [red_m][9] and the 80-byte record is never stored.  PTS: the records of the cells' centroids (contrib [esup
// position][3]), of the faces' centres and normals (pts_face [fsup position][6]) and of the node (pts_own [P][3]) are
// kernels_gls_shape.hip's to take to the vertices; the PTS tangent reads dC [n_tan][E][3] and (dFc, dN) [n_tan][F][6] made there of dX.
#include <hip/hip_runtime.h>

#include "device_grid.hpp"
#include "diff_mag.hpp"
#include "gls_adjoint.hpp"
#include "gls_device_math.hpp"
#include "launch.hpp"
#include "wave_ops.hpp"

namespace nin {

namespace {

using namespace waveops;

// What one launch reads and writes beside the grid: the adjoint's three pointers, or the tangent's.  The reduced adjoint (RED, never
// with TAN) keeps its three words in the tangent's slots, so that the struct -- and with it the kernel arguments of the adjoint and
// tangent instantiations, and their code -- is what it was before RED existed
struct AdjointIo {
    union {
        const double *grad_csr;          // adjoint: dL/d stored weights [nnz_esup]
        const double *tpt_face;          // tangent with PTS: (dFc, dN) of every face [n_tan][F][6]
    };
    const double *grad_nws;              // adjoint: dL/d neumann_ws [P] or null
    double *contrib;                     //          [nnz_esup][10]; RED: the reduced Jacobian R [nnz_esup][red_m]
    union {
        int32_t n_tan;                   // tangent: directions
        int32_t grd_n;                   // GRD: cell fields
        int32_t red_m;                   // RED: parameters per cell
    };
    union {
        const double *tan_perm;          // tangent: dK [n_tan][E][9]
        const double *red_basis;         // RED: B [E][red_m][9] (red_stride = 9 red_m), [red_m][9] (red_stride = 0: shared) or null: g.perm
        const double *tpt_dx;            // tangent with PTS: dX [n_tan][P][3]
        const double *grd_u;             // GRD: the cell fields u [grd_n][E]
    };
    union {
        const double *tan_dm;            // tangent: d diff_mag [n_tan][E] or null (folded from g.perm)
        const double *tpt_cell;          // tangent with PTS: dC of every cell [n_tan][E][3]
        const long long *gop_ptr;        // GOP: where node p's block begins in grd_out [P + 1]
    };
    union {
        double *tan_csr;                 // tangent: d stored weights [n_tan][nnz]
        double *pts_face;                // PTS: (fcbar, Nbar) of every (node, face) pair [nnz_fsup][6]
        double *grd_out;                 // GRD: the corner gradients [grd_n][nnz][3]; GOP: the kept operator [gop_ptr[P]]
    };
    union {
        double *tan_nws;                 // tangent: d neumann_ws [n_tan][P] or null
        double *pts_own;                 // PTS: xbar_own [P][3]
        double *grd_up;                  // GRD: the node values u_p [grd_n][P] or null
    };
    union {
        long long nnz;
        long long red_stride;            // RED: doubles from one cell's basis to the next
    };
};

// d diff_mag of cell e along the direction: given, or (1 - 3 / tr K)^2 differentiated (nin_adjoint_gather_kernel's factor)
__device__ __forceinline__ double tangent_dm(const GridView &g, const double *dK, const double *dm, size_t e) {
    if (dm) return dm[e];
    const double *K = g.perm + 9 * e, *d = dK + 9 * e;
    return diff_mag_fold(K) * ((d[0] + d[4]) + d[8]);
}

// internal face f between cells ca and cb: U = N x T (T from the face centre to the node) and dtau = -ln|U| tau ddm_pick along the
// direction, 0 when the forward's max() takes eta from nobody
__device__ __forceinline__ double tangent_dtau(const GridView &g, size_t f, double xv0, double xv1, double xv2, double N0, double N1, double N2,
                                               size_t ca, size_t cb, const double *dK, const double *dm, double U[3]) {
    const double T0 = xv0 - g.face_center[3 * f + 0], T1 = xv1 - g.face_center[3 * f + 1], T2 = xv2 - g.face_center[3 * f + 2];
    U[0] = N1 * T2 - N2 * T1; U[1] = N2 * T0 - N0 * T2; U[2] = N0 * T1 - N1 * T0;
    const double da = g.diff_mag[ca], db = g.diff_mag[cb];
    if (!(db > da) && !(da > 0.0)) return 0.0;
    const double un = sqrt(U[0] * U[0] + U[1] * U[1] + U[2] * U[2]);
    const double tj = glsmath::face_tau(un, db > da ? db : da);
    return -log(un) * tj * tangent_dm(g, dK, dm, db > da ? cb : ca);
}

// row c of dK_e . N
__device__ __forceinline__ double tangent_kn(const double *dK, size_t e, int c, double N0, double N1, double N2) {
    const double *d = dK + 9 * e + 3 * c;
    return d[0] * N0 + d[1] * N1 + d[2] * N2;
}

// row c of K . v
__device__ __forceinline__ double shape_kn(const double *K, int c, const double v[3]) {
    return K[3 * c + 0] * v[0] + K[3 * c + 1] * v[1] + K[3 * c + 2] * v[2];
}

// internal face f between cells ca and cb along a direction of the coordinates: dT = dx_p - dFc_f and d(tau U) =
// tau dU - eta tau (U.dU) / |U|^2 U with U = N x T, dU = dN x T + N x dT -- the PTS adjoint's Ubar read the other way.  dfn: (dFc, dN)
// of the face, dp: dx_p
__device__ __forceinline__ void shape_face_tangent(const GridView &g, size_t f, double xv0, double xv1, double xv2, const double dp[3],
                                                   const double *dfn, size_t ca, size_t cb, double dT[3], double dtU[3]) {
    const double N[3] = {(double)g.face_normal[3 * f + 0], (double)g.face_normal[3 * f + 1], (double)g.face_normal[3 * f + 2]};
    const double T[3] = {xv0 - g.face_center[3 * f + 0], xv1 - g.face_center[3 * f + 1], xv2 - g.face_center[3 * f + 2]};
    const double U[3] = {N[1] * T[2] - N[2] * T[1], N[2] * T[0] - N[0] * T[2], N[0] * T[1] - N[1] * T[0]};
    const double dN[3] = {dfn[3], dfn[4], dfn[5]};
    dT[0] = dp[0] - dfn[0]; dT[1] = dp[1] - dfn[1]; dT[2] = dp[2] - dfn[2];
    const double dU[3] = {(dN[1] * T[2] - dN[2] * T[1]) + (N[1] * dT[2] - N[2] * dT[1]), (dN[2] * T[0] - dN[0] * T[2]) + (N[2] * dT[0] - N[0] * dT[2]),
                          (dN[0] * T[1] - dN[1] * T[0]) + (N[0] * dT[1] - N[1] * dT[0])};
    const double un2 = U[0] * U[0] + U[1] * U[1] + U[2] * U[2];
    const double da = g.diff_mag[ca], db = g.diff_mag[cb];
    double eta = 0.0;
    eta = da > eta ? da : eta;
    eta = db > eta ? db : eta;
    const double tj = glsmath::face_tau(sqrt(un2), eta);
    const double k = eta != 0.0 ? eta * tj * ((U[0] * dU[0] + U[1] * dU[1]) + U[2] * dU[2]) / un2 : 0.0;
    dtU[0] = tj * dU[0] - k * U[0]; dtU[1] = tj * dU[1] - k * U[1]; dtU[2] = tj * dU[2] - k * U[2];
}

constexpr int JB = 4;  // columns updated together (independent reductions in flight)

// z <- H_k z for the reflector in column k (v_k = 1, v_i = A[i, k] below it; tk = 0: the identity).  A lane touches only its own rows
// of z (i % 64 == lane): no ordering is needed between successive reflectors.
__device__ __forceinline__ void reflect(const double *A, int ld, int m, int k, double tk, double *z, int lane) {
    if (tk == 0.0) return;   // uniform
    const double *col = A + (size_t)k * ld;
    double s = 0.0;
    for (int i = k + lane; i < m; i += 64) s += (i == k ? 1.0 : col[i]) * z[i];
    s = wave_sum(s) * tk;
    for (int i = k + lane; i < m; i += 64) z[i] -= s * (i == k ? 1.0 : col[i]);
}

// x <- R^-1 x for the upper triangle in A's first nc columns, in place, by columns (one wavefront)
template <bool LDS>
__device__ __forceinline__ void back_substitute(const double *A, int ld, int nc, double *x, int lane) {
    for (int k = nc - 1; k >= 0; --k) {
        const double *col = A + (size_t)k * ld;
        const double xk = x[k] / col[k];   // every lane reads the same two words
        wave_sync<LDS>();                  // ... before the owner of x[k] replaces it
        for (int i = lane; i <= k; i += 64) x[i] = i == k ? xk : x[i] - xk * col[i];
        wave_sync<LDS>();
    }
}

template <int TW, bool LDS, bool TAN, bool RED, bool PTS, bool GRD = false, bool GOP = false>
__global__ __launch_bounds__(64 * TW) void nin_gls_adjoint_kernel(GridView g, const int32_t *__restrict__ nodes, int32_t count, int add_neumann,
                                                                 AdjointIo io, double *scratch, long long scratch_stride) {
    // (TAN, RED, PTS): (0, 0, 0) K adjoint, (0, 1, 0) reduced K adjoint, (0, 0, 1) coordinate adjoint, (1, 0, 0) K tangent,
    // (1, 0, 1) coordinate tangent; the other three combinations mean nothing.  GRD, with none
    // of the three: the corner gradients of cell fields.  GOP, with GRD: the fields are the indicators of the node's own
    // cells, one after the other, and column t of the node's block of the kept gradient operator takes the result
    static_assert(!RED || (!TAN && !PTS), "(TAN, RED, PTS) is not one of the five modes: RED goes with neither TAN nor PTS");
    static_assert(!GRD || (!TAN && !RED && !PTS), "GRD is a mode of its own: it goes with none of TAN, RED and PTS");
    static_assert(!GOP || GRD, "GOP is a variant of GRD");
    extern __shared__ double smem[];
    const double *__restrict__ const grad_csr = io.grad_csr, *__restrict__ const grad_nws = io.grad_nws;
    double *__restrict__ const contrib = io.contrib;
    const int tid = threadIdx.x, nthr = 64 * TW;
    const int lane = tid & 63;
    const int wave = ufirst(tid >> 6);
    double *const base = LDS ? smem : scratch + (size_t)blockIdx.x * scratch_stride;

    for (int32_t idx = blockIdx.x; idx < count; idx += gridDim.x) {
        const int32_t p = ufirst(nodes[idx]);
        const int32_t eb = ufirst(g.esup_ptr[p]), ne = ufirst(g.esup_ptr[p + 1]) - eb;
        const int32_t fb = ufirst(g.fsup_ptr[p]), nf = ufirst(g.fsup_ptr[p + 1]) - fb;
        const int fl = ufirst((int)g.flags[p]);
        const bool is_neu = (fl & 2) != 0;

        int n_if = 0;   // internal faces of the node; every wave counts them itself
        for (int f0 = 0; f0 < nf; f0 += 64) {
            const int fi = f0 + lane;
            const bool internal = fi < nf && g.face_cells[2 * (size_t)g.fsup[fb + fi] + 1] >= 0;
            n_if += __popcll(__ballot(internal));
        }
        const int n_bf = nf - n_if;
        const int n = 3 * ne + 1;                              // columns, the last one is c
        const int m = ne + 3 * n_if + (is_neu ? n_bf : 0);     // rows actually populated
        // the forward's zero rows (DenseNode::zero_row, gls_dense.hpp): nothing depends on K there
        if (((fl & 1) && !is_neu) || n_if == 0 || m < n - 1) {
            if constexpr (GOP) {
                double *ob = io.grd_out + io.gop_ptr[p];
                for (int i = tid; i < 3 * ne * ne; i += nthr) ob[i] = 0.0;
            } else if constexpr (GRD) {
                for (int t = 0; t < io.grd_n; ++t) {
                    for (int i = tid; i < 3 * ne; i += nthr) io.grd_out[3 * ((size_t)t * (size_t)io.nnz + (size_t)eb) + i] = 0.0;
                    if (io.grd_up && tid == 0) io.grd_up[(size_t)t * g.n_points + p] = 0.0;
                }
            } else if constexpr (TAN) {
                for (int t = 0; t < io.n_tan; ++t) {
                    for (int i = tid; i < ne; i += nthr) io.tan_csr[(size_t)t * io.nnz + eb + i] = 0.0;
                    if (io.tan_nws && tid == 0) io.tan_nws[(size_t)t * g.n_points + p] = 0.0;
                }
            } else if constexpr (PTS) {
                for (int i = tid; i < 3 * ne; i += nthr) contrib[3 * (size_t)eb + i] = 0.0;
                for (int i = tid; i < 6 * nf; i += nthr) io.pts_face[6 * (size_t)fb + i] = 0.0;
                if (tid < 3) io.pts_own[3 * (size_t)p + tid] = 0.0;
            } else if constexpr (RED) {
                for (int i = tid; i < io.red_m * ne; i += nthr) contrib[(size_t)io.red_m * (size_t)eb + i] = 0.0;
            } else {
                for (int i = tid; i < 10 * ne; i += nthr) contrib[10 * (size_t)eb + i] = 0.0;
            }
            continue;
        }
        const int ld = m;
        // the slot: A [ld * n] | tau [n] | y [n] | s [n] | r [m] | q [m] | cells [ne], frow [nf], fia [nf], fib [nf] (int32)
        double *A = base;
        double *tau = A + (size_t)ld * n;
        double *y = tau + n, *sv = y + n, *rv = sv + n, *qv = rv + m;
        int32_t *cells = reinterpret_cast<int32_t *>(qv + m);
        int32_t *frow = cells + ne, *fia = frow + nf, *fib = fia + nf;

        for (int i = tid; i < ne; i += nthr) cells[i] = g.esup[eb + i];
        for (int i = tid; i < ld * n; i += nthr) A[i] = 0.0;
        __syncthreads();
        const double xv0 = g.coords[3 * (size_t)p + 0], xv1 = g.coords[3 * (size_t)p + 1], xv2 = g.coords[3 * (size_t)p + 2];
        if (wave == 0) {   // assembly, the text of gls_dense.hpp's helpers: a lane per cell / face
            for (int i = lane; i < ne; i += 64) {
                const size_t c = (size_t)cells[i];
                A[i + (size_t)(3 * i + 0) * ld] = g.centroids[3 * c + 0] - xv0;
                A[i + (size_t)(3 * i + 1) * ld] = g.centroids[3 * c + 1] - xv1;
                A[i + (size_t)(3 * i + 2) * ld] = g.centroids[3 * c + 2] - xv2;
                A[i + (size_t)(n - 1) * ld] = 1.0;
            }
            int if_base = 0, bf_base = 0;
            for (int f0 = 0; f0 < nf; f0 += 64) {
                const int fi = f0 + lane;
                const bool valid = fi < nf;
                const size_t f = valid ? (size_t)g.fsup[fb + fi] : 0;
                const int ca = valid ? g.face_cells[2 * f] : 0, cb = valid ? g.face_cells[2 * f + 1] : -1;
                const bool internal = valid && cb >= 0;
                const bool bface = valid && cb < 0;
                const unsigned long long mi = __ballot(internal), mb = __ballot(bface);
                const unsigned long long below = (1ull << lane) - 1ull;
                int Ia = 0, Ib = 0;
                if (valid)
                    for (int q = 0; q < ne; ++q) {
                        const int cq = cells[q];
                        Ia = cq == ca ? q : Ia;
                        Ib = cq == cb ? q : Ib;
                    }
                if (internal) {
                    const int row = ne + 3 * (if_base + __popcll(mi & below));
                    const double N0 = g.face_normal[3 * f + 0], N1 = g.face_normal[3 * f + 1], N2 = g.face_normal[3 * f + 2];
                    const double T0 = xv0 - g.face_center[3 * f + 0], T1 = xv1 - g.face_center[3 * f + 1],
                                 T2 = xv2 - g.face_center[3 * f + 2];
                    const double U0 = N1 * T2 - N2 * T1, U1 = N2 * T0 - N0 * T2, U2 = N0 * T1 - N1 * T0;
                    const double da = g.diff_mag[ca], db = g.diff_mag[cb];
                    double eta = 0.0;
                    eta = da > eta ? da : eta;
                    eta = db > eta ? db : eta;
                    const double tj = glsmath::face_tau(sqrt(U0 * U0 + U1 * U1 + U2 * U2), eta);
                    const double *Ka = g.perm + 9 * (size_t)ca, *Kb = g.perm + 9 * (size_t)cb;
                    double *ra = A + row + (size_t)(3 * Ia) * ld, *rb = A + row + (size_t)(3 * Ib) * ld;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double nLa = Ka[c * 3 + 0] * N0 + Ka[c * 3 + 1] * N1 + Ka[c * 3 + 2] * N2;  // row c of K . N
                        const double nLb = Kb[c * 3 + 0] * N0 + Kb[c * 3 + 1] * N1 + Kb[c * 3 + 2] * N2;
                        const double t1 = c == 0 ? T0 : (c == 1 ? T1 : T2);
                        const double u = tj * (c == 0 ? U0 : (c == 1 ? U1 : U2));
                        ra[(size_t)c * ld + 0] = -nLa; rb[(size_t)c * ld + 0] = nLb;
                        ra[(size_t)c * ld + 1] = -t1;  rb[(size_t)c * ld + 1] = t1;
                        ra[(size_t)c * ld + 2] = -u;   rb[(size_t)c * ld + 2] = u;
                    }
                    frow[fi] = row; fia[fi] = Ia; fib[fi] = Ib;
                } else if (bface && is_neu) {
                    const int row = ne + 3 * n_if + bf_base + __popcll(mb & below);
                    const double N0 = g.face_normal[3 * f + 0], N1 = g.face_normal[3 * f + 1], N2 = g.face_normal[3 * f + 2];
                    const double *Ka = g.perm + 9 * (size_t)ca;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        A[row + (size_t)(3 * Ia + c) * ld] = -(Ka[c * 3 + 0] * N0 + Ka[c * 3 + 1] * N1 + Ka[c * 3 + 2] * N2);
                    frow[fi] = row; fia[fi] = Ia; fib[fi] = -1;
                } else if (valid) {
                    frow[fi] = -1; fia[fi] = Ia; fib[fi] = -1;
                }
                if_base += __popcll(mi);
                bf_base += __popcll(mb);
            }
        }
        __syncthreads();

        // ---- Householder QR of the first n-1 columns, applied to the last one as it goes (kernels_gls.hip); R stays: beta on the
        //      diagonal, row k of the trailing columns above it ----------------------------------------------------------------
        bool singular = false;
        for (int k = 0; k < n - 1; ++k) {
            const double *ck = A + (size_t)k * ld;
            double ss = 0.0;
            for (int r = k + 1 + lane; r < m; r += 64) ss += ck[r] * ck[r];
            ss = wave_sum(ss);
            const double alpha = ck[k];
            double tk = 0.0, sc = 0.0, beta = alpha;
            if (ss != 0.0) {  // dlarfg: beta = -sign(alpha) |(alpha, x)|, tau = (beta-alpha)/beta, v = x/(alpha-beta)
                beta = -copysign(sqrt(alpha * alpha + ss), alpha);
                tk = (beta - alpha) / beta;
                sc = 1.0 / (alpha - beta);
            } else {
                singular = singular || (alpha == 0.0);
            }
            if (tk != 0.0) {
                for (int j0 = k + 1 + JB * wave; j0 < n; j0 += JB * TW) {
                    double s[JB];
                    double *cj[JB];
#pragma unroll
                    for (int jj = 0; jj < JB; ++jj) {
                        s[jj] = 0.0;
                        cj[jj] = A + (size_t)(j0 + jj < n ? j0 + jj : j0) * ld;   // (a column past the end: read j0 again, never written)
                    }
                    for (int r = k + lane; r < m; r += 64) {
                        const double v = r == k ? 1.0 : ck[r] * sc;
#pragma unroll
                        for (int jj = 0; jj < JB; ++jj) s[jj] += v * cj[jj][r];
                    }
#pragma unroll
                    for (int jj = 0; jj < JB; ++jj) s[jj] = wave_sum(s[jj]) * tk;
                    for (int r = k + lane; r < m; r += 64) {
                        const double v = r == k ? 1.0 : ck[r] * sc;
#pragma unroll
                        for (int jj = 0; jj < JB; ++jj)
                            if (j0 + jj < n) cj[jj][r] -= s[jj] * v;
                    }
                }
            }
            __syncthreads();   // every wave has read the pivot column: v_k and beta may replace it (nobody reads column k again before the tail)
            if (wave == 0) {
                double *wk = A + (size_t)k * ld;
                if (tk != 0.0)
                    for (int r = k + 1 + lane; r < m; r += 64) wk[r] *= sc;
                if (lane == 0) { tau[k] = tk; wk[k] = beta; }
            }
        }
        __syncthreads();

        if (wave == 0) {
            const double *ct = A + (size_t)(n - 1) * ld;   // Q^T c
            // rho = |(Q^T c)(n-1:m)|^2;  r = Q [0; (Q^T c)(n-1:m)];  y = R^-1 (Q^T c)(0:n-1)
            double rho = 0.0;
            for (int i = lane; i < m; i += 64) {
                const double z = i >= n - 1 ? ct[i] : 0.0;
                rv[i] = z;
                rho += z * z;
                if (i < n - 1) y[i] = ct[i];
            }
            rho = wave_sum(rho);
            for (int k = n - 2; k >= 0; --k) reflect(A, ld, m, k, tau[k], rv, lane);
            wave_sync<LDS>();
            if constexpr (!GRD) back_substitute<LDS>(A, ld, n - 1, y, lane);   // (GRD solves for every unknown at once and has no use for y)
            // the forward's last zero-row rule: a singular system, or a result that is not finite
            bool ok = !singular && rho > 0.0;
            {
                bool fin = true;
                for (int i = lane; i < ne; i += 64) fin = fin && isfinite(rv[i] / rho);
                ok = ok && __ballot(!fin) == 0ull;
            }
            if constexpr (TAN || GRD) {   // (tau and y hold n words, the reflectors and y n - 1: the last words carry the verdict and rho)
                if (lane == 0) { tau[n - 1] = ok ? 1.0 : 0.0; y[n - 1] = rho; }
            } else {
                // g and rbar (into q)
                double gsum = 0.0;
                for (int i = lane; i < ne; i += 64) gsum += grad_csr[eb + i];
                gsum = wave_sum(gsum);
                const double extra = is_neu ? (add_neumann ? gsum : 0.0) + (grad_nws ? grad_nws[p] : 0.0) : 0.0;
                double gr = 0.0;
                for (int i = lane; i < ne; i += 64) gr += (grad_csr[eb + i] + (i == ne - 1 ? extra : 0.0)) * rv[i];
                gr = wave_sum(gr);
                const double irho = 1.0 / rho, c2 = 2.0 * gr * irho * irho;
                for (int i = lane; i < m; i += 64) {
                    const double gi = i < ne ? grad_csr[eb + i] + (i == ne - 1 ? extra : 0.0) : 0.0;
                    qv[i] = gi * irho - c2 * rv[i];
                }
                // s = R^-1 (Q^T rbar)(0:n-1);  q = Q [0; (Q^T rbar)(n-1:m)]
                for (int k = 0; k < n - 1; ++k) reflect(A, ld, m, k, tau[k], qv, lane);
                for (int i = lane; i < n - 1; i += 64) { sv[i] = qv[i]; qv[i] = 0.0; }
                for (int k = n - 2; k >= 0; --k) reflect(A, ld, m, k, tau[k], qv, lane);
                wave_sync<LDS>();
                back_substitute<LDS>(A, ld, n - 1, sv, lane);
                if (lane == 0) tau[0] = ok ? 1.0 : 0.0;   // (tau is done with: its first word carries the verdict to the other waves)
            }
        }
        __syncthreads();

        if constexpr (GRD) {
            // ---- the gradient tail: per field b = u on the cell rows and 0 on every face row, u_p = (r.b) / rho,
            //      g = R^-1 (Q^T (b - c u_p))(0:n-1) -- with u_p the full least-squares solution of [A | c] x = b.  Wavefront 0 alone: one
            //      Q^T and one triangular solve per field, in q.  Lane sums in lane order, wave_sum's fixed tree: two calls agree bit for bit.
            //      GOP: field t is the indicator of the node's cell t, the same expressions on 1.0 and 0.0, so column t of
            //      the node's block holds, bit for bit, what the loop writes for a global field that is 1 on that cell alone among the node's
            if (wave == 0) {
                const bool ok = tau[n - 1] != 0.0;   // uniform
                const double rho = y[n - 1];
                for (int t = 0; t < (GOP ? ne : io.grd_n); ++t) {
                    const double *u = GOP ? nullptr : io.grd_u + (size_t)t * (size_t)g.n_elems;
                    double *og = GOP ? io.grd_out + ((size_t)io.gop_ptr[p] + (size_t)t * (size_t)(3 * ne))
                                     : io.grd_out + 3 * ((size_t)t * (size_t)io.nnz + (size_t)eb);
                    double up = 0.0;
                    if (ok) {
                        double s = 0.0;
                        for (int i = lane; i < ne; i += 64) s += rv[i] * (GOP ? (i == t ? 1.0 : 0.0) : u[cells[i]]);
                        up = wave_sum(s) / rho;
                        for (int i = lane; i < m; i += 64) qv[i] = i < ne ? (GOP ? (i == t ? 1.0 : 0.0) : u[cells[i]]) - up : 0.0;   // (a lane's own rows, as reflect takes them)
                        for (int k = 0; k < n - 1; ++k) reflect(A, ld, m, k, tau[k], qv, lane);
                        wave_sync<LDS>();
                        back_substitute<LDS>(A, ld, n - 1, qv, lane);
                        for (int i = lane; i < 3 * ne; i += 64) og[i] = qv[i];
                    } else {
                        for (int i = lane; i < 3 * ne; i += 64) og[i] = 0.0;
                    }
                    if constexpr (!GOP)
                        if (io.grd_up && lane == 0) io.grd_up[(size_t)t * g.n_points + p] = up;
                    wave_sync<LDS>();   // (q is the next field's)
                }
            }
            __syncthreads();   // (the slot is the next node's)
            continue;
        }

        if constexpr (TAN) {
            // ---- the tangent tail: per direction z1 = dA y (into q), z2 = dA^T r (into s), then wavefront 0 -----------------------
            const bool ok = tau[n - 1] != 0.0;   // uniform: every thread reads the same word
            const double rho = y[n - 1];
            for (int t = 0; t < io.n_tan; ++t) {   // (n_tan is a kernel argument: the barriers below are reached by every wave)
              if constexpr (PTS) {
                // ---- a direction dX of the coordinates: dA from dC of the node's cells, (dFc, dN) of its faces and dx_p
                const double *dC = io.tpt_cell + (size_t)t * 3 * (size_t)g.n_elems;
                const double *dFN = io.tpt_face + (size_t)t * 6 * (size_t)g.n_faces;
                const double *dxp = io.tpt_dx + ((size_t)t * (size_t)g.n_points + (size_t)p) * 3;
                const double dp[3] = {dxp[0], dxp[1], dxp[2]};
                // z1: the cell rows hold dC_e - dx_p; a thread per face fills the face's rows
                for (int i = tid; i < ne; i += nthr) {
                    double z = 0.0;
                    if (ok) {
                        const double *dc = dC + 3 * (size_t)cells[i];
                        z = ((dc[0] - dp[0]) * y[3 * i + 0] + (dc[1] - dp[1]) * y[3 * i + 1]) + (dc[2] - dp[2]) * y[3 * i + 2];
                    }
                    qv[i] = z;
                }
                for (int fi = tid; ok && fi < nf; fi += nthr) {
                    const int row = frow[fi], Ia = fia[fi], Ib = fib[fi];
                    if (row < 0) continue;
                    const size_t f = (size_t)g.fsup[fb + fi];
                    const double *dfn = dFN + 6 * f;
                    const double dN[3] = {dfn[3], dfn[4], dfn[5]};
                    const size_t ca = (size_t)cells[Ia];
                    const double *Ka = g.perm + 9 * ca;
                    double z = 0.0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) z -= shape_kn(Ka, c, dN) * y[3 * Ia + c];
                    if (Ib < 0) { qv[row] = z; continue; }   // a Neumann boundary face: one row
                    const size_t cb = (size_t)cells[Ib];
                    const double *Kb = g.perm + 9 * cb;
                    double dT[3], dtU[3];
                    shape_face_tangent(g, f, xv0, xv1, xv2, dp, dfn, ca, cb, dT, dtU);
                    double zt = 0.0, zu = 0.0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double dy = y[3 * Ib + c] - y[3 * Ia + c];
                        z += shape_kn(Kb, c, dN) * y[3 * Ib + c];
                        zt += dT[c] * dy;
                        zu += dtU[c] * dy;
                    }
                    qv[row] = z; qv[row + 1] = zt; qv[row + 2] = zu;
                }
                // z2: thread i = cell i of the node, the node's faces in fsup order
                for (int i = tid; ok && i < ne; i += nthr) {
                    const size_t e = (size_t)cells[i];
                    const double *dc = dC + 3 * e, *Ke = g.perm + 9 * e;
                    const double ri = rv[i];
                    double z[3] = {(dc[0] - dp[0]) * ri, (dc[1] - dp[1]) * ri, (dc[2] - dp[2]) * ri};
                    for (int fi = 0; fi < nf; ++fi) {
                        const int row = frow[fi], Ia = fia[fi], Ib = fib[fi];
                        if (row < 0 || (Ia != i && Ib != i)) continue;
                        const size_t f = (size_t)g.fsup[fb + fi];
                        const double *dfn = dFN + 6 * f;
                        const double dN[3] = {dfn[3], dfn[4], dfn[5]};
                        const double sign = Ia == i ? -1.0 : 1.0;
                        const double rt = sign * rv[row];
#pragma unroll
                        for (int c = 0; c < 3; ++c) z[c] += shape_kn(Ke, c, dN) * rt;
                        if (Ib < 0) continue;
                        double dT[3], dtU[3];
                        shape_face_tangent(g, f, xv0, xv1, xv2, dp, dfn, (size_t)cells[Ia], (size_t)cells[Ib], dT, dtU);
                        const double r1 = sign * rv[row + 1], r2 = sign * rv[row + 2];
#pragma unroll
                        for (int c = 0; c < 3; ++c) z[c] += r1 * dT[c] + r2 * dtU[c];
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) sv[3 * i + c] = z[c];
                }
              } else {
                const double *dK = io.tan_perm + (size_t)t * 9 * (size_t)g.n_elems;
                const double *dm = io.tan_dm ? io.tan_dm + (size_t)t * (size_t)g.n_elems : nullptr;
                // z1: the cell rows hold no K; a thread per face fills the face's rows
                for (int i = tid; i < ne; i += nthr) qv[i] = 0.0;
                for (int fi = tid; ok && fi < nf; fi += nthr) {
                    const int row = frow[fi], Ia = fia[fi], Ib = fib[fi];
                    if (row < 0) continue;
                    const size_t f = (size_t)g.fsup[fb + fi];
                    const double N0 = g.face_normal[3 * f + 0], N1 = g.face_normal[3 * f + 1], N2 = g.face_normal[3 * f + 2];
                    const size_t ca = (size_t)cells[Ia];
                    double z = 0.0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) z -= tangent_kn(dK, ca, c, N0, N1, N2) * y[3 * Ia + c];
                    if (Ib < 0) { qv[row] = z; continue; }   // a Neumann boundary face: one row
                    const size_t cb = (size_t)cells[Ib];
                    double U[3];
                    const double dtau = tangent_dtau(g, f, xv0, xv1, xv2, N0, N1, N2, ca, cb, dK, dm, U);
                    double zu = 0.0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        z += tangent_kn(dK, cb, c, N0, N1, N2) * y[3 * Ib + c];
                        zu += U[c] * (y[3 * Ib + c] - y[3 * Ia + c]);
                    }
                    qv[row] = z; qv[row + 1] = 0.0; qv[row + 2] = dtau * zu;
                }
                // z2: thread i = cell i of the node, the node's faces in fsup order (the contributions loop read the other way)
                for (int i = tid; ok && i < ne; i += nthr) {
                    double z[3] = {0.0, 0.0, 0.0};
                    for (int fi = 0; fi < nf; ++fi) {
                        const int row = frow[fi], Ia = fia[fi], Ib = fib[fi];
                        if (row < 0 || (Ia != i && Ib != i)) continue;
                        const size_t f = (size_t)g.fsup[fb + fi];
                        const double N0 = g.face_normal[3 * f + 0], N1 = g.face_normal[3 * f + 1], N2 = g.face_normal[3 * f + 2];
                        const double sign = Ia == i ? -1.0 : 1.0;
                        const double rt = rv[row];
#pragma unroll
                        for (int c = 0; c < 3; ++c) z[c] += sign * tangent_kn(dK, (size_t)cells[i], c, N0, N1, N2) * rt;
                        if (Ib < 0) continue;
                        double U[3];
                        const double dtau = tangent_dtau(g, f, xv0, xv1, xv2, N0, N1, N2, (size_t)cells[Ia], (size_t)cells[Ib], dK, dm, U);
                        const double r2 = sign * dtau * rv[row + 2];
#pragma unroll
                        for (int c = 0; c < 3; ++c) z[c] += r2 * U[c];
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) sv[3 * i + c] = z[c];
                }
              }
                __syncthreads();
                if (wave == 0) {
                    double *oc = io.tan_csr + (size_t)t * (size_t)io.nnz + eb;
                    double dnws = 0.0;
                    if (ok) {
                        for (int k = 0; k < n - 1; ++k) reflect(A, ld, m, k, tau[k], qv, lane);   // Q^T z1
                        // x = R^-T z2 by columns of R: x_k = (z2_k - R(0:k, k) . x(0:k)) / R(k, k)
                        for (int k = 0; k < n - 1; ++k) {
                            const double *col = A + (size_t)k * ld;
                            double s = 0.0;
                            for (int i = lane; i < k; i += 64) s += col[i] * sv[i];
                            s = wave_sum(s);
                            if (lane == (k & 63)) sv[k] = (sv[k] - s) / col[k];
                            wave_sync<LDS>();
                        }
                        for (int i = lane; i < n - 1; i += 64) qv[i] = sv[i];
                        wave_sync<LDS>();
                        for (int k = n - 2; k >= 0; --k) reflect(A, ld, m, k, tau[k], qv, lane);   // q = Q [x; (Q^T z1)(n-1:m)] = -dr
                        wave_sync<LDS>();
                        double rq = 0.0;
                        for (int i = lane; i < m; i += 64) rq += rv[i] * qv[i];
                        rq = wave_sum(rq);
                        const double irho = 1.0 / rho, c2 = -2.0 * rq * irho * irho;   // drho / rho^2
                        if (is_neu) dnws = -(qv[ne - 1] * irho) - c2 * rv[ne - 1];
                        const double add = add_neumann ? dnws : 0.0;
                        for (int i = lane; i < ne; i += 64) oc[i] = (-(qv[i] * irho) - c2 * rv[i]) + add;
                    } else {
                        for (int i = lane; i < ne; i += 64) oc[i] = 0.0;
                    }
                    if (io.tan_nws && lane == 0) io.tan_nws[(size_t)t * g.n_points + p] = dnws;
                }
                __syncthreads();   // (q and s are the next direction's, the slot the next node's)
            }
            continue;
        }

        // ---- contributions: thread i = cell i of the node, the node's faces in fsup order ------------------------------------
        const bool ok = tau[0] != 0.0;
        if constexpr (PTS) {
            // ---- the coordinate mode: Abar meets the geometry instead of K.  Thread i = cell i: cbar = Abar(i, 3i:3i+3);
            //      thread fi = face fi of the node: (fcbar, Nbar); then wavefront 0 sums xbar_own = -sum cbar - sum fcbar in a fixed order
            for (int i = tid; i < ne; i += nthr) {
                double *o = contrib + 3 * (size_t)(eb + i);
                const double qi = qv[i], ri = rv[i];
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = ok ? -(qi * y[3 * i + c]) - ri * sv[3 * i + c] : 0.0;
            }
            for (int fi = tid; fi < nf; fi += nthr) {
                double o[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                const int t = frow[fi], Ia = fia[fi], Ib = fib[fi];
                if (ok && t >= 0) {
                    const size_t f = (size_t)g.fsup[fb + fi];
                    const double N[3] = {(double)g.face_normal[3 * f + 0], (double)g.face_normal[3 * f + 1], (double)g.face_normal[3 * f + 2]};
                    const double *Ka = g.perm + 9 * (size_t)cells[Ia];
                    const double qt = qv[t], rt = rv[t];
                    double aA[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) aA[c] = -(qt * y[3 * Ia + c]) - rt * sv[3 * Ia + c];
                    if (Ib < 0) {   // a Neumann boundary face: the row holds -(K_a N)
#pragma unroll
                        for (int j = 0; j < 3; ++j) o[3 + j] = -((Ka[j] * aA[0] + Ka[3 + j] * aA[1]) + Ka[6 + j] * aA[2]);
                    } else {
                        const double *Kb = g.perm + 9 * (size_t)cells[Ib];
                        const double q1 = qv[t + 1], r1 = rv[t + 1], q2 = qv[t + 2], r2 = rv[t + 2];
                        double nb[3], D1[3], D2[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const double ya = y[3 * Ia + c], yb = y[3 * Ib + c], sa = sv[3 * Ia + c], sb = sv[3 * Ib + c];
                            D1[c] = (-(q1 * yb) - r1 * sb) - (-(q1 * ya) - r1 * sa);
                            D2[c] = (-(q2 * yb) - r2 * sb) - (-(q2 * ya) - r2 * sa);
                        }
#pragma unroll
                        for (int j = 0; j < 3; ++j) {   // K_b^T Abar(t, 3Ib:) - K_a^T Abar(t, 3Ia:)
                            const double aB0 = -(qt * y[3 * Ib + 0]) - rt * sv[3 * Ib + 0], aB1 = -(qt * y[3 * Ib + 1]) - rt * sv[3 * Ib + 1],
                                         aB2 = -(qt * y[3 * Ib + 2]) - rt * sv[3 * Ib + 2];
                            nb[j] = ((Kb[j] * aB0 + Kb[3 + j] * aB1) + Kb[6 + j] * aB2) - ((Ka[j] * aA[0] + Ka[3 + j] * aA[1]) + Ka[6 + j] * aA[2]);
                        }
                        const double T[3] = {xv0 - g.face_center[3 * f + 0], xv1 - g.face_center[3 * f + 1], xv2 - g.face_center[3 * f + 2]};
                        const double U[3] = {N[1] * T[2] - N[2] * T[1], N[2] * T[0] - N[0] * T[2], N[0] * T[1] - N[1] * T[0]};
                        const double un2 = U[0] * U[0] + U[1] * U[1] + U[2] * U[2];
                        const double da = g.diff_mag[cells[Ia]], db = g.diff_mag[cells[Ib]];
                        double eta = 0.0;
                        eta = da > eta ? da : eta;
                        eta = db > eta ? db : eta;
                        const double tj = glsmath::face_tau(sqrt(un2), eta);
                        // Ubar = tau D_2 - eta tau (D_2.U) / |U|^2 U:  d(tau U) = tau dU + U dtau,  dtau = -eta tau (U.dU) / |U|^2
                        const double k = eta != 0.0 ? eta * tj * ((D2[0] * U[0] + D2[1] * U[1]) + D2[2] * U[2]) / un2 : 0.0;
                        const double ub[3] = {tj * D2[0] - k * U[0], tj * D2[1] - k * U[1], tj * D2[2] - k * U[2]};
                        // Tbar = D_1 + Ubar x N (fcbar = -Tbar);  Nbar += T x Ubar
                        o[0] = -(D1[0] + (ub[1] * N[2] - ub[2] * N[1]));
                        o[1] = -(D1[1] + (ub[2] * N[0] - ub[0] * N[2]));
                        o[2] = -(D1[2] + (ub[0] * N[1] - ub[1] * N[0]));
                        o[3] = nb[0] + (T[1] * ub[2] - T[2] * ub[1]);
                        o[4] = nb[1] + (T[2] * ub[0] - T[0] * ub[2]);
                        o[5] = nb[2] + (T[0] * ub[1] - T[1] * ub[0]);
                    }
                }
                double *of = io.pts_face + 6 * (size_t)(fb + fi);
#pragma unroll
                for (int c = 0; c < 6; ++c) of[c] = o[c];
            }
            __syncthreads();   // the node's records are written: wavefront 0 reads them back
            if (wave == 0) {
                double a[3] = {0.0, 0.0, 0.0};
                for (int i = lane; i < ne; i += 64)
#pragma unroll
                    for (int c = 0; c < 3; ++c) a[c] -= contrib[3 * (size_t)(eb + i) + c];
                for (int fi = lane; fi < nf; fi += 64)
#pragma unroll
                    for (int c = 0; c < 3; ++c) a[c] -= io.pts_face[6 * (size_t)(fb + fi) + c];
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] = wave_sum(a[c]);
                if (lane < 3) io.pts_own[3 * (size_t)p + lane] = lane == 0 ? a[0] : (lane == 1 ? a[1] : a[2]);
            }
            __syncthreads();   // (the slot is the next node's)
            continue;
        }
        for (int i = tid; i < ne; i += nthr) {
            double kb[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, etab = 0.0;
            for (int fi = 0; ok && fi < nf; ++fi) {
                const int t = frow[fi], Ia = fia[fi], Ib = fib[fi];
                if (t < 0 || (Ia != i && Ib != i)) continue;
                const size_t f = (size_t)g.fsup[fb + fi];
                const double N0 = g.face_normal[3 * f + 0], N1 = g.face_normal[3 * f + 1], N2 = g.face_normal[3 * f + 2];
                // Abar(t, 3 i + c) = -q_t y_(3i+c) - r_t s_(3i+c); on cell a's columns the row holds -(K_a N), on b's +(K_b N)
                const double sign = Ia == i ? -1.0 : 1.0;
                const double qt = qv[t], rt = rv[t];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double ab = sign * (-(qt * y[3 * i + c]) - rt * sv[3 * i + c]);
                    kb[3 * c + 0] += ab * N0;
                    kb[3 * c + 1] += ab * N1;
                    kb[3 * c + 2] += ab * N2;
                }
                if (Ib < 0) continue;   // a Neumann boundary face: no tau row
                const double da = g.diff_mag[cells[Ia]], db = g.diff_mag[cells[Ib]];
                const int pick = db > da ? Ib : (da > 0.0 ? Ia : -1);   // the cell the forward's max() takes eta from
                if (pick != i) continue;
                const double T0 = xv0 - g.face_center[3 * f + 0], T1 = xv1 - g.face_center[3 * f + 1], T2 = xv2 - g.face_center[3 * f + 2];
                const double U0 = N1 * T2 - N2 * T1, U1 = N2 * T0 - N0 * T2, U2 = N0 * T1 - N1 * T0;
                const double un = sqrt(U0 * U0 + U1 * U1 + U2 * U2);
                const double eta = db > da ? db : da;
                const double tj = glsmath::face_tau(un, eta);
                const double q2 = qv[t + 2], r2 = rv[t + 2];
                double dot = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double abb = -(q2 * y[3 * Ib + c]) - r2 * sv[3 * Ib + c], aba = -(q2 * y[3 * Ia + c]) - r2 * sv[3 * Ia + c];
                    dot += (abb - aba) * (c == 0 ? U0 : (c == 1 ? U1 : U2));
                }
                etab += dot * (-log(un) * tj);   // d tau / d eta = -ln|T2| tau
            }
            if constexpr (RED) {
                // the chain rule folded in where the ten values are: R[pos][m] = sum_k kb[k] B_m[k] + etab fold tr B_m,
                // one chain of fmas from 0.0, k ascending, the fold term last; fold is nin_jac_fold_kernel's expression of g.perm
                const double *K = g.perm + 9 * (size_t)cells[i];
                const double fold = diff_mag_fold(K);
                const double *B = io.red_basis ? io.red_basis + (size_t)io.red_stride * (size_t)cells[i] : K;
                double *o = contrib + (size_t)io.red_m * (size_t)(eb + i);
                for (int m = 0; m < io.red_m; ++m) {
                    const double *bm = B + 9 * m;
                    double r = 0.0;
#pragma unroll
                    for (int c = 0; c < 9; ++c) r = fma(kb[c], bm[c], r);
                    o[m] = fma(etab, fold * ((bm[0] + bm[4]) + bm[8]), r);
                }
            } else {
                double *o = contrib + 10 * (size_t)(eb + i);
#pragma unroll
                for (int c = 0; c < 9; ++c) o[c] = kb[c];
                o[9] = etab;
            }
        }
        __syncthreads();   // (the slot is the next node's)
    }
}

// thread p: the bytes of node p's slot (gls_adjoint.hpp), from the node's shape alone -- the Neumann flag may change, the bin may not
__global__ __launch_bounds__(256) void nin_adjoint_bytes_kernel(GridView g, int64_t *__restrict__ bytes) {
    const int32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.n_points) return;
    const int32_t ne = g.esup_ptr[p + 1] - g.esup_ptr[p];
    const int32_t fb = g.fsup_ptr[p], nf = g.fsup_ptr[p + 1] - fb;
    int nbf = 0;
    for (int i = 0; i < nf; ++i) nbf += g.face_cells[2 * (size_t)g.fsup[fb + i] + 1] < 0;
    bytes[p] = adj_node_bytes(ne, nf, nbf);
}

// thread e: cell e sums the slots of its nodes, ascending node id (the order of cell_pos within a cell)
__global__ __launch_bounds__(256) void nin_adjoint_gather_kernel(int32_t n_elems, const int32_t *__restrict__ cell_ptr, const int32_t *__restrict__ cell_pos,
                                                                const double *__restrict__ contrib, const double *__restrict__ perm,
                                                                double *__restrict__ grad_perm, double *__restrict__ grad_dm) {
    const int32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    double acc[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int32_t j = cell_ptr[e]; j < cell_ptr[e + 1]; ++j) {
        const double *c = contrib + 10 * (size_t)cell_pos[j];
#pragma unroll
        for (int k = 0; k < 10; ++k) acc[k] += c[k];
    }
    if (grad_dm) {
        grad_dm[e] = acc[9];
    } else {   // diff_mag = (1 - 3 / tr K)^2 (diff_mag.hpp): d diff_mag / d K_dd = 2 (1 - 3 / tr) 3 / tr^2 on the three diagonal entries
        const double t = acc[9] * diff_mag_fold(perm + 9 * (size_t)e);
        acc[0] += t; acc[4] += t; acc[8] += t;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) grad_perm[9 * (size_t)e + k] = acc[k];
}

template <int TW, bool LDS, bool TAN, bool RED, bool PTS, bool GRD, bool GOP>
int launch_bin(const GridView &g, const int32_t *nodes, int32_t count, int64_t bytes, int add_neumann, const AdjointIo &io, double *scratch,
               int64_t stride, int32_t slots, hipStream_t stream) {
    auto kern = nin_gls_adjoint_kernel<TW, LDS, TAN, RED, PTS, GRD, GOP>;
    int64_t blocks;
    size_t lds = 0;
    if (LDS) {
        lds = (size_t)bytes;
        if (int rc = allow_dynamic_lds<nin_gls_adjoint_kernel<TW, LDS, TAN, RED, PTS, GRD, GOP>>(lds)) return rc;
        int64_t per_cu = (160 * 1024) / (lds < 1024 ? 1024 : (int64_t)lds);
        if (per_cu > 32 / TW) per_cu = 32 / TW;
        if (per_cu < 1) per_cu = 1;
        blocks = 256 * per_cu * 2;
    } else {
        blocks = slots;   // one scratch slot per workgroup
    }
    if (blocks > count) blocks = count;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64 * TW), lds, stream, g, nodes, count, add_neumann, io, scratch, (long long)stride);
    return launch_status();
}

// one bin's nodes through the class of that bin: 1, 2, 4 wavefronts in LDS, 8 over a global-memory slot
template <bool TAN, bool RED, bool PTS = false, bool GRD = false, bool GOP = false>
int launch_bin_of(const GridView &g, int bin, const AdjBinRun &r, int add_neumann, const AdjointIo &io, hipStream_t stream) {
    if (r.count <= 0) return 0;
    switch (bin) {
        case 0: return launch_bin<1, true, TAN, RED, PTS, GRD, GOP>(g, r.nodes, r.count, r.bytes, add_neumann, io, nullptr, 0, 0, stream);
        case 1: return launch_bin<2, true, TAN, RED, PTS, GRD, GOP>(g, r.nodes, r.count, r.bytes, add_neumann, io, nullptr, 0, 0, stream);
        case 2: return launch_bin<4, true, TAN, RED, PTS, GRD, GOP>(g, r.nodes, r.count, r.bytes, add_neumann, io, nullptr, 0, 0, stream);
        case 3:
            if (!r.scratch || r.scratch_slots < 1 || r.scratch_stride * 8 < r.bytes)
                return fail(NIN_EINVAL, "adjoint bin 3 has no scratch slots of %lld bytes", (long long)r.bytes);
            return launch_bin<8, false, TAN, RED, PTS, GRD, GOP>(g, r.nodes, r.count, r.bytes, add_neumann, io, r.scratch, r.scratch_stride, r.scratch_slots,
                                                       stream);
    }
    return fail(NIN_EINVAL, "the adjoint kernel has no bin %d", bin);
}

}  // namespace

int launch_adjoint_bytes(const GridView &g, int64_t *bytes, hipStream_t stream) {
    if (g.n_points <= 0) return 0;
    hipLaunchKernelGGL(nin_adjoint_bytes_kernel, blocks_for(g.n_points), dim3(256), 0, stream, g, bytes);
    return launch_status();
}

int launch_gls_adjoint(const GridView &g, int bin, const AdjBinRun &run, int add_neumann, const double *grad_csr, const double *grad_nws,
                       double *contrib, hipStream_t stream) {
    AdjointIo io{};
    io.grad_csr = grad_csr; io.grad_nws = grad_nws; io.contrib = contrib;
    return launch_bin_of<false, false>(g, bin, run, add_neumann, io, stream);
}

int launch_gls_adjoint_reduced(const GridView &g, int bin, const AdjBinRun &run, int add_neumann, const double *grad_csr,
                               const double *grad_nws, const AdjointReduce &red, double *reduced, hipStream_t stream) {
    AdjointIo io{};
    io.grad_csr = grad_csr; io.grad_nws = grad_nws; io.contrib = reduced;
    io.red_basis = red.basis; io.red_stride = (long long)red.stride; io.red_m = red.n_params;
    return launch_bin_of<false, true>(g, bin, run, add_neumann, io, stream);
}

int launch_gls_adjoint_points(const GridView &g, int bin, const AdjBinRun &run, int add_neumann, const double *grad_csr,
                              const double *grad_nws, double *cell_bar, double *face_bar, double *own_bar, hipStream_t stream) {
    AdjointIo io{};
    io.grad_csr = grad_csr; io.grad_nws = grad_nws; io.contrib = cell_bar; io.pts_face = face_bar; io.pts_own = own_bar;
    return launch_bin_of<false, false, true>(g, bin, run, add_neumann, io, stream);
}

int launch_gls_tangent(const GridView &g, int bin, const AdjBinRun &run, int add_neumann, int32_t n_tangents, const double *tangent_perm,
                       const double *tangent_diff_mag, double *tangent_csr, double *tangent_nws, int64_t nnz, hipStream_t stream) {
    AdjointIo io{};
    io.n_tan = n_tangents; io.tan_perm = tangent_perm; io.tan_dm = tangent_diff_mag; io.tan_csr = tangent_csr; io.tan_nws = tangent_nws;
    io.nnz = (long long)nnz;
    return launch_bin_of<true, false>(g, bin, run, add_neumann, io, stream);
}

int launch_gls_tangent_points(const GridView &g, int bin, const AdjBinRun &run, int add_neumann, int32_t n_tangents, const double *tangent_points,
                              const double *tangent_cell, const double *tangent_face, double *tangent_csr, double *tangent_nws, int64_t nnz,
                              hipStream_t stream) {
    AdjointIo io{};
    io.n_tan = n_tangents; io.tpt_dx = tangent_points; io.tpt_cell = tangent_cell; io.tpt_face = tangent_face; io.tan_csr = tangent_csr;
    io.tan_nws = tangent_nws; io.nnz = (long long)nnz;
    return launch_bin_of<true, false, true>(g, bin, run, add_neumann, io, stream);
}

int launch_gls_corner_gradients(const GridView &g, int bin, const AdjBinRun &run, int32_t n_fields, const double *u_cells, double *grad,
                                double *node_values, int64_t nnz, hipStream_t stream) {
    AdjointIo io{};
    io.grd_n = n_fields; io.grd_u = u_cells; io.grd_out = grad; io.grd_up = node_values; io.nnz = (long long)nnz;
    return launch_bin_of<false, false, false, true>(g, bin, run, 0, io, stream);
}

int launch_gls_gradop_factorize(const GridView &g, int bin, const AdjBinRun &run, const int64_t *gop_ptr, double *gop, hipStream_t stream) {
    static_assert(sizeof(long long) == sizeof(int64_t), "gop_ptr is read as long long");
    AdjointIo io{};
    io.gop_ptr = reinterpret_cast<const long long *>(gop_ptr); io.grd_out = gop;
    return launch_bin_of<false, false, false, true, true>(g, bin, run, 0, io, stream);
}

int launch_adjoint_gather(const GridView &g, const int32_t *cell_ptr, const int32_t *cell_pos, const double *contrib, double *grad_perm,
                          double *grad_diff_mag, hipStream_t stream) {
    if (g.n_elems <= 0) return 0;
    hipLaunchKernelGGL(nin_adjoint_gather_kernel, blocks_for(g.n_elems), dim3(256), 0, stream, g.n_elems, cell_ptr, cell_pos,
                       contrib, g.perm, grad_perm, grad_diff_mag);
    return launch_status();
}

}  // namespace nin
