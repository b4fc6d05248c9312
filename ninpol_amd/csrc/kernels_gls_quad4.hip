// kernels_gls_quad4.hip -- GLS weights of "quad" nodes (every node inside a boundary face of a hexahedron mesh), gfx950:
// TWO lanes per node, 32 nodes per wavefront -- the cube-node kernel's scheme (kernels_gls_hex8mf.hip) on half a cube.
//
// Such a node has 4 cells, 4 internal and 4 boundary faces, and it is computed only when the variable flags it Neumann
// (gls.pyx:165-166) -- but then a whole boundary plane of them is: 47 k nodes at 216^3, which the one-wavefront kernel for small
// nodes (kernels_gls_mfw.hip, one node per wavefront, 20 of its 64 lanes busy) served at 6.4 ns a node, 0.3 ms per Neumann
// plane against 4.7 ms for the 9.9 M interior nodes.  The system (gls.pyx:252-416): a cell row per cell, three rows per internal
// face [-B_a | +B_b], one Neumann row -(K N) per boundary face on its cell's columns -- 20 x 12 (+ the column c).  The cells
// form a 4-cycle (quad4_desc.hpp): two even cells that share no face, two odd ones, each even cell adjacent to BOTH odd cells.
//   phase 1  lane e eliminates E_e in its front: cell row, 3 + 3 rows of its two internal faces, its Neumann row -- 8 rows x
//            (3 own | 3 + 3 odd | c); three reflectors, the columns through the reflectors' mutual products as in the
//            cube-node kernel; 5 fill rows left (the 3 rows of R are not kept: nothing reads them);
//   phase 2  14 x 6 over the pair: per lane its 5 fill rows, the cell row and the Neumann row of O_e; row-distributed
//            Householder, one DPP stage per reduction, pivot rows dealt round-robin;
//   then     the residual of c, r = Q [0; tail of Q^T c]: the reflectors of phase 2, then of phase 1, applied backwards to the
//            tail; weights r_i / (r . r); neumann_ws = the LAST cell's weight (gls.pyx:470-472).  (Until round 14: back-substitution
//            and r_i = 1 - d_i . y_i -- four digits cancel there where c lies almost in the span of the other columns, a mesh of
//            size 1e3, and y's error cond(A) eps is what is left: up to 35 x the reference's distance from the 80-bit solution,
//            tests/test_gpu_gls_exact.py.  The back-application is backward stable and needs no y at all.)
// Dirichlet nodes of the list (gls.pyx:165-166) get their zero row; a pass without a computed node does nothing else.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "device_grid.hpp"
#include "gls_device_math.hpp"
#include "launch.hpp"
#include "quad4_desc.hpp"

namespace nin {

namespace {

using namespace glsmath;

constexpr int QNPW = 32;         // nodes per wavefront pass (2 lanes each)
constexpr int QR = 7, QC = 7;    // phase 2, per lane: 7 rows x (6 odd columns + c)

__device__ __forceinline__ double pair_sum(double v) { return v + dpp_mov<0xB1>(v); }   // quad_perm [1,0,3,2]
template <int L>
__device__ __forceinline__ double pair_bcast(double v) { return dpp_mov<L | (L << 2) | ((2 + L) << 4) | ((2 + L) << 6)>(v); }

// The panel of an 8-row front (rows 0 = cell row, 1-3 / 4-6 = the two internal faces, 7 = the Neumann row): three Householder
// steps on the own columns; v_k stays in P[k..7][k] (pivot entries included); g[k] the reflectors' scalars
__device__ __forceinline__ void quad_panel(double (&P)[8][3], double (&g)[3]) {
    {
        double ss = 0.0;
#pragma unroll
        for (int r = 1; r < 8; ++r) ss = fma(P[r][0], P[r][0], ss);
        const House h = house_unguarded(P[0][0], ss);
        g[0] = h.g;
        double d1 = h.vp * P[0][1], d2 = h.vp * P[0][2];
#pragma unroll
        for (int r = 1; r < 8; ++r) { d1 = fma(P[r][0], P[r][1], d1); d2 = fma(P[r][0], P[r][2], d2); }
        const double w1 = -(h.g * d1), w2 = -(h.g * d2);
        P[0][0] = h.vp;
#pragma unroll
        for (int r = 0; r < 8; ++r) { P[r][1] = fma(w1, P[r][0], P[r][1]); P[r][2] = fma(w2, P[r][0], P[r][2]); }
    }
    {
        double ss = 0.0;
#pragma unroll
        for (int r = 2; r < 8; ++r) ss = fma(P[r][1], P[r][1], ss);
        const House h = house_unguarded(P[1][1], ss);
        g[1] = h.g;
        double d2 = h.vp * P[1][2];
#pragma unroll
        for (int r = 2; r < 8; ++r) d2 = fma(P[r][1], P[r][2], d2);
        const double w2 = -(h.g * d2);
        P[1][1] = h.vp;
#pragma unroll
        for (int r = 1; r < 8; ++r) P[r][2] = fma(w2, P[r][1], P[r][2]);
    }
    {
        double ss = 0.0;
#pragma unroll
        for (int r = 3; r < 8; ++r) ss = fma(P[r][2], P[r][2], ss);
        const House h = house_unguarded(P[2][2], ss);
        g[2] = h.g;
        P[2][2] = h.vp;
    }
}

// The three reflectors on a column that enters with one face's three entries (rows R0 .. R0 + 2; R0 < 0: the column c = e_0)
// and zeros elsewhere, through the reflectors' mutual products cc = (v1 . v0, v2 . v0, v2 . v1) -- w2_column of
// kernels_gls_hex8mf.hip on 8 rows.  Out: the five fill entries (rows 3 .. 7); rows 0 .. 2, the column's part of R, are needed by
// nobody: the weights come from the residual, which the reflectors give back without R.
template <int R0>
__device__ __forceinline__ void quad_column(const double (&P)[8][3], const double (&g3)[3], const double (&cc)[3], const double (&b)[3],
                                            double (&fill)[5]) {
    double w0, w1, w2;
    if (R0 < 0) {
        w0 = -(g3[0] * P[0][0]);
        w1 = -(g3[1] * (w0 * cc[0]));
        w2 = -(g3[2] * fma(w1, cc[2], w0 * cc[1]));
    } else {
        w0 = -(g3[0] * fma(P[R0 + 2][0], b[2], fma(P[R0 + 1][0], b[1], P[R0][0] * b[0])));
        w1 = -(g3[1] * fma(w0, cc[0], fma(P[R0 + 2][1], b[2], fma(P[R0 + 1][1], b[1], P[R0][1] * b[0]))));
        const double d2 = (R0 >= 2) ? fma(P[R0 + 2][2], b[2], fma(P[R0 + 1][2], b[1], P[R0 < 0 ? 0 : R0][2] * b[0]))
                                    : fma(P[R0 + 2][2], b[2], P[R0 + 1][2] * b[1]);     // (R0 = 1: row 1 lies above v2)
        w2 = -(g3[2] * fma(w1, cc[2], fma(w0, cc[1], d2)));
    }
#pragma unroll
    for (int r = 3; r < 8; ++r) {
        const bool own = R0 >= 0 && r >= R0 && r < R0 + 3;
        const double v = own ? fma(w0, P[r][0], b[own ? r - R0 : 0]) : w0 * P[r][0];
        fill[r - 3] = fma(w2, P[r][2], fma(w1, P[r][1], v));
    }
}

// Phase 2, step K: pivot = local row Q = K / 2 of lane LAM = K % 2 (p2_step_lean of kernels_gls_hex8mf.hip on a pair)
template <int K>
__device__ __forceinline__ void quad_p2_step(double (&C)[QR][QC], double (&gq)[6], double (&vpq)[6], int e) {
    constexpr int Q = K / 2, LAM = K % 2;
    const bool is_piv = (e == LAM);
    const double xq = (e > LAM) ? C[Q][K] : 0.0;
    double ss = xq * xq;
#pragma unroll
    for (int r = Q + 1; r < QR; ++r) ss = fma(C[r][K], C[r][K], ss);
    ss = pair_sum(ss);
    const double alpha = pair_bcast<LAM>(C[Q][K]);
    const House h = house_unguarded(alpha, ss);
    gq[K] = h.g;                                               // (the pair's two lanes hold the same scalars)
    vpq[K] = h.vp;
    const double vq = is_piv ? h.vp : xq;
#pragma unroll
    for (int j = K + 1; j < QC; ++j) {
        double a = vq * C[Q][j];
#pragma unroll
        for (int r = Q + 1; r < QR; ++r) a = fma(C[r][K], C[r][j], a);
        const double w = -(h.g * pair_sum(a));
        C[Q][j] = fma(w, vq, C[Q][j]);
#pragma unroll
        for (int r = Q + 1; r < QR; ++r) C[r][j] = fma(w, C[r][K], C[r][j]);
    }
}
template <int K, int KEND>
struct QuadP2 {
    static __device__ __forceinline__ void run(double (&C)[QR][QC], double (&gq)[6], double (&vpq)[6], int e) {
        quad_p2_step<K>(C, gq, vpq, e);
        QuadP2<K + 1, KEND>::run(C, gq, vpq, e);
    }
};
template <int KEND>
struct QuadP2<KEND, KEND> {
    static __device__ __forceinline__ void run(double (&)[QR][QC], double (&)[6], double (&)[6], int) {}
};
// Reflector K of phase 2 once more, on a vector t over the pair's 14 rows (v_K is still in column K of C: nothing below a pivot is
// written after its step; the pivot entry is vpq[K]); K = 5 first: t <- H_0 .. H_5 t
template <int K>
struct QuadP2Back {
    static __device__ __forceinline__ void run(const double (&C)[QR][QC], const double (&gq)[6], const double (&vpq)[6], double (&t)[QR], int e) {
        constexpr int Q = K / 2, LAM = K % 2;
        const double vq = (e == LAM) ? vpq[K] : (e > LAM) ? C[Q][K] : 0.0;
        double a = vq * t[Q];
#pragma unroll
        for (int r = Q + 1; r < QR; ++r) a = fma(C[r][K], t[r], a);
        const double w = -(gq[K] * pair_sum(a));
        t[Q] = fma(w, vq, t[Q]);
#pragma unroll
        for (int r = Q + 1; r < QR; ++r) t[r] = fma(w, C[r][K], t[r]);
        QuadP2Back<K - 1>::run(C, gq, vpq, t, e);
    }
};
template <>
struct QuadP2Back<-1> {
    static __device__ __forceinline__ void run(const double (&)[QR][QC], const double (&)[6], const double (&)[6], double (&)[QR], int) {}
};

__global__ __launch_bounds__(256) void nin_gls_quad4_kernel(GridView g, const int32_t *__restrict__ nodes,
                                                            const int32_t *__restrict__ desc, int32_t count, int add_neumann,
                                                            double *__restrict__ out, double *__restrict__ nws) {
    __shared__ double wbuf_all[4][QNPW * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = lane & 1, nd = lane >> 1;
    double *const wbuf = wbuf_all[wave];
    const int32_t n_groups = (count + QNPW - 1) / QNPW;
    for (int32_t grp = (int32_t)blockIdx.x * 4 + wave; grp < n_groups; grp += (int32_t)gridDim.x * 4) {
        const int32_t idx = grp * QNPW + nd;
        const bool valid = idx < count;
        const uint32_t sel = (uint32_t)(valid ? idx : count - 1);   // past the end: a clamped (valid) entry, never stored
        const uint32_t p = (uint32_t)nodes[sel], dsc = (uint32_t)desc[2 * (size_t)sel + e];
        const uint32_t fl = g.flags[p];
        const bool is_neu = (fl & 2) != 0;
        const bool computed = !((fl & 1) && !is_neu);              // Dirichlet boundary node: the zero row (gls.pyx:165-166)
        const uint32_t eb = (uint32_t)g.esup_ptr[p], fb = (uint32_t)g.fsup_ptr[p];
        if (!__any(valid && computed)) {                            // (wave-uniform) nothing to compute in this pass
            if (valid) {
                out[eb + 2 * e] = 0.0;
                out[eb + 2 * e + 1] = 0.0;
                if (e == 0) nws[p] = 0.0;
            }
            continue;
        }
        double xv[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) xv[k] = g.coords[3 * (size_t)p + k];
        const uint32_t ce = (uint32_t)g.esup[eb + (dsc & 3)], co = (uint32_t)g.esup[eb + ((dsc >> 2) & 3)];
        const uint32_t cn[2] = {(uint32_t)g.esup[eb + ((dsc >> 18) & 3)], (uint32_t)g.esup[eb + ((dsc >> 20) & 3)]};
        const uint32_t fbe = (uint32_t)g.fsup[fb + ((dsc >> 12) & 7)], fbo = (uint32_t)g.fsup[fb + ((dsc >> 15) & 7)];

        // ---- the front of E_e: rows 0 = cell row, 1 + 3 i + r = row r of face i (A: towards O0, B: towards O1), 7 = its Neumann row
        double P[8][3], de[3], dod[3], nb[2][3][3];   // nb[i][r][t]: row r of face i on the neighbour's columns
        double Ke[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Ke[k] = g.perm[9 * (size_t)ce + k];
        const double dme = g.diff_mag[ce];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            de[t] = g.centroids[3 * (size_t)ce + t] - xv[t];      // gls.pyx:269-277
            dod[t] = g.centroids[3 * (size_t)co + t] - xv[t];
            P[0][t] = de[t];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t w = dsc >> (4 + 4 * i);
            const uint32_t f = (uint32_t)g.fsup[fb + (w & 7)];
            // B = [K N; T1; tau T2] (gls.pyx:293-321), row = [-B_a | +B_b] (gls.pyx:340-356)
            const double N0 = (double)g.face_normal[3 * (size_t)f + 0], N1 = (double)g.face_normal[3 * (size_t)f + 1],
                         N2 = (double)g.face_normal[3 * (size_t)f + 2];
            const double T0 = xv[0] - g.face_center[3 * (size_t)f + 0], T1 = xv[1] - g.face_center[3 * (size_t)f + 1],
                         T2 = xv[2] - g.face_center[3 * (size_t)f + 2];
            const double U0 = N1 * T2 - N2 * T1, U1 = N2 * T0 - N0 * T2, U2 = N0 * T1 - N1 * T0;
            const double dmn = g.diff_mag[cn[i]];
            double eta = 0.0;
            eta = dme > eta ? dme : eta;
            eta = dmn > eta ? dmn : eta;
            const double tj = face_tau_sq(U0 * U0 + U1 * U1 + U2 * U2, eta);
            const double sg = ((w >> 3) & 1) ? -1.0 : 1.0;
            const double *Kn = g.perm + 9 * (size_t)cn[i];
            const double Tv[3] = {sg * T0, sg * T1, sg * T2}, Uv[3] = {sg * (tj * U0), sg * (tj * U1), sg * (tj * U2)};
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                P[1 + 3 * i][t] = sg * (Ke[t * 3 + 0] * N0 + Ke[t * 3 + 1] * N1 + Ke[t * 3 + 2] * N2);
                P[2 + 3 * i][t] = Tv[t];
                P[3 + 3 * i][t] = Uv[t];
                nb[i][0][t] = -sg * (Kn[t * 3 + 0] * N0 + Kn[t * 3 + 1] * N1 + Kn[t * 3 + 2] * N2);
                nb[i][1][t] = -Tv[t];
                nb[i][2][t] = -Uv[t];
            }
        }
        const double mneu = is_neu ? 1.0 : 0.0;                  // (the Neumann rows exist for flagged nodes only, gls.pyx:374-416)
        {
            const double N0 = (double)g.face_normal[3 * (size_t)fbe + 0], N1 = (double)g.face_normal[3 * (size_t)fbe + 1],
                         N2 = (double)g.face_normal[3 * (size_t)fbe + 2];
#pragma unroll
            for (int t = 0; t < 3; ++t) P[7][t] = -mneu * (Ke[t * 3 + 0] * N0 + Ke[t * 3 + 1] * N1 + Ke[t * 3 + 2] * N2);   // gls.pyx:394-416
        }
        double C[QR][QC], g3[3];
        {
            double cc[3];
            quad_panel(P, g3);
            cc[0] = P[1][1] * P[1][0];
            cc[1] = P[2][2] * P[2][0];
            cc[2] = P[2][2] * P[2][1];
#pragma unroll
            for (int r = 2; r < 8; ++r) cc[0] = fma(P[r][1], P[r][0], cc[0]);
#pragma unroll
            for (int r = 3; r < 8; ++r) { cc[1] = fma(P[r][2], P[r][0], cc[1]); cc[2] = fma(P[r][2], P[r][1], cc[2]); }
            {
                const double none[3] = {0.0, 0.0, 0.0};
                double fill[5];
                quad_column<-1>(P, g3, cc, none, fill);   // c = e_0 on entry
#pragma unroll
                for (int r = 0; r < 5; ++r) C[r][6] = fill[r];
            }
#pragma unroll
            for (int t = 0; t < 3; ++t) {                        // odd slot 0 <- face A: rows 1 .. 3
                const double b[3] = {nb[0][0][t], nb[0][1][t], nb[0][2][t]};
                double fill[5];
                quad_column<1>(P, g3, cc, b, fill);
#pragma unroll
                for (int r = 0; r < 5; ++r) C[r][t] = fill[r];
            }
#pragma unroll
            for (int t = 0; t < 3; ++t) {                        // odd slot 1 <- face B: rows 4 .. 6
                const double b[3] = {nb[1][0][t], nb[1][1][t], nb[1][2][t]};
                double fill[5];
                quad_column<4>(P, g3, cc, b, fill);
#pragma unroll
                for (int r = 0; r < 5; ++r) C[r][3 + t] = fill[r];
            }
        }
        // rows 5, 6: the cell row of O_e (c = 1) and its Neumann row (c = 0), on the columns of odd slot e
        {
            const double *Ko = g.perm + 9 * (size_t)co;
            const double N0 = (double)g.face_normal[3 * (size_t)fbo + 0], N1 = (double)g.face_normal[3 * (size_t)fbo + 1],
                         N2 = (double)g.face_normal[3 * (size_t)fbo + 2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const double kn = -mneu * (Ko[t * 3 + 0] * N0 + Ko[t * 3 + 1] * N1 + Ko[t * 3 + 2] * N2);
                    C[5][3 * s + t] = (e == s) ? dod[t] : 0.0;
                    C[6][3 * s + t] = (e == s) ? kn : 0.0;
                }
            }
            C[5][6] = 1.0;
            C[6][6] = 0.0;
        }
        // ---- phase 2: 14 x 6 over the pair ---------------------------------------------------------------------------------
        double gq[6], vpq[6];
        QuadP2<0, 6>::run(C, gq, vpq, e);
        // ---- the residual r = Q [0; tail]: rows 0 .. 2 of either lane were pivot rows, the tail of Q^T c sits in rows 3 .. 6 ----
        double tail = 0.0, t7[QR];
#pragma unroll
        for (int r = 0; r < QR; ++r) t7[r] = r < 3 ? 0.0 : C[r][6];
#pragma unroll
        for (int r = 3; r < QR; ++r) tail = fma(C[r][6], C[r][6], tail);
        const double rr = pair_sum(tail);                        // r . r = |(Q^T c)(12:20)|^2
        QuadP2Back<5>::run(C, gq, vpq, t7, e);
        const double ro = t7[5];                                 // the cell row of O_e
        // phase 1 backwards on the front of E_e: rows 0 .. 2 were its pivot rows, rows 3 .. 7 are the five fill rows (t7[0 .. 4])
        double x8[8] = {0.0, 0.0, 0.0, t7[0], t7[1], t7[2], t7[3], t7[4]};
#pragma unroll
        for (int k = 2; k >= 0; --k) {
            double a = 0.0;
#pragma unroll
            for (int r = k; r < 8; ++r) a = fma(P[r][k], x8[r], a);
            const double w = -(g3[k] * a);
#pragma unroll
            for (int r = k; r < 8; ++r) x8[r] = fma(w, P[r][k], x8[r]);
        }
        const double re = x8[0];                                 // the cell row of E_e
        const double rri = fast_rcp(rr);
        double we = re * rri, wo = ro * rri;
        const bool ok = computed && rr > 0.0;                    // (rank-deficient system or NaN from a zero column: the zero row)
        we = (ok && __builtin_isfinite(we)) ? we : 0.0;
        wo = (ok && __builtin_isfinite(wo)) ? wo : 0.0;
        wbuf[nd * 4 + (dsc & 3)] = we;
        wbuf[nd * 4 + ((dsc >> 2) & 3)] = wo;
        wave_lds_sync();
        const double nwv = (computed && is_neu) ? wbuf[nd * 4 + 3] : 0.0;   // gls.pyx:470-472: the LAST cell's weight
        const double addv = add_neumann ? nwv : 0.0;
        const double o0 = wbuf[nd * 4 + 2 * e] + addv, o1 = wbuf[nd * 4 + 2 * e + 1] + addv;
        if (valid) {
            out[eb + 2 * e] = o0;
            out[eb + 2 * e + 1] = o1;
            if (e == 0) nws[p] = nwv;
        }
        wave_lds_sync();
    }
}

__global__ void k_quad4_desc(GridView g, const int32_t *__restrict__ nodes, int32_t count, int32_t *__restrict__ desc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    int32_t d[2] = {0, 0};
    (void)quad4_descriptor(g, nodes ? nodes[i] : (int32_t)i, d);   // the list holds classified quad nodes only
    desc[2 * i] = d[0];
    desc[2 * i + 1] = d[1];
}

}  // namespace

int launch_quad4_desc(const GridView &g, const int32_t *nodes, int32_t count, int32_t *desc, hipStream_t stream) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL(k_quad4_desc, blocks_for(count), dim3(256), 0, stream, g, nodes, count, desc);
    return launch_status();
}

int launch_gls_quad4(const GridView &g, const int32_t *nodes, const int32_t *desc, int32_t count, int add_neumann, double *out,
                     double *nws, hipStream_t stream) {
    if (count <= 0) return 0;
    int64_t blocks = ((int64_t)count + 4 * QNPW - 1) / (4 * QNPW);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(nin_gls_quad4_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g, nodes, desc, count, add_neumann, out, nws);
    return launch_status();
}

}  // namespace nin
