// gls_shape_chain.hpp -- the chain of one face from (Fcbar_f, Nbar_f) to the point slots of the face, written once for
// the two kernels that end in it: nin_shape_face_kernel (kernels_gls_shape.hip: the sums of the records) and nin_xjac_face_kernel
// (kernels_gls_shape_jacobian.hip: the sums of v_p times the kept records).  With v = 1 the two agree bit for bit, and
// they can because this is one expression.
#pragma once
#include <hip/hip_runtime.h>

namespace nin {

// acc = (Fcbar_f, Nbar_f); v1 = x_0 - x_1, v2 = x_2 - x_1 and nn = |v1 x v2| from the resident coordinates, N the resident normal; slot
// [4][3]: fc_f = sum x_v / npofa gives every point Fcbar_f / npofa, the fourth point of a quadrilateral too (a triangle: 0); N = n / |n|
// gives nbar = (Nbar_f - (Nbar_f . N) N) / |n|, v1bar = v2 x nbar, v2bar = nbar x v1, x_0 += v1bar, x_2 += v2bar, x_1 -= v1bar + v2bar
__device__ __forceinline__ void shape_face_chain(const double (&acc)[6], const double (&v1)[3], const double (&v2)[3], double nn,
                                                 const double (&N)[3], int npofa, double *slot) {
    const double dot = (acc[3] * N[0] + acc[4] * N[1]) + acc[5] * N[2];
    const double nb[3] = {(acc[3] - dot * N[0]) / nn, (acc[4] - dot * N[1]) / nn, (acc[5] - dot * N[2]) / nn};
    const double v1b[3] = {v2[1] * nb[2] - v2[2] * nb[1], v2[2] * nb[0] - v2[0] * nb[2], v2[0] * nb[1] - v2[1] * nb[0]};
    const double v2b[3] = {nb[1] * v1[2] - nb[2] * v1[1], nb[2] * v1[0] - nb[0] * v1[2], nb[0] * v1[1] - nb[1] * v1[0]};
    const double dn = (double)npofa;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double share = acc[c] / dn;
        slot[0 + c] = share + v1b[c];
        slot[3 + c] = share - (v1b[c] + v2b[c]);
        slot[6 + c] = share + v2b[c];
        slot[9 + c] = npofa == 4 ? share : 0.0;
    }
}

}  // namespace nin
