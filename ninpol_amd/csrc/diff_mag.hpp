// diff_mag.hpp -- diff_mag of a cell from the diagonal of its permeability, and its derivative (internal).  diff_mag_of is for the
// device units that write the resident table (fields_update.hip, fields_scatter.hip), both built with -ffp-contract=off (build.py);
// diff_mag_fold is for the derivative kernels (kernels_gls_adjoint.hip, kernels_gls_jacobian.hip), built with the default contraction.
#pragma once
#include <hip/hip_runtime.h>

namespace nin {

// the host's expression (pack_host.cpp: nin_diff_mag), operation for operation
__device__ __forceinline__ double diff_mag_of(double k0, double k4, double k8) {
    const double tr = (k0 + k4) + k8;
    const double x = 1 - (3 * 1.0 / tr);
    return x * x;
}

// d diff_mag / d K_dd = 2 (1 - 3 / tr) 3 / tr^2 of the cell whose permeability K [9] is: the one expression of the tangent, the reduced
// adjoint, the gather and the fold kernel.  launch_vjp(v = 1) = launch_weights_backward and a reduced linearisation = a full one plus
// the chain rule hold bit for bit because these four sites share it
__device__ __forceinline__ double diff_mag_fold(const double *K) {
    const double tr = (K[0] + K[4]) + K[8];
    return (2.0 * (1.0 - 3.0 / tr) * 3.0 / (tr * tr));
}

}  // namespace nin
