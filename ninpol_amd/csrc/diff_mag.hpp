// diff_mag.hpp -- diff_mag of a cell from the diagonal of its permeability, for the device units that write the resident table
// (fields_update.hip, fields_scatter.hip; internal).  Both are built with -ffp-contract=off (build.py).
#pragma once
#include <hip/hip_runtime.h>

namespace nin {

// the host's expression (pack_host.cpp: nin_diff_mag), operation for operation
__device__ __forceinline__ double diff_mag_of(double k0, double k4, double k8) {
    const double tr = (k0 + k4) + k8;
    const double x = 1 - (3 * 1.0 / tr);
    return x * x;
}

}  // namespace nin
