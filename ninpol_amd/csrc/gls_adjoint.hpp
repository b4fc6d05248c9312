// gls_adjoint.hpp -- the bins of the GLS adjoint kernel (kernels_gls_adjoint.hip), shared by the kernels and the C ABI (internal)
#pragma once
#include <cstdint>

#include "gls_plan.hpp"

namespace nin {

// Nodes are binned by the bytes of their slot, as the block kernel bins them: three LDS classes -- one, two and four wavefronts per
// node, budgets chosen for ten, four and one workgroup per CU -- and a global-scratch class (eight wavefronts, a slot per workgroup)
// for the systems that do not fit one CU's LDS.
constexpr int kAdjBins = 4;
NIN_HD inline int64_t adj_bin_budget(int b) { return b == 0 ? 16384 : b == 1 ? 40960 : b == 2 ? 159744 : 0; }

// One node's slot: the m x n system, tau / y / s [n] each, r / q [m] each, and the int32 maps (the node's cells, and per face its row and
// its two cells' positions).  m counts a row for every boundary face, Neumann-flagged or not: the flag can change on the device
// (nin_fields_set_flags_device), the bin is made once.
NIN_HD inline int64_t adj_node_bytes(int64_t ne, int64_t nf, int64_t nbf) {
    const int64_t m = ne + 3 * (nf - nbf) + nbf, n = 3 * ne + 1;
    const int64_t doubles = m * n + 3 * n + 2 * m + ((ne + 3 * nf + 1) >> 1);
    return ((doubles * 8 + 15) / 16) * 16;
}
NIN_HD inline int adj_node_bin(int64_t bytes, bool force_global) {
    for (int b = 0; b < kAdjBins - 1 && !force_global; ++b)
        if (bytes <= adj_bin_budget(b)) return b;
    return kAdjBins - 1;
}

}  // namespace nin
