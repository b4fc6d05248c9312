// flags_update.hip -- the Neumann flags of a grid on a device rewritten from DEVICE memory: the whole array, or a subset of nodes
// (nin_fields_set_flags_device, nin_fields_scatter_flags_device).
//
// The resident flag byte of node p is bit0 = boundary point, bit1 = Neumann (pack_host.cpp: pack_node_flags).  Bit0 belongs to the
// mesh and is on the device since nin_grid_to_device; both kernels keep it and compute
//     new = (old & 1) | (is_set(src) ? 2 : 0)
// is_set(x) of a float64 is (long long)x != 0 -- truncation toward zero, the host packer's rule: 0.5 and -0.5 are NOT set, 1e-300 is
// not, -1.0 and 255.0 are.  NaN and values of magnitude >= 2^63 are outside the contract (the host's cast is undefined there).
// is_set(x) of a one-byte source (torch.bool / uint8) is x != 0.
//
// Which rows can move.  The flag of node n is read by row n only (gls.pyx:165-214, idw.pyx:62-63, ls.pyx:58-59; pinned on the oracle
// by tests/test_update_flags_host.py), so exactly the nodes whose byte CHANGES are marked in the grid's dirty set (fields_scatter.hip),
// with the plain store of 1 the other scatters use.  `dirty` null: no marks (everything is dirty already).
//
// Two kernels:
//   nin_flags_set_kernel<Src, WORD>   one streaming pass over the P nodes, kFlagsPerLane = 8 consecutive nodes per lane: the 8 flag
//       bytes are one 8-byte load (the array comes from hipMalloc); a float64 source is 64 consecutive bytes per lane, eight doubles
//       here and four 16-byte loads in the code object, at whatever multiple of 8 bytes the caller's array begins (measured the same at
//       a 16-byte aligned address and at an odd multiple of 8: DESIGN 4.9); a one-byte source is one 8-byte load per lane when the array is 8-byte aligned (WORD), eight byte
//       loads when it is not (a slice of a larger tensor).  A lane whose bytes changed stores its 8-byte word back (it owns all 8
//       nodes), one that changed nothing stores nothing, and the marks are byte stores for the changed nodes only.  No atomics.  The
//       lane that holds the end of the array goes node by node, so nothing is read or written past node P - 1.  About 9 bytes per node.
//   nin_flags_scatter_kernel<Id, Src>   a lane per entry i of the id list.  The id is checked against [0, P) BEFORE any access; a
//       refused id writes nothing, marks nothing and adds one to the device counter of the other scatters.  Else as above: the byte is
//       written if it changes and the node marked if it was written.  Duplicate ids with equal values are harmless; with different
//       values one of them wins, which one is unspecified, and every lane that writes also marks: a node whose bit ends up different
//       from what it was before the call is marked.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"

namespace nin {

namespace {

constexpr int TPB = 256;
constexpr int kFlagsPerLane = 8;

__device__ __forceinline__ bool is_set(double x) { return (long long)x != 0; }
__device__ __forceinline__ bool is_set(uint8_t x) { return x != 0; }

template <class Src, bool WORD>
__global__ __launch_bounds__(TPB) void nin_flags_set_kernel(int64_t P, const Src *__restrict__ src, uint8_t *__restrict__ flags,
                                                            uint8_t *__restrict__ dirty) {
    const int64_t p0 = ((int64_t)blockIdx.x * TPB + threadIdx.x) * kFlagsPerLane;
    if (p0 >= P) return;
    if (p0 + kFlagsPerLane > P) {   // the end of the array: node by node
        for (int64_t p = p0; p < P; ++p) {
            const uint8_t old = flags[p], now = (uint8_t)((old & 1) | (is_set(src[p]) ? 2 : 0));
            if (now != old) {
                flags[p] = now;
                if (dirty) dirty[p] = 1;
            }
        }
        return;
    }
    bool set[kFlagsPerLane];
    if constexpr (WORD) {
        static_assert(sizeof(Src) == 1, "the one-load form is the one-byte source's");
        const uint64_t v = *reinterpret_cast<const uint64_t *>(src + p0);
#pragma unroll
        for (int k = 0; k < kFlagsPerLane; ++k) set[k] = ((v >> (8 * k)) & 0xff) != 0;
    } else {
#pragma unroll
        for (int k = 0; k < kFlagsPerLane; ++k) set[k] = is_set(src[p0 + k]);
    }
    const uint64_t old = *reinterpret_cast<const uint64_t *>(flags + p0);   // (p0 is a multiple of 8 and the array hipMalloc's)
    uint64_t now = old & 0x0101010101010101ull;
#pragma unroll
    for (int k = 0; k < kFlagsPerLane; ++k) now |= set[k] ? (uint64_t)2 << (8 * k) : 0;
    const uint64_t moved = now ^ old;
    if (moved == 0) return;
    *reinterpret_cast<uint64_t *>(flags + p0) = now;
    if (dirty) {
#pragma unroll
        for (int k = 0; k < kFlagsPerLane; ++k)
            if ((moved >> (8 * k)) & 0xff) dirty[p0 + k] = 1;
    }
}

template <class Id, class Src>
__global__ __launch_bounds__(TPB) void nin_flags_scatter_kernel(int64_t m, const Id *__restrict__ ids, const Src *__restrict__ src, int32_t P,
                                                                uint8_t *__restrict__ flags, uint8_t *__restrict__ dirty,
                                                                int32_t *__restrict__ rejected) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const int64_t p = (int64_t)ids[i];
    if (p < 0 || p >= (int64_t)P) {   // before any access through the id
        atomicAdd(rejected, 1);
        return;
    }
    const uint8_t old = flags[p], now = (uint8_t)((old & 1) | (is_set(src[i]) ? 2 : 0));
    if (now != old) {
        flags[p] = now;
        if (dirty) dirty[p] = 1;
    }
}

template <class Src>
void set_variant(int64_t P, const void *src, uint8_t *flags, uint8_t *dirty, hipStream_t stream) {
    const unsigned blocks = (unsigned)((P + (int64_t)TPB * kFlagsPerLane - 1) / ((int64_t)TPB * kFlagsPerLane));
    if constexpr (sizeof(Src) == 1) {
        if (reinterpret_cast<uintptr_t>(src) % 8 == 0) {
            hipLaunchKernelGGL((nin_flags_set_kernel<Src, true>), dim3(blocks), dim3(TPB), 0, stream, P, static_cast<const Src *>(src), flags, dirty);
            return;
        }
    }
    hipLaunchKernelGGL((nin_flags_set_kernel<Src, false>), dim3(blocks), dim3(TPB), 0, stream, P, static_cast<const Src *>(src), flags, dirty);
}

template <class Id, class Src>
void scatter_variant(int64_t n, const void *ids, const void *src, int32_t P, uint8_t *flags, uint8_t *dirty, int32_t *rejected,
                     hipStream_t stream) {
    hipLaunchKernelGGL((nin_flags_scatter_kernel<Id, Src>), blocks_for(n, TPB), dim3(TPB), 0, stream, n,
                       static_cast<const Id *>(ids), static_cast<const Src *>(src), P, flags, dirty, rejected);
}

}  // namespace

int launch_set_flags(int32_t n_points, const void *dev_flags, int flags_are_bytes, uint8_t *flags, uint8_t *dirty, hipStream_t stream) {
    if (n_points <= 0) return 0;
    if (flags_are_bytes) set_variant<uint8_t>(n_points, dev_flags, flags, dirty, stream);
    else set_variant<double>(n_points, dev_flags, flags, dirty, stream);
    return launch_status();
}

int launch_scatter_flags(int32_t n_points, const void *dev_ids, int ids_are_int64, int64_t n, const void *dev_flags, int flags_are_bytes,
                         uint8_t *flags, uint8_t *dirty, int32_t *rejected, hipStream_t stream) {
    if (n <= 0) return 0;
    if (n > (int64_t)INT32_MAX * TPB) return fail(NIN_ERANGE, "%lld ids are more than one launch takes", (long long)n);
    if (ids_are_int64) {
        if (flags_are_bytes) scatter_variant<int64_t, uint8_t>(n, dev_ids, dev_flags, n_points, flags, dirty, rejected, stream);
        else scatter_variant<int64_t, double>(n, dev_ids, dev_flags, n_points, flags, dirty, rejected, stream);
    } else {
        if (flags_are_bytes) scatter_variant<int32_t, uint8_t>(n, dev_ids, dev_flags, n_points, flags, dirty, rejected, stream);
        else scatter_variant<int32_t, double>(n, dev_ids, dev_flags, n_points, flags, dirty, rejected, stream);
    }
    return launch_status();
}

}  // namespace nin
