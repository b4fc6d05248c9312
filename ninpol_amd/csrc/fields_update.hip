// fields_update.hip -- the permeability of a loaded grid replaced from DEVICE memory (nin_fields_set_permeability_device).
//
// The grid's resident perm[E][9] and diff_mag[E] are written from a caller's K[E][9] and an optional scale[E]:
//   perm[e][k] = K[e][k]  or  scale[e] * K[e][k]   (one multiplication, rounded once),
//   diff_mag[e] = (1 - 3 * 1.0 / ((perm[e][0] + perm[e][4]) + perm[e][8]))^2
// the second exactly as nin_diff_mag (pack_host.cpp; interpolator.pyx:501-509 as compiled: `det ** (1 / 3)` is `det ** 0`) computes
// it on the host from the same nine values: the same operations in the same order, IEEE division, and -- build.py -- no
// contraction, so the bits are the host's.
//
// The kernel is a stream: 72 (+ 8) bytes in and 80 out per cell, nothing is read twice.  A cell is a run of nine doubles, so a lane
// per cell would gather with a stride of 72 bytes.  Instead a workgroup of 256 threads takes the 2304 consecutive doubles of its 256
// cells as a flat run: every lane loads 16 bytes, a wavefront 1 KiB of contiguous bytes per instruction, multiplies by its cells'
// factors, and stores the same 16 bytes to perm; the values also go to LDS, where -- after one barrier -- a lane per cell picks its
// diagonal.  Those reads are 8 bytes at a stride of 18 dwords: the 32 lanes of a group fall on 32 different even banks of the 64, no
// conflict.  The factors of the workgroup's cells come in as one coalesced load and are looked up in LDS by element / 9.
//   * perm comes from hipMalloc and a workgroup's run starts at 256 * 72 bytes times the block index: its stores are always 16-byte
//     aligned.  K is the caller's: a tensor view may start at an odd multiple of 8 bytes.  Then (ALIGNED16 = false) every workgroup
//     takes the plain path below: a lane per double, nine rounds of 8-byte loads and stores at consecutive addresses (512 contiguous
//     bytes per wavefront instruction).  A pair of 8-byte loads in one lane would not do: the compiler fuses it back into one 16-byte
//     load, which only the target's unaligned-access mode would make legal at such an address.
//   * the last workgroup of a launch takes the plain path too, with its bound.
// The other shape the same bytes allow -- a copy / scale pass with a lane per 16 bytes and no LDS, then a pass with a lane per cell
// that gathers the diagonal from perm as just written -- gave the same bits and was timed beside this one, calls interleaved, at
// 216^3 cells: 0.412 against 0.272 ms; it reads the lines of perm a second time.  It is not kept.
// No atomics and no work counters; the grids are sized from E.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "diff_mag.hpp"
#include "launch.hpp"

namespace nin {

namespace {

constexpr int TPB = 256;
constexpr int RUN = 9 * TPB;   // doubles of a workgroup's cells

template <bool SCALED, bool ALIGNED16>
__global__ __launch_bounds__(TPB) void nin_update_perm_kernel(int32_t E, const double *__restrict__ K, const double *__restrict__ scale,
                                                               double *__restrict__ perm, double *__restrict__ diff_mag) {
    __shared__ __attribute__((aligned(16))) double s[RUN];
    __shared__ double sc[TPB];
    const int t = threadIdx.x;
    const int32_t e0 = (int32_t)blockIdx.x * TPB;
    const int valid = min(TPB, E - e0);
    const int64_t base = (int64_t)e0 * 9;
    const double *__restrict__ src = K + base;
    double *__restrict__ dst = perm + base;
    if (SCALED) {
        if (t < valid) sc[t] = scale[e0 + t];
        __syncthreads();
    }
    if (ALIGNED16 && valid == TPB) {
        // 1152 pieces of 16 bytes: four rounds of all lanes and one of the first half
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int j = r * TPB + t;   // piece: doubles 2 j, 2 j + 1
            if (r == 4 && t >= TPB / 2) break;
            double2 v = reinterpret_cast<const double2 *>(src)[j];
            if (SCALED) {
                v.x = sc[(2 * j) / 9] * v.x;
                v.y = sc[(2 * j + 1) / 9] * v.y;
            }
            reinterpret_cast<double2 *>(dst)[j] = v;
            reinterpret_cast<double2 *>(s)[j] = v;
        }
    } else {   // K at an odd multiple of 8 bytes, or the last workgroup of the launch: a lane per double
        double v[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) {   // nine rounds, all loads in flight before the first store
            const int i = r * TPB + t;
            v[r] = i < 9 * valid ? src[i] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int i = r * TPB + t;
            if (i < 9 * valid) {
                if (SCALED) v[r] = sc[i / 9] * v[r];
                dst[i] = v[r];
                s[i] = v[r];
            }
        }
    }
    __syncthreads();
    if (t < valid) diff_mag[e0 + t] = diff_mag_of(s[9 * t], s[9 * t + 4], s[9 * t + 8]);
}


template <bool SCALED, bool ALIGNED16>
void launch_variant(int32_t E, const double *K, const double *scale, double *perm, double *diff_mag, hipStream_t stream) {
    hipLaunchKernelGGL((nin_update_perm_kernel<SCALED, ALIGNED16>), blocks_for(E), dim3(TPB), 0, stream, E, K, scale, perm, diff_mag);
}

}  // namespace

hipError_t launch_update_permeability(int32_t n_elems, const double *dev_K, const double *dev_scale, double *perm, double *diff_mag,
                                      hipStream_t stream) {
    if (n_elems <= 0) return hipSuccess;
    const bool aligned = (reinterpret_cast<uintptr_t>(dev_K) & 15) == 0;
    if (dev_scale) {
        if (aligned) launch_variant<true, true>(n_elems, dev_K, dev_scale, perm, diff_mag, stream);
        else launch_variant<true, false>(n_elems, dev_K, dev_scale, perm, diff_mag, stream);
    } else {
        if (aligned) launch_variant<false, true>(n_elems, dev_K, dev_scale, perm, diff_mag, stream);
        else launch_variant<false, false>(n_elems, dev_K, dev_scale, perm, diff_mag, stream);
    }
    return hipGetLastError();
}

}  // namespace nin
