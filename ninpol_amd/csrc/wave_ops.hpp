// wave_ops.hpp -- the cross-lane primitives of a 64-lane wavefront, once for every kernel (internal, device code only).
// Moves and fences only: the one piece of floating-point arithmetic here is the additions of group_sum and of wave_sum on top of it,
// which no contraction setting can change -- the header is safe in the units built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace nin {
namespace waveops {

template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// v of lane `lane` (wave-uniform) as a scalar: v_readlane
__device__ __forceinline__ double rl64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ uint32_t rl32(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }

__device__ __forceinline__ int ufirst(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Sum over the aligned group of L lanes (8 or 16) a lane belongs to, result in every lane of the group.  All 64 lanes must be active.
// The order of these additions is part of the bitwise contract of every product that uses it (the kept Jacobians' apply kernels, and
// through wave_sum the dense GLS kernels): this is the one place it is written.
template <int L>
__device__ __forceinline__ double group_sum(double v) {
    static_assert(L == 8 || L == 16, "a group is 8 or 16 lanes");
    v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);  // row_half_mirror
    if constexpr (L == 16) v += dpp_mov<0x140>(v);  // row_mirror
    return v;
}

// Sum over the 64 lanes, result in every lane.  All 64 lanes must be active.  (mfwstrips::wave_allsum adds in another order and is
// not this.)
__device__ __forceinline__ double wave_sum(double v) {
    v = group_sum<16>(v);   // every lane holds its 16-lane row sum
    return (rl64(v, 0) + rl64(v, 16)) + (rl64(v, 32) + rl64(v, 48));
}

// Orders this wave's LDS traffic: a lane may read what another lane of the wave wrote.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The same for a wave whose words are in LDS (LDS = true) or in global memory (a scratch slot, a row of the result)
template <bool LDS>
__device__ __forceinline__ void wave_sync() {
    if (LDS) {
        wave_lds_sync();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

}  // namespace waveops
}  // namespace nin
