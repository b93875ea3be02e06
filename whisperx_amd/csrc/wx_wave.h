// wx_wave.h — the wave64 helpers shared by the alignment DP (wx_dp_*.h) and Binarize
// (wx_binarize.hip): lane index, and wave-uniform (SGPR) copies of per-lane values; and the
// attention kernels' block order over the XCDs.
#ifndef WX_WAVE_H
#define WX_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wx {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & (kWave - 1)); }

__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ int64_t uniform64(int64_t x) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uint64_t)x);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ float uniformf(float x) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
// lane l's 64-bit value, wave-uniform (two v_readlane)
__device__ __forceinline__ unsigned long long readlane64(unsigned long long x, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// The attention kernels' block order.  1-D grid, block L runs on XCD L % 8 (round-robin dispatch):
// hand each XCD a contiguous run of units, so the blocks sharing one head's K / V (768 KB at
// T = 1499) meet in one XCD's L2 instead of all eight (round 4 A/B on attn_f32_kernel: the plain
// blockIdx order was 1-2% slower).  Returns this block's unit.
__device__ __forceinline__ unsigned xcd_unit() {
    const unsigned L = blockIdx.x, n = gridDim.x, x = L % 8, i = L / 8, q = n / 8, r = n % 8;
    return x * q + min(x, r) + i;
}

}  // namespace wx

#endif  // WX_WAVE_H
