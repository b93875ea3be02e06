// wx_wave.h — the wave64 helpers shared by the alignment DP (wx_dp_*.h) and Binarize
// (wx_binarize.hip): lane index, and wave-uniform (SGPR) copies of per-lane values.
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

}  // namespace wx

#endif  // WX_WAVE_H
