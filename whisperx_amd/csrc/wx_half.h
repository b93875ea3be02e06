// wx_half.h — the element-type codes of the kernels templated over their element type, and the
// 16-bit <-> fp32 conversions they share.
#ifndef WX_HALF_H
#define WX_HALF_H
#include <hip/hip_runtime.h>

#include "../../include/wx_align.h"

namespace wx {

// fp32, or a wx_*_h16 entry point's dtype argument
enum { kF32 = 0, kF16 = WX_DTYPE_F16, kBF16 = WX_DTYPE_BF16 };
constexpr int half_et(bool bf) { return bf ? kBF16 : kF16; }

// ET: kF16 or kBF16.  Bit patterns travel as shorts; widening is exact, rounding is to nearest even.
template <int ET>
__device__ __forceinline__ float widen16(short x) {
    static_assert(ET == kF16 || ET == kBF16, "a 16-bit element type");
    if constexpr (ET == kBF16) return __uint_as_float((unsigned)(unsigned short)x << 16);
    else return (float)__builtin_bit_cast(_Float16, x);
}
template <int ET>
__device__ __forceinline__ short round16(float x) {
    static_assert(ET == kF16 || ET == kBF16, "a 16-bit element type");
    if constexpr (ET == kBF16) return __builtin_bit_cast(short, (__bf16)x);
    else return __builtin_bit_cast(short, (_Float16)x);
}

}  // namespace wx
#endif  // WX_HALF_H
