// wx_dp_timing.h — the phase-timing layer of the alignment DP (wx_align_dp.h): the debug arrays and
// every macro that touches them.  -DWX_PHASE_TIMING (one TU, wx_align.hip: the arrays must be one
// copy) gives the macros their bodies; in the normal build they expand to nothing.
// What lands where (tools/satbench.py --phases decodes these; the numbers must not move).
// All per workgroup (blockIdx.x < 8192); cycles are s_memtime, times s_memrealtime (100 MHz).
//   wx_phase[6]   cycles at 0 kernel entry, 1 forward end, 2 walk end, 3 exit; time at 4 entry, 5 exit
//   wx_cq[q][3]   chunk q < 48, time when: 0 wave 0 passed barrier q, 1 wave W - 1 stored chunk
//                 q's halo granules, 2 wave 0 had chunk q's halo (split kernels)
//   wx_loop[slot][3], kLoopSlots slots (later phases reuse the slots of earlier ones):
//     wv       Forward::run, DP wave wv: cycles in steps / barrier waits / other chunk work
//     W        the staging helper (helper: column 0 / barrier wait / other; helper_reg: work /
//              barrier wait / DMA wait)
//     W + 1    the column-0 helper (col0_helper: work / barrier wait / 0; else as slot W)
//     6 + wv   walk_spec, wave wv <= 6, cycles since its entry: wave 0 argmax / first walk /
//              barrier; walkers first walk / barrier / K
//     13       wave 0's last walk_range: run-length loop cycles / changes / blocks
//     14       the hand-off consumer: missed prefetches / cycles in the chunk's wait / in slack waits
//     15       align_dp_body's walk phase: argmax / walk / compaction cycles
//     16 + wv  walk_range of wave wv < 8: window gather (its load wait) / run-length loop cycles /
//              blocks (24: wave 0's second walk)
#ifndef WX_DP_TIMING_H
#define WX_DP_TIMING_H

#ifdef WX_PHASE_TIMING
#include <hip/hip_runtime.h>

#include "wx_wave.h"  // lane_id

namespace wx {
__device__ unsigned long long wx_phase[8192 * 6];
constexpr int kLoopSlots = 32;  // per workgroup, 3 counters each
__device__ unsigned long long wx_loop[8192 * kLoopSlots * 3];
__device__ unsigned long long wx_cq[8192 * 48 * 3];
}  // namespace wx
#define WX_TIMED(...) __VA_ARGS__
#else
#define WX_TIMED(...)
#endif

#define WX_CQ(q, i) \
    WX_TIMED(if (lane_id() == 0 && blockIdx.x < 8192 && (q) < 48) wx_cq[(blockIdx.x * 48 + (q)) * 3 + (i)] = __builtin_amdgcn_s_memrealtime())
#define WX_STAMP(i) \
    WX_TIMED(if (threadIdx.x == 0 && blockIdx.x < 8192) wx_phase[blockIdx.x * 6 + (i)] = __builtin_amdgcn_s_memtime())
#define WX_STAMP_RT(i) \
    WX_TIMED(if (threadIdx.x == 0 && blockIdx.x < 8192) wx_phase[blockIdx.x * 6 + (i)] = __builtin_amdgcn_s_memrealtime())
// a cycle stamp in a new variable / counters declared / acc += expr / a variable re-stamped / a timing-only statement
#define WX_T(v) WX_TIMED(unsigned long long v = __builtin_amdgcn_s_memtime())
#define WX_TDECL(...) WX_TIMED(unsigned long long __VA_ARGS__)
#define WX_TACC(acc, ...) WX_TIMED(acc += (__VA_ARGS__))
#define WX_TSET(v) WX_TIMED(v = __builtin_amdgcn_s_memtime())
#define WX_TONLY(...) WX_TIMED(__VA_ARGS__)
// WX_TDUMP: three counters into wx_loop slot k by the lanes where `cond` holds, then `...` under the same guard.
// k continues the sum as written (`6 + wv` adds 6, then wv, as the probes always did): parenthesise a conditional
#define WX_TSTORE(k, a, b, c)                                                       \
    unsigned long long* wx_o = wx_loop + ((size_t)blockIdx.x * kLoopSlots + k) * 3; \
    wx_o[0] = (a), wx_o[1] = (b), wx_o[2] = (c);
#define WX_TDUMP(cond, k, a, b, c, ...) \
    WX_TIMED(if ((cond) && blockIdx.x < 8192) { WX_TSTORE(k, a, b, c) __VA_ARGS__ })

#endif  // WX_DP_TIMING_H
