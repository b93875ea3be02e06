// wx_diarize.hip — speaker assignment (whisperx/diarize.py:35-67 assign_word_speakers), batched
// over files in one launch.  C ABI and semantics: include/wx_align.h (wx_assign_speakers).
//
// Mapping: one lane per query, one wave per 64 consecutive queries of the packed query array.
// A wave takes the files its 64 queries belong to one after the other (almost always one), and
// within a file one speaker group at a time, so a lane holds one Kahan pair and one running
// best in registers.  Inside a group the wave walks the turns in table row order; the turn index
// is wave-uniform, so the turn's two doubles come through the scalar data cache and the lane's
// work per turn is a handful of fp64 VALU operations.  With fill_nearest == 0 a turn that cannot
// overlap [min q_start, max q_end] of the wave's queries is skipped by a wave-uniform test: such
// a turn has x <= 0 (or NaN) in every lane, so no lane would have added it.  A NaN turn fails
// both comparisons of the test and stays on the per-lane path.
//
// The file is built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS): the
// Kahan compensation below is exactly the four fp64 operations written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wx_host.h"  // (and through it include/wx_align.h)

namespace wxd {

constexpr int kWave = 64;

struct AssignSizes {
    int64_t G, n_turns, Q;
    int32_t F, fill_nearest;
};

__device__ __forceinline__ int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// min / max over the wave's lanes that ignore NaN operands (a NaN only where every lane has one)
__device__ __forceinline__ double wave_min(double v) {
    for (int m = kWave / 2; m > 0; m >>= 1) {
        const double o = __shfl_xor(v, m, kWave);
        v = (o < v || v != v) ? o : v;
    }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int m = kWave / 2; m > 0; m >>= 1) {
        const double o = __shfl_xor(v, m, kWave);
        v = (o > v || v != v) ? o : v;
    }
    return v;
}

// the lanes' common value of v, in scalar registers
__device__ __forceinline__ double wave_uniform(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// (the pointers are separate __restrict__ parameters: that is what lets the compiler prove the
// tables are not written here and read the wave-uniform ones through the scalar cache)
__global__ __launch_bounds__(kWave) void assign_speakers_kernel(
    const double* __restrict__ turn_start, const double* __restrict__ turn_end, const int64_t* __restrict__ turn_off,
    const int64_t* __restrict__ grp_off, const double* __restrict__ q_start, const double* __restrict__ q_end,
    const int64_t* __restrict__ q_off, int32_t* __restrict__ speaker, double* __restrict__ best_sum /* may be null */,
    const AssignSizes a) {
    const int lane = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * kWave;  // wave-uniform: the block is one wave
    const int64_t q1 = q0 + kWave < a.Q ? q0 + kWave : a.Q;
    const int64_t q = q0 + lane;
    const bool fill = a.fill_nearest != 0;

    // the file of query q0: the last f with q_off[f] <= q0 (files without queries are passed over)
    int lo = 0, hi = a.F;  // invariant: q_off[lo] <= q0 (q_off[0] == 0); answer in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (q_off[mid] <= q0) lo = mid; else hi = mid;
    }

    for (int f = lo; f < a.F; ++f) {
        const int64_t fq0 = q_off[f], fq1 = q_off[f + 1];
        if (fq0 >= q1) break;
        if (fq1 <= q0 || fq1 <= fq0) continue;
        const bool mine = q >= fq0 && q < fq1 && q < q1;
        const double nan = __builtin_nan("");
        const double qs = mine ? q_start[q] : nan;
        const double qe = mine ? q_end[q] : nan;
        const bool qnan = qs != qs || qe != qe;
        // span of the wave's queries in this file, for the wave-uniform skip (fill_nearest == 0)
        double span_lo = 0.0, span_hi = 0.0;
        if (!fill) {
            span_lo = wave_uniform(wave_min(qs));
            span_hi = wave_uniform(wave_max(qe));
        }
        const int64_t g0 = clampi(grp_off[f], 0, a.G), g1 = clampi(grp_off[f + 1], g0, a.G);

        bool have = false;
        double best = 0.0;
        int32_t best_rank = -1;
        for (int64_t g = g0; g < g1; ++g) {
            const int64_t t0 = clampi(turn_off[g], 0, a.n_turns), t1 = clampi(turn_off[g + 1], t0, a.n_turns);
            double s = 0.0, c = 0.0;
            bool any = fill && t1 > t0;  // fill_nearest: every turn takes part, the group exists
            for (int64_t t = t0; t < t1; ++t) {
                const double ts = turn_start[t], te = turn_end[t];
                if (!fill && (te <= span_lo || ts >= span_hi)) continue;  // false for a NaN turn or span
                // np.minimum / np.maximum propagate NaN
                const double mn = te < qe ? te : qe;
                const double mx = ts > qs ? ts : qs;
                double x = mn - mx;
                if (qnan || ts != ts || te != te) x = nan;
                const bool part = fill ? (x == x) : (x > 0.0);  // a NaN adds nothing in either mode
                if (part) {
                    const double y = x - c;
                    const double tt = s + y;
                    c = (tt - s) - y;
                    s = tt;
                    any = true;
                }
            }
            // the largest sum; the first group (sorted label order) among equal sums; a NaN sum
            // only where there is no other
            if (any && (!have || s > best || (best != best && s == s))) {
                have = true;
                best = s;
                best_rank = (int32_t)(g - g0);
            }
        }
        if (mine) {
            speaker[q] = best_rank;
            if (best_sum) best_sum[q] = have ? best : 0.0;
        }
    }
}

}  // namespace wxd

extern "C" int wx_assign_speakers(const double* turn_start, const double* turn_end, const int64_t* turn_off,
                                  const int64_t* grp_off, int64_t G, int64_t n_turns, const double* q_start,
                                  const double* q_end, const int64_t* q_off, int32_t F, int64_t Q, int32_t fill_nearest,
                                  int32_t* speaker, double* best_sum, void* stream) {
    using namespace wxd;
    if (F < 0 || Q < 0 || G < 0 || n_turns < 0) return WX_E_INVALID;
    if (F == 0 || Q == 0) return WX_OK;
    if (!turn_off || !grp_off || !q_start || !q_end || !q_off || !speaker) return WX_E_INVALID;
    if (n_turns > 0 && (!turn_start || !turn_end)) return WX_E_INVALID;
    const int64_t waves = (Q + kWave - 1) / kWave;
    if (waves > 0x7fffffff) return WX_E_INVALID;
    AssignSizes a;
    a.G = G;
    a.n_turns = n_turns;
    a.Q = Q;
    a.F = F;
    a.fill_nearest = fill_nearest;
    hipLaunchKernelGGL(assign_speakers_kernel, dim3((unsigned)waves), dim3(kWave), 0,
                       reinterpret_cast<hipStream_t>(stream), turn_start, turn_end, turn_off, grp_off, q_start, q_end,
                       q_off, speaker, best_sum, a);
    return wx::launch_status();
}
