// wx_penalty.hip — the repetition penalty and the no-repeat n-gram ban of one decoding step
// (WhisperDecoder's repetition_penalty / no_repeat_ngram_size; whisperx/asr.py:300-326), applied to
// the step's logits in place ahead of the selection.  C ABI and semantics: include/wx_align.h
// (wx_penalize_logits).
//
//   - penalty_kernel, one block of 4 waves per row, three phases around two barriers:
//       1. the row's L ids from global memory into LDS, narrowed to 32 bits after the range check
//          (kSkip for an id outside [0, V)), and a cleared flag per position; L is read from
//          *count here, on the device;
//       2. per position i that holds an id t: whether the n - 1 ids before i equal the last n - 1
//          ids of the history (i >= n - 1; a kSkip on either side matches nothing), and one scan
//          of all ids for the lowest index o at which t occurs, t's owner (two instructions per
//          id: every lane reads the same four ids at a time, a broadcast).  A position that
//          continues the suffix sets flag[o] (every writer stores the same 1);
//       3. the owner alone (o == i) touches column t, with one store: -inf when flag[i] is set,
//          else the penalised logit when the penalty is not 1.
//     So a column has one writer and one store whatever the history repeats, the ban wins without
//     an ordering between two stores, and L > 256 is a strided loop in every phase (at most
//     kMaxL / 256 = 4 positions per lane, their owners kept in registers).  Columns that the
//     history does not name are neither read nor written.  Nothing depends on R; no atomics.
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS): the division is
// the correctly rounded one.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wx_host.h"  // (and through it include/wx_align.h)

namespace wxpenalty {

constexpr int kMaxL = WX_PENALTY_MAX_HISTORY;
constexpr int kThreads = 256;
constexpr int kMaxV = 1 << 24;
constexpr int kSkip = -1;  // an id outside [0, V), and the padding behind position L - 1
constexpr int kPerLane = kMaxL / kThreads;
static_assert(kMaxL % kThreads == 0 && kMaxL % 4 == 0, "whole rounds of the block; the ids are scanned four at a time");

struct Args {
    float* x;
    int64_t stride;
    int32_t V;
    const int64_t* hist;
    int64_t step_stride, row_stride;
    const int64_t* count;
    int32_t offset, max_history;
    float rho;
    int32_t n;
};

__global__ __launch_bounds__(kThreads) void penalty_kernel(const Args a) {
    __shared__ __attribute__((aligned(16))) int s_id[kMaxL];
    __shared__ int s_flag[kMaxL];
    const int r = blockIdx.x, tid = threadIdx.x;
    int64_t L64 = *a.count + (int64_t)a.offset;
    L64 = L64 < 0 ? 0 : L64;
    const int L = (int)(L64 < (int64_t)a.max_history ? L64 : (int64_t)a.max_history);  // <= kMaxL
    if (L == 0) return;
    const int Lpad = (L + 3) & ~3;

    const int64_t* h = a.hist + (int64_t)r * a.row_stride;
    for (int i = tid; i < Lpad; i += kThreads) {
        int id = kSkip;
        if (i < L) {
            const int64_t t = h[(int64_t)i * a.step_stride];
            if (t >= 0 && t < (int64_t)a.V) id = (int)t;  // narrowed only when in range
        }
        s_id[i] = id;
        s_flag[i] = 0;
    }
    __syncthreads();

    // position i continues the suffix when h[i - n + 1 .. i - 1] == h[L - n + 1 .. L - 1]: j = i - n + 1
    // in [0, L - n], so i in [n - 1, L - 1]; nothing when n == 0 or L < n
    const int n = a.n;
    int owner[kPerLane];
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
        const int i = tid + e * kThreads;
        owner[e] = kSkip;
        if (i >= L) continue;
        const int t = s_id[i];
        if (t == kSkip) continue;
        bool same = n >= 1 && i >= n - 1;  // (i <= L - 1 and i >= n - 1: L >= n)
        for (int k = 1; k < n && same; ++k) {
            const int u = s_id[i - k], v = s_id[L - k];
            same = u == v && u != kSkip;
        }
        int o = i;
        for (int j = Lpad - 4; j >= 0; j -= 4) {  // descending: the last hit kept is the lowest index
            const int4 q = *reinterpret_cast<const int4*>(&s_id[j]);
            o = q.w == t ? j + 3 : o;
            o = q.z == t ? j + 2 : o;
            o = q.y == t ? j + 1 : o;
            o = q.x == t ? j : o;
        }
        owner[e] = o;
        if (same) s_flag[o] = 1;
    }
    __syncthreads();

    float* row = a.x + (int64_t)r * a.stride;
    const bool penalise = a.rho != 1.f;
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
        const int i = tid + e * kThreads;
        if (owner[e] != i) continue;  // (kSkip for a position without an id)
        const int t = s_id[i];
        if (s_flag[i]) {
            row[t] = -INFINITY;
        } else if (penalise) {
            const float x = row[t];
            row[t] = x < 0.f ? x * a.rho : x / a.rho;
        }
    }
}

}  // namespace wxpenalty

extern "C" int wx_penalize_logits(float* logits, int64_t row_stride, int32_t R, int32_t V, const int64_t* history,
                                  int64_t step_stride, int64_t hist_row_stride, const int64_t* count,
                                  int32_t count_offset, int32_t max_history, float repetition_penalty,
                                  int32_t no_repeat_ngram_size, void* stream) {
    using namespace wxpenalty;
    if (R < 0 || V < 1 || V > kMaxV || row_stride < V) return WX_E_INVALID;
    if (!isfinite(repetition_penalty) || !(repetition_penalty > 0.f)) return WX_E_INVALID;
    if (no_repeat_ngram_size < 0 || max_history < 0 || max_history > kMaxL) return WX_E_INVALID;
    if (R == 0 || max_history == 0) return WX_OK;
    if (!logits || !history || !count || R > 65535) return WX_E_INVALID;
    Args a;
    a.x = logits;
    a.stride = row_stride;
    a.V = V;
    a.hist = history;
    a.step_stride = step_stride;
    a.row_stride = hist_row_stride;
    a.count = count;
    a.offset = count_offset;
    a.max_history = max_history;
    a.rho = repetition_penalty;
    a.n = no_repeat_ngram_size;
    hipLaunchKernelGGL(penalty_kernel, dim3((unsigned)R), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    return wx::launch_status();
}
