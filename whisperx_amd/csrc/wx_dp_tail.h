// wx_dp_tail.h — around the alignment DP's forward and walk (wx_align_dp.h): q0 = exp(em[t, 0]),
// merge_repeats from the start frames, and the generic forward of the recovery path.
#ifndef WX_DP_TAIL_H
#define WX_DP_TAIL_H

#include "wx_dp_config.h"  // kChunk, Layout
#include "wx_dp_prims.h"   // exp_cr, nan_max, col0_value, block_fence

namespace wx {

// q0[t] = exp(em[t, 0]) for rows [0, T), by the threads [first_thread, blockDim) (the waves
// that do not walk).
__device__ void fill_q0(const float* __restrict__ E, int V, int T, float* __restrict__ q0, int first_thread) {
    const int n = (int)blockDim.x - first_thread;
    for (int t = (int)threadIdx.x - first_thread; t < T; t += n) q0[t] = exp_cr(E[(int64_t)t * V]);
}

// ------------------------------------------------------------------------------------
// Generic forward of one segment by the whole workgroup: one time step per barrier, cells
// strided over the threads, rows ping-ponged in LDS.  Orders of magnitude slower than
// Forward (~1-3 ms per 30 s segment) and used only to recover a segment the fast path could
// not finish: a split segment whose cross-CU hand-off timed out (status 3 before round 2)
// and a large-vocabulary segment with more than kGatherVS distinct columns (status 2 before
// round 2).  Same arithmetic as Forward::advance (alignment.py:367-378: fp32 adds, strict
// `changed > stayed` bit, NaN-propagating max, fp64 column-0 cumsum, +inf in the last N rows
// of column 0) and the same outputs in the same places: the decision words in the launch's
// bitmap layout `lay`, the column-N history cn[0..T-1] and q0.  Returns false (nothing
// written) when two rows plus the decision words of N cells do not fit in `lds_floats`.
__device__ __noinline__ bool generic_forward(int T, int N, int blank, const float* __restrict__ E, int V,
                                             const int32_t* __restrict__ tok /* segment's tokens */,
                                             unsigned* __restrict__ bits, Layout lay, float* __restrict__ cn,
                                             float* __restrict__ q0, float* lds, int lds_floats) {
    if (3 * (N + 1) > lds_floats) return false;
    float* ra = lds;
    float* rb = lds + (N + 1);
    unsigned* wb = reinterpret_cast<unsigned*>(lds + 2 * (N + 1));  // wb[j-1]: cell j's open word
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int inf_from = T + 1 - N;
    for (int j = tid; j <= N; j += nthr) {
        ra[j] = j == 0 ? col0_value(0, 0.0, T, N) : -INFINITY;
        if (j > 0) wb[j - 1] = 0u;
    }
    for (int t = tid; t < T; t += nthr) q0[t] = exp_cr(E[(int64_t)t * V]);
    double acc = 0.0;  // sum of em[0..t, 0] (every thread, same order)
    for (int t = 0; t < T; ++t) {
        __syncthreads();
        const float* row = E + (int64_t)t * V;
        const float eb = row[blank];
        const bool flush = (t & (kChunk - 1)) == kChunk - 1 || t == T - 1;
        const int sh = kChunk - 1 - (t & (kChunk - 1));  // keep bit 31 = first step of the block
        for (int j = tid + 1; j <= N; j += nthr) {
            int tk = tok[j - 1];
            tk = (tk >= 0 && tk < V) ? tk : 0;
            const float s = ra[j] + eb;
            const float c = ra[j - 1] + row[tk];
            unsigned w = (wb[j - 1] << 1) | (c > s ? 1u : 0u);
            rb[j] = nan_max(s, c);
            if (j == N) cn[t] = rb[j];
            if (flush) {
                int g, k;
                lay.locate(j - 1, g, k);
                bits[((int64_t)(t >> 5) * lay.C + k) * lay.lanes + g] = w << sh;
                w = 0u;
            }
            wb[j - 1] = w;
        }
        acc += (double)row[0];
        if (tid == 0) rb[0] = (t + 1 >= inf_from) ? INFINITY : (float)acc;
        float* x = ra;
        ra = rb;
        rb = x;
    }
    __syncthreads();
    return true;
}

// merge_repeats from per-token start frames (alignment.py:438-454 + the prob rule of :409).
__device__ void merge_tokens(const float* __restrict__ E, int V, const int32_t* __restrict__ tok, int N, int t_start,
                             const float* __restrict__ q0, const int32_t* __restrict__ start, int32_t* __restrict__ seg_end,
                             double* __restrict__ seg_score) {
    for (int k = (int)threadIdx.x; k < N; k += (int)blockDim.x) {
        const int s = start[k];
        const int e = (k + 1 < N) ? start[k + 1] : t_start;
        int tk = tok[k];
        tk = (tk >= 0 && tk < V) ? tk : 0;
        double sum = (double)exp_cr(E[(int64_t)s * V + tk]);
        int x = s + 1;
        for (; x + 8 <= e; x += 8) {  // 8 loads in flight, adds in the reference's order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = q0[x + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += (double)v[u];
        }
        for (; x < e; ++x) sum += (double)q0[x];
        seg_end[k] = e;
        seg_score[k] = sum / (double)(e - s);
    }
}

// merge_tokens with the segment's q0 row and start frames staged in LDS first (coalesced, 8
// loads in flight per thread), so each token's left-to-right fp64 sum reads LDS instead of
// a chain of dependent global loads; each token's first-frame emission is loaded one token
// ahead.  Needs T + N floats of `lds`; every thread of the workgroup calls it.
__device__ void merge_tokens_lds(const float* __restrict__ E, int V, const int32_t* __restrict__ tok, int N, int T,
                                 int t_start, const float* __restrict__ q0, const int32_t* __restrict__ start,
                                 int32_t* __restrict__ seg_end, double* __restrict__ seg_score, float* lds) {
    float* qs = lds;
    int* ss = reinterpret_cast<int*>(lds + T);
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    constexpr int kB = 8;
    for (int base = tid; base < T; base += kB * nthr) {
        float v[kB];
#pragma unroll
        for (int u = 0; u < kB; ++u) v[u] = q0[min(base + u * nthr, T - 1)];
#pragma unroll
        for (int u = 0; u < kB; ++u)
            if (base + u * nthr < T) qs[base + u * nthr] = v[u];
    }
    for (int base = tid; base < N; base += kB * nthr) {
        int v[kB];
#pragma unroll
        for (int u = 0; u < kB; ++u) v[u] = start[min(base + u * nthr, N - 1)];
#pragma unroll
        for (int u = 0; u < kB; ++u)
            if (base + u * nthr < N) ss[base + u * nthr] = v[u];
    }
    block_fence();
    auto first = [&](int k) {  // em[start_k, tok_k] (clamped: an unconditional load)
        const int kk = min(k, N - 1);
        int tk = tok[kk];
        tk = (tk >= 0 && tk < V) ? tk : 0;
        return E[(int64_t)ss[kk] * V + tk];
    };
    float e_next = first(tid);
    for (int k = tid; k < N; k += nthr) {
        const float e_cur = e_next;
        e_next = first(k + nthr);
        const int s = ss[k];
        const int e = (k + 1 < N) ? ss[k + 1] : t_start;
        double sum = (double)exp_cr(e_cur);
        for (int x = s + 1; x < e; ++x) sum += (double)qs[x];
        seg_end[k] = e;
        seg_score[k] = sum / (double)(e - s);
    }
}

}  // namespace wx

#endif  // WX_DP_TAIL_H
