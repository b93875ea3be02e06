// wx_beam.hip — the selection of one beam-search step (WhisperDecoder.beam_search; the reference
// decodes with beam_size 5, whisperx/asr.py:301-304): for every chunk the 2G best of its G V
// candidates cum[r] + log_softmax(x[r])[t].  C ABI and semantics: include/wx_align.h (wx_beam_topk).
//
// Within a row the score cum + (x - lse) never decreases with x (both roundings are monotone), and
// the order among equal scores of one row is "higher logit, then lower t": so a row's 2G best
// candidates are its 2G best logits under (logit descending, t ascending), which needs no lse.
//   - slice_kernel, one block of 4 waves per (slice of 4096 columns, row): a wave holds 1024
//     columns, 16 per lane (column = base + 64 e + lane: coalesced dwords, no alignment asked of the
//     row stride).  It computes its maximum and its sum of exp(x - max), then K = 2G rounds of "the
//     best entry after the previous winner" (a scan of the lane's 16 registers and a 6-step butterfly
//     on (value, column)); the order is total, so "after the previous winner" needs no removal.
//     Wave 0 merges the 4 waves' K entries (one per lane) the same way and their (m, l) in wave order.
//   - merge_kernel, one block of G waves per chunk: wave g combines the slices' (m, l) of row b G + g
//     into lse, picks the row's K best of its slices' entries, and scores them; wave 0 then picks the
//     chunk's 2G best of the G K scored entries under the full order (score descending, lower g,
//     higher logit, lower t).
// Nothing depends on B; every sum has one fixed order; no atomics.
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wx_host.h"  // (and through it include/wx_align.h)

namespace wxbeam {

constexpr int kMaxGroup = 8;
constexpr int kMaxK = 2 * kMaxGroup;         // entries kept per slice and per row
constexpr int kSlice = WX_BEAM_TOPK_SLICE;   // columns per block
constexpr int kWaveCols = kSlice / 4;        // columns per wave
constexpr int kPerLane = kWaveCols / 64;     // columns per lane
constexpr int kNone = INT32_MAX;             // the column of "no entry": after every real one
constexpr int kMaxV = 1 << 24;               // (g V + t stays an int32; at most 4096 slices)
static_assert(kPerLane * 64 * 4 == kSlice && 4 * kMaxK == 64, "wave 0 holds the 4 waves' entries one per lane");

struct TopkArgs {
    const float *x, *cum;
    int64_t stride;
    int32_t G, V, ns, K;
    float2* ml;  // [B G][ns] (m, l) of every slice
    float* cv;   // [B G][ns][16] the slice's best logits, best first
    int32_t* cc;  // ... and their columns (kNone: fewer than K columns)
    float* scores;
    int32_t* index;
};

// (v, c) before (w, d): higher logit, then lower column
__device__ __forceinline__ bool before(float v, int c, float w, int d) { return v > w || (v == w && c < d); }

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int o = 32; o; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}
// the same bits in every lane: the two partners of a step add the same pair of values
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
// the first of the 64 lanes' entries; every lane gets it (the order is total on real entries, and
// "none" entries are equal)
__device__ __forceinline__ void wave_first(float& v, int& c) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const float w = __shfl_xor(v, o, 64);
        const int d = __shfl_xor(c, o, 64);
        if (before(w, d, v, c)) {
            v = w;
            c = d;
        }
    }
}

__global__ __launch_bounds__(256) void slice_kernel(const TopkArgs a) {
    __shared__ float s_v[4][kMaxK], s_m[4], s_l[4];
    __shared__ int s_c[4][kMaxK];
    const int s = blockIdx.x, r = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* row = a.x + (int64_t)r * a.stride;
    const int base = s * kSlice + w * kWaveCols + lane;  // (< 2^24 + 4096)

    float x[kPerLane];
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
        const int col = base + 64 * e;
        x[e] = col < a.V ? row[col] : -INFINITY;
    }
    float m = x[0];
#pragma unroll
    for (int e = 1; e < kPerLane; ++e) m = fmaxf(m, x[e]);
    m = wave_max(m);
    float l = 0.f;
    if (m > -INFINITY) {  // (all -inf: l = 0, and no exp(-inf + inf))
#pragma unroll
        for (int e = 0; e < kPerLane; ++e) l += expf(x[e] - m);  // exp(-inf) = 0 for the columns past V
    }
    l = wave_sum(l);

    // round k: the best entry after the previous winner (pv, pc); lane k keeps it
    float pv = INFINITY, mine_v = -INFINITY;
    int pc = -1, mine_c = kNone;
    for (int k = 0; k < a.K; ++k) {
        float bv = -INFINITY;
        int bc = kNone;
#pragma unroll
        for (int e = 0; e < kPerLane; ++e) {
            const int col = base + 64 * e;
            if (col < a.V && before(pv, pc, x[e], col) && before(x[e], col, bv, bc)) {
                bv = x[e];
                bc = col;
            }
        }
        wave_first(bv, bc);
        if (lane == k) {
            mine_v = bv;
            mine_c = bc;
        }
        pv = bv;
        pc = bc;
    }
    if (lane < kMaxK) {
        s_v[w][lane] = mine_v;
        s_c[w][lane] = mine_c;
    }
    if (lane == 0) {
        s_m[w] = m;
        s_l[w] = l;
    }
    __syncthreads();
    if (w) return;

    // wave 0: lane 16 w' + j holds entry j of wave w'
    const float ev = s_v[lane >> 4][lane & 15];
    const int ec = s_c[lane >> 4][lane & 15];
    const int64_t slot = (int64_t)r * a.ns + s;
    pv = INFINITY;
    pc = -1;
    mine_v = -INFINITY;
    mine_c = kNone;
    for (int k = 0; k < a.K; ++k) {
        float bv = -INFINITY;
        int bc = kNone;
        if (ec != kNone && before(pv, pc, ev, ec)) {
            bv = ev;
            bc = ec;
        }
        wave_first(bv, bc);
        if (lane == k) {
            mine_v = bv;
            mine_c = bc;
        }
        pv = bv;
        pc = bc;
    }
    if (lane < kMaxK) {
        a.cv[slot * kMaxK + lane] = mine_v;
        a.cc[slot * kMaxK + lane] = mine_c;
    }
    if (lane == 0) {
        float M = s_m[0];
#pragma unroll
        for (int u = 1; u < 4; ++u) M = fmaxf(M, s_m[u]);
        float L = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (s_m[u] > -INFINITY) L += expf(s_m[u] - M) * s_l[u];
        a.ml[slot] = make_float2(M, L);
    }
}

// a scored entry (s, g, x, t) before (s2, g2, x2, t2): the order of the output
__device__ __forceinline__ bool before4(float s, int g, float x, int t, float s2, int g2, float x2, int t2) {
    if (s != s2) return s > s2;
    if (g != g2) return g < g2;
    return before(x, t, x2, t2);
}

__global__ __launch_bounds__(64 * kMaxGroup) void merge_kernel(const TopkArgs a) {
    __shared__ float s_s[kMaxGroup * kMaxK], s_x[kMaxGroup * kMaxK];
    __shared__ int s_t[kMaxGroup * kMaxK];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;  // wave g: row b G + g
    const int K = a.K;
    {
        const int64_t r = (int64_t)b * a.G + g;
        const float2* ml = a.ml + r * a.ns;
        float M = -INFINITY;
        for (int s = lane; s < a.ns; s += 64) M = fmaxf(M, ml[s].x);
        M = wave_max(M);
        float L = 0.f;
        for (int s = lane; s < a.ns; s += 64) {
            const float2 p = ml[s];
            if (p.x > -INFINITY) L += expf(p.x - M) * p.y;
        }
        L = wave_sum(L);
        const float lse = M + logf(L);

        const float* cv = a.cv + r * a.ns * kMaxK;
        const int32_t* cc = a.cc + r * a.ns * kMaxK;
        const int n = a.ns * kMaxK;
        float pv = INFINITY, mine_v = -INFINITY;
        int pc = -1, mine_c = kNone;
        for (int k = 0; k < K; ++k) {
            float bv = -INFINITY;
            int bc = kNone;
            for (int i = lane; i < n; i += 64) {
                if ((i & (kMaxK - 1)) >= K) continue;
                const float v = cv[i];
                const int c = cc[i];
                if (c != kNone && before(pv, pc, v, c) && before(v, c, bv, bc)) {
                    bv = v;
                    bc = c;
                }
            }
            wave_first(bv, bc);
            if (lane == k) {
                mine_v = bv;
                mine_c = bc;
            }
            pv = bv;
            pc = bc;
        }
        if (lane < K) {  // (V >= 2G: the row has K real entries)
            const float cum = a.cum[r];
            // a suppressed id or a dead beam scores -inf (also where the row's lse is -inf)
            s_s[g * kMaxK + lane] = (mine_v == -INFINITY || cum == -INFINITY) ? -INFINITY : cum + (mine_v - lse);
            s_x[g * kMaxK + lane] = mine_v;
            s_t[g * kMaxK + lane] = mine_c;
        }
    }
    __syncthreads();
    if (g) return;

    // wave 0: the G K scored entries, two per lane, in 2G rounds under the full order
    float es[2], ex[2];
    int eg[2], et[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = lane + 64 * u;
        const bool real = (i >> 4) < a.G && (i & 15) < K;
        es[u] = real ? s_s[i] : -INFINITY;
        ex[u] = real ? s_x[i] : -INFINITY;
        eg[u] = real ? i >> 4 : kNone;
        et[u] = real ? s_t[i] : kNone;
    }
    float ps = INFINITY, px = INFINITY;
    int pg = -1, pt = -1;
    for (int k = 0; k < K; ++k) {
        float bs = -INFINITY, bx = -INFINITY;
        int bg = kNone, bt = kNone;
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (eg[u] != kNone && before4(ps, pg, px, pt, es[u], eg[u], ex[u], et[u]) &&
                before4(es[u], eg[u], ex[u], et[u], bs, bg, bx, bt)) {
                bs = es[u];
                bg = eg[u];
                bx = ex[u];
                bt = et[u];
            }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const float s2 = __shfl_xor(bs, o, 64), x2 = __shfl_xor(bx, o, 64);
            const int g2 = __shfl_xor(bg, o, 64), t2 = __shfl_xor(bt, o, 64);
            if (before4(s2, g2, x2, t2, bs, bg, bx, bt)) {
                bs = s2;
                bg = g2;
                bx = x2;
                bt = t2;
            }
        }
        if (lane == k) {  // (G V >= 2G candidates: the winner is real)
            a.scores[(int64_t)b * K + k] = bs;
            a.index[(int64_t)b * K + k] = bg * a.V + bt;
        }
        ps = bs;
        pg = bg;
        px = bx;
        pt = bt;
    }
}

inline int32_t slices(int32_t V) { return (V + kSlice - 1) / kSlice; }

// The workspace's layout, stated once: measures on a null base, fills `a` on the caller's pointer.
inline size_t carve(void* base, int32_t B, int32_t G, int32_t V, TopkArgs* a) {
    wx::Carver cv{base};
    const bool ok = B > 0 && G >= 1 && G <= kMaxGroup && V >= 1 && V <= kMaxV;
    const size_t slots = ok ? (size_t)B * (size_t)G * (size_t)slices(V) : 1;
    float2* ml = cv.take<float2>(slots);
    float* v = cv.take<float>(slots * kMaxK);
    int32_t* c = cv.take<int32_t>(slots * kMaxK);
    if (a) {
        a->ml = ml;
        a->cv = v;
        a->cc = c;
    }
    return cv.off;
}

}  // namespace wxbeam

extern "C" size_t wx_beam_topk_workspace_bytes(int32_t B, int32_t G, int32_t V) {
    return wxbeam::carve(nullptr, B, G, V, nullptr);
}

extern "C" int wx_beam_topk(const float* logits, int64_t row_stride, const float* cum, int32_t B, int32_t G, int32_t V,
                            float* scores, int32_t* index, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace wxbeam;
    if (B < 0 || G < 1 || G > kMaxGroup || V < 2 * G || V > kMaxV || row_stride < V) return WX_E_INVALID;
    if (B == 0) return WX_OK;
    if (!logits || !cum || !scores || !index || !workspace) return WX_E_INVALID;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return WX_E_INVALID;
    if ((int64_t)B * G > 65535) return WX_E_INVALID;  // grid y
    TopkArgs a;
    if (workspace_bytes < carve(workspace, B, G, V, &a)) return WX_E_WORKSPACE;
    a.x = logits;
    a.cum = cum;
    a.stride = row_stride;
    a.G = G;
    a.V = V;
    a.ns = slices(V);
    a.K = 2 * G;
    a.scores = scores;
    a.index = index;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(slice_kernel, dim3((unsigned)a.ns, (unsigned)(B * G)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)B), dim3(64 * (unsigned)G), 0, st, a);
    return wx::launch_status();
}
