// wx_sample.hip — the selection of one greedy or sampled decoding step (WhisperDecoder.sample; the
// reference's temperature fallback, whisperx/asr.py:305-312): per row the mask, the argmax or the
// Gumbel-max sample, the token's log-probability and the done / eot handling, in one pass over the
// logits.  C ABI and semantics: include/wx_align.h (wx_sample_token).
//
//   - slice_kernel, one block of 4 waves per (slice of 4096 columns, row): a wave holds 1024 columns
//     as 256 groups of 4 consecutive columns, 4 groups per lane (group = 64 e + lane: a lane's four
//     dwords are adjacent, no alignment asked of the row stride).  One Philox4x32-10 block per group
//     gives the four columns' uniforms.  The wave computes its maximum of the masked logits, its sum
//     of exp(m - max) and its best (z, column, logit); lane 0 of wave 0 merges the 4 waves in order.
//   - merge_kernel, one wave per row: combines the slices' (max, sum) into lse and their best
//     entries into the row's, then writes token, logprob, sum_logprob and done.
// A row that is done on entry launches its blocks, which return at once.  Nothing depends on R;
// every sum has one fixed order; no atomics.
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wx_host.h"  // (and through it include/wx_align.h)

namespace wxsample {

constexpr int kSlice = WX_SAMPLE_TOKEN_SLICE;  // columns per block
constexpr int kWaveCols = kSlice / 4;          // columns per wave
constexpr int kGroups = kWaveCols / 256;       // groups of 4 columns per lane
constexpr int kNone = INT32_MAX;               // the column of "no entry": after every real one
constexpr int kMaxV = 1 << 24;                 // (at most 4096 slices; a group index stays below 2^22)
static_assert(kGroups * 256 * 4 == kSlice, "a wave holds whole groups, one per lane and round");

struct Args {
    const float* x;
    int64_t stride;
    int32_t V, ns;
    const uint8_t* suppress;
    float temperature;
    uint32_t key0, key1;
    const int64_t* step;
    int64_t eot;
    uint8_t* done;
    int64_t* token;
    float *logprob, *sum;
    float4* part;  // [R][ns] (max, sum of exp, best z, its logit) of every slice
    int32_t* col;  // ... and the best entry's column (kNone: the slice has no column)
};

// (z, c) before (w, d): higher z, then lower column
__device__ __forceinline__ bool before(float z, int c, float w, int d) { return z > w || (z == w && c < d); }

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
// the first of the 64 lanes' entries (with its logit); every lane gets it
__device__ __forceinline__ void wave_first(float& z, int& c, float& x) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const float w = __shfl_xor(z, o, 64), y = __shfl_xor(x, o, 64);
        const int d = __shfl_xor(c, o, 64);
        if (before(w, d, z, c)) {
            z = w;
            c = d;
            x = y;
        }
    }
}

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key (k0, k1); c becomes the output block
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
        const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += W0;
        k1 += W1;
    }
}

// g = -log(-log(u)), u = ((x >> 9) + 0.5) 2^-23 in (0, 1): exact in fp32, never 0 or 1
__device__ __forceinline__ float gumbel(uint32_t x) {
    const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f;
    return -logf(-logf(u));
}

__global__ __launch_bounds__(256) void slice_kernel(const Args a) {
    __shared__ float s_m[4], s_l[4], s_z[4], s_x[4];
    __shared__ int s_c[4];
    const int s = blockIdx.x, r = blockIdx.y;
    if (a.done[r]) return;  // (the whole block: the merge writes eot without reading this row's slots)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* row = a.x + (int64_t)r * a.stride;
    const uint64_t step = (uint64_t)*a.step;
    const bool sample = a.temperature > 0.f;

    float x[4 * kGroups];
    float bz = -INFINITY, bx = -INFINITY;
    int bc = kNone;
#pragma unroll
    for (int e = 0; e < kGroups; ++e) {
        const int q = s * (kSlice / 4) + w * (kWaveCols / 4) + 64 * e + lane;  // the group: columns 4q .. 4q + 3
        uint32_t u[4] = {(uint32_t)q, (uint32_t)r, (uint32_t)step, (uint32_t)(step >> 32)};
        if (sample && 4 * q < a.V) philox4x32_10(u, a.key0, a.key1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 4 * q + j;
            float v = -INFINITY;
            if (col < a.V) {
                v = row[col];
                if (a.suppress && a.suppress[col]) v = -INFINITY;
                const float z = sample ? v / a.temperature + gumbel(u[j]) : v;
                if (before(z, col, bz, bc)) {
                    bz = z;
                    bc = col;
                    bx = v;
                }
            }
            x[4 * e + j] = v;
        }
    }
    float m = x[0];
#pragma unroll
    for (int i = 1; i < 4 * kGroups; ++i) m = fmaxf(m, x[i]);
    m = wave_max(m);
    float l = 0.f;
    if (m > -INFINITY) {  // (all -inf: l = 0, and no exp(-inf + inf))
#pragma unroll
        for (int i = 0; i < 4 * kGroups; ++i) l += expf(x[i] - m);  // exp(-inf) = 0: masked and past V
    }
    l = wave_sum(l);
    wave_first(bz, bc, bx);
    if (lane == 0) {
        s_m[w] = m;
        s_l[w] = l;
        s_z[w] = bz;
        s_c[w] = bc;
        s_x[w] = bx;
    }
    __syncthreads();
    if (threadIdx.x) return;

    float M = s_m[0];
#pragma unroll
    for (int u = 1; u < 4; ++u) M = fmaxf(M, s_m[u]);
    float L = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (s_m[u] > -INFINITY) L += expf(s_m[u] - M) * s_l[u];
        if (u && before(s_z[u], s_c[u], bz, bc)) {
            bz = s_z[u];
            bc = s_c[u];
            bx = s_x[u];
        }
    }
    const int64_t slot = (int64_t)r * a.ns + s;
    a.part[slot] = make_float4(M, L, bz, bx);
    a.col[slot] = bc;
}

__global__ __launch_bounds__(64) void merge_kernel(const Args a) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (a.done[r]) {  // a finished row: eot, 0, its sum left alone
        if (lane == 0) {
            a.token[r] = a.eot;
            a.logprob[r] = 0.f;
        }
        return;
    }
    const float4* part = a.part + (int64_t)r * a.ns;
    const int32_t* col = a.col + (int64_t)r * a.ns;
    float M = -INFINITY, bz = -INFINITY, bx = -INFINITY;
    int bc = kNone;
    for (int s = lane; s < a.ns; s += 64) {
        const float4 p = part[s];
        const int c = col[s];
        M = fmaxf(M, p.x);
        if (before(p.z, c, bz, bc)) {
            bz = p.z;
            bc = c;
            bx = p.w;
        }
    }
    M = wave_max(M);
    float L = 0.f;
    for (int s = lane; s < a.ns; s += 64) {
        const float4 p = part[s];
        if (p.x > -INFINITY) L += expf(p.x - M) * p.y;
    }
    L = wave_sum(L);
    wave_first(bz, bc, bx);
    if (lane) return;
    if (!(bx > -INFINITY)) {  // every id masked: eot, 0, done
        a.token[r] = a.eot;
        a.logprob[r] = 0.f;
        a.done[r] = 1;
        return;
    }
    const float lp = bx - (M + logf(L));
    a.token[r] = bc;
    a.logprob[r] = lp;
    if (a.sum) a.sum[r] += lp;
    if (bc == a.eot) a.done[r] = 1;
}

inline int32_t slices(int32_t V) { return (V + kSlice - 1) / kSlice; }

// The workspace's layout, stated once: measures on a null base, fills `a` on the caller's pointer.
inline size_t carve(void* base, int32_t R, int32_t V, Args* a) {
    wx::Carver cv{base};
    const bool ok = R > 0 && V >= 1 && V <= kMaxV;
    const size_t slots = ok ? (size_t)R * (size_t)slices(V) : 1;
    float4* part = cv.take<float4>(slots);
    int32_t* col = cv.take<int32_t>(slots);
    if (a) {
        a->part = part;
        a->col = col;
    }
    return cv.off;
}

}  // namespace wxsample

extern "C" size_t wx_sample_token_workspace_bytes(int32_t R, int32_t V) {
    return wxsample::carve(nullptr, R, V, nullptr);
}

extern "C" int wx_sample_token(const float* logits, int64_t row_stride, int32_t R, int32_t V, const uint8_t* suppress,
                               float temperature, uint64_t seed, const int64_t* step, int64_t eot, uint8_t* done,
                               int64_t* token, float* logprob, float* sum_logprob, void* workspace,
                               size_t workspace_bytes, void* stream) {
    using namespace wxsample;
    if (R < 0 || V < 1 || V > kMaxV || row_stride < V) return WX_E_INVALID;
    if (!(temperature >= 0.f) || isinf(temperature)) return WX_E_INVALID;
    if (eot < 0 || eot >= V) return WX_E_INVALID;
    if (R == 0) return WX_OK;
    if (!logits || !step || !done || !token || !logprob || !workspace) return WX_E_INVALID;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return WX_E_INVALID;
    if (R > 65535) return WX_E_INVALID;  // grid y
    Args a;
    if (workspace_bytes < carve(workspace, R, V, &a)) return WX_E_WORKSPACE;
    a.x = logits;
    a.stride = row_stride;
    a.V = V;
    a.ns = slices(V);
    a.suppress = suppress;
    a.temperature = temperature;
    a.key0 = (uint32_t)seed;
    a.key1 = (uint32_t)(seed >> 32);
    a.step = step;
    a.eot = eot;
    a.done = done;
    a.token = token;
    a.logprob = logprob;
    a.sum = sum_logprob;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(slice_kernel, dim3((unsigned)a.ns, (unsigned)R), dim3(256), 0, st, a);
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)R), dim3(64), 0, st, a);
    return wx::launch_status();
}
