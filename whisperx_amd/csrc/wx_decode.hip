// wx_decode.hip — attention of one decode step of Whisper's text decoder (whisperx/asr.py:53-62: the
// reference hands the encoder output to CTranslate2's generate; the arithmetic is transformers'
// WhisperDecoder.forward with its cache): every (batch, head) has ONE query row, which attends to L
// key / value rows read in place through their strides (the self-attention cache, or the two halves
// of the cross-attention [B, P, 2D] GEMM output).  C ABI and semantics: include/wx_align.h
// (wx_decode_attention_f32).
//
// The work is a read of 2 L rows of 256 bytes per (batch, head) and nothing else, so the key range
// is split over workgroups ("flash-decoding"):
//   - The keys are cut into chunks of kChunk = 128 rows: a constant, so neither the chunking nor
//     the merge order depends on B or H, and row (b, h) is bit-identical whatever the batch is.
//   - One block of 4 waves per (chunk, head, batch).  A 16-lane group reads one 64-float row as
//     16 float4, a wave 4 consecutive rows per load (1 KB when the rows are contiguous), the block
//     16 rows per pass and the chunk in 8 passes.  All 8 key loads and all 8 value loads of a lane
//     are issued before the first use (16 x 16 bytes in flight per lane).
//   - A group computes its 8 scores (4 products per lane, then a DPP butterfly over the 16 lanes
//     that leaves the same sum in each of them), their maximum and exponentials, and its partial
//     (m, l, acc[64]).  The 16 groups' partials are merged through LDS in group order by wave 0 and
//     written to the workspace as the chunk's (m, l, acc[64]); with a single chunk the block writes
//     o = acc / l itself.
//   - A second launch (one wave per (batch, head)) merges the chunks in chunk order.
// No atomics, no hand-shake between blocks: two plain launches on the stream.
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wx_host.h"  // (and through it include/wx_align.h)

namespace wxdec {

constexpr int kHead = 64;                       // head dim
constexpr int kChunk = WX_DECODE_ATTENTION_CHUNK;  // keys per block
constexpr int kGroups = 16;                     // 16-lane groups per block (4 waves x 4)
constexpr int kPasses = kChunk / kGroups;       // rows per group
static_assert(kChunk % kGroups == 0, "a chunk is a whole number of passes");

struct DecArgs {
    const float *q, *k, *v;
    float* o;
    float2* ml;   // [B H nc] (m, l) of every chunk
    float* acc;   // [B H nc][64]
    int64_t qs[2], ks[3], vs[3];
    int32_t H, L, nc;
    float scale;
};

template <int CTRL>
__device__ __forceinline__ float dpp_read(float v) {  // v of the lane the DPP control names
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// The sum of x over the 16 lanes of a DPP row, the same bits in every lane: each step adds the
// partner's value, and the two partners of a step hold the same pair of values (a + b == b + a).
__device__ __forceinline__ float row16_sum(float x) {
    x += dpp_read<0xB1>(x);   // quad_perm [1, 0, 3, 2]
    x += dpp_read<0x4E>(x);   // quad_perm [2, 3, 0, 1]
    x += dpp_read<0x141>(x);  // row_half_mirror: a lane of the other quad of the 8
    x += dpp_read<0x140>(x);  // row_mirror: a lane of the other half of the 16
    return x;
}

__global__ __launch_bounds__(256) void decode_chunk_kernel(const DecArgs a) {
    __shared__ float s_m[kGroups], s_l[kGroups];
    __shared__ __attribute__((aligned(16))) float s_acc[kGroups][kHead];
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x;
    const int grp = tid >> 4, d4 = (tid & 15) * 4;
    const int j0 = c * kChunk;  // (< L <= 2^31 - 1)
    const int n = min(kChunk, a.L - j0);  // rows of this chunk, >= 1

    const float4 qv = *reinterpret_cast<const float4*>(a.q + (int64_t)b * a.qs[0] + (int64_t)h * a.qs[1] + d4);
    const float* kb = a.k + (int64_t)b * a.ks[0] + (int64_t)h * a.ks[1] + (int64_t)j0 * a.ks[2] + d4;
    const float* vb = a.v + (int64_t)b * a.vs[0] + (int64_t)h * a.vs[1] + (int64_t)j0 * a.vs[2] + d4;

    // pass i of group grp: row 16 i + grp of the chunk
    float4 kr[kPasses], vr[kPasses];
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        const int r = kGroups * i + grp;
        kr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) kr[i] = *reinterpret_cast<const float4*>(kb + (int64_t)r * a.ks[2]);
    }
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        const int r = kGroups * i + grp;
        vr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) vr[i] = *reinterpret_cast<const float4*>(vb + (int64_t)r * a.vs[2]);
    }

    float s[kPasses];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        const float part = (qv.x * kr[i].x + qv.y * kr[i].y) + (qv.z * kr[i].z + qv.w * kr[i].w);
        s[i] = kGroups * i + grp < n ? a.scale * row16_sum(part) : -INFINITY;
        m = fmaxf(m, s[i]);
    }
    // a group past the chunk's end (m = -inf) contributes l = 0, acc = 0
    float l = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m > -INFINITY) {
#pragma unroll
        for (int i = 0; i < kPasses; ++i) {
            const float p = expf(s[i] - m);  // exp(-inf) = 0 for the rows past n
            l += p;
            acc.x += p * vr[i].x;
            acc.y += p * vr[i].y;
            acc.z += p * vr[i].z;
            acc.w += p * vr[i].w;
        }
    }
    if ((tid & 15) == 0) {
        s_m[grp] = m;
        s_l[grp] = l;
    }
    *reinterpret_cast<float4*>(&s_acc[grp][d4]) = acc;
    __syncthreads();
    if (tid >= kHead) return;

    // wave 0, lane = dim: the 16 groups in group order (group 0 always has row 0: M is finite)
    float M = s_m[0];
#pragma unroll
    for (int g = 1; g < kGroups; ++g) M = fmaxf(M, s_m[g]);
    float Lsum = 0.f, out = 0.f;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const float w = expf(s_m[g] - M);
        Lsum += w * s_l[g];
        out += w * s_acc[g][tid];
    }
    const int64_t bh = (int64_t)b * a.H + h;
    if (a.nc == 1) {
        a.o[bh * kHead + tid] = out / Lsum;
        return;
    }
    const int64_t slot = bh * a.nc + c;
    if (tid == 0) a.ml[slot] = make_float2(M, Lsum);
    a.acc[slot * kHead + tid] = out;
}

// one wave per (batch, head), lane = dim: the chunks in chunk order
__global__ __launch_bounds__(256) void decode_merge_kernel(const DecArgs a, int64_t BH) {
    const int64_t bh = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int d = threadIdx.x & 63;
    if (bh >= BH) return;
    const float2* ml = a.ml + bh * a.nc;
    const float* acc = a.acc + bh * a.nc * kHead;
    float M = -INFINITY;
    for (int c = 0; c < a.nc; ++c) M = fmaxf(M, ml[c].x);
    float Lsum = 0.f, out = 0.f;
    for (int c = 0; c < a.nc; ++c) {
        const float2 p = ml[c];
        const float w = expf(p.x - M);
        Lsum += w * p.y;
        out += w * acc[(int64_t)c * kHead + d];
    }
    a.o[bh * kHead + d] = out / Lsum;
}

// ------------------------------------------------------------------------------ grouped
// The G queries of one batch entry (the beams of one audio chunk) share its keys and values: the
// block loads its 2 x 128 rows once, as above, and then runs the per-query arithmetic of
// decode_chunk_kernel G times on the rows it holds, expression for expression, so that row (b, g, h)
// has the bits the ungrouped kernel gives that query.  The G queries wait in LDS (one 16-byte load
// per lane of the first G 16-lane groups, issued behind the key / value loads); the 16 groups'
// partials of every query go to LDS (G x 4.1 KB, sized by the launch) and wave w merges the queries
// w, w + 4, ... in group order.  The workspace slots are those of B G H ungrouped rows, and
// decode_merge_kernel merges the chunks.
constexpr int kMaxGroup = WX_DECODE_ATTENTION_MAX_GROUP;

struct GrpArgs {
    DecArgs d;       // (qs unused: the grouped strides are qs3)
    int64_t qs3[3];  // b, g, h
    int32_t G;
};

__global__ __launch_bounds__(256) void decode_chunk_grouped_kernel(const GrpArgs ga) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    const DecArgs& a = ga.d;
    const int G = ga.G;
    float* s_q = s_dyn;                        // [G][64]
    float* s_acc = s_q + G * kHead;            // [G][16][64]
    float* s_m = s_acc + G * kGroups * kHead;  // [G][16]
    float* s_l = s_m + G * kGroups;            // [G][16]
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x;
    const int grp = tid >> 4, d4 = (tid & 15) * 4;
    const int j0 = c * kChunk;
    const int n = min(kChunk, a.L - j0);

    const float* kb = a.k + (int64_t)b * a.ks[0] + (int64_t)h * a.ks[1] + (int64_t)j0 * a.ks[2] + d4;
    const float* vb = a.v + (int64_t)b * a.vs[0] + (int64_t)h * a.vs[1] + (int64_t)j0 * a.vs[2] + d4;

    float4 kr[kPasses], vr[kPasses];
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        const int r = kGroups * i + grp;
        kr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) kr[i] = *reinterpret_cast<const float4*>(kb + (int64_t)r * a.ks[2]);
    }
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        const int r = kGroups * i + grp;
        vr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) vr[i] = *reinterpret_cast<const float4*>(vb + (int64_t)r * a.vs[2]);
    }
    if (grp < G)  // query grp of this (batch, head)
        *reinterpret_cast<float4*>(s_q + grp * kHead + d4) = *reinterpret_cast<const float4*>(
            a.q + (int64_t)b * ga.qs3[0] + (int64_t)grp * ga.qs3[1] + (int64_t)h * ga.qs3[2] + d4);
    __syncthreads();

    for (int g = 0; g < G; ++g) {
        const float4 qv = *reinterpret_cast<const float4*>(s_q + g * kHead + d4);
        float s[kPasses];
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < kPasses; ++i) {
            const float part = (qv.x * kr[i].x + qv.y * kr[i].y) + (qv.z * kr[i].z + qv.w * kr[i].w);
            s[i] = kGroups * i + grp < n ? a.scale * row16_sum(part) : -INFINITY;
            m = fmaxf(m, s[i]);
        }
        float l = 0.f;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m > -INFINITY) {
#pragma unroll
            for (int i = 0; i < kPasses; ++i) {
                const float p = expf(s[i] - m);
                l += p;
                acc.x += p * vr[i].x;
                acc.y += p * vr[i].y;
                acc.z += p * vr[i].z;
                acc.w += p * vr[i].w;
            }
        }
        if ((tid & 15) == 0) {
            s_m[g * kGroups + grp] = m;
            s_l[g * kGroups + grp] = l;
        }
        *reinterpret_cast<float4*>(s_acc + (g * kGroups + grp) * kHead + d4) = acc;
    }
    __syncthreads();

    // wave w, lane = dim: the queries w, w + 4, ..., each over its 16 groups in group order
    const int d = tid & 63;
    for (int g = tid >> 6; g < G; g += 4) {
        const float* gm = s_m + g * kGroups;
        const float* gl = s_l + g * kGroups;
        const float* gacc = s_acc + g * kGroups * kHead;
        float M = gm[0];
#pragma unroll
        for (int u = 1; u < kGroups; ++u) M = fmaxf(M, gm[u]);
        float Lsum = 0.f, out = 0.f;
#pragma unroll
        for (int u = 0; u < kGroups; ++u) {
            const float w = expf(gm[u] - M);
            Lsum += w * gl[u];
            out += w * gacc[u * kHead + d];
        }
        const int64_t bgh = ((int64_t)b * G + g) * a.H + h;
        if (a.nc == 1) {
            a.o[bgh * kHead + d] = out / Lsum;
        } else {
            const int64_t slot = bgh * a.nc + c;
            if (d == 0) a.ml[slot] = make_float2(M, Lsum);
            a.acc[slot * kHead + d] = out;
        }
    }
}

inline int64_t chunks(int32_t L) { return ((int64_t)L + kChunk - 1) / kChunk; }

// The workspace's layout, stated once: measures on a null base, fills `a` on the caller's pointer.
inline size_t carve(void* base, int32_t B, int32_t H, int32_t L, DecArgs* a) {
    wx::Carver cv{base};
    const size_t slots = (size_t)(B > 0 ? B : 0) * (size_t)(H > 0 ? H : 0) * (size_t)(L > 0 ? chunks(L) : 0);
    float2* ml = cv.take<float2>(slots > 0 ? slots : 1);
    float* acc = cv.take<float>((slots > 0 ? slots : 1) * kHead);
    if (a) {
        a->ml = ml;
        a->acc = acc;
    }
    return cv.off;
}

}  // namespace wxdec

extern "C" size_t wx_decode_attention_workspace_bytes(int32_t B, int32_t H, int32_t L) {
    return wxdec::carve(nullptr, B, H, L, nullptr);
}

extern "C" int wx_decode_attention_f32(const float* q, const float* k, const float* v, float* o, int32_t B, int32_t H,
                                       int32_t L, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                                       const int64_t* v_strides, float scale, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    using namespace wxdec;
    if (B < 0 || H < 1 || L < 1 || D != kHead) return WX_E_INVALID;
    if (B == 0) return WX_OK;
    if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides || !workspace) return WX_E_INVALID;
    for (const void* p : {(const void*)q, (const void*)k, (const void*)v, (const void*)o, (const void*)workspace})
        if (reinterpret_cast<uintptr_t>(p) & 15) return WX_E_INVALID;
    // 16-byte aligned rows: every stride a multiple of 4 floats; a row stride holds the head dim
    for (int i = 0; i < 2; ++i)
        if (q_strides[i] % 4) return WX_E_INVALID;
    for (int i = 0; i < 3; ++i)
        if (k_strides[i] % 4 || v_strides[i] % 4) return WX_E_INVALID;
    if (B > 65535 || H > 65535) return WX_E_INVALID;  // grid y / z
    if ((int64_t)B * H * chunks(L) > ((int64_t)1 << 40)) return WX_E_INVALID;  // (the workspace size stays in range)
    DecArgs a;
    if (workspace_bytes < carve(workspace, B, H, L, &a)) return WX_E_WORKSPACE;
    a.q = q;
    a.k = k;
    a.v = v;
    a.o = o;
    for (int i = 0; i < 2; ++i) a.qs[i] = q_strides[i];
    for (int i = 0; i < 3; ++i) {
        a.ks[i] = k_strides[i];
        a.vs[i] = v_strides[i];
    }
    a.H = H;
    a.L = L;
    a.nc = (int32_t)chunks(L);
    a.scale = scale;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(decode_chunk_kernel, dim3((unsigned)a.nc, (unsigned)H, (unsigned)B), dim3(256), 0, st, a);
    if (a.nc > 1) {
        const int64_t BH = (int64_t)B * H;  // (<= 65535^2: the merge grid's x fits)
        hipLaunchKernelGGL(decode_merge_kernel, dim3((unsigned)((BH + 3) / 4)), dim3(256), 0, st, a, BH);
    }
    return wx::launch_status();
}

extern "C" size_t wx_decode_attention_grouped_workspace_bytes(int32_t B, int32_t G, int32_t H, int32_t L) {
    const bool ok = B > 0 && G >= 1 && G <= wxdec::kMaxGroup && B <= 65535;
    return wxdec::carve(nullptr, ok ? B * G : 0, H, L, nullptr);
}

extern "C" int wx_decode_attention_f32_grouped(const float* q, const float* k, const float* v, float* o, int32_t B,
                                               int32_t G, int32_t H, int32_t L, int32_t D, const int64_t* q_strides,
                                               const int64_t* k_strides, const int64_t* v_strides, float scale,
                                               void* workspace, size_t workspace_bytes, void* stream) {
    using namespace wxdec;
    if (B < 0 || G < 1 || G > kMaxGroup || H < 1 || L < 1 || D != kHead) return WX_E_INVALID;
    if (B == 0) return WX_OK;
    if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides || !workspace) return WX_E_INVALID;
    for (const void* p : {(const void*)q, (const void*)k, (const void*)v, (const void*)o, (const void*)workspace})
        if (reinterpret_cast<uintptr_t>(p) & 15) return WX_E_INVALID;
    for (int i = 0; i < 3; ++i)
        if (q_strides[i] % 4 || k_strides[i] % 4 || v_strides[i] % 4) return WX_E_INVALID;
    if (B > 65535 || H > 65535) return WX_E_INVALID;  // grid y / z
    if ((int64_t)B * G * H * chunks(L) > ((int64_t)1 << 40)) return WX_E_INVALID;
    GrpArgs ga;
    DecArgs& a = ga.d;
    if (workspace_bytes < carve(workspace, B * G, H, L, &a)) return WX_E_WORKSPACE;
    a.q = q;
    a.k = k;
    a.v = v;
    a.o = o;
    a.qs[0] = a.qs[1] = 0;
    for (int i = 0; i < 3; ++i) {
        ga.qs3[i] = q_strides[i];
        a.ks[i] = k_strides[i];
        a.vs[i] = v_strides[i];
    }
    ga.G = G;
    a.H = H;
    a.L = L;
    a.nc = (int32_t)chunks(L);
    a.scale = scale;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = (size_t)G * (kHead + kGroups * kHead + 2 * kGroups) * sizeof(float);  // (<= 35 KB)
    hipLaunchKernelGGL(decode_chunk_grouped_kernel, dim3((unsigned)a.nc, (unsigned)H, (unsigned)B), dim3(256), lds, st, ga);
    if (a.nc > 1) {
        const int64_t BH = (int64_t)B * G * H;  // (<= 8 x 65535^2: the merge grid's x fits)
        hipLaunchKernelGGL(decode_merge_kernel, dim3((unsigned)((BH + 3) / 4)), dim3(256), 0, st, a, BH);
    }
    return wx::launch_status();
}
