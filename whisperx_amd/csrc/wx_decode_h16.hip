// wx_decode_h16.hip — wx_decode.hip's decode-step attention on 16-bit keys, values and queries
// (whisperx/asr.py:262: the reference loads its model with compute_type="float16", which covers the
// decoder's key / value caches and the cross-attention keys and values).  C ABI and semantics:
// include/wx_align.h (wx_decode_attention_h16, wx_decode_attention_h16_grouped).
//
// The arithmetic contract: every fp16 / bf16 element is widened to fp32 exactly, and from there
// on the kernels are decode_chunk_kernel / decode_chunk_grouped_kernel / decode_merge_kernel of
// wx_decode.hip expression for expression: a lane holds 4 head dims and forms
// (q.x k.x + q.y k.y) + (q.z k.z + q.w k.w), the same 16-lane DPP butterfly, the group's maximum,
// expf, l and acc, the merge of the 16 groups through LDS in group order, chunks of 128 keys merged
// in chunk order, one fp32 division.  The only new operation is the rounding to nearest even of
// acc / l on the store.  So o is wx_decode_attention_f32 on the widened inputs, rounded to the
// type, bit for bit, and the fp32 kernels are the oracle of these.  The contract rules out packed
// 16-bit math, dot instructions and fused multiply-adds; it also fixes the lane <-> dim mapping, so a
// lane loads 8 bytes per row (a 16-lane group one 128-byte row, a wave 4 rows) and holds its 2 x 8
// rows in 32 registers, half of the fp32 kernel's.  The partials in the workspace stay fp32 and
// the workspace is wx_decode_attention_f32's.
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wx_host.h"  // (and through it include/wx_align.h)

namespace wxdech {

typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int kHead = 64;                          // head dim
constexpr int kChunk = WX_DECODE_ATTENTION_CHUNK;  // keys per block
constexpr int kGroups = 16;                        // 16-lane groups per block (4 waves x 4)
constexpr int kPasses = kChunk / kGroups;          // rows per group
constexpr int kMaxGroup = WX_DECODE_ATTENTION_MAX_GROUP;
static_assert(kChunk % kGroups == 0, "a chunk is a whole number of passes");

struct DecArgs {
    const short *q, *k, *v;
    short* o;
    float2* ml;   // [B H nc] (m, l) of every chunk
    float* acc;   // [B H nc][64]
    int64_t qs[3], ks[3], vs[3];  // qs: {b, h} (ungrouped), {b, g, h} (grouped)
    int32_t H, L, nc, G;
    float scale;
};

// BF: bf16 (else fp16).  Bit patterns travel as shorts (as wx_attention_h16.hip); widening is exact,
// rounding is to nearest even.
template <bool BF>
__device__ __forceinline__ short round16(float x) {
    if constexpr (BF) return __builtin_bit_cast(short, (__bf16)x);
    else return __builtin_bit_cast(short, (_Float16)x);
}
template <bool BF>
__device__ __forceinline__ float widen16(short x) {
    if constexpr (BF) return __uint_as_float((unsigned)(unsigned short)x << 16);
    else return (float)__builtin_bit_cast(_Float16, x);
}
template <bool BF>
__device__ __forceinline__ float4 widen4(s16x4 x) {
    return make_float4(widen16<BF>(x[0]), widen16<BF>(x[1]), widen16<BF>(x[2]), widen16<BF>(x[3]));
}

template <int CTRL>
__device__ __forceinline__ float dpp_read(float v) {  // v of the lane the DPP control names
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// wx_decode.hip's row16_sum: the sum of x over the 16 lanes of a DPP row, the same bits in every lane
__device__ __forceinline__ float row16_sum(float x) {
    x += dpp_read<0xB1>(x);   // quad_perm [1, 0, 3, 2]
    x += dpp_read<0x4E>(x);   // quad_perm [2, 3, 0, 1]
    x += dpp_read<0x141>(x);  // row_half_mirror
    x += dpp_read<0x140>(x);  // row_mirror
    return x;
}

// The chunk's rows of one lane: pass i of group grp is row 16 i + grp, 4 elements (8 bytes) of it.
// Rows at and past n issue no load and hold zeros.
__device__ __forceinline__ void load_rows(const short* base, int64_t row_stride, int grp, int n, s16x4 (&r)[kPasses]) {
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        const int row = kGroups * i + grp;
        r[i] = s16x4{0, 0, 0, 0};
        if (row < n) r[i] = *reinterpret_cast<const s16x4*>(base + (int64_t)row * row_stride);
    }
}

// decode_chunk_kernel's per-query arithmetic on the rows a lane holds: the group's (m, l, acc)
template <bool BF>
__device__ __forceinline__ void group_partial(const float4 qv, const s16x4 (&kr)[kPasses], const s16x4 (&vr)[kPasses],
                                              int grp, int n, float scale, float& m, float& l, float4& acc) {
    float s[kPasses];
    m = -INFINITY;
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        const float4 kf = widen4<BF>(kr[i]);
        const float part = (qv.x * kf.x + qv.y * kf.y) + (qv.z * kf.z + qv.w * kf.w);
        s[i] = kGroups * i + grp < n ? scale * row16_sum(part) : -INFINITY;
        m = fmaxf(m, s[i]);
    }
    // a group past the chunk's end (m = -inf) contributes l = 0, acc = 0
    l = 0.f;
    acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m > -INFINITY) {
#pragma unroll
        for (int i = 0; i < kPasses; ++i) {
            const float p = expf(s[i] - m);  // exp(-inf) = 0 for the rows past n
            const float4 vf = widen4<BF>(vr[i]);
            l += p;
            acc.x += p * vf.x;
            acc.y += p * vf.y;
            acc.z += p * vf.z;
            acc.w += p * vf.w;
        }
    }
}

// lane = dim d: the 16 groups' partials in group order (group 0 always has row 0: M is finite)
__device__ __forceinline__ void merge_groups(const float* gm, const float* gl, const float* gacc, int d, float& M,
                                             float& Lsum, float& out) {
    M = gm[0];
#pragma unroll
    for (int u = 1; u < kGroups; ++u) M = fmaxf(M, gm[u]);
    Lsum = 0.f;
    out = 0.f;
#pragma unroll
    for (int u = 0; u < kGroups; ++u) {
        const float w = expf(gm[u] - M);
        Lsum += w * gl[u];
        out += w * gacc[u * kHead + d];
    }
}

template <bool BF>
__global__ __launch_bounds__(256) void decode_chunk_h16_kernel(const DecArgs a) {
    __shared__ float s_m[kGroups], s_l[kGroups];
    __shared__ __attribute__((aligned(16))) float s_acc[kGroups][kHead];
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x;
    const int grp = tid >> 4, d4 = (tid & 15) * 4;
    const int j0 = c * kChunk;            // (< L <= 2^31 - 1)
    const int n = min(kChunk, a.L - j0);  // rows of this chunk, >= 1

    const s16x4 qr = *reinterpret_cast<const s16x4*>(a.q + (int64_t)b * a.qs[0] + (int64_t)h * a.qs[1] + d4);
    s16x4 kr[kPasses], vr[kPasses];
    load_rows(a.k + (int64_t)b * a.ks[0] + (int64_t)h * a.ks[1] + (int64_t)j0 * a.ks[2] + d4, a.ks[2], grp, n, kr);
    load_rows(a.v + (int64_t)b * a.vs[0] + (int64_t)h * a.vs[1] + (int64_t)j0 * a.vs[2] + d4, a.vs[2], grp, n, vr);

    float m, l;
    float4 acc;
    group_partial<BF>(widen4<BF>(qr), kr, vr, grp, n, a.scale, m, l, acc);
    if ((tid & 15) == 0) {
        s_m[grp] = m;
        s_l[grp] = l;
    }
    *reinterpret_cast<float4*>(&s_acc[grp][d4]) = acc;
    __syncthreads();
    if (tid >= kHead) return;

    float M, Lsum, out;  // wave 0, lane = dim
    merge_groups(s_m, s_l, &s_acc[0][0], tid, M, Lsum, out);
    const int64_t bh = (int64_t)b * a.H + h;
    if (a.nc == 1) {
        a.o[bh * kHead + tid] = round16<BF>(out / Lsum);
        return;
    }
    const int64_t slot = bh * a.nc + c;
    if (tid == 0) a.ml[slot] = make_float2(M, Lsum);
    a.acc[slot * kHead + tid] = out;
}

// decode_merge_kernel with the rounding on its store: one wave per (batch, head), lane = dim, the
// chunks in chunk order
template <bool BF>
__global__ __launch_bounds__(256) void decode_merge_h16_kernel(const DecArgs a, int64_t BH) {
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
    a.o[bh * kHead + d] = round16<BF>(out / Lsum);
}

// decode_chunk_grouped_kernel: the block loads its 2 x 128 rows once and runs the per-query
// arithmetic above for each of the G queries of its (batch, head), which wait in LDS as fp32 (widened
// once: G x 256 bytes); wave w merges the queries w, w + 4, ... in group order.
template <bool BF>
__global__ __launch_bounds__(256) void decode_chunk_grouped_h16_kernel(const DecArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    const int G = a.G;
    float* s_q = s_dyn;                        // [G][64]
    float* s_acc = s_q + G * kHead;            // [G][16][64]
    float* s_m = s_acc + G * kGroups * kHead;  // [G][16]
    float* s_l = s_m + G * kGroups;            // [G][16]
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x;
    const int grp = tid >> 4, d4 = (tid & 15) * 4;
    const int j0 = c * kChunk;
    const int n = min(kChunk, a.L - j0);

    s16x4 kr[kPasses], vr[kPasses];
    load_rows(a.k + (int64_t)b * a.ks[0] + (int64_t)h * a.ks[1] + (int64_t)j0 * a.ks[2] + d4, a.ks[2], grp, n, kr);
    load_rows(a.v + (int64_t)b * a.vs[0] + (int64_t)h * a.vs[1] + (int64_t)j0 * a.vs[2] + d4, a.vs[2], grp, n, vr);
    if (grp < G)  // query grp of this (batch, head)
        *reinterpret_cast<float4*>(s_q + grp * kHead + d4) = widen4<BF>(*reinterpret_cast<const s16x4*>(
            a.q + (int64_t)b * a.qs[0] + (int64_t)grp * a.qs[1] + (int64_t)h * a.qs[2] + d4));
    __syncthreads();

    for (int g = 0; g < G; ++g) {
        float m, l;
        float4 acc;
        group_partial<BF>(*reinterpret_cast<const float4*>(s_q + g * kHead + d4), kr, vr, grp, n, a.scale, m, l, acc);
        if ((tid & 15) == 0) {
            s_m[g * kGroups + grp] = m;
            s_l[g * kGroups + grp] = l;
        }
        *reinterpret_cast<float4*>(s_acc + (g * kGroups + grp) * kHead + d4) = acc;
    }
    __syncthreads();

    const int d = tid & 63;
    for (int g = tid >> 6; g < G; g += 4) {
        float M, Lsum, out;
        merge_groups(s_m + g * kGroups, s_l + g * kGroups, s_acc + g * kGroups * kHead, d, M, Lsum, out);
        const int64_t bgh = ((int64_t)b * G + g) * a.H + h;
        if (a.nc == 1) {
            a.o[bgh * kHead + d] = round16<BF>(out / Lsum);
        } else {
            const int64_t slot = bgh * a.nc + c;
            if (d == 0) a.ml[slot] = make_float2(M, Lsum);
            a.acc[slot * kHead + d] = out;
        }
    }
}

inline int64_t chunks(int32_t L) { return ((int64_t)L + kChunk - 1) / kChunk; }

// wx_decode.hip's workspace layout for `rows` = B (G) query rows per head (the partials are fp32
// there and here): fills `a` on the caller's pointer and returns the bytes taken, which
// wx_decode_attention_workspace_bytes / _grouped_workspace_bytes report.
inline size_t carve(void* base, int64_t rows, int32_t H, int32_t L, DecArgs* a) {
    wx::Carver cv{base};
    const size_t slots = (size_t)rows * (size_t)H * (size_t)chunks(L);
    a->ml = cv.take<float2>(slots);
    a->acc = cv.take<float>(slots * kHead);
    return cv.off;
}

// The checks both entry points share, in the header's order; nq: q's stride count (2, grouped 3).
inline int prepare(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t G, int32_t H, int32_t L,
                   int32_t D, const int64_t* q_strides, int nq, const int64_t* k_strides, const int64_t* v_strides,
                   float scale, int32_t dtype, void* workspace, size_t workspace_bytes, DecArgs* a) {
    if (B < 0 || G < 1 || G > kMaxGroup || H < 1 || L < 1 || D != kHead ||
        (dtype != WX_DTYPE_F16 && dtype != WX_DTYPE_BF16))
        return WX_E_INVALID;
    if (B == 0) return WX_OK;
    if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides || !workspace) return WX_E_INVALID;
    for (const void* p : {q, k, v, (const void*)o, (const void*)workspace})
        if (reinterpret_cast<uintptr_t>(p) & 15) return WX_E_INVALID;
    // wx_attention_h16's rule: every stride a multiple of 8 elements (16 bytes)
    for (int i = 0; i < nq; ++i)
        if (q_strides[i] % 8) return WX_E_INVALID;
    for (int i = 0; i < 3; ++i)
        if (k_strides[i] % 8 || v_strides[i] % 8) return WX_E_INVALID;
    if (B > 65535 || H > 65535) return WX_E_INVALID;  // grid y / z
    if ((int64_t)B * G * H * chunks(L) > ((int64_t)1 << 40)) return WX_E_INVALID;  // (the workspace size stays in range)
    if (workspace_bytes < carve(workspace, (int64_t)B * G, H, L, a)) return WX_E_WORKSPACE;
    a->q = static_cast<const short*>(q);
    a->k = static_cast<const short*>(k);
    a->v = static_cast<const short*>(v);
    a->o = static_cast<short*>(o);
    a->qs[2] = 0;
    for (int i = 0; i < nq; ++i) a->qs[i] = q_strides[i];
    for (int i = 0; i < 3; ++i) {
        a->ks[i] = k_strides[i];
        a->vs[i] = v_strides[i];
    }
    a->H = H;
    a->L = L;
    a->nc = (int32_t)chunks(L);
    a->G = G;
    a->scale = scale;
    return -1;  // launch
}

template <bool BF>
void launch(const DecArgs& a, int32_t B, bool grouped, hipStream_t st) {
    const dim3 grid((unsigned)a.nc, (unsigned)a.H, (unsigned)B);
    if (grouped) {
        const size_t lds = (size_t)a.G * (kHead + kGroups * kHead + 2 * kGroups) * sizeof(float);  // (<= 35 KB)
        hipLaunchKernelGGL(decode_chunk_grouped_h16_kernel<BF>, grid, dim3(256), lds, st, a);
    } else {
        hipLaunchKernelGGL(decode_chunk_h16_kernel<BF>, grid, dim3(256), 0, st, a);
    }
    if (a.nc > 1) {
        const int64_t BH = (int64_t)B * a.G * a.H;  // (<= 8 x 65535^2: the merge grid's x fits)
        hipLaunchKernelGGL(decode_merge_h16_kernel<BF>, dim3((unsigned)((BH + 3) / 4)), dim3(256), 0, st, a, BH);
    }
}

}  // namespace wxdech

extern "C" int wx_decode_attention_h16(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H,
                                       int32_t L, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                                       const int64_t* v_strides, float scale, int32_t dtype, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    using namespace wxdech;
    DecArgs a;
    const int rc = prepare(q, k, v, o, B, 1, H, L, D, q_strides, 2, k_strides, v_strides, scale, dtype, workspace,
                           workspace_bytes, &a);
    if (rc >= 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == WX_DTYPE_BF16) launch<true>(a, B, false, st);
    else launch<false>(a, B, false, st);
    return wx::launch_status();
}

extern "C" int wx_decode_attention_h16_grouped(const void* q, const void* k, const void* v, void* o, int32_t B,
                                               int32_t G, int32_t H, int32_t L, int32_t D, const int64_t* q_strides,
                                               const int64_t* k_strides, const int64_t* v_strides, float scale,
                                               int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace wxdech;
    DecArgs a;
    const int rc = prepare(q, k, v, o, B, G, H, L, D, q_strides, 3, k_strides, v_strides, scale, dtype, workspace,
                           workspace_bytes, &a);
    if (rc >= 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == WX_DTYPE_BF16) launch<true>(a, B, true, st);
    else launch<false>(a, B, true, st);
    return wx::launch_status();
}
