// wx_prefill.hip — attention of a prompt prefill of Whisper's text decoder (whisperx/asr.py:35-45:
// the reference prepends `initial_prompt` / `prefix` to every batch's prompt, up to ~223 ids, and
// hands them to CTranslate2 in one forward): Tq query rows per (batch, head) against Tk key / value
// rows read in place through their strides, under a causal mask (the self-attention cache, query i
// at position causal + i) or without one (the two halves of the cross-attention [B, P, 2D] GEMM
// output).  C ABI and semantics: include/wx_align.h (wx_prefill_attention_f32 / _h16).
//
// The arithmetic is attn_f32_kernel's (wx_emission.hip), which see for the MFMA operand layout:
// one workgroup per (batch, head, 32-query tile), its kSplit waves over every kSplit-th 32-key tile,
// S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_32x32x2f32, the online softmax in fp32 with the
// query on the lane, the waves' (m, l, O^T) merged through LDS in wave order.  What is new:
//   - Tq and Tk differ, and the mask.  Key tiles are aligned to key 0 and wave w takes tiles w,
//     w + kSplit, ... whatever the launch is.  A query tile stops at its last row's last key
//     (tiles wholly above the diagonal are skipped), tiles wholly below its first row's diagonal
//     take the no-compare path, and only the straddling ones compare key < min(Tk, causal + i + 1)
//     per lane.  A masked key scores -inf: p = 0 exactly and the running maximum stays.
//   - "Nothing seen yet".  In a straddling tile that is a wave's first, the early query rows see no
//     key while their maximum is still -inf, and exp2(-inf - (-inf)) is NaN.  The update therefore
//     takes its exponents against 0 while the new maximum is -inf (alpha = p = exp2(-inf) = 0, the
//     state stays (-inf, 0, 0)), and the merge gives a wave whose maximum is -inf the weight 0.
//     Wave 0 always holds key 0, which every row sees, so the merged maximum is finite.
//   - So a step over a tile that is masked for a row is the identity on that row's state
//     (alpha = exp2(0) = 1, p = 0), and row (b, i, h) depends only on its query, on causal + i and
//     on the K / V rows below that: not on B, Tq, Tk beyond it, or on how causal + i is split.
//   - The K / V loads go through buffer descriptors that end at the tile's last visible key, so
//     rows at and past min(Tk, causal + Tq) are never read (past the end: zeros, masked).
//   - One template over the element type.  fp16 / bf16 elements are widened to fp32 exactly where
//     the fp32 kernel reads a float, and o is rounded to nearest even once, on the store: the h16
//     entry is the f32 entry on the widened inputs, rounded, bit for bit (the decoder's half
//     contract, wx_decode.hip; no packed 16-bit math, no 16-bit MFMA).
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wx_half.h"
#include "wx_host.h"  // (and through it include/wx_align.h)
#include "wx_wave.h"

namespace wxpre {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int kHead = 64;
constexpr int kSplit = 4;  // waves per 32-query tile, each over every kSplit-th 32-key tile
constexpr int64_t kMaxRowStride = (int64_t)1 << 23;  // K / V time stride: 32-bit byte offsets within a key tile

using wx::kF32, wx::kF16, wx::kBF16, wx::widen16, wx::round16;  // (wx_half.h)

struct PreArgs {
    const void *q, *k, *v;
    void* o;  // [B, Tq, H, 64]
    int32_t H, Tq, Tk, causal;
    int64_t qs[3], ks[3], vs[3];  // element strides {batch, head, time} (head dim: 1)
    float scale_log2;             // softmax scale * log2(e)
};

// What a lane holds of one 32-key tile, as loaded (16-bit elements are widened where they are used,
// so the loads of the next tile stay in flight behind this tile's arithmetic):
//   K[key r][32 hf + j], j < 32;  V[key(j)][r] and V[key(j)][32 + r], key(j) = (j & 3) + 8 (j >> 2) + 4 hf
template <int ET>
struct Tile {
    static constexpr int ES = ET == kF32 ? 4 : 2;   // bytes per element
    static constexpr int NK = 32 * ES / 16;         // 16-byte loads per half row
    u32x4 kraw[NK];
    typename std::conditional<ET == kF32, float, unsigned short>::type a0[16], a1[16];

    __device__ __forceinline__ float k(int j) const {
        if constexpr (ET == kF32) return __uint_as_float(kraw[j >> 2][j & 3]);
        else {
            const unsigned w = kraw[j >> 3][(j >> 1) & 3];
            return widen16<ET>((unsigned short)(j & 1 ? w >> 16 : w & 0xffffu));
        }
    }
    __device__ __forceinline__ float va(int j) const {
        if constexpr (ET == kF32) return a0[j];
        else return widen16<ET>(a0[j]);
    }
    __device__ __forceinline__ float vb(int j) const {
        if constexpr (ET == kF32) return a1[j];
        else return widen16<ET>(a1[j]);
    }
};

template <int ET>
__global__ __launch_bounds__(64 * kSplit) __attribute__((amdgpu_waves_per_eu(2))) void prefill_attn_kernel(PreArgs a) {
    constexpr int ES = Tile<ET>::ES;
    typedef typename std::conditional<ET == kF32, float, short>::type elem;
    const unsigned w = wx::xcd_unit();  // (batch, head, query tile) units
    const int Tq = a.Tq, Tk = a.Tk, causal = a.causal;
    const int nq = (Tq + 31) / 32;
    const int tile = (int)(w % (unsigned)nq);
    const int bh = (int)(w / (unsigned)nq);
    const int b = bh / a.H, h = bh % a.H;
    const elem* Q = static_cast<const elem*>(a.q) + b * a.qs[0] + h * a.qs[1];
    const elem* K = static_cast<const elem*>(a.k) + b * a.ks[0] + h * a.ks[1];
    const elem* V = static_cast<const elem*>(a.v) + b * a.vs[0] + h * a.vs[1];
    const int q0 = tile * 32;
    const int l = threadIdx.x & 63, r = l & 31, hf = l >> 5, wv = threadIdx.x >> 6;
    const int qi = min(q0 + r, Tq - 1);  // (a padding row repeats the last query; it is never stored)
    // keys [0, lim) are visible to this lane's query; every row of the tile sees [0, lim_lo), the
    // tile's last row sees [0, kend): all three are >= 1
    const int lim = causal < 0 ? Tk : (int)min((int64_t)Tk, (int64_t)causal + qi + 1);
    const int lim_lo = causal < 0 ? Tk : (int)min((int64_t)Tk, (int64_t)causal + q0 + 1);
    const int kend = causal < 0 ? Tk : (int)min((int64_t)Tk, (int64_t)causal + min(q0 + 32, Tq));

    float qv[32];
    {
        const elem* qp = Q + (int64_t)qi * a.qs[2] + 32 * hf;
        if constexpr (ET == kF32) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float4 x = reinterpret_cast<const float4*>(qp)[i];
                qv[4 * i] = x.x;
                qv[4 * i + 1] = x.y;
                qv[4 * i + 2] = x.z;
                qv[4 * i + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const u32x4 x = reinterpret_cast<const u32x4*>(qp)[i];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    qv[8 * i + 2 * c] = widen16<ET>((unsigned short)(x[c] & 0xffffu));
                    qv[8 * i + 2 * c + 1] = widen16<ET>((unsigned short)(x[c] >> 16));
                }
            }
        }
    }
    f32x16 o0, o1;
#pragma unroll
    for (int i = 0; i < 16; ++i) o0[i] = o1[i] = 0.f;
    float m = -INFINITY, lsum = 0.f;

    // K / V of the wave's next key tile are loaded while the current one computes, through buffer
    // descriptors rebased per key tile that end with key kend - 1: keys at and past kend read zeros
    // without touching memory, and are masked
    const int64_t skt = a.ks[2], svt = a.vs[2];
    const int vk = (int)((r * skt + 32 * hf) * ES), vv = (int)((4 * hf * svt + r) * ES);
    auto tile_rsrc = [&](const elem* base, int64_t stride, int k0) {
        k0 = __builtin_amdgcn_readfirstlane(k0);  // (32 wv + ...: uniform, which hipcc cannot prove)
        const int64_t rem = (int64_t)(kend - 1 - k0) * stride + 64;  // elements from key k0 to the end of key kend - 1
        const int n = k0 >= kend ? 0 : (int)min(rem * ES, (int64_t)0x7fffffff);
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<elem*>(base + (int64_t)min(k0, kend) * stride), 0, n, 0x00020000);
    };
    auto load_kv = [&](int k0, Tile<ET>& t) {
        const __amdgpu_buffer_rsrc_t rk = tile_rsrc(K, skt, k0), rv = tile_rsrc(V, svt, k0);
#pragma unroll
        for (int i = 0; i < Tile<ET>::NK; ++i)
            t.kraw[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, vk + 16 * i, 0, 0));
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int so = (int)(((j & 3) + 8 * (j >> 2)) * svt * ES);
            if constexpr (ET == kF32) {
                t.a0[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rv, vv, so, 0));
                t.a1[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rv, vv + 32 * ES, so, 0));
            } else {
                t.a0[j] = __builtin_amdgcn_raw_buffer_load_b16(rv, vv, so, 0);
                t.a1[j] = __builtin_amdgcn_raw_buffer_load_b16(rv, vv + 32 * ES, so, 0);
            }
        }
    };
    Tile<ET> cur;
    load_kv(32 * wv, cur);  // (a wave without a tile: zeros, unused)
    for (int k0 = 32 * wv; k0 < kend; k0 += 32 * kSplit) {
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 32; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k(j), qv[j], s, 0, 0, 0);
        float va[16], vb[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            va[j] = cur.va(j);
            vb[j] = cur.vb(j);
        }
        load_kv(k0 + 32 * kSplit, cur);  // (past kend: zeros, unused); cur is dead once S and va / vb are taken
        float mx = -INFINITY;
        if (k0 + 32 <= lim_lo) {  // wholly below the diagonal: no key compare (uniform branch)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s[i] = s[i] * a.scale_log2;
                mx = fmaxf(mx, s[i]);
            }
        } else {  // straddling the diagonal or the end of the keys
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = k0 + (i & 3) + 8 * (i >> 2) + 4 * hf;
                const float x = key < lim ? s[i] * a.scale_log2 : -INFINITY;
                s[i] = x;
                mx = fmaxf(mx, x);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);
        // nothing seen yet (mn = -inf): the exponents are taken against 0, alpha = p = exp2(-inf) = 0
        const float mref = mn == -INFINITY ? 0.f : mn;
        const float alpha = __builtin_amdgcn_exp2f(m - mref);
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float p = __builtin_amdgcn_exp2f(s[i] - mref);
            s[i] = p;
            ps += p;
        }
        ps += __shfl_xor(ps, 32);
        lsum = lsum * alpha + ps;
        m = mn;
        if (__any(alpha != 1.0f)) {  // (the running maximum settles after a few tiles)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                o0[i] *= alpha;
                o1[i] *= alpha;
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[j], s[j], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vb[j], s[j], o1, 0, 0, 0);
        }
    }
    // merge the waves' partial softmax states (m, lsum, O^T) in wave 0, in wave order
    __shared__ float red[kSplit - 1][34][64];
    if (wv > 0) {
        float* o = &red[wv - 1][0][l];
        o[0] = m;
        o[64] = lsum;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            o[64 * (2 + i)] = o0[i];
            o[64 * (18 + i)] = o1[i];
        }
    }
    __syncthreads();
    if (wv > 0) return;
    float mt = m;  // finite: wave 0 holds key 0
#pragma unroll
    for (int w2 = 0; w2 < kSplit - 1; ++w2) mt = fmaxf(mt, red[w2][0][l]);
    {
        const float c = __builtin_amdgcn_exp2f(m - mt);
        lsum *= c;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            o0[i] *= c;
            o1[i] *= c;
        }
    }
#pragma unroll
    for (int w2 = 0; w2 < kSplit - 1; ++w2) {
        const float mw = red[w2][0][l];
        const float c = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - mt);  // a wave that saw no key for this row: 0
        lsum += red[w2][1][l] * c;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            o0[i] += red[w2][2 + i][l] * c;
            o1[i] += red[w2][18 + i][l] * c;
        }
    }
    if (q0 + r >= Tq) return;  // a padding row
    const float inv = 1.0f / lsum;
    elem* orow = static_cast<elem*>(a.o) + (((int64_t)b * Tq + q0 + r) * a.H + h) * kHead;
#pragma unroll
    for (int g = 0; g < 4; ++g) {  // registers 4g..4g+3: head dims 8g + 4hf + 0..3
        const int d = 8 * g + 4 * hf;
        if constexpr (ET == kF32) {
            *reinterpret_cast<float4*>(orow + d) =
                make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            *reinterpret_cast<float4*>(orow + 32 + d) =
                make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
        } else {
            *reinterpret_cast<s16x4*>(orow + d) =
                s16x4{round16<ET>(o0[4 * g] * inv), round16<ET>(o0[4 * g + 1] * inv), round16<ET>(o0[4 * g + 2] * inv),
                      round16<ET>(o0[4 * g + 3] * inv)};
            *reinterpret_cast<s16x4*>(orow + 32 + d) =
                s16x4{round16<ET>(o1[4 * g] * inv), round16<ET>(o1[4 * g + 1] * inv), round16<ET>(o1[4 * g + 2] * inv),
                      round16<ET>(o1[4 * g + 3] * inv)};
        }
    }
}

// The checks of both entry points, in the header's order; `mult`: elements per 16 bytes.
// Returns a status, or -1 to launch.
inline int prepare(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H, int32_t Tq, int32_t Tk,
                   int32_t causal, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                   const int64_t* v_strides, float scale, int mult, bool dtype_ok, PreArgs* a, unsigned* grid) {
    if (B < 0 || H < 1 || Tq < 1 || Tk < 1 || D != kHead || !dtype_ok) return WX_E_INVALID;
    if (B == 0) return WX_OK;
    if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides) return WX_E_INVALID;
    for (const void* p : {q, k, v, (const void*)o})
        if (reinterpret_cast<uintptr_t>(p) & 15) return WX_E_INVALID;
    for (int i = 0; i < 3; ++i)
        if (q_strides[i] % mult || k_strides[i] % mult || v_strides[i] % mult) return WX_E_INVALID;
    // a key tile's rows are addressed by 32-bit byte offsets from the tile's first row
    if (k_strides[2] < 0 || k_strides[2] > kMaxRowStride || v_strides[2] < 0 || v_strides[2] > kMaxRowStride)
        return WX_E_INVALID;
    const int64_t blocks = ((int64_t)Tq + 31) / 32 * B * H;
    if (blocks > INT32_MAX) return WX_E_INVALID;  // (one grid dimension)
    a->q = q;
    a->k = k;
    a->v = v;
    a->o = o;
    a->H = H;
    a->Tq = Tq;
    a->Tk = Tk;
    a->causal = causal < 0 ? -1 : causal;
    for (int i = 0; i < 3; ++i) {
        a->qs[i] = q_strides[i];
        a->ks[i] = k_strides[i];
        a->vs[i] = v_strides[i];
    }
    a->scale_log2 = scale * 1.4426950408889634f;
    *grid = (unsigned)blocks;
    return -1;
}

}  // namespace wxpre

extern "C" int wx_prefill_attention_f32(const float* q, const float* k, const float* v, float* o, int32_t B, int32_t H,
                                        int32_t Tq, int32_t Tk, int32_t causal, int32_t D, const int64_t* q_strides,
                                        const int64_t* k_strides, const int64_t* v_strides, float scale,
                                        void* stream) {
    using namespace wxpre;
    PreArgs a;
    unsigned grid = 0;
    const int rc = prepare(q, k, v, o, B, H, Tq, Tk, causal, D, q_strides, k_strides, v_strides, scale, 4, true, &a, &grid);
    if (rc >= 0) return rc;
    hipLaunchKernelGGL(prefill_attn_kernel<kF32>, dim3(grid), dim3(64 * kSplit), 0, reinterpret_cast<hipStream_t>(stream), a);
    return wx::launch_status();
}

extern "C" int wx_prefill_attention_h16(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H,
                                        int32_t Tq, int32_t Tk, int32_t causal, int32_t D, const int64_t* q_strides,
                                        const int64_t* k_strides, const int64_t* v_strides, float scale, int32_t dtype,
                                        void* stream) {
    using namespace wxpre;
    PreArgs a;
    unsigned grid = 0;
    const int rc = prepare(q, k, v, o, B, H, Tq, Tk, causal, D, q_strides, k_strides, v_strides, scale, 8,
                           dtype == WX_DTYPE_F16 || dtype == WX_DTYPE_BF16, &a, &grid);
    if (rc >= 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == WX_DTYPE_BF16) hipLaunchKernelGGL(prefill_attn_kernel<kBF16>, dim3(grid), dim3(64 * kSplit), 0, st, a);
    else hipLaunchKernelGGL(prefill_attn_kernel<kF16>, dim3(grid), dim3(64 * kSplit), 0, st, a);
    return wx::launch_status();
}
