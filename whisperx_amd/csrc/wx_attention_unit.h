// wx_attention_unit.h — what the attention entry points share (wx_attention_f32 / _packed in
// wx_emission.hip, wx_prefill_attention_f32 / _h16 in wx_prefill.hip, wx_attention_h16 / _packed in
// wx_attention_h16.hip): the kernels' argument block and its host-side checks, the map from a work
// unit to its (batch entry or packed segment, head, query tile), and the flash-attention body on the
// f32-input MFMA that the emission and prefill kernels run.
#ifndef WX_ATTENTION_UNIT_H
#define WX_ATTENTION_UNIT_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "wx_half.h"
#include "wx_host.h"  // (and through it include/wx_align.h)
#include "wx_wave.h"

namespace wx {

struct AttnArgs {
    const void *q, *k, *v;
    void* o;                      // [B, Tq, H, 64] (packed: [rows, H, 64]) contiguous
    int64_t qs[3], ks[3], vs[3];  // element strides {batch, head, time} (head dim: 1; packed: batch 0)
    float scale_log2;             // softmax scale * log2(e)
    int32_t H, Tq, Tk, causal;    // (dense kernels; causal < 0: no mask)
    // packed segments: segment s owns rows [seg_rows[s], seg_rows[s + 1]) and work units
    // [seg_units[s], seg_units[s + 1]) (H x its query tiles, head-major, so that one (segment, head)'s
    // units are a contiguous run of one XCD)
    const int32_t *seg_rows, *seg_units;
    int32_t nseg;
};

// K / V time stride of the f32-MFMA body: 32-bit byte offsets within a key tile
constexpr int64_t kMaxRowStride = (int64_t)1 << 23;

// The checks every attention entry makes after its own size checks and empty-input returns, and the
// pointers, strides and scale of `a`: pointers non-null and 16-byte aligned, the `nstrides` strides
// of each operand ({batch, head, time}, or a pack's {head, row}) multiples of `mult` elements (16
// bytes), `blocks` within one grid dimension and, for the f32-MFMA body (`bound_rows`), the K / V
// time stride in [0, kMaxRowStride].  False: WX_E_INVALID.
inline bool attn_args(AttnArgs* a, const void* q, const void* k, const void* v, void* o, const int64_t* q_strides,
                      const int64_t* k_strides, const int64_t* v_strides, int nstrides, int mult, bool bound_rows,
                      int64_t blocks, float scale) {
    if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides) return false;
    for (const void* p : {q, k, v, (const void*)o})
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    const int64_t* in[3] = {q_strides, k_strides, v_strides};
    int64_t* out[3] = {a->qs, a->ks, a->vs};
    for (int t = 0; t < 3; ++t) {
        out[t][0] = 0;
        for (int i = 0; i < nstrides; ++i) {
            if (in[t][i] % mult) return false;
            out[t][3 - nstrides + i] = in[t][i];
        }
    }
    if (bound_rows && (a->ks[2] < 0 || a->ks[2] > kMaxRowStride || a->vs[2] < 0 || a->vs[2] > kMaxRowStride)) return false;
    if (blocks > INT32_MAX) return false;
    a->q = q;
    a->k = k;
    a->v = v;
    a->o = o;
    a->scale_log2 = scale * 1.4426950408889634f;
    return true;
}

// Unit w of a dense launch of B x H x nq units -> batch entry, head, query tile
__device__ __forceinline__ void dense_unit(unsigned w, int nq, int H, int& b, int& h, int& tile) {
    tile = (int)(w % (unsigned)nq);
    const int bh = (int)(w / (unsigned)nq);
    b = bh / H;
    h = bh % H;
}

// Unit w of a packed launch -> its segment's first row and length, head, query tile (`rows` queries
// each).  The segment owning w is the last s with seg_units[s] <= w (an empty segment owns no unit,
// so the last such s is never one of them: T >= 1).
__device__ __forceinline__ void packed_unit(unsigned w, const int32_t* seg_rows, const int32_t* seg_units, int nseg,
                                            int rows, int64_t& row0, int& T, int& h, int& tile) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((unsigned)seg_units[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    row0 = seg_rows[lo];
    T = seg_rows[lo + 1] - (int)row0;
    const int nq = (T + rows - 1) / rows;
    const int u = (int)w - seg_units[lo];
    tile = u % nq;
    h = u / nq;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// What a lane holds of one 32-key tile, as loaded (16-bit elements are widened where they are used,
// so the loads of the next tile stay in flight behind this tile's arithmetic):
//   K[key r][32 hf + j], j < 32;  V[key(j)][r] and V[key(j)][32 + r], key(j) = (j & 3) + 8 (j >> 2) + 4 hf
template <int ET>
struct AttnTile {
    static constexpr int ES = ET == kF32 ? 4 : 2;  // bytes per element
    static constexpr int NK = 32 * ES / 16;        // 16-byte loads per half row
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

// One (head, 32-query tile) unit of a flash-attention forward on the f32-input MFMA
// (v_mfma_f32_32x32x2_f32: exact f32 fmaf chains, 64 FLOP per clock per SIMD), run by a workgroup of
// SPLIT waves: wave w takes key tiles w, w + SPLIT, ... (32 keys each, aligned to key 0) and the
// waves' (max, sum, O^T) states are merged through LDS in wave order (SPLIT = 1: no LDS, no barrier).
// Q / K / V point at row 0 of one (batch entry or packed segment, head) with row strides sqt / skt /
// svt (skt, svt in [0, kMaxRowStride]), O at its output row 0 (row stride orow); Tq queries against
// Tk keys, query i seeing keys [0, min(Tk, causal + i + 1)) or, with causal < 0, all of them.  So a
// unit is computed exactly as the same rows under any other launch: square unmasked attention is
// causal = -1, Tq = Tk = T.  Per wave:
//   * S^T = K Q^T per 32-key tile: lane l holds key row (l & 31) of K and query row (l & 31) of Q as
//     the A / B operands; the head dimension is split 32 / 32 between the lane halves (the
//     contraction order is free), so each lane reads contiguous half rows;
//   * S^T's accumulator has the query on the lane and 16 keys per lane in registers, so the online
//     softmax is lane-local plus one exchange with the other lane half, and the same registers are
//     the B operand (P^T) of O^T += V^T P^T without any lane movement: MFMA j takes key
//     (j & 3) + 8 (j >> 2) + 4 (l >> 5) from each half, and V is read at those rows;
//   * O^T lives in two 32x32 accumulators (head dims 0-31, 32-63), rescaled lane-locally.
// The mask.  A query tile stops at its last row's last key (tiles wholly above the diagonal are
// skipped), tiles wholly below its first row's diagonal take the no-compare path, and only the
// straddling ones compare key < min(Tk, causal + i + 1) per lane.  A masked key scores -inf: p = 0
// exactly and the running maximum stays.
// "Nothing seen yet".  In a straddling tile that is a wave's first, the early query rows see no key
// while their maximum is still -inf, and exp2(-inf - (-inf)) is NaN.  The update therefore takes its
// exponents against 0 while the new maximum is -inf (alpha = p = exp2(-inf) = 0, the state stays
// (-inf, 0, 0)), and the merge gives a wave whose maximum is -inf the weight 0.  Wave 0 always holds
// key 0, which every row sees, so the merged maximum is finite.  So a step over a tile that is
// masked for a row is the identity on that row's state (alpha = exp2(0) = 1, p = 0), and a row
// depends only on its query, on causal + i and on the K / V rows below that.  Without a mask all of
// this is the identity: every wave's first tile gives every row a finite maximum.
// The K / V loads go through buffer descriptors rebased per key tile (no per-lane address
// arithmetic) that end at the unit's last visible key, so rows at and past min(Tk, causal + Tq) are
// never read (past the end: zeros, masked).
// ET: fp16 / bf16 elements are widened to fp32 exactly where the fp32 form reads a float, and o is
// rounded to nearest even once, on the store (no packed 16-bit math, no 16-bit MFMA).
template <int ET, int SPLIT>
__device__ __forceinline__ void attn_mfma32_unit(const void* Qv, const void* Kv, const void* Vv, void* Ov, const int Tq,
                                                 const int Tk, const int causal, const int tile, const int64_t sqt,
                                                 const int64_t skt, const int64_t svt, const int64_t orow,
                                                 const float scale_log2) {
    constexpr int ES = AttnTile<ET>::ES;
    typedef typename std::conditional<ET == kF32, float, short>::type elem;
    const elem *Q = static_cast<const elem*>(Qv), *K = static_cast<const elem*>(Kv), *V = static_cast<const elem*>(Vv);
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
        const elem* qp = Q + (int64_t)qi * sqt + 32 * hf;
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
    // descriptors that end with key kend - 1: keys at and past kend read zeros without touching memory
    const int vk = (int)((r * skt + 32 * hf) * ES), vv = (int)((4 * hf * svt + r) * ES);
    auto tile_rsrc = [&](const elem* base, int64_t stride, int k0) {
        // `left` keys from k0 to kend - 1, (left - 1) stride + 64 elements; at and past kend none, at kend's
        // row.  Written as a product: hipcc turns the select into a branch, and a basic block's end
        // between the S chain and the loads keeps them from being issued beside its MFMAs
        const int left = max(kend - k0, 0);
        const int64_t rem = (int64_t)(left - 1) * stride + 64;
        const int n = min(left, 1) * (int)min(rem * ES, (int64_t)0x7fffffff);
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<elem*>(base + (int64_t)min(k0, kend) * stride), 0, n, 0x00020000);
    };
    auto load_kv = [&](int k0, AttnTile<ET>& t) {
        k0 = __builtin_amdgcn_readfirstlane(k0);  // (32 wv + ...: uniform, which hipcc cannot prove)
        const __amdgpu_buffer_rsrc_t rk = tile_rsrc(K, skt, k0), rv = tile_rsrc(V, svt, k0);
#pragma unroll
        for (int i = 0; i < AttnTile<ET>::NK; ++i)
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
    AttnTile<ET> cur;
    load_kv(32 * wv, cur);  // (a wave without a tile: zeros, unused)
    for (int k0 = 32 * wv; k0 < kend; k0 += 32 * SPLIT) {
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
        load_kv(k0 + 32 * SPLIT, cur);  // (past kend: zeros, unused); cur is dead once S and va / vb are taken
        float mx = -INFINITY;
        if (k0 + 32 <= lim_lo) {  // wholly below the diagonal: no key compare (uniform branch)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s[i] = s[i] * scale_log2;
                mx = fmaxf(mx, s[i]);
            }
        } else {  // straddling the diagonal or the end of the keys
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = k0 + (i & 3) + 8 * (i >> 2) + 4 * hf;
                const float x = key < lim ? s[i] * scale_log2 : -INFINITY;
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
    if constexpr (SPLIT > 1) {
        __shared__ float red[SPLIT - 1][34][64];
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
        for (int w = 0; w < SPLIT - 1; ++w) mt = fmaxf(mt, red[w][0][l]);
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
        for (int w = 0; w < SPLIT - 1; ++w) {
            const float mw = red[w][0][l];
            const float c = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - mt);  // a wave that saw no key for this row: 0
            lsum += red[w][1][l] * c;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                o0[i] += red[w][2 + i][l] * c;
                o1[i] += red[w][18 + i][l] * c;
            }
        }
    }
    if (q0 + r >= Tq) return;  // a padding row
    const float inv = 1.0f / lsum;
    elem* op = static_cast<elem*>(Ov) + (int64_t)(q0 + r) * orow;
#pragma unroll
    for (int g = 0; g < 4; ++g) {  // registers 4g..4g+3: head dims 8g + 4hf + 0..3
        const int d = 8 * g + 4 * hf;
        if constexpr (ET == kF32) {
            *reinterpret_cast<float4*>(op + d) =
                make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            *reinterpret_cast<float4*>(op + 32 + d) =
                make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
        } else {
            *reinterpret_cast<s16x4*>(op + d) =
                s16x4{round16<ET>(o0[4 * g] * inv), round16<ET>(o0[4 * g + 1] * inv), round16<ET>(o0[4 * g + 2] * inv),
                      round16<ET>(o0[4 * g + 3] * inv)};
            *reinterpret_cast<s16x4*>(op + 32 + d) =
                s16x4{round16<ET>(o1[4 * g] * inv), round16<ET>(o1[4 * g + 1] * inv), round16<ET>(o1[4 * g + 2] * inv),
                      round16<ET>(o1[4 * g + 3] * inv)};
        }
    }
}

}  // namespace wx
#endif  // WX_ATTENTION_UNIT_H
