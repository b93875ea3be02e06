// wx_attention_h16.hip — Whisper's encoder self-attention on 16-bit inputs (whisperx/asr.py:262: the
// reference loads its model with compute_type="float16"): softmax(scale q k^T) v for fp16 or bf16
// q / k / v, no mask, head dim 64, on v_mfma_f32_32x32x16_{f16,bf16}.  C ABI and semantics:
// include/wx_align.h (wx_attention_h16).  wx_attention_h16_packed runs the same body over segments
// packed back to back (the half route of the wav2vec2 emission forward, alignment.py:217-233: one
// unpadded forward per segment), each segment bit for bit as if launched alone.
//
// The structure is attn_mfma32_unit's (wx_attention_unit.h): one workgroup per (batch, head, query
// tile), whose kSplit waves each take every kSplit-th 32-key tile and merge their (max, sum, O) states
// through LDS; the 1-D grid is handed to the XCDs in contiguous runs.  A query tile is kNQ = 2
// MFMA tiles of 32 queries: every wave holds both, so a K / V tile fetched from L2 serves two S
// chains and two P V products.  Per wave, key tile and 32 queries:
//   * S^T = K Q^T, 4 MFMAs: lane l (r = l & 31, hf = l >> 5) holds key row r of K and query row r of
//     Q as the A / B fragments, head dims 32 hf + 8 t .. + 7 in k-step t (the contraction order is
//     free; each lane reads one contiguous 64-byte half row).  The accumulator has the query on the
//     lane and 16 keys in registers (register i: key (i & 3) + 8 (i >> 2) + 4 hf), so the softmax is
//     lane-local plus one exchange with the other lane half.
//   * The probabilities, rounded to the element type, are the B fragment (P^T) of O^T += V^T P^T
//     with no lane movement: registers 8 s .. 8 s + 7 are k-step s, whose element j is key
//     16 s + 8 (j >> 2) + 4 hf + (j & 3).  The A fragment must hold V at exactly those keys with the
//     head dim on the lane: the wave stages its V tile row-major in LDS (4 KB, 16-byte chunks
//     XOR-swizzled by bit 1 of the row so that the four rows of a transposed read meet four
//     different bank windows) and reads it back with ds_read_b64_tr_b16, 8 reads per key tile (shared
//     by the two query tiles) and 4 MFMAs (O^T is two 32x32 accumulators, head dims 0-31 and 32-63).
//   * K and V of the wave's next tile are loaded into registers behind the S chain and V is written
//     to the wave's LDS tile after the last transposed read of the current one (one buffer: a wave's
//     LDS operations execute in order, the fences keep the compiler from reordering them).
// Keys at and past T: a lane whose K or V row is >= T issues no load and holds zeros (no address
// outside the tensors is formed for a load that is issued; zeros, so that a probability of 0 never
// meets a NaN), and their scores are -inf.  Every lane takes part in every transposed read (the
// loops and branches around them are wave-uniform): the LDS tile always holds all 32 rows.
// The running sum is taken over the ROUNDED probabilities, the values the second MFMA multiplies
// with V, so that the weights of a row sum to one exactly as they are applied.
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wx_attention_unit.h"  // (and through it wx_half.h, wx_host.h, wx_wave.h)

namespace wxh {

using wx::f32x16, wx::s16x4;
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kSplit = 4;                    // waves per 32-query tile, each over every kSplit-th 32-key tile
constexpr int kTileBytes = 32 * 128;         // a wave's V tile: 32 keys x 64 x 16 bit
constexpr int kNQ = 2;                       // 32-query tiles per workgroup: each wave holds them all
constexpr int kQueries = 32 * kNQ;
constexpr int kRedFloats = kNQ * 34 * 64;    // a wave's state in the merge: per query tile m, sum, 2 x 16 accumulator registers
constexpr int kLdsBytes = (kSplit - 1) * kRedFloats * 4 > kSplit * kTileBytes ? (kSplit - 1) * kRedFloats * 4
                                                                              : kSplit * kTileBytes;

// BF: bf16 (else fp16).  Bit patterns travel as shorts (wx_half.h).
template <bool BF>
__device__ __forceinline__ f32x16 mfma16(s16x8 a, s16x8 b, f32x16 c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// orders the wave's own LDS writes and transposed reads as written (the hardware executes one
// wave's LDS instructions in order; other waves never touch this wave's tile)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One (head, 64-query tile) unit of one batch entry or packed segment: Q / K / V point at row 0 of
// that (entry, head) (row strides sqt / skt / svt), O at its output row 0 (row stride orow elements),
// T is its length.  Both entry points below resolve these and run the same body, so a segment of a
// pack is computed exactly as the same rows alone (same per-wave key tiles, same merge order).
template <bool BF>
__device__ __forceinline__ void attn_h16_unit(const short* Q, const short* K, const short* V, short* O, const int T,
                                              const int tile, const int64_t sqt, const int64_t skt, const int64_t svt,
                                              const int64_t orow, const float scale_log2, char* lds) {
    constexpr int ET = wx::half_et(BF);
    const int q0 = tile * kQueries;
    const int l = threadIdx.x & 63, r = l & 31, hf = l >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform, which hipcc cannot prove)
    s16x8 qf[kNQ][4];  // query q0 + 32 u + r (past the end: the last row again, never stored)
#pragma unroll
    for (int u = 0; u < kNQ; ++u) {
        const s16x8* qp = reinterpret_cast<const s16x8*>(Q + (int64_t)min(q0 + 32 * u + r, T - 1) * sqt + 32 * hf);
#pragma unroll
        for (int t = 0; t < 4; ++t) qf[u][t] = qp[t];
    }
    f32x16 o0[kNQ], o1[kNQ];
    float m[kNQ], lsum[kNQ];
#pragma unroll
    for (int u = 0; u < kNQ; ++u) {
#pragma unroll
        for (int i = 0; i < 16; ++i) o0[u][i] = o1[u][i] = 0.f;
        m[u] = -INFINITY;
        lsum[u] = 0.f;
    }
    // V tile in LDS: row `key`, 16-byte chunk c (8 per row) at 128 key + 16 (c ^ 4 ((key >> 1) & 1))
    char* vt = lds + wv * kTileBytes;
    const int vrow = l >> 3, vch = l & 7;  // this lane's chunk of rows vrow + 8 i in the global loads
    // transposed reads: lane 4 qq + p of a 16-lane group supplies row key0 + qq, 4 elements from
    // column 32 acc + 16 (group & 1) + 4 p, and receives column (lane & 15) of the block's 4 rows
    const int qq = (l >> 2) & 3, p = l & 3, g1 = (l >> 4) & 1;
    const int tr0 = 128 * (4 * hf + qq) + 16 * ((2 * g1 + (p >> 1)) ^ (4 * (qq >> 1))) + 8 * (p & 1);
    const int tr1 = tr0 ^ 64;  // head dims 32-63: chunk bit 2
    s16x8 kf[4], vf[4];
    const s16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    auto load_kv = [&](int k0) {  // K row k0 + r and this lane's 4 chunks of the V tile; rows >= T: zeros, no load
#pragma unroll
        for (int t = 0; t < 4; ++t) kf[t] = vf[t] = zero8;
        if (k0 + r < T) {
            const s16x8* kp = reinterpret_cast<const s16x8*>(K + (int64_t)(k0 + r) * skt + 32 * hf);
#pragma unroll
            for (int t = 0; t < 4; ++t) kf[t] = kp[t];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = k0 + vrow + 8 * i;
            if (key < T) vf[i] = *reinterpret_cast<const s16x8*>(V + (int64_t)key * svt + 8 * vch);
        }
    };
    auto stage_v = [&] {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = vrow + 8 * i;
            *reinterpret_cast<s16x8*>(vt + 128 * row + 16 * (vch ^ (4 * ((row >> 1) & 1)))) = vf[i];
        }
    };
    auto read_vt = [&](int off) {  // ds_read_b64_tr_b16
        return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            reinterpret_cast<__attribute__((address_space(3))) s16x4*>(reinterpret_cast<uintptr_t>(vt + off)));
    };
    if (32 * wv < T) {
        load_kv(32 * wv);
        stage_v();
        wave_lds_fence();
    }
    for (int k0 = 32 * wv; k0 < T; k0 += 32 * kSplit) {
        f32x16 s[kNQ];
#pragma unroll
        for (int u = 0; u < kNQ; ++u) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[u][i] = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) s[u] = mfma16<BF>(kf[t], qf[u][t], s[u]);
        }
        const bool more = k0 + 32 * kSplit < T;  // (uniform)
        if (more) load_kv(k0 + 32 * kSplit);     // kf is dead once the S chains have been issued
        s16x8 pf[kNQ][2];
#pragma unroll
        for (int u = 0; u < kNQ; ++u) {
            float mx = -INFINITY;
            if (k0 + 32 <= T) {  // a whole key tile: no key compare (uniform branch)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    s[u][i] = s[u][i] * scale_log2;
                    mx = fmaxf(mx, s[u][i]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = k0 + (i & 3) + 8 * (i >> 2) + 4 * hf;
                    const float x = key < T ? s[u][i] * scale_log2 : -INFINITY;
                    s[u][i] = x;
                    mx = fmaxf(mx, x);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m[u], mx);
            const float alpha = __builtin_amdgcn_exp2f(m[u] - mn);
            float ps = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const short ph = wx::round16<ET>(__builtin_amdgcn_exp2f(s[u][i] - mn));
                pf[u][i >> 3][i & 7] = ph;
                ps += wx::widen16<ET>(ph);
            }
            ps += __shfl_xor(ps, 32);
            lsum[u] = lsum[u] * alpha + ps;
            m[u] = mn;
            if (__any(alpha != 1.0f)) {  // (the running maximum settles after a few tiles)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    o0[u][i] *= alpha;
                    o1[u][i] *= alpha;
                }
            }
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            s16x8 v0, v1;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const s16x4 x0 = read_vt(tr0 + 2048 * st + 1024 * e), x1 = read_vt(tr1 + 2048 * st + 1024 * e);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v0[4 * e + j] = x0[j];
                    v1[4 * e + j] = x1[j];
                }
            }
#pragma unroll
            for (int u = 0; u < kNQ; ++u) {
                o0[u] = mfma16<BF>(v0, pf[u][st], o0[u]);
                o1[u] = mfma16<BF>(v1, pf[u][st], o1[u]);
            }
        }
        if (more) {
            wave_lds_fence();
            stage_v();
            wave_lds_fence();
        }
    }
    // merge the waves' partial softmax states (m, lsum, O^T) in wave 0, through the LDS the V tiles used
    __syncthreads();
    float(*red)[kNQ][34][64] = reinterpret_cast<float(*)[kNQ][34][64]>(lds);
    if (wv > 0) {
#pragma unroll
        for (int u = 0; u < kNQ; ++u) {
            float* o = &red[wv - 1][u][0][l];
            o[0] = m[u];
            o[64] = lsum[u];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                o[64 * (2 + i)] = o0[u][i];
                o[64 * (18 + i)] = o1[u][i];
            }
        }
    }
    __syncthreads();
    if (wv > 0) return;
#pragma unroll
    for (int u = 0; u < kNQ; ++u) {
        float mt = m[u];
#pragma unroll
        for (int x = 0; x < kSplit - 1; ++x) mt = fmaxf(mt, red[x][u][0][l]);
        {
            const float c = __builtin_amdgcn_exp2f(m[u] - mt);
            lsum[u] *= c;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                o0[u][i] *= c;
                o1[u][i] *= c;
            }
        }
#pragma unroll
        for (int x = 0; x < kSplit - 1; ++x) {
            const float c = __builtin_amdgcn_exp2f(red[x][u][0][l] - mt);  // a wave without keys: 0
            lsum[u] += red[x][u][1][l] * c;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                o0[u][i] += red[x][u][2 + i][l] * c;
                o1[u][i] += red[x][u][18 + i][l] * c;
            }
        }
        const int qi = q0 + 32 * u + r;
        if (qi >= T) continue;
        const float inv = 1.0f / lsum[u];
        short* orow_p = O + (int64_t)qi * orow;
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // registers 4g..4g+3: head dims 8g + 4hf + 0..3
            const int d = 8 * g + 4 * hf;
            s16x4 x0, x1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x0[j] = wx::round16<ET>(o0[u][4 * g + j] * inv);
                x1[j] = wx::round16<ET>(o1[u][4 * g + j] * inv);
            }
            *reinterpret_cast<s16x4*>(orow_p + d) = x0;
            *reinterpret_cast<s16x4*>(orow_p + 32 + d) = x1;
        }
    }
}

// amdgpu_waves_per_eu(2): 223 VGPRs, no spill.  With one query tile per wave (141 VGPRs) two, three
// and four waves per SIMD measured the same to 1%, as did whole key tiles loaded without the row
// compares: the kernel was bound by the K / V traffic from L2 (8 KB per wave and key tile for 4 + 4
// MFMAs), which the second query tile halves (B 16, T 1500, fp16: H 8 0.198 -> 0.173 ms, H 20
// 0.440 -> 0.380 ms).
// PACKED (wx_attention_h16_packed): one launch over many segments of their own lengths, 64-query units
template <bool BF, bool PACKED>
__global__ __launch_bounds__(64 * kSplit) __attribute__((amdgpu_waves_per_eu(2))) void attn_h16_kernel(wx::AttnArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[kLdsBytes];
    const short *q = static_cast<const short*>(a.q), *k = static_cast<const short*>(a.k), *v = static_cast<const short*>(a.v);
    int T, b = 0, h, tile;
    int64_t row0 = 0;  // first row of this packed segment
    const unsigned w = wx::xcd_unit();
    if constexpr (PACKED) {
        wx::packed_unit(w, a.seg_rows, a.seg_units, a.nseg, kQueries, row0, T, h, tile);
    } else {
        T = a.Tq;
        wx::dense_unit(w, (T + kQueries - 1) / kQueries, a.H, b, h, tile);
    }
    attn_h16_unit<BF>(q + b * a.qs[0] + h * a.qs[1] + row0 * a.qs[2], k + b * a.ks[0] + h * a.ks[1] + row0 * a.ks[2],
                      v + b * a.vs[0] + h * a.vs[1] + row0 * a.vs[2],
                      static_cast<short*>(a.o) + ((row0 + (int64_t)b * T) * a.H + h) * 64, T, tile, a.qs[2], a.ks[2], a.vs[2],
                      (int64_t)a.H * 64, a.scale_log2, lds);
}

}  // namespace wxh

extern "C" int wx_attention_h16(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H, int32_t T,
                                int32_t D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                float scale, int32_t dtype, void* stream) {
    using namespace wxh;
    if (B < 0 || H < 1 || T < 1 || D != 64 || (dtype != WX_DTYPE_F16 && dtype != WX_DTYPE_BF16)) return WX_E_INVALID;
    if (B == 0) return WX_OK;
    if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides) return WX_E_INVALID;
    const int64_t blocks = ((int64_t)T + kQueries - 1) / kQueries * B * H;
    wx::AttnArgs a{};
    if (!wx::attn_args(&a, q, k, v, o, q_strides, k_strides, v_strides, 3, 8, false, blocks, scale)) return WX_E_INVALID;
    a.H = H;
    a.Tq = a.Tk = T;
    const dim3 grid((unsigned)blocks);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == WX_DTYPE_BF16) hipLaunchKernelGGL((attn_h16_kernel<true, false>), grid, dim3(64 * kSplit), 0, s, a);
    else hipLaunchKernelGGL((attn_h16_kernel<false, false>), grid, dim3(64 * kSplit), 0, s, a);
    return wx::launch_status();
}

extern "C" int wx_attention_h16_packed(const void* q, const void* k, const void* v, void* o, int32_t nseg,
                                       const int32_t* seg_rows, const int32_t* seg_units, int32_t n_units, int32_t H,
                                       int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                                       const int64_t* v_strides, float scale, int32_t dtype, void* stream) {
    using namespace wxh;
    if (nseg < 0 || H <= 0 || D != 64 || (dtype != WX_DTYPE_F16 && dtype != WX_DTYPE_BF16) || n_units < 0 || !q || !k ||
        !v || !o || !q_strides || !k_strides || !v_strides)
        return WX_E_INVALID;
    if (nseg == 0 || n_units == 0) return WX_OK;
    if (!seg_rows || !seg_units) return WX_E_INVALID;
    wx::AttnArgs a{};  // (strides {head, row}: batch 0)
    if (!wx::attn_args(&a, q, k, v, o, q_strides, k_strides, v_strides, 2, 8, false, n_units, scale)) return WX_E_INVALID;
    a.H = H;
    a.nseg = nseg;
    a.seg_rows = seg_rows;
    a.seg_units = seg_units;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n_units);
    if (dtype == WX_DTYPE_BF16) hipLaunchKernelGGL((attn_h16_kernel<true, true>), grid, dim3(64 * kSplit), 0, s, a);
    else hipLaunchKernelGGL((attn_h16_kernel<false, true>), grid, dim3(64 * kSplit), 0, s, a);
    return wx::launch_status();
}
