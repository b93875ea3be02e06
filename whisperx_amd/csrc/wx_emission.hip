// wx_emission.hip — gfx950 kernels of the emission producer (reference
// whisperx/alignment.py:226-233, the wav2vec2 forward) and their entry points: the channel norm
// (wx_channel_norm), the first feature-encoder layer as conv + channel norm + GELU in one pass over
// its output (wx_conv0_channel_norm, _h16), fp32 self-attention on the f32-input MFMA
// (wx_attention_f32, _packed) and the positional convolution over packed segments
// (wx_posconv_packed).  `layer_norm(residual + x)` is wx_add_layernorm.hip, the 16-bit attention
// wx_attention_h16.hip.
//
// The channel norm: the first feature-encoder layer's GroupNorm(512 groups = per channel over time)
// + GELU, fused, on time-major activations.
// emission.prepare_model keeps the conv feature encoder time-major ([L, C], the GEMM route's
// natural output).  torch's GroupNorm wants channel-major input, so on that layout it first
// copied the 96k x 512 activation (196 MB for a 30 s segment) and then normalised it: ~1 ms per
// forward.  Here: pass 1 reduces per-channel sums over time (column tiles, coalesced 256-B row
// segments, fp64 partials), pass 2 normalises, applies the affine and the exact (erf) GELU in
// one read + one write.  HBM-bound: ~3 x 4 B x L x C moved.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wx_attention_unit.h"  // (and through it wx_half.h, wx_host.h, wx_wave.h)

namespace wxe {

constexpr int kCols = 64;    // channels per column tile (one wave-row of 64 lanes: 256 B)
constexpr int kRows = 4;     // waves per block, each striding rows
constexpr int kSplit = 256;  // row slices per channel tile in pass 1

// A block's kRows wave partials (s, q) of kCols columns, summed through LDS: wave 0 gets the sums
// (.x, .y) of column `col`, the other waves what they gave.  In wave order, the own partial first;
// PAIRWISE: (0 + 1) + (2 + 3).  Each caller keeps the order it was measured and pinned with.
// (Arguments and result by value: partials passed by reference stay in memory until this is inlined,
// and the loop that sums them is then compiled differently.)
template <bool PAIRWISE = false>
__device__ __forceinline__ double2 wave_partials(int wv, int col, double s, double q) {
    __shared__ double ss[kRows][kCols], qq[kRows][kCols];
    ss[wv][col] = s;
    qq[wv][col] = q;
    __syncthreads();
    if (wv == 0) {
        if constexpr (PAIRWISE) {
            static_assert(kRows == 4, "two pairs");
            s = (ss[0][col] + ss[1][col]) + (ss[2][col] + ss[3][col]);
            q = (qq[0][col] + qq[1][col]) + (qq[2][col] + qq[3][col]);
        } else {
            for (int r = 1; r < kRows; ++r) {
                s += ss[r][col];
                q += qq[r][col];
            }
        }
    }
    return make_double2(s, q);
}

// A channel's (sum, sum of squares) over L values, folded with the affine: y = x * a + b with a = ab[c],
// b = ab[C + c]
__device__ __forceinline__ void chan_fold(double s, double q, int64_t L, int c, int C, const float* __restrict__ gamma,
                                          const float* __restrict__ beta, float eps, float* __restrict__ ab) {
    const double mean = s / (double)L;
    const double var = fmax(q / (double)L - mean * mean, 0.0);  // biased, as GroupNorm
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const double g = gamma ? (double)gamma[c] : 1.0, b = beta ? (double)beta[c] : 0.0;
    ab[c] = (float)(rstd * g);
    ab[C + c] = (float)(b - mean * rstd * g);
}

// pass 1: partial (sum, sum of squares) per (row slice, channel) in fp64
__global__ __launch_bounds__(kCols * kRows) void chan_stats_kernel(const float* __restrict__ x, int64_t L, int C,
                                                                  double* __restrict__ part /* [kSplit][2][C] */) {
    const int c = blockIdx.x * kCols + (threadIdx.x & (kCols - 1));
    const int r0 = threadIdx.x / kCols;
    const int slice = blockIdx.y;
    const int64_t per = (L + kSplit - 1) / kSplit;
    const int64_t lo = slice * per, hi = min(L, lo + per);
    double s = 0.0, q = 0.0;
    if (c < C) {
        for (int64_t t = lo + r0; t < hi; t += kRows) {
            const double v = (double)x[t * C + c];
            s += v;
            q += v * v;
        }
    }
    const double2 sq = wave_partials(r0, threadIdx.x & (kCols - 1), s, q);
    if (r0 == 0 && c < C) {
        part[(int64_t)slice * 2 * C + c] = sq.x;
        part[(int64_t)slice * 2 * C + C + c] = sq.y;
    }
}

// mean / rstd per channel from the partials, folded with the affine: y = x * a + b
__global__ void chan_finish_kernel(const double* __restrict__ part, int64_t L, int C, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float eps, float* __restrict__ ab /* [2][C] */) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < kSplit; ++k) {
        s += part[(int64_t)k * 2 * C + c];
        q += part[(int64_t)k * 2 * C + C + c];
    }
    chan_fold(s, q, L, c, C, gamma, beta, eps, ab);
}

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// pass 2: y = gelu(x * a[c] + b[c]), float4 per thread along channels
__global__ __launch_bounds__(256) void chan_apply_kernel(const float* __restrict__ x, int64_t n4, int C4,
                                                          const float* __restrict__ ab, int C, int gelu,
                                                          float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)(i % C4) * 4;
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    float o[4] = {v.x * ab[c] + ab[C + c], v.y * ab[c + 1] + ab[C + c + 1], v.z * ab[c + 2] + ab[C + c + 2],
                  v.w * ab[c + 3] + ab[C + c + 3]};
    if (gelu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = gelu_erf(o[k]);
    }
    reinterpret_cast<float4*>(y)[i] = make_float4(o[0], o[1], o[2], o[3]);
}

// ------------------------------------------------------------------------------------
// The feature encoder's first layer as one pass over its output: conv (1 input channel, k taps,
// stride s: wav2vec2's 512 x 10 / 5) -> GroupNorm(one group per channel, over time) -> exact
// GELU, time-major [Lout, C].  Through the GEMM route this layer was a bias fill, a K = 10 GEMM
// writing 196 MB per 30 s segment (~12 TFLOP/s: HBM-bound on its own output), and the three
// channel-norm kernels reading it back twice (~230 us).  Here pass 1 computes the convolution in
// registers and reduces per-channel fp64 (sum, sum of squares) without writing it; pass 2
// recomputes it (k multiply-adds per value, cheaper than reading it back) and writes
// gelu(v * a[c] + b[c]) once.  A thread owns one channel (its k weights in registers) over
// kC0Rows consecutive rows; a wave covers 64 consecutive channels, so every row's store is 256
// contiguous bytes and the k waveform samples of a row are the same for the whole wave.
// The conv bias is not read: GroupNorm with one group per channel subtracts the channel's mean, so a
// per-channel constant cancels exactly, and a convolution summed onto a bias some tens of times the
// signal's spread lost the digits the normalisation then magnifies (tests/test_gpu_conv_probes.py:
// test_conv0_channel_norm_silence, 2.7e-5 against fp64 where fp32 torch is within 4.5e-6).
constexpr int kC0Rows = 16;  // rows per thread
constexpr int kC0MaxK = 16;  // taps held in registers

template <int K>
__device__ __forceinline__ float conv0_at(const float* __restrict__ x, int64_t t, int stride, const float (&w)[K]) {
    const float* xr = x + t * stride;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) v = v + xr[j] * w[j];  // (-ffp-contract=off: separate multiply and add)
    return v;
}

template <int K>
__global__ __launch_bounds__(256) void conv0_stats_kernel(const float* __restrict__ x, int64_t L, int stride,
                                                          const float* __restrict__ wt, int C,
                                                          double* __restrict__ part /* [nblk][2][C] */) {
    const int c = blockIdx.x * kCols + (threadIdx.x & (kCols - 1));
    const int wv = threadIdx.x / kCols;
    float w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = c < C ? wt[(int64_t)c * K + j] : 0.f;
    const int64_t t0 = ((int64_t)blockIdx.y * kRows + wv) * kC0Rows;
    double s = 0.0, q = 0.0;
    for (int r = 0; r < kC0Rows; ++r) {
        const int64_t t = t0 + r;
        if (t >= L) break;
        const double v = (double)conv0_at<K>(x, t, stride, w);
        s += v;
        q += v * v;
    }
    const double2 sq = wave_partials(wv, threadIdx.x & (kCols - 1), s, q);
    if (wv == 0 && c < C) {
        part[(int64_t)blockIdx.y * 2 * C + c] = sq.x;
        part[(int64_t)blockIdx.y * 2 * C + C + c] = sq.y;
    }
}

// (a, b) per channel from nblk partials: 4 row groups per channel tile sum a quarter each with
// 8 loads in flight, combined in group order
__global__ __launch_bounds__(256) void conv0_finish_kernel(const double* __restrict__ part, int nblk, int64_t L, int C,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, float* __restrict__ ab) {
    const int c = blockIdx.x * kCols + (threadIdx.x & (kCols - 1));
    const int g = threadIdx.x / kCols;
    double s = 0.0, q = 0.0;
    if (c < C) {
        const int lo = g * nblk / kRows, hi = (g + 1) * nblk / kRows;
        int k = lo;
        for (; k + 8 <= hi; k += 8) {
            double vs[8], vq[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                vs[u] = part[(int64_t)(k + u) * 2 * C + c];
                vq[u] = part[(int64_t)(k + u) * 2 * C + C + c];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s += vs[u];
                q += vq[u];
            }
        }
        for (; k < hi; ++k) {
            s += part[(int64_t)k * 2 * C + c];
            q += part[(int64_t)k * 2 * C + C + c];
        }
    }
    const double2 sq = wave_partials(g, threadIdx.x & (kCols - 1), s, q);
    if (g == 0 && c < C) chan_fold(sq.x, sq.y, L, c, C, gamma, beta, eps, ab);
}

// The apply passes' store (ET: wx::kF32, or the dtype of wx_conv0_channel_norm_h16): the fp32 value,
// computed by the same expressions whatever ET is, rounded to nearest even on the way out.
template <int ET>
struct C0Out {
    using type = short;
    static __device__ __forceinline__ short put(float v) { return wx::round16<ET>(v); }
};
template <>
struct C0Out<wx::kF32> {
    using type = float;
    static __device__ __forceinline__ float put(float v) { return v; }
};

template <int K, int ET = wx::kF32>
__global__ __launch_bounds__(256) void conv0_apply_kernel(const float* __restrict__ x, int64_t L, int stride,
                                                          const float* __restrict__ wt, int C,
                                                          const float* __restrict__ ab, int gelu,
                                                          typename C0Out<ET>::type* __restrict__ y) {
    const int c = blockIdx.x * kCols + (threadIdx.x & (kCols - 1));
    const int wv = threadIdx.x / kCols;
    if (c >= C) return;
    float w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = wt[(int64_t)c * K + j];
    const float sa = ab[c], sb = ab[C + c];
    const int64_t t0 = ((int64_t)blockIdx.y * kRows + wv) * kC0Rows;
#pragma unroll 4
    for (int r = 0; r < kC0Rows; ++r) {
        const int64_t t = t0 + r;
        if (t >= L) break;
        float v = conv0_at<K>(x, t, stride, w) * sa + sb;
        if (gelu) v = gelu_erf(v);
        y[t * C + c] = C0Out<ET>::put(v);
    }
}

// The same two passes for wav2vec2's geometry (K = 10 taps, stride 5), register-resident: a
// wave covers 32 consecutive rows x 64 channels, and the 165 waveform samples those rows read
// are loaded once (3 coalesced loads per lane) and broadcast per use with v_readlane (the
// sample index is uniform over the wave), instead of 10 dependent global loads per row
// (the generic kernels above: ~90 us per pass for a 30 s segment, latency-bound).  fma
// accumulation (equal to torch's conv to fp32 tolerance, like the generic path).
constexpr int kC0R = 32;  // rows per wave

template <int K, int S>
__device__ __forceinline__ float conv0_row(const float (&sv)[((kC0R - 1) * S + K + 63) / 64], int r,
                                           const float (&w)[K]) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int k = r * S + j;
        acc = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv[k >> 6]), k & 63)), w[j], acc);
    }
    return acc;
}

template <int K, int S>
__device__ __forceinline__ void conv0_samples(const float* __restrict__ x, int64_t nsamp, int64_t t0,
                                              float (&sv)[((kC0R - 1) * S + K + 63) / 64]) {
    constexpr int NV = ((kC0R - 1) * S + K + 63) / 64;
    const int l = threadIdx.x & 63;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int64_t i = t0 * S + 64 * v + l;
        sv[v] = i < nsamp ? x[i] : 0.f;
    }
}

// A wave whose kC0R rows read only samples inside the waveform (all but the last) reads them
// straight from memory at wave-uniform addresses: scalar loads into SGPRs that the FMAs take as
// operands — no v_readlane per tap and none of the SGPR-hazard s_nops after it (the register
// form, conv0_samples + conv0_row, stays for the last wave).  Same fma chain per row.
template <int K, int S>
__device__ __forceinline__ float conv0_row_s(const float* __restrict__ xs /* wave-uniform */, int r,
                                             const float (&w)[K]) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) acc = fmaf(xs[r * S + j], w[j], acc);
    return acc;
}

// The register-resident passes' walk over a wave's rows, the channel's taps in w:
// acc = f(acc, r, v) for r = 0 .. kC0R - 1, v the convolution at row t0 + r, on whichever of the two
// forms the wave's samples allow.  Rows at or past L are walked too (their samples read as zeros): f
// tests r.  What a pass carries from row to row goes through acc by value (the apply pass: nothing):
// sums that f updated through references were compiled to a branch per row, with the sample loads
// split between them, instead of the selects and the ten 16-dword loads of the loops written out.
template <int K, int S, class A, class F>
__device__ __forceinline__ A conv0_rows_rl(const float* __restrict__ x, int64_t nsamp, int64_t t0,
                                           const float (&w)[K], A acc, F f) {
    if (t0 * S + (kC0R - 1) * S + K <= nsamp) {
        const float* xs = x + t0 * S;
#pragma unroll
        for (int r = 0; r < kC0R; ++r) acc = f(acc, r, conv0_row_s<K, S>(xs, r, w));
    } else {
        float sv[((kC0R - 1) * S + K + 63) / 64];
        conv0_samples<K, S>(x, nsamp, t0, sv);
#pragma unroll
        for (int r = 0; r < kC0R; ++r) acc = f(acc, r, conv0_row<K, S>(sv, r, w));
    }
    return acc;
}

template <int K, int S>
__global__ __launch_bounds__(256) void conv0_stats_rl_kernel(const float* __restrict__ x, int64_t nsamp, int64_t L,
                                                             const float* __restrict__ wt, int C,
                                                             double* __restrict__ part /* [nblk][2][C] */) {
    const int lc = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int c = blockIdx.x * 64 + lc;
    const int cc = min(c, C - 1);
    float w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = wt[(int64_t)cc * K + j];
    const int64_t t0 = ((int64_t)blockIdx.y * kRows + wv) * kC0R;
    const int64_t nr = L - t0;
    const auto add = [=](double2 a, int r, float v) {  // a: (sum, sum of squares)
        const double d = (double)v;
        if (r < nr) {
            a.x += d;
            a.y = fma(d, d, a.y);
        }
        return a;
    };
    const double2 own = conv0_rows_rl<K, S>(x, nsamp, t0, w, make_double2(0.0, 0.0), add);
    const double2 sq = wave_partials<true>(wv, lc, own.x, own.y);
    if (wv == 0 && c < C) {
        part[(int64_t)blockIdx.y * 2 * C + c] = sq.x;
        part[(int64_t)blockIdx.y * 2 * C + C + c] = sq.y;
    }
}

template <int K, int S, int ET = wx::kF32>
__global__ __launch_bounds__(256) void conv0_apply_rl_kernel(const float* __restrict__ x, int64_t nsamp, int64_t L,
                                                             const float* __restrict__ wt, int C,
                                                             const float* __restrict__ ab, int gelu,
                                                             typename C0Out<ET>::type* __restrict__ y) {
    const int lc = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int c = blockIdx.x * 64 + lc;
    const int cc = min(c, C - 1);
    float w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = wt[(int64_t)cc * K + j];
    const float sa = ab[cc], sb = ab[C + cc];
    const int64_t t0 = ((int64_t)blockIdx.y * kRows + wv) * kC0R;
    const int64_t nr = L - t0;
    typename C0Out<ET>::type* yr = y + t0 * C + c;  // (row r at yr + r C)
    conv0_rows_rl<K, S>(x, nsamp, t0, w, 0, [=](int, int r, float v) {
        v = v * sa + sb;
        if (gelu) v = gelu_erf(v);
        if (r < nr && c < C) yr[(int64_t)r * C] = C0Out<ET>::put(v);
        return 0;
    });
}

// ------------------------------------------------------------------------------------
// wav2vec2 self-attention, fp32 (alignment.py:226-233: the encoder's 12 / 24 attention layers,
// one unpadded segment per forward, no mask).  torch's fused attention kernel for fp32
// (aotriton attn_fwd) took 34% of config 3's GPU time at ~26 TFLOP/s (profiles/
// r2_config3_kernel_stats.csv: 246 us per layer of a 29 s chunk).  Here: attn_mfma32_unit
// (wx_attention_unit.h: the flash-attention forward on the f32-input MFMA, square and unmasked),
// one workgroup per (batch, head, 32-query tile) whose SPLIT waves take every SPLIT-th 32-key tile
// (a single 30 s segment has only 12 x 47 query tiles).
// Not bit-identical to torch's kernel (different summation order); tests compare it with
// torch's attention at fp32 tolerance and the whole prepared forward with the stock one.
constexpr int kAttnSplit = 4;  // waves per 32-query tile, each over every kAttnSplit-th 32-key tile

// amdgpu_waves_per_eu(2): two waves per SIMD, stated so the allocator keeps everything in VGPRs
// instead of splitting them with AGPR copies (A/B: 1-2% faster).  A third wave per SIMD (168
// registers: V loaded behind the S chain instead of a tile ahead, 2 spills) was 10-15% slower.
// Round 6: the K / V loads through per-tile buffer descriptors (no per-lane address arithmetic) and
// no key compare on whole tiles took 12 packed 30 s segments (H = 12) from 818 to 727 us per call;
// PMC before the change: 327 VALU instructions per (wave, key tile) beside 64 MFMAs, ~150 of them
// address arithmetic (32-bit multiplies and 64-bit adds), MFMA busy 65% of the cycles.  With it the
// software-pipelined one-wave form of the same kernel (tile k + 1's S chain beside tile k's softmax,
// +2% before) measured equal (729 us) and was removed.  On the shared body (213-215 VGPRs) the same
// call measured 717 / 730 / 719 us at SPLIT 1 / 2 / 4 beside 722 / 734 / 725 us for the kernel it
// replaced, in one session.
// SPLIT waves per 32-query tile (SPLIT = 1: one wave, no merge); PACKED: one launch over many
// segments of their own lengths (rows packed back to back: wx_attention_f32_packed)
template <int SPLIT, bool PACKED>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(2))) void attn_f32_kernel(wx::AttnArgs a) {
    const float *q = static_cast<const float*>(a.q), *k = static_cast<const float*>(a.k), *v = static_cast<const float*>(a.v);
    int T, b = 0, h, tile;
    int64_t row0 = 0;  // first row of this packed segment
    const unsigned w = wx::xcd_unit();
    if constexpr (PACKED) {
        wx::packed_unit(w, a.seg_rows, a.seg_units, a.nseg, 32, row0, T, h, tile);
    } else {
        T = a.Tq;
        wx::dense_unit(w, (T + 31) / 32, a.H, b, h, tile);
    }
    wx::attn_mfma32_unit<wx::kF32, SPLIT>(q + b * a.qs[0] + h * a.qs[1] + row0 * a.qs[2],
                                          k + b * a.ks[0] + h * a.ks[1] + row0 * a.ks[2],
                                          v + b * a.vs[0] + h * a.vs[1] + row0 * a.vs[2],
                                          static_cast<float*>(a.o) + ((row0 + (int64_t)b * T) * a.H + h) * 64, T, T, -1, tile,
                                          a.qs[2], a.ks[2], a.vs[2], (int64_t)a.H * 64, a.scale_log2);
}

// ------------------------------------------------------------------------------------
// wav2vec2 positional convolution over packed segments (alignment.py:226-233: the encoder's
// Wav2Vec2PositionalConvEmbedding — Conv1d(D, D, K = 128, padding K / 2, groups G), the last
// output dropped, GELU — run per segment, zero padding at each segment's own ends).  As
// GEMMs it is G x [T, K Cg] x [K Cg, Cg] per segment with a patch operand (im2col of 128
// shifted rows) that torch had to gather, 4 x 32-tap blocks: 0.42 ms per 30 s segment at
// ~34 TFLOP/s.  Here one block per (segment, 128-frame tile, group): the tile's input window
// (255 rows x Cg channels) sits in LDS once and every tap reads its A fragments from it
// shifted by one row; the group's weights stream tap by tap through a double-buffered LDS
// slab (register-staged a tap ahead).  4 waves x 32 frames x Cg outputs on
// v_mfma_f32_16x16x4_f32 (exact f32 fma chains: not bit-identical to torch's conv, whose
// summation order differs); bias, erf GELU and optionally the residual (h + pos) fused.
constexpr int kPcFrames = 128;  // output frames per block (4 waves x 32)
constexpr int kPcK = 128;       // taps (wav2vec2's num_conv_pos_embeddings)
constexpr int kPcBlock = 4;     // taps per summation block (a power of two that divides kPcK)
static_assert(kPcK % kPcBlock == 0 && (kPcBlock & (kPcBlock - 1)) == 0, "posconv: whole blocks of taps");
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct PosConvArgs {
    const float* h;      // [rows, D] packed segments
    const float* w;      // [G][K][Cg / 4][Cg][4]: w[g][j][i / 4][o][i % 4] = conv.weight[g Cg + o][i][j]
    const float* bias;   // [D] or null
    float* out;          // [rows, D]
    const int32_t* seg_rows;
    const int32_t* seg_tiles;  // prefix of ceil(T_s / kPcFrames)
    int nseg, D;
    int residual;
};

template <int CG>
__global__ __launch_bounds__(256) void posconv_kernel(PosConvArgs a) {
    constexpr int RS = CG + 4;  // window row stride (floats): 16-B rows, banks spread over 16 rows
    constexpr int WR = kPcFrames + kPcK - 1;
    constexpr int NOB = CG / 16, NIC = CG / 16;
    constexpr int NB4 = CG * CG / 4;  // float4 per tap of the group's weights
    constexpr int PER = (NB4 + 255) / 256;
    __shared__ __attribute__((aligned(16))) float xa[WR * RS];
    __shared__ __attribute__((aligned(16))) float wb[2][CG * CG];
    const int g = blockIdx.y;
    const int w = blockIdx.x;
    int lo = 0, hi = a.nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.seg_tiles[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    const int row0 = a.seg_rows[lo];
    const int T = a.seg_rows[lo + 1] - row0;
    const int t0 = (w - a.seg_tiles[lo]) * kPcFrames;
    const float* hg = a.h + (int64_t)row0 * a.D + g * CG;
    // the input window: row r <-> segment frame t0 - K / 2 + r (zero outside [0, T))
    for (int e = threadIdx.x; e < WR * (CG / 4); e += 256) {
        const int r = e / (CG / 4), c4 = e - r * (CG / 4);
        const int t = t0 - kPcK / 2 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < T) v = *reinterpret_cast<const float4*>(hg + (int64_t)t * a.D + 4 * c4);
        *reinterpret_cast<float4*>(xa + r * RS + 4 * c4) = v;
    }
    const float4* wg = reinterpret_cast<const float4*>(a.w) + (int64_t)g * kPcK * NB4;
    // the next tap's weights in named registers, loaded unconditionally (the last slot of a
    // partial tap re-reads a valid element, not stored) and pinned above the tap's MFMAs by a
    // sched_barrier: a register array with conditional stores had hipcc sink each load into
    // its store's branch after the MFMAs — a global round trip per slot and tap
    static_assert(PER <= 4, "posconv: at most four float4 slots per thread");
    float4 b0, b1, b2, b3;
    auto bload = [&](int j) {
        const float4* src = wg + (int64_t)j * NB4;
        const int t = (int)threadIdx.x;
        b0 = src[min(t, NB4 - 1)];
        if constexpr (PER > 1) b1 = src[min(t + 256, NB4 - 1)];
        if constexpr (PER > 2) b2 = src[min(t + 512, NB4 - 1)];
        if constexpr (PER > 3) b3 = src[min(t + 768, NB4 - 1)];
    };
    auto bstore = [&](int buf) {
        float4* dst = reinterpret_cast<float4*>(wb[buf]);
        const int t = (int)threadIdx.x;
        if (t < NB4) dst[t] = b0;
        if constexpr (PER > 1) if (t + 256 < NB4) dst[t + 256] = b1;
        if constexpr (PER > 2) if (t + 512 < NB4) dst[t + 512] = b2;
        if constexpr (PER > 3) if (t + 768 < NB4) dst[t + 768] = b3;
    };
    bload(0);
    bstore(0);
    __syncthreads();
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, r16 = l & 15;
    // Blocked summation: kPcBlock taps (kPcBlock Cg products) are summed in `part` and then added to
    // the total.  One chain over all K Cg = 6,144 / 8,192 products was 6 to 9 times less accurate than
    // torch's fp32 conv (tests/test_gpu_conv_probes.py: test_posconv_against_fp64); the error now grows
    // with the block length and the block count instead of with their product.
    f32x4 acc[2][NOB], part[2][NOB];
#pragma unroll
    for (int fb = 0; fb < 2; ++fb)
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) acc[fb][ob] = part[fb][ob] = f32x4{0.f, 0.f, 0.f, 0.f};
    // A fragment rows: frame wv 32 + 16 fb + r16 of the tile, shifted by the tap
    const float* xrow = xa + (wv * 32 + r16) * RS + 4 * q;
    auto tap = [&](int j) {
        if (j + 1 < kPcK) bload(j + 1);
        __builtin_amdgcn_sched_barrier(0);
        const float* bb = wb[j & 1] + (q * CG + r16) * 4;
#pragma unroll
        for (int ic = 0; ic < NIC; ++ic) {
            float4 av[2], bv[NOB];
#pragma unroll
            for (int fb = 0; fb < 2; ++fb) av[fb] = *reinterpret_cast<const float4*>(xrow + (16 * fb + j) * RS + 16 * ic);
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) bv[ob] = *reinterpret_cast<const float4*>(bb + (ic * 4 * CG + 16 * ob) * 4);
#pragma unroll
            for (int fb = 0; fb < 2; ++fb)
#pragma unroll
                for (int ob = 0; ob < NOB; ++ob) {
                    part[fb][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[fb].x, bv[ob].x, part[fb][ob], 0, 0, 0);
                    part[fb][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[fb].y, bv[ob].y, part[fb][ob], 0, 0, 0);
                    part[fb][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[fb].z, bv[ob].z, part[fb][ob], 0, 0, 0);
                    part[fb][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[fb].w, bv[ob].w, part[fb][ob], 0, 0, 0);
                }
        }
        if (j + 1 < kPcK) bstore((j + 1) & 1);
        __syncthreads();
    };
    // (the tap loop unrolled by the block: with the block's end behind a branch in the rolled loop the
    // Cg = 48 instance was 10% slower than the single chain, this way it is 4% faster)
    for (int jb = 0; jb < kPcK; jb += kPcBlock) {
#pragma unroll
        for (int jj = 0; jj < kPcBlock; ++jj) tap(jb + jj);
#pragma unroll
        for (int fb = 0; fb < 2; ++fb)
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) {
                acc[fb][ob] += part[fb][ob];
                part[fb][ob] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
    }
    // accumulator (fb, ob) register v: frame 16 fb + 4 q + v of the wave's 32, output 16 ob + r16
#pragma unroll
    for (int fb = 0; fb < 2; ++fb)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int t = t0 + wv * 32 + 16 * fb + 4 * q + v;
            if (t >= T) continue;
            const int64_t rb = (int64_t)(row0 + t) * a.D + g * CG;
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) {
                const int c = 16 * ob + r16;
                float y = acc[fb][ob][v] + (a.bias ? a.bias[g * CG + c] : 0.f);
                y = gelu_erf(y);
                if (a.residual) y += a.h[rb + c];
                a.out[rb + c] = y;
            }
        }
}

}  // namespace wxe

extern "C" size_t wx_channel_norm_workspace_bytes(int32_t C) {
    return (size_t)wxe::kSplit * 2 * C * sizeof(double) + 2 * (size_t)C * sizeof(float);
}

extern "C" int wx_channel_norm(const float* x, int64_t L, int32_t C, const float* gamma, const float* beta, float eps,
                               int32_t gelu, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace wxe;
    if (L < 0 || C <= 0 || (C & 3) || !x || !y || !workspace) return WX_E_INVALID;
    if (workspace_bytes < wx_channel_norm_workspace_bytes(C)) return WX_E_WORKSPACE;
    if (L == 0) return WX_OK;
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(y) & 15)) return WX_E_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* part = reinterpret_cast<double*>(workspace);
    float* ab = reinterpret_cast<float*>(part + (size_t)kSplit * 2 * C);
    hipLaunchKernelGGL(chan_stats_kernel, dim3((C + kCols - 1) / kCols, kSplit), dim3(kCols * kRows), 0, st, x, L, C,
                       part);
    hipLaunchKernelGGL(chan_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, st, part, L, C, gamma, beta, eps, ab);
    const int64_t n4 = L * (C / 4);
    hipLaunchKernelGGL(chan_apply_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, x, n4, C / 4, ab, C,
                       gelu, y);
    return wx::launch_status();
}

extern "C" size_t wx_conv0_channel_norm_workspace_bytes(int64_t L, int32_t C) {
    if (L <= 0 || C <= 0) return 0;
    const int64_t nblk = (L + wxe::kRows * wxe::kC0Rows - 1) / (wxe::kRows * wxe::kC0Rows);
    return (size_t)nblk * 2 * C * sizeof(double) + 2 * (size_t)C * sizeof(float);
}

namespace wxe {

// wx_conv0_channel_norm (ET wx::kF32, y fp32) and wx_conv0_channel_norm_h16 (ET its dtype, y 16 bit):
// the same statistics passes, the apply pass instantiated for the output type
template <int ET>
static int conv0_channel_norm(const float* x, int64_t S, int32_t K, int32_t stride, const float* w, int32_t C,
                              const float* gamma, const float* beta, float eps, int32_t gelu, void* yv, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (S < 0 || C <= 0 || K < 1 || K > kC0MaxK || stride < 1 || !x || !w || !yv) return WX_E_INVALID;
    typename C0Out<ET>::type* y = static_cast<typename C0Out<ET>::type*>(yv);
    const int64_t L = S >= K ? (S - K) / stride + 1 : 0;
    if (L == 0) return WX_OK;
    if (!workspace || workspace_bytes < wx_conv0_channel_norm_workspace_bytes(L, C)) return WX_E_WORKSPACE;
    const bool rl = K == 10 && stride == 5;  // wav2vec2's geometry: the register-resident kernels
    const int64_t rows_per_blk = rl ? 4 * kC0R : kRows * kC0Rows;
    const int64_t nblk = (L + rows_per_blk - 1) / rows_per_blk;
    if (nblk > 65535) return WX_E_INVALID;  // (grid y; ~4.2 h of 16 kHz audio at stride 5)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* part = reinterpret_cast<double*>(workspace);
    float* ab = reinterpret_cast<float*>(part + (size_t)nblk * 2 * C);
    if (rl) {
        const dim3 grid((C + 63) / 64, (unsigned)nblk);
        hipLaunchKernelGGL((conv0_stats_rl_kernel<10, 5>), grid, dim3(256), 0, st, x, S, L, w, C, part);
        hipLaunchKernelGGL(conv0_finish_kernel, dim3((C + kCols - 1) / kCols), dim3(kCols * kRows), 0, st, part,
                           (int)nblk, L, C, gamma, beta, eps, ab);
        hipLaunchKernelGGL((conv0_apply_rl_kernel<10, 5, ET>), grid, dim3(256), 0, st, x, S, L, w, C, ab, gelu, y);
        return wx::launch_status();
    }
    const dim3 grid((C + kCols - 1) / kCols, (unsigned)nblk), blk(kCols * kRows);
#define WX_C0(KK)                                                                                              \
    case KK:                                                                                                   \
        hipLaunchKernelGGL(conv0_stats_kernel<KK>, grid, blk, 0, st, x, L, stride, w, C, part);           \
        hipLaunchKernelGGL(conv0_finish_kernel, dim3((C + kCols - 1) / kCols), blk, 0, st, part, (int)nblk, L, C, \
                           gamma, beta, eps, ab);                                                              \
        hipLaunchKernelGGL((conv0_apply_kernel<KK, ET>), grid, blk, 0, st, x, L, stride, w, C, ab, gelu, y); \
        break;
    switch (K) {
        WX_C0(1) WX_C0(2) WX_C0(3) WX_C0(4) WX_C0(5) WX_C0(6) WX_C0(7) WX_C0(8) WX_C0(9) WX_C0(10) WX_C0(11)
        WX_C0(12) WX_C0(13) WX_C0(14) WX_C0(15) WX_C0(16)
        default: return WX_E_INVALID;
    }
#undef WX_C0
    return wx::launch_status();
}

}  // namespace wxe

extern "C" int wx_conv0_channel_norm(const float* x, int64_t S, int32_t K, int32_t stride, const float* w,
                                     const float* bias, int32_t C, const float* gamma, const float* beta, float eps,
                                     int32_t gelu, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    (void)bias;  // cancels in the per-channel normalisation (see above): never added
    return wxe::conv0_channel_norm<wx::kF32>(x, S, K, stride, w, C, gamma, beta, eps, gelu, y, workspace, workspace_bytes,
                                      stream);
}

extern "C" int wx_conv0_channel_norm_h16(const float* x, int64_t S, int32_t K, int32_t stride, const float* w,
                                         const float* bias, int32_t C, const float* gamma, const float* beta, float eps,
                                         int32_t gelu, int32_t dtype, void* y, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    (void)bias;
    if (dtype == WX_DTYPE_F16)
        return wxe::conv0_channel_norm<wx::kF16>(x, S, K, stride, w, C, gamma, beta, eps, gelu, y, workspace,
                                                     workspace_bytes, stream);
    if (dtype == WX_DTYPE_BF16)
        return wxe::conv0_channel_norm<wx::kBF16>(x, S, K, stride, w, C, gamma, beta, eps, gelu, y, workspace,
                                                      workspace_bytes, stream);
    return WX_E_INVALID;
}

extern "C" int wx_attention_f32(const float* q, const float* k, const float* v, float* o, int32_t B, int32_t H,
                                int32_t T, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                                const int64_t* v_strides, float scale, void* stream) {
    using namespace wxe;
    if (B < 0 || H <= 0 || T < 0 || D != 64 || !q || !k || !v || !o || !q_strides || !k_strides || !v_strides)
        return WX_E_INVALID;
    if (B == 0 || T == 0) return WX_OK;
    const int64_t blocks = ((int64_t)T + 31) / 32 * B * H;
    wx::AttnArgs a{};
    if (!wx::attn_args(&a, q, k, v, o, q_strides, k_strides, v_strides, 3, 4, true, blocks, scale)) return WX_E_INVALID;
    a.H = H;
    a.Tq = a.Tk = T;
    const dim3 grid((unsigned)blocks);
    hipLaunchKernelGGL((attn_f32_kernel<kAttnSplit, false>), grid, dim3(64 * kAttnSplit), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    return wx::launch_status();
}

extern "C" int wx_attention_f32_packed(const float* q, const float* k, const float* v, float* o, int32_t nseg,
                                       const int32_t* seg_rows, const int32_t* seg_units, int32_t n_units,
                                       int32_t H, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                                       const int64_t* v_strides, float scale, int32_t split, void* stream) {
    using namespace wxe;
    if (nseg < 0 || H <= 0 || D != 64 || n_units < 0 || !q || !k || !v || !o || !q_strides || !k_strides ||
        !v_strides)
        return WX_E_INVALID;
    if (nseg == 0 || n_units == 0) return WX_OK;
    if (!seg_rows || !seg_units) return WX_E_INVALID;
    wx::AttnArgs a{};  // (strides {head, row}: batch 0)
    if (!wx::attn_args(&a, q, k, v, o, q_strides, k_strides, v_strides, 2, 4, true, n_units, scale)) return WX_E_INVALID;
    a.H = H;
    a.seg_rows = seg_rows;
    a.seg_units = seg_units;
    a.nseg = nseg;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // a few segments' units leave SIMDs idle unless each query tile's keys are split over waves;
    // with ~10 units per CU or more, one wave per tile (no merge) keeps them as busy
    if (split <= 0) split = n_units >= 2560 ? 1 : 4;
    switch (split) {
        case 1: hipLaunchKernelGGL((attn_f32_kernel<1, true>), dim3((unsigned)n_units), dim3(64), 0, s, a); break;
        case 2: hipLaunchKernelGGL((attn_f32_kernel<2, true>), dim3((unsigned)n_units), dim3(128), 0, s, a); break;
        case 4: hipLaunchKernelGGL((attn_f32_kernel<4, true>), dim3((unsigned)n_units), dim3(256), 0, s, a); break;
        default: return WX_E_INVALID;
    }
    return wx::launch_status();
}

extern "C" int wx_posconv_packed(const float* h, int32_t D, const float* w_packed, const float* bias, int32_t G,
                                 int32_t K, int32_t nseg, const int32_t* seg_rows, const int32_t* seg_tiles,
                                 int32_t n_tiles, int32_t residual, float* out, void* stream) {
    using namespace wxe;
    if (!h || !w_packed || !out || G <= 0 || D <= 0 || D % G || nseg < 0 || n_tiles < 0) return WX_E_INVALID;
    if (K != kPcK) return WX_E_INVALID;
    if (nseg == 0 || n_tiles == 0) return WX_OK;
    if (!seg_rows || !seg_tiles || G > 65535) return WX_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(h) & 15) || (D & 3)) return WX_E_INVALID;
    PosConvArgs a;
    a.h = h;
    a.w = w_packed;
    a.bias = bias;
    a.out = out;
    a.seg_rows = seg_rows;
    a.seg_tiles = seg_tiles;
    a.nseg = nseg;
    a.D = D;
    a.residual = residual;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n_tiles, (unsigned)G);
    switch (D / G) {
        case 48: hipLaunchKernelGGL(posconv_kernel<48>, grid, dim3(256), 0, s, a); break;
        case 64: hipLaunchKernelGGL(posconv_kernel<64>, grid, dim3(256), 0, s, a); break;
        default: return WX_E_INVALID;
    }
    return wx::launch_status();
}
