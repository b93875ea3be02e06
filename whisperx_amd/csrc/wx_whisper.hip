// wx_whisper.hip — the stem of Whisper's audio encoder (whisperx/asr.py:77-86, WhisperModel.encode:
// the reference hands the features to CTranslate2; the arithmetic is transformers'
// WhisperEncoder.forward): conv1 (k = 3, padding 1) + GELU, conv2 (k = 3, stride 2, padding 1) +
// GELU, + positional table, from channel-major mel features to time-major rows.  C ABI and
// semantics: include/wx_align.h (wx_whisper_stem).
//
// Both convolutions are implicit GEMMs on v_mfma_f32_16x16x4_f32, computed transposed,
// D[channel][time] = W . window^T: the accumulator then holds 4 consecutive output channels of one
// output row per lane, so the epilogue (bias, erf GELU, positional row) ends in one 16-byte
// time-major store per lane and tile.  No patch buffer: a tap is a row shift of the LDS window.
//
// One block of 4 waves per (chunk, 64 output rows, 64 NT output channels):
//   - The block stages its input window time-major in LDS.  conv1 stages all n_mels channels of
//     rows t0 - 1 .. t0 + 64 at once, transposing the channel-major features on the way; conv2
//     walks the D input channels of the time-major conv1 activation in chunks of 64, rows
//     2 u0 - 1 .. 2 u0 + 127.  Rows outside the chunk's own [0, Tin) are zeros: padding is per
//     chunk, never a neighbour's row.  Row stride 136 / 68 floats: the row step of the 16 rows of a
//     ds_read_b128 (1 row for conv1, 2 for conv2) is then 8 mod 64 banks, conflict-free over the
//     instruction's lane groups.
//   - Wave w owns the 16-channel weight tiles w, w + 4, ... (NT of them) for all 4 row tiles: each
//     host-packed weight fragment is one coalesced 16-byte load per lane (from L2), used against
//     the 4 row fragments read from LDS: 16 MFMAs per weight load.
//   - Each tap of a chunk is summed in an accumulator of its own and then added to the total
//     (blocks of CH products): a single chain over K = 3 Cin was less accurate than torch's conv.
//   - Tiles are laid out per chunk (grid z), so a chunk's values do not depend on the batch.
// The time-major conv1 activation a1 [B][Tin][D] in the caller's workspace is the one intermediate.
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wx_host.h"  // (and through it include/wx_align.h)

namespace wxw {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRows = 64;  // output rows per block

struct ConvArgs {
    const float* in;      // conv1: x (channel-major); conv2: a1 (time-major, row stride Cin)
    int64_t in_bs, in_rs;  // conv1: batch / channel-row stride of x; conv2: in_bs only
    const float4* w;      // [Cout / 16][3][Cin / 16][64] float4 (see wx_align.h)
    const float* bias;    // [Cout]
    const float* pos;     // conv2: [Tout][Cout]; conv1: null
    float* out;           // [B][Tout][Cout]
    int32_t Tin, Tout, Cin, Cout;
};

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// S: stride (1: conv1, channel-major input of CH = Cin channels; 2: conv2, time-major input walked
// in chunks of CH = 64 channels).  NT: 16-channel output tiles per wave.
// Registers: conv2 fits 128 VGPRs (4 blocks of 35 KB LDS per CU: one block's staging and barriers
// hide under the others' MFMAs); conv1's unrolled 5 / 8 weight loads per tap want a few more and
// spilled 4 to 8 registers at that budget, so it is bound only to 2 blocks (134 VGPRs: 3 blocks).
template <int S, int CH, int NT>
__global__ __launch_bounds__(256, S == 1 ? 2 : 4) void stem_conv_kernel(const ConvArgs a) {
    constexpr int RS = S == 1 ? 136 : 68;            // window row stride (floats)
    constexpr int WR = (kRows - 1) * S + 3;          // window rows
    constexpr int NIC = CH / 16;                     // k-groups of 16 channels per chunk
    static_assert(CH <= RS && CH % 16 == 0, "window row holds the chunk's channels");
    __shared__ __attribute__((aligned(16))) float xs[WR * RS];
    const int b = blockIdx.z;
    const int u0 = blockIdx.x * kRows;
    const int tid = threadIdx.x;
    const int l = tid & 63, wv = tid >> 6, q = l >> 4, r16 = l & 15;
    const int r_first = S * u0 - 1;  // input row of window row 0
    const int G = a.Cin / 16;
    const int ot0 = blockIdx.y * 4 * NT + wv;  // the wave's weight tiles: ot0 + 4 nt

    f32x4 acc[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) acc[nt][ft] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nchunk = S == 1 ? 1 : a.Cin / CH;
    for (int ck = 0; ck < nchunk; ++ck) {
        if (ck > 0) __syncthreads();  // every wave is done with the previous chunk's window
        if constexpr (S == 1) {
            // x[b][c][t] -> xs[r][c]: 16 consecutive rows x 4 channels per wave instruction
            const float* xb = a.in + (int64_t)b * a.in_bs;
            constexpr int RB = (WR + 15) / 16;  // 16-row bands
            for (int e = tid; e < RB * 16 * CH; e += 256) {
                const int rl = e & 15, cl = (e >> 4) & 3, rest = e >> 6;  // rest = band * (CH / 4) + c / 4
                const int band = rest / (CH / 4), c = 4 * (rest - band * (CH / 4)) + cl;
                const int r = 16 * band + rl;
                if (r < WR) {
                    const int t = r_first + r;
                    xs[r * RS + c] = (t >= 0 && t < a.Tin) ? xb[(int64_t)c * a.in_rs + t] : 0.f;
                }
            }
        } else {
            const float* ab = a.in + (int64_t)b * a.in_bs + ck * CH;
            for (int e = tid; e < WR * (CH / 4); e += 256) {
                const int r = e / (CH / 4), c4 = e - r * (CH / 4);
                const int t = r_first + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t >= 0 && t < a.Tin) v = *reinterpret_cast<const float4*>(ab + (int64_t)t * a.Cin + 4 * c4);
                *reinterpret_cast<float4*>(xs + r * RS + 4 * c4) = v;
            }
        }
        __syncthreads();
        // fragment of (tile ot, tap j, group g): w[((ot * 3 + j) * G + g) * 64 + l]
        const float* xrow = xs + S * r16 * RS + 4 * q;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // one tap of the chunk (CH products) is summed on its own and then added to the total:
            // blocked summation, the error of a K = 3 Cin chain grows with the block count and the
            // block length instead of with K (3,840 at D = 1280)
            f32x4 part[NT][4];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int ft = 0; ft < 4; ++ft) part[nt][ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ic = 0; ic < NIC; ++ic) {
                float4 av[NT], xv[4];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    av[nt] = a.w[((int64_t)((ot0 + 4 * nt) * 3 + j) * G + ck * NIC + ic) * 64 + l];
#pragma unroll
                for (int ft = 0; ft < 4; ++ft)
                    xv[ft] = *reinterpret_cast<const float4*>(xrow + (S * 16 * ft + j) * RS + 16 * ic);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int ft = 0; ft < 4; ++ft) {
                        f32x4 c = part[nt][ft];
                        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[nt].x, xv[ft].x, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[nt].y, xv[ft].y, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[nt].z, xv[ft].z, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[nt].w, xv[ft].w, c, 0, 0, 0);
                        part[nt][ft] = c;
                    }
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int ft = 0; ft < 4; ++ft) acc[nt][ft] += part[nt][ft];
        }
    }

    // accumulator (nt, ft) register v: channel 16 (ot0 + 4 nt) + 4 q + v of row u0 + 16 ft + r16
    float* ob = a.out + (int64_t)b * a.Tout * a.Cout;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int o = 16 * (ot0 + 4 * nt) + 4 * q;
        const float4 bv = *reinterpret_cast<const float4*>(a.bias + o);
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
            const int u = u0 + 16 * ft + r16;
            if (u >= a.Tout) continue;
            const f32x4 c = acc[nt][ft];
            float4 y = make_float4(gelu_erf(c[0] + bv.x), gelu_erf(c[1] + bv.y), gelu_erf(c[2] + bv.z),
                                   gelu_erf(c[3] + bv.w));
            if constexpr (S == 2) {
                const float4 p = *reinterpret_cast<const float4*>(a.pos + (int64_t)u * a.Cout + o);
                y = make_float4(y.x + p.x, y.y + p.y, y.z + p.z, y.w + p.w);
            }
            *reinterpret_cast<float4*>(ob + (int64_t)u * a.Cout + o) = y;
        }
    }
}

inline size_t ws_bytes(int32_t B, int32_t Tin, int32_t D) {
    if (B <= 0 || Tin <= 0 || D <= 0) return 256;
    return wx::align_up((size_t)B * (size_t)Tin * (size_t)D * sizeof(float), 256);
}

template <int S, int CH>
void launch(const ConvArgs& a, int32_t B, hipStream_t st) {
    const unsigned tiles = (unsigned)((a.Tout + kRows - 1) / kRows);
    if (a.Cout % 128 == 0)
        hipLaunchKernelGGL((stem_conv_kernel<S, CH, 2>), dim3(tiles, (unsigned)(a.Cout / 128), (unsigned)B), dim3(256), 0,
                           st, a);
    else
        hipLaunchKernelGGL((stem_conv_kernel<S, CH, 1>), dim3(tiles, (unsigned)(a.Cout / 64), (unsigned)B), dim3(256), 0,
                           st, a);
}

}  // namespace wxw

extern "C" size_t wx_whisper_stem_workspace_bytes(int32_t B, int32_t Tin, int32_t D) { return wxw::ws_bytes(B, Tin, D); }

extern "C" int wx_whisper_stem(const float* x, int64_t x_batch_stride, int64_t x_row_stride, int32_t B, int32_t n_mels,
                               int32_t Tin, const float* w1_packed, const float* b1, const float* w2_packed,
                               const float* b2, const float* pos, int32_t D, float* out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    using namespace wxw;
    if (B < 0 || Tin < 2 || (Tin & 1) || Tin > (1 << 24) || (n_mels != 80 && n_mels != 128)) return WX_E_INVALID;
    if (D < 64 || D % 64 || D > 1280) return WX_E_INVALID;
    if (B == 0) return WX_OK;
    if (B > 65535 || x_row_stride < Tin || x_batch_stride < 0) return WX_E_INVALID;
    if (!x || !w1_packed || !b1 || !w2_packed || !b2 || !pos || !out || !workspace) return WX_E_INVALID;
    if (reinterpret_cast<uintptr_t>(x) & 3) return WX_E_INVALID;
    for (const void* p : {(const void*)w1_packed, (const void*)b1, (const void*)w2_packed, (const void*)b2,
                          (const void*)pos, (const void*)out, (const void*)workspace})
        if (reinterpret_cast<uintptr_t>(p) & 15) return WX_E_INVALID;
    if (workspace_bytes < ws_bytes(B, Tin, D)) return WX_E_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* a1 = reinterpret_cast<float*>(workspace);
    ConvArgs c1;
    c1.in = x;
    c1.in_bs = x_batch_stride;
    c1.in_rs = x_row_stride;
    c1.w = reinterpret_cast<const float4*>(w1_packed);
    c1.bias = b1;
    c1.pos = nullptr;
    c1.out = a1;
    c1.Tin = Tin;
    c1.Tout = Tin;
    c1.Cin = n_mels;
    c1.Cout = D;
    if (n_mels == 80)
        launch<1, 80>(c1, B, st);
    else
        launch<1, 128>(c1, B, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    ConvArgs c2;
    c2.in = a1;
    c2.in_bs = (int64_t)Tin * D;
    c2.in_rs = D;
    c2.w = reinterpret_cast<const float4*>(w2_packed);
    c2.bias = b2;
    c2.pos = pos;
    c2.out = out;
    c2.Tin = Tin;
    c2.Tout = Tin / 2;
    c2.Cin = D;
    c2.Cout = D;
    launch<2, 64>(c2, B, st);
    return wx::launch_status();
}
