// wx_mel.hip — Whisper's input features (whisperx/audio.py:140-159 log_mel_spectrogram), batched
// over chunks of one waveform in one fused launch.  C ABI and semantics: include/wx_align.h
// (wx_log_mel).
//
// The 400-point windowed real DFT of a frame is a row of a [frames x 400] . [400 x 416] fp32 GEMM
// (the Hann window folded into the basis): 13 tiles of 16 bins (201 used), each with a cosine and
// a sine tile.  The product is computed transposed, D[bin][frame] = basis^T . frames^T, on
// v_mfma_f32_16x16x4_f32: the accumulator then holds 4 consecutive bins of one frame per lane,
// power = re^2 + im^2 is lane-local, and the power tile is at once the B operand (k = bin,
// column = frame) of the mel projection mel[m][frame] = filt[m][bin] . P[bin][frame] — no lane
// movement, and neither the complex STFT nor the power spectrum leaves the registers.
//
// Mapping: one block of 4 waves per (chunk, 64 frames).
//   - The block stages the 63 * 160 + 400 samples its frames cover in LDS once, reflect extension
//     (torch.stft center=True) and right zero padding resolved per sample; frames are read from
//     there as overlapping rows (row stride 160).  A skew of 4 floats per 32 samples spreads the 16
//     rows of a ds_read_b128 over the banks (row stride 160 alone maps them to two).
//   - Wave w owns bin tiles w, w + 4, w + 8 (and 12 for w = 0) for all 4 frame tiles: each basis
//     fragment is loaded once per block (coalesced 16-byte loads of the host-packed basis, from
//     L2) and used against 4 frame fragments; a k-group of 16 taps is 8 basis loads, 4 LDS reads
//     and 128 MFMAs in wave 0.
//   - Each wave multiplies its bins' power into a partial [n_mels x 64] mel tile (in passes of
//     4 or 5 16-row mel tiles, the power tiles staying in registers); the four
//     partials are added through LDS in wave order (a fixed order: results do not depend on
//     scheduling), then log10(max(., 1e-10)) is written and the block's maximum goes to the
//     chunk's slot of the workspace as an order-preserving integer key (atomicMax: exact and
//     order-independent).
//   - A block none of whose samples comes from the audio (all in the zero padding) skips both
//     GEMMs and feeds zeros to the same epilogue: identical values (a zero frame has power 0).
// A second launch applies max(., chunk_max - 8) and (. + 4) / 4 in place.
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "wx_host.h"  // (and through it include/wx_align.h)

namespace wxm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kNfft = 400, kHop = 160, kBins = 201;
constexpr int kFrames = 64;                          // frames per block
constexpr int kSpan = (kFrames - 1) * kHop + kNfft;  // samples a block stages
constexpr int kBinTiles = 13;                        // 16-bin tiles (208 >= 201)
constexpr int kGroups = kNfft / 16;                  // k-groups of 16 taps
constexpr int kRedStride = kFrames + 1;

__host__ __device__ constexpr int skew(int p) { return p + 4 * (p >> 5); }
constexpr int kLdsFloats = skew(kSpan - 1) + 4;
static_assert(kLdsFloats >= 128 * kRedStride, "the mel reduction reuses the sample buffer");
static_assert(16 * kBinTiles >= kBins && kBinTiles == 4 * 3 + 1, "wave 0 owns 4 bin tiles, waves 1..3 own 3");

struct MelArgs {
    const float* wave;
    int64_t n_wave;
    const int64_t* chunks;  // device [3][B]: first sample, length, right zero padding
    const float* filt;      // [n_mels][201]
    const float4* basis;    // [13][2][25][64] float4 (see wx_align.h)
    float* out;
    int64_t row_stride;
    uint32_t* cmax;  // [B] keys
    int32_t B, n_mels, n_frames_max, skip;
};

// order-preserving map float -> uint32 (no NaN in scope)
__device__ __forceinline__ uint32_t key_of(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ int64_t chunk_frames(const MelArgs& a, int b, int64_t& first, int64_t& len, int64_t& L) {
    first = a.chunks[b];
    len = a.chunks[a.B + b];
    L = len + a.chunks[2 * a.B + b];
    int64_t F = L / kHop;
    return F < a.n_frames_max ? F : a.n_frames_max;
}

// Registers: the DFT's 32 accumulators, two sets of basis fragments and the frame fragments, then
// the 16 power tiles and one pass of mel accumulators (5 mel tiles at 80 mels; 128 mels take two
// passes of 4: all 8 at once would spill) fit 221 VGPRs, so two blocks share a CU and one's
// staging, barriers and reduction hide under the other's MFMAs.
// (-DWX_MEL_OCC=1: one block per CU, the A/B variant for tools/mel_bench.py under WX_LIB_PATH.)
#ifndef WX_MEL_OCC
#define WX_MEL_OCC 2
#endif

template <int NMT, int MP>  // 16-row mel tiles: n_mels = 16 NMT, MP of them per projection pass
__global__ __launch_bounds__(256, WX_MEL_OCC) void log_mel_kernel(const MelArgs a) {
    static_assert(NMT % MP == 0, "whole passes");
    __shared__ __attribute__((aligned(16))) float xs[kLdsFloats];
    __shared__ int any_audio;
    const int b = blockIdx.y;
    const int f0 = blockIdx.x * kFrames;
    int64_t first, len, L;
    const int64_t F = chunk_frames(a, b, first, len, L);
    if (f0 >= F) return;
    const int tid = threadIdx.x;
    if (tid == 0) any_audio = 0;
    __syncthreads();

    // ---- stage: padded-signal positions i = 160 f0 - 200 + pp, pp < kSpan
    {
        const int64_t i0 = (int64_t)f0 * kHop - kNfft / 2;
        bool mine = false;
        for (int pp = tid; pp < kSpan; pp += 256) {
            const int64_t i = i0 + pp;
            int64_t j = i < 0 ? -i : i;
            if (j >= L) j = 2 * (L - 1) - j;  // right reflection (i < L + 200: j >= L - 201 >= 0)
            float v = 0.f;
            if (i < L + kNfft / 2 && j >= 0 && j < len && first + j < a.n_wave) {
                v = a.wave[first + j];
                mine = true;
            }
            xs[skew(pp)] = v;
        }
        if (mine) any_audio = 1;  // (benign race: every writer stores 1)
    }
    __syncthreads();
    const bool active = any_audio != 0 || a.skip == 0;  // block-uniform

    const int l = tid & 63, wv = tid >> 6, kq = l >> 4, r16 = l & 15;
    f32x4 pw[4][4];  // power of bin tile wv + 4 t, frame tile ft: bins 4 kq + v of frame r16 per lane
    const int nt = wv == 0 ? 4 : 3;  // bin tiles wv + 4 t, t < nt (wave-uniform)

    if (active) {
        f32x4 acc[4][2][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int cs = 0; cs < 2; ++cs)
#pragma unroll
                for (int ft = 0; ft < 4; ++ft) acc[t][cs][ft] = f32x4{0.f, 0.f, 0.f, 0.f};
        // basis fragment of (bin tile bt, cs, group g): basis[((bt * 2 + cs) * 25 + g) * 64 + l]
        const float4* bp = a.basis + (int64_t)wv * 2 * kGroups * 64 + l;
        constexpr int kTileStride = 4 * 2 * kGroups * 64;  // bin tile bt -> bt + 4
        const float* xrow = xs + kq * 4;
        int xoff[4];
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) xoff[ft] = kHop * (16 * ft + r16);
        float4 an[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int cs = 0; cs < 2; ++cs)
                an[t][cs] = t < nt ? bp[t * kTileStride + cs * kGroups * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int g = 0; g < kGroups; ++g) {
            float4 av[4][2];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int cs = 0; cs < 2; ++cs) av[t][cs] = an[t][cs];
            if (g + 1 < kGroups) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int cs = 0; cs < 2; ++cs)
                        if (t < nt) an[t][cs] = bp[t * kTileStride + (cs * kGroups + g + 1) * 64];
            }
            float4 xv[4];
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) {
                const int p = xoff[ft] + 16 * g;  // + 4 kq through xrow: same 32-sample skew block
                xv[ft] = *reinterpret_cast<const float4*>(xrow + skew(p));
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < nt) {
#pragma unroll
                    for (int cs = 0; cs < 2; ++cs)
#pragma unroll
                        for (int ft = 0; ft < 4; ++ft) {
                            f32x4 c = acc[t][cs][ft];
                            c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][cs].x, xv[ft].x, c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][cs].y, xv[ft].y, c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][cs].z, xv[ft].z, c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][cs].w, xv[ft].w, c, 0, 0, 0);
                            acc[t][cs][ft] = c;
                        }
                }
            }
        }
        // ---- power: re^2 + im^2, lane-local
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) {
                const f32x4 re = acc[t][0][ft], im = acc[t][1][ft];
                pw[t][ft] = re * re + im * im;
            }
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) pw[t][ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();  // every wave is done with the samples: xs becomes red[n_mels][kRedStride]

    // ---- the mel projection of the wave's own bins, MP mel tiles per pass (the accumulators of
    // a pass and the power tiles fit the two-blocks-per-CU register budget), and the four waves'
    // partial tiles added through LDS in wave order
#pragma unroll
    for (int ps = 0; ps < NMT / MP; ++ps) {
        f32x4 macc[MP][4];
#pragma unroll
        for (int i = 0; i < MP; ++i)
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) macc[i][ft] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (active) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < nt) {
                    const int bin0 = 16 * (wv + 4 * t) + 4 * kq;
#pragma unroll
                    for (int i = 0; i < MP; ++i) {
                        const float* frow = a.filt + (int64_t)(16 * (ps * MP + i) + r16) * kBins;
                        float fv[4];
#pragma unroll
                        for (int v = 0; v < 4; ++v) fv[v] = bin0 + v < kBins ? frow[bin0 + v] : 0.f;
#pragma unroll
                        for (int ft = 0; ft < 4; ++ft) {
                            f32x4 c = macc[i][ft];
                            c = __builtin_amdgcn_mfma_f32_16x16x4f32(fv[0], pw[t][ft][0], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_16x16x4f32(fv[1], pw[t][ft][1], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_16x16x4f32(fv[2], pw[t][ft][2], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_16x16x4f32(fv[3], pw[t][ft][3], c, 0, 0, 0);
                            macc[i][ft] = c;
                        }
                    }
                }
            }
        }
        for (int w = 0; w < 4; ++w) {
            if (wv == w) {
#pragma unroll
                for (int i = 0; i < MP; ++i)
#pragma unroll
                    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            float* r = xs + (16 * (ps * MP + i) + 4 * kq + v) * kRedStride + 16 * ft + r16;
                            *r = w == 0 ? macc[i][ft][v] : *r + macc[i][ft][v];
                        }
            }
            __syncthreads();
        }
    }

    // ---- log10, write, maximum
    const int n_mels = 16 * NMT;
    float* ob = a.out + (int64_t)b * n_mels * a.row_stride;
    float mx = -__builtin_inff();
    for (int e = tid; e < n_mels * kFrames; e += 256) {
        const int m = e >> 6, fl = e & 63;
        const int64_t f = (int64_t)f0 + fl;
        if (f < F) {
            // (the clamp value itself maps to -10, its correctly rounded log10, whatever the
            // device log10f returns for it: silence is exactly -10, as on the host)
            const float c = fmaxf(xs[m * kRedStride + fl], 1e-10f);
            const float v = c == 1e-10f ? -10.0f : log10f(c);
            ob[(int64_t)m * a.row_stride + f] = v;
            mx = fmaxf(mx, v);
        }
    }
    for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
    if (l == 0) atomicMax(a.cmax + b, key_of(mx));  // (every wave has a valid element: f0 < F)
}

__global__ __launch_bounds__(256) void log_mel_finish_kernel(const MelArgs a) {
    const int b = blockIdx.z, m = blockIdx.y;
    int64_t first, len, L;
    const int64_t F = chunk_frames(a, b, first, len, L);
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const float floor_v = float_of(a.cmax[b]) - 8.0f;
    float* p = a.out + ((int64_t)b * a.n_mels + m) * a.row_stride + f;
    *p = (fmaxf(*p, floor_v) + 4.0f) / 4.0f;
}

inline size_t ws_bytes(int32_t B) { return ((size_t)(B > 0 ? B : 1) * sizeof(uint32_t) + 255) / 256 * 256; }

}  // namespace wxm

extern "C" size_t wx_log_mel_workspace_bytes(int32_t B) { return wxm::ws_bytes(B); }

extern "C" int wx_log_mel(const float* wave, int64_t n_wave, const int64_t* chunk_first, const int64_t* chunk_len,
                          const int64_t* chunk_pad, const int64_t* chunks_dev, int32_t B, int32_t n_mels,
                          const float* filters, const float* basis, float* out, int64_t n_frames_max,
                          int64_t row_stride, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace wxm;
    if (B < 0 || (n_mels != 80 && n_mels != 128)) return WX_E_INVALID;
    if (B == 0) return WX_OK;
    if (B > 65535 || n_wave < 0 || n_frames_max < 0 || n_frames_max > 0x7fffffff - kFrames || row_stride < n_frames_max)
        return WX_E_INVALID;
    if (!chunk_first || !chunk_len || !chunk_pad || !chunks_dev || !filters || !basis || !out || !workspace ||
        (!wave && n_wave > 0))
        return WX_E_INVALID;
    int64_t max_frames = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t first = chunk_first[b], len = chunk_len[b], pad = chunk_pad[b];
        if (first < 0 || len < 0 || pad < 0 || len > n_wave || first > n_wave - len) return WX_E_INVALID;
        if (len > 0x7fffffff || pad > 0x7fffffff) return WX_E_INVALID;
        const int64_t L = len + pad;
        if (L <= kNfft / 2) return WX_E_INVALID;  // torch's reflect padding needs L > 200
        if (L / kHop > n_frames_max) return WX_E_INVALID;
        if (L / kHop > max_frames) max_frames = L / kHop;
    }
    if (workspace_bytes < ws_bytes(B)) return WX_E_WORKSPACE;
    if (max_frames == 0) return WX_OK;  // (L < 160: the reference returns [n_mels, 0])
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)B * sizeof(uint32_t), st);
    if (e != hipSuccess) return (int)e;
    MelArgs a;
    a.wave = wave;
    a.n_wave = n_wave;
    a.chunks = chunks_dev;
    a.filt = filters;
    a.basis = reinterpret_cast<const float4*>(basis);
    a.out = out;
    a.row_stride = row_stride;
    a.cmax = reinterpret_cast<uint32_t*>(workspace);
    a.B = B;
    a.n_mels = n_mels;
    a.n_frames_max = (int32_t)n_frames_max;
    const char* ns = getenv("WX_NO_MEL_SKIP");
    a.skip = (ns && ns[0] && ns[0] != '0') ? 0 : 1;
    const dim3 grid((unsigned)((max_frames + kFrames - 1) / kFrames), (unsigned)B);
    if (n_mels == 80)
        hipLaunchKernelGGL((log_mel_kernel<5, 5>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((log_mel_kernel<8, 4>), grid, dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const dim3 fgrid((unsigned)((max_frames + 255) / 256), (unsigned)n_mels, (unsigned)B);
    hipLaunchKernelGGL(log_mel_finish_kernel, fgrid, dim3(256), 0, st, a);
    return wx::launch_status();
}
