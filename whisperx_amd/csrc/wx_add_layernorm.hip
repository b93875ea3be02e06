// wx_add_layernorm.hip — the gfx950 kernel of `layer_norm(residual + x)` and its three entry points:
// wx_add_layernorm (fp32: the wav2vec2 encoder layers of the emission forward and Whisper's fp32
// residual chains), wx_add_layernorm_h16 (between a fp32 residual stream and 16-bit GEMMs) and
// wx_add_layernorm_h16_dual (the norm in fp32 and in 16 bit from one pass).  One kernel body for the
// three; compiled with -ffp-contract=off, so that every instantiation evaluates the same expressions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wx_half.h"
#include "wx_host.h"  // (and through it include/wx_align.h)

namespace wxe {

// Residual add + LayerNorm over rows of D floats (the wav2vec2 encoder layer's
// `layer_norm(residual + x)`, twice per layer): one wave per row, the row in registers (D / 256
// float4 per lane), mean and biased variance in fp32 from the registers (two passes, not
// torch's Welford: equal to fp32 tolerance), y = (s - mean) * rstd * gamma + beta.  Optionally
// also writes the sum s (the pre-norm residual stream of the stable-layer-norm layers).
// D4 < 64 NV (Whisper-tiny's D = 384: 96 float4): the lanes past the row's end hold zeros and
// skip their loads and stores; the full-width instantiations compile as before.
// ET is the element type of b and y16:
//   wx::kF32          b fp32 and y32 are required (no null test is compiled), y16 is not touched;
//   wx::kF16 / kBF16  b is widened on the load (a null b: zeros, added like any other, so that the
//                     result is the fp32 form's on a zero b), y16 is y rounded to nearest even on the
//                     store, the sum stays fp32.
// Y32: the entry point has a y32 (fp32: always, and required).  For the 16-bit types it is y itself,
// written when the pointer is not null: a post-norm wav2vec2 layer needs norm(residual + x) in fp32 as
// the next residual and in 16 bit as the next GEMM operand.  wx_add_layernorm_h16 has none, which is a
// template parameter and not a null y32: through the null test it measured 0.3% over its own kernel of
// before at 17,988 x 1024, and with "y32 is not null" known to the compiler the dual form took 2 to 5
// more VGPRs.
// The expressions between the load of b and the stores do not depend on ET: y32 is bit for bit the
// fp32 form's y on float(b), y16 its rounding.
template <int ET, bool Y32, int NV, int D4 = 64 * NV>  // NV float4 per lane, D4 per row: D = 4 D4
__global__ __launch_bounds__(256) void add_ln_kernel(const float* __restrict__ a, const void* __restrict__ b,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float eps, int64_t rows, int64_t sa, int64_t sb, int64_t sy,
                                                      float* __restrict__ y32, unsigned short* __restrict__ y16,
                                                      float* __restrict__ sum_out) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int l = threadIdx.x & 63;
    constexpr int D = 4 * D4;
    constexpr bool kFull = D4 == 64 * NV, kHalf = ET != wx::kF32;
    static_assert(D4 <= 64 * NV && D4 > 64 * (NV - 1), "NV float4 per lane cover the row");
    static_assert(kHalf || Y32, "the fp32 form has no other output");
    const float4* pa = reinterpret_cast<const float4*>(a + row * sa);
    const float4* pb32 = nullptr;
    const ushort4* pb16 = nullptr;
    if constexpr (!kHalf) pb32 = reinterpret_cast<const float4*>(static_cast<const float*>(b) + row * sb);
    else if (b) pb16 = reinterpret_cast<const ushort4*>(static_cast<const unsigned short*>(b) + row * sb);
    float4 v[NV];
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!kFull && 64 * i + l >= D4) {
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float4 x = pa[64 * i + l];
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (!kHalf) {
            z = pb32[64 * i + l];
        } else if (pb16) {
            const ushort4 u = pb16[64 * i + l];
            z = make_float4(wx::widen16<ET>(u.x), wx::widen16<ET>(u.y), wx::widen16<ET>(u.z), wx::widen16<ET>(u.w));
        }
        v[i] = make_float4(x.x + z.x, x.y + z.y, x.z + z.z, x.w + z.w);
        acc += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    const float mean = acc / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!kFull && 64 * i + l >= D4) continue;
        const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
        q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q / (float)D + eps);
    float4* p32 = Y32 && (!kHalf || y32) ? reinterpret_cast<float4*>(y32 + row * sy) : nullptr;
    ushort4* p16 = kHalf ? reinterpret_cast<ushort4*>(y16 + row * sy) : nullptr;
    float4* ps = sum_out ? reinterpret_cast<float4*>(sum_out + row * sy) : nullptr;
    const float4* pg = reinterpret_cast<const float4*>(gamma);
    const float4* pt = reinterpret_cast<const float4*>(beta);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!kFull && 64 * i + l >= D4) continue;
        const float4 g = pg[64 * i + l], t = pt[64 * i + l];
        const float4 y = make_float4((v[i].x - mean) * rstd * g.x + t.x, (v[i].y - mean) * rstd * g.y + t.y,
                                     (v[i].z - mean) * rstd * g.z + t.z, (v[i].w - mean) * rstd * g.w + t.w);
        if (Y32 && (!kHalf || p32)) p32[64 * i + l] = y;
        if constexpr (kHalf)
            p16[64 * i + l] = make_ushort4(wx::round16<ET>(y.x), wx::round16<ET>(y.y), wx::round16<ET>(y.z), wx::round16<ET>(y.w));
        if (ps) ps[64 * i + l] = v[i];
    }
}

using AddLnKernel = decltype(&add_ln_kernel<wx::kF32, true, 1>);

template <int NV, int D4 = 64 * NV>
static AddLnKernel add_ln_of(int et, bool has_y32) {
    if (et == wx::kF32) return add_ln_kernel<wx::kF32, true, NV, D4>;
    if (et == wx::kF16) return has_y32 ? add_ln_kernel<wx::kF16, true, NV, D4> : add_ln_kernel<wx::kF16, false, NV, D4>;
    return has_y32 ? add_ln_kernel<wx::kBF16, true, NV, D4> : add_ln_kernel<wx::kBF16, false, NV, D4>;
}

// a wx_*_h16 entry point's dtype argument as an element type, or -1
static int half_et_of(int32_t dtype) { return dtype == WX_DTYPE_F16 || dtype == WX_DTYPE_BF16 ? dtype : -1; }

// The three entry points' validation and launch.  et is wx::kF32 (b and y32 required, rows of b at a
// multiple of 4 elements), a 16-bit type (y16 required, b and, where the entry has one, y32 optional,
// rows of b at a multiple of 8: 16-byte rows either way) or -1 for a dtype that is none.
static int add_ln_launch(int et, bool has_y32, const float* a, const void* b, int64_t rows, int32_t D, int64_t a_stride,
                         int64_t b_stride, const float* gamma, const float* beta, float eps, float* y32, void* y16,
                         float* sum_out, void* stream) {
    const bool half = et != wx::kF32;
    AddLnKernel kernel;
    switch (D) {
        case 256: kernel = add_ln_of<1>(et, has_y32); break;
        case 384: kernel = add_ln_of<2, 96>(et, has_y32); break;
        case 512: kernel = add_ln_of<2>(et, has_y32); break;
        case 768: kernel = add_ln_of<3>(et, has_y32); break;
        case 1024: kernel = add_ln_of<4>(et, has_y32); break;
        case 1280: kernel = add_ln_of<5>(et, has_y32); break;
        default: return WX_E_INVALID;
    }
    if (rows < 0 || et < 0) return WX_E_INVALID;
    if (rows == 0) return WX_OK;  // (an empty tensor may have no storage)
    if (!a || !gamma || !beta || (half ? !y16 : !b || !y32)) return WX_E_INVALID;
    if (a_stride < D || (a_stride & 3) || (b && (b_stride < D || (b_stride & (half ? 7 : 3))))) return WX_E_INVALID;
    for (const void* p : {(const void*)a, b, (const void*)gamma, (const void*)beta, (const void*)y32, (const void*)y16,
                          (const void*)sum_out})  // (the optional ones: when present)
        if (reinterpret_cast<uintptr_t>(p) & 15) return WX_E_INVALID;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a,
                       b, gamma, beta, eps, rows, a_stride, b_stride, (int64_t)D, y32, static_cast<unsigned short*>(y16),
                       sum_out);
    return wx::launch_status();
}

}  // namespace wxe

extern "C" int wx_add_layernorm(const float* a, const float* b, int64_t rows, int32_t D, int64_t a_stride,
                                int64_t b_stride, const float* gamma, const float* beta, float eps, float* y,
                                float* sum_out, void* stream) {
    return wxe::add_ln_launch(wx::kF32, true, a, b, rows, D, a_stride, b_stride, gamma, beta, eps, y, nullptr, sum_out, stream);
}

extern "C" int wx_add_layernorm_h16_dual(const float* a, const void* b, int64_t rows, int32_t D, int64_t a_stride,
                                         int64_t b_stride, const float* gamma, const float* beta, float eps,
                                         int32_t dtype, float* y32, void* y16, float* sum_out, void* stream) {
    return wxe::add_ln_launch(wxe::half_et_of(dtype), true, a, b, rows, D, a_stride, b_stride, gamma, beta, eps, y32, y16,
                              sum_out, stream);
}

extern "C" int wx_add_layernorm_h16(const float* a, const void* b, int64_t rows, int32_t D, int64_t a_stride,
                                    int64_t b_stride, const float* gamma, const float* beta, float eps, int32_t dtype,
                                    void* y, float* sum_out, void* stream) {
    return wxe::add_ln_launch(wxe::half_et_of(dtype), false, a, b, rows, D, a_stride, b_stride, gamma, beta, eps, nullptr,
                              y, sum_out, stream);
}
