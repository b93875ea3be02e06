// wx_prefill.hip — attention of a prompt prefill of Whisper's text decoder (whisperx/asr.py:35-45:
// the reference prepends `initial_prompt` / `prefix` to every batch's prompt, up to ~223 ids, and
// hands them to CTranslate2 in one forward): Tq query rows per (batch, head) against Tk key / value
// rows read in place through their strides, under a causal mask (the self-attention cache, query i
// at position causal + i) or without one (the two halves of the cross-attention [B, P, 2D] GEMM
// output).  C ABI and semantics: include/wx_align.h (wx_prefill_attention_f32 / _h16).
//
// The kernel is attn_mfma32_unit (wx_attention_unit.h, which see for the operand layout, the mask
// rules and "nothing seen yet") with kSplit waves, one workgroup per (batch, head, 32-query tile):
// row (b, i, h) depends only on its query, on causal + i and on the K / V rows below that, not on
// B, Tq, Tk beyond it, or on how causal + i is split; K / V rows at and past min(Tk, causal + Tq)
// are never read.  The h16 entry is the f32 entry on the widened inputs, rounded, bit for bit (the
// decoder's half contract, wx_decode.hip).
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wx_attention_unit.h"

namespace wxpre {

constexpr int kSplit = 4;  // waves per 32-query tile, each over every kSplit-th 32-key tile

using wx::kF32, wx::kF16, wx::kBF16;  // (wx_half.h)

template <int ET>
__global__ __launch_bounds__(64 * kSplit) __attribute__((amdgpu_waves_per_eu(2))) void prefill_attn_kernel(wx::AttnArgs a) {
    typedef typename std::conditional<ET == kF32, float, short>::type elem;
    int b, h, tile;
    wx::dense_unit(wx::xcd_unit(), (a.Tq + 31) / 32, a.H, b, h, tile);
    wx::attn_mfma32_unit<ET, kSplit>(static_cast<const elem*>(a.q) + b * a.qs[0] + h * a.qs[1],
                                     static_cast<const elem*>(a.k) + b * a.ks[0] + h * a.ks[1],
                                     static_cast<const elem*>(a.v) + b * a.vs[0] + h * a.vs[1],
                                     static_cast<elem*>(a.o) + ((int64_t)b * a.Tq * a.H + h) * 64, a.Tq, a.Tk, a.causal,
                                     tile, a.qs[2], a.ks[2], a.vs[2], (int64_t)a.H * 64, a.scale_log2);
}

// Both entry points, in the header's order; `mult`: elements per 16 bytes.
template <int ET>
inline int prefill(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H, int32_t Tq, int32_t Tk,
                   int32_t causal, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                   const int64_t* v_strides, float scale, int mult, void* stream) {
    if (B < 0 || H < 1 || Tq < 1 || Tk < 1 || D != 64) return WX_E_INVALID;
    if (B == 0) return WX_OK;
    const int64_t blocks = ((int64_t)Tq + 31) / 32 * B * H;
    wx::AttnArgs a{};
    if (!wx::attn_args(&a, q, k, v, o, q_strides, k_strides, v_strides, 3, mult, true, blocks, scale)) return WX_E_INVALID;
    a.H = H;
    a.Tq = Tq;
    a.Tk = Tk;
    a.causal = causal < 0 ? -1 : causal;
    hipLaunchKernelGGL(prefill_attn_kernel<ET>, dim3((unsigned)blocks), dim3(64 * kSplit), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    return wx::launch_status();
}

}  // namespace wxpre

extern "C" int wx_prefill_attention_f32(const float* q, const float* k, const float* v, float* o, int32_t B, int32_t H,
                                        int32_t Tq, int32_t Tk, int32_t causal, int32_t D, const int64_t* q_strides,
                                        const int64_t* k_strides, const int64_t* v_strides, float scale,
                                        void* stream) {
    return wxpre::prefill<wx::kF32>(q, k, v, o, B, H, Tq, Tk, causal, D, q_strides, k_strides, v_strides, scale, 4, stream);
}

extern "C" int wx_prefill_attention_h16(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H,
                                        int32_t Tq, int32_t Tk, int32_t causal, int32_t D, const int64_t* q_strides,
                                        const int64_t* k_strides, const int64_t* v_strides, float scale, int32_t dtype,
                                        void* stream) {
    if (dtype == WX_DTYPE_BF16)
        return wxpre::prefill<wx::kBF16>(q, k, v, o, B, H, Tq, Tk, causal, D, q_strides, k_strides, v_strides, scale, 8, stream);
    if (dtype == WX_DTYPE_F16)
        return wxpre::prefill<wx::kF16>(q, k, v, o, B, H, Tq, Tk, causal, D, q_strides, k_strides, v_strides, scale, 8, stream);
    return WX_E_INVALID;
}
