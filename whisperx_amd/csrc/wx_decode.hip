// wx_decode.hip — attention of one decode step of Whisper's text decoder (whisperx/asr.py:53-62: the
// reference hands the encoder output to CTranslate2's generate; the arithmetic is transformers'
// WhisperDecoder.forward with its cache): every (batch, head) has ONE query row, which attends to L
// key / value rows read in place through their strides (the self-attention cache, or the two halves
// of the cross-attention [B, P, 2D] GEMM output).  fp32, and fp16 / bf16 (whisperx/asr.py:262: the
// reference loads its model with compute_type="float16", which covers the decoder's key / value
// caches and the cross-attention keys and values).  C ABI and semantics: include/wx_align.h
// (wx_decode_attention_f32, _f32_grouped, _h16, _h16_grouped, wx_decode_self_attention_f32, _h16).
//
// The work is a read of 2 L rows of 256 (16-bit: 128) bytes per (batch, head) and nothing else, so
// the key range is split over workgroups ("flash-decoding"):
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
// The arithmetic contract of the 16-bit forms: o is wx_decode_attention_f32 on the widened inputs,
// rounded to the type, bit for bit, and the fp32 kernels are the oracle of the 16-bit ones.  It holds
// by construction: the kernels are one template over the element type, a fp16 / bf16 element is
// widened to fp32 (exactly) where the fp32 kernel reads a float, and everything from there on is
// the same source: a lane holds 4 head dims and forms (q.x k.x + q.y k.y) + (q.z k.z + q.w k.w), the
// 16-lane DPP butterfly, the group's maximum, expf, l and acc, the merge of the 16 groups in group
// order, the chunks in chunk order, one fp32 division.  The only other operation is the rounding to
// nearest even of acc / l on the store.  The contract rules out packed 16-bit math, dot
// instructions and fused multiply-adds; it also fixes the lane <-> dim mapping, so a lane of the
// 16-bit kernels loads 8 bytes per row (a 16-lane group one 128-byte row, a wave 4 rows) and holds
// its 2 x 8 rows in 32 registers, half of the fp32 kernel's.  The partials in the workspace are
// fp32 for every element type, so the workspace is one.
//
// Built with -ffp-contract=off -fno-fast-math (whisperx_amd/_lib.py BASE_FLAGS).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "wx_half.h"
#include "wx_host.h"  // (and through it include/wx_align.h)

namespace wxdec {

using wx::kF32, wx::kF16, wx::kBF16;

typedef short s16x4 __attribute__((ext_vector_type(4)));
// ET's element in memory (16-bit patterns travel as shorts), and the 4 head dims of one row that a
// lane holds, as loaded
template <int ET>
using elem_t = typename std::conditional<ET == kF32, float, short>::type;
template <int ET>
using row_t = typename std::conditional<ET == kF32, float4, s16x4>::type;

constexpr int kHead = 64;                          // head dim
constexpr int kChunk = WX_DECODE_ATTENTION_CHUNK;  // keys per block
constexpr int kGroups = 16;                        // 16-lane groups per block (4 waves x 4)
constexpr int kPasses = kChunk / kGroups;          // rows per group
constexpr int kMaxGroup = WX_DECODE_ATTENTION_MAX_GROUP;
static_assert(kChunk % kGroups == 0, "a chunk is a whole number of passes");

struct DecArgs {
    const void *q, *k, *v;  // elem_t<ET>
    void* o;
    float2* ml;   // [B G H nc] (m, l) of every chunk
    float* acc;   // [B G H nc][64]
    int64_t qs[3], ks[3], vs[3];  // in elements; qs: {b, h} (ungrouped), {b, g, h} (grouped)
    int32_t H, L, nc;
    float scale;
    int32_t G;  // queries per (batch, head): 1 (ungrouped)
};

template <int ET>
__device__ __forceinline__ float4 widen4(row_t<ET> x) {
    if constexpr (ET == kF32) return x;
    else return make_float4(wx::widen16<ET>(x[0]), wx::widen16<ET>(x[1]), wx::widen16<ET>(x[2]), wx::widen16<ET>(x[3]));
}
template <int ET>
__device__ __forceinline__ elem_t<ET> narrow(float x) {  // o's element: x, or its rounding to nearest even
    if constexpr (ET == kF32) return x;
    else return wx::round16<ET>(x);
}

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

// Row j0 of (batch b, head h) of k or v by its strides s, at the lane's first head dim d4
template <int ET>
__device__ __forceinline__ const elem_t<ET>* rows_at(const void* p, const int64_t (&s)[3], int b, int h, int j0,
                                                     int d4) {
    return static_cast<const elem_t<ET>*>(p) + (int64_t)b * s[0] + (int64_t)h * s[1] + (int64_t)j0 * s[2] + d4;
}

// The chunk's rows of one lane: pass i of group grp is row 16 i + grp, 4 elements of it.  Rows at
// and past n issue no load and hold zeros.
template <int ET>
__device__ __forceinline__ void load_rows(const elem_t<ET>* base, int64_t row_stride, int grp, int n,
                                          row_t<ET> (&r)[kPasses]) {
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        const int row = kGroups * i + grp;
        if constexpr (ET == kF32) r[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        else r[i] = s16x4{0, 0, 0, 0};
        if (row < n) r[i] = *reinterpret_cast<const row_t<ET>*>(base + (int64_t)row * row_stride);
    }
}

// The per-query arithmetic on the rows a lane holds: the group's (m, l, acc)
template <int ET>
__device__ __forceinline__ void group_partial(const float4 qv, const row_t<ET> (&kr)[kPasses],
                                              const row_t<ET> (&vr)[kPasses], int grp, int n, float scale, float& m,
                                              float& l, float4& acc) {
    float s[kPasses];
    m = -INFINITY;
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        const float4 kf = widen4<ET>(kr[i]);
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
            const float4 vf = widen4<ET>(vr[i]);
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

// A block's rows to its result, for the kernels of one query per (batch, head): the 16 groups'
// partials of the n rows in kr / vr, merged through LDS in group order by wave 0, which writes
// o = acc / l when the keys are one chunk (nc == 1) and the chunk's slot of the workspace otherwise.
template <int ET>
__device__ __forceinline__ void chunk_result(const DecArgs& a, const row_t<ET> qr, const row_t<ET> (&kr)[kPasses],
                                             const row_t<ET> (&vr)[kPasses], int b, int h, int c, int n, int nc) {
    __shared__ float s_m[kGroups], s_l[kGroups];
    __shared__ __attribute__((aligned(16))) float s_acc[kGroups][kHead];
    const int tid = threadIdx.x;
    const int grp = tid >> 4, d4 = (tid & 15) * 4;
    float m, l;
    float4 acc;
    group_partial<ET>(widen4<ET>(qr), kr, vr, grp, n, a.scale, m, l, acc);
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
    if (nc == 1) {
        static_cast<elem_t<ET>*>(a.o)[bh * kHead + tid] = narrow<ET>(out / Lsum);
        return;
    }
    const int64_t slot = bh * nc + c;
    if (tid == 0) a.ml[slot] = make_float2(M, Lsum);
    a.acc[slot * kHead + tid] = out;
}

// Row (b, h) of q (or of the step's new key / value rows) by its strides {b, h}, the lane's 4 dims
template <int ET>
__device__ __forceinline__ row_t<ET> row_of(const void* p, const int64_t* s, int b, int h, int d4) {
    return *reinterpret_cast<const row_t<ET>*>(static_cast<const elem_t<ET>*>(p) + (int64_t)b * s[0] + (int64_t)h * s[1] +
                                               d4);
}

template <int ET>
__global__ __launch_bounds__(256) void decode_chunk_kernel(const DecArgs a) {
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int grp = threadIdx.x >> 4, d4 = (threadIdx.x & 15) * 4;
    const int j0 = c * kChunk;            // (< L <= 2^31 - 1)
    const int n = min(kChunk, a.L - j0);  // rows of this chunk, >= 1

    const row_t<ET> qr = row_of<ET>(a.q, a.qs, b, h, d4);
    row_t<ET> kr[kPasses], vr[kPasses];
    load_rows<ET>(rows_at<ET>(a.k, a.ks, b, h, j0, d4), a.ks[2], grp, n, kr);
    load_rows<ET>(rows_at<ET>(a.v, a.vs, b, h, j0, d4), a.vs[2], grp, n, vr);
    chunk_result<ET>(a, qr, kr, vr, b, h, c, n, a.nc);
}

// one (batch, head) of a wave, lane d = dim: its nc chunks in chunk order
template <int ET>
__device__ __forceinline__ void merge_chunks(const DecArgs& a, int64_t bh, int nc, int d) {
    const float2* ml = a.ml + bh * nc;
    const float* acc = a.acc + bh * nc * kHead;
    float M = -INFINITY;
    for (int c = 0; c < nc; ++c) M = fmaxf(M, ml[c].x);
    float Lsum = 0.f, out = 0.f;
    for (int c = 0; c < nc; ++c) {
        const float2 p = ml[c];
        const float w = expf(p.x - M);
        Lsum += w * p.y;
        out += w * acc[(int64_t)c * kHead + d];
    }
    static_cast<elem_t<ET>*>(a.o)[bh * kHead + d] = narrow<ET>(out / Lsum);
}

// one wave per (batch, head), lane = dim: the chunks in chunk order
template <int ET>
__global__ __launch_bounds__(256) void decode_merge_kernel(const DecArgs a, int64_t BH) {
    const int64_t bh = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bh >= BH) return;
    merge_chunks<ET>(a, bh, a.nc, threadIdx.x & 63);
}

// ------------------------------------------------------------------------------ self
// The self-attention of one decode step at a position that lives in device memory
// (wx_decode_self_attention_f32 / _h16): p = *pos is read by the kernels, so that the launch is the
// same at every step and a captured graph can replay it.  The grid covers the cache's Lcap rows; a
// block whose first row lies above p returns at once, the others are decode_chunk_kernel's blocks at
// L = p + 1 (same load_rows, chunk_result and slots, nc = p / 128 + 1 computed here), except that
// row p comes from the step's new key / value rows, not from the cache: load_rows stops below it,
// the lanes of its group and pass take it from k_new / v_new and store it to the cache.  Only the
// block that owns row p touches it, so there is no hand-shake.  The merge kernel reads p the same
// way and returns when one chunk block has written o itself.  p outside [0, Lcap): every block of
// both kernels returns before it reads or writes anything else.
struct SelfArgs {
    DecArgs d;  // k / v: the caches (written at row p); L: Lcap; nc: chunks(Lcap), the grid's x
    const void *kn, *vn;  // elem_t<ET>: the new rows, by {b, h} strides
    int64_t kns[2], vns[2];
    const int32_t* pos;
};

template <int ET>
__global__ __launch_bounds__(256) void decode_self_chunk_kernel(const SelfArgs s) {
    typedef elem_t<ET> elem;
    const DecArgs& a = s.d;
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int grp = threadIdx.x >> 4, d4 = (threadIdx.x & 15) * 4;
    const int p = *s.pos;
    const int j0 = c * kChunk;  // (< Lcap)
    if (p < 0 || p >= a.L || j0 > p) return;
    const int n = min(kChunk, p + 1 - j0);       // rows of this chunk at L = p + 1, >= 1
    const int fresh = p - j0 < kChunk ? p - j0 : -1;  // row p's place in this chunk (then n - 1), or none
    const int cached = fresh < 0 ? n : fresh;    // the rows the cache holds

    const row_t<ET> qr = row_of<ET>(a.q, a.qs, b, h, d4);
    const elem* kb = rows_at<ET>(a.k, a.ks, b, h, j0, d4);
    const elem* vb = rows_at<ET>(a.v, a.vs, b, h, j0, d4);
    row_t<ET> kr[kPasses], vr[kPasses];
    load_rows<ET>(kb, a.ks[2], grp, cached, kr);
    load_rows<ET>(vb, a.vs[2], grp, cached, vr);
    if (fresh >= 0 && (fresh & (kGroups - 1)) == grp) {  // the 16 lanes that hold row p
        const row_t<ET> kn = row_of<ET>(s.kn, s.kns, b, h, d4), vn = row_of<ET>(s.vn, s.vns, b, h, d4);
#pragma unroll
        for (int i = 0; i < kPasses; ++i)
            if (i == fresh / kGroups) {
                kr[i] = kn;
                vr[i] = vn;
            }
        *reinterpret_cast<row_t<ET>*>(const_cast<elem*>(kb) + (int64_t)fresh * a.ks[2]) = kn;
        *reinterpret_cast<row_t<ET>*>(const_cast<elem*>(vb) + (int64_t)fresh * a.vs[2]) = vn;
    }
    chunk_result<ET>(a, qr, kr, vr, b, h, c, n, p / kChunk + 1);
}

template <int ET>
__global__ __launch_bounds__(256) void decode_self_merge_kernel(const SelfArgs s, int64_t BH) {
    const int64_t bh = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int p = *s.pos;
    if (bh >= BH || p < kChunk || p >= s.d.L) return;  // (p < 128: one chunk, whose block wrote o)
    merge_chunks<ET>(s.d, bh, p / kChunk + 1, threadIdx.x & 63);
}

// ------------------------------------------------------------------------------ grouped
// The G queries of one batch entry (the beams of one audio chunk) share its keys and values: the
// block loads its 2 x 128 rows once, as above, and then runs group_partial G times on the rows it
// holds, so that row (b, g, h) has the bits the ungrouped kernel gives that query.  The G queries
// wait in LDS as fp32, widened once (one load per lane of the first G 16-lane groups, issued behind
// the key / value loads); the 16 groups' partials of every query go to LDS (G x 4.1 KB, sized by the
// launch) and wave w merges the queries w, w + 4, ... in group order.  The workspace slots are
// those of B G H ungrouped rows, and decode_merge_kernel merges the chunks.
template <int ET>
__global__ __launch_bounds__(256) void decode_chunk_grouped_kernel(const DecArgs a) {
    typedef elem_t<ET> elem;
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

    const elem* kb = rows_at<ET>(a.k, a.ks, b, h, j0, d4);
    const elem* vb = rows_at<ET>(a.v, a.vs, b, h, j0, d4);
    row_t<ET> kr[kPasses], vr[kPasses];
    load_rows<ET>(kb, a.ks[2], grp, n, kr);
    load_rows<ET>(vb, a.vs[2], grp, n, vr);
    if (grp < G)  // query grp of this (batch, head)
        *reinterpret_cast<float4*>(s_q + grp * kHead + d4) = widen4<ET>(*reinterpret_cast<const row_t<ET>*>(
            static_cast<const elem*>(a.q) + (int64_t)b * a.qs[0] + (int64_t)grp * a.qs[1] + (int64_t)h * a.qs[2] + d4));
    __syncthreads();

    for (int g = 0; g < G; ++g) {
        float m, l;
        float4 acc;
        group_partial<ET>(*reinterpret_cast<const float4*>(s_q + g * kHead + d4), kr, vr, grp, n, a.scale, m, l, acc);
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
        float M, Lsum, out;
        merge_groups(s_m + g * kGroups, s_l + g * kGroups, s_acc + g * kGroups * kHead, d, M, Lsum, out);
        const int64_t bgh = ((int64_t)b * G + g) * a.H + h;
        if (a.nc == 1) {
            static_cast<elem*>(a.o)[bgh * kHead + d] = narrow<ET>(out / Lsum);
        } else {
            const int64_t slot = bgh * a.nc + c;
            if (d == 0) a.ml[slot] = make_float2(M, Lsum);
            a.acc[slot * kHead + d] = out;
        }
    }
}

inline int64_t chunks(int32_t L) { return ((int64_t)L + kChunk - 1) / kChunk; }

// The workspace's layout for B (grouped: B G) query rows per head, stated once: measures on a null
// base, fills `a` on the caller's pointer.
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

template <int ET>
void launch(const DecArgs& a, int32_t B, bool grouped, hipStream_t st) {
    const dim3 grid((unsigned)a.nc, (unsigned)a.H, (unsigned)B);
    if (grouped) {
        const size_t lds = (size_t)a.G * (kHead + kGroups * kHead + 2 * kGroups) * sizeof(float);  // (<= 35 KB)
        hipLaunchKernelGGL(decode_chunk_grouped_kernel<ET>, grid, dim3(256), lds, st, a);
    } else {
        hipLaunchKernelGGL(decode_chunk_kernel<ET>, grid, dim3(256), 0, st, a);
    }
    if (a.nc > 1) {
        const int64_t BH = (int64_t)B * a.G * a.H;  // (<= 8 x 65535^2: the merge grid's x fits)
        hipLaunchKernelGGL(decode_merge_kernel<ET>, dim3((unsigned)((BH + 3) / 4)), dim3(256), 0, st, a, BH);
    }
}

// The four entry points: the checks in the header's order, then the launches.  et: kF32, or the
// h16 entry points' dtype argument as it came; grouped: q has the strides {b, g, h} and the grouped
// kernel runs (the ungrouped entry points pass G = 1).
inline int run(int32_t et, bool grouped, const void* q, const void* k, const void* v, void* o, int32_t B, int32_t G,
               int32_t H, int32_t L, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
               const int64_t* v_strides, float scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 0 || G < 1 || G > kMaxGroup || H < 1 || L < 1 || D != kHead || (et != kF32 && et != kF16 && et != kBF16))
        return WX_E_INVALID;
    if (B == 0) return WX_OK;
    if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides || !workspace) return WX_E_INVALID;
    for (const void* p : {q, k, v, (const void*)o, (const void*)workspace})
        if (reinterpret_cast<uintptr_t>(p) & 15) return WX_E_INVALID;
    // 16-byte aligned rows: every stride a multiple of 4 floats / 8 16-bit elements
    const int nq = grouped ? 3 : 2, mult = et == kF32 ? 4 : 8;
    for (int i = 0; i < nq; ++i)
        if (q_strides[i] % mult) return WX_E_INVALID;
    for (int i = 0; i < 3; ++i)
        if (k_strides[i] % mult || v_strides[i] % mult) return WX_E_INVALID;
    if (B > 65535 || H > 65535) return WX_E_INVALID;  // grid y / z
    if ((int64_t)B * G * H * chunks(L) > ((int64_t)1 << 40)) return WX_E_INVALID;  // (the workspace size: in range)
    DecArgs a;
    if (workspace_bytes < carve(workspace, B * G, H, L, &a)) return WX_E_WORKSPACE;
    a.q = q;
    a.k = k;
    a.v = v;
    a.o = o;
    a.qs[2] = 0;
    for (int i = 0; i < nq; ++i) a.qs[i] = q_strides[i];
    for (int i = 0; i < 3; ++i) {
        a.ks[i] = k_strides[i];
        a.vs[i] = v_strides[i];
    }
    a.H = H;
    a.L = L;
    a.nc = (int32_t)chunks(L);
    a.G = G;
    a.scale = scale;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (et == kF32) launch<kF32>(a, B, grouped, st);
    else if (et == kF16) launch<kF16>(a, B, grouped, st);
    else launch<kBF16>(a, B, grouped, st);
    return wx::launch_status();
}

template <int ET>
void launch_self(const SelfArgs& s, int32_t B, hipStream_t st) {
    const DecArgs& a = s.d;
    hipLaunchKernelGGL(decode_self_chunk_kernel<ET>, dim3((unsigned)a.nc, (unsigned)a.H, (unsigned)B), dim3(256), 0, st, s);
    if (a.nc > 1) {
        const int64_t BH = (int64_t)B * a.H;
        hipLaunchKernelGGL(decode_self_merge_kernel<ET>, dim3((unsigned)((BH + 3) / 4)), dim3(256), 0, st, s, BH);
    }
}

// The two self-attention entry points: the checks in the header's order, then the launches, which
// depend on Lcap only.  Nothing here reads *pos, allocates or synchronises.
inline int run_self(int32_t et, const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                    void* o, int32_t B, int32_t H, int32_t Lcap, int32_t D, const int64_t* q_strides,
                    const int64_t* kn_strides, const int64_t* vn_strides, const int64_t* k_strides,
                    const int64_t* v_strides, float scale, const int32_t* pos, void* workspace, size_t workspace_bytes,
                    void* stream) {
    if (B < 0 || H < 1 || Lcap < 1 || D != kHead || (et != kF32 && et != kF16 && et != kBF16)) return WX_E_INVALID;
    if (B == 0) return WX_OK;
    if (!q || !k_new || !v_new || !k_cache || !v_cache || !o || !pos || !q_strides || !kn_strides || !vn_strides ||
        !k_strides || !v_strides || !workspace)
        return WX_E_INVALID;
    for (const void* p : {q, k_new, v_new, (const void*)k_cache, (const void*)v_cache, (const void*)o,
                          (const void*)workspace})
        if (reinterpret_cast<uintptr_t>(p) & 15) return WX_E_INVALID;
    if (reinterpret_cast<uintptr_t>(pos) & 3) return WX_E_INVALID;
    const int mult = et == kF32 ? 4 : 8;
    for (int i = 0; i < 2; ++i)
        if (q_strides[i] % mult || kn_strides[i] % mult || vn_strides[i] % mult) return WX_E_INVALID;
    for (int i = 0; i < 3; ++i)
        if (k_strides[i] % mult || v_strides[i] % mult) return WX_E_INVALID;
    if (B > 65535 || H > 65535) return WX_E_INVALID;  // grid y / z
    if ((int64_t)B * H * chunks(Lcap) > ((int64_t)1 << 40)) return WX_E_INVALID;
    SelfArgs s;
    DecArgs& a = s.d;
    if (workspace_bytes < carve(workspace, B, H, Lcap, &a)) return WX_E_WORKSPACE;
    a.q = q;
    a.k = k_cache;
    a.v = v_cache;
    a.o = o;
    s.kn = k_new;
    s.vn = v_new;
    s.pos = pos;
    a.qs[2] = 0;
    for (int i = 0; i < 2; ++i) {
        a.qs[i] = q_strides[i];
        s.kns[i] = kn_strides[i];
        s.vns[i] = vn_strides[i];
    }
    for (int i = 0; i < 3; ++i) {
        a.ks[i] = k_strides[i];
        a.vs[i] = v_strides[i];
    }
    a.H = H;
    a.L = Lcap;
    a.nc = (int32_t)chunks(Lcap);
    a.G = 1;
    a.scale = scale;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (et == kF32) launch_self<kF32>(s, B, st);
    else if (et == kF16) launch_self<kF16>(s, B, st);
    else launch_self<kBF16>(s, B, st);
    return wx::launch_status();
}

// a dtype argument that is no 16-bit type must not pass for kF32
inline int32_t et_of(int32_t dtype) { return dtype == WX_DTYPE_F16 || dtype == WX_DTYPE_BF16 ? dtype : -1; }

}  // namespace wxdec

extern "C" size_t wx_decode_attention_workspace_bytes(int32_t B, int32_t H, int32_t L) {
    return wxdec::carve(nullptr, B, H, L, nullptr);
}

extern "C" size_t wx_decode_attention_grouped_workspace_bytes(int32_t B, int32_t G, int32_t H, int32_t L) {
    const bool ok = B > 0 && G >= 1 && G <= wxdec::kMaxGroup && B <= 65535;
    return wxdec::carve(nullptr, ok ? B * G : 0, H, L, nullptr);
}

extern "C" int wx_decode_attention_f32(const float* q, const float* k, const float* v, float* o, int32_t B, int32_t H,
                                       int32_t L, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                                       const int64_t* v_strides, float scale, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return wxdec::run(wxdec::kF32, false, q, k, v, o, B, 1, H, L, D, q_strides, k_strides, v_strides, scale, workspace,
                      workspace_bytes, stream);
}

extern "C" int wx_decode_attention_f32_grouped(const float* q, const float* k, const float* v, float* o, int32_t B,
                                               int32_t G, int32_t H, int32_t L, int32_t D, const int64_t* q_strides,
                                               const int64_t* k_strides, const int64_t* v_strides, float scale,
                                               void* workspace, size_t workspace_bytes, void* stream) {
    return wxdec::run(wxdec::kF32, true, q, k, v, o, B, G, H, L, D, q_strides, k_strides, v_strides, scale, workspace,
                      workspace_bytes, stream);
}

extern "C" int wx_decode_attention_h16(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H,
                                       int32_t L, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                                       const int64_t* v_strides, float scale, int32_t dtype, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return wxdec::run(wxdec::et_of(dtype), false, q, k, v, o, B, 1, H, L, D, q_strides, k_strides, v_strides, scale,
                      workspace, workspace_bytes, stream);
}

extern "C" int wx_decode_attention_h16_grouped(const void* q, const void* k, const void* v, void* o, int32_t B,
                                               int32_t G, int32_t H, int32_t L, int32_t D, const int64_t* q_strides,
                                               const int64_t* k_strides, const int64_t* v_strides, float scale,
                                               int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    return wxdec::run(wxdec::et_of(dtype), true, q, k, v, o, B, G, H, L, D, q_strides, k_strides, v_strides, scale,
                      workspace, workspace_bytes, stream);
}

extern "C" int wx_decode_self_attention_f32(const float* q, const float* k_new, const float* v_new, float* k_cache,
                                            float* v_cache, float* o, int32_t B, int32_t H, int32_t Lcap, int32_t D,
                                            const int64_t* q_strides, const int64_t* k_new_strides,
                                            const int64_t* v_new_strides, const int64_t* k_strides,
                                            const int64_t* v_strides, float scale, const int32_t* pos, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    return wxdec::run_self(wxdec::kF32, q, k_new, v_new, k_cache, v_cache, o, B, H, Lcap, D, q_strides, k_new_strides,
                           v_new_strides, k_strides, v_strides, scale, pos, workspace, workspace_bytes, stream);
}

extern "C" int wx_decode_self_attention_h16(const void* q, const void* k_new, const void* v_new, void* k_cache,
                                            void* v_cache, void* o, int32_t B, int32_t H, int32_t Lcap, int32_t D,
                                            const int64_t* q_strides, const int64_t* k_new_strides,
                                            const int64_t* v_new_strides, const int64_t* k_strides,
                                            const int64_t* v_strides, float scale, int32_t dtype, const int32_t* pos,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    return wxdec::run_self(wxdec::et_of(dtype), q, k_new, v_new, k_cache, v_cache, o, B, H, Lcap, D, q_strides,
                           k_new_strides, v_new_strides, k_strides, v_strides, scale, pos, workspace, workspace_bytes,
                           stream);
}
