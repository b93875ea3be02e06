// wx_dp_prims.h — device primitives every phase of the alignment DP (wx_align_dp.h) uses: the
// reference's numerics, DPP and column 0's fp64 chain, segment descriptors, LDS-DMA staging and the
// column map, fences, the write-through stores / loads and hand-off granules of split segments.
#ifndef WX_DP_PRIMS_H
#define WX_DP_PRIMS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wx_dp_config.h"  // kChunk, kGatherVS
#include "wx_wave.h"       // kWave, lane_id, uniform*, readlane64

namespace wx {

template <bool B>
struct BoolTag {
    static constexpr bool value = B;
};

__device__ __forceinline__ float nan_max(float a, float b) {
    // IEEE-754-2019 maximum (NaN-propagating): torch.maximum for non-zero-sign cases.
    return __builtin_elementwise_maximum(a, b);
}

// w <- 2w + (c > s): strict compare (false when unordered), shifted into the lane's
// 32-step column word with an add-with-carry.
__device__ __forceinline__ unsigned shift_in(unsigned w, float c, float s) {
    unsigned r;
    asm("v_cmp_gt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %3, %3, vcc"
        : "=v"(r)
        : "v"(c), "v"(s), "v"(w)
        : "vcc");
    return r;
}

// Correctly rounded fp32 exp (the reference's torch-CPU exp is within 1 ULP of it).
__device__ __forceinline__ float exp_cr(float x) { return (float)exp((double)x); }

__device__ __forceinline__ float dpp_shr1(float old_lane0, float v) {
    // lane l <- v[l-1]; lane 0 keeps old_lane0 (bound_ctrl off).
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old_lane0), __builtin_bit_cast(int, v),
                                           0x138 /* wave_shr:1 */, 0xF, 0xF, false));
}

// Column 0's running sum over one 32-row chunk (alignment.py:366-370: torch's CPU cumsum
// accumulates em[:, 0] in double, row by row).  Lane j converts em[t0 + j, 0] (one instruction
// for the chunk), the doubles go through LDS and come back broadcast (16-byte reads, every lane
// the same address), and at step j the lanes r > j add row j: an EXEC-masked v_add_f64 with a
// scalar s_bitset0 retiring lane j + 1 after it.  Lane r (0..32) thus adds em[t0 + 0 .. r - 1, 0]
// in row order onto S(t0) and nothing else — the sequential chain's additions exactly.  (Round
// 5: two instructions per row instead of a conversion, a DPP shift and the add; config 2 50.8
// -> 47.5 us.)
// col0_run: the chain alone, on the chunk's 32 doubles already broadcast into registers (the
// register-resident forward's column-0 helper reads the next chunk's while it waits: col0_helper).
__device__ __forceinline__ double col0_run(double acc, const double (&dv)[kChunk]) {
    double a = acc;
    unsigned long long sv;
#define WX_C0_STEP(J, BIT) "v_add_f64 %[a], %[a], %[d" #J "]\n\ts_bitset0_b64 exec, " #BIT "\n\t"
#define WX_C0_BLOCK(B, J0, B1, B2, B3, B4, B5, B6, B7, B8)                                                      \
    asm volatile("s_mov_b64 %[sv], exec\n\t"                                                                  \
                 "s_mov_b32 exec_lo, %[mlo]\n\t"                                                              \
                 "s_mov_b32 exec_hi, 1\n\t" WX_C0_STEP(0, B1) WX_C0_STEP(1, B2) WX_C0_STEP(2, B3)              \
                     WX_C0_STEP(3, B4) WX_C0_STEP(4, B5) WX_C0_STEP(5, B6) WX_C0_STEP(6, B7)                   \
                         WX_C0_STEP(7, B8) "s_mov_b64 exec, %[sv]\n\t"                                        \
                 : [a] "+v"(a), [sv] "=&s"(sv)                                                                 \
                 : [mlo] "s"((unsigned)(0xFFFFFFFFu << ((J0) + 1))), [d0] "v"(dv[(J0)]),                      \
                   [d1] "v"(dv[(J0) + 1]), [d2] "v"(dv[(J0) + 2]), [d3] "v"(dv[(J0) + 3]),                     \
                   [d4] "v"(dv[(J0) + 4]), [d5] "v"(dv[(J0) + 5]), [d6] "v"(dv[(J0) + 6]),                     \
                   [d7] "v"(dv[(J0) + 7]))
    // block b: rows 8b .. 8b + 7, lanes 8b + 1 .. 32 active at its start (exec_hi = lane 32)
    WX_C0_BLOCK(0, 0, 1, 2, 3, 4, 5, 6, 7, 8);
    WX_C0_BLOCK(1, 8, 9, 10, 11, 12, 13, 14, 15, 16);
    WX_C0_BLOCK(2, 16, 17, 18, 19, 20, 21, 22, 23, 24);
    WX_C0_BLOCK(3, 24, 25, 26, 27, 28, 29, 30, 31, 32);
#undef WX_C0_BLOCK
#undef WX_C0_STEP
    return a;
}
__device__ __forceinline__ double col0_chain(double acc, float e) {
    const int l = lane_id();
    __shared__ __attribute__((aligned(16))) double c0d[kChunk];
    if (l < kChunk) c0d[l] = (double)e;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (other lanes' writes, read below)
    double dv[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) dv[j] = c0d[j];
    return col0_run(acc, dv);
}

// One chunk of column 0's running sum: lane l (0..31) holds e = em[t0 + l, 0] (lanes 32..63:
// any copy), acc = S(t0) (uniform).  Returns S(t0 + l) on lane l and advances acc to S(t0 + 32)
// (lane 32's sum, by v_readlane: no LDS round trip).
__device__ __forceinline__ double col0_chunk(double& acc, float e) {
    const double a = col0_chain(acc, e);
    acc = __builtin_bit_cast(double, readlane64(__builtin_bit_cast(unsigned long long, a), kChunk));
    return a;
}

struct SegDesc {
    int64_t row0;  // first emission row
    int T;
    int64_t tok0;
    int N;
    int blank;
};

__device__ __forceinline__ SegDesc load_desc(const int64_t* em_off, const int64_t* tok_off, const int32_t* blank_id,
                                             int seg) {
    SegDesc d;
    d.row0 = em_off[seg];
    d.T = uniform((int)(em_off[seg + 1] - d.row0));
    d.tok0 = tok_off[seg];
    d.N = uniform((int)(tok_off[seg + 1] - d.tok0));
    d.blank = uniform(blank_id[seg]);
    return d;
}

// LDS byte address of a __shared__ pointer (for M0).
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(uintptr_t)((const __attribute__((address_space(3))) char*)p);
}

// Wave-uniform 64-bit pointer (SGPR pair).
__device__ __forceinline__ const float* uniform_ptr(const float* p) {
    const uint64_t v = (uint64_t)(uintptr_t)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (const float*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

// LDS-DMA loads (global_load_lds), saddr form: wave-uniform base + 32-bit lane offset
// (inline-asm 64-bit VGPR operands are not guaranteed the even alignment gfx950 requires).
// Lane l's dword (or 16 bytes) lands at LDS m0 + 4*l (16*l).  Issued from inline asm so
// that hipcc's waitcnt pass does not see them (it would otherwise drain vmcnt before every
// ds_read, serialising the prefetch); callers wait vmcnt(0) themselves before reading.
__device__ __forceinline__ void glds_dword(const float* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(uniform_ptr(sbase)), "s"(lds_dst)
                 : "memory");
}
__device__ __forceinline__ void glds_dwordx4(const float* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(uniform_ptr(sbase)), "s"(lds_dst)
                 : "memory");
}

// Large vocabularies (V > 64, e.g. ja/zh character sets): the DP reads only column 0, the
// blank and the segment's own tokens, so a per-segment column map (built in LDS by
// build_colmap) lets the staging gather exactly those columns into a compact LDS row of
// VS = kGatherVS floats.  Token ids are remapped to their compact rank.
struct ColMap {
    const unsigned* bm;  // LDS: used-column bitmap
    const int* wpre;     // LDS: set bits in the words before each word
    const int* cols;     // LDS: compact index -> column
    int n;               // compact width (uniform)
    __device__ __forceinline__ int rank(int c) const {
        const int w = c >> 5;
        return wpre[w] + __popc(bm[w] & ((1u << (c & 31)) - 1u));
    }
};

// Stage emission rows [r0, r0+nrows) of a segment into LDS buffer `dst` (row stride VS
// floats).  Every wave of the workgroup issues its share.  When V == VS == 32 and the
// rows are 16-byte aligned (`x4`), a chunk is one contiguous 4 KB block in both places:
// one 16-byte-per-lane instruction moves 8 rows.  VS == kGatherVS: per row, lane l of pass
// i gathers column cols[64i + l] (the LDS-DMA source address is per lane, the destination
// lane-linear).  Otherwise one dword per lane per row, lanes >= V masked.  Asynchronous:
// every wave waits vmcnt(0) before the chunk barrier.
template <int VS, int W, bool ONE_WAVE = false>
__device__ __forceinline__ void stage_rows(const float* __restrict__ E, int V, int r0, int nrows, float* dst,
                                           bool x4, const ColMap& cm) {
    const int wv = ONE_WAVE ? 0 : uniform((int)threadIdx.x >> 6);
    const int l = lane_id();
    const unsigned base = (unsigned)uniform((int)lds_addr(dst));
    if (VS == kGatherVS) {
        const int passes = (cm.n + kWave - 1) / kWave;
        for (int i = 0; i < passes; ++i) {
            const int c = i * kWave + l;
            if (c < cm.n) {
                const unsigned off = (unsigned)cm.cols[c] * 4u;
                for (int r = wv; r < nrows; r += W)
                    glds_dword(E + (int64_t)(r0 + r) * V, off, base + (unsigned)(r * VS * 4 + i * kWave * 4));
            }
        }
    } else if (VS == 32 && x4) {
        for (int i = wv; i * 8 < nrows; i += W) {
            if (i * 8 + (l >> 3) < nrows)
                glds_dwordx4(E + (int64_t)(r0 + i * 8) * 32, (unsigned)l * 16u, base + (unsigned)(i * 1024));
        }
    } else if (l < V) {
        for (int r = wv; r < nrows; r += W)
            glds_dword(E + (int64_t)(r0 + r) * V, (unsigned)l * 4u, base + (unsigned)(r * VS * 4));
    }
}

// The column map of one segment (all threads of the workgroup): columns 0 and `blank` and
// every token id (ids outside [0, V) count as 0, as the DP reads them).  Returns the compact
// width, uniform; > kGatherVS means the segment cannot be staged.
__device__ int build_colmap(const int32_t* __restrict__ tok, int N, int blank, int V, unsigned* bm, int* wpre,
                            int* cols) {
    const int nw = (V + 31) >> 5;
    for (int w = (int)threadIdx.x; w < nw; w += (int)blockDim.x) bm[w] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int b = (blank >= 0 && blank < V) ? blank : 0;
        atomicOr(&bm[0], 1u);
        atomicOr(&bm[b >> 5], 1u << (b & 31));
    }
    for (int j = (int)threadIdx.x; j < N; j += (int)blockDim.x) {
        int t = tok[j];
        t = (t >= 0 && t < V) ? t : 0;
        atomicOr(&bm[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
    if (threadIdx.x < kWave) {  // exclusive prefix of popcounts, 64 words per pass
        int base = 0;
        for (int w0 = 0; w0 < nw; w0 += kWave) {
            const int w = w0 + (int)threadIdx.x;
            const int c = w < nw ? __popc(bm[w]) : 0;
            int incl = c;
#pragma unroll
            for (int off = 1; off < kWave; off <<= 1) {
                const int y = __shfl_up(incl, off);
                if ((int)threadIdx.x >= off) incl += y;
            }
            if (w < nw) wpre[w] = base + incl - c;
            base += __shfl(incl, kWave - 1);
        }
        if (threadIdx.x == 0) wpre[nw] = base;
    }
    __syncthreads();
    const int n = wpre[nw];
    if (n <= kGatherVS) {
        for (int w = (int)threadIdx.x; w < nw; w += (int)blockDim.x) {
            unsigned m = bm[w];
            int k = wpre[w];
            while (m) {
                cols[k++] = w * 32 + __ffs((int)m) - 1;
                m &= m - 1u;
            }
        }
    }
    __syncthreads();
    return uniform(n);
}

__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// Order one wave's own global/LDS writes before its later reads by other lanes (no
// barrier: safe inside wave-divergent regions of multi-wave workgroups).
__device__ __forceinline__ void wave_fence() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ void block_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Column-0 value tr[t][0]: 0 / fp32(cumsum) / +inf in the last N rows (alignment.py:367-370).
__device__ __forceinline__ float col0_value(int t, double acc, int T, int N) {
    const bool inf_row = (N == 0) || (t >= T + 1 - N);
    if (inf_row) return INFINITY;
    return t == 0 ? 0.0f : (float)acc;
}

__device__ __forceinline__ void granule_store(uint64_t* g, float v, unsigned tag) {
    const uint64_t x = ((uint64_t)tag << 32) | (uint64_t)__builtin_bit_cast(unsigned, v);
    __hip_atomic_store(g, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_store_dwordx2 sc1
}
__device__ __forceinline__ uint64_t granule_load(const uint64_t* g) {
    return __hip_atomic_load(const_cast<uint64_t*>(g), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Split segments publish their decision words and column-N history write-through (WT: sc1
// stores, which leave the XCD's L2 at once) and the last part to arrive reads them with sc1
// loads, L1-bypassing: the arrival then needs neither the release fence (buffer_wbl2: the
// write-back of every dirty line of the XCD's L2, ~2-6 us behind a part's freshly written
// bits) nor the acquire (MI355X_MICROARCH.md, "Valid forms": one lane per storing workgroup
// adds to one counter after every storing wave's vmcnt(0) wait and a workgroup barrier, the
// workgroup whose add came last loads after it returned, its other waves after a barrier;
// 4- and 16-byte sc1 stores and loads).  That table is measured behaviour on gfx950 / ROCm
// 7.2 (the guide's hand-off table, row 1), not an architectural guarantee, so the launch flag
// kArgFenced (WX_SPLIT_FENCED=1) adds the agent-scope release and acquire on top of the
// write-through stores — the memory model's own protocol — and the parity tests compare the
// two bit for bit with the parts of every segment spread over different XCDs (kArgXcdSpread).
constexpr bool kSplitWT = true;
// Register-resident split kernels only (C = 1, config 2): in the C > 1 split kernels the
// consumer's hand-off waits drain vmcnt inside the chain, and write-through stores take longer
// to drain (A/B, 64 x T = 2999, N ~ 900: fenced 166 us, write-through 178 us).
template <int C, int VS, bool SP>
constexpr bool split_wt() {
    return SP && kSplitWT && C == 1 && VS != kGatherVS;
}
template <bool WT, class T>
__device__ __forceinline__ T ld_pub(const T* p) {
    if constexpr (WT)
        return __hip_atomic_load(const_cast<T*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_load_dword sc1
    else
        return *p;
}
template <bool WT, class T>
__device__ __forceinline__ void st_pub(T* p, T v) {
    if constexpr (WT)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_store_dword sc1
    else
        *p = v;
}
// 16 bytes at base[i .. i + 3] (base wave-uniform).  WT: a buffer store with the sc1 bit (aux
// 16), through the builtin so that the compiler keeps its hazard and vmcnt bookkeeping (an asm
// dwordx4 store's data registers could be overwritten in the next instruction).
template <bool WT>
__device__ __forceinline__ void st_pub4(float* base, int i, float4 v) {
    if constexpr (WT) {
        typedef unsigned u4 __attribute__((ext_vector_type(4)));
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7fffffff, 0x00020000);
        const u4 x = {__builtin_bit_cast(unsigned, v.x), __builtin_bit_cast(unsigned, v.y),
                      __builtin_bit_cast(unsigned, v.z), __builtin_bit_cast(unsigned, v.w)};
        __builtin_amdgcn_raw_buffer_store_b128(x, r, i * 4, 0, 16);
    } else {
        *reinterpret_cast<float4*>(base + i) = v;
    }
}

}  // namespace wx

#endif  // WX_DP_PRIMS_H
